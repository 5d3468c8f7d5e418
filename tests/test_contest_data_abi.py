"""CPU: the C ABI of contest data (include/eg_hip_contestdata.h): the header declares exactly the
six entry points, native.EXPORTED_CONTEST_DATA lists them and nothing another list holds, the built
library exports them, and each rejects a null context without touching a device."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_contestdata.h"

SIX = ["eg_derive_contest_data_nonces", "eg_derive_contest_data_nonces_dev", "eg_open_contest_data",
       "eg_open_contest_data_dev", "eg_seal_contest_data", "eg_seal_contest_data_dev"]


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_six_entry_points():
    assert header_functions() == SIX
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    assert re.search(r"#define\s+EG_CD_MAX_BYTES\s+1024\b", text)
    assert "eg_ctx_set_ct_pow" in text   # the header says which switch the exponentiations follow


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_CONTEST_DATA) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES)
    assert not set(native.EXPORTED_CONTEST_DATA) & others
    for name in SIX:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name


def test_null_ctx_is_an_argument_error(lib):
    for name in ("eg_derive_contest_data_nonces", "eg_derive_contest_data_nonces_dev"):
        assert getattr(lib, name)(None, 0, 2, None, None) == 1, name
        assert b"null" in lib.eg_last_error()
    K = bytes(512)
    for name in ("eg_seal_contest_data", "eg_seal_contest_data_dev"):
        assert getattr(lib, name)(None, K, 0, 2, 32, None, None, None, None, None, None) == 1, name
        assert b"null" in lib.eg_last_error()
    for name in ("eg_open_contest_data", "eg_open_contest_data_dev"):
        assert getattr(lib, name)(None, 0, 2, 32, None, None, None, None, None, None, None) == 1, name
        assert b"null" in lib.eg_last_error()


def test_the_source_list_of_the_build_names_the_header():
    src = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_contestdata.h"' in src
    assert '#include "eg_capi_contestdata.inc"' in (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
