"""CPU: the C ABI of the pre-encrypted ballots (include/eg_hip_preencrypt.h): the header declares
exactly the six entry points, the caps and the chunk constant, native.EXPORTED_PREENCRYPT lists
them and nothing another list holds, the built library exports them, each rejects a null context
without touching a device, and the build's source list names the header and the include."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_preencrypt.h"

SIX = ["eg_preencrypt_ballots", "eg_preencrypt_ballots_dev", "eg_preencrypt_record", "eg_preencrypt_record_dev",
       "eg_preencrypt_verify", "eg_preencrypt_verify_dev"]


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_six_entry_points_the_caps_and_the_chunk():
    assert header_functions() == SIX
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    assert re.search(r"#define\s+EG_PRE_MAX_SPC\s+64\b", text)
    assert re.search(r"#define\s+EG_PRE_CHUNK_CTS\s+\(1u << 18\)", text)
    assert "eg_ctx_set_ct_encrypt" in text   # the header says which switch the encryptions follow


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    from electionguard import preencrypt
    assert sorted(native.EXPORTED_PREENCRYPT) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES) | \
        set(native.EXPORTED_CONTEST_DATA) | set(native.EXPORTED_RANGE)
    assert not set(native.EXPORTED_PREENCRYPT) & others
    for name in SIX:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert preencrypt.MAX_SPC == 64 and preencrypt.CHUNK_CTS == 1 << 18


def test_null_ctx_is_an_argument_error(lib):
    K = bytes(512)
    spc = (ctypes.c_uint32 * 1)(2)
    for name in ("eg_preencrypt_ballots", "eg_preencrypt_ballots_dev"):
        assert getattr(lib, name)(None, K, 0, 1, spc, 2, *[None] * 11) == 1, name
        assert b"preencrypt" in lib.eg_last_error() and b"null" in lib.eg_last_error()
    for name in ("eg_preencrypt_record", "eg_preencrypt_record_dev"):
        assert getattr(lib, name)(None, K, 0, 1, spc, spc, 2, *[None] * 10) == 1, name
        assert b"preencrypt" in lib.eg_last_error() and b"null" in lib.eg_last_error()
    for name in ("eg_preencrypt_verify", "eg_preencrypt_verify_dev"):
        assert getattr(lib, name)(None, 0, 1, spc, spc, 2, *[None] * 11) == 1, name
        assert b"preencrypt" in lib.eg_last_error() and b"null" in lib.eg_last_error()


def test_the_source_list_of_the_build_names_the_header_and_the_include():
    src = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_preencrypt.h"' in src
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert '#include "eg_capi_preencrypt.inc"' in capi
    assert '#include "eg_preencrypt.hpp"' in capi
