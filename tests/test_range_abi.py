"""CPU: the C ABI of the 0..L range proofs (include/eg_hip_range.h): the header declares exactly
the four entry points and the cap, native.EXPORTED_RANGE lists them and nothing another list holds,
the built library exports them, each rejects a null context without touching a device, and the
build's source list names the header and the include."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_range.h"

FOUR = ["eg_range_prove", "eg_range_prove_dev", "eg_range_verify", "eg_range_verify_dev"]


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_four_entry_points_and_the_cap():
    assert header_functions() == FOUR
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    assert re.search(r"#define\s+EG_RANGE_MAX_LIMIT\s+15\b", text)
    assert "eg_ctx_set_ct_encrypt" in text   # the header says which switch the prover follows


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    from electionguard import range_proof
    assert sorted(native.EXPORTED_RANGE) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES) | \
        set(native.EXPORTED_CONTEST_DATA)
    assert not set(native.EXPORTED_RANGE) & others
    for name in FOUR:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert range_proof.MAX_LIMIT == 15


def test_null_ctx_is_an_argument_error(lib):
    K, qbar = bytes(512), bytes(32)
    for name in ("eg_range_prove", "eg_range_prove_dev"):
        assert getattr(lib, name)(None, K, qbar, 0, 1, None, None, None, None, None) == 1, name
        assert b"range" in lib.eg_last_error() and b"null" in lib.eg_last_error()
    for name in ("eg_range_verify", "eg_range_verify_dev"):
        assert getattr(lib, name)(None, K, qbar, 0, 1, None, None, None) == 1, name
        assert b"range" in lib.eg_last_error() and b"null" in lib.eg_last_error()


def test_the_source_list_of_the_build_names_the_header_and_the_include():
    src = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_range.h"' in src
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert '#include "eg_capi_range.inc"' in capi
