"""CPU: the C ABI of ballot nonces, ballot hashes and the code chain (include/eg_hip_codes.h):
the header declares exactly the six entry points, native.EXPORTED_CODES lists them, the built
library exports them, and each rejects a null context without touching a device."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

SIX = ["eg_ballot_hashes", "eg_ballot_hashes_dev", "eg_derive_ballot_nonces", "eg_derive_ballot_nonces_dev",
       "eg_verify_code_chain", "eg_verify_code_chain_dev"]


def header_functions():
    src = (ROOT / "include" / "eg_hip_codes.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_six_entry_points():
    assert header_functions() == SIX
    assert '#include "eg_hip.h"' in (ROOT / "include" / "eg_hip_codes.h").read_text()


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_CODES) == header_functions()
    assert not set(native.EXPORTED_CODES) & (set(native.EXPORTED) | set(native.EXPORTED_MANIFEST))
    for name in SIX:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name


def test_null_ctx_is_an_argument_error(lib):
    shape = np.array([3, 2], np.uint32)
    spc = shape.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    for name in ("eg_derive_ballot_nonces", "eg_derive_ballot_nonces_dev"):
        assert getattr(lib, name)(None, 0, 2, spc, None, None, None) == 1, name
        assert b"null" in lib.eg_last_error()
    for name in ("eg_ballot_hashes", "eg_ballot_hashes_dev"):
        assert getattr(lib, name)(None, 0, 2, spc, None, None, None, None, None, None, None, None) == 1, name
        assert b"null" in lib.eg_last_error()
    for name in ("eg_verify_code_chain", "eg_verify_code_chain_dev"):
        assert getattr(lib, name)(None, 0, None, None, None, None, None) == 1, name
        assert b"null" in lib.eg_last_error()


def test_the_source_list_of_the_build_names_the_header():
    src = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_codes.h"' in src
