"""CPU: the C ABI of the device-side decode (include/eg_hip_decode.h): the header declares exactly
the seven entry points, native.EXPORTED_DECODE lists them and nothing another list holds, the built
library exports them, every refusal is an argument error naming decode made before the context or
the table is read (a pointer that is merely not NULL stands in for both), and n == 0 is EG_OK."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_decode.h"

SEVEN = sorted(["eg_batch_inverse", "eg_batch_inverse_dev", "eg_decode_table_create", "eg_decode_table_destroy",
                "eg_decode_counts", "eg_decode_counts_dev", "eg_decode_plan"])
EG_OK, EG_ERR_ARG = 0, 1
CTX = ctypes.c_void_p(0x1000)   # never read: every call below is refused, or returns, before it would be
TAB = ctypes.c_void_p(0x3000)
BUF = ctypes.c_void_p(0x2000)
ODD = ctypes.c_void_p(0x2008)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def refused(lib, rc):
    return rc == EG_ERR_ARG and b"decode" in lib.eg_last_error()


def test_header_declares_exactly_the_entry_points():
    assert header_functions() == SEVEN
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    for word in ("EG_DECODE_MAX_TEXTS ((size_t)1 << 24)", "EG_DECODE_MAX_COUNT ((uint64_t)1 << 32)",
                 "EG_DECODE_STOP 16", "VARIABLE", "eg_ctx_set_ct_pow", "eg_multinv_batch", "UPPER BOUND",
                 "CANONICAL", "Not counted", "ONLY so that tests"):
        assert word in text, word


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_DECODE) == header_functions()
    others = set()
    for name in dir(native):
        if name.startswith("EXPORTED") and name != "EXPORTED_DECODE":
            others |= set(getattr(native, name))
    assert len(others) > 90 and not set(native.EXPORTED_DECODE) & others
    nargs = {"eg_batch_inverse": 4, "eg_batch_inverse_dev": 4, "eg_decode_table_create": 4,
             "eg_decode_table_destroy": 1, "eg_decode_counts": 5, "eg_decode_counts_dev": 5, "eg_decode_plan": 10}
    for name in SEVEN:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == nargs[name], name


def test_the_build_names_the_header_and_the_include():
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_decode.h"' in entry and "eg_capi_decode.inc" in entry
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert '#include "eg_decode.hpp"' in capi
    assert re.search(r'#include "eg_capi_shuffle.inc"\s*#include "eg_capi_decode.inc"', capi)
    assert re.search(r"W_SH_W,\s*(//[^\n]*\n\s*)*W_DC_", capi), "the new workspace slots follow W_SH_W"


@pytest.mark.parametrize("name", ["eg_batch_inverse", "eg_batch_inverse_dev"])
def test_batch_inverse_refusals_and_nothing_to_do(lib, name):
    fn = getattr(lib, name)
    assert refused(lib, fn(None, BUF, BUF, 1)) and b"null" in lib.eg_last_error()
    assert refused(lib, fn(CTX, None, BUF, 1))
    assert refused(lib, fn(CTX, BUF, None, 1))
    assert refused(lib, fn(CTX, BUF, BUF, (1 << 24) + 1)) and b"2^24" in lib.eg_last_error()
    assert fn(CTX, BUF, BUF, 0) == EG_OK
    assert fn(CTX, None, None, 0) == EG_OK
    assert refused(lib, fn(None, None, None, 0))            # a NULL context is refused whatever n


def test_misaligned_device_pointers_are_refused(lib):
    for a, out in ((ODD, BUF), (BUF, ODD)):
        assert refused(lib, lib.eg_batch_inverse_dev(CTX, a, out, 1)) and b"aligned" in lib.eg_last_error()
    for b, m, cnt in ((ODD, BUF, BUF), (BUF, ODD, BUF), (BUF, BUF, ODD), (ODD, None, BUF)):
        assert refused(lib, lib.eg_decode_counts_dev(TAB, b, m, 1, cnt)) and b"aligned" in lib.eg_last_error()
    # host pointers need no alignment: the same call is refused for nothing and would go on to read
    # the context, so only the device variants are asked


def test_table_create_refusals(lib):
    tab = ctypes.c_void_p(0x55)
    create = lib.eg_decode_table_create
    assert refused(lib, create(None, 100, 0, ctypes.byref(tab))) and b"null" in lib.eg_last_error()
    assert refused(lib, create(CTX, 100, 0, None)) and b"null" in lib.eg_last_error()
    assert refused(lib, create(CTX, (1 << 32) + 1, 0, ctypes.byref(tab))) and b"2^32" in lib.eg_last_error()
    for fp in (-1, 1, 7, 65, 128):
        assert refused(lib, create(CTX, 100, fp, ctypes.byref(tab))) and b"fp_bits" in lib.eg_last_error(), fp
    assert tab.value == 0x55                                # a refused call leaves the out pointer alone
    assert lib.eg_decode_table_destroy(None) == EG_OK


@pytest.mark.parametrize("name", ["eg_decode_counts", "eg_decode_counts_dev"])
def test_counts_refusals_and_nothing_to_do(lib, name):
    fn = getattr(lib, name)
    assert refused(lib, fn(None, BUF, BUF, 1, BUF)) and b"null table" in lib.eg_last_error()
    assert refused(lib, fn(TAB, None, BUF, 1, BUF))         # B
    assert refused(lib, fn(TAB, BUF, BUF, 1, None))         # counts
    assert refused(lib, fn(TAB, BUF, None, (1 << 24) + 1, BUF)) and b"2^24" in lib.eg_last_error()
    assert fn(TAB, BUF, None, 0, BUF) == EG_OK              # M may be NULL, and n == 0 touches nothing
    assert fn(TAB, None, None, 0, None) == EG_OK


def test_the_plan_refuses_what_the_calls_refuse(lib):
    from electionguard import decode as dc
    from electionguard.core.native import EgError
    for args in (((1 << 24) + 1, 0), (1, (1 << 32) + 1)):
        with pytest.raises(EgError, match="decode") as e:
            dc.plan(*args)
        assert e.value.code == EG_ERR_ARG
    assert lib.eg_decode_plan(5, 100, *([None] * 8)) == EG_OK  # every out pointer is optional
    assert dc.plan(1 << 24, 1 << 32).m == 65537
