"""CPU: the C ABI of the multi-exponentiation (include/eg_hip_prodpow.h): the header declares
exactly the three entry points, native.EXPORTED_PRODPOW lists them and nothing another list holds,
the built library exports them, a null context and every limit are refused as argument errors
naming prod_pow before anything is touched, and the plan keeps the bounds of the cost model."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_prodpow.h"

THREE = ["eg_prod_pow", "eg_prod_pow_dev", "eg_prod_pow_plan"]
EG_ERR_ARG = 1
# every refusal below comes before the context is read: a pointer that is merely not NULL stands in
CTX = ctypes.c_void_p(0x1000)
BUF = ctypes.c_void_p(0x2000)


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
    return rc == EG_ERR_ARG and b"prod_pow" in lib.eg_last_error()


def test_header_declares_exactly_the_three_entry_points():
    assert header_functions() == THREE
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    for word in ("EG_PRODPOW_AUTO 0", "EG_PRODPOW_INTERLEAVED 1", "EG_PRODPOW_BUCKETS 2", "VARIABLE TIME",
                 "eg_ctx_set_ct_pow", "eg_powp_batch", "2 GiB", "NOT reduced mod q", "UPPER BOUND"):
        assert word in text, word


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_PRODPOW) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES) | \
        set(native.EXPORTED_CONTEST_DATA) | set(native.EXPORTED_RANGE) | set(native.EXPORTED_PREENCRYPT) | \
        set(native.EXPORTED_BALLOT2) | set(native.EXPORTED_CODES2)
    assert not set(native.EXPORTED_PRODPOW) & others
    for name in THREE:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == (7 if name.endswith("plan") else 10), name


def test_the_build_names_the_header_and_the_include():
    assert '"eg_hip_prodpow.h"' in (ROOT / "__graft_entry__.py").read_text()
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert '#include "eg_capi_prodpow.inc"' in capi and '#include "eg_prodpow.hpp"' in capi
    assert re.search(r"W_C2_KR,\s*(//[^\n]*\n\s*)*W_PP_", capi), "the new workspace slots follow W_C2_KR"


@pytest.mark.parametrize("name", THREE[:2])
def test_null_arguments_are_argument_errors(lib, name):
    fn = getattr(lib, name)
    assert refused(lib, fn(None, BUF, 1, 1, BUF, 1, 1, 0, 0, BUF))
    assert b"null" in lib.eg_last_error()
    assert refused(lib, fn(CTX, None, 1, 1, BUF, 1, 1, 0, 0, BUF))      # bases
    assert refused(lib, fn(CTX, BUF, 1, 1, None, 1, 1, 0, 0, BUF))      # exps
    assert refused(lib, fn(CTX, BUF, 1, 1, BUF, 1, 1, 0, 0, None))      # out
    assert refused(lib, fn(CTX, None, 1, 1, None, 1, 0, 0, 0, None))    # n == 0 frees bases and exps, not out


@pytest.mark.parametrize("name", THREE[:2])
def test_every_limit_is_refused(lib, name):
    fn = getattr(lib, name)
    call = lambda rs, ts, rows, n, method=0, w=0: fn(CTX, BUF, rs, ts, BUF, rows, n, method, w, BUF)
    assert refused(lib, call(1, 1, 1, (1 << 20) + 1))
    assert refused(lib, call(1, 1, (1 << 16) + 1, 1))
    assert refused(lib, call(1, 1, 1 << 16, (1 << 8) + 1))             # rows * n > 2^24
    assert refused(lib, call(0, 1, 2, 3)) and b"stride" in lib.eg_last_error()
    assert refused(lib, call(3, 0, 2, 3)) and b"stride" in lib.eg_last_error()
    for method, w in ((3, 0), (-1, 0), (1, 6), (2, 14), (0, 14), (1, -1), (2, -1)):
        assert refused(lib, call(3, 1, 2, 3, method, w)), (method, w)


def test_a_misaligned_device_pointer_is_refused(lib):
    odd = ctypes.c_void_p(0x2008)
    for args in ((odd, BUF, BUF), (BUF, odd, BUF), (BUF, BUF, odd)):
        assert refused(lib, lib.eg_prod_pow_dev(CTX, args[0], 1, 1, args[1], 1, 1, 0, 0, args[2]))
        assert b"aligned" in lib.eg_last_error()


def test_the_plan_refuses_what_the_call_refuses(lib):
    from electionguard import prodpow as pp
    from electionguard.core.native import EgError
    for args in ((1, (1 << 20) + 1), ((1 << 16) + 1, 1), (1 << 16, 257), (1, 5, 3), (1, 5, 1, 6), (1, 5, 2, 14),
                 (1, 5, 0, 14)):
        with pytest.raises(EgError, match="prod_pow") as e:
            pp.plan(*args)
        assert e.value.code == EG_ERR_ARG
    assert lib.eg_prod_pow_plan(1, 5, 0, 0, None, None, None) == 0     # every out pointer is optional


def test_plan_bounds_of_the_cost_model(lib):
    from electionguard import prodpow as pp
    assert pp.plan(1, 3).mont_ops <= 600
    assert pp.plan(1, 5).mont_ops <= 800
    assert pp.plan(1, 1 << 14).mont_ops <= 40 * (1 << 14)
    assert pp.plan(1, 1 << 20).mont_ops <= 32 * (1 << 20)
    for n in (0, 1, 3, 5, 159, 4096, 1 << 14, 1 << 20):
        one = pp.plan(1, n)
        for rows in (0, 2, 7, 16):
            if rows * n <= 1 << 24:
                many = pp.plan(rows, n)
                assert many[:2] == one[:2] and many.mont_ops == rows * one.mont_ops, (rows, n)
    assert pp.plan(1, 0).mont_ops == 0
    assert pp.plan(1, 3).method == pp.INTERLEAVED and pp.plan(1, 5).method == pp.INTERLEAVED
    assert pp.plan(2, 4096).method == pp.BUCKETS and pp.plan(8, 1 << 18).method == pp.BUCKETS
    # auto is the smaller of the two forced plans, and they cross between 100 and 250 terms
    for n in (5, 100, 250, 4096):
        a, i, b = pp.plan(1, n), pp.plan(1, n, pp.INTERLEAVED), pp.plan(1, n, pp.BUCKETS)
        assert a.mont_ops == min(i.mont_ops, b.mont_ops)
    assert pp.plan(1, 100).method == pp.INTERLEAVED and pp.plan(1, 250).method == pp.BUCKETS
    # a forced width is the width that runs
    assert pp.plan(1, 7, pp.BUCKETS, 4)[:2] == (pp.BUCKETS, 4)
    assert pp.plan(1, 7, pp.INTERLEAVED, 1)[:2] == (pp.INTERLEAVED, 1)
    assert pp.plan(1, 7, pp.AUTO, 9)[:2] == (pp.BUCKETS, 9)
