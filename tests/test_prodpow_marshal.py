"""The marshalling of electionguard.prodpow's GPU wrappers, without the library or a GPU: the
recording stub of tests/test_marshal.py stands in for libeg_hip.so, and each call is compared,
argument by argument, with the prototype's parameter list read from include/eg_hip_prodpow.h.
Both layouts, a padded stride, host and device; the strided extent and the limits are checked
before anything is allocated or called."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_marshal import StubGroup, addr

from electionguard import prodpow as pp
from electionguard.core.group import DeviceBuffer

HEADER = Path(__file__).resolve().parent.parent / "include" / "eg_hip_prodpow.h"
U8 = np.uint8
MODES = [False, True]
IDS = ["host", "device"]


def prototype(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in params.split(",")]
    return [p[2:] if p.startswith("d_") else p for p in names]


def make(g, shape, device):
    a = np.random.default_rng(1).integers(0, 256, shape, U8)
    return g.to_device(a) if device else a


def check(g, device, bases, exps, out, rows, n, rs, ts, method=0, w=0):
    (called, args), = g._lib.calls
    assert called == "eg_prod_pow" + ("_dev" if device else "")
    names = prototype(called)
    assert names == prototype("eg_prod_pow") and len(args) == len(names)
    got = dict(zip(names, args))
    assert addr(got["ctx"]) == 0xC0DE
    assert addr(got["bases_be"]) == addr(bases) and addr(got["exps_be"]) == addr(exps)   # passed through, not copied
    assert (got["row_stride"], got["term_stride"], got["rows"], got["n"]) == (rs, ts, rows, n)
    assert (got["method"], got["window_bits"]) == (method, w)
    assert isinstance(out, DeviceBuffer) == device and tuple(out.shape) == (rows, 512)
    if device:
        assert addr(got["out_be"]) == out.ptr
    else:
        assert addr(got["out_be"]) == out.ctypes.data and out.dtype == U8


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_rows_layout_with_a_padded_stride(device):
    g = StubGroup()
    bases, exps = make(g, (3, 7, 512), device), make(g, (5, 32), device)
    out = pp.prod_pow(g, bases, exps, layout="rows", method=pp.BUCKETS, window_bits=4)
    check(g, device, bases, exps, out, rows=3, n=5, rs=7, ts=1, method=2, w=4)


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_terms_layout(device):
    g = StubGroup()
    bases, exps = make(g, (9, 4, 512), device), make(g, (9, 32), device)
    out = pp.prod_pow(g, bases, exps, layout="terms")
    check(g, device, bases, exps, out, rows=4, n=9, rs=1, ts=4)


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_lagrange_combine_is_one_call_in_the_rows_layout(device):
    g = StubGroup()
    shares, w = make(g, (6, 3, 512), device), make(g, (3, 32), device)
    out = pp.lagrange_combine(g, shares, w)
    check(g, device, shares, w, out, rows=6, n=3, rs=3, ts=1)


def test_host_exponents_may_be_ints():
    g = StubGroup()
    out = pp.prod_pow(g, np.zeros((2, 3, 512), U8), [1, 2**256 - 1, 0])
    (_, args), = g._lib.calls
    assert args[6] == 3 and out.shape == (2, 512)
    rows = pp._exps_array([1, 2**256 - 1, 0])          # what the call was handed: 32 big-endian bytes each
    assert rows.shape == (3, 32) and rows.tobytes() == (1).to_bytes(32, "big") + b"\xff" * 32 + bytes(32)


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_what_does_not_fit_is_refused_before_any_call(device):
    g = StubGroup()
    bases, exps = make(g, (3, 4, 512), device), make(g, (5, 32), device)
    other = np.zeros((4, 32), U8) if device else g.to_device(np.zeros((4, 32), U8))
    before = (g.allocs, len(g.uploads))
    with pytest.raises(ValueError, match="bases"):         # 5 terms in rows of 4
        pp.prod_pow(g, bases, exps, layout="rows")
    with pytest.raises(ValueError, match="bases"):         # 5 terms, 3 given
        pp.prod_pow(g, bases, exps, layout="terms")
    with pytest.raises(ValueError, match="layout"):
        pp.prod_pow(g, bases, exps[:4] if not device else make(g, (4, 32), True), layout="columns")
    with pytest.raises(ValueError, match="bases"):         # not (., ., 512)
        pp.prod_pow(g, make(g, (12, 512), device), make(g, (4, 32), device))
    with pytest.raises(ValueError, match="exps"):          # no whole number of 32-byte rows
        pp.prod_pow(g, bases, make(g, (33,), device))
    with pytest.raises(TypeError):
        pp.prod_pow(g, bases, other)
    with pytest.raises(ValueError, match="out"):
        pp.prod_pow(g, bases, make(g, (4, 32), device), out=make(g, (2, 512), device))
    assert g._lib.calls == []
    if not device:
        assert (g.allocs, len(g.uploads)) == before


def test_the_limits_are_checked_on_the_shape_alone():
    g = StubGroup()
    big = g.device_empty(((1 << 16) + 1, 1, 512))
    with pytest.raises(ValueError, match="2\\^16 rows"):
        pp.prod_pow(g, big, g.device_empty((1, 32)))
    assert g._lib.calls == []
