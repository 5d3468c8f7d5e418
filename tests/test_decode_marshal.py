"""CPU: the plan of the device-side decode against the formula restated in tests/decode_ref.py and
the 5 n bound of the inversion; the restated algorithms on a 64-bit toy Schnorr group (segmented
inverse with its multiply count, baby-step giant-step with 64-bit and 8-bit fingerprints); the
package's host mirrors; and the marshalling of electionguard.decode's wrappers against the
prototypes read from include/eg_hip_decode.h, with the recording stub of tests/test_marshal.py."""
import random
import re
from pathlib import Path

import numpy as np
import pytest

import decode_ref as R
from test_marshal import StubGroup, addr

from electionguard import decode as dc
from electionguard.core.group import DeviceBuffer

HEADER = Path(__file__).resolve().parent.parent / "include" / "eg_hip_decode.h"
U8 = np.uint8
MODES = [False, True]
IDS = ["host", "device"]


# ---- the plan ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_plan_values_equal_the_restated_formula(lib):
    ns = [0, 1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257, 1000, 4096, 4097, 10000, 65535, 65536, 65537,
          70000, 1 << 20, 1310720, 1 << 24]
    for n in ns:
        for max_count in (0, 1, 3, 100, 1_000_000, (1 << 32) - 1, 1 << 32):
            assert tuple(dc.plan(n, max_count)) == R.plan(n, max_count), (n, max_count)
    assert dc.plan(5, 1_000_000)[3:6] == (1001, 2048, 1001 / 2048)
    assert dc.plan(5, 0).m == 1 and dc.plan(5, 3).m == 2 and dc.plan(5, 4).m == 3
    assert dc.plan(5, 0).slots == 16


def test_levels_and_segments_of_the_inversion(lib):
    assert [dc.plan(n).seg_len for n in (1, 64, 65, 128, 129, 1 << 24)] == [4, 4, 8, 8, 16, 16]
    assert [dc.plan(n)[:3] for n in (16, 17, 256, 257, 4096, 4097)] == \
        [(4, 0, 16), (4, 1, 5), (16, 1, 16), (16, 2, 2), (16, 2, 16), (16, 3, 2)]
    for n in range(1, 3000):
        p = dc.plan(n)
        assert 1 <= p.pow_jobs <= dc.STOP and (p.levels == 0) == (n <= dc.STOP), n
        assert p.inv_ops == 3 * (n - p.pow_jobs) + 5129 * p.pow_jobs


def test_the_inversion_stays_under_five_multiplies_per_element(lib):
    assert dc.plan(65536).inv_ops <= 5 * 65536
    for n in (65537, 70000, 100000, 1 << 17, 1310720, (1 << 24) - 1, 1 << 24):
        p = dc.plan(n)
        assert p.inv_ops <= 5 * n and p.inv_ops <= 3 * n * (1 + 1 / (p.seg_len - 1)) + 5129 * p.pow_jobs, n


# ---- the restated algorithms on a toy group ----
@pytest.fixture(scope="module")
def toy():
    p, q, g = R.toy_group()
    assert R.is_prime(p) and R.is_prime(q) and (p - 1) % q == 0 and p.bit_length() == 64
    assert g != 1 and pow(g, q, p) == 1
    return p, q, g


@pytest.mark.parametrize("n", [1, 2, 7, 15, 16, 17, 63, 64, 65, 129, 256, 257, 1000, 4097])
def test_segmented_inverse_on_the_toy_group(toy, n):
    p, _, _ = toy
    rng = random.Random(n)
    a = [rng.randrange(1, p) for _ in range(n)]
    for i in {0, n - 1, n // 2, n // 3}:
        a[i] = rng.choice([0, p, 1, p - 1, p + 5])
    if n >= 129:
        a[32:48] = [0] * 16                                  # one all-zero segment
    cnt = R.Count()
    got = R.batch_inverse(p, a, cnt)
    assert got == dc.batch_inverse_host(p, a)
    s, levels, jobs = R.inv_plan(n)
    assert (cnt.levels, cnt.pow_jobs) == (levels, jobs)
    assert cnt.mul == 3 * (n - jobs)
    assert 3 * (n - jobs) + R.POW_OPS * jobs == R.plan(n)[6]


@pytest.mark.parametrize("max_count", [0, 1, 3, 100, 1_000_000])
@pytest.mark.parametrize("fp_bits", [0, 8])
def test_fingerprinted_baby_step_giant_step_on_the_toy_group(toy, max_count, fp_bits):
    p, q, g = toy
    tab = R.Table(p, g, max_count, fp_bits)
    m = tab.m
    ts = sorted({t for t in (0, 1, m - 1, m, m + 1, max_count // 2, max_count) if 0 <= t <= max_count})
    ys = [pow(g, t, p) for t in ts] + [pow(g, max_count + 1, p), pow(g, q - 1, p), 0, p - 1]
    want = ts + [-1] * 4
    assert tab.counts(ys) == want
    assert dc.counts_host(p, g, ys, max_count) == want
    rng = random.Random(max_count)
    M = [pow(g, rng.randrange(q), p) for _ in ys]
    M[1 % len(M)] = 0
    B = [y * v % p for y, v in zip(ys, M)]
    want_m = [-1 if v == 0 else t for t, v in zip(want, M)]
    assert tab.counts(B, M) == want_m
    if fp_bits == 8 and max_count == 1_000_000:
        # 1,001 baby steps in 256 fingerprints: comparisons fail, and every answer above was exact
        assert tab.false_hits > 0 and tab.compares > tab.false_hits


# ---- the wrappers ----
def prototype(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in params.split(",")]
    return [p[2:] if p.startswith("d_") else p for p in names]


def make(g, shape, device, seed=1):
    a = np.random.default_rng(seed).integers(0, 256, shape, U8)
    return g.to_device(a) if device else a


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_batch_inverse_marshals_one_call(device):
    g = StubGroup()
    a = make(g, (5, 512), device)
    out = dc.batch_inverse(g, a)
    (called, args), = g._lib.calls
    assert called == "eg_batch_inverse" + ("_dev" if device else "")
    names = prototype(called)
    assert names == prototype("eg_batch_inverse") and len(args) == len(names)
    got = dict(zip(names, args))
    assert addr(got["ctx"]) == 0xC0DE and addr(got["a_be"]) == addr(a) and got["n"] == 5
    assert isinstance(out, DeviceBuffer) == device and tuple(out.shape) == (5, 512)
    assert addr(got["out_be"]) == addr(out)


@pytest.mark.parametrize("with_m", [True, False], ids=["M", "no M"])
@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_table_and_counts_marshal(device, with_m):
    g = StubGroup()
    tab = dc.DecodeTable(g, 1_000_000, 8)
    (called, args), = g._lib.calls
    assert called == "eg_decode_table_create" and len(args) == len(prototype(called))
    assert addr(args[0]) == 0xC0DE and tuple(args[1:3]) == (1_000_000, 8)
    g._lib.calls.clear()
    tab._tab.value = 0x7AB
    B, M = make(g, (9, 512), device), make(g, (9, 512), device, 2) if with_m else None
    out = tab.counts(B, M)
    (called, args), = g._lib.calls
    assert called == "eg_decode_counts" + ("_dev" if device else "")
    names = prototype(called)
    assert names == prototype("eg_decode_counts") and len(args) == len(names)
    got = dict(zip(names, args))
    assert addr(got["tab"]) == 0x7AB                        # the table, not the context, leads the call
    assert addr(got["B_be"]) == addr(B) and addr(got["M_be"]) == addr(M) and got["n"] == 9
    assert isinstance(out, DeviceBuffer) == device and tuple(out.shape) == (9,) and out.dtype == np.int64
    assert addr(got["counts"]) == addr(out)
    tab.close()
    with pytest.raises(ValueError, match="closed"):
        tab.counts(B, M)


def test_wrong_shapes_and_mixed_kinds_are_refused_before_any_call():
    g = StubGroup()
    tab = dc.DecodeTable(g, 100)
    g._lib.calls.clear()
    with pytest.raises(ValueError, match="M"):
        tab.counts(make(g, (4, 512), False), make(g, (3, 512), False))
    with pytest.raises(TypeError, match="do not mix"):
        tab.counts(make(g, (4, 512), True), make(g, (4, 512), False))
    assert g._lib.calls == [] and g.allocs == 1              # the one device B above; no output was made


def test_decode_counts_keeps_one_table_per_max_count():
    g = StubGroup()
    B = make(g, (2, 512), False)
    dc.decode_counts(g, B, None, 100)
    dc.decode_counts(g, B, None, 100)
    dc.decode_counts(g, B, B, 3)
    names = [c[0] for c in g._lib.calls]
    assert names == ["eg_decode_table_create", "eg_decode_counts", "eg_decode_counts", "eg_decode_table_create",
                     "eg_decode_counts"]
    assert sorted(g._decode_tables) == [3, 100]
    dc.close_tables(g)
    assert "_decode_tables" not in g.__dict__


def test_decrypt_record_takes_a_decode_argument():
    import inspect
    from electionguard.decrypt2 import DECODES, Decryption2
    assert DECODES == ("host", "device")
    for name in ("decrypt_record", "decrypt", "decrypt_ballots_record", "decryptBallots"):
        assert inspect.signature(getattr(Decryption2, name)).parameters["decode"].default == "host", name
    d = Decryption2.__new__(Decryption2)
    with pytest.raises(ValueError, match="decode"):
        d.decrypt_record(np.zeros((0, 2, 512), U8), 3, decode="gpu")
