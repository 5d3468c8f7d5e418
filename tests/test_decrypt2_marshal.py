"""The marshalling of electionguard.decrypt2's GPU wrappers, without the library or a GPU: the
recording stub of tests/test_marshal.py stands in for libeg_hip.so, and each call is compared,
argument by argument, with the prototype's parameter list read from include/eg_hip_decrypt2.h.
The three pairs in both modes, the two trustee calls on the host; the column sizes and the limits
are checked before anything is allocated or called."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_marshal import StubGroup, addr

from electionguard import decrypt2 as D
from electionguard.core.group import DeviceBuffer

HEADER = Path(__file__).resolve().parent.parent / "include" / "eg_hip_decrypt2.h"
U8 = np.uint8
MODES = [False, True]
IDS = ["host", "device"]
N, K_G, QBAR, KEY = 5, 3, 0x1234567, 0xABCDEF


def prototype(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?$", p.strip()).group(1) for p in params.split(",")]
    return [p[2:] if p.startswith("d_") else p for p in names]


def make(g, shape, device, seed=1):
    a = np.random.default_rng(seed).integers(0, 256, shape, U8)
    return g.to_device(a) if device else a


def the_call(g, name, device):
    (called, args), = g._lib.calls
    assert called == name + ("_dev" if device else "")
    names = prototype(called)
    assert names == prototype(name) and len(args) == len(names)
    got = dict(zip(names, args))
    assert addr(got["ctx"]) == 0xC0DE
    return got


def same(got, given):
    return addr(got) == addr(given)                      # passed through, not copied


def is_out(got, value, device, shape, dtype=U8):
    assert isinstance(value, DeviceBuffer) == device and tuple(value.shape) == shape, (value.shape, shape)
    if device:
        return addr(got) == value.ptr
    return value.dtype == dtype                          # a bool flag array is a converted copy


def bytes_at(p, n):
    import ctypes
    return ctypes.string_at(addr(p), n)


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_combine(device):
    g = StubGroup()
    texts, shares, comm = make(g, (N, 2, 512), device), make(g, (N, K_G, 512), device), make(g, (N, K_G, 2, 512), device)
    w = [1, 2**256 - 1, 7]
    M, c, ci = D.combine(g, KEY, QBAR, w, texts, shares, comm)
    got = the_call(g, "eg_decrypt2_combine", device)
    assert (got["n"], got["k"]) == (N, K_G)
    assert bytes_at(got["K_be"], 512) == KEY.to_bytes(512, "big") and bytes_at(got["qbar_be"], 32) == QBAR.to_bytes(32, "big")
    assert bytes_at(got["weights"], 96) == b"".join(x.to_bytes(32, "big") for x in w)   # a host pointer in both modes
    assert same(got["texts"], texts) and same(got["shares"], shares) and same(got["comm"], comm)
    assert is_out(got["out_M"], M, device, (N, 512)) and is_out(got["out_c"], c, device, (N, 32))
    assert is_out(got["out_ci"], ci, device, (N, K_G, 32))


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_check(device):
    g = StubGroup()
    texts, shares, comm = make(g, (N, 2, 512), device), make(g, (N, K_G, 512), device), make(g, (N, K_G, 2, 512), device)
    ci, vi = make(g, (N, K_G, 32), device, 2), make(g, (N, K_G, 32), device, 3)
    Z = [3, 5, 2**4096 - 1]
    ok, v = D.check(g, Z, texts, shares, comm, ci, vi)
    got = the_call(g, "eg_decrypt2_check", device)
    assert (got["n"], got["k"]) == (N, K_G)
    assert bytes_at(got["Z"], 3 * 512) == b"".join(z.to_bytes(512, "big") for z in Z)
    for name, given in (("texts", texts), ("shares", shares), ("comm", comm), ("ci", ci), ("vi", vi)):
        assert same(got[name], given), name
    assert is_out(got["ok"], ok, device, (N, K_G), bool) and is_out(got["out_v"], v, device, (N, 32))


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_verify(device):
    g = StubGroup()
    texts, M, proofs = make(g, (N, 2, 512), device), make(g, (N, 512), device), make(g, (N, 2, 32), device)
    ok = D.verify(g, KEY, QBAR, texts, M, proofs)
    got = the_call(g, "eg_decrypt2_verify", device)
    assert got["n"] == N
    assert bytes_at(got["K_be"], 512) == KEY.to_bytes(512, "big") and bytes_at(got["qbar_be"], 32) == QBAR.to_bytes(32, "big")
    assert same(got["texts"], texts) and same(got["M"], M) and same(got["proofs"], proofs)
    assert is_out(got["ok"], ok, device, (N,), bool)


def test_commit_and_respond_are_host_calls():
    g = StubGroup()
    pads, nonces = make(g, (N, 512), False), make(g, (N, 32), False, 2)
    M, a, b = D.commit(g, 77, pads, nonces)
    got = the_call(g, "eg_decrypt2_commit", False)
    assert got["n"] == N and bytes_at(got["secret_be"], 32) == (77).to_bytes(32, "big")
    assert same(got["pads"], pads) and same(got["nonces"], nonces)
    for name, out in (("out_M", M), ("out_a", a), ("out_b", b)):
        assert same(got[name], out) and out.shape == (N, 512) and out.dtype == U8
    g = StubGroup()
    chal = make(g, (N, 32), False, 3)
    v = D.respond(g, 77, nonces, chal)
    got = the_call(g, "eg_decrypt2_respond", False)
    assert got["n"] == N and bytes_at(got["secret_be"], 32) == (77).to_bytes(32, "big")
    assert same(got["nonces"], nonces) and same(got["challenges"], chal) and same(got["out_v"], v)
    assert v.shape == (N, 32)
    g = StubGroup()
    D.respond(g, 1, [0, 2**256 - 1], [5, 6])              # ints become 32 big-endian bytes each
    got = the_call(g, "eg_decrypt2_respond", False)
    assert bytes_at(got["nonces"], 64) == bytes(32) + b"\xff" * 32 and got["n"] == 2


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_what_does_not_fit_is_refused_before_any_call(device):
    g = StubGroup()
    texts, shares, comm = make(g, (N, 2, 512), device), make(g, (N, K_G, 512), device), make(g, (N, K_G, 2, 512), device)
    ci, vi = make(g, (N, K_G, 32), device), make(g, (N, K_G, 32), device)
    short = make(g, (N - 1, K_G, 512), device)
    other = np.zeros((N, K_G, 512), U8) if device else g.to_device(np.zeros((N, K_G, 512), U8))
    before = (g.allocs, len(g.uploads))
    w = [1, 2, 3]
    with pytest.raises(ValueError, match="shares"):
        D.combine(g, KEY, QBAR, w, texts, short, comm)
    with pytest.raises(ValueError, match="comm"):
        D.combine(g, KEY, QBAR, w, texts, shares, make(g, (N, K_G, 512), device))
    with pytest.raises(ValueError, match="shares"):        # two weights: rows of 2 x 512
        D.combine(g, KEY, QBAR, w[:2], texts, shares, comm)
    with pytest.raises(TypeError):
        D.combine(g, KEY, QBAR, w, texts, other, comm)
    with pytest.raises(ValueError, match="vi"):
        D.check(g, [1, 2, 3], texts, shares, comm, ci, make(g, (N, K_G, 31), device))
    with pytest.raises(ValueError, match="ci"):
        D.check(g, [1, 2, 3], texts, shares, comm, make(g, (N, 2, 32), device), vi)
    with pytest.raises(ValueError, match="M"):
        D.verify(g, KEY, QBAR, texts, make(g, (N + 1, 512), device), make(g, (N, 2, 32), device))
    with pytest.raises(ValueError, match="proofs"):
        D.verify(g, KEY, QBAR, texts, make(g, (N, 512), device), make(g, (N, 32), device))
    with pytest.raises(ValueError, match="guardians"):
        D.combine(g, KEY, QBAR, list(range(65)), texts, make(g, (N, 65, 512), device), make(g, (N, 65, 2, 512), device))
    assert g._lib.calls == []
    if not device:
        assert (g.allocs, len(g.uploads)) == before


def test_the_limits_are_checked_on_the_shape_alone():
    g = StubGroup()
    n = (1 << 24) // 64 + 1
    with pytest.raises(ValueError, match="2\\^24"):
        D.check(g, [1] * 64, g.device_empty((n, 2, 512)), g.device_empty((n, 64, 512)), g.device_empty((n, 64, 2, 512)),
                g.device_empty((n, 64, 32)), g.device_empty((n, 64, 32)))
    with pytest.raises(ValueError, match="nonces"):
        D.commit(g, 1, np.zeros((3, 512), U8), np.zeros((2, 32), U8))
    with pytest.raises(ValueError, match="challenges"):
        D.respond(g, 1, np.zeros((3, 32), U8), np.zeros((2, 32), U8))
    assert g._lib.calls == []
