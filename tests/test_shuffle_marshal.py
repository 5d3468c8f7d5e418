"""The marshalling of electionguard.shuffle's GPU wrappers, without the library or a GPU: the
recording stub of tests/test_marshal.py stands in for libeg_hip.so, and each call is compared,
argument by argument, with the prototype's parameter list read from include/eg_hip_shuffle.h.  Host
and device; shapes and limits are checked before anything is allocated or called."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_marshal import StubGroup, addr

from electionguard import shuffle as S
from electionguard.core.group import DeviceBuffer

HEADER = Path(__file__).resolve().parent.parent / "include" / "eg_hip_shuffle.h"
U8, U32 = np.uint8, np.uint32
MODES = [False, True]
IDS = ["host", "device"]
N, W = 5, 3
P_TOY = 2**4096 - 2**4032 + 1     # any 4096-bit p and a q dividing nothing: the stub computes nothing


class Group(StubGroup):
    p = P_TOY


def prototype(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?$", p.strip()).group(1) for p in params.split(",")]
    return [p[2:] if p.startswith("d_") else p for p in names]


def make(g, shape, device, dtype=U8):
    a = np.random.default_rng(1).integers(0, 200, shape).astype(dtype)
    return g.to_device(a) if device else a


def called(g, name, device):
    (got, args), = g._lib.calls
    assert got == name + ("_dev" if device else "")
    names = prototype(got)
    assert names == prototype(name) and len(args) == len(names)
    d = dict(zip(names, args))
    assert addr(d["ctx"]) == 0xC0DE
    return d


def be_of(arg, n):
    import ctypes
    return int.from_bytes(ctypes.string_at(addr(arg), n), "big")


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_generators(device):
    g = Group()
    out = S.generators(g, 0xABC, N, device=device)
    d = called(g, "eg_shuffle_generators", device)
    assert d["N"] == N and be_of(d["gseed_be"], 32) == 0xABC
    assert be_of(d["cof_be"], 512) == (g.p - 1) // g.q
    assert isinstance(out, DeviceBuffer) == device and tuple(out.shape) == (N + 2, 512)
    assert addr(d["G"]) == addr(out)


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_mix(device):
    g = Group()
    rows, psi, r = make(g, (N, W, 2, 512), device), make(g, (N,), device, U32), make(g, (N, W, 32), device)
    out = S.mix(g, 0x77, rows, psi, r)
    d = called(g, "eg_shuffle_mix", device)
    assert (d["N"], d["w"]) == (N, W) and be_of(d["K_be"], 512) == 0x77
    assert addr(d["E"]) == addr(rows) and addr(d["psi"]) == addr(psi) and addr(d["r"]) == addr(r)   # not copied
    assert isinstance(out, DeviceBuffer) == device and tuple(out.shape) == (N, W, 2, 512)
    assert addr(d["E2"]) == addr(out)


def test_host_nonces_may_be_ints():
    g = Group()
    S.mix(g, 5, np.zeros((2, 1, 2, 512), U8), [1, 0], [[1], [2**256 - 1]])
    d = called(g, "eg_shuffle_mix", False)
    import ctypes
    assert ctypes.string_at(addr(d["r"]), 64) == (1).to_bytes(32, "big") + b"\xff" * 32
    assert ctypes.string_at(addr(d["psi"]), 8) == np.array([1, 0], U32).tobytes()


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_prove_and_verify(device):
    g = Group()
    rows, rows2 = make(g, (N, W, 2, 512), device), make(g, (N, W, 2, 512), device)
    psi, r = make(g, (N,), device, U32), make(g, (N, W, 32), device)
    G, nonces = make(g, (N + 2, 512), device), make(g, (4 * N + 3 + W, 32), device)
    proof = S.prove(g, 0x77, 0x88, 0x99, G, rows, rows2, psi, r, nonces)
    d = called(g, "eg_shuffle_prove", device)
    assert (d["N"], d["w"]) == (N, W)
    assert [be_of(d[k], n) for k, n in (("K_be", 512), ("qbar_be", 32), ("gseed_be", 32))] == [0x77, 0x88, 0x99]
    for name, val in (("G", G), ("E", rows), ("E2", rows2), ("psi", psi), ("r", r), ("nonces", nonces),
                      ("pc", proof.pc), ("chain", proof.chain), ("c", proof.c), ("s", proof.s),
                      ("s_hat", proof.s_hat), ("s_prime", proof.s_prime)):
        assert addr(d[name]) == addr(val), name
    shapes = [tuple(x.shape) for x in (proof.pc, proof.chain, proof.c, proof.s, proof.s_hat, proof.s_prime)]
    assert shapes == [(N, 512), (N, 512), (32,), (3 + W, 32), (N, 32), (N, 32)]
    assert all(isinstance(x, DeviceBuffer) == device for x in vars(proof).values())
    g._lib.calls.clear()
    ok, failed = S.verify(g, 0x77, 0x88, 0x99, G, rows, rows2, proof, check_inputs=True)
    d = called(g, "eg_shuffle_verify", device)
    assert (d["N"], d["w"], d["check_inputs"]) == (N, W, 1)
    for name, val in (("G", G), ("E", rows), ("E2", rows2), ("pc", proof.pc), ("chain", proof.chain), ("c", proof.c),
                      ("s", proof.s), ("s_hat", proof.s_hat), ("s_prime", proof.s_prime)):
        assert addr(d[name]) == addr(val), name
    if device:
        assert addr(d["ok"]) == ok.ptr and addr(d["failed_mask"]) == failed.ptr
        assert (ok.nbytes, failed.nbytes) == (1, 4)
    else:
        assert (ok, failed) == (False, 0)          # the stub wrote nothing: ok stays 0


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_what_does_not_fit_is_refused_before_any_call(device):
    g = Group()
    rows, psi, r = make(g, (N, W, 2, 512), device), make(g, (N,), device, U32), make(g, (N, W, 32), device)
    G, nonces = make(g, (N + 2, 512), device), make(g, (4 * N + 3 + W, 32), device)
    other = np.zeros((N,), U32) if device else g.to_device(np.zeros((N,), U32))
    before = (g.allocs, len(g.uploads))
    with pytest.raises(ValueError, match="rows"):
        S.mix(g, 5, make(g, (N, W, 512), device), psi, r)
    with pytest.raises(ValueError, match="psi"):
        S.mix(g, 5, rows, make(g, (N + 1,), device, U32), r)
    with pytest.raises(ValueError, match="r:"):
        S.mix(g, 5, rows, psi, make(g, (N, W + 1, 32), device))
    with pytest.raises(TypeError):
        S.mix(g, 5, rows, other, r)
    with pytest.raises(ValueError, match="G"):
        S.prove(g, 5, 6, 7, make(g, (N + 1, 512), device), rows, rows, psi, r, nonces)
    with pytest.raises(ValueError, match="nonces"):
        S.prove(g, 5, 6, 7, G, rows, rows, psi, r, make(g, (4 * N + 3, 32), device))
    with pytest.raises(ValueError, match="rows2"):
        S.prove(g, 5, 6, 7, G, rows, make(g, (N, W + 1, 2, 512), device), psi, r, nonces)
    assert g._lib.calls == []
    if not device:
        assert (g.allocs, len(g.uploads)) == before


def test_the_limits_are_checked_on_the_shape_alone():
    g = Group()
    with pytest.raises(ValueError, match="2\\^20"):
        S.mix(g, 5, g.device_empty(((1 << 20) + 1, 1, 2, 512)), g.device_empty(((1 << 20) + 1,), U32),
              g.device_empty(((1 << 20) + 1, 1, 32)))
    with pytest.raises(ValueError, match="2\\^21"):
        S.mix(g, 5, g.device_empty((1 << 11, (1 << 10) + 1, 2, 512)), g.device_empty((1 << 11,), U32),
              g.device_empty((1 << 11, (1 << 10) + 1, 32)))
    with pytest.raises(ValueError, match="shuffle"):
        S.generators(g, 1, 0)
    assert g._lib.calls == []
