"""The marshalling of electionguard.codes2's GPU wrappers, without the library or a GPU: the
recording stub of tests/test_marshal.py stands in for libeg_hip.so, and each call of a host / _dev
pair is compared, argument by argument, with the prototype's parameter list read from
include/eg_hip_codes2.h (the ballot hashes: from include/eg_hip_codes.h, with spc = nsel).
Manifest [(2, 1, 1), (1, 2, 2)], nb = 3: two limits, ragged rows and more than one ballot."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from test_marshal import KEY, StubGroup, addr

from electionguard import ballot2 as b2
from electionguard import codes as C
from electionguard import codes2 as c2
from electionguard.core.group import DeviceBuffer

INCLUDE = Path(__file__).resolve().parent.parent / "include"
NB = 3
MAN = b2.Manifest2([(2, 1, 1), (1, 2, 2)])
U8 = np.uint8
MODES = [False, True]
IDS = ["host", "device"]

SHAPES = {"ballot_nonces": (32,), "sel_nonces": (MAN.SN, 32), "contest_nonces": (MAN.CN, 32),
          "cts": (MAN.NS, 2, 512), "votes": (MAN.NS,), "ok": (MAN.NS,), "ballot_ids": (32,),
          "out_ballot_hash": (32,), "out_sel_hash": (MAN.NS, 32), "out_contest_hash": (MAN.n_contests, 32)}


def prototype(header, name):
    """The parameter names of name's declaration in the header, in order, without a d_ prefix."""
    src = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\w+\])?\s*$", p.strip()).group(1) for p in params.split(",")]
    return [p[2:] if p.startswith("d_") else p for p in names]


def columns(g, names, device):
    rng = np.random.default_rng(1)
    x = {n: rng.integers(0, 2, (NB,) + SHAPES[n], U8) for n in names}
    return {n: g.to_device(a) for n, a in x.items()} if device else x


def check(g, header, name, device, given, outs, once=()):
    """The one recorded call against the prototype; given: parameter -> what the caller passed,
    outs: parameter -> what the wrapper returned (None: a null pointer expected), once: the
    parameters that are host tables read once per call."""
    (called, args), = g._lib.calls
    assert called == name + ("_dev" if device else "")
    names = prototype(header, called)
    assert names == prototype(header, name), "the pair's prototypes differ in more than the d_ prefix"
    assert len(args) == len(names)
    assert names[0] == "ctx" and addr(args[0]) == 0xC0DE
    for p, a in zip(names[1:], args[1:]):
        if p == "K_be":
            assert ctypes.string_at(addr(a), 512) == KEY.K_be
        elif p == "nballots":
            assert a == NB
        elif p == "ncontest":
            assert a == MAN.n_contests
        elif p in ("nsel", "olimit", "climit"):
            assert addr(a) == getattr(MAN, p).ctypes.data and getattr(MAN, p).dtype == np.uint32
        elif p == "spc":
            assert ctypes.cast(a, ctypes.POINTER(ctypes.c_uint32))[:MAN.n_contests] == MAN.nsel.tolist()
        elif p in once:
            assert a is not None
        elif p in given:
            assert isinstance(given[p], DeviceBuffer) == device
            assert addr(a) == addr(given[p]), p        # passed through, not copied
        else:
            out = outs[p]
            if out is None:
                assert a is None, p
                continue
            assert isinstance(out, DeviceBuffer) == device, p
            if device:
                assert addr(a) == out.ptr, p
            assert tuple(out.shape) == (NB,) + SHAPES[p], p


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_derive_marshals_the_prototype(device):
    g = StubGroup()
    x = columns(g, ["ballot_nonces"], device)
    sn, cn = c2.derive_nonces2(g, MAN, x["ballot_nonces"])
    check(g, "eg_hip_codes2.h", "eg_derive_ballot_nonces_v2", device, x, {"sel_nonces": sn, "contest_nonces": cn})


@pytest.mark.parametrize("as_eb", [False, True])
@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_open_marshals_the_prototype(device, as_eb):
    g = StubGroup()
    x = columns(g, ["ballot_nonces", "cts"], device)
    eb = b2.EncryptedBallots2(x["cts"], None, None) if as_eb else x["cts"]
    votes, ok = c2.open_ballots2(g, KEY, MAN, eb, x["ballot_nonces"])
    check(g, "eg_hip_codes2.h", "eg_open_ballots_v2", device, x, {"votes": votes, "ok": ok})
    if not device:
        assert votes.dtype == U8 and ok.dtype == bool


@pytest.mark.parametrize("parts", [False, True])
@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_ballot_hashes_marshal_the_codes_prototype_with_spc_nsel(device, parts):
    g = StubGroup()
    rng = np.random.default_rng(2)
    h = C.ManifestHashes(*(rng.integers(0, 256, s, U8) for s in ((MAN.NS, 32), (MAN.n_contests, 32), (32,))))
    x = columns(g, ["cts", "ballot_ids"], device)
    r = c2.ballot_hashes2(g, MAN, h, x["ballot_ids"], x["cts"], parts=parts)
    B, hs, hc = r if parts else (r, None, None)
    check(g, "eg_hip_codes.h", "eg_ballot_hashes", device, x,
          {"out_ballot_hash": B, "out_sel_hash": hs, "out_contest_hash": hc}, once=("dsel", "dcon", "manifest_hash"))


@pytest.mark.parametrize("device", MODES, ids=IDS)
def test_a_column_of_the_wrong_size_is_refused_before_any_call(device):
    g = StubGroup()
    x = columns(g, ["ballot_nonces", "cts", "ballot_ids"], device)
    short = lambda n: g.to_device(np.zeros((NB - 1,) + SHAPES[n], U8)) if device else x[n][:NB - 1]
    with pytest.raises(ValueError, match="ballot_nonces"):
        c2.open_ballots2(g, KEY, MAN, x["cts"], short("ballot_nonces"))
    with pytest.raises(ValueError, match="ballot_ids"):
        h = C.ManifestHashes(np.zeros((MAN.NS, 32), U8), np.zeros((MAN.n_contests, 32), U8), np.zeros(32, U8))
        c2.ballot_hashes2(g, MAN, h, short("ballot_ids"), x["cts"])
    with pytest.raises(TypeError):
        other = np.zeros((NB, 32), U8) if device else g.to_device(x["ballot_nonces"])
        c2.open_ballots2(g, KEY, MAN, x["cts"], other)
    before = (g.allocs, len(g.uploads))
    with pytest.raises(ValueError, match="option limit"):      # before anything is uploaded
        c2.encrypt_ballots_seeded2(g, KEY, 1, MAN, None, [[2, 0, 0]], np.zeros((1, 32), U8), np.zeros((1, 32), U8),
                                   [0], 0)
    assert g._lib.calls == [] and (g.allocs, len(g.uploads)) == before
