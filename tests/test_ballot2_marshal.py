"""The marshalling of electionguard.ballot2's two GPU wrappers, without the library or a GPU: a
recording stub stands in for libeg_hip.so (the pattern of tests/test_marshal.py), and the call of
each host / _dev pair is compared, argument by argument, with the prototype's parameter list read
from include/eg_hip_ballot2.h.  Manifest [(2, 1, 1), (1, 2, 2)], nb = 3: two limits, ragged rows and
more than one ballot."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from electionguard import ballot2 as b2
from electionguard.core.group import DeviceBuffer

HEADER = Path(__file__).resolve().parent.parent / "include" / "eg_hip_ballot2.h"
NB, QBAR = 3, 0x1234567
MAN = b2.Manifest2([(2, 1, 1), (1, 2, 2)])
KEY = SimpleNamespace(K_be=bytes(range(256)) * 2)
U8 = np.uint8


class RecordingLib:
    """Every eg_* attribute appends (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("eg_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


class StubGroup:
    q, hash_format, ct_encrypt = 2**256 - 189, "fixed", False

    def __init__(self):
        self._lib, self.handle = RecordingLib(), ctypes.c_void_p(0xC0DE)
        self._next, self.allocs = 0x7000_0000_0000, 0

    def device_empty(self, shape, dtype=U8):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        d = DeviceBuffer.__new__(DeviceBuffer)
        d.group, d.shape, d.dtype = self, shape, np.dtype(dtype)
        d.nbytes = int(np.prod(shape)) * d.dtype.itemsize
        d._h, d._owner = ctypes.c_void_p(self._next), self   # a fake address; never freed
        self._next += (d.nbytes + 256) // 256 * 256
        self.allocs += 1
        return d

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        return self.device_empty(a.shape, a.dtype)


def addr(x):
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if isinstance(x, bytes):
        return ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value
    return ctypes.cast(x, ctypes.c_void_p).value


def prototype(name):
    """The parameter names of name's declaration in the header, in order."""
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    return [re.search(r"(\w+)\s*(\[\w+\])?\s*$", p.strip()).group(1) for p in params.split(",")]


SHAPES = {"votes": (MAN.NS,), "sel_nonces": (MAN.SN, 32), "contest_nonces": (MAN.CN, 32), "cts": (MAN.NS, 2, 512),
          "sproof": (MAN.SP, 2, 32), "cproof": (MAN.CP, 2, 32), "cast": (), "ok_sel": (MAN.NS,),
          "ok_contest": (MAN.n_contests,)}


def columns(g, names, device):
    rng = np.random.default_rng(1)
    x = {n: rng.integers(0, 2, (NB,) + SHAPES[n], U8) for n in names}
    return {n: g.to_device(a) for n, a in x.items()} if device else x


def check(g, name, device, given, outs):
    """The one recorded call against the prototype; given: parameter -> what the caller passed,
    outs: parameter -> what the wrapper returned (None: a null pointer expected)."""
    (called, args), = g._lib.calls
    assert called == name + ("_dev" if device else "")
    names = [p[2:] if p.startswith("d_") else p for p in prototype(called)]
    assert prototype(name) == names, "the pair's prototypes differ in more than the d_ prefix"
    assert len(args) == len(names)
    assert names[0] == "ctx" and addr(args[0]) == 0xC0DE
    for p, a in zip(names[1:], args[1:]):
        if p == "K_be":
            assert ctypes.string_at(addr(a), 512) == KEY.K_be
        elif p == "qbar_be":
            assert ctypes.string_at(addr(a), 32) == QBAR.to_bytes(32, "big")
        elif p == "nballots":
            assert a == NB
        elif p == "ncontest":
            assert a == MAN.n_contests
        elif p in ("nsel", "olimit", "climit"):
            assert addr(a) == getattr(MAN, p).ctypes.data and getattr(MAN, p).dtype == np.uint32
        elif p in given:
            want = given[p]
            assert isinstance(want, DeviceBuffer) == device
            if device or p != "cast":
                assert addr(a) == addr(want), p    # passed through, not copied
            else:
                assert a is not None               # host cast flags are normalised to 0 / 1 bytes
        else:
            out = outs[p]
            if out is None:
                assert a is None, p
            else:
                assert isinstance(out, DeviceBuffer) == device, p
                if device:
                    assert addr(a) == out.ptr, p
                want = (NB,) + SHAPES[p] if p in SHAPES else (MAN.NS, 2, 512)
                assert tuple(out.shape) == want, p


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_encrypt_marshals_the_prototype(device):
    g = StubGroup()
    x = columns(g, ["votes", "sel_nonces", "contest_nonces"], device)
    eb = b2.encrypt(g, KEY, QBAR, MAN, x["votes"], x["sel_nonces"], x["contest_nonces"])
    check(g, "eg_encrypt_ballots_v2", device, x, {"cts": eb.cts, "sproof": eb.sproof, "cproof": eb.cproof})
    assert eb.n == NB


@pytest.mark.parametrize("with_tally", [True, False])
@pytest.mark.parametrize("cast", [True, False])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_verify_marshals_the_prototype(device, cast, with_tally):
    g = StubGroup()
    x = columns(g, ["cts", "sproof", "cproof"] + (["cast"] if cast else []), device)
    ok_s, ok_c, tally = b2.Verifier2(g, KEY, QBAR, MAN).verify(b2.EncryptedBallots2(x["cts"], x["sproof"], x["cproof"]),
                                                              cast=x.get("cast"), with_tally=with_tally)
    assert (tally is None) == (not with_tally)
    if not cast:
        x["cast"] = None
    check(g, "eg_verify_ballots_v2", device, {k: v for k, v in x.items() if v is not None},
          {"cast": None, "ok_sel": ok_s, "ok_contest": ok_c, "tally_be": tally})
    if not device:
        assert ok_s.dtype == bool and ok_c.dtype == bool


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_short_column_is_refused_before_any_call(device):
    g = StubGroup()
    x = columns(g, ["votes", "sel_nonces", "contest_nonces", "cts", "sproof", "cproof"], device)
    short = x["sel_nonces"][:NB - 1]
    with pytest.raises(ValueError, match="sel_nonces"):
        b2.encrypt(g, KEY, QBAR, MAN, x["votes"], short, x["contest_nonces"])
    with pytest.raises(ValueError, match="cproof"):
        b2.Verifier2(g, KEY, QBAR, MAN).verify(b2.EncryptedBallots2(x["cts"], x["sproof"], x["cproof"][:NB - 1]))
    with pytest.raises(TypeError):
        mixed = x["sproof"] if not device else np.zeros((NB, MAN.SP, 2, 32), U8)
        other = g.to_device(mixed) if not device else mixed
        b2.Verifier2(g, KEY, QBAR, MAN).verify(b2.EncryptedBallots2(x["cts"], other, x["cproof"]))
    assert g._lib.calls == []
