"""The Python wrappers' marshalling, without the library or a GPU: a recording stub stands in for
libeg_hip.so, and every call of the 11 host / _dev pairs and of ballot.py's four ballot functions is
compared, argument by argument, with the prototype in include/eg_hip*.h (restated in CASES below).

Shapes: ElectionManifest([(2, 1), (3, 2)]) and Manifest(2, 1, 1), nb = 3, limit L = 2, nbytes = 32,
code_bytes = 2: the smallest where per-contest tables, a limit above 1 and more than one item all
appear."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from electionguard import ballot as B
from electionguard import codes as C
from electionguard import contest_data as D
from electionguard import preencrypt as P
from electionguard import range_proof as R
from electionguard.core.group import DeviceBuffer

NB, L, NBYTES, CODE_BYTES, QBAR = 3, 2, 32, 2, 0x1234567
MANS = [B.ElectionManifest([(2, 1), (3, 2)]), B.Manifest(2, 1, 1)]
MODES = ["host", "device"]
U8, U32 = np.uint8, np.uint32


# ---------------------------------------------------------------------------------------------
# the stubs
# ---------------------------------------------------------------------------------------------
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
        self._next, self.allocs, self.uploads = 0x7000_0000_0000, 0, []

    def device_empty(self, shape, dtype=U8):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        d = DeviceBuffer.__new__(DeviceBuffer)   # as DeviceBuffer.__getitem__ makes its views
        d.group, d.shape, d.dtype = self, shape, np.dtype(dtype)
        d.nbytes = int(np.prod(shape)) * d.dtype.itemsize
        d._h, d._owner = ctypes.c_void_p(self._next), self   # a fake address; never freed
        self._next += (d.nbytes + 256) // 256 * 256
        self.allocs += 1
        return d

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        d = self.device_empty(a.shape, a.dtype)
        self.uploads.append((d, a.copy()))
        return d


KEY = SimpleNamespace(K_be=bytes(range(256)) * 2)


def addr(x):
    """The address a pointer argument holds, or of what a caller passed."""
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if isinstance(x, bytes):
        return ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value
    return ctypes.cast(x, ctypes.c_void_p).value


# ---------------------------------------------------------------------------------------------
# the 11 pairs.  A case gives its per-item inputs (the first decides the mode), the wrapper call,
# the prototype's arguments after ctx, and its outputs (shape, dtype, flag), None when not wanted.
# Prototype tokens: an int is a scalar; ("u32", table); "K"; "qbar"; ("in", name); ("once", i) the
# i-th of the case's once tables; ("out", j).
# ---------------------------------------------------------------------------------------------
def dims(man):
    sh = P.pre_shape(man)
    return SimpleNamespace(nsel=man.nsel, nc=man.n_contests, spc=("u32", man.spc_list), lim=("u32", man.limits),
                           V=sh.V, S=sh.S, T=sh.T)


def hashes_of(man, rng):
    return C.ManifestHashes(*(rng.integers(0, 256, s, U8) for s in ((man.nsel, 32), (man.n_contests, 32), (32,))))


def ins(*names):
    return [("in", n) for n in names]


def outs(n):
    return [("out", j) for j in range(n)]


CASES = {
    # eg_derive_ballot_nonces(ctx, nballots, ncontest, spc, ballot_nonces, sel_nonces, contest_nonces)
    "eg_derive_ballot_nonces": dict(
        inputs=lambda d, nb: {"bn": ((nb, 32), U8)},
        call=lambda g, man, h, x, opt: C.derive_nonces(g, man, x["bn"]),
        proto=lambda d, nb, h: [nb, d.nc, d.spc, *ins("bn"), *outs(2)],
        outs=lambda d, nb, opt: [((nb, d.nsel, 4, 32), U8, 0), ((nb, d.nc, 32), U8, 0)]),
    # eg_ballot_hashes(ctx, nballots, ncontest, spc, dsel, dcon, manifest_hash, ballot_ids, cts, out_ballot_hash,
    #                  out_sel_hash, out_contest_hash)
    "eg_ballot_hashes": dict(
        optional=True, once=lambda h: [h.dsel, h.dcon, h.manifest_hash],
        inputs=lambda d, nb: {"cts": ((nb, d.nsel, 2, 512), U8), "ids": ((nb, 32), U8)},
        call=lambda g, man, h, x, opt: C.ballot_hashes(g, man, h, x["ids"], x["cts"], parts=opt),
        flat=lambda r, opt: list(r) if opt else [r, None, None],
        proto=lambda d, nb, h: [nb, d.nc, d.spc, ("once", 0), ("once", 1), ("once", 2), *ins("ids", "cts"), *outs(3)],
        outs=lambda d, nb, opt: [((nb, 32), U8, 0), ((nb, d.nsel, 32), U8, 0) if opt else None,
                                 ((nb, d.nc, 32), U8, 0) if opt else None]),
    # eg_verify_code_chain(ctx, nballots, seed, timestamps, ballot_hashes, codes, ok)
    "eg_verify_code_chain": dict(
        inputs=lambda d, nb: {"B": ((nb, 32), U8), "ts": ((nb, 32), U8), "codes": ((nb, 32), U8), "seed": ((32,), U8)},
        call=lambda g, man, h, x, opt: C.verify_code_chain(g, x["seed"], x["ts"], x["B"], x["codes"]),
        flat=lambda r, opt: [r],
        proto=lambda d, nb, h: [nb, *ins("seed", "ts", "B", "codes"), *outs(1)],
        outs=lambda d, nb, opt: [((nb,), U8, 1)]),
    # eg_derive_contest_data_nonces(ctx, nballots, ncontest, ballot_nonces, out_r)
    "eg_derive_contest_data_nonces": dict(
        inputs=lambda d, nb: {"bn": ((nb, 32), U8)},
        call=lambda g, man, h, x, opt: D.derive_nonces(g, man.n_contests, x["bn"]),
        flat=lambda r, opt: [r],
        proto=lambda d, nb, h: [nb, d.nc, *ins("bn"), *outs(1)],
        outs=lambda d, nb, opt: [((nb, d.nc, 32), U8, 0)]),
    # eg_seal_contest_data(ctx, K_be, nballots, ncontest, nbytes, ballot_ids, nonces_r, data, out_c0, out_c1, out_c2)
    "eg_seal_contest_data": dict(
        inputs=lambda d, nb: {"ids": ((nb, 32), U8), "r": ((nb * d.nc, 32), U8), "data": ((nb * d.nc, NBYTES), U8)},
        call=lambda g, man, h, x, opt: D.seal(g, KEY, man.n_contests, NBYTES, x["ids"], x["r"], x["data"]),
        proto=lambda d, nb, h: ["K", nb, d.nc, NBYTES, *ins("ids", "r", "data"), *outs(3)],
        outs=lambda d, nb, opt: [((nb * d.nc, 512), U8, 0), ((nb * d.nc, NBYTES), U8, 0), ((nb * d.nc, 32), U8, 0)]),
    # eg_open_contest_data(ctx, nballots, ncontest, nbytes, ballot_ids, c0, kappa, c1, c2, out_data, out_ok)
    "eg_open_contest_data": dict(
        inputs=lambda d, nb: {"ids": ((nb, 32), U8), "c0": ((nb * d.nc, 512), U8), "kappa": ((nb * d.nc, 512), U8),
                              "c1": ((nb * d.nc, NBYTES), U8), "c2": ((nb * d.nc, 32), U8)},
        call=lambda g, man, h, x, opt: D.open_sealed(g, man.n_contests, NBYTES, x["ids"], x["c0"], x["kappa"], x["c1"],
                                                     x["c2"]),
        proto=lambda d, nb, h: [nb, d.nc, NBYTES, *ins("ids", "c0", "kappa", "c1", "c2"), *outs(2)],
        outs=lambda d, nb, opt: [((nb * d.nc, NBYTES), U8, 0), ((nb * d.nc,), U8, 1)]),
    # eg_range_prove(ctx, K_be, qbar_be, n, limit, cts, values, R, nonces, proofs)
    "eg_range_prove": dict(
        inputs=lambda d, nb: {"cts": ((nb, 2, 512), U8), "values": ((nb,), U8), "R": ((nb, 32), U8),
                              "nonces": ((nb, 2 * L + 3, 32), U8)},
        call=lambda g, man, h, x, opt: R.prove(g, KEY, QBAR, L, x["cts"], x["values"], x["R"], x["nonces"]),
        flat=lambda r, opt: [r],
        proto=lambda d, nb, h: ["K", "qbar", nb, L, *ins("cts", "values", "R", "nonces"), *outs(1)],
        outs=lambda d, nb, opt: [((nb, L + 1, 2, 32), U8, 0)]),
    # eg_range_verify(ctx, K_be, qbar_be, n, limit, cts, proofs, ok)
    "eg_range_verify": dict(
        inputs=lambda d, nb: {"cts": ((nb, 2, 512), U8), "proofs": ((nb, L + 1, 2, 32), U8)},
        call=lambda g, man, h, x, opt: R.verify(g, KEY, QBAR, L, x["cts"], x["proofs"]),
        flat=lambda r, opt: [r],
        proto=lambda d, nb, h: ["K", "qbar", nb, L, *ins("cts", "proofs"), *outs(1)],
        outs=lambda d, nb, opt: [((nb,), U8, 1)]),
    # eg_preencrypt_ballots(ctx, K_be, nballots, ncontest, spc, code_bytes, dcon, manifest_hash, ballot_ids,
    #                       ballot_nonces, sorted, perm, codes, unique, conf, chash, vec_cts)
    "eg_preencrypt_ballots": dict(
        optional=True, once=lambda h: [h.dcon, h.manifest_hash],
        inputs=lambda d, nb: {"bn": ((nb, 32), U8), "ids": ((nb, 32), U8)},
        call=lambda g, man, h, x, opt: P.preencrypt_ballots(g, KEY, man, h, x["ids"], x["bn"], CODE_BYTES,
                                                            with_cts=opt),
        flat=lambda r, opt: [r.sorted, r.perm, r.codes, r.unique, r.conf, r.chash, r.vec_cts],
        proto=lambda d, nb, h: ["K", nb, d.nc, d.spc, CODE_BYTES, ("once", 0), ("once", 1), *ins("ids", "bn"),
                                *outs(7)],
        outs=lambda d, nb, opt: [((nb, d.nsel, 32), U8, 0), ((nb, d.nsel), U32, 0), ((nb, d.nsel), U32, 0),
                                 ((nb,), U8, 0), ((nb, 32), U8, 0), ((nb, d.nc, 32), U8, 0),
                                 ((nb, d.V, 2, 512), U8, 0) if opt else None]),
    # eg_preencrypt_record(ctx, K_be, nballots, ncontest, spc, limits, code_bytes, dcon, ballot_nonces, votes, sorted,
    #                      sel_vecs, sel_rank, sel_codes, sel_nonces, contest_nonces, ok)
    "eg_preencrypt_record": dict(
        once=lambda h: [h.dcon],
        inputs=lambda d, nb: {"votes": ((nb, d.nsel), U8), "bn": ((nb, 32), U8), "sorted": ((nb, d.nsel, 32), U8)},
        call=lambda g, man, h, x, opt: P.record_parts(g, KEY, man, h, x["bn"], x["votes"], x["sorted"], CODE_BYTES),
        flat=lambda r, opt: [r.sel_vecs, r.sel_rank, r.sel_codes, r.sel_nonces, r.contest_nonces, r.ok],
        proto=lambda d, nb, h: ["K", nb, d.nc, d.spc, d.lim, CODE_BYTES, ("once", 0), *ins("bn", "votes", "sorted"),
                                *outs(6)],
        outs=lambda d, nb, opt: [((nb, d.S, 2, 512), U8, 0), ((nb, d.T), U32, 0), ((nb, d.T), U32, 0),
                                 ((nb, d.nsel, 4, 32), U8, 0), ((nb, d.nc, 32), U8, 0), ((nb, d.nc), U8, 0)]),
    # eg_preencrypt_verify(ctx, nballots, ncontest, spc, limits, code_bytes, dcon, manifest_hash, ballot_ids, sel_vecs,
    #                      sel_rank, sel_codes, sorted, cts, conf, ok_contest, ok_conf)
    "eg_preencrypt_verify": dict(
        once=lambda h: [h.dcon, h.manifest_hash],
        inputs=lambda d, nb: {"conf": ((nb, 32), U8), "ids": ((nb, 32), U8), "sel_vecs": ((nb, d.S, 2, 512), U8),
                              "sel_rank": ((nb, d.T), U32), "sel_codes": ((nb, d.T), U32),
                              "sorted": ((nb, d.nsel, 32), U8), "cts": ((nb, d.nsel, 2, 512), U8)},
        call=lambda g, man, h, x, opt: P.verify_recorded(g, man, h, x["ids"], x["sel_vecs"], x["sel_rank"],
                                                         x["sel_codes"], x["sorted"], x["cts"], x["conf"], CODE_BYTES),
        proto=lambda d, nb, h: [nb, d.nc, d.spc, d.lim, CODE_BYTES, ("once", 0), ("once", 1),
                                *ins("ids", "sel_vecs", "sel_rank", "sel_codes", "sorted", "cts", "conf"), *outs(2)],
        outs=lambda d, nb, opt: [((nb, d.nc), U8, 1), ((nb,), U8, 1)]),
}
PAIRS = sorted(CASES)


def setup(name, man, nb, mode, device=None):
    """-> (group, hashes, host inputs, the inputs as passed: DeviceBuffers where device(name) says so)."""
    rng = np.random.default_rng(5)
    g, h = StubGroup(), hashes_of(man, rng)
    host = {k: rng.integers(0, 200, shape).astype(dt)
            for k, (shape, dt) in CASES[name]["inputs"](dims(man), nb).items()}
    device = device or (lambda k: mode == "device")
    return g, h, host, {k: g.to_device(a) if device(k) else a for k, a in host.items()}


def run(name, man, nb, mode, opt):
    """One valid call -> (group, hashes, passed inputs, flat outputs, the uploads the wrapper made)."""
    case = CASES[name]
    g, h, _, x = setup(name, man, nb, mode)
    before = len(g.uploads)
    r = case["call"](g, man, h, x, opt)
    return g, h, x, case.get("flat", lambda r, opt: list(r))(r, opt), g.uploads[before:]


@pytest.mark.parametrize("nb", [NB, 0])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("man", MANS, ids=["unequal", "uniform"])
@pytest.mark.parametrize("name,opt", [(n, o) for n in PAIRS
                                      for o in ((False, True) if CASES[n].get("optional") else (False,))])
def test_pair_call_matches_prototype(name, opt, man, mode, nb):
    case, d = CASES[name], dims(man)
    g, h, x, got, uploads = run(name, man, nb, mode, opt)
    dev = mode == "device"
    assert [c[0] for c in g._lib.calls] == [name + "_dev" if dev else name]
    args = g._lib.calls[0][1]
    assert args[0] is g.handle
    once = case.get("once", lambda h: [])(h)
    if dev and once:   # one buffer of 32-byte rows, in prototype order
        assert len(uploads) == 1
        assert bytes(uploads[0][1].reshape(-1)) == b"".join(bytes(t.reshape(-1)) for t in once)
    else:
        assert not uploads
    want_outs = case["outs"](d, nb, opt)
    proto = case["proto"](d, nb, h)
    assert len(args) == 1 + len(proto) and len(got) == len(want_outs)
    for pos, (tok, a) in enumerate(zip(proto, args[1:]), 1):
        where = f"{name} argument {pos} ({tok})"
        if isinstance(tok, int):
            assert a == tok and not isinstance(a, bool), where
        elif tok == "K":
            assert addr(a) == addr(KEY.K_be), where
        elif tok == "qbar":
            assert ctypes.string_at(addr(a), 32) == QBAR.to_bytes(32, "big"), where
        elif tok[0] == "u32":
            assert np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint32)), (d.nc,)).tolist() == \
                [int(v) for v in tok[1]], where
        elif tok[0] == "in":
            assert addr(a) == addr(x[tok[1]]), where
        elif tok[0] == "once":
            rows = sum(t.size for t in once[:tok[1]])
            assert addr(a) == (uploads[0][0].ptr + rows if dev else addr(once[tok[1]])), where
        else:
            spec, out = want_outs[tok[1]], got[tok[1]]
            if spec is None:
                assert a is None and out is None, where
                continue
            shape, dtype, flag = spec
            assert isinstance(out, DeviceBuffer if dev else np.ndarray), where
            assert tuple(out.shape) == shape and out.dtype == (bool if flag and not dev else dtype), where
            if flag and not dev:   # the bool array is a copy of the flag bytes the library wrote
                assert addr(a), where
            else:
                assert addr(a) == addr(out) and out.nbytes == int(np.prod(shape)) * np.dtype(dtype).itemsize, where
    if name == "eg_preencrypt_record":   # the sorted hashes are published as they were given
        r = case["call"](g, man, h, x, opt)
        assert r.ballots is None and addr(r.sorted) == addr(x["sorted"])
        assert r.sorted.shape == (nb, d.nsel, 32)


def columns(name):
    return list(CASES[name]["inputs"](dims(MANS[0]), NB))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,col", [(n, c) for n in PAIRS for c in columns(n)])
def test_short_column_is_a_value_error(name, col, mode):
    man = MANS[0]
    g, h, host, _ = setup(name, man, NB, mode)
    host[col] = host[col][:-1]   # one row short (the first column: one item fewer than the others hold)
    if len(host) == 1:
        host[col] = host[col].reshape(-1)[:-1]   # the only column: no whole number of items
    x = {k: g.to_device(a) if mode == "device" else a for k, a in host.items()}
    allocs = g.allocs
    with pytest.raises(ValueError):
        CASES[name]["call"](g, man, h, x, False)
    assert not g._lib.calls and g.allocs == allocs


@pytest.mark.parametrize("name,col", [(n, c) for n in PAIRS for c in columns(n) if len(columns(n)) > 1])
def test_host_and_device_columns_do_not_mix(name, col):
    man = MANS[0]
    for device in (lambda k: k != col, lambda k: k == col):   # one host array among buffers, and the reverse
        g, h, _, x = setup(name, man, NB, None, device)
        allocs = g.allocs
        with pytest.raises(TypeError):
            CASES[name]["call"](g, man, h, x, False)
        assert not g._lib.calls and g.allocs == allocs


def test_error_names_the_column_and_both_counts():
    g, h, host, _ = setup("eg_range_prove", MANS[0], NB, "host")
    with pytest.raises(ValueError, match=r"nonces: expected 3 x 224 bytes, got 448"):
        R.prove(g, KEY, QBAR, L, host["cts"], host["values"], host["R"], host["nonces"][:-1])
    with pytest.raises(TypeError, match="R: a DeviceBuffer"):
        R.prove(g, KEY, QBAR, L, g.to_device(host["cts"]), g.to_device(host["values"]), host["R"], host["nonces"])


# ---------------------------------------------------------------------------------------------
# ballot.py: the uniform and the manifest entries
# eg_encrypt_ballots(ctx, K_be, qbar_be, nballots, ncontest, spc, votes, sel_nonces, contest_nonces, cts, rproof,
#                    cproof); _manifest: spc is a table
# eg_verify_ballots(ctx, K_be, qbar_be, nballots, ncontest, spc, placeholders, limit, cts, rproof, cproof, cast,
#                   ok_sel, ok_contest, tally_be); _manifest: spc, placeholders and limit are tables
# ---------------------------------------------------------------------------------------------
def shape_args_ok(man, args, verify):
    tables = [man.spc_list] + ([man.placeholders, man.limits] if verify else [])
    if isinstance(man, B.ElectionManifest):
        got = [np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint32)), (man.n_contests,)).tolist()
               for a in args]
        return got == [[int(v) for v in t] for t in tables]
    return list(args) == [man.spc] + ([man.votes_allowed, man.votes_allowed] if verify else [])


def head_ok(g, args, nb, man):
    return args[0] is g.handle and addr(args[1]) == addr(KEY.K_be) and \
        ctypes.string_at(addr(args[2]), 32) == QBAR.to_bytes(32, "big") and args[3:5] == (nb, man.n_contests)


@pytest.mark.parametrize("man", MANS, ids=["unequal", "uniform"])
def test_ballot_entries(man):
    suffix = "_manifest" if isinstance(man, B.ElectionManifest) else ""
    nsel, nc = man.nsel, man.n_contests
    g = StubGroup()
    votes, sn, cn = np.zeros((NB, nsel), U8), np.zeros((NB, nsel, 4, 32), U8), np.zeros((NB, nc, 32), U8)
    eb = B.batch_encryption(g, KEY, QBAR, man, votes, sn, cn)
    B.batch_encryption_device(g, KEY, QBAR, man, NB, 11, 12, 13, 14, 15, 16)
    v = B.Verifier(g, KEY, QBAR, man)
    ok_s, ok_c, tally = v.verify(eb, cast=np.array([1, 0, 1], bool))
    assert v.verify(eb, with_tally=False)[2] is None
    v.verify_device(21, 22, 23, NB, 24, 25, None, 26)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3), (n4, a4) = g._lib.calls
    enc, ver = "eg_encrypt_ballots" + suffix, "eg_verify_ballots" + suffix
    assert [n0, n1, n2, n3, n4] == [enc, enc + "_dev", ver, ver, ver + "_dev"]
    for a in (a0, a1):
        assert len(a) == 12 and head_ok(g, a, NB, man) and shape_args_ok(man, a[5:6], False)
    assert [addr(p) for p in a0[6:]] == [addr(t) for t in (votes, sn, cn, eb.cts, eb.rproof, eb.cproof)]
    assert a1[6:] == (11, 12, 13, 14, 15, 16)
    assert (eb.cts.shape, eb.rproof.shape, eb.cproof.shape) == ((NB, nsel, 2, 512), (NB, nsel, 4, 32), (NB, nc, 2, 32))
    for a in (a2, a3, a4):
        assert len(a) == 15 and head_ok(g, a, NB, man) and shape_args_ok(man, a[5:8], True)
    assert [addr(p) for p in a2[8:11]] == [addr(t) for t in (eb.cts, eb.rproof, eb.cproof)]
    assert addr(a2[11]) and addr(a2[12]) and addr(a2[13]) and addr(a2[14]) == addr(tally)
    assert a3[11] is None and a3[14] is None
    assert a4[8:] == (21, 22, 23, 26, 24, 25, None)
    assert (ok_s.shape, ok_s.dtype, ok_c.shape, ok_c.dtype) == ((NB, nsel), bool, (NB, nc), bool)
    assert tally.shape == (man.n_real, 2, 512) and tally.dtype == U8


def test_empty_ballot_batches_encrypt_nothing():
    g = StubGroup()
    eb = B.batch_encryption(g, KEY, QBAR, MANS[0], np.zeros((0, 8), U8), np.zeros((0, 8, 4, 32), U8),
                            np.zeros((0, 2, 32), U8))
    B.batch_encryption_device(g, KEY, QBAR, MANS[0], 0, 1, 2, 3, 4, 5, 6)
    assert not g._lib.calls and eb.cts.shape == (0, 8, 2, 512)
