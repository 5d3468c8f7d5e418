"""GPU: ballot nonces, ballot hashes and the code chain (include/eg_hip_codes.h,
electionguard.codes, csrc/eg_codes.hpp) against the bare-hashlib restatement of codes_ref.py,
byte for byte.  Ciphertext bytes are random unless a test says otherwise: hashing needs no valid
group elements."""
import ctypes

import numpy as np
import pytest

import codes_ref as R

pytestmark = pytest.mark.gpu

FORMATS = ("fixed", "minimal")
RAGGED = [(2, 1), (1, 1), (4, 2)]   # spc 3, 2, 6
U32P = ctypes.POINTER(ctypes.c_uint32)


def _man(shape):
    from electionguard.ballot import ElectionManifest, Manifest
    return Manifest(*shape) if isinstance(shape, tuple) else ElectionManifest(shape)


def _data(man, nb, seed):
    from electionguard.codes import ManifestHashes
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    return dict(man=man, nb=nb, bn=r(nb, 32), ids=r(nb, 32), cts=r(nb, man.nsel, 2, 512), seed=r(32),
                ts=R.arr([R.i32(1700000000 + 3 * b) for b in range(nb)], (nb, 32)),
                hashes=ManifestHashes(r(man.nsel, 32), r(man.n_contests, 32), r(32)))


def _ref_hashes(q, fmt, d):
    h = d["hashes"]
    return R.hashes(q, fmt, d["man"].spc_list, h.dsel, h.dcon, h.manifest_hash, d["ids"], d["cts"])


@pytest.fixture
def fmt_group(group):
    """the session's group, handed back in the fixed-width format whatever the test set"""
    try:
        yield group
    finally:
        group.hash_format = "fixed"


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------------------------------
# parity with hashlib
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RAGGED, (2, 2, 1)], ids=["ragged", "uniform"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_with_hashlib(fmt_group, fmt, shape):
    from electionguard import codes as C
    g = fmt_group
    g.hash_format = fmt
    d = _data(_man(shape), 3, 11)
    man, q = d["man"], g.q
    rsn, rcn = R.nonces(q, fmt, man.spc_list, d["bn"])
    rB, rhs, rhc = _ref_hashes(q, fmt, d)
    rcodes = R.chain(q, fmt, d["seed"], d["ts"], rB)
    # host-pointer entry points
    sn, cn = C.derive_nonces(g, man, d["bn"])
    assert np.array_equal(sn, rsn) and np.array_equal(cn, rcn)
    B, hs, hc = C.ballot_hashes(g, man, d["hashes"], d["ids"], d["cts"], parts=True)
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)
    assert np.array_equal(C.ballot_hashes(g, man, d["hashes"], d["ids"], d["cts"]), rB)
    assert C.verify_code_chain(g, d["seed"], d["ts"], B, rcodes).all()
    bad = rcodes.copy()
    bad[1, 31] ^= 1
    want = R.check(q, fmt, d["seed"], d["ts"], rB, bad)
    assert want.tolist() == [True, False, False]
    assert np.array_equal(C.verify_code_chain(g, d["seed"], d["ts"], B, bad), want)
    # device-pointer entry points
    dsn, dcn = C.derive_nonces(g, man, g.to_device(d["bn"]))
    assert np.array_equal(dsn.download(), rsn) and np.array_equal(dcn.download(), rcn)
    dB, dhs, dhc = C.ballot_hashes(g, man, d["hashes"], g.to_device(d["ids"]), g.to_device(d["cts"]), parts=True)
    assert np.array_equal(dhs.download(), rhs) and np.array_equal(dhc.download(), rhc)
    assert np.array_equal(dB.download(), rB)
    dB2 = C.ballot_hashes(g, man, d["hashes"], g.to_device(d["ids"]), g.to_device(d["cts"]))
    assert np.array_equal(dB2.download(), rB)
    dok = C.verify_code_chain(g, g.to_device(d["seed"]), g.to_device(d["ts"]), dB, g.to_device(bad))
    assert np.array_equal(dok.download().astype(bool), want)
    # the host mirrors agree as well
    assert np.array_equal(C.chain_codes(q, d["seed"], d["ts"], B, fmt=fmt), rcodes)


# ---------------------------------------------------------------------------------------------
# SHA-256 padding boundaries
# ---------------------------------------------------------------------------------------------
def test_fixed_width_contest_preimage_at_55_56_and_0(fmt_group):
    """fixed width: a contest pre-image is 65 spc + 66 = spc + 2 (mod 64) bytes long; spc 53, 54
    and 62 put it at 55 (the last length whose padding fits the block), 56 (the first that needs
    another block) and 0 (a whole number of blocks)."""
    from electionguard import codes as C
    g = fmt_group
    d = _data(_man([(52, 1), (53, 1), (61, 1)]), 2, 12)
    assert [(65 * int(s) + 66) % 64 for s in d["man"].spc_list] == [55, 56, 0]
    rB, rhs, rhc = _ref_hashes(g.q, "fixed", d)
    B, hs, hc = C.ballot_hashes(g, d["man"], d["hashes"], d["ids"], d["cts"], parts=True)
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)


@pytest.mark.parametrize("nc", [52, 53, 61])
def test_fixed_width_ballot_preimage_at_55_56_and_0(fmt_group, nc):
    """the ballot pre-image is 65 nc + 131 = nc + 3 (mod 64) bytes: hash-only manifests of nc
    one-selection contests"""
    from electionguard import codes as C
    g = fmt_group
    d = _data(_man([(1, 0)] * nc), 2, 13 + nc)
    assert (65 * nc + 131) % 64 == {52: 55, 53: 56, 61: 0}[nc]
    rB, rhs, rhc = _ref_hashes(g.q, "fixed", d)
    B, hs, hc = C.ballot_hashes(g, d["man"], d["hashes"], d["ids"], d["cts"], parts=True)
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)


def test_minimal_form_leading_zero_bytes_and_extreme_values(fmt_group):
    """minimal form: alpha / beta / Q rows with 0, 1, 15, 16, 17 and 511 (Q: 31) leading zero
    bytes, and the values 0, 1, p - 1 and 2^4096 - 1"""
    from electionguard import codes as C
    g = fmt_group
    g.hash_format = "minimal"
    lz = [0, 1, 15, 16, 17, 511]
    d = _data(_man([(5, 1), (3, 1)]), 2, 14)   # spc 6 (the leading-zero rows) and 4 (the values)
    cts, h = d["cts"], d["hashes"]
    cts[:, :, :, 0] |= 1    # no accidental leading zero, and a non-zero last byte everywhere
    cts[:, :, :, 511] |= 1
    for s, z in enumerate(lz):
        cts[0, s, 0, :z] = 0            # ballot 0: alpha
        cts[1, s, 1, :z] = 0            # ballot 1: beta
        h.dsel[s, :min(z, 31)] = 0
        h.dsel[s, 31] |= 1
    vals = [0, 1, g.p - 1, 2 ** 4096 - 1]
    for s, v in enumerate(vals):
        cts[0, 6 + s, 0] = np.frombuffer(int(v).to_bytes(512, "big"), np.uint8)
        cts[0, 6 + s, 1] = np.frombuffer(int(vals[3 - s]).to_bytes(512, "big"), np.uint8)
    h.dcon[0] = 0                       # Q value 0 -> "00"
    h.dcon[1, :31] = 0
    h.dcon[1, 31] = 1                   # Q value 1 -> "01"
    h.manifest_hash[:16] = 0
    d["ids"][0, :17] = 0
    d["ids"][1] = 0xFF                  # 2^256 - 1: above q, taken as given
    d["bn"][0, :15] = 0
    d["bn"][1] = 0
    d["seed"][:1] = 0
    q = g.q
    rB, rhs, rhc = _ref_hashes(q, "minimal", d)
    B, hs, hc = C.ballot_hashes(g, d["man"], h, d["ids"], cts, parts=True)
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)
    rsn, rcn = R.nonces(q, "minimal", d["man"].spc_list, d["bn"])
    sn, cn = C.derive_nonces(g, d["man"], d["bn"])
    assert np.array_equal(sn, rsn) and np.array_equal(cn, rcn)
    rcodes = R.chain(q, "minimal", d["seed"], d["ts"], rB)
    assert C.verify_code_chain(g, d["seed"], d["ts"], B, rcodes).all()
    # and the same rows in fixed width
    g.hash_format = "fixed"
    rB, rhs, rhc = _ref_hashes(q, "fixed", d)
    B, hs, hc = C.ballot_hashes(g, d["man"], h, d["ids"], cts, parts=True)
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)


# ---------------------------------------------------------------------------------------------
# grid tail and the empty batch
# ---------------------------------------------------------------------------------------------
def test_grid_tail_65_ballots_of_4_selections(fmt_group):
    """65 x 4 = 260 selection hashes and 65 x 18 = 1170 nonces: more than one 256-thread block,
    the last one partly filled"""
    from electionguard import codes as C
    g = fmt_group
    d = _data(_man((2, 1, 1)), 65, 15)
    assert d["man"].nsel == 4
    rsn, rcn = R.nonces(g.q, "fixed", d["man"].spc_list, d["bn"])
    sn, cn = C.derive_nonces(g, d["man"], d["bn"])
    assert np.array_equal(sn, rsn) and np.array_equal(cn, rcn)
    rB, rhs, rhc = _ref_hashes(g.q, "fixed", d)
    dB, dhs, dhc = C.ballot_hashes(g, d["man"], d["hashes"], g.to_device(d["ids"]), g.to_device(d["cts"]), parts=True)
    assert np.array_equal(dhs.download(), rhs) and np.array_equal(dhc.download(), rhc)
    assert np.array_equal(dB.download(), rB)
    codes = R.chain(g.q, "fixed", d["seed"], d["ts"], rB)
    assert C.verify_code_chain(g, d["seed"], d["ts"], rB, codes).all()


def test_no_ballots(fmt_group):
    from electionguard import codes as C
    g, lib = fmt_group, fmt_group._lib
    d = _data(_man(RAGGED), 0, 16)
    man = d["man"]
    sn, cn = C.derive_nonces(g, man, d["bn"])
    assert sn.shape == (0, man.nsel, 4, 32) and cn.shape == (0, 3, 32)
    assert C.ballot_hashes(g, man, d["hashes"], d["ids"], d["cts"]).shape == (0, 32)
    assert C.verify_code_chain(g, d["seed"], d["ts"].reshape(0, 32), np.zeros((0, 32), np.uint8),
                               np.zeros((0, 32), np.uint8)).shape == (0,)
    # EG_OK and nothing written, host and device variants, with every data pointer NULL
    spc = man.spc_list.ctypes.data_as(U32P)
    for name in ("eg_derive_ballot_nonces", "eg_derive_ballot_nonces_dev"):
        assert getattr(lib, name)(g.handle, 0, 3, spc, None, None, None) == 0, name
    for name in ("eg_ballot_hashes", "eg_ballot_hashes_dev"):
        assert getattr(lib, name)(g.handle, 0, 3, spc, None, None, None, None, None, None, None, None) == 0, name
    for name in ("eg_verify_code_chain", "eg_verify_code_chain_dev"):
        assert getattr(lib, name)(g.handle, 0, None, None, None, None, None) == 0, name
    out = np.full((2, 32), 0xA5, np.uint8)
    h = d["hashes"]
    assert lib.eg_ballot_hashes(g.handle, 0, 3, spc, _ptr(h.dsel), _ptr(h.dcon), _ptr(h.manifest_hash), _ptr(out),
                                _ptr(out), _ptr(out), _ptr(out), _ptr(out)) == 0
    assert (out == 0xA5).all()


# ---------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(fmt_group):
    g, lib = fmt_group, fmt_group._lib
    d = _data(_man(RAGGED), 2, 17)
    man, h, nb = d["man"], d["hashes"], 2
    good = man.spc_list.ctypes.data_as(U32P)
    err = lambda: lib.eg_last_error().decode()
    sent = lambda *shape: np.full(shape, 0xA5, np.uint8)
    sn, cn, B = sent(nb, man.nsel, 4, 32), sent(nb, 3, 32), sent(nb, 32)
    hs, hc, ok = sent(nb, man.nsel, 32), sent(nb, 3, 32), sent(nb)
    untouched = lambda: all((a == 0xA5).all() for a in (sn, cn, B, hs, hc, ok))

    def derive(spc=good, nc=3, bn=_ptr(d["bn"]), o1=_ptr(sn), o2=_ptr(cn), handle=g.handle):
        return lib.eg_derive_ballot_nonces(handle, nb, nc, spc, bn, o1, o2)

    def hashes(spc=good, nc=3, dsel=_ptr(h.dsel), dcon=_ptr(h.dcon), mh=_ptr(h.manifest_hash), ids=_ptr(d["ids"]),
               cts=_ptr(d["cts"]), oB=_ptr(B)):
        return lib.eg_ballot_hashes(g.handle, nb, nc, spc, dsel, dcon, mh, ids, cts, oB, _ptr(hs), _ptr(hc))

    def chain(seed=_ptr(d["seed"]), ts=_ptr(d["ts"]), b=_ptr(d["ids"]), codes=_ptr(d["bn"]), o=_ptr(ok)):
        return lib.eg_verify_code_chain(g.handle, nb, seed, ts, b, codes, o)

    # NULL required pointers
    for call, names in ((derive, ("spc", "bn", "o1", "o2", "handle")),
                        (hashes, ("spc", "dsel", "dcon", "mh", "ids", "cts", "oB")),
                        (chain, ("seed", "ts", "b", "codes", "o"))):
        for name in names:
            assert call(**{name: None}) == 1 and "null" in err(), (call.__name__, name)
    # bad shapes: no contests, an empty contest, more than 2^20 selections per ballot
    empty = np.array([3, 0, 6], np.uint32).ctypes.data_as(U32P)
    huge_a = np.full(3, 2 ** 19, np.uint32)
    huge = huge_a.ctypes.data_as(U32P)
    for call in (derive, hashes):
        assert call(nc=0) == 1 and "manifest" in err() and "no contests" in err()
        assert call(spc=empty) == 1 and "manifest" in err() and "contest 1" in err()
        assert call(spc=huge) == 1 and "manifest" in err() and "2^20" in err()
    assert untouched()
    # the same through the _dev variants, and a device pointer that is not 16-byte aligned
    z = lambda *shape: g.device_zeros(shape)
    d_bn, d_ids, d_cts, d_ts = g.to_device(d["bn"]), g.to_device(d["ids"]), g.to_device(d["cts"]), g.to_device(d["ts"])
    d_desc = g.to_device(np.concatenate([h.dsel.reshape(-1), h.dcon.reshape(-1), h.manifest_hash]))
    d_seed = g.to_device(np.concatenate([d["seed"], d["seed"]]))   # room for a misaligned 32-byte read
    d_sn, d_cn, d_B, d_hs, d_hc, d_ok = z(nb + 1, man.nsel, 4, 32), z(nb + 1, 3, 32), z(nb + 1, 32), \
        z(nb + 1, man.nsel, 32), z(nb + 1, 3, 32), z(nb + 16)
    dsel_p, dcon_p, mh_p = d_desc.ptr, d_desc.ptr + man.nsel * 32, d_desc.ptr + (man.nsel + 3) * 32

    def derive_dev(spc=good, nc=3, bn=d_bn.ptr, o1=d_sn.ptr, o2=d_cn.ptr):
        return lib.eg_derive_ballot_nonces_dev(g.handle, nb, nc, spc, bn, o1, o2)

    def hashes_dev(spc=good, nc=3, dsel=dsel_p, dcon=dcon_p, mh=mh_p, ids=d_ids.ptr, cts=d_cts.ptr, oB=d_B.ptr,
                   ohs=d_hs.ptr, ohc=d_hc.ptr):
        return lib.eg_ballot_hashes_dev(g.handle, nb, nc, spc, dsel, dcon, mh, ids, cts, oB, ohs, ohc)

    def chain_dev(seed=d_seed.ptr, ts=d_ts.ptr, b=d_ids.ptr, codes=d_bn.ptr, o=d_ok.ptr):
        return lib.eg_verify_code_chain_dev(g.handle, nb, seed, ts, b, codes, o)

    for call, names in ((derive_dev, ("spc", "bn", "o1", "o2")),
                        (hashes_dev, ("spc", "dsel", "dcon", "mh", "ids", "cts", "oB")),
                        (chain_dev, ("seed", "ts", "b", "codes", "o"))):
        for name in names:
            assert call(**{name: None}) == 1 and "null" in err(), (call.__name__, name)
    for call in (derive_dev, hashes_dev):
        assert call(nc=0) == 1 and "manifest" in err()
        assert call(spc=empty) == 1 and "manifest" in err()
        assert call(spc=huge) == 1 and "manifest" in err()
    for call, ptrs in ((derive_dev, dict(bn=d_bn.ptr, o1=d_sn.ptr, o2=d_cn.ptr)),
                       (hashes_dev, dict(dsel=dsel_p, dcon=dcon_p, mh=mh_p, ids=d_ids.ptr, cts=d_cts.ptr, oB=d_B.ptr,
                                         ohs=d_hs.ptr, ohc=d_hc.ptr)),
                       (chain_dev, dict(seed=d_seed.ptr, ts=d_ts.ptr, b=d_ids.ptr, codes=d_bn.ptr))):
        for name, p in ptrs.items():
            for off in (4, 8):
                assert call(**{name: p + off}) == 1 and "aligned" in err(), (call.__name__, name, off)
    g.sync()
    for buf in (d_sn, d_cn, d_B, d_hs, d_hc, d_ok):
        assert not buf.download().any()
    # the optional outputs may be NULL, and the ok flags need no alignment
    assert hashes_dev(ohs=None, ohc=None) == 0
    assert chain_dev(o=d_ok.ptr + 1) == 0
    g.sync()
    assert np.array_equal(d_B.download()[:nb], _ref_hashes(g.q, "fixed", d)[0])
    assert not d_hs.download().any() and not d_hc.download().any()


# ---------------------------------------------------------------------------------------------
# chain tampering
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain5(group):
    from electionguard import codes as C
    d = _data(_man((2, 2, 1)), 5, 18)
    B = C.ballot_hashes(group, d["man"], d["hashes"], d["ids"], d["cts"])
    d["B"] = B
    d["codes"] = C.chain_codes(group.q, d["seed"], d["ts"], B)
    return d


def _failed(ok):
    return np.flatnonzero(~ok).tolist()


def test_chain_tampering(group, chain5):
    from electionguard import codes as C
    d, g = chain5, group
    man, h = d["man"], d["hashes"]
    verify = lambda B, codes, seed=d["seed"]: C.verify_code_chain(g, seed, d["ts"], B, codes)
    assert np.array_equal(d["codes"], R.chain(g.q, "fixed", d["seed"], d["ts"], d["B"]))
    assert verify(d["B"], d["codes"]).tolist() == [True] * 5
    # one ciphertext byte of ballot 2
    cts = d["cts"].copy()
    cts[2, 3, 1, 100] ^= 0x04
    B = C.ballot_hashes(g, man, h, d["ids"], cts)
    assert _failed((B == d["B"]).all(axis=1)) == [2]
    assert _failed(verify(B, d["codes"])) == [2]
    # a recorded code altered: its own link and the next one
    codes = d["codes"].copy()
    codes[2, 0] ^= 0x01
    assert _failed(verify(d["B"], codes)) == [2, 3]
    # ballots 1 and 3 swapped
    order = [0, 3, 2, 1, 4]
    B = C.ballot_hashes(g, man, h, d["ids"][order], d["cts"][order])
    bad = _failed(verify(B, d["codes"]))
    assert 1 in bad and 3 in bad
    # a wrong seed
    seed = d["seed"].copy()
    seed[31] ^= 1
    assert _failed(verify(d["B"], d["codes"], seed)) == [0]


# ---------------------------------------------------------------------------------------------
# chunk crossing of the host-pointer variants
# ---------------------------------------------------------------------------------------------
def test_host_variants_one_ballot_more_than_a_chunk(fmt_group):
    """16,385 ballots of one selection: the host variants stage 16,384-ballot chunks, so the last
    ballot is a chunk of its own.  Against hashlib on both sides of the boundary, and against the
    device variants (one launch / chunks of device pointers) over the whole batch."""
    from electionguard import codes as C
    g = fmt_group
    nb = 16385
    d = _data(_man([(1, 0)]), nb, 19)
    man, h = d["man"], d["hashes"]
    assert man.nsel == 1 and d["cts"].nbytes == nb * 1024
    edge = [0, 16383, 16384, nb - 1]
    sn, cn = C.derive_nonces(g, man, d["bn"])
    B, hs, hc = C.ballot_hashes(g, man, h, d["ids"], d["cts"], parts=True)
    B2 = C.ballot_hashes(g, man, h, d["ids"], d["cts"])
    rsn, rcn = R.nonces(g.q, "fixed", man.spc_list, d["bn"][edge])
    assert np.array_equal(sn[edge], rsn) and np.array_equal(cn[edge], rcn)
    rB, rhs, rhc = R.hashes(g.q, "fixed", man.spc_list, h.dsel, h.dcon, h.manifest_hash, d["ids"][edge], d["cts"][edge])
    assert np.array_equal(B[edge], rB) and np.array_equal(hs[edge], rhs) and np.array_equal(hc[edge], rhc)
    assert np.array_equal(B2, B)
    dsn, dcn = C.derive_nonces(g, man, g.to_device(d["bn"]))
    assert np.array_equal(dsn.download(), sn) and np.array_equal(dcn.download(), cn)
    d_ids, d_cts = g.to_device(d["ids"]), g.to_device(d["cts"])
    dB, dhs, dhc = C.ballot_hashes(g, man, h, d_ids, d_cts, parts=True)
    assert np.array_equal(dB.download(), B) and np.array_equal(dhs.download(), hs)
    assert np.array_equal(dhc.download(), hc)
    assert np.array_equal(C.ballot_hashes(g, man, h, d_ids, d_cts).download(), B)
