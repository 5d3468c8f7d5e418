"""GPU: contest data under HashedElGamal (include/eg_hip_contestdata.h, electionguard.contest_data,
csrc/eg_hmac.hpp) against the restatement on hashlib, hmac and CPython pow of contest_data_ref.py,
byte for byte; opening through the seed and through the trustees; the record's public check."""
import copy
import ctypes

import numpy as np
import pytest

import contest_data_ref as R

pytestmark = pytest.mark.gpu

FORMATS = ("fixed", "minimal")
NB, NC = 3, 2
# 512 + nbytes bytes of MAC input: 55, 56, 63, 64 sit on every SHA-256 padding edge; 31, 32, 33 put
# the stream on a block edge (and 1, 31, 33, 55, 63, 65, 119 take the byte path, the others the
# word path); 1024 is the cap
SIZES = [1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 1024]
QBAR = 0xC0DA7A


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@pytest.fixture
def fmt_group(group):
    try:
        yield group
    finally:
        group.hash_format = "fixed"


@pytest.fixture(scope="module")
def ceremony(group):
    from electionguard.ballot import ElectionKey
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=77)
    return gk, K, ElectionKey(group, K)


@pytest.fixture(scope="module")
def small(group, ceremony):
    """3 ballots x 2 contests: nonces, c0 and kappa from the reference (CPython pow), computed once"""
    _, K, _ = ceremony
    bn, ids = _rand(1, NB, 32), _rand(2, NB, 32)
    r = R.nonces(group.q, "fixed", NC, bn).reshape(-1, 32)
    es = [int.from_bytes(bytes(x), "big") for x in r]
    c0 = np.stack([np.frombuffer(pow(group.g, e, group.p).to_bytes(512, "big"), np.uint8) for e in es])
    kappa = np.stack([np.frombuffer(pow(K, e, group.p).to_bytes(512, "big"), np.uint8) for e in es])
    return dict(bn=bn, ids=ids, r=r, c0=c0, kappa=kappa)


def _seal_dev(group, key, nc, nbytes, ids, r, data):
    from electionguard import contest_data as CD
    out = CD.seal(group, key, nc, nbytes, group.to_device(ids), group.to_device(r), group.to_device(data))
    return [x.download() for x in out]


# ---------------------------------------------------------------------------------------------
# parity with the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_nonces_under_both_hash_formats(fmt_group, fmt):
    from electionguard import contest_data as CD
    g = fmt_group
    g.hash_format = fmt
    bn = _rand(3, 5, 32)
    bn[2, :19] = 0   # leading zero bytes: the two formats hash different strings
    want = R.nonces(g.q, fmt, 3, bn)
    assert np.array_equal(CD.derive_nonces(g, 3, bn), want)
    assert np.array_equal(CD.derive_nonces(g, 3, g.to_device(bn)).download(), want)
    assert np.array_equal(CD.derive_nonces_host(g.q, 3, bn, fmt=fmt), want)


@pytest.mark.parametrize("nbytes", SIZES)
def test_seal_is_byte_exact(group, ceremony, small, nbytes):
    from electionguard import contest_data as CD
    key, d = ceremony[2], small
    data = _rand(100 + nbytes, NB * NC, nbytes)
    rc1, rc2 = R.seal_with_kappa(NC, d["ids"], d["c0"], d["kappa"], data)
    c0, c1, c2 = CD.seal(group, key, NC, nbytes, d["ids"], d["r"], data)
    assert c1.shape == (NB * NC, nbytes)
    assert np.array_equal(c0, d["c0"]) and np.array_equal(c1, rc1) and np.array_equal(c2, rc2)
    # the device-pointer variant agrees
    dc0, dc1, dc2 = _seal_dev(group, key, NC, nbytes, d["ids"], d["r"], data)
    assert np.array_equal(dc0, c0) and np.array_equal(dc1, c1) and np.array_equal(dc2, c2)


def test_seal_is_the_same_in_constant_time_mode(group, ceremony, small):
    from electionguard import contest_data as CD
    key, d = ceremony[2], small
    data = _rand(7, NB * NC, 33)
    want = CD.seal(group, key, NC, 33, d["ids"], d["r"], data)
    group.ct_pow = True
    try:
        got = CD.seal(group, key, NC, 33, d["ids"], d["r"], data)
    finally:
        group.ct_pow = False
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(got[0], d["c0"])


def _check_against_the_batch_calls(group, key, nb, nc, nbytes, seed, dev):
    """The exponent half against gPowP_batch and FixedBase.pow_batch, the hash half against the
    reference fed those kappa (a CPython pow per item would take minutes)."""
    from electionguard import contest_data as CD
    from electionguard.core.group import FixedBase
    n = nb * nc
    ids, bn, data = _rand(seed, nb, 32), _rand(seed + 1, nb, 32), _rand(seed + 2, n, nbytes)
    r = CD.derive_nonces(group, nc, bn).reshape(-1, 32)
    if dev:
        c0, c1, c2 = _seal_dev(group, key, nc, nbytes, ids, r, data)
    else:
        c0, c1, c2 = CD.seal(group, key, nc, nbytes, ids, r, data)
    assert np.array_equal(c0, group.gPowP_batch(r))
    ktab = FixedBase(group, key.K, key.window_bits)
    try:
        kappa = ktab.pow_batch(r)
    finally:
        ktab.close()
    rc1, rc2 = R.seal_with_kappa(nc, ids, c0, kappa, data)
    assert np.array_equal(c1, rc1) and np.array_equal(c2, rc2)
    return ids, c0, kappa, c1, c2, data


@pytest.mark.parametrize("nb,nc", [(85, 3), (64, 4), (257, 1)], ids=["255", "256", "257"])
def test_thread_block_edge(group, ceremony, nb, nc):
    from electionguard import contest_data as CD
    ids, c0, kappa, c1, c2, data = _check_against_the_batch_calls(group, ceremony[2], nb, nc, 33, 40 + nc, dev=True)
    got, ok = CD.open_sealed(group, nc, 33, ids, c0, kappa, c1, c2)
    assert ok.all() and np.array_equal(got, data)


def test_host_variant_crosses_a_staging_chunk_by_one_ballot(group, ceremony):
    from electionguard import contest_data as CD
    nb = 16384 + 1   # the verifier's chunk is 16,384 ballots
    ids, c0, kappa, c1, c2, data = _check_against_the_batch_calls(group, ceremony[2], nb, 1, 1, 50, dev=False)
    bn = _rand(51, nb, 32)
    assert np.array_equal(CD.derive_nonces(group, 1, bn), R.nonces(group.q, "fixed", 1, bn))
    got, ok = CD.open_sealed(group, 1, 1, ids, c0, kappa, c1, c2)
    assert ok.all() and np.array_equal(got, data)


# ---------------------------------------------------------------------------------------------
# open
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [33, 64])
def test_open_round_trips_and_one_flipped_bit_fails_its_item_alone(group, small, nbytes):
    from electionguard import contest_data as CD
    d = small
    n = NB * NC
    data = _rand(60 + nbytes, n, nbytes)
    c1, c2 = R.seal_with_kappa(NC, d["ids"], d["c0"], d["kappa"], data)
    base = dict(ids=d["ids"], c0=d["c0"], kappa=d["kappa"], c1=c1, c2=c2)

    def run(args, dev):
        order = ("ids", "c0", "kappa", "c1", "c2")
        if dev:
            got, ok = CD.open_sealed(group, NC, nbytes, *[group.to_device(args[k]) for k in order])
            return got.download(), ok.download().astype(bool)
        return CD.open_sealed(group, NC, nbytes, *[args[k] for k in order])

    for dev in (False, True):
        got, ok = run(base, dev)
        assert ok.all() and np.array_equal(got, data)
    item = 3   # ballot 1, contest 1
    flips = {"c0": (item, 17, 0x01), "c1": (item, nbytes - 1, 0x80), "c2": (item, 31, 0x04),
             "kappa": (item, 511, 0x10), "ids": (item // NC, 5, 0x02)}
    for name, (row, col, bit) in flips.items():
        args = dict(base)
        args[name] = base[name].copy()
        args[name][row, col] ^= bit
        # a ballot id is shared by the ballot's contests: flipping it fails both of them
        hit = [row * NC + k for k in range(NC)] if name == "ids" else [row]
        want_ok = np.array([i not in hit for i in range(n)])
        rgot, rok = R.open_all(NC, args["ids"], args["c0"], args["kappa"], args["c1"], args["c2"])
        assert rok.tolist() == want_ok.tolist(), name
        for dev in (False, True):
            got, ok = run(args, dev)
            assert ok.tolist() == want_ok.tolist(), (name, dev)
            assert not got[~want_ok].any(), (name, dev)                      # the failed rows are zeroed
            assert np.array_equal(got[want_ok], data[want_ok]), (name, dev)  # the others are intact
            assert np.array_equal(got, rgot), (name, dev)


# ---------------------------------------------------------------------------------------------
# the C ABI's edges
# ---------------------------------------------------------------------------------------------
def test_no_ballots_writes_nothing(group, ceremony):
    lib, h, K = group._lib, group.handle, ceremony[2].K_be
    fill = lambda n: np.full(n, 0xA5, np.uint8)
    a, b, c, d = fill(64), fill(1024), fill(64), fill(64)
    assert lib.eg_derive_contest_data_nonces(h, 0, 2, _ptr(a), _ptr(c)) == 0
    assert lib.eg_seal_contest_data(h, K, 0, 2, 32, _ptr(a), _ptr(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d)) == 0
    assert lib.eg_open_contest_data(h, 0, 2, 32, _ptr(a), _ptr(b), _ptr(b), _ptr(a), _ptr(a), _ptr(c), _ptr(d)) == 0
    assert all((x == 0xA5).all() for x in (a, b, c, d))
    dev = group.to_device(fill(2048))
    p = dev.ptr
    assert lib.eg_derive_contest_data_nonces_dev(h, 0, 2, p, p + 64) == 0
    assert lib.eg_seal_contest_data_dev(h, K, 0, 2, 32, p, p, p, p + 512, p, p) == 0
    assert lib.eg_open_contest_data_dev(h, 0, 2, 32, p, p, p + 512, p, p, p + 1024, p) == 0
    # null data pointers are fine when there is nothing to do
    assert lib.eg_seal_contest_data(h, K, 0, 2, 32, None, None, None, None, None, None) == 0
    group.sync()
    assert (dev.download() == 0xA5).all()


def test_argument_errors(group, ceremony):
    lib, h, K = group._lib, group.handle, ceremony[2].K_be
    ERR = 1   # EG_ERR_ARG
    buf = group.device_zeros(8192)
    p = buf.ptr
    host = np.zeros(4096, np.uint8)
    hp = _ptr(host)
    seal_h = lambda *a: lib.eg_seal_contest_data(h, *a)
    seal_d = lambda *a: lib.eg_seal_contest_data_dev(h, *a)
    open_h = lambda *a: lib.eg_open_contest_data(h, *a)
    open_d = lambda *a: lib.eg_open_contest_data_dev(h, *a)
    good_seal_h = [K, 1, 2, 8, hp, hp, hp, hp, hp, hp]
    good_seal_d = [K, 1, 2, 8, p, p + 64, p + 128, p + 1024, p + 2048, p + 2304]
    good_open_h = [1, 2, 8, hp, hp, hp, hp, hp, hp, hp]
    good_open_d = [1, 2, 8, p, p + 1024, p + 2048, p + 3072, p + 3200, p + 3328, p + 3456]

    def swapped(args, i, v):
        out = list(args)
        out[i] = v
        return out

    # a NULL required pointer, every position
    assert lib.eg_derive_contest_data_nonces(h, 1, 2, None, hp) == ERR
    assert lib.eg_derive_contest_data_nonces(h, 1, 2, hp, None) == ERR
    assert lib.eg_derive_contest_data_nonces_dev(h, 1, 2, None, p) == ERR
    assert lib.eg_derive_contest_data_nonces_dev(h, 1, 2, p, None) == ERR
    for i in (0, 4, 5, 6, 7, 8, 9):
        assert seal_h(*swapped(good_seal_h, i, None)) == ERR, i
        assert seal_d(*swapped(good_seal_d, i, None)) == ERR, i
    for i in range(3, 10):
        assert open_h(*swapped(good_open_h, i, None)) == ERR, i
        assert open_d(*swapped(good_open_d, i, None)) == ERR, i
    assert b"null" in lib.eg_last_error()
    # ncontest == 0
    assert lib.eg_derive_contest_data_nonces(h, 1, 0, hp, hp) == ERR
    assert lib.eg_derive_contest_data_nonces_dev(h, 1, 0, p, p) == ERR
    assert seal_h(*swapped(good_seal_h, 2, 0)) == ERR and seal_d(*swapped(good_seal_d, 2, 0)) == ERR
    assert open_h(*swapped(good_open_h, 1, 0)) == ERR and open_d(*swapped(good_open_d, 1, 0)) == ERR
    assert b"ncontest" in lib.eg_last_error()
    # nbytes outside [1, 1024]
    for bad in (0, 1025):
        assert seal_h(*swapped(good_seal_h, 3, bad)) == ERR and seal_d(*swapped(good_seal_d, 3, bad)) == ERR
        assert open_h(*swapped(good_open_h, 2, bad)) == ERR and open_d(*swapped(good_open_d, 2, bad)) == ERR
        assert b"nbytes" in lib.eg_last_error()
    # a _dev pointer to 512-byte rows that is not 16-byte aligned: c0 of a seal, c0 and kappa of an open
    assert seal_d(*swapped(good_seal_d, 7, p + 1024 + 8)) == ERR
    assert b"aligned" in lib.eg_last_error()
    assert open_d(*swapped(good_open_d, 4, p + 1024 + 4)) == ERR
    assert open_d(*swapped(good_open_d, 5, p + 2048 + 1)) == ERR
    assert b"aligned" in lib.eg_last_error()
    # nothing ran: the buffer is as it was
    group.sync()
    assert not buf.download().any()


def test_c1_and_data_rows_need_no_alignment(group, ceremony, small):
    """the _dev variants on c1 / data rows at an odd address, nbytes a multiple of 4: the kernels
    must take the byte path there"""
    lib, h, key, d = group._lib, group.handle, ceremony[2], small
    nbytes, n = 32, NB * NC
    data = _rand(70, n, nbytes)
    rc1, rc2 = R.seal_with_kappa(NC, d["ids"], d["c0"], d["kappa"], data)
    ids, r = group.to_device(d["ids"]), group.to_device(d["r"])
    din = group.device_zeros(n * nbytes + 16)
    lib.eg_memcpy_htod(h, din.ptr + 1, _ptr(data), data.nbytes)
    c0, c2, c1 = group.device_empty((n, 512)), group.device_empty((n, 32)), group.device_zeros(n * nbytes + 16)
    assert lib.eg_seal_contest_data_dev(h, key.K_be, NB, NC, nbytes, ids.ptr, r.ptr, din.ptr + 1, c0.ptr, c1.ptr + 3,
                                        c2.ptr) == 0
    raw = c1.download()
    assert np.array_equal(raw[3:3 + n * nbytes].reshape(n, nbytes), rc1) and not raw[:3].any() and not raw[-13:].any()
    assert np.array_equal(c2.download(), rc2) and np.array_equal(c0.download(), d["c0"])
    out, ok, kappa = group.device_zeros(n * nbytes + 16), group.device_zeros(n), group.to_device(d["kappa"])
    assert lib.eg_open_contest_data_dev(h, NB, NC, nbytes, ids.ptr, c0.ptr, kappa.ptr, c1.ptr + 3, c2.ptr, out.ptr + 5,
                                        ok.ptr) == 0
    raw = out.download()
    assert ok.download().all() and np.array_equal(raw[5:5 + n * nbytes].reshape(n, nbytes), data)
    assert not raw[:5].any() and not raw[-11:].any()


# ---------------------------------------------------------------------------------------------
# from the ballot nonces, through the trustees, in the record
# ---------------------------------------------------------------------------------------------
WRITE_INS = [[("Ada Lovelace",), ()], [("Zoë", "王小明"), ("a name that is far too long for forty bytes of room",)]]


@pytest.fixture(scope="module")
def spoiled(group, ceremony):
    """2 ballots x 2 contests of packed ContestData, sealed once from their ballot nonces"""
    from electionguard import contest_data as CD
    from electionguard.ballot import Manifest
    man = Manifest(2, 2, 1)
    cds = [[CD.ContestData(CD.NORMAL if w else CD.UNDER_VOTE, [] if w else [1], list(w)) for w in row]
           for row in WRITE_INS]
    bn, ids = _rand(80, 2, 32), _rand(81, 2, 32)
    data = CD.pack_ballots(cds, 40)
    sealed = CD.seal_contest_data_seeded(group, ceremony[2], man, bn, ids, data)
    return dict(man=man, cds=cds, bn=bn, ids=ids, data=data, sealed=sealed)


def test_seeded_seal_equals_the_host_mirror_and_opens_from_the_seed(group, ceremony, spoiled):
    from electionguard import contest_data as CD
    (_, K, key), d = ceremony, spoiled
    s = d["sealed"]
    assert s.c0.shape == (2, 2, 512) and s.c1.shape == (2, 2, 40) and s.c2.shape == (2, 2, 32) and s.num_bytes == 40
    c0, c1, c2 = CD.seal_contest_data_host(group.p, group.q, group.g, K, 2, d["bn"], d["ids"], d["data"])
    assert np.array_equal(s.c0.reshape(-1, 512), c0) and np.array_equal(s.c1.reshape(-1, 40), c1)
    assert np.array_equal(s.c2.reshape(-1, 32), c2)
    got, ok = CD.open_contest_data_seeded(group, key, d["man"], s, d["bn"], d["ids"])
    assert ok.shape == (2, 2) and ok.all() and np.array_equal(got, d["data"])
    back = [[CD.ContestData.unpack(got[b, k]) for k in range(2)] for b in range(2)]
    assert back[0] == d["cds"][0] and back[1][0] == d["cds"][1][0]
    assert back[1][1] == CD.ContestData(CD.NORMAL | CD.TRUNCATED, [], [])   # the long name was dropped whole
    # an item whose c0 is not g^r
    bad = copy.copy(s)
    bad.c0 = s.c0.copy()
    bad.c0[1, 0] = s.c0[0, 0]
    got, ok = CD.open_contest_data_seeded(group, key, d["man"], bad, d["bn"], d["ids"])
    assert ok.tolist() == [[True, True], [False, True]] and not got[1, 0].any()
    assert np.array_equal(got[0], d["data"][0]) and np.array_equal(got[1, 1], d["data"][1, 1])
    # another ballot's seed opens nothing of this one
    bn = d["bn"].copy()
    bn[0, 3] ^= 1
    got, ok = CD.open_contest_data_seeded(group, key, d["man"], s, bn, d["ids"])
    assert ok.tolist() == [[False, False], [True, True]] and not got[0].any()


@pytest.fixture(scope="module")
def trustees(group, ceremony):
    from electionguard.decrypt import DecryptingTrustee, Decryption
    gk, _, _ = ceremony
    comm = {g.gid: g.commitments for g in gk}
    avail = [DecryptingTrustee(group, g, comm) for g in gk[:2]]   # 3 guardians, quorum 2, one missing
    return avail, Decryption(group, QBAR, avail, [gk[2].gid], {g.gid: g.public_key for g in gk})


def test_trustees_open_the_contest_data_of_spoiled_ballots(group, spoiled, trustees):
    from electionguard import contest_data as CD
    d, (_, dec) = spoiled, trustees
    s = d["sealed"]
    got, ok = dec.decryptContestData(s.c0, s.c1, s.c2, d["ids"], 2)
    assert ok.shape == (2, 2) and ok.all() and np.array_equal(got, d["data"])
    assert CD.ContestData.unpack(got[1, 0]).write_ins == ["Zoë", "王小明"]
    assert CD.ContestData.unpack(got[0, 1]) == CD.ContestData(CD.UNDER_VOTE, [1], [])
    # a tampered c2 fails that item alone
    c2 = s.c2.copy()
    c2[0, 1, 0] ^= 1
    got, ok = dec.decryptContestData(s.c0, s.c1, c2, d["ids"], 2)
    assert ok.tolist() == [[True, False], [True, True]] and not got[0, 1].any()
    keep = np.array([[True, False], [True, True]])
    assert np.array_equal(got[keep], d["data"][keep])


def test_a_tampered_share_raises(group, spoiled, trustees):
    from electionguard.decrypt import Decryption, ShareBatch
    d, (avail, dec) = spoiled, trustees
    s = d["sealed"]

    class Tampering:
        """the first trustee, with one byte of one direct share changed"""
        def __init__(self, inner):
            self._t = inner

        def __getattr__(self, name):
            return getattr(self._t, name)

        def directDecrypt(self, group, texts, qbar, nonce=None):
            res = self._t.directDecrypt(group, texts, qbar, nonce)
            M = res.M.copy()
            M[2, 400] ^= 1
            return ShareBatch(M, res.proofs)

    bad = Decryption(group, QBAR, [Tampering(avail[0]), avail[1]], dec.missing, dec.public_keys)
    with pytest.raises(ValueError, match="invalid direct decryption proof"):
        bad.decryptContestData(s.c0, s.c1, s.c2, d["ids"], 2)


def test_record_check_on_public_data(group, ceremony, spoiled, trustees):
    from electionguard.ballot import Verifier, batch_encryption, random_scalars, random_votes
    from electionguard.record import ElectionRecord, GuardianRecord, verify_election_record
    (gk, K, key), d, (_, dec) = ceremony, spoiled, trustees
    man, s = d["man"], d["sealed"]
    rng = np.random.default_rng(90)
    eb = batch_encryption(group, key, QBAR, man, random_votes(rng, man, 2), random_scalars(rng, (2, man.nsel, 4), group.q),
                          random_scalars(rng, (2, man.n_contests), group.q))
    _, _, tally = Verifier(group, key, QBAR, man).verify(eb)
    guardians = [GuardianRecord(g.gid, g.x, list(g.commitments), list(g.proofs)) for g in gk]
    rec = ElectionRecord(man, QBAR, K, guardians, eb, tally, dec.decrypt_record(tally, 2))
    base = verify_election_record(group, rec)
    assert all(base.values()) and "contest_data" not in base, base
    res = verify_election_record(group, rec, contest_data=s)
    assert sorted(res) == sorted(list(base) + ["contest_data"]) and all(res.values()), res

    def failing(**changes):
        bad = copy.copy(s)
        for k, v in changes.items():
            setattr(bad, k, v)
        out = verify_election_record(group, rec, contest_data=bad)
        return sorted(k for k, v in out.items() if not v)

    # c0 (p - 1): still below p, but of order 2q
    c0 = s.c0.copy()
    x = int.from_bytes(bytes(c0[1, 1]), "big") * (group.p - 1) % group.p
    c0[1, 1] = np.frombuffer(x.to_bytes(512, "big"), np.uint8)
    assert failing(c0=c0) == ["contest_data"]
    # outside [1, p)
    for v in (0, group.p, 2**4096 - 1):
        c0 = s.c0.copy()
        c0[0, 0] = np.frombuffer(v.to_bytes(512, "big"), np.uint8)
        assert failing(c0=c0) == ["contest_data"], hex(v)[:12]
    # len(c1) != numBytes, and a contest without its ciphertext
    assert failing(num_bytes=41) == ["contest_data"]
    assert failing(c1=s.c1[:, :, :39]) == ["contest_data"]
    assert failing(c0=s.c0[:, :1], c1=s.c1[:, :1], c2=s.c2[:, :1]) == ["contest_data"]
