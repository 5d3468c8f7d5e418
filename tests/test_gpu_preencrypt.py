"""GPU: pre-encrypted ballots (include/eg_hip_preencrypt.h, electionguard.preencrypt) against the
reference of tests/preencrypt_ref.py frozen in tests/golden/Mode4096/preencrypt.json, the existing
fixed-base / multiply batches and the host mirror: parity in both hash formats, partial last
blocks, short codes, a chunk crossing, recording, tampering, constant-time mode, argument errors,
the election-record hook and the host variants' chunk crossings."""
import copy
import ctypes
import json

import numpy as np
import pytest

import preencrypt_ref as ref
from preencrypt_ref import b2i, sha

pytestmark = pytest.mark.gpu

QBAR = 0x5EED0F


@pytest.fixture(scope="module")
def env(group):
    from electionguard import preencrypt as pe
    from electionguard.ballot import ElectionKey, ElectionManifest
    from electionguard.codes import ManifestHashes
    fx = json.loads(ref.FIXTURE.read_text())
    K, dcon, mh, ids, bn, votes = ref.fixture_inputs(fx)
    man = ElectionManifest([tuple(c) for c in fx["manifest"]])
    hashes = ManifestHashes(np.zeros((man.nsel, 32), np.uint8), dcon, mh)
    return pe, fx, ElectionKey(group, K), man, hashes, ids, bn, votes


@pytest.fixture(scope="module")
def recorded(group, env):
    """The fixture's ballots pre-encrypted and recorded on the GPU (fixed format, 2-byte codes)."""
    pe, fx, key, man, hashes, ids, bn, votes = env
    pre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2, with_cts=True)
    rec = pe.record_ballots(group, key, QBAR, man, hashes, bn, votes, pre.sorted, 2)
    return pre, rec


def rows32(hexes, shape):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), np.uint8).reshape(shape)


PRE_FIELDS = ("sorted", "perm", "codes", "unique", "conf", "chash")
REC_FIELDS = ("sel_vecs", "sel_rank", "sel_codes", "ok", "sel_nonces", "contest_nonces")


def same(a, b, fields):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields)


# ---------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_parity_with_the_reference_and_between_the_variants(group, env, fmt):
    pe, fx, key, man, hashes, ids, bn, _ = env
    f = fx[fmt]
    group.hash_format = fmt
    try:
        pre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2, with_cts=True)
        dev = pe.preencrypt_ballots(group, key, man, hashes, group.to_device(ids), group.to_device(bn), 2,
                                    with_cts=True)
        lean = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2)
    finally:
        group.hash_format = "fixed"
    assert sha(pre.vec_cts) == f["vec_cts_sha256"]
    assert np.array_equal(pre.sorted, rows32(f["sorted"], (5, 10, 32)))
    assert pre.perm.reshape(-1).tolist() == f["perm"]
    assert pre.codes.reshape(-1).tolist() == f["codes2"]
    assert pre.unique.tolist() == f["unique"]["2"]
    assert np.array_equal(pre.chash, rows32(f["chash"], (5, 3, 32)))
    assert np.array_equal(pre.conf, rows32(f["conf"], (5, 32)))
    for name in PRE_FIELDS + ("vec_cts",):
        assert np.array_equal(getattr(dev, name).download(), getattr(pre, name)), name
    assert lean.vec_cts is None and same(lean, pre, PRE_FIELDS)


# ---------------------------------------------------------------------------------------------
# partial last blocks
# ---------------------------------------------------------------------------------------------
def test_86_ballots_end_every_kernel_on_a_partial_block(group, env):
    """3,268 components, 860 vectors, 258 contests; recording: 1,290 chosen components, 344 chosen
    vectors.  Ciphertexts against the fixed-base and multiply batches, hashes / order / codes
    against the host mirror over the GPU's ciphertexts, recording against the pre-encryption."""
    from electionguard.ballot import Verifier, random_votes
    from electionguard.core.group import FixedBase
    pe, fx, key, man, hashes, _, _, _ = env
    sh = pe.pre_shape(man)
    nb, q = 86, group.q
    rng = np.random.default_rng(86)
    ids = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    bn = rng.integers(0, 128, (nb, 32), dtype=np.uint8)   # top bit clear: below q
    pre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2, with_cts=True)
    rho = np.frombuffer(b"".join(ref.H(q, "fixed", bn[b], ref.i32(4), ref.i32(w)) for b in range(nb)
                                 for w in range(sh.V)), np.uint8).reshape(-1, 32)
    alpha = group.gPowP_batch(rho)
    ktab = FixedBase(group, key.K, key.window_bits)
    try:
        beta = ktab.pow_batch(rho).copy()
    finally:
        ktab.close()
    diag = np.zeros(sh.V, bool)
    for m, vo in zip(sh.spc, sh.voff):
        diag[[vo + i * m + i for i in range(m)]] = True
    diag = np.tile(diag, nb)
    g_rows = np.tile(np.frombuffer(group._g_be, np.uint8), (int(diag.sum()), 1))
    beta[diag] = group.multP_batch(np.ascontiguousarray(beta[diag]), g_rows)
    assert np.array_equal(pre.vec_cts[:, :, 0].reshape(-1, 512), alpha)
    assert np.array_equal(pre.vec_cts[:, :, 1].reshape(-1, 512), beta)
    want = pe.hashes_from_cts_host(q, man, 2, hashes, ids, pre.vec_cts)
    assert same(pre, want, PRE_FIELDS)
    # recording: the chosen vectors are the pre-encryption's rows, ranks and codes follow perm
    votes = random_votes(rng, man, nb)
    rec = pe.record_ballots(group, key, QBAR, man, hashes, bn, votes, pre.sorted, 2)
    assert rec.ok.all()
    for b in range(nb):
        for m, L, o, vo, so, to in zip(sh.spc, sh.limits, sh.off, sh.voff, sh.soff, sh.toff):
            rank_of = {int(i): r for r, i in enumerate(pre.perm[b, o:o + m])}
            chosen = sorted(np.flatnonzero(votes[b, o:o + m]).tolist(), key=lambda i: rank_of[i])
            assert rec.sel_rank[b, to:to + L].tolist() == [rank_of[i] for i in chosen]
            assert rec.sel_codes[b, to:to + L].tolist() == [int(pre.codes[b, o + i]) for i in chosen]
            for t, i in enumerate(chosen):
                assert np.array_equal(rec.sel_vecs[b, so + t * m: so + (t + 1) * m],
                                      pre.vec_cts[b, vo + i * m: vo + (i + 1) * m])
    ok_s, ok_c, _ = Verifier(group, key, QBAR, man).verify(rec.ballots, with_tally=False)
    assert ok_s.all() and ok_c.all()
    okc, okb = pe.verify_recorded(group, man, hashes, ids, rec.sel_vecs, rec.sel_rank, rec.sel_codes, pre.sorted,
                                  rec.ballots.cts, pre.conf, 2)
    assert okc.shape == (nb, 3) and okc.all() and okb.all()


# ---------------------------------------------------------------------------------------------
# short codes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [1, 2, 3, 4])
def test_short_codes_and_the_collision_flag(group, env, recorded, cb):
    pe, fx, key, man, hashes, ids, bn, _ = env
    sh = pe.pre_shape(man)
    base, _ = recorded
    pre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, cb)
    assert pre.unique.tolist() == fx["fixed"]["unique"][str(cb)]
    if cb == 1:
        assert 0 in pre.unique.tolist() and 1 in pre.unique.tolist()
    assert np.array_equal(pre.sorted, base.sorted) and np.array_equal(pre.perm, base.perm)
    for b in range(5):
        for m, o in zip(sh.spc, sh.off):
            for r in range(m):
                i = int(pre.perm[b, o + r])
                assert int(pre.codes[b, o + i]) == b2i(pre.sorted[b, o + r, 32 - cb:])


# ---------------------------------------------------------------------------------------------
# chunk crossing
# ---------------------------------------------------------------------------------------------
def test_one_ballot_more_than_a_chunk(group, env):
    from electionguard.ballot import ElectionManifest
    from electionguard.codes import ManifestHashes
    pe, _, key, *_ = env
    man = ElectionManifest([(15, 1)])
    assert pe.pre_shape(man).V == 256
    per = pe.ballots_per_chunk(man)
    assert per == pe.CHUNK_CTS // 256
    nb = per + 1
    rng = np.random.default_rng(256)
    hashes = ManifestHashes(np.zeros((16, 32), np.uint8), rng.integers(0, 256, (1, 32), dtype=np.uint8),
                            rng.integers(0, 256, 32, dtype=np.uint8))
    ids = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    bn = rng.integers(0, 128, (nb, 32), dtype=np.uint8)
    d = pe.preencrypt_ballots(group, key, man, hashes, group.to_device(ids), group.to_device(bn), 2)
    assert d.vec_cts is None
    got = {f: getattr(d, f).download() for f in PRE_FIELDS}
    for b in (per - 1, per):   # the last ballot of the first chunk, the first of the second
        one = pe.preencrypt_ballots(group, key, man, hashes, ids[b:b + 1], bn[b:b + 1], 2)
        for f in PRE_FIELDS:
            assert np.array_equal(got[f][b:b + 1], getattr(one, f)), (b, f)
    assert len({bytes(x) for x in got["conf"][[0, per - 1, per]]}) == 3


# ---------------------------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------------------------
def test_recording_matches_the_reference_and_the_encryptor(group, env, recorded):
    from electionguard.ballot import Verifier
    pe, fx, key, man, hashes, ids, bn, votes = env
    f = fx["fixed"]
    pre, rec = recorded
    sh = pe.pre_shape(man)
    # 0, 1 and 2 real choices in the limit-2 contest, an undervote in each limit-1 contest
    assert sorted(set(votes[:, 2:5].sum(axis=1).tolist())) == [0, 1, 2]
    assert votes[:, 1].any() and votes[:, 9].any()
    assert rec.ok.all()
    assert sha(rec.sel_vecs) == f["sel_vecs_sha256"]
    assert rec.sel_rank.reshape(-1).tolist() == f["sel_rank"]
    assert rec.sel_codes.reshape(-1).tolist() == f["sel_codes2"]
    assert sha(rec.sel_nonces) == f["sel_nonces_sha256"]
    assert sha(rec.contest_nonces) == f["contest_nonces_sha256"]
    assert np.array_equal(pe.vector_product_host(group.p, man, rec.sel_vecs), rec.ballots.cts)
    ok_s, ok_c, _ = Verifier(group, key, QBAR, man).verify(rec.ballots, with_tally=False)
    assert ok_s.all() and ok_c.all()
    okc, okb = pe.verify_recorded(group, man, hashes, ids, rec.sel_vecs, rec.sel_rank, rec.sel_codes, pre.sorted,
                                  rec.ballots.cts, pre.conf, 2)
    assert okc.all() and okb.all()
    # the device variant: same bytes
    d = pe.record_ballots(group, key, QBAR, man, hashes, group.to_device(bn), group.to_device(votes),
                          group.to_device(pre.sorted), 2)
    for name in REC_FIELDS:
        assert np.array_equal(getattr(d, name).download(), getattr(rec, name)), name
    assert np.array_equal(d.ballots.cts.download(), rec.ballots.cts)
    assert np.array_equal(d.ballots.rproof.download(), rec.ballots.rproof)
    dk, dv = pe.verify_recorded(group, man, hashes, group.to_device(ids), d.sel_vecs, d.sel_rank, d.sel_codes,
                                group.to_device(pre.sorted), d.ballots.cts, group.to_device(pre.conf), 2)
    assert dk.download().all() and dv.download().all()


def test_bad_votes_fail_their_contest_only(group, env, recorded):
    pe, _, key, man, hashes, _, bn, votes = env
    pre, rec = recorded
    v = votes.copy()
    v[0, 2:7] = [1, 1, 1, 0, 0]   # contest 1 sums to 3
    v[1, 7:10] = [2, 0, 0]        # a 2 in contest 2
    v[2, 0:2] = [0, 0]            # contest 0 sums to 0
    bad = pe.record_parts(group, key, man, hashes, bn, v, pre.sorted, 2)
    assert bad.ok.tolist() == [[1, 0, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1], [1, 1, 1]]
    sh = pe.pre_shape(man)
    # the untouched contests of those ballots are recorded as before
    assert np.array_equal(bad.sel_vecs[0, : sh.soff[1]], rec.sel_vecs[0, : sh.soff[1]])
    assert np.array_equal(bad.sel_vecs[1, : sh.soff[2]], rec.sel_vecs[1, : sh.soff[2]])
    assert np.array_equal(bad.sel_vecs[3:], rec.sel_vecs[3:])
    # a sorted list that does not hold the chosen vector's hash
    srt = pre.sorted.copy()
    srt[4, sh.off[2]: sh.off[2] + 3, 5] ^= 1
    assert pe.record_parts(group, key, man, hashes, bn, votes, srt, 2).ok.tolist() == [[1, 1, 1]] * 4 + [[1, 1, 0]]


# ---------------------------------------------------------------------------------------------
# tampering
# ---------------------------------------------------------------------------------------------
def test_every_tampering_flips_the_flags_the_host_mirror_flips(group, env, recorded):
    pe, _, key, man, hashes, ids, _, _ = env
    pre, rec = recorded
    good = dict(sel_vecs=rec.sel_vecs, sel_rank=rec.sel_rank, sel_codes=rec.sel_codes, sorted=pre.sorted,
                cts=rec.ballots.cts, conf=pre.conf)
    corpus = ref.tamper_corpus(group.p, ref.M, good)
    assert len(corpus) == 9
    cat = {k: np.concatenate([a[k] for _, a, _, _ in corpus]) for k in good}
    ids9 = np.tile(ids, (9, 1))
    okc, okb = pe.verify_recorded(group, man, hashes, ids9, cat["sel_vecs"], cat["sel_rank"], cat["sel_codes"],
                                  cat["sorted"], cat["cts"], cat["conf"], 2)
    hc, hb = pe.verify_recorded_host(group.p, group.q, man, 2, hashes, ids9, cat["sel_vecs"], cat["sel_rank"],
                                     cat["sel_codes"], cat["sorted"], cat["cts"], cat["conf"])
    assert np.array_equal(okc, hc) and np.array_equal(okb, hb)
    for n, (name, _, contests, ballots) in enumerate(corpus):
        c, b = okc[5 * n: 5 * n + 5], okb[5 * n: 5 * n + 5]
        assert {(int(x), int(y)) for x, y in zip(*np.nonzero(~c))} == contests, name
        assert set(np.flatnonzero(~b).tolist()) == ballots, name


# ---------------------------------------------------------------------------------------------
# constant-time mode
# ---------------------------------------------------------------------------------------------
def test_constant_time_mode_gives_identical_bytes(group, env, recorded):
    pe, _, key, man, hashes, ids, bn, votes = env
    pre, rec = recorded
    group.ct_encrypt = True
    try:
        cpre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2, with_cts=True)
        crec = pe.record_parts(group, key, man, hashes, bn, votes, pre.sorted, 2)
    finally:
        group.ct_encrypt = False
    assert same(cpre, pre, PRE_FIELDS + ("vec_cts",))
    assert same(crec, rec, REC_FIELDS)


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def test_arguments_on_a_live_context(group, env, recorded):
    from electionguard.core import native
    pe, _, key, man, hashes, ids, bn, votes = env
    pre, rec = recorded
    lib, h = group._lib, group.handle
    K = native.buf(key.K_be)
    p = lambda a: a.ctypes.data_as(native.c_vp)
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    spc, lim = u32(2, 5, 3), u32(1, 2, 1)
    dcon, mh = np.ascontiguousarray(hashes.dcon), np.ascontiguousarray(hashes.manifest_hash)
    o = pe.PreEncrypted(*(np.empty_like(getattr(pre, f)) for f in ("sorted", "perm", "codes", "unique", "conf")))
    outs = [p(o.sorted), p(o.perm), p(o.codes), p(o.unique), p(o.conf), None, None]

    def pre_call(nc, spc_, cb, dcon_=p(dcon)):
        return lib.eg_preencrypt_ballots(h, K, 5, nc, spc_, cb, dcon_, p(mh), p(ids), p(bn), *outs)

    def err(*words):
        msg = lib.eg_last_error()
        return b"preencrypt" in msg and all(w in msg for w in words)

    assert pre_call(3, spc, 2) == 0 and np.array_equal(o.conf, pre.conf)
    assert pre_call(3, spc, 0) == 1 and err(b"code_bytes")
    assert pre_call(3, spc, 5) == 1 and err(b"code_bytes")
    assert pre_call(0, spc, 2) == 1 and err(b"no contests")
    assert pre_call(3, u32(2, 0, 3), 2) == 1 and err(b"contest 1", b"no selections")
    assert pre_call(3, u32(2, 65, 3), 2) == 1 and err(b"contest 1", b"64")
    # the per-ballot caps stop the shape scan before anything is sized by it
    assert pre_call(1025, u32(*[64] * 1025), 2) == 1 and err(b"2^22 component ciphertexts")
    assert pre_call((1 << 20) + 1, u32(*[1] * ((1 << 20) + 1)), 2) == 1 and err(b"2^20 selections")
    assert pre_call(3, None, 2) == 1 and err(b"null")
    assert pre_call(3, spc, 2, None) == 1 and err(b"null")
    r = [np.empty_like(getattr(rec, f)) for f in REC_FIELDS]
    r_out = [p(r[0]), p(r[1]), p(r[2]), p(r[4]), p(r[5]), p(r[3])]

    def rec_call(lim_, cb=2):
        return lib.eg_preencrypt_record(h, K, 5, 3, spc, lim_, cb, p(dcon), p(bn), p(votes), p(pre.sorted), *r_out)

    assert rec_call(lim) == 0 and np.array_equal(r[0], rec.sel_vecs)
    assert rec_call(u32(1, 6, 1)) == 1 and err(b"contest 1", b"limit")
    assert rec_call(u32(0, 2, 1)) == 1 and err(b"contest 0", b"limit")
    assert rec_call(None) == 1 and err(b"null")
    assert rec_call(lim, 9) == 1 and err(b"code_bytes")
    okc, okb = np.zeros((5, 3), np.uint8), np.zeros(5, np.uint8)
    ver = [p(dcon), p(mh), p(ids), p(rec.sel_vecs), p(rec.sel_rank), p(rec.sel_codes), p(pre.sorted),
           p(rec.ballots.cts), p(pre.conf), p(okc), p(okb)]
    assert lib.eg_preencrypt_verify(h, 5, 3, spc, lim, 2, *ver) == 0 and okc.all() and okb.all()
    assert lib.eg_preencrypt_verify(h, 5, 3, spc, u32(1, 2, 4), 2, *ver) == 1 and err(b"contest 2", b"limit")
    assert lib.eg_preencrypt_verify(h, 5, 3, spc, lim, 2, *ver[:-1], None) == 1 and err(b"null")
    # nballots == 0 is fine and touches nothing
    assert lib.eg_preencrypt_ballots(h, K, 0, 3, spc, 2, *[None] * 11) == 0
    assert lib.eg_preencrypt_ballots_dev(h, K, 0, 3, spc, 2, *[None] * 11) == 0
    assert lib.eg_preencrypt_record(h, K, 0, 3, spc, lim, 2, *[None] * 10) == 0
    assert lib.eg_preencrypt_record_dev(h, K, 0, 3, spc, lim, 2, *[None] * 10) == 0
    assert lib.eg_preencrypt_verify(h, 0, 3, spc, lim, 2, *[None] * 11) == 0
    assert lib.eg_preencrypt_verify_dev(h, 0, 3, spc, lim, 2, *[None] * 11) == 0
    # a misaligned device pointer
    raw = group.device_empty((5 * 32 + 16,))
    d = [group.to_device(x) for x in (np.concatenate([dcon.reshape(-1), mh]), ids, bn)]
    dout = [group.device_empty(s, t) for s, t in (((5, 10, 32), np.uint8), ((5, 10), np.uint32), ((5, 10), np.uint32),
                                                  ((5,), np.uint8), ((5, 32), np.uint8))]
    args = [d[0].ptr, d[0].ptr + 96, d[1].ptr, d[2].ptr] + [x.ptr for x in dout] + [None, None]
    assert lib.eg_preencrypt_ballots_dev(h, K, 5, 3, spc, 2, *args) == 0
    assert np.array_equal(dout[4].download(), pre.conf)
    args[3] = raw[8:].ptr
    assert lib.eg_preencrypt_ballots_dev(h, K, 5, 3, spc, 2, *args) == 1 and err(b"aligned")


# ---------------------------------------------------------------------------------------------
# the election record
# ---------------------------------------------------------------------------------------------
def test_election_record_hook(group, env):
    from electionguard import codes
    from electionguard.ballot import ElectionKey, Verifier
    from electionguard.decrypt import DecryptingTrustee, Decryption
    from electionguard.keyceremony import key_ceremony
    from electionguard.record import ElectionRecord, GuardianRecord, verify_election_record
    pe, _, _, man, hashes, ids, bn, votes = env
    gk, K = key_ceremony(group, 3, 2, seed=14)
    key = ElectionKey(group, K)
    nb = len(votes)
    pre = pe.preencrypt_ballots(group, key, man, hashes, ids, bn, 2)
    assert pre.unique.all()
    rec = pe.record_ballots(group, key, QBAR, man, hashes, bn, votes, pre.sorted, 2)
    _, _, tally = Verifier(group, key, QBAR, man).verify(rec.ballots)
    comm = {g.gid: g.commitments for g in gk}
    drec = Decryption(group, QBAR, [DecryptingTrustee(group, g, comm) for g in gk[:2]], [gk[2].gid],
                      {g.gid: g.public_key for g in gk}).decrypt_record(tally, nb)
    ts = [1700000000 + 7 * b for b in range(nb)]
    seed = bytes(range(32))
    chain = codes.chain_codes(group.q, seed, ts, pre.conf)
    er = ElectionRecord(man, QBAR, K, [GuardianRecord(g.gid, g.x, list(g.commitments), list(g.proofs)) for g in gk],
                        rec.ballots, tally, drec, ballot_ids=ids, timestamps=np.array(ts), code_seed=seed,
                        codes=chain, hashes=hashes)
    part = pe.PreencryptedRecord(rec.sel_vecs, rec.sel_rank, rec.sel_codes, pre.sorted, pre.conf, 2)
    res = verify_election_record(group, er, preencrypted=part)
    assert res["preencrypted"] and res["ballot_codes"] and all(res.values()), res
    # without the pre-encryption part the chain is taken over the ballot hashes and does not close
    assert not verify_election_record(group, er)["ballot_codes"]
    bad = copy.copy(er)
    bad.codes = chain.copy()
    bad.codes[2, 9] ^= 4   # a broken link
    res = verify_election_record(group, bad, preencrypted=part)
    assert sorted(k for k, v in res.items() if not v) == ["ballot_codes"]
    bad_part = copy.copy(part)
    bad_part.sel_rank = part.sel_rank.copy()
    bad_part.sel_rank[1, 0] ^= 1
    res = verify_election_record(group, er, preencrypted=bad_part)
    assert sorted(k for k, v in res.items() if not v) == ["preencrypted"]


# ---------------------------------------------------------------------------------------------
# chunk crossing of the host-pointer variants
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crossing(group, env):
    """The (15, 1) manifest: 256 components and 16 chosen components per ballot, so pre-encryption
    chunks by ballots_per_chunk(man) = 1,024 ballots, recording and the check by CHUNK_CTS // 16 =
    16,384.  One ballot more than the larger chunk, pre-encrypted and recorded by the device
    variants and downloaded once."""
    from electionguard.ballot import ElectionManifest
    from electionguard.codes import ManifestHashes
    pe, _, key, *_ = env
    man = ElectionManifest([(15, 1)])
    sh = pe.pre_shape(man)
    assert (sh.V, sh.S, sh.T) == (256, 16, 1)
    chunk = pe.CHUNK_CTS // sh.S
    nb = chunk + 1
    rng = np.random.default_rng(257)
    hashes = ManifestHashes(np.zeros((16, 32), np.uint8), rng.integers(0, 256, (1, 32), dtype=np.uint8),
                            rng.integers(0, 256, 32, dtype=np.uint8))
    ids = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    bn = rng.integers(0, 128, (nb, 32), dtype=np.uint8)
    votes = np.zeros((nb, 16), np.uint8)   # one vote per ballot, the placeholder included
    votes[np.arange(nb), rng.integers(0, 16, nb)] = 1
    d_bn = group.to_device(bn)
    dpre = pe.preencrypt_ballots(group, key, man, hashes, group.to_device(ids), d_bn, 2)
    pre = {f: getattr(dpre, f).download() for f in PRE_FIELDS}
    drec = pe.record_parts(group, key, man, hashes, d_bn, group.to_device(votes), dpre.sorted, 2)
    rec = {f: getattr(drec, f).download() for f in REC_FIELDS}
    return man, hashes, ids, bn, votes, chunk, pre, rec


def test_host_preencryption_one_ballot_more_than_a_chunk(group, env, crossing):
    pe, _, key, *_ = env
    man, hashes, ids, bn, _, _, pre, _ = crossing
    nb = pe.ballots_per_chunk(man) + 1
    host = pe.preencrypt_ballots(group, key, man, hashes, ids[:nb], bn[:nb], 2)
    assert host.vec_cts is None
    dev = pe.preencrypt_ballots(group, key, man, hashes, group.to_device(ids[:nb]), group.to_device(bn[:nb]), 2)
    for f in PRE_FIELDS:
        assert np.array_equal(getattr(host, f), getattr(dev, f).download()), f
        assert np.array_equal(getattr(host, f), pre[f][:nb]), f


def test_host_record_and_check_one_ballot_more_than_a_chunk(group, env, crossing):
    pe, _, key, *_ = env
    man, hashes, ids, bn, votes, chunk, pre, rec = crossing
    nb = chunk + 1
    host = pe.record_parts(group, key, man, hashes, bn, votes, pre["sorted"], 2)
    assert host.ok.all()
    for f in REC_FIELDS:
        assert np.array_equal(getattr(host, f), rec[f]), f
    # one chosen vector per contest (limit 1): the selections' ciphertexts are the chosen vectors
    sv, rank, codes = rec["sel_vecs"], rec["sel_rank"], rec["sel_codes"]
    okc, okb = pe.verify_recorded(group, man, hashes, ids, sv, rank, codes, pre["sorted"], sv, pre["conf"], 2)
    assert okc.shape == (nb, 1) and okc.all() and okb.all()
    # ballot `chunk` is the second chunk: a wrong rank, and a confirmation hash off by a bit
    bad_rank, bad_conf = rank.copy(), pre["conf"].copy()
    bad_rank[chunk, 0] ^= 1
    bad_conf[chunk, 7] ^= 2
    okc, okb = pe.verify_recorded(group, man, hashes, ids, sv, bad_rank, codes, pre["sorted"], sv, bad_conf, 2)
    d_sv = group.to_device(sv)
    dkc, dkb = pe.verify_recorded(group, man, hashes, group.to_device(ids), d_sv, group.to_device(bad_rank),
                                  group.to_device(codes), group.to_device(pre["sorted"]), d_sv,
                                  group.to_device(bad_conf), 2)
    assert np.array_equal(okc, dkc.download().astype(bool)) and np.array_equal(okb, dkb.download().astype(bool))
    assert np.flatnonzero(~okc[:, 0]).tolist() == [chunk] and np.flatnonzero(~okb).tolist() == [chunk]
