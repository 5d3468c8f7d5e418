"""GPU: ballots without placeholders (include/eg_hip_ballot2.h, electionguard.ballot2) against the
fixture of tests/ballot2_ref.py (tests/golden/Mode4096/ballots2.json), the range-proof calls that
already exist, and CPython products: the encryptors' bytes, the verifier's verdicts and tally, the
tamper matrix, two chunks, the k_pow work and the argument checks."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest

import ballot2_ref as ref
import eg_oracle as O
from range_proof_ref import be2i, rows

pytestmark = pytest.mark.gpu

DEFAULT = ("fixed", ("minus", "message_first"))


@pytest.fixture(scope="module")
def fx(group):
    """The fixture, its inputs, the expected bytes and the GPU's honest ballots (never modified)."""
    from electionguard import ballot2 as b2
    from electionguard.ballot import ElectionKey
    og = O.production_group()
    f = json.loads(ref.FIXTURE.read_text())
    K, qbar, man_l, votes, sn, cn = ref.fixture_inputs(og, f)
    man = b2.Manifest2(man_l)
    sproof, cproof = ref.fixture_proofs(f)
    cts = np.stack([np.stack([rows([og.gPowP(be2i(sn[b, nr])),
                                    og.multP(og.powP(K, be2i(sn[b, nr])), og.gPowP(int(votes[b, s])))], 512)
                              for _, _, s, _, _, nr in man.selections()]) for b in range(len(votes))])
    key = ElectionKey(group, K)
    eb = b2.encrypt(group, key, qbar, man, votes, sn, cn)
    out = SimpleNamespace(og=og, K=K, qbar=qbar, man=man, man_l=man_l, votes=votes, sn=sn, cn=cn, cts=cts,
                          sproof=sproof, cproof=cproof, key=key, eb=eb, nb=len(votes))
    for a in (votes, sn, cn, cts, sproof, cproof, eb.cts, eb.sproof, eb.cproof):
        a.setflags(write=False)
    return out


def products(og, cts, cast=None):
    """CPython products over the cast ballots of cts (nb, NS, 2, 512) -> (NS, 2, 512)"""
    nb, ns = cts.shape[:2]
    out = []
    for s in range(ns):
        a = b = 1
        for i in range(nb):
            if cast is None or cast[i]:
                a, b = a * be2i(cts[i, s, 0]) % og.p, b * be2i(cts[i, s, 1]) % og.p
        out.append(rows([a, b], 512))
    return np.stack(out)


def down(x):
    return x if isinstance(x, np.ndarray) else x.download()


def verify(group, f, eb, man=None, dev=False, **kw):
    from electionguard import ballot2 as b2
    if dev:
        eb = b2.EncryptedBallots2(*(group.to_device(np.ascontiguousarray(a)) for a in (eb.cts, eb.sproof, eb.cproof)))
        if kw.get("cast") is not None:
            kw["cast"] = group.to_device(np.asarray(kw["cast"], np.uint8))
    ok_s, ok_c, tally = b2.Verifier2(group, f.key, f.qbar, man or f.man).verify(eb, **kw)
    return down(ok_s).astype(bool), down(ok_c).astype(bool), None if tally is None else down(tally)


# ---------------------------------------------------------------------------------------------
# byte parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True], ids=["radix", "ct_encrypt"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("nb", [1, 5])
def test_encryptors_reproduce_the_fixture(group, fx, nb, dev, ct):
    from electionguard import ballot2 as b2
    up = group.to_device if dev else (lambda a: a)
    group.ct_encrypt = ct
    try:
        eb = b2.encrypt(group, fx.key, fx.qbar, fx.man, up(fx.votes[:nb]), up(fx.sn[:nb]), up(fx.cn[:nb]))
    finally:
        group.ct_encrypt = False
    assert np.array_equal(down(eb.cts), fx.cts[:nb])
    assert np.array_equal(down(eb.sproof), fx.sproof[:nb])
    assert np.array_equal(down(eb.cproof), fx.cproof[:nb])


_OTHER = {}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_one_ballot_under_another_proof_format(group, fx, dev):
    from electionguard import ballot2 as b2
    own = ("minimal", "plus", "with_key")
    if not _OTHER:   # the reference's ballot, once for both variants
        with O.hash_format(own[0]), O.proof_format(*own[1:]):
            _OTHER["want"] = ref.encrypt(fx.og, fx.K, fx.qbar, fx.man_l, fx.votes[:1], fx.sn[:1], fx.cn[:1])
    want = _OTHER["want"]
    up = group.to_device if dev else (lambda a: a)
    try:
        group.hash_format, group.proof_format = own[0], own[1:]
        eb = b2.encrypt(group, fx.key, fx.qbar, fx.man, up(fx.votes[:1]), up(fx.sn[:1]), up(fx.cn[:1]))
        eb = b2.EncryptedBallots2(down(eb.cts), down(eb.sproof), down(eb.cproof))
        ok_s, ok_c, _ = verify(group, fx, eb)
        assert ok_s.all() and ok_c.all()
        group.hash_format, group.proof_format = DEFAULT
        bad_s, bad_c, _ = verify(group, fx, eb)
        assert not bad_s.any() and not bad_c.any()
    finally:
        group.hash_format, group.proof_format = DEFAULT
    assert np.array_equal(eb.sproof, want[1]) and np.array_equal(eb.cproof, want[2])
    assert not np.array_equal(eb.sproof, fx.sproof[:1])


# ---------------------------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("nb", [1, 5])
def test_verdicts_and_tally(group, fx, nb, dev):
    from electionguard import ballot2 as b2
    eb = b2.EncryptedBallots2(fx.eb.cts[:nb], fx.eb.sproof[:nb], fx.eb.cproof[:nb])
    ok_s, ok_c, tally = verify(group, fx, eb, dev=dev)
    assert ok_s.shape == (nb, fx.man.NS) and ok_c.shape == (nb, 4)
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(tally, products(fx.og, fx.cts[:nb]))
    ok_s, ok_c, none = verify(group, fx, eb, dev=dev, with_tally=False)
    assert ok_s.all() and ok_c.all() and none is None


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_only_cast_ballots_are_tallied(group, fx, dev):
    cast = [1, 0, 1, 1, 0]
    ok_s, ok_c, tally = verify(group, fx, fx.eb, dev=dev, cast=cast)
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(tally, products(fx.og, fx.cts, cast))
    assert not np.array_equal(tally, products(fx.og, fx.cts))
    _, _, none_cast = verify(group, fx, fx.eb, dev=dev, cast=[0] * 5)
    assert np.array_equal(none_cast, products(fx.og, fx.cts, [0] * 5))   # all ones


def test_the_tally_decrypts_to_the_vote_sums(group):
    from electionguard import ballot2 as b2
    from electionguard.ballot import ElectionKey
    from electionguard.decrypt import DecryptingTrustee, Decryption
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=5)
    key, qbar, man = ElectionKey(group, K), 0xB2, b2.Manifest2(ref.M0)
    votes, nb = np.array(ref.VOTES0, np.uint8), len(ref.VOTES0)
    sn, cn = b2.random_nonces2(np.random.default_rng(3), man, nb, group.q)
    eb = b2.encrypt(group, key, qbar, man, votes, sn, cn)
    ok_s, ok_c, tally = b2.Verifier2(group, key, qbar, man).verify(eb)
    assert ok_s.all() and ok_c.all()
    comm = {g.gid: g.commitments for g in gk}
    dec = Decryption(group, qbar, [DecryptingTrustee(group, g, comm) for g in gk[:2]], [gk[2].gid],
                     {g.gid: g.public_key for g in gk})
    assert dec.decrypt(tally, nb * 3) == votes.sum(axis=0).tolist()


# ---------------------------------------------------------------------------------------------
# agreement with the range-proof calls
# ---------------------------------------------------------------------------------------------
def aggregates(og, man, cts):
    """(nb, nc, 2, 512) by CPython products"""
    out = np.zeros((len(cts), man.n_contests, 2, 512), np.uint8)
    for b in range(len(cts)):
        for k, (n, _, _) in enumerate(man.contests):
            f = int(man.first[k])
            out[b, k] = products(og, cts[b, f:f + n].reshape(n, 1, 2, 512))[0]
    return out


def class_items(man, votes, sn, cts, L):
    """The selections of option limit L as range items: index (b, s), cts, values, R, nonces, proof rows"""
    sel = [(s, pr, nr) for _, _, s, o, pr, nr in man.selections() if o == L]
    idx = [(b, s, pr) for b in range(len(votes)) for s, pr, _ in sel]
    R = np.stack([sn[b, nr] for b in range(len(votes)) for _, _, nr in sel])
    non = np.stack([sn[b, nr + 1:nr + 2 * L + 4] for b in range(len(votes)) for _, _, nr in sel])
    return idx, np.stack([cts[b, s] for b, s, _ in idx]), np.array([votes[b, s] for b, s, _ in idx], np.uint8), R, non


def test_selection_rows_equal_range_prove_per_class(group, fx):
    from electionguard import range_proof as rp
    for L in sorted(set(int(o) for o in fx.man.olimit)):
        idx, cts, values, R, non = class_items(fx.man, fx.votes, fx.sn, fx.cts, L)
        pr = rp.prove(group, fx.key, fx.qbar, L, cts, values, R, non)
        for i, (b, s, row) in enumerate(idx):
            assert np.array_equal(fx.eb.sproof[b, row:row + L + 1], pr[i]), (L, b, s)


def test_ok_contest_is_contest_limit_verify_and_the_residue_verdicts(group, fx):
    from electionguard import range_proof as rp
    man, nb = fx.man, fx.nb
    cts = fx.eb.cts.copy()
    cts[2, 8, 0] = rows([fx.og.p - be2i(cts[2, 8, 0])], 512)[0]   # alpha (p - 1): not a residue
    for s in (4, 6):                                              # a twisted pair: contest 1's aggregate is unchanged
        cts[3, s, 1] = rows([fx.og.p - be2i(cts[3, s, 1])], 512)[0]
    duck = SimpleNamespace(contests=[SimpleNamespace(n_selections=n, votes_allowed=c) for n, _, c in man.contests],
                           offsets=man.first, n_contests=4, nsel=man.NS, max_votes_allowed=int(man.climit.max()))
    Lmax = duck.max_votes_allowed
    wide = np.zeros((nb, 4, Lmax + 1, 2, 32), np.uint8)
    for k, (_, _, c) in enumerate(man.contests):
        wide[:, k, :c + 1] = fx.eb.cproof[:, int(man.cp_off[k]):int(man.cp_off[k]) + c + 1]
    limit_ok = rp.contest_limit_verify(group, fx.key, fx.qbar, duck, SimpleNamespace(n=nb, cts=cts), wide)
    hg = rp.HostGroup(fx.og.p, fx.og.q, fx.og.g)
    resid = np.array([[all(rp.valid_residue_host(hg, be2i(cts[b, s, c])) for s in range(int(man.first[k]),
                           int(man.first[k]) + n) for c in range(2)) for k, (n, _, _) in enumerate(man.contests)]
                      for b in range(nb)])
    from electionguard import ballot2 as b2
    _, ok_c, _ = verify(group, fx, b2.EncryptedBallots2(cts, fx.eb.sproof, fx.eb.cproof))
    assert not resid[2, 3] and not resid[3, 1] and resid.sum() == resid.size - 2
    assert not limit_ok[2, 3] and limit_ok[3, 1]   # the limit proof alone does not see the twisted pair
    assert np.array_equal(ok_c, limit_ok & resid) and not ok_c[3, 1]


# ---------------------------------------------------------------------------------------------
# tamper matrix: each case changes exactly the listed verdicts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_tampered_ballots_change_exactly_their_verdicts(group, fx, dev):
    from electionguard import ballot2 as b2
    man = fx.man
    cts, sp, cp = (np.stack([a[0]] * 5) for a in (fx.eb.cts, fx.eb.sproof, fx.eb.cproof))
    want_s, want_c = np.ones((5, man.NS), bool), np.ones((5, 4), bool)
    sel = {s: (pr, L) for _, _, s, L, pr, _ in man.selections()}
    sp[0, sel[4][0] + 1, 1, 31] ^= 1; want_s[0, 4] = False              # a bit of one selection response
    cp[1, int(man.cp_off[1]) + 2, 0, 5] ^= 0x10; want_c[1, 1] = False   # a bit of one contest challenge
    cts[2, 8, 0] = rows([fx.og.p - be2i(cts[2, 8, 0])], 512)[0]         # alpha (p - 1)
    want_s[2, 8] = False; want_c[2, 3] = False
    a, b = sel[0][0], sel[1][0]                                         # proofs of neighbours swapped
    sp[3, a:a + 2], sp[3, b:b + 2] = fx.eb.sproof[0, b:b + 2], fx.eb.sproof[0, a:a + 2]
    want_s[3, 0] = want_s[3, 1] = False
    # a twisted pair: two alphas of one contest (option limit 2: a class with gather jobs) times
    # p - 1.  The aggregate is unchanged, so the contest's own proof still verifies and only the
    # fold with its selections' residue flags can reject the contest.
    for s in (3, 4):
        cts[4, s, 0] = rows([fx.og.p - be2i(cts[4, s, 0])], 512)[0]
    assert np.array_equal(aggregates(fx.og, man, cts[4:5]), aggregates(fx.og, man, fx.cts[:1]))
    want_s[4, 3] = want_s[4, 4] = False; want_c[4, 1] = False
    ok_s, ok_c, tally = verify(group, fx, b2.EncryptedBallots2(cts, sp, cp), dev=dev)
    assert np.array_equal(ok_s, want_s) and np.array_equal(ok_c, want_c)
    assert np.array_equal(tally, products(fx.og, cts))   # whatever the verdicts


def test_dev_encryptor_zeroes_the_rows_of_votes_over_a_limit(group, fx):
    from electionguard import ballot2 as b2
    man = fx.man
    votes = np.stack([fx.votes[1]] * 2)                  # empty ballots
    votes[0, 8] = 2                                      # 2 in an olimit = 1 selection; its contest allows 2
    votes[1, 0] = votes[1, 1] = 1                        # contest 0 holds 2 of 1, every selection within 1
    with pytest.raises(Exception, match=r"ballot2: ballot 0 contest 3 selection 0 holds 2, above its option limit 1"):
        b2.encrypt(group, fx.key, fx.qbar, man, votes, fx.sn[:2], fx.cn[:2])
    with pytest.raises(Exception, match=r"ballot2: ballot 0 contest 0 holds 2, above its contest limit 1"):
        b2.encrypt(group, fx.key, fx.qbar, man, votes[1:], fx.sn[:2][1:], fx.cn[:2][1:])
    eb = b2.encrypt(group, fx.key, fx.qbar, man, *(group.to_device(a) for a in (votes, fx.sn[:2], fx.cn[:2])))
    sp, cp = eb.sproof.download(), eb.cproof.download()
    sel = {s: pr for _, _, s, _, pr, _ in man.selections()}
    assert not sp[0, sel[8]:sel[8] + 2].any() and sp[0, :sel[8]].any() and not cp[1, :2].any()
    want_s, want_c = np.ones((2, man.NS), bool), np.ones((2, 4), bool)
    want_s[0, 8] = False
    want_c[1, 0] = False
    ok_s, ok_c, _ = b2.Verifier2(group, fx.key, fx.qbar, man).verify(eb)
    assert np.array_equal(ok_s.download().astype(bool), want_s)
    assert np.array_equal(ok_c.download().astype(bool), want_c)
    want_cts = np.stack([np.stack([rows([fx.og.gPowP(be2i(fx.sn[b, nr])),
                                         fx.og.multP(fx.og.powP(fx.K, be2i(fx.sn[b, nr])),
                                                     fx.og.gPowP(int(votes[b, s])))], 512)
                                   for _, _, s, _, _, nr in man.selections()]) for b in range(2)])
    assert np.array_equal(eb.cts.download(), want_cts)   # the ciphertexts are written as defined


# ---------------------------------------------------------------------------------------------
# two chunks
# ---------------------------------------------------------------------------------------------
def test_two_chunks(group, fx):
    """[(64, 15, 15)]: 1,950 verifier jobs per ballot, so a chunk is 33 ballots; 7 more make a
    second chunk of another size."""
    from electionguard import ballot2 as b2
    from electionguard import range_proof as rp
    og, L = fx.og, 15
    man_l = [(64, L, L)]
    man = b2.Manifest2(man_l)
    chunk = b2.chunk_ballots(man)
    assert chunk == (1 << 16) // (2 * L * 64 + 2 * L) and chunk > 1
    nb = chunk + 7
    rng = np.random.default_rng(15)
    votes = b2.random_votes2(rng, man, nb)
    votes[0] = 0
    votes[0, 63] = L                                       # a selection and its contest at the limit
    sn, cn = b2.random_nonces2(rng, man, nb, og.q)
    eb = b2.encrypt(group, fx.key, fx.qbar, man, votes, sn, cn)
    d_eb = b2.encrypt(group, fx.key, fx.qbar, man, *(group.to_device(a) for a in (votes, sn, cn)))
    for a, d in ((eb.cts, d_eb.cts), (eb.sproof, d_eb.sproof), (eb.cproof, d_eb.cproof)):
        assert np.array_equal(a, d.download())
    # the proofs are range_proof.prove's on the same items, selections and contests
    idx, cts, values, R, non = class_items(man, votes, sn, eb.cts, L)
    pr = rp.prove(group, fx.key, fx.qbar, L, cts, values, R, non)
    assert np.array_equal(eb.sproof.reshape(nb * 64, L + 1, 2, 32), pr)
    agg = aggregates(og, man, eb.cts)
    rsum = rows([sum(be2i(sn[b, s * (2 * L + 4)]) for s in range(64)) % og.q for b in range(nb)], 32)
    cpr = rp.prove(group, fx.key, fx.qbar, L, agg.reshape(nb, 2, 512), votes.sum(axis=1).astype(np.uint8), rsum, cn)
    assert np.array_equal(eb.cproof.reshape(nb, L + 1, 2, 32), cpr)
    # two ballots, one per chunk, against the reference (one selection and the contest of each)
    for b in (0, chunk + 1):
        only = {("s", 63), ("c", 0)}
        _, want_s, want_c = ref.encrypt(og, fx.K, fx.qbar, man_l, votes[b:b + 1], sn[b:b + 1], cn[b:b + 1], only=only)
        assert np.array_equal(eb.sproof[b, 63 * (L + 1):], want_s[0, 63 * (L + 1):]), b
        assert np.array_equal(eb.cproof[b], want_c[0]), b
    # verdicts, the tally across the boundary, tampering in the second chunk
    ok_s, ok_c, tally = verify(group, fx, eb, man=man)
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(tally, products(og, eb.cts))
    sp, cp = eb.sproof.copy(), eb.cproof.copy()
    sp[chunk + 2, 5 * (L + 1) + 9, 1, 7] ^= 2
    cp[chunk + 4, 15, 0, 31] ^= 1
    want_s, want_c = np.ones((nb, 64), bool), np.ones((nb, 1), bool)
    want_s[chunk + 2, 5] = False
    want_c[chunk + 4, 0] = False
    ok_s, ok_c, tally2 = verify(group, fx, b2.EncryptedBallots2(eb.cts, sp, cp), man=man, dev=True)
    assert np.array_equal(ok_s, want_s) and np.array_equal(ok_c, want_c) and np.array_equal(tally2, tally)


# ---------------------------------------------------------------------------------------------
# work
# ---------------------------------------------------------------------------------------------
def test_k_pow_work_is_the_range_calls_work(group, fx):
    """Montgomery multiplies of the k_pow launches (the context's profile).  Verifier: no more per
    ballot than eg_range_verify reports for its 14 items, each at its limit.  Encryptor: exactly
    eg_range_prove's for the same items plus one ciphertext job per selection, which has the shape
    of one simulated branch (the prover's step from L to L + 1)."""
    from electionguard import ballot2 as b2
    from electionguard import range_proof as rp
    man, nb = fx.man, fx.nb
    limits = [L for _, _, _, L, _, _ in man.selections()] + [int(c) for c in man.climit]
    assert len(limits) == 14
    per_v, per_p = {}, {}
    for L in sorted(set(limits) | {4}):
        idx, cts, values, R, non = class_items(b2.Manifest2([(4, L, L)]), np.zeros((2, 4), np.uint8),
                                               np.ascontiguousarray(fx.sn[:2, :4 * (2 * L + 4)]), fx.cts[:2, :4], L)
        n = len(idx)
        group.profile_begin()
        pr = rp.prove(group, fx.key, fx.qbar, L, cts, values, R, non)
        per_p[L] = group.profile_end().mont_ops / n
        group.profile_begin()
        rp.verify(group, fx.key, fx.qbar, L, cts, pr)
        per_v[L] = group.profile_end().mont_ops / n
    group.profile_begin()
    ok_s, ok_c, _ = verify(group, fx, fx.eb)
    got_v = group.profile_end().mont_ops / nb
    assert ok_s.all() and ok_c.all()
    want_v = sum(per_v[L] for L in limits)
    print(f"verify: {got_v:.1f} multiplies per ballot, the 14 range items' {want_v:.1f}")
    assert 0 < got_v <= want_v * (1 + 1e-9)
    group.profile_begin()
    b2.encrypt(group, fx.key, fx.qbar, man, fx.votes, fx.sn, fx.cn)
    got_e = group.profile_end().mont_ops / nb
    branch = per_p[4] - per_p[3]
    want_e = sum(per_p[L] for L in limits) + man.NS * branch
    print(f"encrypt: {got_e:.1f} multiplies per ballot, range prover {want_e - man.NS * branch:.1f} + "
          f"{man.NS} ciphertext jobs of {branch:.1f}")
    assert abs(got_e - want_e) <= 1e-6 * want_e


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_batch(group, fx):
    """Every refusal of the header on a live context, all four entry points.  That a refusal
    allocates nothing is not observable through the ABI; the 4 KB the pointers share would not
    survive a call that went on past the checks."""
    from electionguard.core import native
    lib, h = group._lib, group.handle
    K, qb = native.buf(fx.key.K_be), native.buf(fx.qbar.to_bytes(32, "big"))
    u32 = lambda v: np.array(v, np.uint32)
    p32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    buf = group.device_empty((4096,), np.uint8)
    d = buf.ptr

    def both(nc, nsel, ol, cl, nb=1, ptrs=None, what=b"ballot2"):
        nsel, ol, cl = u32(nsel), u32(ol), u32(cl)
        e = ptrs or [d] * 6
        v = ptrs or [d] * 7
        for name, args in (("eg_encrypt_ballots_v2", e), ("eg_encrypt_ballots_v2_dev", e),
                           ("eg_verify_ballots_v2", v), ("eg_verify_ballots_v2_dev", v)):
            args = args[:len(e) if "encrypt" in name else len(v)]
            rc = getattr(lib, name)(h, K, qb, nb, nc, p32(nsel), p32(ol), p32(cl), *args)
            assert rc == 1 and what in lib.eg_last_error(), (name, lib.eg_last_error())

    both(0, [1], [1], [1])                                  # no contest
    both(2, [3, 0], [1, 1], [1, 1])                          # a contest without selections
    both(1, [3], [0], [1]); both(1, [3], [16], [1])          # option limit outside 1..15
    both(1, [3], [1], [0]); both(1, [3], [1], [16])          # contest limit outside 1..15
    both(2, [1 << 20, 1], [1, 1], [1, 1])                    # NS > 2^20 (refused through J >= 2 NS > 2^16)
    both(1, [2200], [15], [15])                              # one ballot's jobs 66,030 > 2^16
    both(1, [3], [1], [1], ptrs=[None] * 7, what=b"null")    # required pointers
    for name, n in (("eg_encrypt_ballots_v2_dev", 6), ("eg_verify_ballots_v2_dev", 7)):
        args = [d] * n
        args[2] = d + 8                                      # a misaligned device row pointer
        rc = getattr(lib, name)(h, K, qb, 1, 1, p32(u32([3])), p32(u32([1])), p32(u32([1])), *args)
        assert rc == 1 and b"ballot2" in lib.eg_last_error() and b"aligned" in lib.eg_last_error()
    # a NULL shape array
    assert lib.eg_verify_ballots_v2(h, K, qb, 1, 1, None, p32(u32([1])), p32(u32([1])), *[d] * 7) == 1
    assert b"ballot2" in lib.eg_last_error()
    # nballots == 0: an all-ones tally and nothing else
    from electionguard import ballot2 as b2
    empty = b2.EncryptedBallots2(*(np.zeros((0,) + s, np.uint8) for s in
                                   ((fx.man.NS, 2, 512), (fx.man.SP, 2, 32), (fx.man.CP, 2, 32))))
    ok_s, ok_c, tally = b2.Verifier2(group, fx.key, fx.qbar, fx.man).verify(empty)
    assert ok_s.shape == (0, fx.man.NS) and ok_c.shape == (0, 4)
    assert np.array_equal(tally, products(fx.og, fx.cts[:0]))
    d_tally = group.device_empty((fx.man.NS, 2, 512), np.uint8)
    man = fx.man
    assert lib.eg_verify_ballots_v2_dev(h, K, qb, 0, 4, p32(man.nsel), p32(man.olimit), p32(man.climit), None, None,
                                        None, None, None, None, d_tally.ptr) == 0
    assert np.array_equal(d_tally.download(), tally)
    buf.free()
