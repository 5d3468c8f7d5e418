"""GPU: ballots of manifests whose contests differ in size (include/eg_hip_manifest.h,
electionguard.ballot.ElectionManifest) through the fused verifier, the encryptor and the tally.

A ragged oracle ballot is the concatenation of one-contest oracle ballots
(O.encrypt_ballot with O.Manifest(1, n_k, L_k) per contest, one shared rng), judged contest by
contest by O.verify_ballot.  Base shape M = (real selections, votes_allowed) per contest:
spc 3, 6, 2, 3 -- three distinct sizes, one size class with two non-adjacent members, and the
smallest possible gathered product (2)."""
import ctypes
import random

import numpy as np
import pytest

import eg_oracle as O
from conftest import be2i

pytestmark = pytest.mark.gpu

M = [(2, 1), (4, 2), (1, 1), (2, 1)]


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def _b(x, n):
    return np.frombuffer(int(x).to_bytes(n, "big"), np.uint8)


def _votes(mo, rng):
    """0..L real votes in the (single) contest; placeholders make its sum equal L."""
    k = rng.randrange(0, min(mo.votes_allowed, mo.n_selections) + 1)
    real = [0] * mo.n_selections
    for i in rng.sample(range(mo.n_selections), k):
        real[i] = 1
    return real + [1] * (mo.votes_allowed - k) + [0] * k


def _wire(ebs):
    """one-contest oracle ballots of ONE ragged ballot -> its (nsel,2,512), (nsel,4,32), (nc,2,32)"""
    cts = np.stack([np.stack([_b(ct.pad, 512), _b(ct.data, 512)]) for eb in ebs for ct in eb.cts])
    rp = np.stack([np.stack([_b(v, 32) for v in (pr.c0, pr.v0, pr.c1, pr.v1)]) for eb in ebs for pr in eb.proofs])
    cp = np.stack([np.stack([_b(eb.contest_proofs[0].c, 32), _b(eb.contest_proofs[0].v, 32)]) for eb in ebs])
    return cts, rp, cp


def _oracle_ballots(og, K, qbar, shape, nb, rng):
    """-> wire arrays of nb ragged oracle ballots, their votes, and the one-contest ballots"""
    per, votes = [], []
    for _ in range(nb):
        ebs, vs = [], []
        for n_k, L_k in shape:
            mo = O.Manifest(1, n_k, L_k)
            v = _votes(mo, rng)
            ebs.append(O.encrypt_ballot(og, K, qbar, mo, v, rng))
            vs += v
        per.append(ebs)
        votes.append(vs)
    w = [_wire(ebs) for ebs in per]
    return (np.stack([x[0] for x in w]), np.stack([x[1] for x in w]), np.stack([x[2] for x in w]),
            np.array(votes, np.uint8), per)


def _replay(og, shape, nb, state):
    """The votes and nonces _oracle_ballots drew from the rng in `state`: per contest its votes,
    per selection (R, u, c_fake, v_fake), then the contest's u."""
    r = random.Random()
    r.setstate(state)
    votes, sn, cn = [], [], []
    for _ in range(nb):
        vs, s4, c1 = [], [], []
        for n_k, L_k in shape:
            vs += _votes(O.Manifest(1, n_k, L_k), r)
            for _s in range(n_k + L_k):
                s4 += [r.randrange(1, og.q), r.randrange(1, og.q), r.randrange(og.q), r.randrange(og.q)]
            c1.append(r.randrange(1, og.q))
        votes.append(vs)
        sn.append(s4)
        cn.append(c1)
    to = lambda xs: np.frombuffer(b"".join(int(x).to_bytes(32, "big") for x in xs), np.uint8)
    return (np.array(votes, np.uint8), np.stack([to(b).reshape(-1, 4, 32) for b in sn]),
            np.stack([to(b).reshape(-1, 32) for b in cn]))


def _py_tally(cts, sels, cast=None):
    """CPython products over the (cast) ballots of the listed selections -> (len(sels), 2, 512)"""
    p = O.production_group().p
    rows = range(cts.shape[0]) if cast is None else np.flatnonzero(cast)
    out = np.zeros((len(sels), 2, 512), np.uint8)
    for i, s in enumerate(sels):
        for comp in range(2):
            acc = 1
            for b in rows:
                acc = acc * be2i(cts[b, s, comp]) % p
            out[i, comp] = _b(acc, 512)
    return out


def _gpu_ballots(group, key, qbar, man, nb, seed):
    from electionguard.ballot import batch_encryption, random_scalars, random_votes
    rng = np.random.default_rng(seed)
    votes = random_votes(rng, man, nb)
    sn = random_scalars(rng, (nb, man.nsel, 4), group.q)
    cn = random_scalars(rng, (nb, man.n_contests), group.q)
    return votes, sn, cn, batch_encryption(group, key, qbar, man, votes, sn, cn)


@pytest.fixture(scope="module")
def election(group):
    from electionguard.ballot import ElectionKey
    og = O.production_group()
    rng = random.Random(2024)
    _, K = O.key_ceremony(og, 2, 2, rng)
    return og, K, rng.randrange(og.q), ElectionKey(group, K)


@pytest.fixture(scope="module")
def oracle_m(election):
    """3 oracle ballots on M (about 2 s each), shared and left unchanged"""
    og, K, qbar, _ = election
    rng = random.Random(7)
    state = rng.getstate()
    cts, rp, cp, votes, per = _oracle_ballots(og, K, qbar, M, 3, rng)
    for a in (cts, rp, cp, votes):
        a.setflags(write=False)
    return state, cts, rp, cp, votes, per


@pytest.fixture(scope="module")
def gpu_m7(group, election):
    """7 GPU-encrypted ballots on M (the encryptor is tied to the oracle by the parity test)"""
    from electionguard.ballot import ElectionManifest
    _, _, qbar, key = election
    man = ElectionManifest(M)
    votes, sn, cn, eb = _gpu_ballots(group, key, qbar, man, 7, 11)
    for a in (eb.cts, eb.rproof, eb.cproof):
        a.setflags(write=False)
    return man, votes, sn, cn, eb


@pytest.fixture()
def fmt_group(group):
    yield group
    group.proof_format = ("minus", "message_first")


# ---------------------------------------------------------------------------------------------
# 1, 2: oracle parity and tamper localisation
# ---------------------------------------------------------------------------------------------
def test_oracle_parity(group, election, oracle_m):
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier, batch_encryption
    og, K, qbar, key = election
    state, cts, rp, cp, votes, per = oracle_m
    man = ElectionManifest(M)
    assert (man.nsel, man.n_contests, man.n_real) == (14, 4, 9)
    # the oracle accepts its own one-contest ballots (ballot 0: all four contests)
    for (n_k, L_k), eb in zip(M, per[0]):
        assert O.verify_ballot(og, K, qbar, O.Manifest(1, n_k, L_k), eb)
    ok_s, ok_c, tally = Verifier(group, key, qbar, man).verify(EncryptedBallots(cts, rp, cp))
    assert ok_s.shape == (3, 14) and ok_c.shape == (3, 4)
    assert ok_s.all() and ok_c.all()
    assert tally.shape == (9, 2, 512)
    want = [ct for k, (n_k, L_k) in enumerate(M)
            for ct in O.accumulate_tally(og, O.Manifest(1, n_k, L_k), [b[k] for b in per])]
    assert len(want) == 9
    for s, ct in enumerate(want):
        assert be2i(tally[s, 0]) == ct.pad and be2i(tally[s, 1]) == ct.data, s
    # the GPU encryptor with the oracle's injected nonces reproduces every byte
    v2, sn, cn = _replay(og, M, 3, state)
    assert np.array_equal(v2, votes)
    eb = batch_encryption(group, key, qbar, man, v2, sn, cn)
    assert np.array_equal(eb.cts, cts) and np.array_equal(eb.rproof, rp) and np.array_equal(eb.cproof, cp)


def test_tamper_localisation(group, election, oracle_m):
    from test_oracle_golden import forge_negated_alpha
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier
    og, K, qbar, key = election
    _, cts, rp, cp, _, _ = oracle_m
    man = ElectionManifest(M)
    V = Verifier(group, key, qbar, man)
    # a range-proof byte of contest 1's fifth selection (selection 3 + 4) of ballot 1
    t = rp.copy()
    t[1, 7, 1, 9] ^= 0x20
    ok_s, ok_c, _ = V.verify(EncryptedBallots(cts, t, cp), with_tally=False)
    assert np.argwhere(~ok_s).tolist() == [[1, 7]] and ok_c.all()
    # a contest-proof byte of contest 2 of ballot 2
    t = cp.copy()
    t[2, 2, 0, 17] ^= 0x01
    ok_s, ok_c, _ = V.verify(EncryptedBallots(cts, rp, t), with_tally=False)
    assert ok_s.all() and np.argwhere(~ok_c).tolist() == [[2, 2]]
    # limit[1] = 1 instead of 2: contest 1 of every ballot, nothing else
    wrong = ElectionManifest(M)
    wrong.limits[1] = 1
    ok_s, ok_c, _ = Verifier(group, key, qbar, wrong).verify(EncryptedBallots(cts, rp, cp), with_tally=False)
    assert ok_s.all() and np.argwhere(~ok_c).tolist() == [[0, 1], [1, 1], [2, 1]]
    # contest 3 of ballot 0 replaced by a forgery: the alpha of its last selection times p - 1 with
    # every Fiat-Shamir equation re-made to hold, so only the residue tests can reject it
    rng = random.Random(99)
    mo = O.Manifest(1, 2, 1)
    forged = forge_negated_alpha(og, K, qbar, mo, _votes(mo, rng), rng, 2)
    assert not O.is_valid_residue(og, forged.cts[2].pad)
    fc, fr, fp = _wire([forged])
    c2, r2, p2 = cts.copy(), rp.copy(), cp.copy()
    c2[0, 11:14], r2[0, 11:14], p2[0, 3] = fc, fr, fp[0]
    ok_s, ok_c, _ = V.verify(EncryptedBallots(c2, r2, p2), with_tally=False)
    assert np.argwhere(~ok_s).tolist() == [[0, 13]]
    assert np.argwhere(~ok_c).tolist() == [[0, 3]]


# ---------------------------------------------------------------------------------------------
# 3: a uniform shape through both sets of entry points
# ---------------------------------------------------------------------------------------------
def test_uniform_shape_bytes_equal_the_uniform_entries(group, election):
    from electionguard.ballot import ElectionManifest, Manifest, Verifier, batch_encryption
    _, _, qbar, key = election
    uni = Manifest(2, 3, 2)
    man = ElectionManifest([(3, 2), (3, 2)])
    assert man.spc_list.tolist() == [5, 5] and man.placeholders.tolist() == [2, 2] and man.limits.tolist() == [2, 2]
    votes, sn, cn, eb = _gpu_ballots(group, key, qbar, man, 7, 5)
    eu = batch_encryption(group, key, qbar, uni, votes, sn, cn)
    assert np.array_equal(eb.cts, eu.cts) and np.array_equal(eb.rproof, eu.rproof)
    assert np.array_equal(eb.cproof, eu.cproof)
    rp = eu.rproof.copy()
    rp[4, 6, 3, 3] ^= 0x40  # so the verdicts are not all alike
    eu.rproof = rp
    us, uc, ut = Verifier(group, key, qbar, uni).verify(eu)
    ms, mc, mt = Verifier(group, key, qbar, man).verify(eu)
    assert np.argwhere(~us).tolist() == [[4, 6]] and uc.all()
    assert np.array_equal(us, ms) and np.array_equal(uc, mc) and np.array_equal(ut, mt)


# ---------------------------------------------------------------------------------------------
# 4, 5: cast mask, empty batch, device-pointer entries
# ---------------------------------------------------------------------------------------------
def test_cast_mask_and_empty_batch(group, election, gpu_m7):
    from electionguard.ballot import EncryptedBallots, Verifier, accumulate_tally
    _, _, qbar, key = election
    man, _, _, _, eb = gpu_m7
    cast = np.array([1, 0, 1, 1, 0, 0, 1], bool)
    V = Verifier(group, key, qbar, man)
    ok_s, ok_c, tally = V.verify(eb, cast=cast)
    assert ok_s.shape == (7, 14) and ok_s.all() and ok_c.all()   # spoiled ballots are verified too
    want = _py_tally(eb.cts, man.real_index.tolist(), cast)
    assert np.array_equal(tally, want)
    assert np.array_equal(accumulate_tally(group, man, eb, cast), want)
    empty = EncryptedBallots(eb.cts[:0], eb.rproof[:0], eb.cproof[:0])
    ok_s, ok_c, tally = V.verify(empty)
    assert ok_s.shape == (0, 14) and ok_c.shape == (0, 4)
    one = np.zeros((9, 2, 512), np.uint8)
    one[:, :, 511] = 1
    assert np.array_equal(tally, one)


def test_device_pointer_entries_equal_host_entries(group, election, gpu_m7):
    from electionguard.ballot import Verifier, batch_encryption_device
    _, _, qbar, key = election
    man, votes, sn, cn, eb = gpu_m7
    nb = 7
    dv, dsn, dcn = (group.to_device(np.ascontiguousarray(x)) for x in (votes, sn, cn))
    oc, orp, ocp = (group.device_empty(x.shape) for x in (eb.cts, eb.rproof, eb.cproof))
    batch_encryption_device(group, key, qbar, man, nb, dv.ptr, dsn.ptr, dcn.ptr, oc.ptr, orp.ptr, ocp.ptr)
    assert np.array_equal(oc.download(), eb.cts)
    assert np.array_equal(orp.download(), eb.rproof)
    assert np.array_equal(ocp.download(), eb.cproof)
    cast = np.array([0, 1, 1, 0, 1, 1, 1], bool)
    rp = eb.rproof.copy()
    rp[5, 10, 0, 0] ^= 0x02           # contest 2's placeholder
    V = Verifier(group, key, qbar, man)
    from electionguard.ballot import EncryptedBallots
    hs, hc, ht = V.verify(EncryptedBallots(eb.cts, rp, eb.cproof), cast=cast)
    assert np.argwhere(~hs).tolist() == [[5, 10]] and hc.all()
    d_rp = group.to_device(rp)
    dm = group.to_device(cast.astype(np.uint8))
    oks, okc, tal = group.device_zeros((nb, 14)), group.device_zeros((nb, 4)), group.device_zeros((9, 2, 512))
    V.verify_device(oc.ptr, d_rp.ptr, ocp.ptr, nb, oks.ptr, okc.ptr, tal.ptr, dm.ptr)
    group.sync()
    assert np.array_equal(oks.download().astype(bool), hs)
    assert np.array_equal(okc.download().astype(bool), hc)
    assert np.array_equal(tal.download(), ht)


# ---------------------------------------------------------------------------------------------
# 6, 7: a contest longer than one product pass; a batch crossing the verifier's chunk
# ---------------------------------------------------------------------------------------------
def test_long_contest(group, election):
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier
    og, K, qbar, key = election
    man = ElectionManifest([(39, 1), (1, 1)])     # spc 40: a two-pass aggregate, gather 40
    assert man.nsel == 42
    _, _, _, eb = _gpu_ballots(group, key, qbar, man, 2, 17)
    V = Verifier(group, key, qbar, man)
    ok_s, ok_c, tally = V.verify(eb)
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(tally[[0, 38, 39]], _py_tally(eb.cts, [0, 38, 40]))
    A = B = 1
    for s in range(40):
        A = A * be2i(eb.cts[0, s, 0]) % og.p
        B = B * be2i(eb.cts[0, s, 1]) % og.p
    pr = O.GenericProof(be2i(eb.cproof[0, 0, 0]), be2i(eb.cproof[0, 0, 1]))
    assert O.verify_constant_proof(og, K, qbar, A, B, 1, pr)
    cts = eb.cts.copy()
    cts[1, 37, 1, 200] ^= 0x08
    ok_s, ok_c, _ = V.verify(EncryptedBallots(cts, eb.rproof, eb.cproof), with_tally=False)
    assert np.argwhere(~ok_s).tolist() == [[1, 37]]
    assert np.argwhere(~ok_c).tolist() == [[1, 0]]


def test_chunk_crossing(group, election):
    """nsel = 203 lowers the chunk to 2^21 // 203 = 10,330 ballots, so 10,360 ballots run as two
    verify chunks and two encryption chunks (as test_wide_manifest_smaller_chunks, ragged)."""
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier, batch_encryption
    _, _, qbar, key = election
    man = ElectionManifest([(200, 1), (1, 1)])
    chunk = (1 << 21) // man.nsel
    assert man.nsel == 203 and chunk == 10330
    nb = 10360
    votes, sn, cn, eb = _gpu_ballots(group, key, qbar, man, nb, 83)
    a, b = 10326, 10335
    part = batch_encryption(group, key, qbar, man, votes[a:b], sn[a:b], cn[a:b])
    assert np.array_equal(part.cts, eb.cts[a:b]) and np.array_equal(part.rproof, eb.rproof[a:b])
    assert np.array_equal(part.cproof, eb.cproof[a:b])
    rp = eb.rproof.copy()
    rp[10341, 150, 0, 7] ^= 0x10
    ok_s, ok_c, tally = Verifier(group, key, qbar, man).verify(EncryptedBallots(eb.cts, rp, eb.cproof))
    assert np.argwhere(~ok_s).tolist() == [[10341, 150]] and ok_c.all()
    assert tally.shape == (201, 2, 512)
    # real selections 0, 117 and the last one (selection 201, the second contest's)
    assert np.array_equal(tally[[0, 117, 200]], _py_tally(eb.cts, [0, 117, 201]))


# ---------------------------------------------------------------------------------------------
# 8: the other response sign and pre-image order (the per-contest L table meets the in-place negation)
# ---------------------------------------------------------------------------------------------
def test_proof_format_switches(fmt_group, election):
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier, batch_encryption
    group = fmt_group
    og, K, qbar, key = election
    man = ElectionManifest(M)
    rng = random.Random(31)
    state = rng.getstate()
    with O.proof_format("plus", "with_key"):
        cts, rp, cp, votes, per = _oracle_ballots(og, K, qbar, M, 3, rng)
        assert O.verify_ballot(og, K, qbar, O.Manifest(1, 4, 2), per[0][1])
    V = Verifier(group, key, qbar, man)
    ok_s, ok_c, _ = V.verify(EncryptedBallots(cts, rp, cp), with_tally=False)
    assert not ok_s.any() and not ok_c.any()          # the default convention rejects every proof
    group.proof_format = ("plus", "with_key")
    ok_s, ok_c, tally = V.verify(EncryptedBallots(cts, rp, cp))
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(tally, _py_tally(cts, man.real_index.tolist()))
    wrong = ElectionManifest(M)
    wrong.limits[1] = 1
    ok_s, ok_c, _ = Verifier(group, key, qbar, wrong).verify(EncryptedBallots(cts, rp, cp), with_tally=False)
    assert ok_s.all() and np.argwhere(~ok_c).tolist() == [[0, 1], [1, 1], [2, 1]]
    v2, sn, cn = _replay(og, M, 3, state)
    eb = batch_encryption(group, key, qbar, man, v2, sn, cn)
    assert np.array_equal(eb.cts, cts) and np.array_equal(eb.rproof, rp) and np.array_equal(eb.cproof, cp)


# ---------------------------------------------------------------------------------------------
# 9: ballot styles
# ---------------------------------------------------------------------------------------------
def test_ballot_styles(group, election):
    from electionguard.ballot import ElectionManifest, Verifier, merge_style_tallies
    _, _, qbar, key = election
    man = ElectionManifest(M)
    styles = [([0, 1, 3], 4, 41), ([1, 2], 3, 42)]
    parts, ballots = [], []
    for idx, nb, seed in styles:
        st = man.style(idx)
        _, _, _, eb = _gpu_ballots(group, key, qbar, st, nb, seed)
        ok_s, ok_c, tally = Verifier(group, key, qbar, st).verify(eb)
        assert ok_s.all() and ok_c.all() and tally.shape == (st.n_real, 2, 512)
        parts.append((idx, tally))
        ballots.append((st, eb))
    merged = merge_style_tallies(group, man, parts)
    assert merged.shape == (9, 2, 512)
    p = O.production_group().p
    row = 0
    for k, c in enumerate(man.contests):
        for s in range(c.n_selections):
            acc, n = [1, 1], 0
            for (idx, _, _), (st, eb) in zip(styles, ballots):
                if k in idx:
                    pos = int(st.offsets[idx.index(k)]) + s
                    n += eb.n
                    for b in range(eb.n):
                        for comp in range(2):
                            acc[comp] = acc[comp] * be2i(eb.cts[b, pos, comp]) % p
            assert n == {0: 4, 1: 7, 2: 3, 3: 4}[k]
            assert [be2i(merged[row, 0]), be2i(merged[row, 1])] == acc, (k, s)
            row += 1
    # a contest that no style covers stays 1
    only = merge_style_tallies(group, man, parts[1:])
    assert all(be2i(only[r, c]) == 1 for r in (0, 1, 7, 8) for c in range(2))
    assert np.array_equal(only[2:7], parts[1][1])


# ---------------------------------------------------------------------------------------------
# 10: argument validation
# ---------------------------------------------------------------------------------------------
def test_argument_validation(group, election, oracle_m):
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier
    _, K, qbar, key = election
    _, cts, rp, cp, _, _ = oracle_m
    lib = group._lib
    one = ctypes.create_string_buffer(1024)
    u32 = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)
    bad = [
        ("no contests", [], [], []),
        ("an empty contest", [3, 0, 2], [1, 0, 1], [1, 0, 1]),
        ("placeholders fill a contest", [3, 2, 2], [1, 2, 1], [1, 1, 1]),
        ("too many selections", [1 << 20, 1], [1, 0], [1, 1]),
    ]
    V = Verifier(group, key, qbar, ElectionManifest(M))
    for what, spc, ph, lim in bad:
        n = len(spc)
        for dev in (False, True):
            fn = lib.eg_verify_ballots_manifest_dev if dev else lib.eg_verify_ballots_manifest
            rc = fn(group.handle, one, one, 1, n, u32(spc), u32(ph), u32(lim), one, one, one, None, one, one, None)
            assert rc == 1 and b"manifest" in lib.eg_last_error(), (what, dev)
        if what != "placeholders fill a contest":   # the encryptor takes no placeholder counts
            for fn in (lib.eg_encrypt_ballots_manifest, lib.eg_encrypt_ballots_manifest_dev):
                rc = fn(group.handle, one, one, 1, n, u32(spc), one, one, one, one, one, one)
                assert rc == 1 and b"manifest" in lib.eg_last_error(), what
        # the context is still usable
        ok_s, ok_c, _ = V.verify(EncryptedBallots(cts, rp, cp), with_tally=False)
        assert ok_s.all() and ok_c.all(), what


# ---------------------------------------------------------------------------------------------
# the k_pow launch plan of the table-addressed path
# ---------------------------------------------------------------------------------------------
def test_launch_split_independent_table_path(group, election, monkeypatch):
    """The table-addressed verifier shares the uniform one's beta head (the first betas ride in
    launch 1 to fill its last round of resident workgroups).  Three classes, nsel = 15, 12
    ballots: 180 selection jobs = 6 workgroups; EG_POW_SLOTS = 0 (no head), 4 (a head of 64
    jobs) and 5 (128) move the split.  Verdicts and tally must not depend on it, against the
    CPython product and a tamper on each side of the contest layer."""
    from electionguard.ballot import ElectionManifest, EncryptedBallots, Verifier
    _, _, qbar, key = election
    man = ElectionManifest([(2, 1), (7, 3), (1, 1)])
    assert man.nsel == 15 and len(set(man.spc_list.tolist())) == 3
    nb = 12
    _, _, _, eb = _gpu_ballots(group, key, qbar, man, nb, 23)
    want = _py_tally(eb.cts, man.real_index.tolist())
    rp, cp = eb.rproof.copy(), eb.cproof.copy()
    rp[0, 4, 2, 6] ^= 0x10     # a selection of ballot 0 (a beta-head job when split)
    cp[11, 1, 1, 8] ^= 0x01    # the 10-selection contest of the last ballot
    V = Verifier(group, key, qbar, man)
    base = None
    for slots in ("0", "4", "5"):
        monkeypatch.setenv("EG_POW_SLOTS", slots)
        ok_s, ok_c, tally = V.verify(eb)
        assert ok_s.all() and ok_c.all(), slots
        assert np.array_equal(tally, want), slots
        if base is None:
            base = (ok_s, ok_c, tally)
        assert all(np.array_equal(x, y) for x, y in zip((ok_s, ok_c, tally), base)), slots
        ok_s, ok_c, _ = V.verify(EncryptedBallots(eb.cts, rp, eb.cproof), with_tally=False)
        assert np.argwhere(~ok_s).tolist() == [[0, 4]] and ok_c.all(), slots
        ok_s, ok_c, _ = V.verify(EncryptedBallots(eb.cts, eb.rproof, cp), with_tally=False)
        assert ok_s.all() and np.argwhere(~ok_c).tolist() == [[11, 1]], slots
