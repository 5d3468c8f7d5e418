"""GPU: the threshold decryption with one combined proof per text (include/eg_hip_decrypt2.h,
electionguard.decrypt2): every output byte of commit, combine, respond, check and verify against
the CPython reference tests/decrypt2_ref.py, host and _dev variants alike.

The reference costs about ten milliseconds per modular power, so the shapes are the smallest that
reach every path: the texts and nonces of the 257-text case repeat with period 7 (7 distinct
reference computations, and 256 is no multiple of 7, so a text index that wraps at a block shows),
the larger quorums take one or two texts, and the chunk-crossing run checks four rows against
CPython and the rest against the protocol's own checks."""
import json
import random
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import decrypt2_ref as R

pytestmark = pytest.mark.gpu

QBAR = 0xD2C0FFEE
U8 = np.uint8


def be(x, n=512):
    return np.frombuffer(int(x).to_bytes(n, "big"), U8)


def P(xs):
    return np.stack([be(x) for x in xs])


def Q(xs):
    return np.stack([be(x, 32) for x in xs])


def arrays(run):
    """The lists of a reference run in the library's layouts."""
    return SimpleNamespace(
        T=np.stack([np.stack([be(A), be(B)]) for A, B in run.texts]),
        shares=np.stack([P(row) for row in run.shares]),
        comm=np.stack([np.stack([np.stack([be(a), be(b)]) for a, b in row]) for row in run.comm]),
        ci=np.stack([Q(row) for row in run.ci]), vi=np.stack([Q(row) for row in run.vi]),
        M=P(run.M), proofs=np.stack([np.stack([be(c, 32), be(v, 32)]) for c, v in run.proofs]))


def eq(got, want):
    got = got.download() if hasattr(got, "download") else got
    return np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))


def mediator_calls(group, K, qbar, run, a, up=lambda x: x):
    """combine, check and verify on the arrays a (through up: host arrays or device buffers)
    against the reference run -> their outputs."""
    from electionguard import decrypt2 as D
    T, shares, comm = up(a.T), up(a.shares), up(a.comm)
    M, c, ci = D.combine(group, K, qbar, run.w, T, shares, comm)
    ok, v = D.check(group, run.Z, T, shares, comm, up(a.ci), up(a.vi))
    okv = D.verify(group, K, qbar, T, up(a.M), up(a.proofs))
    return M, c, ci, ok, v, okv


def assert_equals_reference(group, K, qbar, run, trustee=True):
    """Every byte of every call against the run; the _dev variants against the host variants."""
    from electionguard import decrypt2 as D
    a = arrays(run)
    n, k = len(run.texts), len(run.xs)
    if trustee:
        for i in range(k):
            M, aa, bb = D.commit(group, run.z[i], a.T[:, 0], Q(run.nonces[i]))
            assert eq(M, a.shares[:, i]) and eq(aa, a.comm[:, i, 0]) and eq(bb, a.comm[:, i, 1]), i
            assert eq(D.respond(group, run.z[i], Q(run.nonces[i]), a.ci[:, i]), a.vi[:, i]), i
    M, c, ci, ok, v, okv = mediator_calls(group, K, qbar, run, a)
    want_M, want_c, want_ci = R.combine(group.p, group.q, K, qbar, run.w, run.texts, run.shares, run.comm,
                                        group.hash_format)
    assert eq(M, P(want_M)) and eq(c, Q(want_c)) and eq(ci, np.stack([Q(r) for r in want_ci]))
    assert M.shape == (n, 512) and c.shape == (n, 32) and ci.shape == (n, k, 32)
    assert ok.dtype == bool and ok.tolist() == run.ok
    want_v = R.check(group.p, group.q, group.g, run.Z, run.texts, run.shares, run.comm, run.ci, run.vi)[1]
    assert eq(v, Q(want_v))
    assert okv.tolist() == run.verified
    dev = mediator_calls(group, K, qbar, run, a, group.to_device)
    for host_out, dev_out in zip((M, c, ci, ok, v, okv), dev):
        assert hasattr(dev_out, "download") and eq(dev_out, host_out.astype(U8))


def edge_texts(group, rng, n, period=None):
    p = group.p
    As = [1, group.g, p - 1, 0, p + 5, rng.randrange(2, p)] + [rng.randrange(2, p) for _ in range(3)]
    base = [(A, rng.randrange(p)) for A in As[:period or n]]
    return [base[t % len(base)] for t in range(n)]


def nonce_rows(group, rng, k, n, period=None, edges=False):
    q = group.q
    per = period or n
    rows = [[rng.randrange(q) for _ in range(per)] for _ in range(k)]
    if edges:
        for t, u in enumerate([0, 1, q - 1, q, 2**256 - 1][:per]):
            rows[t % k][t] = u
    return [[row[t % per] for t in range(n)] for row in rows]


# (guardians, quorum, available x's, n, period)
CASES = {
    "1of1_n257": (1, 1, [1], 257, 7),
    "2of3_n9": (3, 2, [1, 3], 9, None),
    "3of5_n1": (5, 3, [2, 3, 5], 1, None),
    "5of5_n2": (5, 3, [1, 2, 3, 4, 5], 2, None),
}


@pytest.fixture(scope="module")
def ceremonies(group):
    """One CPython ceremony per (guardians, quorum); never modified."""
    rng = random.Random(41)
    return {(n_g, qu): R.ceremony(group.p, group.q, group.g, n_g, qu, rng) for n_g, qu in ((1, 1), (3, 2), (5, 3))}


@pytest.mark.parametrize("case", list(CASES))
def test_every_byte_against_the_reference(group, ceremonies, case):
    n_g, quorum, xs, n, period = CASES[case]
    rng = random.Random(n * 31 + n_g)
    cer = ceremonies[(n_g, quorum)]
    texts = edge_texts(group, rng, 5)[1::3] if n == 2 else edge_texts(group, rng, n, period)   # n = 2: A = g, p + 5
    nonces = nonce_rows(group, rng, len(xs), n, period, edges=(n == 9))
    run = R.run(cer, QBAR, xs, texts, nonces)
    assert_equals_reference(group, cer.K, QBAR, run)
    if n == 1:                                    # an honest text of order q passes everything
        A = pow(group.g, 12345, group.p)
        honest = R.run(cer, QBAR, xs, [(A, pow(cer.K, 12345, group.p) * group.g % group.p)], nonces, limit=3)
        assert honest.ok == [[True] * 3] and honest.verified == [True] and honest.counts == [1]
        assert_equals_reference(group, cer.K, QBAR, honest)


def test_edge_nonces_challenges_and_secrets(group):
    """commit and respond with u, c in {0, 1, q-1, q, 2^256-1} and z in {1, q-1}: the powers take the
    scalars as given, the response reduces all three mod q."""
    from electionguard import decrypt2 as D
    p, q, g = group.p, group.q, group.g
    edges = [0, 1, q - 1, q, 2**256 - 1]
    rng = random.Random(6)
    pads = [rng.randrange(2, p), p + 5, 0, 1, g]
    for z in (1, q - 1):
        M, a, b = D.commit(group, z, P(pads), Q(edges))
        wM, wa, wb = R.commit(p, g, z, pads, edges)
        assert eq(M, P(wM)) and eq(a, P(wa)) and eq(b, P(wb)), z
        for shift in range(5):
            chal = edges[shift:] + edges[:shift]
            assert eq(D.respond(group, z, Q(edges), Q(chal)), Q(R.respond(q, z, edges, chal))), (z, shift)
    assert eq(D.respond(group, 2**256 - 1, Q(edges), Q(edges)), Q(R.respond(q, 2**256 - 1, edges, edges)))


def test_both_hash_formats(group, ceremonies):
    """A = 1 supplies the leading zero bytes the minimal format drops."""
    cer = ceremonies[(3, 2)]
    rng = random.Random(8)
    texts = [(1, 5), (group.g, rng.randrange(group.p)), (rng.randrange(group.p), 0)]
    nonces = nonce_rows(group, rng, 2, 3)
    fixed = R.run(cer, QBAR, [2, 3], texts, nonces, "fixed")
    minimal = R.run(cer, QBAR, [2, 3], texts, nonces, "minimal")
    assert all(x != y for x, y in zip(fixed.c, minimal.c))
    assert group.hash_format == "fixed"
    try:
        group.hash_format = "minimal"
        assert_equals_reference(group, cer.K, QBAR, minimal)
    finally:
        group.hash_format = "fixed"
    assert_equals_reference(group, cer.K, QBAR, fixed, trustee=False)


def test_the_proof_format_does_not_apply(group, ceremonies):
    cer = ceremonies[(3, 2)]
    rng = random.Random(8)
    texts = [(1, 5), (group.g, rng.randrange(group.p)), (rng.randrange(group.p), 0)]
    run = R.run(cer, QBAR, [2, 3], texts, nonce_rows(group, rng, 2, 3))          # the run of the test above
    before = group.proof_format
    try:
        group.proof_format = ("plus", "commitments_first")
        assert_equals_reference(group, cer.K, QBAR, run)
    finally:
        group.proof_format = before


def _other_groups():
    gs = json.loads((Path(__file__).resolve().parent / "golden" / "test_groups.json").read_text())["groups"]
    return ["Mode4096_V2", gs[0]["name"]]


@pytest.mark.parametrize("name", _other_groups())
def test_other_groups(name):
    from electionguard.core import GroupContext, productionGroup
    if name == "Mode4096_V2":
        G, own = productionGroup(0, "Mode4096_V2"), False
    else:
        gd = next(g for g in json.loads((Path(__file__).resolve().parent / "golden" / "test_groups.json")
                                        .read_text())["groups"] if g["name"] == name)
        G, own = GroupContext(int(gd["p"], 16), int(gd["q"], 16), int(gd["g"], 16)), True
    try:
        rng = random.Random(12)
        cer = R.ceremony(G.p, G.q, G.g, 3, 2, rng)
        r = rng.randrange(1, G.q)
        texts = [(pow(G.g, r, G.p), pow(cer.K, r, G.p) * pow(G.g, 2, G.p) % G.p), (G.p + 5, rng.randrange(G.p))]
        run = R.run(cer, QBAR % G.q, [1, 2], texts, nonce_rows(G, rng, 2, 2), limit=3)
        assert run.ok[0] == [True, True] and run.verified[0] and run.counts[0] == 2
        assert_equals_reference(G, cer.K, QBAR % G.q, run)
    finally:
        if own:
            G.close()


@pytest.fixture(scope="module")
def tamper_world(group, ceremonies):
    rng = random.Random(19)
    cer = ceremonies[(3, 2)]
    texts = []
    for t in range(3):
        r = rng.randrange(1, group.q)
        texts.append((pow(group.g, r, group.p), pow(cer.K, r, group.p) * pow(group.g, t, group.p) % group.p))
    return SimpleNamespace(cer=cer, texts=texts, nonces=nonce_rows(group, rng, 2, 3), xs=[1, 2])


@pytest.mark.parametrize("kind", list(R.TAMPERINGS))
def test_a_tampering_flips_exactly_its_flags(group, tamper_world, kind):
    from electionguard import decrypt2 as D
    w, t, i = tamper_world, 1, 1
    run, bad_items, bad_texts = R.tampered(w.cer, QBAR, w.xs, w.texts, w.nonces, kind, t, i)
    a = arrays(run)
    for up in (lambda x: x, group.to_device):
        ok, v = D.check(group, run.Z, up(a.T), up(a.shares), up(a.comm), up(a.ci), up(a.vi))
        okv = D.verify(group, w.cer.K, QBAR, up(a.T), up(a.M), up(a.proofs))
        ok, okv = (np.asarray(x.download() if hasattr(x, "download") else x).astype(bool) for x in (ok, okv))
        assert {(tt, ii) for tt in range(3) for ii in range(2) if not ok[tt, ii]} == bad_items
        assert {tt for tt in range(3) if not okv[tt]} == bad_texts
        assert ok.tolist() == run.ok and okv.tolist() == run.verified
        if not kind.startswith("pub"):
            assert eq(v, Q(run.v))


# ---- the mediator classes ------------------------------------------------------------------------
def guardian_keys(cer, x):
    from electionguard.keyceremony import GuardianKeys
    j = x - 1
    keys = GuardianKeys(f"guardian{x}", x, cer.coeffs[j], cer.commitments[j])
    for l in range(cer.n):
        if l != j:
            keys.shares_from[f"guardian{l + 1}"] = R.poly_eval(cer.coeffs[l], x, cer.q)
    return keys


def encrypt_counts(group, K, counts, rng):
    rs = [rng.randrange(1, group.q) for _ in counts]
    pad = group.gPowP_batch(rs)
    Kr = group.powP_batch([K] * len(rs), rs)
    data = group.multP_batch(Kr, group.gPowP_batch(counts))
    return np.ascontiguousarray(np.stack([pad, data], axis=1))


def test_the_same_tally_through_1_0_and_2_0(group, ceremonies):
    """5 guardians, quorum 3, 2 missing: Decryption (1.0) and Decryption2 give byte-identical M and
    equal counts; the record verifies, and an altered count, M or proof does not."""
    from electionguard import decrypt2 as D
    from electionguard.decrypt import DecryptingTrustee, Decryption
    cer = ceremonies[(5, 3)]
    rng = random.Random(23)
    counts = [0, 7, 3, 10]
    T = encrypt_counts(group, cer.K, counts, rng)
    keys = {x: guardian_keys(cer, x) for x in cer.xs}
    comm = {k.gid: k.commitments for k in keys.values()}
    avail = [1, 3, 4]
    share_keys = D.share_public_keys(group, comm, {keys[x].gid: x for x in avail})
    assert [share_keys[keys[x].gid] for x in avail] == [pow(group.g, R.key_share(cer, x), group.p) for x in avail]
    assert [D.key_share(keys[x], group.q) for x in avail] == [R.key_share(cer, x) for x in avail]
    old = Decryption(group, QBAR, [DecryptingTrustee(group, keys[x], comm) for x in avail],
                     [keys[x].gid for x in (2, 5)], {k.gid: k.public_key for k in keys.values()})
    rec1, M1 = old._shares_and_combine(T)
    dec = D.Decryption2(group, QBAR, cer.K, [D.DecryptingTrustee2(group, keys[x]) for x in avail], share_keys)
    rec = dec.decrypt_record(T, 10)
    assert eq(rec.M, M1) and rec.counts == counts == old.decrypt(T, 10)
    assert rec.M.shape == (4, 512) and rec.proofs.shape == (4, 2, 32) and rec.xs == {keys[x].gid: x for x in avail}
    assert dec.decrypt(T, 10) == counts
    assert D.verify_decryption_record2(group, QBAR, cer.K, rec, 10) == {"proofs": True, "tally": True}
    assert D.verify_decryption_record2(group, QBAR, cer.K, rec, 9) == {"proofs": True, "tally": False}
    bad = D.DecryptionRecord2(rec.texts, rec.xs, rec.M, rec.proofs, [0, 7, 4, 10])
    assert D.verify_decryption_record2(group, QBAR, cer.K, bad, 10) == {"proofs": True, "tally": False}
    pr = rec.proofs.copy()
    pr[2, 1, 31] ^= 1
    bad = D.DecryptionRecord2(rec.texts, rec.xs, rec.M, pr, rec.counts)
    assert D.verify_decryption_record2(group, QBAR, cer.K, bad, 10) == {"proofs": False, "tally": True}
    # a guardian answering with a wrong share is named
    liar = D.DecryptingTrustee2(group, keys[3])
    liar.z = (liar.z + 1) % group.q
    dec = D.Decryption2(group, QBAR, cer.K, [D.DecryptingTrustee2(group, keys[1]), liar,
                                            D.DecryptingTrustee2(group, keys[4])], share_keys)
    with pytest.raises(ValueError, match="guardian3"):
        dec.decrypt(T, 10)


def test_ballots_with_an_option_limit_of_3_and_contest_data_come_back(group):
    from electionguard import ballot2 as b2
    from electionguard import contest_data as CD
    from electionguard import decrypt2 as D
    from electionguard.ballot import ElectionKey
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=11)
    key, man = ElectionKey(group, K), b2.Manifest2([(2, 3, 3), (1, 1, 1)])
    votes = np.array([[3, 0, 1], [1, 2, 0]], U8)
    sn, cn = b2.random_nonces2(np.random.default_rng(4), man, 2, group.q)
    eb = b2.encrypt(group, key, QBAR, man, votes, sn, cn)
    comm = {g.gid: g.commitments for g in gk}
    avail = [gk[0], gk[2]]
    share_keys = D.share_public_keys(group, comm, {g.gid: g.x for g in avail})
    dec = D.Decryption2(group, QBAR, K, [D.DecryptingTrustee2(group, g) for g in avail], share_keys)
    assert np.array_equal(dec.decryptBallots(eb, man), votes)
    rec = dec.decrypt_ballots_record(eb, man)
    assert rec.counts == votes.reshape(-1).tolist()
    assert D.verify_decryption_record2(group, QBAR, K, rec, 3) == {"proofs": True, "tally": True}
    # sealed contest data: 2 ballots x 2 contests x 32 bytes
    rng = np.random.default_rng(5)
    ids, data = rng.integers(0, 256, (2, 32), U8), rng.integers(0, 256, (4, 32), U8)
    r = Q([random.Random(3 + j).randrange(1, group.q) for j in range(4)])
    c0, c1, c2 = CD.seal(group, key, 2, 32, ids, r, data)
    got, ok = dec.decryptContestData(c0, c1, c2, ids, 2)
    assert ok.all() and np.array_equal(got.reshape(4, 32), data)
    c2 = c2.copy()
    c2.reshape(-1, 32)[3, 0] ^= 1
    got, ok = dec.decryptContestData(c0, c1, c2, ids, 2)
    assert ok.reshape(-1).tolist() == [True, True, True, False]


def test_a_run_that_crosses_the_chunk(group, ceremonies):
    """k = 2 and one text more than a chunk through the host variants: rows 0, chunk - 1, chunk and
    n - 1 against CPython, every other row accepted by check and verify, M, c and v byte-equal to
    the _dev run (whose chunks are the same, on the caller's buffers)."""
    from electionguard import decrypt2 as D
    cer, xs, k = ceremonies[(3, 2)], [1, 3], 2
    ch = D.chunk_texts(k)
    n = ch + 1
    assert n * k <= 20000
    rs = np.random.default_rng(7)

    def rand_q(m):
        a = rs.integers(0, 256, (m, 32), U8)
        a[:, 0] &= 0x7F                            # below q, whatever the group
        return a

    T = np.ascontiguousarray(np.stack([group.gPowP_batch(rand_q(n)), group.gPowP_batch(rand_q(n))], axis=1))
    z = [R.key_share(cer, x) for x in xs]
    Z = [pow(group.g, zi, group.p) for zi in z]
    w = [R.lagrange(xs, x, group.q) for x in xs]
    U = [rand_q(n) for _ in xs]
    r1 = [D.commit(group, z[i], T[:, 0], U[i]) for i in range(k)]
    shares = np.ascontiguousarray(np.stack([r[0] for r in r1], axis=1))
    comm = np.ascontiguousarray(np.stack([np.stack([r[1], r[2]], axis=1) for r in r1], axis=1))
    M, c, ci = D.combine(group, cer.K, QBAR, w, T, shares, comm)
    vi = np.ascontiguousarray(np.stack([D.respond(group, z[i], U[i], ci[:, i]) for i in range(k)], axis=1))
    ok, v = D.check(group, Z, T, shares, comm, ci, vi)
    proofs = np.ascontiguousarray(np.stack([c, v], axis=1))
    okv = D.verify(group, cer.K, QBAR, T, M, proofs)
    assert ok.shape == (n, k) and ok.all() and okv.shape == (n,) and okv.all()
    up = group.to_device
    dT, dS, dC = up(T), up(shares), up(comm)
    dM, dc, dci = D.combine(group, cer.K, QBAR, w, dT, dS, dC)
    dok, dv = D.check(group, Z, dT, dS, dC, dci, up(vi))
    dokv = D.verify(group, cer.K, QBAR, dT, dM, up(proofs))
    assert eq(dM, M) and eq(dc, c) and eq(dci, ci) and eq(dv, v)
    assert dok.download().all() and dokv.download().all()
    rows = [0, ch - 1, ch, n - 1]
    ints = lambda a: [int.from_bytes(bytes(r), "big") for r in np.asarray(a).reshape(-1, a.shape[-1])]
    texts = [tuple(ints(T[r])) for r in rows]
    run = R.run(cer, QBAR, xs, texts, [ints(U[i][rows]) for i in range(k)])
    a = arrays(run)
    assert eq(shares[rows], a.shares) and eq(comm[rows], a.comm) and eq(M[rows], a.M)
    assert eq(ci[rows], a.ci) and eq(vi[rows], a.vi) and eq(proofs[rows], a.proofs)
    assert run.ok == [[True, True]] * 4 and run.verified == [True] * 4
    # one altered response beyond the first chunk is found where it is, and nowhere else
    vi[ch, 1, 31] ^= 1
    ok, _ = D.check(group, Z, T, shares, comm, ci, vi)
    assert not ok[ch, 1] and ok.sum() == n * k - 1


def test_check_on_the_guardians_tables_against_the_reference(group, ceremonies):
    """k = 2 and n = 8193: at 8192 texts and more the check reads Z_i^c from the guardians' cached
    radix tables, with guardian-major jobs, here in one full chunk of 8192 texts and a second of
    one.  The rows tile 24 texts of one CPython run, five edge texts (A = 1, g, p - 1, 0, p + 5) and
    19 encryptions; a c_i, a v_i and a commitment of encryptions are altered in both chunks and on
    both guardians, and every ok flag and v sum comes from the reference."""
    from electionguard import decrypt2 as D
    cer, xs, k, per = ceremonies[(3, 2)], [1, 3], 2, 24
    p, q, g = group.p, group.q, group.g
    n = D.chunk_texts(k) + 1
    assert n == 8193
    rng = random.Random(53)
    texts = edge_texts(group, rng, 5)
    for t in range(per - 5):
        r = rng.randrange(1, q)
        texts.append((pow(g, r, p), pow(cer.K, r, p) * pow(g, t, p) % p))
    run = R.run(cer, QBAR, xs, texts, nonce_rows(group, rng, k, per))
    assert run.ok[5:] == [[True] * k] * (per - 5) and run.ok[:5] != [[True] * k] * 5
    a = arrays(run)
    idx = np.arange(n) % per
    T, shares, comm, ci, vi = (np.ascontiguousarray(x[idx]) for x in (a.T, a.shares, a.comm, a.ci, a.vi))
    # (row, guardian, what): rows 0..8191 are the first chunk, row 8192 the second
    tamperings = [(6, 0, "ci"), (101, 1, "ci=q"), (4097, 1, "vi"), (8191, 0, "ai"), (8192, 0, "vi"), (8192, 1, "bi")]
    assert all(r % per >= 5 for r, _, _ in tamperings)
    want_ok = np.array(run.ok, bool)[idx]
    want_v = Q(run.v)[idx]
    for row in sorted({r for r, _, _ in tamperings}):
        t = row % per
        sh, cm = list(run.shares[t]), [list(x) for x in run.comm[t]]
        cr, vr = list(run.ci[t]), list(run.vi[t])
        for r, i, what in tamperings:
            if r != row:
                continue
            if what == "ci":
                cr[i] = (cr[i] + 1) % q
            elif what == "ci=q":
                cr[i] = q
            elif what == "vi":
                vr[i] = (vr[i] + 1) % q
            else:
                cm[i]["ab".index(what[0])] = cm[i]["ab".index(what[0])] * g % p
        ok1, v1 = R.check(p, q, g, run.Z, [run.texts[t]], [sh], [cm], [cr], [vr])
        assert ok1[0] == [not any(r == row and j == i for r, j, _ in tamperings) for i in range(k)], row
        want_ok[row], want_v[row] = ok1[0], be(v1[0], 32)
        comm[row], ci[row], vi[row] = np.stack([np.stack([be(x), be(y)]) for x, y in cm]), Q(cr), Q(vr)
    assert (~want_ok).sum() == (~np.array(run.ok, bool)[idx]).sum() + len(tamperings)
    for up in (lambda x: x, group.to_device):
        ok, v = D.check(group, run.Z, up(T), up(shares), up(comm), up(ci), up(vi))
        ok = np.asarray(ok.download() if hasattr(ok, "download") else ok).astype(bool).reshape(n, k)
        assert np.array_equal(ok, want_ok), np.argwhere(ok != want_ok)[:8].tolist()
        assert eq(v, want_v)


def test_commit_and_respond_cross_their_chunk(group):
    """One text more than the trustee calls' chunk: the bytes of the two halves called apart."""
    from electionguard import decrypt2 as D
    n = D.chunk_texts(1) + 1
    rs = np.random.default_rng(13)

    def rand_q(m):
        a = rs.integers(0, 256, (m, 32), U8)
        a[:, 0] &= 0x7F
        return a

    pads, U, C, z = group.gPowP_batch(rand_q(n)), rand_q(n), rand_q(n), group.q - 12345
    whole = D.commit(group, z, pads, U)
    cut = n - 3
    for got, lo, hi in zip(whole, D.commit(group, z, pads[:cut], U[:cut]), D.commit(group, z, pads[cut:], U[cut:])):
        assert got.shape == (n, 512) and eq(got[:cut], lo) and eq(got[cut:], hi)
    v = D.respond(group, z, U, C)
    assert v.shape == (n, 32) and eq(v[:cut], D.respond(group, z, U[:cut], C[:cut]))
    assert eq(v[cut:], D.respond(group, z, U[cut:], C[cut:]))
    last = n - 1                                       # the row past the chunk, against CPython
    be_int = lambda row: int.from_bytes(bytes(row), "big")
    want = R.commit(group.p, group.g, z, [be_int(pads[last])], [be_int(U[last])])
    assert [be_int(x[last]) for x in whole] == [w[0] for w in want]
    assert be_int(v[last]) == R.respond(group.q, z, [be_int(U[last])], [be_int(C[last])])[0]


def test_the_1_0_calls_and_prod_pow_give_what_they_gave(group, ceremonies):
    """No cached table or workspace slot of the other entry points is disturbed by decrypt2 calls."""
    from electionguard import decrypt as D1
    from electionguard import decrypt2 as D
    from electionguard import prodpow as pp
    cer = ceremonies[(3, 2)]
    rng = random.Random(29)
    T = encrypt_counts(group, cer.K, [1, 2, 3], rng)
    secret, nonces = cer.coeffs[0][0], Q([rng.randrange(group.q) for _ in range(3)])
    stack = np.ascontiguousarray(np.stack([T[:, 0], T[:, 1]], axis=1))

    def existing():
        M, pr = D1.partial_decrypt_batch(group, secret, QBAR, T, nonces)
        ok = D1.verify_shares(group, QBAR, cer.commitments[0][0], T, M, pr)
        return M, pr, ok, pp.prod_pow(group, stack, [5, group.q - 2])

    before = existing()
    assert before[2].all()
    texts = [(int.from_bytes(bytes(T[t, 0]), "big"), int.from_bytes(bytes(T[t, 1]), "big")) for t in range(3)]
    run = R.run(cer, QBAR, [1, 2], texts, nonce_rows(group, rng, 2, 3))
    assert run.ok == [[True, True]] * 3 and run.verified == [True] * 3
    assert_equals_reference(group, cer.K, QBAR, run)
    for x, y in zip(before, existing()):
        assert np.array_equal(x, y)
