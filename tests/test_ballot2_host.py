"""CPU: the host mirror of the placeholder-free ballots (electionguard.ballot2.encrypt_host /
verify_host) against the fixture of tests/ballot2_ref.py and the oracle, the Manifest2 offsets
against a brute-force walk, the limit checks, and the tamper matrix.  No GPU call."""
import json

import numpy as np
import pytest

import ballot2_ref as ref
import eg_oracle as O
from range_proof_ref import be2i, rows

from electionguard import ballot2 as b2
from electionguard import range_proof as rp

SMALL = [(2, 1, 1), (1, 2, 2)]   # two neighbours at L = 1 and a one-selection contest at L = 2


@pytest.fixture(scope="module")
def fx():
    og = O.production_group()
    f = json.loads(ref.FIXTURE.read_text())
    K, qbar, man_l, votes, sn, cn = ref.fixture_inputs(og, f)
    sproof, cproof = ref.fixture_proofs(f)
    return dict(og=og, hg=rp.HostGroup(og.p, og.q, og.g), K=K, qbar=qbar, man=b2.Manifest2(man_l), votes=votes, sn=sn,
                cn=cn, sproof=sproof, cproof=cproof)


@pytest.fixture(scope="module")
def small(fx):
    """One honest ballot of SMALL from the host mirror, shared (never modified)."""
    man = b2.Manifest2(SMALL)
    votes = np.array([[0, 1, 2]], np.uint8)
    sn, cn = b2.random_nonces2(np.random.default_rng(2), man, 1, fx["og"].q)
    eb = b2.encrypt_host(fx["hg"], fx["K"], fx["qbar"], man, votes, sn, cn)
    return man, votes, sn, cn, eb


def test_the_fixture_names_its_manifest_and_votes():
    f = json.loads(ref.FIXTURE.read_text())
    assert [tuple(c) for c in f["manifest"]] == ref.M0 and f["votes"] == ref.VOTES0
    man, v = b2.Manifest2(ref.M0), np.array(ref.VOTES0)
    sums = [[int(v[b, int(man.first[k]):int(man.first[k]) + n].sum()) for k, (n, _, _) in enumerate(ref.M0)]
            for b in range(len(v))]
    assert [0, 0, 0, 0] in sums                                   # an empty ballot
    assert any(s[k] == c for s in sums for k, (_, _, c) in enumerate(ref.M0))   # a contest at its limit
    assert any(0 < s[k] < c for s in sums for k, (_, _, c) in enumerate(ref.M0))  # an undervote
    assert (v[:, 3:7] == 2).any()                                 # a selection holding 2


def test_encrypt_host_reproduces_the_fixture_and_verify_host_accepts_it(fx):
    """All five ballots, the all-empty one and the empty contest beside voted ones among them."""
    eb = b2.encrypt_host(fx["hg"], fx["K"], fx["qbar"], fx["man"], fx["votes"], fx["sn"], fx["cn"])
    assert np.array_equal(eb.sproof, fx["sproof"]) and np.array_equal(eb.cproof, fx["cproof"])
    fixture = b2.EncryptedBallots2(eb.cts, fx["sproof"], fx["cproof"])
    ok_s, ok_c, tally = b2.verify_host(fx["hg"], fx["K"], fx["qbar"], fx["man"], fixture, cast=[1, 0, 1, 1, 0])
    assert ok_s.shape == (5, fx["man"].NS) and ok_c.shape == (5, 4) and ok_s.all() and ok_c.all()
    p = fx["og"].p
    for s in range(fx["man"].NS):
        for c in range(2):
            assert be2i(tally[s, c]) == be2i(eb.cts[0, s, c]) * be2i(eb.cts[2, s, c]) * be2i(eb.cts[3, s, c]) % p


def test_limit_1_selection_proofs_are_the_oracle_selection_proofs(fx):
    og, K, qbar = fx["og"], fx["K"], fx["qbar"]
    man = b2.Manifest2([(2, 1, 1)])
    votes = np.array([[0, 1]], np.uint8)
    sn, cn = b2.random_nonces2(np.random.default_rng(4), man, 1, og.q)
    eb = b2.encrypt_host(fx["hg"], K, qbar, man, votes, sn, cn)
    for s in range(2):
        m, f, r = int(votes[0, s]), 1 - int(votes[0, s]), sn[0, 6 * s:6 * s + 6]   # rows R, u, c_0, v_0, c_1, v_1
        ct = O.Ciphertext(be2i(eb.cts[0, s, 0]), be2i(eb.cts[0, s, 1]))
        pr = O.make_range_proof(og, K, qbar, ct, m, be2i(r[0]), be2i(r[1]), be2i(r[2 + 2 * f]), be2i(r[3 + 2 * f]))
        assert np.array_equal(eb.sproof[0, 2 * s:2 * s + 2], rows([pr.c0, pr.v0, pr.c1, pr.v1], 32).reshape(2, 2, 32)), s


def test_offsets_equal_a_brute_force_walk():
    for man_l in (ref.M0, SMALL, [(64, 15, 15)], [(1, 1, 1)], [(5, 3, 2), (2, 15, 1), (7, 1, 15)]):
        man, lay = b2.Manifest2(man_l), ref.layout(man_l)
        assert (man.NS, man.SP, man.SN, man.CP, man.CN) == tuple(lay[k] for k in ("NS", "SP", "SN", "CP", "CN"))
        assert [(k, s, L, pr, nr) for k, _, s, L, pr, nr in man.selections()] == lay["sels"]
        assert [(k, int(man.first[k]), n, c, int(man.cp_off[k]), int(man.cn_off[k]))
                for k, (n, _, c) in enumerate(man_l)] == lay["cons"]
        first = {k: (pr, nr) for k, i, _, _, pr, nr in man.selections() if i == 0}
        assert [first[k] for k in range(len(man_l))] == list(zip(man.sp_off.tolist(), man.sn_off.tolist()))
        assert man.jobs == sum(2 * o * n + 2 * c for n, o, c in man_l)
        assert b2.chunk_ballots(man) == max(1, (1 << 16) // man.jobs)
    assert b2.Manifest2(ref.M0).style([2, 0]) == b2.Manifest2([ref.M0[2], ref.M0[0]])
    for bad in ([], [(0, 1, 1)], [(1, 0, 1)], [(1, 1, 16)]):
        with pytest.raises(ValueError):
            b2.Manifest2(bad)


def test_host_encryptor_refuses_votes_over_a_limit(fx, small):
    man, votes, sn, cn, _ = small
    v = np.concatenate([votes, votes])
    v[1, 1] = 2
    with pytest.raises(ValueError, match="ballot 1 contest 0 selection 1 holds 2, above its option limit 1"):
        b2.encrypt_host(fx["hg"], fx["K"], fx["qbar"], man, v, np.concatenate([sn, sn]), np.concatenate([cn, cn]))
    v[1, :2] = 1
    with pytest.raises(ValueError, match="ballot 1 contest 0 holds 2, above its contest limit 1"):
        b2.encrypt_host(fx["hg"], fx["K"], fx["qbar"], man, v, np.concatenate([sn, sn]), np.concatenate([cn, cn]))


def test_tamper_matrix_on_the_host_mirror(fx, small):
    """Each case changes exactly the listed verdicts.  Six copies of one ballot, one case each."""
    man, _, _, _, eb = small
    n = 6
    cts, sp, cp = (np.stack([a[0]] * n) for a in (eb.cts, eb.sproof, eb.cproof))
    want_s, want_c = np.ones((n, 3), bool), np.ones((n, 2), bool)
    sp[0, 4 + 1, 1, 31] ^= 1; want_s[0, 2] = False                 # a bit of one selection response
    cp[1, 2 + 2, 0, 3] ^= 8; want_c[1, 1] = False                  # a bit of one contest challenge
    cts[2, 1, 0] = rows([fx["og"].p - be2i(cts[2, 1, 0])], 512)[0]  # alpha (p - 1): the selection and its contest
    want_s[2, 1] = False; want_c[2, 0] = False
    sp[3, 0:2], sp[3, 2:4] = eb.sproof[0, 2:4], eb.sproof[0, 0:2]  # a proof moved to the neighbour: both fall
    want_s[3, 0] = want_s[3, 1] = False
    sp[4, 2:4] = 0; cp[4, 2:5] = 0                                 # the _dev encryptor's all-zero rows
    want_s[4, 1] = False; want_c[4, 1] = False
    # a twisted pair: both alphas of contest 0 times p - 1.  The aggregate is unchanged and the
    # contest's own proof still verifies: only the selections' residue verdicts reject the contest.
    for s in (0, 1):
        cts[5, s, 0] = rows([fx["og"].p - be2i(cts[5, s, 0])], 512)[0]
    p = fx["og"].p
    assert be2i(cts[5, 0, 0]) * be2i(cts[5, 1, 0]) % p == be2i(eb.cts[0, 0, 0]) * be2i(eb.cts[0, 1, 0]) % p
    want_s[5, 0] = want_s[5, 1] = False; want_c[5, 0] = False
    ok_s, ok_c, tally = b2.verify_host(fx["hg"], fx["K"], fx["qbar"], man, b2.EncryptedBallots2(cts, sp, cp),
                                       cast=[1, 0, 0, 0, 0, 0])
    assert np.array_equal(ok_s, want_s) and np.array_equal(ok_c, want_c)
    assert np.array_equal(tally, eb.cts[0])   # the cast ballot alone
    # the reference agrees on the two residue cases: alone the aggregate falls too, twisted it does not
    r_s, r_c, _ = ref.verify(fx["og"], fx["K"], fx["qbar"], SMALL, cts[[2, 5]], sp[[2, 5]], cp[[2, 5]])
    assert np.array_equal(r_s, want_s[[2, 5]]) and np.array_equal(r_c, want_c[[2, 5]])
