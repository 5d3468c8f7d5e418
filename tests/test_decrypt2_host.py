"""CPU: the threshold decryption with one combined proof per text on CPython ints.  The reference
(tests/decrypt2_ref.py) is self-consistent on a small Schnorr group; every tampering flips exactly
the flags it must; electionguard.decrypt2's ``*_host`` mirrors equal the reference; a trustee
answers a commitment once."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import decrypt2_ref as R


def _is_prime(n):
    if n < 2:
        return False
    for sp in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % sp == 0:
            return n == sp
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):   # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def small_group():
    """q = 2^31 - 1, p = m q + 1 the first such prime above 2^70, g of order q."""
    q = 2**31 - 1
    m = (2**70 // q) & ~1
    while not _is_prime(m * q + 1):
        m += 2
    p = m * q + 1
    h = 2
    while pow(h, m, p) == 1:
        h += 1
    return SimpleNamespace(p=p, q=q, g=pow(h, m, p), hash_format="fixed")


G = small_group()
QBAR = 0x1234567
N_G, QUORUM = 5, 3


@pytest.fixture(scope="module")
def world():
    rng = random.Random(2)
    cer = R.ceremony(G.p, G.q, G.g, N_G, QUORUM, rng)
    votes = [0, 1, 3, 7, 2, 5]
    texts = []
    for t in votes:
        r = rng.randrange(1, G.q)
        texts.append((pow(G.g, r, G.p), pow(cer.K, r, G.p) * pow(G.g, t, G.p) % G.p))
    nonces = [[rng.randrange(G.q) for _ in texts] for _ in range(N_G)]
    return SimpleNamespace(cer=cer, votes=votes, texts=texts, nonces=nonces)


def test_the_group_is_a_schnorr_group():
    assert _is_prime(G.p) and _is_prime(G.q) and (G.p - 1) % G.q == 0
    assert G.g != 1 and pow(G.g, G.q, G.p) == 1


def test_an_honest_run_verifies_and_decrypts(world):
    run = R.run(world.cer, QBAR, [1, 3, 4], world.texts, world.nonces[:3], limit=10)
    assert all(all(row) for row in run.ok) and all(run.verified)
    assert run.counts == world.votes
    assert run.M == [pow(A, world.cer.s, G.p) for A, _ in world.texts]


def test_weights_shares_and_share_keys(world):
    cer = world.cer
    for xs in ([1, 2, 3], [2, 4, 5], [1, 2, 3, 4, 5]):
        w = [R.lagrange(xs, x, G.q) for x in xs]
        assert sum(wi * R.key_share(cer, x) for wi, x in zip(w, xs)) % G.q == cer.s
    for x in cer.xs:
        assert R.share_public_key(cer, x) == pow(G.g, R.key_share(cer, x), G.p)


def test_two_quorums_of_one_ceremony_agree(world):
    a = R.run(world.cer, QBAR, [1, 2, 3], world.texts, world.nonces[:3], limit=10)
    b = R.run(world.cer, QBAR, [2, 3, 4, 5], world.texts, world.nonces[:4], limit=10)
    assert a.M == b.M and a.counts == b.counts == world.votes
    assert a.shares != [row[:3] for row in b.shares]


@pytest.mark.parametrize("kind", list(R.TAMPERINGS))
def test_a_tampering_flips_exactly_its_flags(world, kind):
    xs, t, i = [1, 3, 5], 4, 1
    run, bad_items, bad_texts = R.tampered(world.cer, QBAR, xs, world.texts, world.nonces[:3], kind, t, i)
    n = len(world.texts)
    assert {(tt, ii) for tt in range(n) for ii in range(3) if not run.ok[tt][ii]} == bad_items
    assert {tt for tt in range(n) if not run.verified[tt]} == bad_texts
    assert bad_items or bad_texts


def test_range_flags_of_check_and_verify(world):
    """c_i, v_i, c, v >= q are refused even where the group equations hold (an exponent + q)."""
    xs = [1, 2, 3]
    base = R.run(world.cer, QBAR, xs, world.texts, world.nonces[:3])
    run = R.run(world.cer, QBAR, xs, world.texts, world.nonces[:3],
                after_respond=lambda ci, vi: vi[2].__setitem__(0, vi[2][0] + G.q))
    assert [(t, i) for t in range(6) for i in range(3) if not run.ok[t][i]] == [(2, 0)]
    assert run.v == base.v                                  # the sum reduces what it is handed
    run = R.run(world.cer, QBAR, xs, world.texts, world.nonces[:3],
                publish=lambda M, c, v: v.__setitem__(3, v[3] + G.q))
    assert [t for t in range(6) if not run.verified[t]] == [3]


# ---- electionguard.decrypt2's mirrors ----------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fixed", "minimal"])
def test_the_host_mirrors_equal_the_reference(world, fmt):
    from electionguard import decrypt2 as D
    g = SimpleNamespace(p=G.p, q=G.q, g=G.g, hash_format=fmt)
    cer, xs = world.cer, [2, 3, 5]
    texts = world.texts + [(1, 5), (0, 7), (G.p + 5, G.p - 1)]       # A = 1 gives the leading zero bytes
    edge = [0, 1, G.q - 1, G.q, 2**256 - 1]
    nonces = [[edge[(t + i) % 5] if t < 5 else 11 * t + i for t in range(len(texts))] for i in range(3)]
    run = R.run(cer, QBAR, xs, texts, nonces, fmt)
    pads = [A for A, _ in texts]
    for i, x in enumerate(xs):
        assert D.commit_host(g, run.z[i], pads, nonces[i]) == R.commit(G.p, G.g, run.z[i], pads, nonces[i])
        ci = [row[i] for row in run.ci]
        assert D.respond_host(g, run.z[i], nonces[i], ci) == [row[i] for row in run.vi]
    assert D.combine_host(g, cer.K, QBAR, run.w, texts, run.shares, run.comm) == (run.M, run.c, run.ci)
    assert D.check_host(g, run.Z, texts, run.shares, run.comm, run.ci, run.vi) == (run.ok, run.v)
    assert D.verify_host(g, cer.K, QBAR, texts, run.M, run.proofs) == run.verified
    bad, _, _ = R.tampered(cer, QBAR, xs, texts, nonces, "bi", 1, 2, fmt)
    assert D.check_host(g, bad.Z, texts, bad.shares, bad.comm, bad.ci, bad.vi) == (bad.ok, bad.v)
    assert D.verify_host(g, cer.K, QBAR, texts, bad.M, bad.proofs) == bad.verified
    comm = {f"guardian{j + 1}": cm for j, cm in enumerate(cer.commitments)}
    keys = D.share_public_keys_host(g, comm, {f"guardian{x}": x for x in xs})
    assert [keys[f"guardian{x}"] for x in xs] == run.Z


def guardian_keys(cer, x):
    from electionguard.keyceremony import GuardianKeys
    j = x - 1
    keys = GuardianKeys(f"guardian{x}", x, cer.coeffs[j], cer.commitments[j])
    for l in range(cer.n):
        if l != j:
            keys.shares_from[f"guardian{l + 1}"] = R.poly_eval(cer.coeffs[l], x, cer.q)
    return keys


def test_key_share_is_the_sum_over_every_polynomial(world):
    from electionguard import decrypt2 as D
    for x in world.cer.xs:
        assert D.key_share(guardian_keys(world.cer, x), G.q) == R.key_share(world.cer, x)


def test_respond_twice_on_one_handle_raises(world):
    from electionguard import decrypt2 as D
    tr = D.DecryptingTrustee2(G, guardian_keys(world.cer, 2), host=True)
    texts = world.texts[:2]
    h, M, a, b = tr.commit(texts, nonces=[5, 6])
    want = R.commit(G.p, G.g, tr.z, [A for A, _ in texts], [5, 6])
    assert [[int.from_bytes(bytes(r), "big") for r in x] for x in (M, a, b)] == [list(x) for x in want]
    h2, *_ = tr.commit(texts, nonces=[7, 8])
    assert h2 != h
    v = tr.respond(h, [9, 10])
    assert [int.from_bytes(bytes(r), "big") for r in v] == R.respond(G.q, tr.z, [5, 6], [9, 10])
    with pytest.raises(ValueError, match="once"):
        tr.respond(h, [11, 12])
    with pytest.raises(ValueError, match="once"):
        tr.respond("no such handle", [1, 2])
    assert len(tr.respond(h2, np.zeros((2, 32), np.uint8))) == 2     # the other commitment is still open
