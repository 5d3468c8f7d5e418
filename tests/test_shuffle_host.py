"""CPU: the verifiable shuffle on a toy Schnorr group (64-bit p): the reference of
tests/shuffle_ref.py accepts honest proofs for N in 1..50 and w in 1..3 and rejects every tampering,
electionguard.shuffle's *_host mirrors equal it byte for byte in both hash formats, and the tagged
tree T is checked level by level at the lengths 1, 256, 257 and 65,537."""
import random
from types import SimpleNamespace

import pytest

import shuffle_ref as R

P, Q, G0 = R.find_group(64, 32)
QBAR, GSEED = 0x1234567, 0xABCDEF0123


def toy(fmt="fixed"):
    return SimpleNamespace(p=P, q=Q, g=G0, hash_format=fmt)


def make(N, w, seed, fmt="fixed", psi=None):
    rng = random.Random(seed)
    K = pow(G0, rng.randrange(1, Q), P)
    E = [[(pow(G0, rng.randrange(Q), P), pow(G0, rng.randrange(Q), P)) for _ in range(w)] for _ in range(N)]
    if psi is None:
        psi = list(range(N))
        rng.shuffle(psi)
    r = [[rng.randrange(Q) for _ in range(w)] for _ in range(N)]
    nonces = [rng.getrandbits(40) for _ in range(4 * N + 3 + w)]       # some above q: reduced on use
    G = R.generators(P, Q, GSEED, N, fmt)
    E2 = R.mix(P, Q, G0, K, E, psi, r)
    proof = R.prove(P, Q, G0, K, QBAR, GSEED, G, E, E2, psi, r, nonces, fmt)
    return SimpleNamespace(N=N, w=w, K=K, E=E, psi=psi, r=r, nonces=nonces, G=G, E2=E2, proof=proof, fmt=fmt)


def check(c, **kw):
    a = dict(K=c.K, qbar=QBAR, gseed=GSEED, G=c.G, E=c.E, E2=c.E2, proof=c.proof, check_inputs=True)
    a.update(kw)
    return R.verify(P, Q, G0, a["K"], a["qbar"], a["gseed"], a["G"], a["E"], a["E2"], a["proof"], a["check_inputs"],
                    c.fmt)


def test_the_toy_group_is_a_schnorr_group():
    assert (P - 1) % Q == 0 and P.bit_length() == 64 and Q.bit_length() == 32
    assert G0 not in (0, 1) and pow(G0, Q, P) == 1


@pytest.mark.parametrize("w", [1, 2, 3])
def test_honest_proofs_are_accepted(w):
    for N in range(1, 51):
        c = make(N, w, 100 * w + N)
        assert check(c) == (True, 0), (N, w)
        assert sorted(c.psi) == list(range(N))
        # the chain's closed form equals its recursive form
        for i in range(N):
            prev = c.proof.chain[i - 1] if i else c.G[0]
            assert c.proof.chain[i] == pow(G0, c.nonces[N + i] % Q, P) * pow(prev, c.proof.up[i], P) % P


def with_(proof, **kw):
    d = dict(vars(proof))
    d.update(kw)
    return SimpleNamespace(**d)


def bump(xs, i, q=None):
    xs = list(xs)
    xs[i] = q if q is not None else (xs[i] + 1) % Q
    return xs


def test_every_tampering_is_rejected():
    c = make(7, 3, 5)
    pr = c.proof
    assert check(c) == (True, 0)
    swapped = [c.E2[1], c.E2[0]] + c.E2[2:]
    assert check(c, E2=swapped)[1] & R.CHALLENGE
    E2 = [list(row) for row in c.E2]
    E2[2][1] = (E2[2][1][0], E2[2][1][1] * G0 % P)
    assert check(c, E2=E2)[1] & R.CHALLENGE
    other = R.mix(P, Q, G0, pow(c.K, 3, P), c.E, c.psi, c.r)
    assert check(c, E2=other)[1] & R.CHALLENGE
    # a psi that is no bijection, proven by the reference prover
    bad = [0, 0] + c.psi[2:]
    E2b = R.mix(P, Q, G0, c.K, c.E, bad, c.r)
    prb = R.prove(P, Q, G0, c.K, QBAR, GSEED, c.G, c.E, E2b, bad, c.r, c.nonces)
    assert check(c, E2=E2b, proof=prb)[1] & R.CHALLENGE
    assert check(c, proof=with_(pr, pc=bump(pr.pc, 4, pow(G0, 77, P))))[1] & R.CHALLENGE
    assert check(c, proof=with_(pr, chain=bump(pr.chain, 4, pow(G0, 77, P))))[1] & R.CHALLENGE
    assert check(c, proof=with_(pr, c=(pr.c + 1) % Q))[1] & R.CHALLENGE
    for i in (0, 1, 2, 4):                                   # s1, s2, s3, s4[1]
        assert check(c, proof=with_(pr, s=bump(pr.s, i)))[1] & R.CHALLENGE, i
    assert check(c, proof=with_(pr, s_hat=bump(pr.s_hat, 3)))[1] & R.CHALLENGE
    assert check(c, proof=with_(pr, s_prime=bump(pr.s_prime, 5)))[1] & R.CHALLENGE
    assert check(c, proof=with_(pr, s=bump(pr.s, 1, Q)))[1] & R.RANGE
    assert check(c, proof=with_(pr, c=pr.c + Q))[1] & R.RANGE
    E2 = [list(row) for row in c.E2]
    E2[3][0] = (P - E2[3][0][0], E2[3][0][1])
    assert check(c, E2=E2)[1] & R.RESIDUE
    E = [list(row) for row in c.E]
    E[0][0] = (P - E[0][0][0], E[0][0][1])
    assert check(c, E=E)[1] & R.RESIDUE
    assert not check(c, E=E, check_inputs=False)[1] & R.RESIDUE
    assert check(c, qbar=QBAR + 1)[1] == R.CHALLENGE
    assert check(c, gseed=GSEED + 1)[1] == R.CHALLENGE
    assert check(c, G=R.generators(P, Q, GSEED + 1, 7))[1] == R.CHALLENGE


@pytest.mark.parametrize("fmt", ["fixed", "minimal"])
def test_the_host_mirrors_equal_the_reference(fmt):
    from electionguard import shuffle as S
    g = toy(fmt)
    for N, w in ((1, 1), (2, 1), (7, 3), (9, 2)):
        c = make(N, w, 31 * N + w, fmt)
        assert S.generators_host(g, GSEED, N) == c.G
        assert S.mix_host(g, c.K, c.E, c.psi, c.r) == c.E2
        got = S.prove_host(g, c.K, QBAR, GSEED, c.G, c.E, c.E2, c.psi, c.r, c.nonces)
        for name in ("pc", "chain", "c", "s", "s_hat", "s_prime"):
            assert getattr(got, name) == getattr(c.proof, name), (N, w, name)
        assert S.verify_host(g, c.K, QBAR, GSEED, c.G, c.E, c.E2, got, True) == (True, 0)
        bad = S.ShuffleProof(got.pc, got.chain, got.c, bump(got.s, 0), got.s_hat, got.s_prime)
        assert S.verify_host(g, c.K, QBAR, GSEED, c.G, c.E, c.E2, bad) == check(c, proof=bad) == (False, R.CHALLENGE)
        bad = S.ShuffleProof(got.pc, got.chain, got.c, bump(got.s, 0, Q), got.s_hat, got.s_prime)
        assert S.verify_host(g, c.K, QBAR, GSEED, c.G, c.E, c.E2, bad) == check(c, proof=bad)
    with pytest.raises(ValueError, match="permutation"):
        S.mix_host(g, 5, [[(1, 1)], [(1, 1)]], [0, 0], [[1], [1]])
    # bytes: the arrays the GPU calls take and give
    rows = S.ints_to_rows(c.E)
    assert rows.shape == (9, 2, 2, 512) and S.rows_to_ints(rows) == c.E


def test_the_formats_differ_and_a_generator_has_order_q():
    a, b = R.generators(P, Q, GSEED, 3, "fixed"), R.generators(P, Q, GSEED, 3, "minimal")
    assert a != b
    for x in a + b:
        assert x not in (0, 1) and pow(x, Q, P) == 1
    assert a[4] == a[1] * a[2] * a[3] % P
    assert R.generators(P, Q, GSEED, 5)[:4] == a[:4]           # gen(k) does not depend on N


@pytest.mark.parametrize("n", [1, 256, 257, 65537])
def test_the_tree_level_by_level(n):
    from electionguard import shuffle as S
    rng = random.Random(n)
    vs = [rng.randrange(Q) for _ in range(n)]
    node = lambda xs: R.hash_elems(Q, [("Q", 0x41), ("Q", len(xs))] + [("Q", x) for x in xs])
    level = vs
    while len(level) > 256:
        level = [node(level[i:i + 256]) for i in range(0, len(level), 256)]
    want = node(level)
    assert R.tree(Q, vs) == want == S.tree_host(toy(), vs)
    if n == 257:
        assert want == node([node(vs[:256]), node(vs[256:])])
    if n == 65537:                                             # three levels: 257 nodes, then 2, then 1
        assert len([0 for i in range(0, n, 256)]) == 257
    assert R.tree(Q, vs[:-1] + [(vs[-1] + 1) % Q]) != want
