"""GPU: the verifiable shuffle (include/eg_hip_shuffle.h, electionguard.shuffle): generators, mix,
prover and verifier, every output byte (G, E', pc, chain, c and every response) against the CPython
reference of tests/shuffle_ref.py, for the host and the _dev variants alike.  Shapes (N, w) = (1, 1); (2, 1) with the swap; (7, 3) with a
random psi; (9, 2) with edge nonces (0, 1, q-1, q, 2^256-1) and edge elements (alpha = 1, alpha = g);
N = 300, w = 1, which crosses a 256-thread block in every scalar kernel and a k_pow
workgroup of 32 jobs many times, at rows 0, 255, 256 and 299.  A 4096-bit cofactor power costs
CPython some 15 ordinary powers, so the full generator arrays stop at N = 9 and the large case checks
gen(k) at k = 0, 256, 257 and 300 and the product by the GPU's own rows.  Each reference is computed
once per module.  The proof is checked in full at the four small shapes; at N = 300 every scalar
output against CPython given the proof's own c, and rows 0, 255, 256 and 299 of pc and chain; at
N = 65,537, the smallest N at which the scan and the tree have a third level, the chain rows at the
boundary and at N - 1 against CPython's recurrence.  The tamperings turn verify false with the
expected bit of the mask."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import shuffle_ref as R

pytestmark = pytest.mark.gpu

EG_ERR_ARG, EG_ERR_STATE = 1, 5
GSEED = 0x5EED0000000000000000000000000000000000000000000000000000000000A5
SHAPES = [(1, 1), (2, 1), (7, 3), (9, 2)]


def be(x, n=512):
    return np.frombuffer(int(x).to_bytes(n, "big"), np.uint8)


def ints(a):
    a = np.asarray(a)
    return [int.from_bytes(bytes(r), "big") for r in a.reshape(-1, a.shape[-1])]


def rows_of(E):
    return np.stack([np.stack([np.stack([be(a), be(b)]) for a, b in row]) for row in E])


def nonce_rows(r):
    return np.stack([np.stack([be(x, 32) for x in row]) for row in r])


def case(group, N, w, seed):
    p, q, g = group.p, group.q, group.g
    rng = random.Random(seed)
    K = pow(g, rng.randrange(1, q), p)
    E = [[(pow(g, rng.randrange(q), p), pow(g, rng.randrange(q), p)) for _ in range(w)] for _ in range(N)]
    r = [[rng.randrange(q) for _ in range(w)] for _ in range(N)]
    if (N, w) == (2, 1):
        psi = [1, 0]
    else:
        psi = list(range(N))
        rng.shuffle(psi)
    if (N, w) == (9, 2):
        edge = [0, 1, q - 1, q, 2**256 - 1]
        for i, x in enumerate(edge):
            r[i][i % 2] = x
        r[5] = [q + 1, 2**256 - 2]
        E[0][0] = (1, E[0][0][1])
        E[1][1] = (g, E[1][1][1])
    return SimpleNamespace(N=N, w=w, K=K, E=E, psi=psi, r=r, E2=R.mix(p, q, g, K, E, psi, r),
                           rows=rows_of(E), rbytes=nonce_rows(r), psi32=np.array(psi, np.uint32))


@pytest.fixture(scope="module")
def cases(group):
    return {s: case(group, s[0], s[1], 11 * s[0] + s[1]) for s in SHAPES}


@pytest.fixture(scope="module")
def gens(group):
    """gen(0..10) in both hash formats, by CPython once."""
    return {fmt: [R.gen(group.p, group.q, GSEED, k, fmt) for k in range(11)] for fmt in ("fixed", "minimal")}


def want_G(group, gens, N, fmt="fixed"):
    G = gens[fmt][:N + 1]
    prod = 1
    for x in G[1:]:
        prod = prod * x % group.p
    return G + [prod]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_generators_against_cpython(group, gens, device):
    from electionguard import shuffle as S
    for N in (1, 2, 7, 9):
        G = S.generators(group, GSEED, N, device=device)
        G = G.download() if device else G
        assert G.shape == (N + 2, 512)
        assert ints(G) == want_G(group, gens, N), N
    assert S.generators_host(group, GSEED, 2) == want_G(group, gens, 2)


def test_generators_follow_the_hash_format(group, gens):
    from electionguard import shuffle as S
    assert gens["fixed"] != gens["minimal"]
    group.hash_format = "minimal"
    try:
        G = S.generators(group, GSEED, 9)
    finally:
        group.hash_format = "fixed"
    assert ints(G) == want_G(group, gens, 9, "minimal")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mix_against_cpython(group, cases, shape, device):
    from electionguard import shuffle as S
    c = cases[shape]
    if device:
        out = S.mix(group, c.K, group.to_device(c.rows), group.to_device(c.psi32), group.to_device(c.rbytes))
        out = out.download()
    else:
        out = S.mix(group, c.K, c.rows, c.psi32, c.r)              # nonces as ints
    assert out.shape == (c.N, c.w, 2, 512)
    assert S.rows_to_ints(out) == c.E2
    if shape == (7, 3) and not device:
        assert S.mix_host(group, c.K, c.E, c.psi, c.r) == c.E2
        assert np.array_equal(S.mix(group, c.K, c.rows, c.psi32, c.rbytes), out)    # ... and as bytes


@pytest.fixture(scope="module")
def large(group):
    """N = 300, w = 1: rows g^{a_i}, K^{b_i} by the fixed-base path, and CPython's rows 0, 255, 256, 299."""
    from electionguard.core.group import FixedBase
    p, q, g = group.p, group.q, group.g
    rng = random.Random(300)
    N = 300
    K = pow(g, rng.randrange(1, q), p)
    a, b = [rng.randrange(q) for _ in range(N)], [rng.randrange(q) for _ in range(N)]
    r = [rng.randrange(q) for _ in range(N)]
    psi = list(range(N))
    rng.shuffle(psi)
    rows = np.ascontiguousarray(np.stack([group.gPowP_batch(a), FixedBase(group, K).pow_batch(b)], axis=1))
    rows = rows.reshape(N, 1, 2, 512)
    want = {i: (pow(g, (a[psi[i]] + r[i]) % q, p), pow(K, (b[psi[i]] + r[i]) % q, p))
            for i in (0, 255, 256, 299)}
    return SimpleNamespace(N=N, K=K, rows=rows, psi=np.array(psi, np.uint32), r=nonce_rows([[x] for x in r]), want=want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mix_across_blocks(group, large, device):
    from electionguard import shuffle as S
    c = large
    if device:
        out = S.mix(group, c.K, group.to_device(c.rows), group.to_device(c.psi), group.to_device(c.r)).download()
    else:
        out = S.mix(group, c.K, c.rows, c.psi, c.r)
    got = S.rows_to_ints(out)
    for i, pair in c.want.items():
        assert got[i][0] == pair, i
    # every row is a re-encryption of some row: the products of the columns differ by g^{sum r}, K^{sum r}
    rsum = sum(ints(c.r)) % group.q
    for k, base in ((0, group.g), (1, c.K)):
        before = group.prodP_groups(np.ascontiguousarray(c.rows[:, 0, k]), 1, c.N)
        after = group.prodP_groups(np.ascontiguousarray(out[:, 0, k]), 1, c.N)
        assert ints(after)[0] == ints(before)[0] * pow(base, rsum, group.p) % group.p


def test_generators_across_blocks(group, gens):
    from electionguard import shuffle as S
    N = 300
    G = S.generators(group, GSEED, N)
    got = ints(G)
    assert got[:11] == gens["fixed"]
    for k in (256, 257, 300):
        assert got[k] == R.gen(group.p, group.q, GSEED, k), k
    assert len(set(got[:N + 1])) == N + 1
    assert ints(group.prodP_groups(np.ascontiguousarray(G[1:N + 1]), 1, N))[0] == got[N + 1]
    d = S.generators(group, GSEED, N, device=True).download()
    assert np.array_equal(d, G)


def test_refusals_on_the_device(group, cases):
    from electionguard import shuffle as S
    from electionguard.core.native import EgError
    c = cases[(7, 3)]
    lib = group._lib
    out = np.zeros((9, 512), np.uint8)
    cof = (S.cofactor(group) + 2).to_bytes(512, "big")
    for name, o in (("eg_shuffle_generators", out.ctypes.data), ("eg_shuffle_generators_dev", 0x7000)):
        assert getattr(lib, name)(group.handle, cof, (5).to_bytes(32, "big"), 7, o) == EG_ERR_ARG
        assert b"shuffle" in lib.eg_last_error() and b"cof" in lib.eg_last_error()
    assert not out.any()
    for bad in ([0, 0, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 7]):
        with pytest.raises(EgError, match="psi") as e:
            S.mix(group, c.K, c.rows, np.array(bad, np.uint32), c.rbytes)
        assert e.value.code == EG_ERR_ARG


def test_ct_pow_refuses_the_mix_and_keeps_the_generators(group, cases, gens):
    from electionguard import shuffle as S
    from electionguard.core.native import EgError
    c = cases[(7, 3)]
    d_rows, d_psi, d_r = group.to_device(c.rows), group.to_device(c.psi32), group.to_device(c.rbytes)
    sentinel = np.full((7, 3, 2, 512), 0xA5, np.uint8)
    d_out = group.to_device(sentinel)
    out = sentinel.copy()
    group.ct_pow = True
    try:
        rc = group._lib.eg_shuffle_mix(group.handle, c.K.to_bytes(512, "big"), 7, 3, c.rows.ctypes.data,
                                       c.psi32.ctypes.data, c.rbytes.ctypes.data, out.ctypes.data)
        assert rc == EG_ERR_STATE and b"variable time" in group._lib.eg_last_error()
        rc = group._lib.eg_shuffle_mix_dev(group.handle, c.K.to_bytes(512, "big"), 7, 3, d_rows.ptr, d_psi.ptr,
                                           d_r.ptr, d_out.ptr)
        assert rc == EG_ERR_STATE
        with pytest.raises(EgError, match="variable time"):
            S.mix(group, c.K, c.rows, c.psi32, c.rbytes)
        assert ints(S.generators(group, GSEED, 7)) == want_G(group, gens, 7)
    finally:
        group.ct_pow = False
    assert np.array_equal(out, sentinel) and np.array_equal(d_out.download(), sentinel)


QBAR = 0x0BA5E0000000000000000000000000000000000000000000000000000000077


def be_rows(xs, n):
    return np.frombuffer(b"".join(int(x).to_bytes(n, "big") for x in xs), np.uint8).reshape(-1, n)


@pytest.fixture(scope="module")
def proofs(group, cases, gens):
    """The reference proof of each small case, once: nonces with the edge values at (9, 2)."""
    p, q, g = group.p, group.q, group.g
    out = {}
    for shape, c in cases.items():
        N, w = shape
        rng = random.Random(1000 + N)
        nonces = [rng.randrange(q) for _ in range(4 * N + 3 + w)]
        if shape == (9, 2):
            for k, x in enumerate([0, 1, q - 1, q, 2**256 - 1]):
                nonces[k] = nonces[N + 1 + k] = nonces[2 * N + 2 + k] = nonces[3 * N + 3 + k] = x
            nonces[4 * N], nonces[4 * N + 3] = q, 2**256 - 1
        G = want_G(group, gens, N)
        pr = R.prove(p, q, g, c.K, QBAR, GSEED, G, c.E, c.E2, c.psi, c.r, nonces)
        out[shape] = SimpleNamespace(G=G, Gb=be_rows(G, 512), nonces=nonces, nb=be_rows(nonces, 32), proof=pr,
                                     E2b=rows_of(c.E2))
    return out


REF_VERDICT = {}


def proof_arrays(pr):
    from electionguard import shuffle as S
    return S.ShuffleProof(be_rows(pr.pc, 512), be_rows(pr.chain, 512), be_rows([pr.c], 32)[0], be_rows(pr.s, 32),
                          be_rows(pr.s_hat, 32), be_rows(pr.s_prime, 32))


def up(group, a):
    return group.to_device(np.ascontiguousarray(a))


def down(x):
    return x.download() if hasattr(x, "download") else x


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_prove_against_cpython(group, cases, proofs, shape, device):
    from electionguard import shuffle as S
    c, pf = cases[shape], proofs[shape]
    f = (lambda a: up(group, a)) if device else (lambda a: a)
    got = S.prove(group, c.K, QBAR, GSEED, f(pf.Gb), f(c.rows), f(pf.E2b), f(c.psi32), f(c.rbytes), f(pf.nb))
    got = S.ShuffleProof(*[down(x) for x in (got.pc, got.chain, got.c, got.s, got.s_hat, got.s_prime)]).to_ints()
    for name in ("pc", "chain", "c", "s", "s_hat", "s_prime"):
        assert getattr(got, name) == getattr(pf.proof, name), (shape, name)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_verify_accepts_the_reference_proof(group, cases, proofs, shape, device):
    from electionguard import shuffle as S
    c, pf = cases[shape], proofs[shape]
    f = (lambda a: up(group, a)) if device else (lambda a: a)
    pr = proof_arrays(pf.proof)
    pr = S.ShuffleProof(*[f(x) for x in (pr.pc, pr.chain, pr.c, pr.s, pr.s_hat, pr.s_prime)])
    want = (True, 0)
    if shape not in REF_VERDICT:        # the reference's verdict, once per shape
        REF_VERDICT[shape] = R.verify(group.p, group.q, group.g, c.K, QBAR, GSEED, pf.G, c.E, c.E2, pf.proof, True)
    assert REF_VERDICT[shape] == want
    ok, failed = S.verify(group, c.K, QBAR, GSEED, f(pf.Gb), f(c.rows), f(pf.E2b), pr, check_inputs=True)
    if device:
        ok, failed = bool(ok.download()[0]), int(failed.download()[0])
    assert (ok, failed) == want


def test_every_tampering_is_rejected(group, cases, proofs, gens):
    from electionguard import shuffle as S
    p, q, g = group.p, group.q, group.g
    c, pf = cases[(7, 3)], proofs[(7, 3)]
    base = proof_arrays(pf.proof)

    def check(K=c.K, qbar=QBAR, gseed=GSEED, G=pf.Gb, E2=pf.E2b, proof=base, **kw):
        d = dict(vars(base))
        d.update(kw)
        if kw:
            proof = S.ShuffleProof(**d)
        return S.verify(group, K, qbar, gseed, G, c.rows, E2, proof, check_inputs=True)

    def bumped(a, i, value=None):
        a = a.copy()
        x = int.from_bytes(bytes(a[i]), "big")
        a[i] = be((x + 1) % q if value is None else value, a.shape[-1])
        return a

    assert check() == (True, 0)
    E2 = pf.E2b.copy()
    E2[[0, 1]] = E2[[1, 0]]
    assert check(E2=E2) == (False, R.CHALLENGE)                                    # two rows swapped
    E2 = pf.E2b.copy()
    E2[2, 1, 1] = be(c.E2[2][1][1] * g % p)
    assert check(E2=E2) == (False, R.CHALLENGE)                                    # one beta' times g
    other = rows_of(R.mix(p, q, g, pow(c.K, 3, p), c.E, c.psi, c.r))
    assert check(E2=other) == (False, R.CHALLENGE)                                 # a mix under another key
    bad = [0, 0] + c.psi[2:]
    E2b = R.mix(p, q, g, c.K, c.E, bad, c.r)
    prb = R.prove(p, q, g, c.K, QBAR, GSEED, pf.G, c.E, E2b, bad, c.r, pf.nonces)
    assert check(E2=rows_of(E2b), proof=proof_arrays(prb)) == (False, R.CHALLENGE)  # psi no bijection
    assert check(pc=bumped(base.pc, 4, pow(g, 77, p))) == (False, R.CHALLENGE)
    assert check(chain=bumped(base.chain, 4, pow(g, 77, p))) == (False, R.CHALLENGE)
    assert check(c=bumped(base.c.reshape(1, 32), 0)[0]) == (False, R.CHALLENGE)
    for i in (0, 1, 2, 4):                                                          # s1, s2, s3, s4[1]
        assert check(s=bumped(base.s, i)) == (False, R.CHALLENGE), i
    assert check(s_hat=bumped(base.s_hat, 3)) == (False, R.CHALLENGE)
    assert check(s_prime=bumped(base.s_prime, 5)) == (False, R.CHALLENGE)
    ok, failed = check(s=bumped(base.s, 1, q))                                     # a response set to q
    assert not ok and failed & R.RANGE
    ok, failed = check(s_prime=bumped(base.s_prime, 6, 2**256 - 1))
    assert not ok and failed & R.RANGE
    E2 = pf.E2b.copy()
    E2[3, 0, 0] = be(p - c.E2[3][0][0])
    ok, failed = check(E2=E2)                                                       # alpha' -> p - alpha'
    assert not ok and failed & R.RESIDUE
    assert check(qbar=QBAR + 1) == (False, R.CHALLENGE)
    assert check(gseed=GSEED + 1) == (False, R.CHALLENGE)
    assert check(G=S.generators(group, GSEED + 1, 7)) == (False, R.CHALLENGE)      # generators of another seed


@pytest.fixture(scope="module")
def large_proof(group, large):
    """The GPU's mix and proof at N = 300 with cheap generators g^{k_i} of the test's own (G is an
    argument), all on the device."""
    from electionguard import shuffle as S
    rng = random.Random(301)
    q, N = group.q, large.N
    k = [rng.randrange(1, q) for _ in range(N + 1)]
    Gb = np.concatenate([group.gPowP_batch(k), group.gPowP_batch([sum(k[1:]) % q])])
    nonces = [rng.randrange(q) for _ in range(4 * N + 4)]
    d = SimpleNamespace(G=up(group, Gb), rows=up(group, large.rows), psi=up(group, large.psi), r=up(group, large.r),
                        nonces=up(group, be_rows(nonces, 32)))
    d.rows2 = S.mix(group, large.K, d.rows, d.psi, d.r)
    d.proof = S.prove(group, large.K, QBAR, GSEED, d.G, d.rows, d.rows2, d.psi, d.r, d.nonces)
    return SimpleNamespace(d=d, k=k, Gb=Gb, nonces=nonces)


def scalars_want(group, N, w, K, G, E, E2, pc, psi, r, nonces, c):
    """y, u, R, U and the responses of the reference, given the proof's own pc and c."""
    q = group.q
    y = R.seed(q, QBAR, K, GSEED, N, w, E, E2, pc)
    u = R.challenges(q, y, N)
    upr = [u[psi[i]] for i in range(N)]
    rho, rho_hat, om_hat, om_p = (nonces[k * N:(k + 1) * N] for k in range(4))
    om = nonces[4 * N:]
    Rs, Us = R.scan(q, rho_hat, upr)
    wit = [sum(rho) % q, Rs[-1], sum(a * b for a, b in zip(rho, u)) % q] + \
        [sum(r[i][j] * upr[i] for i in range(N)) % q for j in range(w)]
    s = [(om[k] + c * wit[k]) % q for k in range(3 + w)]
    return SimpleNamespace(u=u, up=upr, R=Rs, U=Us, s=s, s_hat=[(om_hat[i] + c * rho_hat[i]) % q for i in range(N)],
                           s_prime=[(om_p[i] + c * upr[i]) % q for i in range(N)])


def test_proof_across_blocks(group, large, large_proof):
    from electionguard import shuffle as S
    p, q, g, N = group.p, group.q, group.g, large.N
    d, lp = large_proof.d, large_proof
    assert [x.download()[0] for x in S.verify(group, large.K, QBAR, GSEED, d.G, d.rows, d.rows2, d.proof, True)] == [1, 0]
    pr = S.ShuffleProof(*[x.download() for x in (d.proof.pc, d.proof.chain, d.proof.c, d.proof.s, d.proof.s_hat,
                                                 d.proof.s_prime)])
    pi = pr.to_ints()
    E, E2 = S.rows_to_ints(large.rows), S.rows_to_ints(d.rows2.download())
    psi, r = [int(x) for x in large.psi], [[x] for x in ints(large.r)]
    want = scalars_want(group, N, 1, large.K, ints(lp.Gb), E, E2, pi.pc, psi, r, lp.nonces, pi.c)
    assert pi.s == want.s and pi.s_hat == want.s_hat and pi.s_prime == want.s_prime
    inv = {psi[i]: i for i in range(N)}
    for j in (0, 255, 256, 299):
        assert pi.pc[j] == pow(g, (lp.nonces[j] + lp.k[1 + inv[j]]) % q, p), j
        assert pi.chain[j] == pow(g, (want.R[j] + lp.k[0] * want.U[j]) % q, p), j
    # the host variants give the same bytes, and a tampering on each side of index 255 / 256 is seen
    host = S.prove(group, large.K, QBAR, GSEED, lp.Gb, large.rows, d.rows2.download(), large.psi, large.r,
                   be_rows(lp.nonces, 32))
    for a, b in zip(vars(host).values(), vars(pr).values()):
        assert np.array_equal(a, b)
    for name, i in (("s_hat", 255), ("s_prime", 256), ("chain", 255), ("pc", 256)):
        a = getattr(pr, name).copy()
        a[i] = a[(i + 1) % N]
        bad = S.ShuffleProof(**{**vars(pr), name: a})
        assert S.verify(group, large.K, QBAR, GSEED, lp.Gb, large.rows, d.rows2.download(), bad) == \
            (False, R.CHALLENGE), (name, i)


def test_proof_in_the_minimal_format_against_cpython(group):
    """N = 257, w = 1 with hash_format = "minimal": the small-integer elements of the proof's hashes
    (the tags and the `len` of k_sh_leaf and k_sh_tree, the index of k_sh_challenges) in the format
    the generators alone were checked in.  257 is the smallest N with a second tree level: a node of
    len 256 (two hex bytes in minimal form) beside a node of len 1, and challenge indices on both
    sides of 255 -> 256.  Every output of the prover against shuffle_ref.prove(fmt="minimal").
    The rows and generators are g^x by the fixed-base path (G is an argument), and rho, omega^,
    omega', r are below 2^32, so that CPython's full-size powers are the chain's 2 N only; rho^ and
    omega_1..4 are full-size, and every response is."""
    from electionguard import shuffle as S
    p, q, g, N = group.p, group.q, group.g, 257
    rng = random.Random(257)
    K = pow(g, rng.randrange(1, q), p)
    rows = group.gPowP_batch([rng.randrange(q) for _ in range(2 * N)]).reshape(N, 1, 2, 512)
    k = [rng.randrange(1, q) for _ in range(N + 1)]
    Gb = group.gPowP_batch(k + [sum(k[1:]) % q])        # h, h_1 .. h_N and their product
    E, G = S.rows_to_ints(rows), ints(Gb)
    psi = list(range(N))
    rng.shuffle(psi)
    r = [[rng.randrange(1 << 32)] for _ in range(N)]
    E2 = R.mix(p, q, g, K, E, psi, r)
    small = lambda n: [rng.randrange(1 << 32) for _ in range(n)]
    nonces = small(N) + [rng.randrange(q) for _ in range(N)] + small(2 * N) + [rng.randrange(q) for _ in range(4)]
    want = R.prove(p, q, g, K, QBAR, GSEED, G, E, E2, psi, r, nonces, fmt="minimal")
    E2b, nb = rows_of(E2), be_rows(nonces, 32)
    group.hash_format = "minimal"
    try:
        pr = S.prove(group, K, QBAR, GSEED, Gb, rows, E2b, np.array(psi, np.uint32), nonce_rows(r), nb)
        verdict = S.verify(group, K, QBAR, GSEED, Gb, rows, E2b, pr, check_inputs=True)
        bad = pr.c.copy()
        bad[31] ^= 0xFF
        tampered = S.verify(group, K, QBAR, GSEED, Gb, rows, E2b, S.ShuffleProof(**{**vars(pr), "c": bad}))
    finally:
        group.hash_format = "fixed"
    got = pr.to_ints()
    for name in ("c", "s", "s_hat", "s_prime"):
        assert getattr(got, name) == getattr(want, name), name
    assert np.array_equal(pr.pc, be_rows(want.pc, 512)) and np.array_equal(pr.chain, be_rows(want.chain, 512))
    assert verdict == (True, 0)
    assert R.CHALLENGE == 4 and not tampered[0] and tampered[1] & R.CHALLENGE


def test_proof_across_levels(group):
    """N = 65,537, w = 1: the scan and the tree have a third level (256-way levels).  Generators
    derived on the GPU; verify is true; chain rows at the boundary and at N - 1 by CPython's recurrence."""
    from electionguard import shuffle as S
    p, q, g, N = group.p, group.q, group.g, 65537
    rng = random.Random(65537)
    K = pow(g, rng.randrange(1, q), p)
    ab = np.frombuffer(rng.randbytes(2 * N * 32), np.uint8).reshape(2 * N, 32)
    rows = group.gPowP_batch(ab).reshape(N, 1, 2, 512)
    psi = list(range(N))
    rng.shuffle(psi)
    r = np.frombuffer(rng.randbytes(N * 32), np.uint8).reshape(N, 1, 32)
    nonces = np.frombuffer(rng.randbytes((4 * N + 4) * 32), np.uint8).reshape(-1, 32)
    d_rows, d_psi, d_r = up(group, rows), up(group, np.array(psi, np.uint32)), up(group, r)
    G = S.generators(group, GSEED, N, device=True)
    rows2 = S.mix(group, K, d_rows, d_psi, d_r)
    proof = S.prove(group, K, QBAR, GSEED, G, d_rows, rows2, d_psi, d_r, up(group, nonces))
    ok, failed = S.verify(group, K, QBAR, GSEED, G, d_rows, rows2, proof)
    assert (ok.download()[0], failed.download()[0]) == (1, 0)
    Gb, pc, chain = G.download(), proof.pc.download(), proof.chain.download()
    assert ints(Gb[65536:65538]) == [R.gen(p, q, GSEED, k) for k in (65536, 65537)]
    y = R.seed(q, QBAR, K, GSEED, N, 1, S.rows_to_ints(rows), S.rows_to_ints(rows2.download()), ints(pc))
    u = R.challenges(q, y, N)
    Rs, Us = R.scan(q, [x % q for x in ints(nonces[N:2 * N])], [u[psi[i]] for i in range(N)])
    h = ints(Gb[:1])[0]
    for i in (255, 256, 65535, 65536):
        assert ints(chain[i:i + 1])[0] == pow(g, Rs[i], p) * pow(h, Us[i], p) % p, i
    bad = proof.s_prime.download()
    bad[65536] = bad[65535]
    proof.s_prime = up(group, bad)
    ok, failed = S.verify(group, K, QBAR, GSEED, G, d_rows, rows2, proof)
    assert (ok.download()[0], failed.download()[0]) == (0, R.CHALLENGE)


def test_ct_pow_refuses_the_prover_and_keeps_the_verifier(group, cases, proofs):
    from electionguard import shuffle as S
    from electionguard.core.native import EgError
    c, pf = cases[(7, 3)], proofs[(7, 3)]
    outs = [np.full(sh, 0xA5, np.uint8) for sh in ((7, 512), (7, 512), (32,), (6, 32), (7, 32), (7, 32))]
    group.ct_pow = True
    try:
        rc = group._lib.eg_shuffle_prove(group.handle, c.K.to_bytes(512, "big"), QBAR.to_bytes(32, "big"),
                                         GSEED.to_bytes(32, "big"), 7, 3, pf.Gb.ctypes.data, c.rows.ctypes.data,
                                         pf.E2b.ctypes.data, c.psi32.ctypes.data, c.rbytes.ctypes.data,
                                         pf.nb.ctypes.data, *[o.ctypes.data for o in outs])
        assert rc == EG_ERR_STATE and b"variable time" in group._lib.eg_last_error()
        with pytest.raises(EgError, match="variable time"):
            S.prove(group, c.K, QBAR, GSEED, pf.Gb, c.rows, pf.E2b, c.psi32, c.rbytes, pf.nb)
        assert S.verify(group, c.K, QBAR, GSEED, pf.Gb, c.rows, pf.E2b, proof_arrays(pf.proof), True) == (True, 0)
    finally:
        group.ct_pow = False
    assert all((o == 0xA5).all() for o in outs)


def test_shuffle_draws_and_proves(group, cases):
    from electionguard import shuffle as S
    c = cases[(7, 3)]
    rows2, proof = S.shuffle(group, c.K, QBAR, c.rows, GSEED)
    G = S.generators(group, GSEED, 7)
    assert S.verify(group, c.K, QBAR, GSEED, G, c.rows, rows2, proof, check_inputs=True) == (True, 0)
    again, _ = S.shuffle(group, c.K, QBAR, c.rows, GSEED)
    assert not np.array_equal(again, rows2)
    d2, dproof = S.shuffle(group, c.K, QBAR, up(group, c.rows), GSEED)
    ok, failed = S.verify(group, c.K, QBAR, GSEED, up(group, G), up(group, c.rows), d2, dproof)
    assert (ok.download()[0], failed.download()[0]) == (1, 0)


def test_the_other_paths_keep_their_bytes_after_a_shuffle(group, cases, large):
    """No workspace slot is shared: one eg_prod_pow_dev, one eg_decrypt2_combine and one small
    verify_ballots_v2 give after the generators, two mixes, a proof and its check the bytes they gave
    before them."""
    from electionguard import ballot2 as b2
    from electionguard import decrypt2 as d2
    from electionguard import prodpow as pp
    from electionguard import shuffle as S
    from electionguard.ballot import ElectionKey
    q = group.q
    rng = random.Random(91)
    c = cases[(9, 2)]
    qbar = rng.randrange(q)
    bases = group.to_device(np.ascontiguousarray(large.rows.reshape(300, 2, 512)))
    exps = group.to_device(np.stack([be(rng.getrandbits(256), 32) for _ in range(300)]))
    flat = large.rows.reshape(-1, 512)
    texts = np.ascontiguousarray(flat[:8].reshape(4, 2, 512))
    shares = np.ascontiguousarray(flat[8:20].reshape(4, 3, 512))
    comm = np.ascontiguousarray(flat[20:44].reshape(4, 3, 2, 512))
    weights = [rng.randrange(q) for _ in range(3)]
    key, man = ElectionKey(group, c.K), b2.Manifest2([(2, 3, 3), (1, 1, 1)])
    votes = np.array([[3, 0, 1], [1, 2, 0]], np.uint8)
    sn, cn = b2.random_nonces2(np.random.default_rng(4), man, 2, q)
    eb = b2.encrypt(group, key, qbar, man, votes, sn, cn)
    ver = b2.Verifier2(group, key, qbar, man)

    def others():
        out = [pp.prod_pow(group, bases, exps, layout="terms").download()]
        out += list(d2.combine(group, c.K, qbar, weights, texts, shares, comm))
        out += list(ver.verify(eb))
        return out

    before = others()
    assert before[4].all() and before[5].all()
    S.generators(group, GSEED, 9)
    S.mix(group, c.K, c.rows, c.psi32, c.rbytes)
    S.mix(group, large.K, group.to_device(large.rows), group.to_device(large.psi), group.to_device(large.r))
    rows2, proof = S.shuffle(group, c.K, qbar, c.rows, GSEED)
    assert S.verify(group, c.K, qbar, GSEED, S.generators(group, GSEED, 9), c.rows, rows2, proof)[0]
    after = others()
    assert len(before) == len(after) == 7
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
