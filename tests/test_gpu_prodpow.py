"""GPU: the multi-exponentiation out[r] = prod_i B[r,i]^{e_i} (include/eg_hip_prodpow.h,
electionguard.prodpow), bit-exact.  Small shapes against CPython pow (every method and forced
width, both layouts, a padded stride, a tail group at 9 rows, the edge bases and exponents of the
ABI); the bucket structure and the medium shape against g^(sum x_i e_i) with bases g^{x_i} made by
the existing fixed-base path (one CPython pow per row); the combine against the existing
powP_batch + prodP_groups path; the device twin against the host variant."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import eg_oracle as O

pytestmark = pytest.mark.gpu

ROWS, TERMS = 9, 7
METHODS = [(1, 1), (1, 4), (2, 1), (2, 2), (2, 4), (0, 0)]
EG_ERR_ARG, EG_ERR_STATE = 1, 5


def be(x, n=512):
    return np.frombuffer(int(x).to_bytes(n, "big"), np.uint8)


def ints(a):
    return [int.from_bytes(bytes(r), "big") for r in np.asarray(a).reshape(-1, a.shape[-1])]


@pytest.fixture(scope="module")
def small(group):
    """9 rows x 7 terms drawn from the edge lists and random values, with every power B[r,i]^{e_i}
    by CPython once (63 pows); never modified."""
    p, q = group.p, group.q
    rng = random.Random(17)
    edges = [0, 1, p - 1, p, p + 1, 2**4096 - 1]
    exps = [0, 1, 2, q - 1, q, 2**256 - 1, rng.getrandbits(256)]
    B = [[rng.randrange(p) for _ in range(TERMS)] for _ in range(ROWS)]
    B[1] = edges + [rng.randrange(p)]                    # 0^0 = 1 first, then p^(q-1) = 0
    B[2] = edges[3:] + edges[:3] + [rng.randrange(p)]    # p^0, ..., 0^(q-1)
    nice = [1, p - 1, p + 1, 2**4096 - 1]                # edge bases that are not 0 mod p
    for r in range(3, ROWS):
        for i in range(TERMS):
            if rng.random() < 0.4:
                B[r][i] = rng.choice(nice)
    pw = [[pow(b % p, e, p) for b, e in zip(row, exps)] for row in B]
    bases = np.stack([np.stack([be(b) for b in row]) for row in B])           # (9, 7, 512)
    bases.setflags(write=False)
    E = np.stack([be(e, 32) for e in exps])
    E.setflags(write=False)
    return SimpleNamespace(p=p, pw=pw, bases=bases, exps=E)


def expected(small, rows, n):
    out = []
    for r in range(rows):
        acc = 1
        for i in range(n):
            acc = acc * small.pw[r][i] % small.p
        out.append(acc)
    return out


@pytest.mark.parametrize("method,w", METHODS)
def test_small_matrix_against_cpython(group, small, method, w):
    from electionguard import prodpow as pp
    for rows in (1, 3, 9):
        for n in (0, 1, 2, 7):
            want = expected(small, rows, n)
            padded = np.zeros((rows, TERMS + 1, 512), np.uint8)       # row_stride 8 > n
            padded[:, :TERMS] = small.bases[:rows]
            by_terms = np.ascontiguousarray(small.bases[:rows, :n].transpose(1, 0, 2))   # (n, rows, 512)
            for layout, arr in (("rows", padded), ("terms", by_terms)):
                if layout == "terms" and n == 0:
                    arr = np.zeros((0, rows, 512), np.uint8)
                got = pp.prod_pow(group, arr, small.exps[:n], layout=layout, method=method, window_bits=w)
                assert got.shape == (rows, 512)
                assert ints(got) == want, (rows, n, layout, method, w)


@pytest.fixture(scope="module")
def dlog(group):
    """4096 bases g^{x_i} and K^{x_i} (K = g^s) by the existing fixed-base path, laid out by terms:
    (4096, 2, 512); never modified."""
    from electionguard.core.group import FixedBase
    rng = random.Random(23)
    q = group.q
    s = rng.randrange(1, q)
    K = pow(group.g, s, group.p)
    x = [rng.randrange(q) for _ in range(4096)]
    gx = group.gPowP_batch(x)
    Kx = FixedBase(group, K).pow_batch(x)
    bases = np.ascontiguousarray(np.stack([gx, Kx], axis=1))
    bases.setflags(write=False)
    return SimpleNamespace(x=x, s=s, K=K, bases=bases, rng=rng)


def dlog_want(group, d, exps):
    t = sum(x * e for x, e in zip(d.x, exps)) % group.q
    return [pow(group.g, t, group.p), pow(d.K, t, group.p)]


def test_bucket_structure_at_c4_n64(group, dlog):
    from electionguard import prodpow as pp
    q, rng, n = group.q, random.Random(5), 64
    bases = dlog.bases[:n]
    same = rng.randrange(q)
    cases = {
        "all equal": [same] * n,                                         # one bucket per window holds everything
        "one digit each": [rng.randrange(1, 16) << (4 * rng.randrange(64)) for _ in range(n)],
        "e_i = i": list(range(n)),
        "top digit": [15 << 252] * n,
    }
    for name, exps in cases.items():
        for method, w in ((pp.BUCKETS, 4), (pp.BUCKETS, 1), (pp.INTERLEAVED, 4)):
            got = pp.prod_pow(group, bases, exps, layout="terms", method=method, window_bits=w)
            assert ints(got) == dlog_want(group, dlog, exps), (name, method, w)
    # all exponents 0: the answer is 1 even where a base is 0
    with_zero = bases.copy()
    with_zero[5, 0] = 0
    with_zero[9, 1] = 0
    got = pp.prod_pow(group, with_zero, [0] * n, layout="terms", method=pp.BUCKETS, window_bits=4)
    assert ints(got) == [1, 1]
    # a base 0 with exponent 0 among non-zero terms counts as 1; with a positive one the product is 0
    exps = [rng.randrange(q) for _ in range(n)]
    exps[5] = 0
    got = pp.prod_pow(group, with_zero, exps, layout="terms", method=pp.BUCKETS, window_bits=4)
    assert ints(got) == [dlog_want(group, dlog, exps)[0], 0]
    exps[9] = 0
    got = pp.prod_pow(group, with_zero, exps, layout="terms", method=pp.BUCKETS, window_bits=4)
    assert ints(got) == dlog_want(group, dlog, exps)


@pytest.mark.parametrize("kind", ["random", "equal"])
def test_medium_auto_is_the_bucket_method(group, dlog, kind):
    from electionguard import prodpow as pp
    n = 4096
    assert pp.plan(2, n).method == pp.BUCKETS
    rng = random.Random(31)
    exps = [rng.getrandbits(256) for _ in range(n)] if kind == "random" else [rng.getrandbits(256)] * n
    got = pp.prod_pow(group, dlog.bases, exps, layout="terms")
    assert ints(got) == dlog_want(group, dlog, exps)


@pytest.mark.parametrize("method,w,n,bits", [(1, 1, (1 << 12) + 3, 24), (2, 0, (1 << 16) + 3, 256)])
def test_term_chunks_multiply(group, dlog, method, w, n, bits):
    """Three terms more than one chunk of the method holds (2^12 interleaved, 2^16 buckets): the
    result is the product of the chunks' results, and a chunk of three terms runs too.  The
    interleaved method chains every multiply of a row on one group, about 10 us each, so its case
    takes 24-bit exponents at w = 1: about 50,000 multiplies; full-width digits are the small
    matrix's."""
    from electionguard import prodpow as pp
    reps = -(-n // len(dlog.x))
    bases = np.concatenate([dlog.bases] * reps)[:n]
    x = (dlog.x * reps)[:n]
    rng = random.Random(37)
    exps = [rng.getrandbits(bits) for _ in range(n)]
    t = sum(a * e for a, e in zip(x, exps)) % group.q
    assert pp.plan(2, n, method, w).method == method
    got = pp.prod_pow(group, bases, exps, layout="terms", method=method, window_bits=w)
    assert ints(got) == [pow(group.g, t, group.p), pow(dlog.K, t, group.p)]


def test_combine_shape_equals_the_existing_path(group):
    from electionguard import prodpow as pp
    from electionguard.decrypt import lagrange
    rng = random.Random(41)
    texts, k, q = 1000, 3, group.q
    shares = np.ascontiguousarray(
        group.gPowP_batch([rng.randrange(q) for _ in range(texts * k)]).reshape(texts, k, 512))
    xs = [1, 2, 3]
    w = [lagrange(xs, xi, q) for xi in xs]
    old = group.prodP_groups(
        np.ascontiguousarray(np.stack([group.powP_batch(shares[:, j], [w[j]] * texts) for j in range(k)], axis=1))
        .reshape(texts * k, 512), texts, k)
    assert pp.plan(texts, k).method == pp.INTERLEAVED
    assert np.array_equal(pp.prod_pow(group, shares, w, layout="rows"), old)
    assert np.array_equal(pp.prod_pow(group, shares, w, layout="rows", method=pp.BUCKETS), old)
    # what _shares_and_combine multiplies: a direct share as it is, compensated ones to their weights
    parts = [shares[:, 0]] + [group.powP_batch(shares[:, j], [w[j]] * texts) for j in (1, 2)]
    mediator = group.prodP_groups(np.ascontiguousarray(np.stack(parts, axis=1)).reshape(texts * k, 512), texts, k)
    assert np.array_equal(pp.lagrange_combine(group, shares, [1, w[1], w[2]]), mediator)


def test_row_chunks_of_the_host_variant(group):
    """33,000 rows x 4 terms pass the host variant's 2^17 staged elements: it runs 32,768 rows and
    then 232, and equals the device variant (one chunk) and the existing path."""
    from electionguard import prodpow as pp
    rng = random.Random(53)
    rows, k = 33000, 4
    x = np.frombuffer(rng.randbytes(rows * k * 32), np.uint8).reshape(-1, 32).copy()
    x[:, 0] &= 0x7F
    shares = np.ascontiguousarray(group.gPowP_batch(x).reshape(rows, k, 512))
    w = [rng.randrange(group.q) for _ in range(k)]
    old = group.prodP_groups(group.powP_batch(shares.reshape(-1, 512), w * rows), rows, k)
    host = pp.prod_pow(group, shares, w, layout="rows")
    assert np.array_equal(host, old)
    dev = pp.prod_pow(group, group.to_device(shares), group.to_device(pp._exps_array(w)), layout="rows")
    assert np.array_equal(dev.download(), old)


def test_device_twin_and_refusals(group, small, dlog):
    from electionguard import prodpow as pp
    from electionguard.core.native import EgError
    rng = random.Random(43)
    exps64 = np.stack([be(rng.getrandbits(256), 32) for _ in range(64)])
    for bases, exps, layout, method, w in ((small.bases, small.exps, "rows", 0, 0),
                                           (small.bases, small.exps, "rows", pp.BUCKETS, 2),
                                           (dlog.bases[:64], exps64, "terms", pp.BUCKETS, 4),
                                           (dlog.bases[:64], exps64, "terms", pp.INTERLEAVED, 4)):
        host = pp.prod_pow(group, bases, exps, layout=layout, method=method, window_bits=w)
        dev = pp.prod_pow(group, group.to_device(bases), group.to_device(exps), layout=layout, method=method,
                          window_bits=w)
        assert not isinstance(dev, np.ndarray) and np.array_equal(dev.download(), host)
    d_b, d_e = group.to_device(small.bases), group.to_device(small.exps)
    d_out = group.to_device(np.full((ROWS, 512), 0xAB, np.uint8))
    lib = group._lib
    for args in ((d_b.ptr + 8, d_e.ptr, d_out.ptr), (d_b.ptr, d_e.ptr + 8, d_out.ptr), (d_b.ptr, d_e.ptr, d_out.ptr + 8)):
        rc = lib.eg_prod_pow_dev(group.handle, args[0], TERMS, 1, args[1], ROWS, TERMS, 0, 0, args[2])
        assert rc == EG_ERR_ARG and b"prod_pow" in lib.eg_last_error() and b"aligned" in lib.eg_last_error()
    # the constant-time switch refuses the call and nothing is written
    h_out = np.full((ROWS, 512), 0xAB, np.uint8)
    group.ct_pow = True
    try:
        for call in (lambda: pp.prod_pow(group, d_b, d_e, out=d_out),
                     lambda: pp.prod_pow(group, small.bases, small.exps, out=h_out)):
            with pytest.raises(EgError, match="variable time") as e:
                call()
            assert e.value.code == EG_ERR_STATE
    finally:
        group.ct_pow = False
    assert (d_out.download() == 0xAB).all() and (h_out == 0xAB).all()
    assert ints(pp.prod_pow(group, d_b, d_e, out=d_out).download()) == expected(small, ROWS, TERMS)


def test_the_other_paths_keep_their_bytes_after_prod_pow(group, small, dlog):
    """No workspace slot is shared: powP_batch, prodP_groups and a small verify give after a
    prod_pow (both methods) the bytes they gave before it."""
    from electionguard import prodpow as pp
    from electionguard.ballot import ElectionKey, EncryptedBallots, Manifest, Verifier
    og = O.production_group()
    rng = random.Random(47)
    _, K = O.key_ceremony(og, 3, 3, rng)
    qbar = rng.randrange(og.q)
    man_o, man = O.Manifest(2, 3, 1), Manifest(2, 3, 1)
    ebs = [O.encrypt_ballot(og, K, qbar, man_o, O.ballot_plaintexts(man_o, rng), rng) for _ in range(2)]
    cts = np.stack([np.stack([np.stack([be(ct.pad), be(ct.data)]) for ct in eb.cts]) for eb in ebs])
    rp = np.stack([np.stack([np.stack([be(v, 32) for v in (pr.c0, pr.v0, pr.c1, pr.v1)]) for pr in eb.proofs])
                   for eb in ebs])
    cp = np.stack([np.stack([np.stack([be(pr.c, 32), be(pr.v, 32)]) for pr in eb.contest_proofs]) for eb in ebs])
    ver = Verifier(group, ElectionKey(group, K), qbar, man)
    flat = np.ascontiguousarray(small.bases[3:9].reshape(-1, 512))
    e42 = [rng.randrange(group.q) for _ in range(len(flat))]

    def others():
        ok_s, ok_c, tally = ver.verify(EncryptedBallots(cts, rp, cp))
        return [group.powP_batch(flat, e42), group.prodP_groups(flat, 6, 7), ok_s, ok_c, tally]

    before = others()
    assert before[2].all() and before[3].all()
    pp.prod_pow(group, small.bases, small.exps, method=pp.INTERLEAVED)
    pp.prod_pow(group, dlog.bases[:300], [rng.getrandbits(256) for _ in range(300)], layout="terms",
                method=pp.BUCKETS)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
