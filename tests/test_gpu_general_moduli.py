"""GPU: prod_pow, the device-side decode and the shuffle on general and adversarial moduli, bit-exact
against CPython (no tolerance).  Every kernel of eg_prodpow.hpp, eg_decode.hpp and eg_shuffle.hpp that is
launched through LAUNCH_F, and the k_mul calls of their call layers, run here on both Montgomery
instantiations; tests/test_gpu_prodpow.py, test_gpu_decode.py and test_gpu_shuffle.py know the
production prime alone.  The fixtures are tests/general_moduli.py (checked on the CPU by
tests/test_general_moduli.py):

    sparse_c, dense_c   the Schnorr groups of tests/golden/test_groups.json: general moduli (Mont<false>);
                        sparse_c has a q below 2^255, dense_c a random 256-bit q
    Mode4096_V2         friendly: a second prime for Mont<true>
    ones .. min_top     the seven composite moduli of tests/adversarial_moduli.py, g = 3, the production q:
                        three general, four friendly; saturated and sparse operands, zero divisors
    degenerate          p = 2^4096 - 1, g = 2, q = 4096: every element the dLog meets is a single bit

prod_pow runs on the first ten, batch_inverse on all, the dLog on the Schnorr groups and the degenerate
group, the shuffle on sparse_c and dense_c.

On a composite modulus a^(p-2) is no inverse, so batch_inverse is held there to what its algorithm
defines for units and zeros (general_moduli.inverse_closed_form: a_i^-1 t^(p-1), t the product of the
non-zero elements of i's top-level block), which the CPU test shows to be the mirror's output.  Zero
divisors are left out of batch_inverse: the "for every input" of include/eg_hip_decode.h presumes a
prime p, and a non-unit has no a_i^-1 for the closed form to start from.  For the same reason the M
rows of the degenerate group decode B = 2^(t+k) to t only for k = 0 and 2048; any other k gives what
the mirror gives.

One path stays out of reach of the public API: the subtraction branch of regs_reduce_lazy for a lazy
value in [p, 2p).  With R = 2^4118 a Montgomery product exceeds p with probability about 2^-22, and no
giant step of these cases produces one; only x = p exactly (the zero input) takes the branch.

What these cases catch, tried once against a deliberately broken build whose prod_pow and decode call
layers always launch the friendly instantiation (wrong arithmetic only, the same addresses and loop
bounds): 80 of the 167 cases fail, all of them on the five general moduli, and every case of the five
friendly moduli and of the degenerate group passes.  On sparse_c, dense_c, gen_dense, gen_square and
min_top every prod_pow case fails (each method and width, and the 64-term sets, whose expected
products are non-zero on every modulus); on the two general Schnorr groups also the combine, every
dLog case (the table's canonical form and the giant steps), the shuffle's prover, verifier and drawn
proof at every shape (their products over N go through prod_pow's chunks), and batch_inverse at 17, 65
and 257; on the three general ring moduli batch_inverse at 17 and 65 and the zero-absorbing product
(the wrong reduction does not keep a 0).  What still passes there does not run the replaced code:
batch_inverse at 1 and 16 has no level (k_pow alone), and the generators and the mix use k_pow and
k_sh_gather_mul of the shuffle's own call layer.
"""
import random
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import decode_ref as D
import general_moduli as GM
import shuffle_ref as R
from general_moduli import contexts  # noqa: F401  (the module-scoped fixture)
from test_gpu_prodpow import METHODS
from test_gpu_shuffle import GSEED, QBAR, be_rows, case, proof_arrays, rows_of

pytestmark = pytest.mark.gpu

U8 = np.uint8
TEN = GM.SCHNORR + GM.RING


def be(x, n=512):
    return np.frombuffer(int(x).to_bytes(n, "big"), U8)


def rows(xs, n=512):
    return np.stack([be(x, n) for x in xs])


def ints(a):
    a = np.asarray(a)
    return [int.from_bytes(bytes(r), "big") for r in a.reshape(-1, a.shape[-1])]


# ---------------------------------------------------------------------------------------------------
# prod_pow and lagrange_combine
# ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def pp_arrays(name):
    m = GM.pp_matrix(name)
    bases = np.stack([rows(row) for row in m.B])                       # (9, 7, 512)
    bases.setflags(write=False)
    E = rows(m.exps, 32)
    E.setflags(write=False)
    return m, bases, E


@pytest.mark.parametrize("method,w", METHODS)
@pytest.mark.parametrize("name", TEN)
def test_prod_pow_small_matrix(contexts, name, method, w):
    """rows 1 and 9 (9 leaves a tail group), the last 1, 2 and 7 terms (exponents: random; 2^256 - 1 and
    random; all seven), both layouts, the "rows" layout with a padded stride."""
    ctx = contexts(name)
    from electionguard import prodpow as pp
    m, bases, E = pp_arrays(ctx.name)
    for nrows in (1, 9):
        for n in (1, 2, 7):
            cols = range(GM.TERMS - n, GM.TERMS)
            want = GM.pp_expected(m, nrows, cols)
            padded = np.zeros((nrows, n + 1, 512), U8)                  # row_stride n + 1 > n
            padded[:, :n] = bases[:nrows, GM.TERMS - n:]
            by_terms = np.ascontiguousarray(bases[:nrows, GM.TERMS - n:].transpose(1, 0, 2))
            for layout, arr in (("rows", padded), ("terms", by_terms)):
                got = pp.prod_pow(ctx.G, arr, E[GM.TERMS - n:], layout=layout, method=method, window_bits=w)
                assert got.shape == (nrows, 512)
                assert ints(got) == want, (ctx.name, nrows, n, layout, method, w)


@pytest.mark.parametrize("name", TEN)
def test_prod_pow_bucket_structure_at_64_terms(contexts, name):
    """64 terms with the exponent sets "all equal", "one digit each" and "top digit".  A Schnorr group
    takes bases g^{x_i} of its own fixed-base path, in order and reversed (two rows), against
    g^(sum x_i e_i); a ring modulus 64 directed bases, none 0 or nilpotent, against CPython's powers:
    every expected product is non-zero."""
    ctx = contexts(name)
    from electionguard import prodpow as pp
    G, name = ctx.G, ctx.name
    if name in GM.RING:
        c = GM.bucket_case_ring(name)
        bases = rows(c.bases)[:, None, :]                               # (64, 1, 512)
        want = {k: [v] for k, v in c.want.items()}
    else:
        c = GM.bucket_case_schnorr(name)
        gx = G.gPowP_batch(c.x)
        bases = np.ascontiguousarray(np.stack([gx, gx[::-1]], axis=1))  # (64, 2, 512)
        want = c.want
    for label, exps in c.sets.items():
        for method, w in ((pp.BUCKETS, 4), (pp.BUCKETS, 1), (pp.INTERLEAVED, 4)):
            got = pp.prod_pow(G, bases, exps, layout="terms", method=method, window_bits=w)
            assert ints(got) == want[label], (name, label, method, w)


@pytest.mark.parametrize("name", GM.RING)
def test_prod_pow_absorbs_a_zero_base_at_64_terms(contexts, name):
    """The same 64 terms with 0 at term 21 and p at term 40: the product is 0 for every exponent set
    (each exponent is at least 1), whichever bucket, segment or table entry the zero lands in."""
    from electionguard import prodpow as pp
    ctx = contexts(name)
    c = GM.bucket_case_ring(name)
    bases = rows(c.zeroed)[:, None, :]
    for label, exps in c.sets.items():
        for method, w in ((pp.BUCKETS, 4), (pp.BUCKETS, 1), (pp.INTERLEAVED, 4)):
            got = pp.prod_pow(ctx.G, bases, exps, layout="terms", method=method, window_bits=w)
            assert ints(got) == [0], (name, label, method, w)


@pytest.mark.parametrize("name", GM.GENERAL)
def test_lagrange_combine_on_the_general_groups(contexts, name):
    """3 texts x 3 shares: the combine equals powP_batch + prodP_groups of the same context, and CPython"""
    ctx = contexts(name)
    from electionguard import prodpow as pp
    from electionguard.decrypt import lagrange
    G, p, q, g = ctx.G, ctx.p, ctx.q, ctx.g
    rng = random.Random("combine-" + ctx.name)
    texts, k = 3, 3
    x = [rng.randrange(q) for _ in range(texts * k)]
    shares = np.ascontiguousarray(G.gPowP_batch(x).reshape(texts, k, 512))
    xs = [1, 2, 3]
    wt = [lagrange(xs, xi, q) for xi in xs]
    old = G.prodP_groups(G.powP_batch(shares.reshape(-1, 512), wt * texts), texts, k)
    want = [pow(g, sum(x[t * k + j] * wt[j] for j in range(k)) % q, p) for t in range(texts)]
    assert ints(shares)[:2] == [pow(g, x[0], p), pow(g, x[1], p)]
    got = pp.lagrange_combine(G, shares, wt)
    assert np.array_equal(got, old) and ints(got) == want
    assert np.array_equal(pp.prod_pow(G, shares, wt, layout="rows", method=pp.BUCKETS), old)
    dev = pp.lagrange_combine(G, G.to_device(shares), G.to_device(rows(wt, 32)))
    assert np.array_equal(dev.download(), old)


# ---------------------------------------------------------------------------------------------------
# batch_inverse
# ---------------------------------------------------------------------------------------------------
def check_inverse(G, els, want, multinv):
    """host, _dev, and in place on both sides"""
    from electionguard import decode as dc
    n = len(els)
    a = rows(els)
    got = dc.batch_inverse(G, a)
    assert got.shape == (n, 512) and got.dtype == U8
    bad = [i for i, (x, y) in enumerate(zip(ints(got), want)) if x != y]
    assert not bad, (n, bad[:8])
    if multinv:
        assert np.array_equal(got, G.multInv_batch(a))
    d = G.to_device(a)
    out = dc.batch_inverse(G, d)
    assert not isinstance(out, np.ndarray) and np.array_equal(out.download(), got)
    lib = G._lib
    assert lib.eg_batch_inverse_dev(G.handle, d.ptr, d.ptr, n) == 0
    assert np.array_equal(d.download(), got)
    same = a.copy()
    assert lib.eg_batch_inverse(G.handle, same.ctypes.data, same.ctypes.data, n) == 0
    assert np.array_equal(same, got)


@pytest.mark.parametrize("n", GM.INV_SIZES_SCHNORR)
@pytest.mark.parametrize("name", GM.SCHNORR)
def test_batch_inverse_on_the_schnorr_groups(contexts, name, n):
    """pow(a, -1, p) and multInv_batch's bytes at no level (1, 16), one level (17), a ragged last
    segment (65) and two levels (257), with the placements of test_gpu_decode.placements"""
    ctx = contexts(name)
    els, want = GM.inverse_case_schnorr(ctx.name, n)
    check_inverse(ctx.G, els, want, multinv=True)


@pytest.mark.parametrize("name", GM.SCHNORR)
def test_batch_inverse_of_one_nonzero_element(contexts, name):
    """at n = 1 the placements leave p alone: this one-element batch inverts a subgroup element"""
    ctx = contexts(name)
    els, want = GM.inverse_case_schnorr(name, 1, placed=False)
    assert els[0] % ctx.p > 1 and want[0] != 0
    check_inverse(ctx.G, els, want, multinv=True)


@pytest.mark.parametrize("n", GM.INV_SIZES_RING)
@pytest.mark.parametrize("name", GM.RING)
def test_batch_inverse_on_the_ring_moduli(contexts, name, n):
    """Units, 0 and p against the closed form a_i^-1 t^(p-1) of the segmented inversion (the module
    docstring says why, and why zero divisors are left out)."""
    ctx = contexts(name)
    els, want = GM.inverse_case_ring(ctx.name, n)
    check_inverse(ctx.G, list(els), list(want), multinv=False)


# ---------------------------------------------------------------------------------------------------
# dLog counts
# ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def mirror_counts(name, max_count, fp_bits):
    p, _, g = GM.groups()[name]
    return D.Table(p, g, max_count, fp_bits).counts(GM.count_texts(name, max_count)[0])


def window(ys, want, n, off):
    idx = [(off + i) % len(ys) for i in range(n)]
    return [ys[i] for i in idx], [want[i] for i in idx]


@pytest.mark.parametrize("fp_bits", GM.FP_BITS, ids=["fp64", "fp8"])
@pytest.mark.parametrize("max_count", GM.MAX_COUNTS)
@pytest.mark.parametrize("name", GM.SCHNORR)
def test_counts_on_the_schnorr_groups(contexts, name, max_count, fp_bits):
    """The exponents 0, 1, m - 1, m, m + 1, max_count and the non-exponents g^(max_count + 1), g^(q - 1),
    0, p - 1: the largest exponent alone, then nine texts from the front and nine up to the end of the
    list; without M, and with an M that has one zero row (at one text that is its only row, so the one
    text is decoded through a non-zero M too); host and _dev at nine texts."""
    ctx = contexts(name)
    from electionguard import decode as dc
    G, name, q = ctx.G, ctx.name, ctx.q
    ys, want = GM.count_texts(name, max_count)
    assert mirror_counts(name, max_count, fp_bits) == list(want)
    rng = random.Random("counts-%s-%d" % (name, max_count))
    M9 = G.gPowP_batch([rng.randrange(1, q) for _ in range(9)])
    tab = dc.DecodeTable(G, max_count, fp_bits)
    try:
        top = want.index(max_count)
        batches = [([ys[top]], [max_count])] + [window(ys, want, 9, off) for off in (0, max(0, len(ys) - 9))]
        for y, w in batches:
            n = len(y)
            Y = rows(y)
            got = tab.counts(Y)                                     # M = NULL: a plain dLog
            assert got.dtype == np.int64 and got.shape == (n,) and got.tolist() == w, (name, n, "no M")
            M = M9[:n].copy()
            B = G.multP_batch(Y, M)
            z = n // 2
            M[z] = 0
            wm = list(w)
            wm[z] = -1
            assert tab.counts(B, M).tolist() == wm, (name, n, "M")
            if n == 1:
                assert tab.counts(B, M9[:1]).tolist() == w, (name, n, "non-zero M")
            if n == 9:
                dev = tab.counts(G.to_device(B), G.to_device(M))
                assert not isinstance(dev, np.ndarray) and dev.download().tolist() == wm
                assert tab.counts(G.to_device(Y)).download().tolist() == w
    finally:
        tab.close()


# ---------------------------------------------------------------------------------------------------
# the shuffle on the two general Schnorr groups
# ---------------------------------------------------------------------------------------------------
# (2, 1) with the swap and (7, 3); on sparse_c, whose q has 255 bits, also (9, 2) with the edge nonces
# 0, 1, q - 1, q, 2^256 - 1 and the edge elements of test_gpu_shuffle.case
SHUFFLE_CASES = [(name, shape) for name in GM.GENERAL
                 for shape in [(2, 1), (7, 3)] + ([(9, 2)] if name == "sparse_c" else [])]
shuffle_cases = pytest.mark.parametrize("name,shape", SHUFFLE_CASES,
                                        ids=["%s-%dx%d" % (n, *s) for n, s in SHUFFLE_CASES])


# The CPython references, each computed once per module and when a test first needs it.
@lru_cache(maxsize=None)
def ref_gen(name, k):
    p, q, _ = GM.groups()[name]
    return R.gen(p, q, GSEED, k)


@lru_cache(maxsize=None)
def ref_case(name, shape):
    """the case of test_gpu_shuffle.case (with its CPython mix) and the generators"""
    p, q, g = GM.groups()[name]
    N, w = shape
    c = case(SimpleNamespace(p=p, q=q, g=g), N, w, 11 * N + w)
    gens = [ref_gen(name, k) for k in range(N + 1)]
    prod = 1
    for x in gens[1:]:
        prod = prod * x % p
    c.G = gens + [prod]
    c.Gb, c.E2b = be_rows(c.G, 512), rows_of(c.E2)
    return c


@lru_cache(maxsize=None)
def ref_proof(name, shape):
    """-> (nonce rows, the reference proof): nonces with the edge values at (9, 2), as in
    test_gpu_shuffle.proofs"""
    p, q, g = GM.groups()[name]
    N, w = shape
    c = ref_case(name, shape)
    rng = random.Random(1000 + N)
    nonces = [rng.randrange(q) for _ in range(4 * N + 3 + w)]
    if shape == (9, 2):
        for k, x in enumerate([0, 1, q - 1, q, 2**256 - 1]):
            nonces[k] = nonces[N + 1 + k] = nonces[2 * N + 2 + k] = nonces[3 * N + 3 + k] = x
        nonces[4 * N], nonces[4 * N + 3] = q, 2**256 - 1
    return be_rows(nonces, 32), R.prove(p, q, g, c.K, QBAR, GSEED, c.G, c.E, c.E2, c.psi, c.r, nonces)


@lru_cache(maxsize=None)
def ref_verdict(name, shape):
    """the reference's own verdict on its proof"""
    p, q, g = GM.groups()[name]
    c = ref_case(name, shape)
    return R.verify(p, q, g, c.K, QBAR, GSEED, c.G, c.E, c.E2, ref_proof(name, shape)[1], True)


@shuffle_cases
def test_shuffle_generators(contexts, name, shape):
    from electionguard import shuffle as S
    G, c = contexts(name).G, ref_case(name, shape)
    assert ints(S.generators(G, GSEED, c.N)) == c.G
    if shape == (7, 3):
        assert ints(S.generators(G, GSEED, 7, device=True).download()) == c.G


@shuffle_cases
def test_shuffle_mix(contexts, name, shape):
    from electionguard import shuffle as S
    G, c = contexts(name).G, ref_case(name, shape)
    out = S.mix(G, c.K, c.rows, c.psi32, c.rbytes)
    assert out.shape == (c.N, c.w, 2, 512) and S.rows_to_ints(out) == c.E2
    if shape == (7, 3):
        dev = S.mix(G, c.K, G.to_device(c.rows), G.to_device(c.psi32), G.to_device(c.rbytes))
        assert np.array_equal(dev.download(), out)


@shuffle_cases
def test_shuffle_prove(contexts, name, shape):
    """every output byte of the prover against shuffle_ref.prove"""
    from electionguard import shuffle as S
    G, c = contexts(name).G, ref_case(name, shape)
    nb, want = ref_proof(name, shape)
    names = ("pc", "chain", "c", "s", "s_hat", "s_prime")
    for device in ((False, True) if shape == (7, 3) else (False,)):
        f = (lambda a: G.to_device(np.ascontiguousarray(a))) if device else (lambda a: a)
        got = S.prove(G, c.K, QBAR, GSEED, f(c.Gb), f(c.rows), f(c.E2b), f(c.psi32), f(c.rbytes), f(nb))
        if device:
            got = S.ShuffleProof(*[getattr(got, k).download() for k in names])
        got = got.to_ints()
        for k in names:
            assert getattr(got, k) == getattr(want, k), (device, k)


@shuffle_cases
def test_shuffle_verify_and_a_flipped_response(contexts, name, shape):
    """The reference accepts its own proof, and so does the GPU; at (7, 3) also the _dev variant, and
    one flipped bit of a response turns verify false with the challenge bit of the mask."""
    from electionguard import shuffle as S
    ctx, c = contexts(name), ref_case(name, shape)
    G = ctx.G
    pr = proof_arrays(ref_proof(name, shape)[1])
    assert ref_verdict(name, shape) == (True, 0)
    assert S.verify(G, c.K, QBAR, GSEED, c.Gb, c.rows, c.E2b, pr, check_inputs=True) == (True, 0)
    if shape == (7, 3):
        f = lambda a: G.to_device(np.ascontiguousarray(a))
        dpr = S.ShuffleProof(*[f(x) for x in (pr.pc, pr.chain, pr.c, pr.s, pr.s_hat, pr.s_prime)])
        ok, failed = S.verify(G, c.K, QBAR, GSEED, f(c.Gb), f(c.rows), f(c.E2b), dpr, check_inputs=True)
        assert (bool(ok.download()[0]), int(failed.download()[0])) == (True, 0)
        bad = pr.s_hat.copy()
        bad[3, 31] ^= 1                                              # one bit of one response: still below q
        assert int.from_bytes(bytes(bad[3]), "big") < ctx.q
        tampered = S.ShuffleProof(**{**vars(pr), "s_hat": bad})
        assert S.verify(G, c.K, QBAR, GSEED, c.Gb, c.rows, c.E2b, tampered, check_inputs=True) == \
            (False, R.CHALLENGE)


@pytest.mark.parametrize("name", GM.GENERAL)
def test_shuffle_draws_and_proves(contexts, name):
    from electionguard import shuffle as S
    ctx, c = contexts(name), ref_case(name, (7, 3))
    G = ctx.G
    rows2, proof = S.shuffle(G, c.K, QBAR, c.rows, GSEED)
    Gb = S.generators(G, GSEED, 7)
    assert S.verify(G, c.K, QBAR, GSEED, Gb, c.rows, rows2, proof, check_inputs=True) == (True, 0)
    assert R.verify(ctx.p, ctx.q, ctx.g, c.K, QBAR, GSEED, ints(Gb), c.E,
                    S.rows_to_ints(rows2), proof.to_ints(), True) == (True, 0)


# ---------------------------------------------------------------------------------------------------
# the degenerate group (last: it is the eleventh context of the module)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp_bits", GM.FP_BITS, ids=["fp64", "fp8"])
def test_counts_on_the_degenerate_group(contexts, fp_bits):
    """max_count = 4000, m = 64: 2^t -> t for t in {0, 1, 63, 64, 65, 2047, 4000}; 2^4001, 3, 0 and p
    -> -1; with M[i] = 2^k and B[i] = 2^(t + k mod 4096): t for k in {2048, 0}, and for k in
    {1, 5, 2047, 4095} what the mirror gives (t - 2 k mod 4096 where that is at most 4000)."""
    ctx = contexts(GM.DEGENERATE)
    from electionguard import decode as dc
    G = ctx.G
    ys, want = GM.degenerate_texts()
    tab = dc.DecodeTable(G, GM.DEG_MAX_COUNT, fp_bits)
    try:
        Y = rows(ys)
        assert tab.counts(Y).tolist() == want
        assert tab.counts(G.to_device(Y)).download().tolist() == want
        for ks in (GM.DEG_K_INVERTIBLE, GM.DEG_K_OTHER):
            B, M, wm = GM.degenerate_with_m(ks)
            if ks is GM.DEG_K_INVERTIBLE:
                assert wm == want
            assert tab.counts(rows(B), rows(M)).tolist() == wm, ks
            assert tab.counts(G.to_device(rows(B)), G.to_device(rows(M))).download().tolist() == wm, ks
    finally:
        tab.close()


def test_batch_inverse_of_single_bits(contexts):
    """17 single-bit elements of the degenerate group: one level of segments of 4 (inv_plan(17)), every
    product and every result a single bit"""
    ctx = contexts(GM.DEGENERATE)
    els = [1 << (241 * i % 4096) for i in range(17)]
    assert D.inv_plan(17) == (4, 1, 5)
    check_inverse(ctx.G, els, GM.inverse_closed_form(GM.DEG_P, els), multinv=False)
