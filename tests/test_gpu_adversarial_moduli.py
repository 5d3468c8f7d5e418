"""GPU: every Montgomery instantiation on adversarial moduli and saturated operands, bit-exact against
CPython's pow and * (no tolerance).  The fixtures are tests/adversarial_moduli.py (checked on the CPU by
tests/test_adversarial_moduli.py); eg_ctx_create takes any odd modulus with the top bit set.

    ones        2^4096 - 1             friendly, per-wave mode 2 with p~_2 = 0; every limb saturated;
                                       composite: (2^2048 - 1)(2^2048 + 1); p + 1 carries out of word 127
    f58_dense   2^4096 - 2^58 - 1      mode 2 with p~_2 = 2^29 - 1, the largest delayed term
    f58_only    random, -1 mod 2^58    mode 2 with a random p~_2 != 0
    f29_only    random, -1 mod 2^29    mode 1 on the per-wave kernel; friendly on 8 and 16 lanes
    gen_dense   2^4096 - 3             general path, saturated limbs
    gen_square  (2^2048 - 1)^2         general path, n0 = 2^29 - 1; 2^2048 - 1 is nilpotent
    min_top     2^4095 + 1             the smallest modulus: 2^4096 - 1 is the largest unreduced import

Routes (adversarial_moduli.POW_ROUTES; the knobs are read when the context is made, so each case sets
them with monkeypatch and makes its own context): the 8-lane k_pow (EG_LATENCY_POW=0), the 16-lane
eg16::k_pow (=16), the per-wave kernel with 4 waves per job right to left (the default for n <= compute
units) and with one wave per element (EG_WAVE_R2L=0), and on the mode-2 moduli both of these with the
per-step quotient (EG_POWWAVE_D2=0: mode 1).  Route evidence: the profile window counts k_pow launches,
so it reports >= 1 on the 8-lane route and 0 on a latency route; the 16-lane and the per-wave routes
are told apart only by the documented knobs (no export reports the kernel that ran).

What these cases catch, tried once against deliberately broken builds: with the export's cross-lane carry
ripple cut to one round (regs_normalize and the per-wave normalize) the result-directed groups fail on
every modulus and the powP group on every saturated one; with the delayed term p~_2 dropped from the
per-wave constants exactly the delayed-quotient routes of f58_dense and f58_only fail, and nothing on
ones or the production group can.

Batches stay at n <= 128 per call except one fixed-base call of 1025 repeated exponents, which is what
it takes to pass the per-wave limit of one element per SIMD (1024 on 256 compute units)."""
import random
from functools import lru_cache

import pytest

import adversarial_moduli as A
from conftest import be2i

pytestmark = pytest.mark.gpu

CHUNK = 128
CT = (False, True)
POW_CASES = [(n, r, ct) for n, r in A.cases() for ct in CT]
FB_CASES = [(n, r, ct) for n, r in A.cases(A.FB_ROUTES) for ct in CT]
ids3 = lambda cs: ["%s-%s-%s" % (n, r, "ct" if ct else "vt") for n, r, ct in cs]


def small_exps():
    q = A.production_q()
    return (2, 3, 15, 16, 31, 1 << 255, (1 << 256) - 1, q)


@lru_cache(maxsize=None)
def pow_jobs(name):
    """(label, base, exponent, expected) of the variable-base jobs of one modulus; the CPython
    references are computed once and shared by every route"""
    p = A.moduli()[name]
    jobs = []
    # the small exponents keep the saturated value as the running multiplier through the window-table build
    for i, b in enumerate(A.directed_bases(name)):
        for e in small_exps():
            jobs.append(("directed[%d]^%d" % (i, e), b, e, pow(b, e, p)))
    for v in A.import_edges(name):                                  # unreduced inputs, exponent 1
        jobs.append(("import %#x.." % (v >> 4064), v, 1, v % p))
    for b in (0, p):                                                # both forms of zero
        for e in (1, 2, (1 << 256) - 1):
            jobs.append(("zero^%d" % e, b, e, 0))
    if name in A.ZERO_DIVISORS:
        # gen_square: 2^2048 - 1 is nilpotent, b^2 = 0 appears inside the chain and is squared onward
        # as the lazy-domain p; ones: a zero divisor, never 0 itself
        u = A.ZERO_DIVISORS[name][0]
        for e in (1, 2, 3, (1 << 256) - 1):
            jobs.append(("zero divisor^%d" % e, u, e, pow(u, e, p)))
        if name == "gen_square":
            assert [j[3] for j in jobs[-4:]] == [u, 0, 0, 0]
    return tuple(jobs)


def check(got_rows, jobs, what):
    bad = [(what, j[0]) for row, j in zip(got_rows, jobs) if be2i(row) != j[3]]
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("name,route,ct", POW_CASES, ids=ids3(POW_CASES))
def test_powp_directed_zero_and_import_edges(monkeypatch, name, route, ct):
    """powP on the directed Montgomery-domain operands (exponents 2, 3, 15, 16, 31, 2^255, 2^256 - 1, q),
    on 0, p, the zero divisors / the nilpotent base, and on the unreduced inputs p, p + 1, 2^4096 - 1
    with exponent 1; the profile window shows whether the 8-lane k_pow ran."""
    jobs = pow_jobs(name)
    G = A.open_group(monkeypatch, name, route)
    try:
        G.ct_pow = ct
        for k in range(0, len(jobs), CHUNK):
            part = jobs[k:k + CHUNK]
            if k == 0:
                G.profile_begin()
            out = G.powP_batch([j[1] for j in part], [j[2] for j in part])
            if k == 0:
                launches = G.profile_end().launches
                assert (launches == 0) if A.is_latency_route(route) else (launches >= 1), (route, launches)
            check(out, part, (name, route, ct))
    finally:
        G.close()


@lru_cache(maxsize=None)
def inverse_jobs(name):
    """multInv as eg_multinv_batch documents it: a^(q-1) where that is the inverse, else a^(p-2) (on a
    composite modulus that is not an inverse, but it is what the code computes; 0 is left out)"""
    p, q = A.moduli()[name], A.production_q()
    rng = random.Random("inv-" + name)
    xs = [1, p - 1, 2, A._unit(rng, p), A.mont_preimage(p - 1, p)]
    jobs = []
    for a in xs:
        r = pow(a, q - 1, p)
        jobs.append(("inv %#x.." % (a >> 4064), a, None, r if r * a % p == 1 else pow(a, p - 2, p)))
    assert jobs[0][3] == 1
    return tuple(jobs)


@pytest.mark.parametrize("name,route,ct", POW_CASES, ids=ids3(POW_CASES))
def test_multinv(monkeypatch, name, route, ct):
    """a^(q-1) on the route's layout, the check multiply, then a^(p-2) on the 8-lane k_pow with its
    512-byte exponent: on the dense moduli 4096 bits of nearly all ones."""
    jobs = inverse_jobs(name)
    G = A.open_group(monkeypatch, name, route)
    try:
        G.ct_pow = ct
        check(G.multInv_batch([j[1] for j in jobs]), jobs, (name, route, ct))
    finally:
        G.close()


@lru_cache(maxsize=None)
def mult_jobs(name):
    p = A.moduli()[name]
    jobs = [("pair -> %#x.." % (t >> 4064), a, b, t) for a, b, t in A.result_pairs(name)]
    jobs += [("import %#x.. * 1" % (v >> 4064), v, 1, v % p) for v in A.import_edges(name)]
    jobs += [("1 * import", 1, v, v % p) for v in A.import_edges(name)]
    return tuple(jobs)


@pytest.mark.parametrize("name", A.NAMES)
def test_result_directed_multp_and_prodp(monkeypatch, name):
    """multP_batch and prodP_groups on operands chosen by their RESULT: 0 through zero divisors, 1,
    p - 1, 2^4095, and 2^k, 2^k - 1 at every lane boundary of the three layouts -- long runs of zeros and
    ones for the cross-lane carry ripple of the export.  k_mul and k_prod exist on the 8-lane layout
    only, so this group runs there alone.  The product groups have lengths 1, 2, 7 and 33 and their
    running products pass through the targets."""
    p = A.moduli()[name]
    G = A.open_group(monkeypatch, name, "lanes8")
    try:
        jobs = mult_jobs(name)
        for k in range(0, len(jobs), CHUNK):
            part = jobs[k:k + CHUNK]
            check(G.multP_batch([j[1] for j in part], [j[2] for j in part]), part, (name, "multP"))
            check(G.multP_batch([j[2] for j in part], [j[1] for j in part]), part, (name, "multP swapped"))
        rng = random.Random("prod-" + name)
        for length in (1, 2, 7, 33):
            xs, ts = A.product_chain(name, length)
            groups = [list(xs), list(reversed(xs))]
            if name in A.ZERO_DIVISORS and length >= 2:  # a product that becomes 0 inside the chain
                u, v = A.ZERO_DIVISORS[name]
                z = list(xs)
                z[length // 2 - 1], z[length // 2] = u * A._unit(rng, p) % p, v * A._unit(rng, p) % p
                groups.append(z)
            want = []
            for g in groups:
                r = 1
                for x in g:
                    r = r * x % p
                want.append(r)
            assert want[0] == ts[-1] and (len(groups) < 3 or want[2] == 0)
            out = G.prodP_groups([x for g in groups for x in g], len(groups), length)
            assert [be2i(r) for r in out] == want, (name, length)
    finally:
        G.close()


@pytest.mark.parametrize("name", A.NAMES)
def test_result_directed_multp_per_wave(monkeypatch, name):
    """The same pairs as per-element jobs: queued together they form one batch of the per-wave kernel
    (two bases, no exponent: one wave per job, the modulus's mode), whose export ripples carries over
    up to 47 lane hops."""
    jobs = mult_jobs(name)
    G = A.open_group(monkeypatch, name, "wave4_r2l")
    try:
        tickets = [G.mexp_submit([j[1], j[2]]) for j in jobs]
        got = [t.wait() for t in tickets]
        check(got, jobs, (name, "per-wave multP"))
    finally:
        G.close()


@lru_cache(maxsize=None)
def fixed_jobs(name):
    p, q = A.moduli()[name], A.production_q()
    rng = random.Random("fb-" + name)
    base = A.mont_preimage(p - 1, p)  # the Montgomery-domain base is p - 1: saturated limbs
    exps = [0, 1, q - 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(16)]
    return base, tuple(exps), tuple(pow(base, e, p) for e in exps), tuple(pow(A.G, e, p) for e in exps)


@pytest.mark.parametrize("name,route,ct", FB_CASES, ids=ids3(FB_CASES))
def test_fixed_base(monkeypatch, name, route, ct):
    """gPowP_batch and fixed_base(base, window_bits) with 4-, 9- and 16-bit windows over a saturated
    base: a small batch (the per-wave fixed-base kernel, 4 waves per job; the 8-lane k_pow with
    EG_LATENCY_POW=0), 1025 elements (past one per SIMD: the 8-lane k_pow) and per-element jobs queued
    into one batch (8 waves per job on a mode-2 modulus, 4 with EG_WAVE_W8=0 or in any other mode)."""
    base, exps, want, gwant = fixed_jobs(name)
    G = A.open_group(monkeypatch, name, route, A.FB_ROUTES)
    try:
        G.ct_pow = ct
        assert [be2i(r) for r in G.gPowP_batch(exps)] == list(gwant), (name, route, ct, "gPowP_batch")
        tickets = [G.mexp_submit([], None, [(None, e)]) for e in exps]
        assert [be2i(t.wait()) for t in tickets] == list(gwant), (name, route, ct, "gPowP per element")
        for wbits in (4, 9, 16):
            fb = G.fixed_base(base, window_bits=wbits)
            try:
                assert [be2i(r) for r in fb.pow_batch(exps)] == list(want), (name, route, ct, wbits, "batch")
                tickets = [G.mexp_submit([], None, [(fb, e)]) for e in exps]
                assert [be2i(t.wait()) for t in tickets] == list(want), (name, route, ct, wbits, "per element")
                if route == "wave":
                    n = 1025
                    out = fb.pow_batch([exps[i % len(exps)] for i in range(n)])
                    bad = [i for i in range(n) if be2i(out[i]) != want[i % len(exps)]]
                    assert not bad, (name, route, ct, wbits, "n = 1025", bad[:6])
            finally:
                fb.close()
    finally:
        G.close()
