"""CPU: the adversarial-modulus fixtures (tests/adversarial_moduli.py) are what they claim to be, and
a column model of the 8-lane Montgomery multiply and of its half-row squaring (eg_bignum.hpp,
mont_mul_impl<*, false> and <*, true>) on those fixtures.

The model restates the kernel's schedule on Python integers: 8 lanes x 18 accumulator registers, 142
CIOS steps, register (j + r) % 18 of a lane holding position j at rotation r; after each step the
retiring register keeps the low 29 bits of the lane above (0 for the top lane) and its carry is added to
the lane's next register -- so a register lives 18 steps in its lane, its low 29 bits move to the lane
below and its carry stays.  Then the two carry passes.  The squaring doubles x and adds, at the row of
register r, the diagonal (x_r on the row's own lane, 2 x_r above it, 0 below) and the doubled partners
r+1 .. r+9 (r < 9) or r+8 of every lane.  The result must be x * y * R^-1 mod p below 2p, and every
64-bit accumulator column must stay below 2^64 (the header bounds a multiply by 36 x (2^29 + 2^6)^2 +
2^35 < 2^63.2 and a squaring by 18 x (2^59 + 2^58) < 2^63.8).

Measured peak columns, log2 (test_column_model_peaks prints them; x = y = p - 1 unless said otherwise,
the second figure of a pair is the peak over three further operations on the kernel's own
non-canonical output limbs):

    modulus, operands                     multiply          squaring
    random p, random operands             61.59             61.94
    ones       (2^4096 - 1)               62.17 / 62.17     62.32 / 62.32
    f58_dense  (2^4096 - 2^58 - 1)        62.81 / 62.81     62.86 / 62.86
    f58_only                              61.66 / 61.66     61.73 / 61.78
    f29_only                              61.64 / 61.86     61.72 / 62.00
    gen_dense  (2^4096 - 3)               62.75 / 62.75     62.86 / 62.86
    gen_square ((2^2048 - 1)^2)           62.17 / 63.17     62.32 / 63.25
    min_top    (2^4095 + 1)               12.00 / 48.00     12.00 / 48.00

The multiply figures of ones, f58_dense and gen_dense reproduce the ones that motivated these fixtures
(62.17, 62.81, 62.76; a random modulus gave 61.51 there, another draw).  The highest, gen_square after
the first operation (the running value is then a multiple of 2^2048 - 1 with saturated limbs, and n0 =
2^29 - 1 makes every quotient digit large), sits at the header's multiply bound of 2^63.17 and below
its 2^63.2; no column reaches 2^64.  p - 1 of min_top is 2^4095: one non-zero limb."""
import math
import random

import pytest

import adversarial_moduli as A
from adversarial_moduli import B, MASK, N_LIMBS, R, STEPS

T, L = 8, 18  # lanes per element, limbs per lane
SATURATED = ("ones", "f58_dense", "gen_dense", "gen_square")  # moduli whose limbs are (nearly) all 2^29 - 1


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMES)
def test_modulus_shape_and_predicates(name):
    p = A.moduli()[name]
    assert p % 2 == 1 and p >> 4095 == 1 and p < A.TOP          # odd, top bit set, 4096 bits
    mode = A.EXPECTED_MODE[name]
    assert A.wave_mode(p) == mode
    assert A.friendly(p) == (mode != 0) == ((p + 1) % (1 << B) == 0)
    assert A.d2_predicate(p) == ((p + 1) % (1 << 58) == 0)
    if mode == 2:
        assert A.d2_predicate(p) and A.wave_mode(p, d2_enabled=False) == 1
        assert (A.pt2(p) != 0) == A.PT2_NONZERO[name]
    if mode == 1:
        assert not A.d2_predicate(p) and (p >> B) & 1 == 0     # exactly 29 low ones
    assert (p * A.n0(p) + 1) % (1 << B) == 0


def test_moduli_cover_every_mode():
    modes = [A.EXPECTED_MODE[n] for n in A.NAMES]
    assert set(modes) == {0, 1, 2}
    d2 = [n for n in A.NAMES if A.EXPECTED_MODE[n] == 2]
    assert any(A.pt2(A.moduli()[n]) == 0 for n in d2) and any(A.pt2(A.moduli()[n]) != 0 for n in d2)
    M = A.moduli()
    assert M["ones"] == 2**4096 - 1 and M["f58_dense"] == 2**4096 - 2**58 - 1 and M["gen_dense"] == 2**4096 - 3
    assert M["gen_square"] == 2**4096 - 2**2049 + 1 and M["min_top"] == 2**4095 + 1
    assert A.pt2(M["f58_dense"]) == MASK                          # the largest delayed term
    assert A.n0(M["gen_square"]) == MASK                          # p = 1 mod 2^29: the largest quotient multiplier
    assert A.n0(M["gen_dense"]) == pow(3, -1, 1 << B)
    assert all(l == 0 for l in A.limbs(M["min_top"])[1:141])      # every middle limb zero
    assert 2 * M["min_top"] - 3 == 2**4096 - 1                    # the largest unreduced import, just below 2p
    # the random fixtures are fixed: the same values on every run
    assert M["f58_only"] % 1000003 == A._f58_only() % 1000003 and M["f29_only"] == A._f29_only()


@pytest.mark.parametrize("name", A.NAMES)
def test_directed_operands(name):
    p = A.moduli()[name]
    vs, bs = A.directed_values(name), A.directed_bases(name)
    assert len(vs) == len(bs) == len(set(vs)) and 32 <= len(vs) <= 72  # (min_top: zeroing a zero limb changes nothing)
    for v, b in zip(vs, bs):
        assert 0 <= b < p and b * R % p == v                    # mont_preimage round-trips
    assert p - 1 in vs and 1 in vs and R % p in vs
    if name != "min_top":
        assert any(bin(v).count("1") > 4000 for v in vs)        # saturated operands
    for v in A.import_edges(name):
        assert p <= v < A.TOP


@pytest.mark.parametrize("name", A.NAMES)
def test_result_directed_pairs(name):
    p = A.moduli()[name]
    pairs = A.result_pairs(name)
    assert len(pairs) <= 128
    targets = {t for _, _, t in pairs}
    for a, b, t in pairs:
        assert 0 <= a < p and 0 <= b < p and a * b % p == t
    assert {1, p - 1, 1 << 4095} <= targets
    for k in (B * 18, B * 9, B * 3, B * 18 * 7, B * 9 * 15, B * 3 * 47):
        assert (1 << k) % p in targets and ((1 << k) - 1) % p in targets
    assert (0 in targets) == (name in A.ZERO_DIVISORS)
    for length in (1, 2, 7, 33):
        xs, ts = A.product_chain(name, length)
        assert len(xs) == length
        run = 1
        for x, t in zip(xs, ts):
            run = run * x % p
            assert run == t


def test_zero_divisors_and_nilpotent():
    M = A.moduli()
    for name, (u, v) in A.ZERO_DIVISORS.items():
        p = M[name]
        assert 1 < u < p and 1 < v < p and u * v % p == 0 and u * v == p
    p = M["gen_square"]
    b = 2**2048 - 1
    assert [pow(b, e, p) for e in (1, 2, 3, 2**256 - 1)] == [b, 0, 0, 0]
    assert all(math.gcd(a, M[n]) == 1 for n in A.NAMES for a, _, t in A.result_pairs(n) if t != 0)


def test_routes():
    for name in A.NAMES:
        rs = [r for r, _ in A.routes_for(name)]
        assert rs[:4] == ["lanes8", "lanes16", "wave4_r2l", "wave1"]
        assert ("wave1_cios" in rs) == ("wave4_r2l_cios" in rs) == (A.EXPECTED_MODE[name] == 2)
        assert [A.is_latency_route(r) for r in rs[:2]] == [False, True]
        for _, env in A.routes_for(name) + A.routes_for(name, A.FB_ROUTES):
            assert set(env) <= set(A.KNOBS)


# ---------------------------------------------------------------------------------------------------
# the column model
# ---------------------------------------------------------------------------------------------------
def lane_limbs(v):
    """canonical limbs, [lane][register]"""
    l = A.limbs(v)
    return [l[k * L:(k + 1) * L] for k in range(T)]


def lanes_value(x):
    return sum(x[l][j] << (B * (l * L + j)) for l in range(T) for j in range(L))


class Peak:
    def __init__(self):
        self.v = 0

    def see(self, a):
        if a > self.v:
            self.v = a
        return a


def mont_model(x, y, p, sqr, peak):
    """mont_mul_impl<*, sqr>: x, y as [lane][limb] (limbs as the kernel holds them, possibly above 2^29);
    returns the result limbs the same way.  With sqr the multiplier is x itself."""
    n0 = A.n0(p)
    pl = lane_limbs(p)
    if sqr:
        y = x
        x2 = [[v << 1 for v in lane] for lane in x]
    yflat = [y[l][j] for l in range(T) for j in range(L)]
    acc = [[0] * L for _ in range(T)]
    for i in range(STEPS):
        r, s = i % L, i // L
        yi = yflat[i]
        if sqr:
            jmax = L // 2 if r < L // 2 else L // 2 - 1
            for l in range(T):
                d = x2[l][r] if l > s else (x2[l][r] >> 1 if l == s else 0)
                a = acc[l]
                a[(r + r) % L] += d * yi
                for jj in range(1, jmax + 1):
                    j = (r + jj) % L
                    a[(j + r) % L] += x2[l][j] * yi
        else:
            for l in range(T):
                a, xl = acc[l], x[l]
                for j in range(L):
                    a[(j + r) % L] += xl[j] * yi
        m = ((acc[0][r] & 0xFFFFFFFF) * n0) & MASK
        for l in range(T):
            a, ql = acc[l], pl[l]
            for j in range(L):
                a[(j + r) % L] += ql[j] * m
        assert acc[0][r] & MASK == 0
        low = [acc[l][r] & MASK for l in range(T)]
        for l in range(T):
            a = acc[l]
            peak.see(a[r])  # every addend is non-negative: a register peaks when it retires
            a[(r + 1) % L] += a[r] >> B
            a[r] = low[l + 1] if l + 1 < T else 0
    rot = STEPS % L
    for a in acc:
        peak.see(max(a))
    # the two carry passes (the carry out of a lane's top register goes to the lane above)
    d = [[0] * L for _ in range(T)]
    for l in range(T):
        for j in range(L):
            c = (acc[l][(rot + j - 1) % L] >> B) if j else (acc[l - 1][(rot + L - 1) % L] >> B if l else 0)
            d[l][j] = (acc[l][(rot + j) % L] & MASK) + c
    out = [[0] * L for _ in range(T)]
    for l in range(T):
        for j in range(L):
            c = (d[l][j - 1] >> B) if j else (d[l - 1][L - 1] >> B if l else 0)
            out[l][j] = (d[l][j] & MASK) + c
            assert out[l][j] < 1 << 32
    assert acc[T - 1][(rot + L - 1) % L] >> B == 0 and d[T - 1][L - 1] >> B == 0  # nothing leaves the top lane
    return out


def run_model(p, x, y, sqr, follow=3):
    """(peak of the first operation, peak over `follow` further operations on the non-canonical
    output limbs), each result checked against CPython"""
    rinv = pow(R, -1, p)
    pk = Peak()
    xl = lane_limbs(x)
    out = mont_model(xl, None if sqr else lane_limbs(y), p, sqr, pk)
    v = lanes_value(out)
    want = x * (x if sqr else y) * rinv % p
    assert v < 2 * p and v % p == want
    first = pk.v
    for _ in range(follow):
        prev_v = v
        out = mont_model(out, None if sqr else out, p, sqr, pk)
        v = lanes_value(out)
        assert v < 2 * p and v % p == prev_v * prev_v * rinv % p
    return first, pk.v


def test_column_model_peaks():
    rng = random.Random(29)
    lg = lambda a: math.log2(a)
    # the baseline: a random modulus with random operands
    p = rng.getrandbits(4096) | (1 << 4095) | 1
    base = {}
    for sqr in (False, True):
        first, _ = run_model(p, rng.randrange(p), rng.randrange(p), sqr, follow=0)
        base[sqr] = first
        assert first < 1 << 64
    print("\nrandom p, random operands: multiply 2^%.2f, squaring 2^%.2f" % (lg(base[False]), lg(base[True])))
    over = []
    for name in A.NAMES:
        p = A.moduli()[name]
        x = p - 1
        res = {}
        for sqr in (False, True):
            first, later = run_model(p, x, x, sqr)
            res[sqr] = (first, later)
            if later >= 1 << 64:
                over.append((name, sqr, lg(later)))
            # eg_bignum.hpp's own bounds: 2^63.2 for a multiply, 2^63.8 for a squaring
            assert later < (2**63.8 if sqr else 2**63.2), (name, sqr, lg(later))
        print("%-10s x = y = p - 1: multiply 2^%.2f / 2^%.2f, squaring 2^%.2f / 2^%.2f" %
              (name, lg(res[False][0]), lg(res[False][1]), lg(res[True][0]), lg(res[True][1])))
        if name in SATURATED:
            assert res[False][1] > base[False] and res[True][1] > base[True], name
    assert not over, over  # a peak at or past 2^64 is a finding about eg_bignum.hpp's bound


@pytest.mark.parametrize("name", A.NAMES)
def test_column_model_directed_operands(name):
    """the model is exact on a sample of the directed Montgomery-domain operands (both schedules)"""
    p = A.moduli()[name]
    vs = A.directed_values(name)
    rng = random.Random(name)
    for v in rng.sample(vs, 3):
        w = rng.choice(vs)
        for sqr in (False, True):
            for x in (v, v + p):  # either representative of the lazy domain [0, 2p)
                first, _ = run_model(p, x, w, sqr, follow=0)
                assert first < 1 << 64
