"""CPU: the fixtures of tests/general_moduli.py are what they claim to be.  The Schnorr groups and the
degenerate group have g of order dividing q; sparse_c and dense_c select the general Montgomery
instantiation and Mode4096_V2 and `ones` the friendly one; on the composite moduli a^(p-2) is no
inverse, and what the segmented inversion gives there instead (general_moduli.inverse_closed_form:
a_i^-1 t^(p-1) with t the product of the top-level block) is what its CPython mirror
decode_ref.batch_inverse computes; decode_ref's table decodes the single-bit powers of the
degenerate group."""
import math
import random

import pytest

import adversarial_moduli as A
import decode_ref as D
import general_moduli as GM


@pytest.mark.parametrize("name", GM.SCHNORR + (GM.DEGENERATE,))
def test_generator_has_order_q(name):
    p, q, g = GM.groups()[name]
    assert p % 2 == 1 and p >> 4095 == 1 and p < GM.TOP
    assert g != 1 and pow(g, q, p) == 1
    if name in GM.SCHNORR:
        assert (p - 1) % q == 0 and D.is_prime(q)           # the shuffle's cofactor exists
    else:
        assert all(pow(g, q // f, p) != 1 for f in (2,))    # q = 2^12: the order is q itself
        assert A.R % p == 1 << 22                           # every Montgomery form of 2^t is a single bit


def test_which_instantiation_each_modulus_selects():
    G = GM.groups()
    assert [A.n0(G[n][0]) != 1 for n in GM.GENERAL] == [True, True]
    assert A.n0(G["Mode4096_V2"][0]) == 1 and A.n0(G["ones"][0]) == 1 and A.n0(GM.DEG_P) == 1
    import eg_oracle as O
    assert G["Mode4096_V2"][0] != O.production_group().p    # a second prime for the friendly kernels
    assert G["sparse_c"][1] < 1 << 255 <= G["dense_c"][1] < (1 << 256) - 189   # addmod256 never carries on the first
    assert [A.friendly(G[n][0]) for n in GM.RING] == [A.EXPECTED_MODE[n] != 0 for n in GM.RING]
    assert sum(not A.friendly(G[n][0]) for n in GM.SCHNORR + GM.RING) == 5     # five general, five friendly


@pytest.mark.parametrize("name", GM.RING)
def test_ring_moduli_are_composite(name):
    """a * a^(p-2) != 1 for 17 random units: p - 2 inverts nothing there"""
    p = GM.groups()[name][0]
    rng = random.Random("fermat-" + name)
    for _ in range(17):
        a = A._unit(rng, p)
        assert a * pow(a, p - 2, p) % p != 1


@pytest.mark.parametrize("name", GM.SCHNORR + GM.RING)
def test_prod_pow_matrix(name):
    p, q, _ = GM.groups()[name]
    m = GM.pp_matrix(name)
    assert len(m.B) == GM.ROWS and all(len(row) == GM.TERMS for row in m.B)
    assert all(0 <= b < GM.TOP for row in m.B for b in row)
    assert m.exps[:6] == [0, 1, 2, q - 1, q, 2**256 - 1] and m.exps[6].bit_length() > 200
    flat = [b for row in m.B for b in row]
    assert {0, p, GM.TOP - 1} <= set(flat) and (p + 1 in flat) == (p + 1 < GM.TOP)
    if name in A.ZERO_DIVISORS:
        u, v = A.ZERO_DIVISORS[name]
        # u^(q-1) v^q = 0 and u v^2 = 0; on `ones` no factor alone is 0 (gen_square's u is nilpotent)
        assert m.pw[2][3] * m.pw[2][4] % p == 0 and (name != "ones" or (m.pw[2][3] and m.pw[2][4]))
        assert m.pw[3][1] == u and (name != "ones" or m.pw[3][2]) and GM.pp_expected(m, 4, range(7))[2:] == [0, 0]
    if name in GM.RING:
        assert len(set(flat) & set(A.directed_bases(name))) >= 40 or name == "min_top"
    assert GM.pp_expected(m, 2, [0]) == [1, 1]              # x^0 = 1, for 0 too


@pytest.mark.parametrize("name", GM.RING)
def test_bucket_case_ring(name):
    """64 terms, none 0 or nilpotent, the other non-units kept, every expected product non-zero; the shortcut
    (prod b_i)^e of the equal-exponent sets equals the term-wise product; the zeroed terms give 0."""
    p = GM.groups()[name][0]
    c = GM.bucket_case_ring(name)
    assert len(c.bases) == 64 and all(b % p for b in c.bases)
    kept = [b for b in A.directed_bases(name) if b * b % p]
    assert c.bases == [kept[i % len(kept)] for i in range(64)] and len(kept) >= 30
    assert any(math.gcd(b, p) != 1 for b in c.bases)
    assert set(c.want) == set(c.sets) == {"all equal", "one digit each", "top digit"}
    assert all(len(e) == 64 for e in c.sets.values()) and all(c.want.values())
    for label in ("all equal", "top digit"):
        acc = 1
        for b, e in list(zip(c.bases, c.sets[label]))[:5]:
            acc = acc * pow(b, e, p) % p
        rest = 1
        for b in c.bases[5:]:
            rest = rest * b % p
        assert acc * pow(rest, c.sets[label][0], p) % p == c.want[label] != 0
    assert all(bin(e).count("1") <= 4 and 0 < e < 1 << 256 for e in c.sets["one digit each"])
    assert c.zeroed[21] == 0 and c.zeroed[40] == p and sum(x != y for x, y in zip(c.zeroed, c.bases)) == 2
    assert all(GM._bucket_product(p, c.zeroed, e) == 0 for e in c.sets.values())


INV_RING_CASES = [(name, n) for name in GM.RING for n in (17, 65)] + [("ones", 16), ("gen_square", 16)]


@pytest.mark.parametrize("name,n", INV_RING_CASES, ids=["%s-%d" % c for c in INV_RING_CASES])
def test_closed_form_of_the_inverse_equals_the_mirror(name, n):
    """17: one level of segments of 4; 65: one level of segments of 8 with a last segment of one;
    16: no level, where the closed form is a_i^(p-2) itself."""
    p = GM.groups()[name][0]
    els, want = GM.inverse_case_ring(name, n)
    assert len(els) == n and els[2] == 0 and els[n - 1] == p and want[2] == want[n - 1] == 0
    cnt = D.Count()
    assert D.batch_inverse(p, list(els), cnt) == list(want)
    seg, levels, jobs = D.inv_plan(n)
    assert (cnt.levels, cnt.pow_jobs) == (levels, jobs) and levels == (0 if n == 16 else 1)
    # no inverse: some element times its result is not 1
    assert any(a * w % p != 1 for a, w in zip(els, want) if a % p)


def test_closed_form_at_two_levels_and_on_a_prime():
    """257 elements (two levels, blocks of 64) on the toy prime: the closed form is the inverse, and
    on a composite 64-bit modulus it is the mirror's output."""
    p, q, g = D.toy_group()
    rng = random.Random(257)
    a = [rng.randrange(1, p) for _ in range(257)]
    a[0] = a[100] = 0
    assert D.inv_plan(257)[:2] == (16, 2)
    want = GM.inverse_closed_form(p, a)
    assert want == D.batch_inverse(p, a) == [pow(v, -1, p) if v else 0 for v in a]
    n = (2**32 - 1) * (2**32 + 15)
    b = [A._unit(rng, n) for _ in range(257)]
    b[7] = 0
    assert GM.inverse_closed_form(n, b) == D.batch_inverse(n, b) != [pow(v, -1, n) if v else 0 for v in b]


@pytest.mark.parametrize("name", GM.GENERAL)
def test_schnorr_inverse_cases(name):
    p = GM.groups()[name][0]
    for n in GM.INV_SIZES_SCHNORR:
        els, want = GM.inverse_case_schnorr(name, n)
        assert len(els) == n and all((a % p) * w % p == (1 if a % p else 0) for a, w in zip(els, want))
    els, want = GM.inverse_case_schnorr(name, 1, placed=False)
    assert els[0] % p > 1 and els[0] * want[0] % p == 1 and GM.inverse_case_schnorr(name, 1)[0] == [p]
    assert [D.inv_plan(n)[1] for n in GM.INV_SIZES_SCHNORR] == [0, 0, 1, 1, 2]
    els, _ = GM.inverse_case_schnorr(name, 65)
    assert all(els[i] == 0 for i in range(32, 48)) and els[64] == p and els[6] == GM.TOP - 1


@pytest.mark.parametrize("name", GM.GENERAL)
def test_count_texts(name):
    p, q, g = GM.groups()[name]
    for mc in GM.MAX_COUNTS:
        ys, want = GM.count_texts(name, mc)
        assert len(ys) == len(want) and want[-4:] == (-1,) * 4 and mc in want
        for fp in GM.FP_BITS:
            assert D.Table(p, g, mc, fp).counts(ys) == list(want), (mc, fp)


def test_degenerate_table():
    p = GM.DEG_P
    for fp in GM.FP_BITS:
        tab = D.Table(p, 2, 4000, fp)
        assert tab.m == 64
        assert [tab.count(1 << t) for t in (0, 1, 63, 64, 65, 4000)] == [0, 1, 63, 64, 65, 4000]
        assert tab.count(1 << 4001) == -1 and tab.count(3) == -1
        ys, want = GM.degenerate_texts()
        assert tab.counts(ys) == want
    # what the inversion of up to 16 elements gives for 2^k, and when that is the inverse
    for k in GM.DEG_K_INVERTIBLE + GM.DEG_K_OTHER:
        assert pow(1 << k, p - 2, p) == GM.degenerate_m_inverse(k)
        assert (GM.degenerate_m_inverse(k) << k) % p == (1 if k in GM.DEG_K_INVERTIBLE else 1 << (-2 * k % 4096))
    B, M, want = GM.degenerate_with_m(GM.DEG_K_INVERTIBLE)
    assert want == GM.degenerate_texts()[1] and B[2] == 1 << (63 + 2048) and B[6] == 1 << (4000 + 2048 - 4096)
    B, M, want = GM.degenerate_with_m(GM.DEG_K_OTHER)
    # t - 2 k mod 4096 where that is at most 4000
    ks = [GM.DEG_K_OTHER[i % 4] for i in range(7)]
    shifted = [(t - 2 * k) % 4096 for t, k in zip(GM.DEG_EXPONENTS, ks)]
    assert want == [e if e <= 4000 else -1 for e in shifted] + [-1] * 4
    assert want[:7] == [-1, -1, 65, 66, 63, 2037, -1]
    assert D.Table(p, 2, 4000, 0).counts(B[:4], M[:4]) == want[:4]    # the mirror's own route
    # 17 single-bit elements: one level of segments of 4, every result a single bit
    els = [1 << (241 * i % 4096) for i in range(17)]
    inv = GM.inverse_closed_form(p, els)
    assert D.inv_plan(17) == (4, 1, 5) and inv == D.batch_inverse(p, els)
    assert all(bin(v).count("1") == 1 for v in inv)
