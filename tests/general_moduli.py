"""Contexts and CPython references for prod_pow, the device-side decode and the shuffle on moduli other
than the production prime.

Shared by tests/test_general_moduli.py (CPU: keeps these fixtures honest) and
tests/test_gpu_general_moduli.py (GPU: every LAUNCH_F kernel of eg_prodpow.hpp, eg_decode.hpp and
eg_shuffle.hpp on both Montgomery instantiations).  Everything is computed in code or read from
tests/golden/test_groups.json and tests/adversarial_moduli.py; nothing is written to disk.

Three sets of moduli (eg_ctx_create asks only for an odd p with the top bit set and nothing of q):

  SCHNORR     sparse_c and dense_c of test_groups.json (general: n0 != 1, the Mont<false> kernels) and
              Mode4096_V2 (friendly: a second prime for the Mont<true> kernels).  g has order q.
  RING        the seven moduli of adversarial_moduli.moduli() with g = 3 and the production q.  None is
              prime: only ring operations mean anything on them, and a^(p-2) is no inverse there.
  DEGENERATE  p = 2^4096 - 1, g = 2, q = 4096: 2 has order 4096, every power of g is a single bit, and
              so is every Montgomery form (R = 2^4118 = 2^22 mod p): a giant step is a rotation.

The `contexts` fixture is module-scoped: one GroupContext(p, q, g) per modulus, opened at first use,
closed at teardown, at most ten open at a time.  A test module imports it and takes the moduli's names
as parameters.
"""
import json
import math
import random
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import pytest

import adversarial_moduli as A
import decode_ref as D

TOP = A.TOP
GENERAL = ("sparse_c", "dense_c")
SCHNORR = GENERAL + ("Mode4096_V2",)
RING = A.NAMES
DEGENERATE = "degenerate"
DEG_P, DEG_Q, DEG_G, DEG_MAX_COUNT = TOP - 1, 4096, 2, 4000
ROWS, TERMS = 9, 7


@lru_cache(maxsize=None)
def groups() -> dict:
    """name -> (p, q, g) of every modulus of the three sets"""
    import eg_oracle as O
    out = {}
    doc = json.loads((Path(__file__).resolve().parent / "golden" / "test_groups.json").read_text())
    for d in doc["groups"]:
        out[d["name"]] = (int(d["p"], 16), int(d["q"], 16), int(d["g"], 16))
    v2 = O.production_group(O.MODE4096_V2)
    out["Mode4096_V2"] = (v2.p, v2.q, v2.g)
    for name, p in A.moduli().items():
        out[name] = (p, A.production_q(), A.G)
    out[DEGENERATE] = (DEG_P, DEG_Q, DEG_G)
    assert set(GENERAL) <= set(out)
    return out


MAX_OPEN = 10


@pytest.fixture(scope="module")
def contexts():
    """contexts(name) -> SimpleNamespace(name, p, q, g, G = the GroupContext): one GroupContext(p, q, g)
    per modulus for the whole module, opened at its first use and closed at teardown.  At most ten are
    open: the eleventh closes the one used longest ago."""
    from electionguard.core import GroupContext
    held = {}

    def get(name):
        if name in held:
            held[name] = held.pop(name)                  # most recently used last
            return held[name]
        if len(held) == MAX_OPEN:
            held.pop(next(iter(held))).G.close()
        p, q, g = groups()[name]
        held[name] = SimpleNamespace(name=name, p=p, q=q, g=g, G=GroupContext(p, q, g))
        return held[name]

    try:
        yield get
    finally:
        for c in held.values():
            c.G.close()


# ---------------------------------------------------------------------------------------------------
# prod_pow
# ---------------------------------------------------------------------------------------------------
def pp_exponents(name):
    """0, 1, 2, q - 1, q, 2^256 - 1 and a random 256-bit value: one per term"""
    q = groups()[name][1]
    return [0, 1, 2, q - 1, q, (1 << 256) - 1, random.Random("pp-exp-" + name).getrandbits(256)]


@lru_cache(maxsize=None)
def pp_matrix(name):
    """9 rows x 7 terms with every power B[r, i]^{e_i} by CPython once (63 pows).

    A Schnorr group takes random bases with the edge bases 0, 1, p - 1, p, p + 1, 2^4096 - 1 in rows 1
    and 2 and sprinkled over the others.  A ring modulus takes adversarial_moduli.directed_bases (the
    saturated and sparse Montgomery operands) in order, row 1 from 0, p, p + 1 (where it fits 512
    bytes) and 2^4096 - 1, and, where the modulus has zero divisors u v = 0, u and v at the terms of
    q - 1 and q in row 2 (the two exponents share every digit but the lowest, so u v = 0 arises inside
    a bucket) and at the terms of 1 and 2 in row 3 (different buckets: the product becomes 0 in the
    Horner chain)."""
    p, q, _ = groups()[name]
    rng = random.Random("pp-" + name)
    exps = pp_exponents(name)
    if name in RING:
        pool = A.directed_bases(name)
        B = [[pool[(r * TERMS + i) % len(pool)] for i in range(TERMS)] for r in range(ROWS)]
        edges = [v for v in (0, p, p + 1, TOP - 1) if v < TOP]
        B[1][:len(edges)] = edges
        if name in A.ZERO_DIVISORS:
            u, v = A.ZERO_DIVISORS[name]
            B[2][3], B[2][4] = u, v
            B[3][1], B[3][2] = u, v
            B[1][len(edges)] = u * A._unit(rng, p) % p
    else:
        edges = [0, 1, p - 1, p, p + 1, TOP - 1]
        B = [[rng.randrange(p) for _ in range(TERMS)] for _ in range(ROWS)]
        B[1] = edges + [rng.randrange(p)]
        B[2] = edges[3:] + edges[:3] + [rng.randrange(p)]
        for r in range(3, ROWS):
            for i in range(TERMS):
                if rng.random() < 0.4:
                    B[r][i] = rng.choice(edges[1:])
    pw = [[pow(b % p, e, p) for b, e in zip(row, exps)] for row in B]
    return SimpleNamespace(p=p, B=B, exps=exps, pw=pw)


def pp_expected(m, rows, cols):
    """prod over the term indices `cols` of the first `rows` rows"""
    out = []
    for r in range(rows):
        acc = 1
        for i in cols:
            acc = acc * m.pw[r][i] % m.p
        out.append(acc)
    return out


def bucket_exponents(name, n):
    """the sets "all equal", "one digit each" and "top digit" of test_bucket_structure_at_c4_n64"""
    q = groups()[name][1]
    rng = random.Random("bucket-" + name)
    same = rng.randrange(q)
    return {
        "all equal": [same] * n,                                      # one bucket per window holds everything
        "one digit each": [rng.randrange(1, 16) << (4 * rng.randrange(64)) for _ in range(n)],
        "top digit": [15 << 252] * n,
    }


def _bucket_product(p, bases, exps):
    """prod b_i^{e_i}: one CPython pow per term, or, where every exponent is one value e, (prod b_i)^e,
    the same element of a commutative ring"""
    acc = 1
    if len(set(exps)) == 1:
        for b in bases:
            acc = acc * b % p
        return pow(acc, exps[0], p)
    for b, e in zip(bases, exps):
        acc = acc * pow(b, e, p) % p
    return acc


@lru_cache(maxsize=None)
def bucket_case_ring(name):
    """64 terms: the directed bases whose square is not 0 mod p (that drops 0 and, on gen_square, the
    multiples of the nilpotent 2^2048 - 1; the other non-units stay), cycled where a modulus has fewer
    than 64 of them, with the expected product per exponent set.  Every expected product is non-zero,
    so a wrong bucket, window or Horner step shows.  `zeroed` is the separate zero-absorbing
    case: the same terms with 0 at term 21 and p at term 40, expected 0 for every set."""
    p = groups()[name][0]
    pool = [b for b in A.directed_bases(name) if b * b % p]
    bases = [pool[i % len(pool)] for i in range(64)]
    sets = bucket_exponents(name, 64)
    want = {label: _bucket_product(p, bases, exps) for label, exps in sets.items()}
    assert all(want.values()), name
    zeroed = list(bases)
    zeroed[21], zeroed[40] = 0, p
    return SimpleNamespace(bases=bases, sets=sets, want=want, zeroed=zeroed)


@lru_cache(maxsize=None)
def bucket_case_schnorr(name):
    """64 secret logarithms x_i (the bases g^{x_i} come from the context's own gPowP_batch) and, per
    exponent set, g^(sum x_i e_i) for the terms in order and in reverse order: one pow per row."""
    p, q, g = groups()[name]
    rng = random.Random("bucket-x-" + name)
    x = [rng.randrange(q) for _ in range(64)]
    sets = bucket_exponents(name, 64)
    want = {label: [pow(g, sum(a * e for a, e in zip(xs, exps)) % q, p) for xs in (x, x[::-1])]
            for label, exps in sets.items()}
    return SimpleNamespace(x=x, sets=sets, want=want)


# ---------------------------------------------------------------------------------------------------
# batch_inverse
# ---------------------------------------------------------------------------------------------------
INV_SIZES_SCHNORR = (1, 16, 17, 65, 257)     # no level (1 and the limit), one level, a ragged last segment, two levels
INV_SIZES_RING = (16, 17, 65)


@lru_cache(maxsize=None)
def inverse_pool(name):
    """257 elements of a Schnorr group, every eighth of the subgroup and the others random in [1, p),
    with their inverses by CPython and the inverses of the special values"""
    p, q, g = groups()[name]
    rng = random.Random("inv-pool-" + name)
    vals = [pow(g, rng.randrange(q), p) if i % 8 == 0 else rng.randrange(1, p) for i in range(257)]
    inv = [pow(v, -1, p) for v in vals]
    special = {0: 0, 1: 1, p - 1: p - 1, p: 0, p + 1: 1, TOP - 1: pow((TOP - 1) % p, -1, p)}
    return SimpleNamespace(p=p, vals=vals, inv=inv, special=special)


def inverse_placements(p, n):
    """test_gpu_decode.placements: zeros first, last and mid-segment, one all-zero segment where
    there is room for one, and 1, p - 1 and the values >= p"""
    placed = {0: 0, n - 1: p}
    if n > 6:
        placed.update({5: 0, 2: 1, 3: p - 1, 4: p + 1, 6: TOP - 1})
    if n >= 64:
        placed.update({i: 0 for i in range(32, 48)})
        placed.update({31: p - 1, 48: 1})
    return placed


def inverse_case_schnorr(name, n, placed=True):
    """-> (elements, wanted inverses) as ints.  placed=False leaves the pool's elements as they are:
    at n = 1 the placements are p alone, and this is the one-element batch that inverts something."""
    pool = inverse_pool(name)
    els, want = pool.vals[:n], pool.inv[:n]
    if placed:
        for i, v in inverse_placements(pool.p, n).items():
            els[i], want[i] = v, pool.special[v]
    return els, want


def inverse_closed_form(p, a):
    """What the segmented inversion defines on ANY odd modulus, for units and zeros: every total left
    at the top level takes t^(p-2), so with t the product of the non-zero elements of the top-level
    block that holds i (seg_len^levels elements, decode_ref.inv_plan), out[i] = a_i^-1 t^(p-1), and
    0 for a zero.  On a prime t^(p-1) = 1."""
    n = len(a)
    seg, levels, _ = D.inv_plan(n)
    block = seg ** levels
    out = []
    for b0 in range(0, n, block):
        part = [v % p for v in a[b0:b0 + block]]
        t = 1
        for v in part:
            if v:
                t = t * v % p
        f = pow(t, p - 1, p)
        out += [pow(v, -1, p) * f % p if v else 0 for v in part]
    return out


@lru_cache(maxsize=None)
def inverse_case_ring(name, n):
    """-> (elements, closed form): units of adversarial_moduli.directed_bases cycled, alternating
    with random units, 0 at index 2 and p at index n - 1.  Zero divisors are left out: the closed
    form needs a_i^-1."""
    p = groups()[name][0]
    rng = random.Random("inv-ring-%s-%d" % (name, n))
    units = [b for b in A.directed_bases(name) if math.gcd(b, p) == 1]
    els = [units[(i // 2) % len(units)] if i % 2 == 0 else A._unit(rng, p) for i in range(n)]
    els[2], els[n - 1] = 0, p
    assert all(math.gcd(v, p) == 1 for v in els if v % p)
    return tuple(els), tuple(inverse_closed_form(p, els))


# ---------------------------------------------------------------------------------------------------
# dLog counts
# ---------------------------------------------------------------------------------------------------
MAX_COUNTS = (0, 3, 100, 10_000)
FP_BITS = (0, 8)


@lru_cache(maxsize=None)
def count_texts(name, max_count):
    """(texts, wanted counts): g^t for t in {0, 1, m - 1, m, m + 1, max_count} (those <= max_count),
    then the non-exponents g^(max_count + 1), g^(q - 1), 0 and p - 1"""
    p, q, g = groups()[name]
    m = math.isqrt(max_count) + 1
    ts = [t for t in (0, 1, m - 1, m, m + 1, max_count) if t <= max_count]
    ys = [pow(g, t, p) for t in ts] + [pow(g, max_count + 1, p), pow(g, q - 1, p), 0, p - 1]
    return tuple(ys), tuple(ts + [-1] * 4)


DEG_EXPONENTS = (0, 1, 63, 64, 65, 2047, 4000)


def degenerate_texts():
    """(texts, wanted counts) of the degenerate group: 2^t -> t, and 2^4001, 3, 0 and p -> -1"""
    ys = [1 << t for t in DEG_EXPONENTS] + [1 << 4001, 3, 0, DEG_P]
    return ys, list(DEG_EXPONENTS) + [-1] * 4


# the M rows of the degenerate group are 2^k.  Its p is no prime, so M^(p-2) = 2^(-3k) is the inverse
# of 2^k only for 2 k = 0 mod 4096: k = 0 and 2048 decode B = 2^(t+k) to t.  Any other k decodes it
# to what the mirror computes from 2^(t + k - 3 k).
DEG_K_INVERTIBLE = (2048, 0)
DEG_K_OTHER = (1, 5, 2047, 4095)


def degenerate_m_inverse(k):
    """(2^k)^(p-2) mod 2^4096 - 1, what an inversion of at most 16 elements gives for 2^k: p - 2 = -3
    mod 4096, the order of 2 (the CPU test checks it against CPython's pow)"""
    return 1 << (-3 * k % 4096)


def degenerate_with_m(ks):
    """-> (B, M, wanted) for the eleven texts with M[i] = 2^k, k cycling through ks, and
    B[i] = y_i 2^k (2^(t + k mod 4096) for y_i = 2^t); the wanted count is decode_ref's for
    B[i] M[i]^(p-2)"""
    ys, _ = degenerate_texts()
    ks = [ks[i % len(ks)] for i in range(len(ys))]
    M = [1 << k for k in ks]
    B = [y * v % DEG_P for y, v in zip(ys, M)]
    B[-1] = DEG_P                                                   # 0 as p
    tab = D.Table(DEG_P, DEG_G, DEG_MAX_COUNT, 8)
    return B, M, [tab.count(b * degenerate_m_inverse(k) % DEG_P) for b, k in zip(B, ks)]
