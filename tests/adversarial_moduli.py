"""Adversarial moduli, directed operands and layout routes for the Montgomery kernels.

Shared by tests/test_adversarial_moduli.py (CPU: keeps these fixtures honest) and
tests/test_gpu_adversarial_moduli.py (GPU: every kernel instantiation against CPython).  Everything here
is deterministic and computed in code; nothing is read from or written to disk.

eg_ctx_create takes any odd modulus with the top bit set, so the public group API reaches instantiations
the production p (= -1 mod 2^256, random middle limbs) never selects:

  * the per-wave kernel (eg_pow16.hip, egw) picks mode 0 for a general modulus, mode 1 for p = -1 mod
    2^29 and mode 2 (the delayed-quotient multiply mul_d2) for p = -1 mod 2^58;
  * the 8-lane and 16-lane kernels pick their FRIENDLY instantiation for n0 = -p^-1 mod 2^29 == 1.

The Montgomery domain is R = 2^(29 * 142) = 2^4118 (eg_bignum.hpp kSteps): after the import
(x * R^2 * R^-1) the kernel holds x * R mod p or that plus p, so mont_preimage(v, p) = v * R^-1 mod p is
the public input whose Montgomery-domain operand is v (or v + p).
"""
import math
import random
from functools import lru_cache

B = 29                     # limb bits
MASK = (1 << B) - 1
N_LIMBS = 144              # limbs of an element (8 x 18 = 16 x 9 = 48 x 3)
STEPS = 142                # CIOS steps of one Montgomery operation
R = 1 << (B * STEPS)       # 2^4118
TOP = 1 << 4096
G = 3


def production_q() -> int:
    import eg_oracle as O
    return O.production_group().q


def _f58_only() -> int:
    """random, exactly 58 low one-bits (bit 58 clear), limb 2 of p + 1 non-zero, top bit set: the
    construction of tests/test_delayed_quotient.py with a fixed seed"""
    rng = random.Random(5858)
    while True:
        p = (rng.getrandbits(4096 - 59) << 59) | ((1 << 58) - 1) | (1 << 4095)
        if (p >> 58) & 1 == 0 and limbs(p + 1)[2] != 0:
            return p


def _f29_only() -> int:
    """random, exactly 29 low one-bits (bit 29 clear), top bit set"""
    rng = random.Random(2929)
    return (rng.getrandbits(4096 - 30) << 30) | MASK | (1 << 4095)


def limbs(v: int, n: int = N_LIMBS):
    return [(v >> (B * i)) & MASK for i in range(n)]


@lru_cache(maxsize=None)
def moduli() -> dict:
    """name -> p, in the order of the table in the module docstring of the GPU test"""
    return {
        "ones": TOP - 1,
        "f58_dense": TOP - (1 << 58) - 1,
        "f58_only": _f58_only(),
        "f29_only": _f29_only(),
        "gen_dense": TOP - 3,
        "gen_square": ((1 << 2048) - 1) ** 2,
        "min_top": (1 << 4095) + 1,
    }


NAMES = ("ones", "f58_dense", "f58_only", "f29_only", "gen_dense", "gen_square", "min_top")
# what the per-wave kernel must select (powwave_jobs) and whether limb 2 of p + 1 is non-zero
EXPECTED_MODE = {"ones": 2, "f58_dense": 2, "f58_only": 2, "f29_only": 1, "gen_dense": 0, "gen_square": 0,
                 "min_top": 0}
PT2_NONZERO = {"ones": False, "f58_dense": True, "f58_only": True}
# non-trivial factorisations p = u * v of the composite fixtures (u * v = 0 mod p)
ZERO_DIVISORS = {
    "ones": ((1 << 2048) - 1, (1 << 2048) + 1),
    "gen_square": ((1 << 2048) - 1, (1 << 2048) - 1),
}


# ---- the predicates the library evaluates on a modulus ----
def n0(p: int) -> int:
    """-p^-1 mod 2^29 (eg_ctx_create)"""
    return (-pow(p, -1, 1 << B)) & MASK


def friendly(p: int) -> bool:
    return n0(p) == 1


def d2_predicate(p: int) -> bool:
    """powwave_consts_create: p[0] == 0xFFFFFFFF && (p[1] & 0x03FFFFFF) == 0x03FFFFFF on 32-bit words"""
    w0, w1 = p & 0xFFFFFFFF, (p >> 32) & 0xFFFFFFFF
    return w0 == 0xFFFFFFFF and (w1 & 0x03FFFFFF) == 0x03FFFFFF


def wave_mode(p: int, d2_enabled: bool = True) -> int:
    """powwave_jobs: (friendly && d2) ? 2 : friendly ? 1 : 0"""
    if friendly(p) and d2_predicate(p) and d2_enabled:
        return 2
    return 1 if friendly(p) else 0


def pt2(p: int) -> int:
    """limb 2 of p~ = p + 1: the first delayed term of mul_d2"""
    return ((p + 1) >> (2 * B)) & MASK


# ---- directed operands ----
def mont_preimage(v: int, p: int) -> int:
    """the input x < p with x * R = v mod p"""
    return v * pow(R, -1, p) % p


_ZEROED = (0, 1, 2, 3, 8, 9, 17, 18, 19, 26, 27, 35, 36, 53, 54, 71, 72, 89, 90, 107, 125, 126, 140, 141)


@lru_cache(maxsize=None)
def directed_values(name: str) -> tuple:
    """About 64 Montgomery-domain values v (reduced mod p, distinct, a fixed order) with saturated or
    sparse limbs."""
    p = moduli()[name]
    vs = [p - 1 - k for k in range(16)]
    vs += [p & ~(MASK << (B * i)) for i in _ZEROED]                        # p with one limb zeroed
    vs.append(TOP - 1)                                                    # every limb 2^29 - 1 up to bit 4095
    vs.append(sum(MASK << (B * i) for i in range(0, N_LIMBS, 2)) % TOP)   # alternating max / zero limbs
    vs.append(sum(MASK << (B * i) for i in range(1, N_LIMBS, 2)) % TOP)
    vs += [1, R % p, (R - 1) % p, 2, p >> 1, 1 << 4095, (1 << 4095) - 1]
    vs += [(1 << (B * 18 * j)) - 1 for j in range(1, 8)]                   # ones up to an 8-lane boundary
    vs += [p - (1 << (B * 18 * j)) for j in range(1, 8)]
    out, seen = [], set()
    for v in vs:
        v %= p
        if v not in seen:
            seen.add(v)
            out.append(v)
    return tuple(out)


@lru_cache(maxsize=None)
def directed_bases(name: str) -> tuple:
    """the public inputs whose Montgomery-domain operands are directed_values(name)"""
    p = moduli()[name]
    return tuple(mont_preimage(v, p) for v in directed_values(name))


def lane_boundaries():
    """bit positions that are lane boundaries of a layout: multiples of 29 * 3 (per-wave), which
    include those of 29 * 9 (16-lane) and 29 * 18 (8-lane)"""
    return list(range(B * 3, 4096, B * 3))


@lru_cache(maxsize=None)
def result_targets(name: str) -> tuple:
    p = moduli()[name]
    ts = [1, p - 1, 1 << 4095]
    for k in lane_boundaries():
        ts += [1 << k, (1 << k) - 1]
    return tuple(t % p for t in ts)


def _unit(rng, p):
    while True:
        a = rng.randrange(2, p)
        if math.gcd(a, p) == 1:
            return a


@lru_cache(maxsize=None)
def result_pairs(name: str) -> tuple:
    """(a, b, t) with a * b = t mod p: a a random unit, b = t * a^-1; then products that are 0
    through the modulus's zero divisors"""
    p = moduli()[name]
    rng = random.Random("pairs-" + name)
    out = []
    for t in result_targets(name):
        a = _unit(rng, p)
        out.append((a, t * pow(a, -1, p) % p, t))
    if name in ZERO_DIVISORS:
        u, v = ZERO_DIVISORS[name]
        out.append((u, v, 0))
        for _ in range(6):
            out.append((u * _unit(rng, p) % p, v * _unit(rng, p) % p, 0))
    return tuple(out)


@lru_cache(maxsize=None)
def product_chain(name: str, length: int) -> tuple:
    """(elements, running products): `length` elements whose running product passes through the
    invertible result targets in turn (x_1 = t_1, x_k = t_k * t_(k-1)^-1)"""
    p = moduli()[name]
    ts = [t for t in result_targets(name) if math.gcd(t, p) == 1 and t != 1]
    rng = random.Random("chain-%s-%d" % (name, length))
    ts = rng.sample(ts, length)
    xs, prev = [], 1
    for t in ts:
        xs.append(t * pow(prev, -1, p) % p)
        prev = t
    return tuple(xs), tuple(ts)


def import_edges(name: str):
    """unreduced inputs that fit the 512-byte element: p, p + 1, 2^4096 - 1, 2p - 1"""
    p = moduli()[name]
    out = []
    for v in (p, p + 1, TOP - 1, 2 * p - 1):
        if v < TOP and v not in out:
            out.append(v)
    return out


# ---- layout routes ----
# Every knob a route may set; cleared before a route's own values are applied.  eg_ctx_create and
# powwave_consts_create read them when the context is made.
KNOBS = ("EG_LATENCY_POW", "EG_WAVE_R2L", "EG_POWWAVE_D2", "EG_WAVE_W8", "EG_WAVE_MAX", "EG_WAVE_SPLIT",
         "EG_COALESCE_ZC")

# variable-base routes of a batch of n <= compute units elements: (name, env, mode-2 moduli only)
POW_ROUTES = (
    ("lanes8", {"EG_LATENCY_POW": "0"}, False),                  # k_pow, 8 lanes x 18 limbs
    ("lanes16", {"EG_LATENCY_POW": "16"}, False),                # eg16::k_pow, 16 lanes x 9 limbs
    ("wave4_r2l", {}, False),                                    # 4 waves per job, right to left
    ("wave1", {"EG_WAVE_R2L": "0"}, False),                      # one wave per element, sliding window
    ("wave4_r2l_cios", {"EG_POWWAVE_D2": "0"}, True),            # mode 1 on a mode-2 modulus
    ("wave1_cios", {"EG_POWWAVE_D2": "0", "EG_WAVE_R2L": "0"}, True),
)
# fixed-base routes.  Batches: up to one element per SIMD on the per-wave kernel (4 waves per job),
# larger ones on the 8-lane k_pow.  Per-element calls (the coalescer): 8 waves per job on a mode-2
# modulus up to EG_WAVE_W8 jobs (default: one per compute unit), else 4.
FB_ROUTES = (
    ("wave", {}, False),
    ("wave_w8_off", {"EG_WAVE_W8": "0"}, True),
    ("lanes8", {"EG_LATENCY_POW": "0"}, False),
)


def routes_for(name: str, routes=POW_ROUTES):
    p = moduli()[name]
    return [(r, env) for r, env, d2_only in routes if not d2_only or wave_mode(p) == 2]


def is_latency_route(route: str) -> bool:
    """routes whose variable-base batches bypass the 8-lane k_pow (nothing for the profile to count)"""
    return route != "lanes8"


def cases(routes=POW_ROUTES):
    """(modulus name, route name) for every modulus and every route valid for it"""
    return [(name, r) for name in NAMES for r, _ in routes_for(name, routes)]


def open_group(monkeypatch, name: str, route: str, routes=POW_ROUTES):
    """A GroupContext over modulus `name` with the route's knobs in the environment (set before the
    context is made).  The caller closes it in a finally block."""
    from electionguard.core import GroupContext
    env = dict(routes_for(name, routes))[route]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return GroupContext(moduli()[name], production_q(), G)
