"""The device-side decode restated on CPython ints (include/eg_hip_decode.h), without
the package: the plan's formula, the segmented batch inverse with its multiply count, and baby-step
giant-step over an open-addressing table keyed by fingerprints, where a hit counts only after the
whole element is compared.  Any Schnorr group will do: the tests run it on a 64-bit toy group."""
import math

STOP = 16          # EG_DECODE_STOP: at most this many totals take a^(p-2)
POW_OPS = 5129     # Montgomery multiplies of one a^(p-2) on the 4-bit window
MAX_TEXTS, MAX_COUNT = 1 << 24, 1 << 32
EMPTY = 0xFFFFFFFF


# ---- the plan ----
def seg_len(n: int) -> int:
    """S = min(16, max(4, the least power of two >= ceil(n / 16)))"""
    s = 4
    while s * STOP < n and s < 16:
        s *= 2
    return s


def inv_plan(n: int):
    """-> (S, levels, jobs): n_0 = n; while n_l > STOP: n_(l+1) = ceil(n_l / S)."""
    s, levels, left = seg_len(n), 0, n
    while left > STOP:
        left = -(-left // s)
        levels += 1
    return s, levels, left


def plan(n: int, max_count: int = 0):
    """The tuple electionguard.decode.plan gives: (seg_len, levels, pow_jobs, m, slots, load, inv_ops, mont_ops)."""
    s, levels, jobs = inv_plan(n)
    m = math.isqrt(max_count) + 1
    slots = 16
    while slots < 2 * m:
        slots *= 2
    inv = 3.0 * (n - jobs) + POW_OPS * jobs
    return s, levels, jobs, m, slots, m / slots, inv, inv + n + n * m


# ---- the segmented inverse ----
class Count:
    """Multiplies made and a^(p-2) jobs run by one batch_inverse."""

    def __init__(self):
        self.mul = self.pow_jobs = self.levels = 0


def batch_inverse(p: int, a, count: Count = None, seg: int = None):
    """a[i]^-1 mod p with 0 -> 0, by the sweeps the kernels make.  A zero enters as 1 and leaves as 0."""
    count = count or Count()
    n = len(a)
    s = seg or seg_len(n)
    x = [int(v) % p for v in a]
    zero = [v == 0 for v in x]
    x = [1 if z else v for v, z in zip(x, zero)]
    if n > STOP:
        x = _invert(p, x, s, count)
    else:
        count.pow_jobs += n
        x = [pow(v, p - 2, p) for v in x]
    return [0 if z else v for v, z in zip(x, zero)]


def _invert(p, x, s, count):
    n = len(x)
    if n <= STOP:
        count.pow_jobs += n
        return [pow(v, p - 2, p) for v in x]
    count.levels += 1
    starts = range(0, n, s)
    prefix, totals = list(x), []
    for st in starts:                       # forward: one group per segment
        for i in range(st + 1, min(n, st + s)):
            prefix[i] = prefix[i - 1] * x[i] % p
            count.mul += 1
        totals.append(prefix[min(n, st + s) - 1])
    tinv = _invert(p, totals, s, count)
    out = list(x)
    for k, st in enumerate(starts):         # backward, from the segment's end
        acc = tinv[k]
        for i in range(min(n, st + s) - 1, st, -1):
            out[i] = acc * prefix[i - 1] % p
            acc = acc * x[i] % p
            count.mul += 2
        out[st] = acc
    return out


# ---- baby-step giant-step with fingerprints ----
def fingerprint(x: int, fp_bits: int) -> int:
    """The top fp_bits of splitmix64's finalizer over the low 64 bits of the canonical residue x."""
    h = x & (2**64 - 1)
    h ^= h >> 30
    h = h * 0xBF58476D1CE4E5B9 % 2**64
    h ^= h >> 27
    h = h * 0x94D049BB133111EB % 2**64
    h ^= h >> 31
    return h >> (64 - fp_bits)


def home(fp: int, slots: int) -> int:
    return ((fp * 0x9E3779B97F4A7C15 % 2**64) >> 32) & (slots - 1)


class Table:
    """Baby steps g^0 .. g^(m-1), the step g^(-m), and the open-addressing table (j, fingerprint)."""

    def __init__(self, p: int, g: int, max_count: int, fp_bits: int = 0):
        self.p, self.max_count, self.fp_bits = p, max_count, fp_bits or 64
        _, _, _, self.m, self.slots, _, _, _ = plan(0, max_count)
        self.baby, x = [], 1 % p
        for _ in range(self.m):
            self.baby.append(x)
            x = x * g % p
        self.step = pow(g, -self.m, p)
        self.j = [EMPTY] * self.slots
        self.fp = [0] * self.slots
        self.compares = self.false_hits = 0
        for j, b in enumerate(self.baby):
            f = fingerprint(b, self.fp_bits)
            pos = home(f, self.slots)
            while self.j[pos] != EMPTY:
                pos = (pos + 1) & (self.slots - 1)
            self.j[pos], self.fp[pos] = j, f

    def count(self, y: int) -> int:
        """The t in [0, max_count] with g^t = y, else -1.  y is canonical at every step."""
        y %= self.p
        for i in range(self.m + 1):
            f = fingerprint(y, self.fp_bits)
            pos = home(f, self.slots)
            while self.j[pos] != EMPTY:
                if self.fp[pos] == f:
                    self.compares += 1
                    if self.baby[self.j[pos]] == y:      # the whole element, not the fingerprint
                        t = i * self.m + self.j[pos]
                        if t <= self.max_count:
                            return t
                        break                            # the only equal baby step: on to the next giant step
                    self.false_hits += 1
                pos = (pos + 1) & (self.slots - 1)
            y = y * self.step % self.p
        return -1

    def counts(self, B, M=None):
        ys = B if M is None else [b * v % self.p for b, v in zip(B, batch_inverse(self.p, M))]
        return [self.count(y) for y in ys]


# ---- a 64-bit toy Schnorr group ----
def is_prime(n: int) -> bool:
    if n < 2:
        return False
    for sp in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % sp == 0:
            return n == sp
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):     # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def toy_group():
    """(p, q, g): q the first prime above 2^31, p = k q + 1 the first such prime above 2^63, g of order q."""
    q = 2**31 + 1
    while not is_prime(q):
        q += 2
    k = (2**63) // q + 1
    while not is_prime(k * q + 1):
        k += 1
    p = k * q + 1
    h = 2
    while pow(h, k, p) == 1:
        h += 1
    return p, q, pow(h, k, p)
