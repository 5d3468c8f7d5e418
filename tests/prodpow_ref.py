"""A CPython restatement of the two multi-exponentiation schedules of include/eg_hip_prodpow.h,
for the tests: it imports nothing from the package, works modulo any odd p and COUNTS its
modular multiplies the way the header's cost model does (squarings included; the conversions and
the multiplies by one that pad a wave are the kernels' own and have no counterpart here, while
the multiplies the schedule runs whatever the exponents are, such as an empty bucket's place in a
bit product, are counted).

  interleaved(p, bases, exps, w)  ->  (prod_i bases[i]^exps[i] mod p, multiplies)
  buckets(p, bases, exps, c)      ->  the same by digit buckets
"""

INTER_TERMS = 1 << 12    # terms per chunk of the interleaved method
BUCKET_TERMS = 1 << 16   # ... of the bucket method


class Counter:
    def __init__(self, p):
        self.p, self.n = p, 0

    def mul(self, a, b):
        self.n += 1
        return a * b % self.p


def segment(m):
    """The bucket method's segment length for a chunk of m terms."""
    s = 16
    while s * s < m:
        s *= 2
    return s


def _chunks(bases, exps, size):
    for t0 in range(0, len(bases), size):
        yield bases[t0:t0 + size], exps[t0:t0 + size]


def _combine(M, parts):
    acc = parts[0]
    for x in parts[1:]:
        acc = M.mul(acc, x)
    return acc


def _interleaved_chunk(M, bases, exps, w):
    tw = (1 << w) - 1
    tabs = []
    for b in bases:                       # b^1 .. b^(2^w - 1): 2^w - 2 multiplies per base
        t = [b]
        for _ in range(2, tw + 1):
            t.append(M.mul(t[-1], b))
        tabs.append(t)
    rounds = -(-256 // w)
    acc = 1 % M.p
    for rd in reversed(range(rounds)):
        if rd != rounds - 1:
            for _ in range(w):
                acc = M.mul(acc, acc)
        for t, e in zip(tabs, exps):
            d = (e >> (rd * w)) & tw
            if d:
                acc = M.mul(acc, t[d - 1])
    return acc


def interleaved(p, bases, exps, w, terms=INTER_TERMS):
    M = Counter(p)
    bases = [b % p for b in bases]
    if not bases:
        return 1 % p, 0
    return _combine(M, [_interleaved_chunk(M, b, e, w) for b, e in _chunks(bases, exps, terms)]), M.n


def _bucket_chunk(M, bases, exps, c):
    one = 1 % M.p
    W = -(-256 // c)
    S = segment(len(bases))
    Q = []
    for w in range(W):
        members = [[] for _ in range(1 << c)]
        for i, e in enumerate(exps):
            members[(e >> (c * w)) & ((1 << c) - 1)].append(i)
        bk = [one] * (1 << c)
        for j in range(1, 1 << c):        # step 2: segments of S members, then the segments
            segs = []
            for s0 in range(0, len(members[j]), S):
                x = bases[members[j][s0]]
                for i in members[j][s0 + 1:s0 + S]:
                    x = M.mul(x, bases[i])
                segs.append(x)
            if segs:
                bk[j] = _combine(M, segs)
        for t in range(c):                # step 3: 2^(c-1) - 1 multiplies per bit, empty buckets being one
            js = [j for j in range(1, 1 << c) if (j >> t) & 1]
            Q.append(_combine(M, [bk[j] for j in js]))
    acc = Q[255]                          # step 4: bits past 255 are always one and are not read
    for k in reversed(range(255)):
        acc = M.mul(acc, acc)
        acc = M.mul(acc, Q[k])
    return acc


def buckets(p, bases, exps, c, terms=BUCKET_TERMS):
    M = Counter(p)
    bases = [b % p for b in bases]
    if not bases:
        return 1 % p, 0
    return _combine(M, [_bucket_chunk(M, b, e, c) for b, e in _chunks(bases, exps, terms)]), M.n
