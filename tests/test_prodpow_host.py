"""CPU: the host restatements of the multi-exponentiation.  prodpow.prod_pow_host and the two
schedules of tests/prodpow_ref.py agree with prod pow() on the edge bases and exponents of the ABI,
and for each forced (method, window) the library's plan is at least the multiplies the restated
schedule really runs, on random and on all-ones exponents: the bound is an upper bound of the
schedule that include/eg_hip_prodpow.h documents."""
import random

import pytest

import prodpow_ref as ref
from electionguard import prodpow as pp
from electionguard.core.constants import P, Q

EDGE_BASES = [0, 1, P - 1, P, P + 1, 2**4096 - 1]
EDGE_EXPS = [0, 1, 2, Q - 1, Q, 2**256 - 1]
FORCED = [(pp.INTERLEAVED, w) for w in (1, 2, 3, 4, 5)] + [(pp.BUCKETS, c) for c in (1, 2, 3, 4, 5)]


def want(bases, exps):
    acc = 1
    for b, e in zip(bases, exps):
        acc = acc * pow(b % P, e, P) % P
    return acc


def run(method, w, bases, exps, **kw):
    return (ref.interleaved if method == pp.INTERLEAVED else ref.buckets)(P, bases, exps, w, **kw)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_every_edge_base_under_every_edge_exponent():
    rows = [[b] * len(EDGE_EXPS) for b in EDGE_BASES]
    got = pp.prod_pow_host(P, rows, EDGE_EXPS)
    assert got == [want(r, EDGE_EXPS) for r in rows]
    for b in EDGE_BASES:
        for e in EDGE_EXPS:
            w = pow(b % P, e, P)
            assert pp.prod_pow_host(P, [[b]], [e]) == [w]
            assert ref.interleaved(P, [b], [e], 4)[0] == w and ref.buckets(P, [b], [e], 4)[0] == w
    assert pp.prod_pow_host(P, [[0, 0]], [0, 0]) == [1]                 # 0^0 = 1
    assert pp.prod_pow_host(P, [[], []], []) == [1, 1]                  # the empty product
    assert ref.interleaved(P, [], [], 4) == (1, 0) and ref.buckets(P, [], [], 4) == (1, 0)
    with pytest.raises(ValueError):
        pp.prod_pow_host(P, [[1, 2]], [1])


@pytest.mark.parametrize("method,w", FORCED)
def test_the_restated_schedules_compute_the_product(method, w):
    rng = random.Random(100 * method + w)
    bases = EDGE_BASES + [rng.randrange(P) for _ in range(3)]
    exps = [rng.randrange(Q) for _ in range(3)] + EDGE_EXPS
    assert run(method, w, bases, exps)[0] == want(bases, exps)
    # term chunks: the product of the chunks' results, one multiply per further chunk
    got, mm = run(method, w, bases, exps, terms=4)
    assert got == want(bases, exps)


@pytest.mark.parametrize("n", [1, 7, 20])
@pytest.mark.parametrize("method,w", FORCED)
def test_the_plan_bounds_the_restated_schedule(lib, method, w, n):
    rng = random.Random(n)
    bases = [rng.randrange(P) for _ in range(n)]
    bound = pp.plan(1, n, method, w)
    assert bound[:2] == (method, w)
    for exps in ([rng.randrange(Q) for _ in range(n)], [2**256 - 1] * n, [rng.getrandbits(256) for _ in range(n)]):
        got, mm = run(method, w, bases, exps)
        assert got == want(bases, exps)
        assert mm <= bound.mont_ops, (mm, bound)
    # all-ones exponents are the interleaved worst case exactly
    if method == pp.INTERLEAVED:
        assert run(method, w, bases, [2**256 - 1] * n)[1] == bound.mont_ops


def test_equal_exponents_run_the_segment_path(lib):
    # 300 terms in one bucket per window: segments of 32 and a pass over ten of them
    rng = random.Random(3)
    n = 300
    assert ref.segment(n) == 32 and ref.segment(7) == 16 and ref.segment(1 << 16) == 256
    bases = [rng.randrange(2, 1000) for _ in range(n)]
    e = rng.randrange(Q)
    got, mm = ref.buckets(P, bases, [e] * n, 4)
    prod = 1
    for b in bases:
        prod = prod * b % P
    assert got == pow(prod, e, P)
    assert mm <= pp.plan(1, n, pp.BUCKETS, 4).mont_ops


def test_a_wide_bucket_window_with_a_tree_of_bit_products(lib):
    rng = random.Random(8)
    bases = [rng.randrange(P) for _ in range(50)]
    exps = [rng.getrandbits(256) for _ in range(50)]
    got, mm = ref.buckets(P, bases, exps, 8)
    assert got == want(bases, exps)
    assert mm <= pp.plan(1, 50, pp.BUCKETS, 8).mont_ops
