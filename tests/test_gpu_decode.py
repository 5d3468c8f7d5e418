"""GPU: the device-side decode (include/eg_hip_decode.h, electionguard.decode), bit-exact.
batch_inverse against CPython's pow(a, -1, p) and against multInv_batch's bytes at every size where
the plan changes its shape, with zeros, 1, p - 1 and values >= p placed where a segment begins, ends
and is all zero; counts against known exponents made by the existing fixed-base path, at every
max_count of the issue, without M and with an M that has a zero row, and with 8-bit fingerprints
that make every probe collide; Decryption2 with decode="device" against the host route; the
constant-time switch's refusal; and multInv_batch's bytes with the new module loaded."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8 = np.uint8
QBAR = 0xDEC0DE
EG_ERR_STATE = 5
TOP = 4097           # the smallest n at which the plan reports three levels


def be(x, n=512):
    return np.frombuffer(int(x).to_bytes(n, "big"), U8)


def ints(a):
    return [int.from_bytes(bytes(r), "big") for r in np.asarray(a).reshape(-1, 512)]


@pytest.fixture(scope="module")
def pool(group):
    """4,097 elements, alternately of the subgroup (g^x by the fixed-base path) and random in
    [1, p), with their inverses by CPython once, and the inverses of the special values; never
    modified."""
    from electionguard import decode as dc
    p, q = group.p, group.q
    rng = random.Random(61)
    sub = ints(group.gPowP_batch([rng.randrange(q) for _ in range((TOP + 1) // 2)]))
    vals = [sub[i // 2] if i % 2 == 0 else rng.randrange(1, p) for i in range(TOP)]
    inv = [pow(v, -1, p) for v in vals]
    special = {0: 0, 1: 1, p - 1: p - 1, p: 0, p + 1: 1, 2**4096 - 1: pow((2**4096 - 1) % p, -1, p)}
    rows = np.stack([be(v) for v in vals])
    rows.setflags(write=False)
    levels = lambda n: dc.plan(n).levels
    two = next(n for n in range(17, 70001) if levels(n) == 2)
    three = next(n for n in range(two, 70001) if levels(n) == 3)
    assert (two, three) == (257, TOP) and dc.plan(TOP).seg_len == 16
    return SimpleNamespace(p=p, vals=vals, inv=inv, special=special, rows=rows, two=two, three=three)


def case(pool, n, placed):
    """The first n pool elements with the special values of placed {index: value} -> (rows, wanted ints)."""
    rows, want = pool.rows[:n].copy(), pool.inv[:n]
    for i, v in placed.items():
        rows[i], want[i] = be(v), pool.special[v]
    return rows, want


def placements(pool, n):
    """Zeros first, last and mid-segment, one all-zero segment where there is room for one, and
    1, p - 1 and the values >= p."""
    p = pool.p
    placed = {0: 0, n - 1: p}
    if n > 6:
        placed.update({5: 0, 2: 1, 3: p - 1, 4: p + 1, 6: 2**4096 - 1})
    if n >= 64:
        placed.update({i: 0 for i in range(32, 48)})        # segment 2 of 16 (segments 4 .. 5 of 8)
        placed.update({31: p - 1, 48: 1})
    return placed


@pytest.mark.parametrize("n", [1, 2, 7, 15, 16, 17, 63, 64, 65, 257, TOP])
def test_batch_inverse_against_cpython_and_multinv(group, pool, n):
    from electionguard import decode as dc
    assert n in (pool.two, pool.three) or n < pool.two
    rows, want = case(pool, n, placements(pool, n))
    got = dc.batch_inverse(group, rows)
    assert got.shape == (n, 512) and got.dtype == U8
    assert ints(got) == want
    assert np.array_equal(got, group.multInv_batch(rows))
    # the device twin, and in place on both sides
    d = group.to_device(rows)
    out = dc.batch_inverse(group, d)
    assert not isinstance(out, np.ndarray) and np.array_equal(out.download(), got)
    lib = group._lib
    assert lib.eg_batch_inverse_dev(group.handle, d.ptr, d.ptr, n) == 0
    assert np.array_equal(d.download(), got)
    same = rows.copy()
    assert lib.eg_batch_inverse(group.handle, same.ctypes.data, same.ctypes.data, n) == 0
    assert np.array_equal(same, got)


def test_an_unplaced_run_and_a_run_of_zeros_alone(group, pool):
    from electionguard import decode as dc
    assert ints(dc.batch_inverse(group, pool.rows[:300])) == pool.inv[:300]
    zeros = np.zeros((40, 512), U8)
    assert not dc.batch_inverse(group, zeros).any()


def test_ct_pow_refuses_the_inverse_and_nothing_is_written(group, pool):
    from electionguard import decode as dc
    from electionguard.core.native import EgError
    rows = pool.rows[:9]
    d_in, d_out = group.to_device(rows), group.to_device(np.full((9, 512), 0xAB, U8))
    h_out = np.full((9, 512), 0xAB, U8)
    lib = group._lib
    group.ct_pow = True
    try:
        with pytest.raises(EgError, match="variable time") as e:
            dc.batch_inverse(group, rows)
        assert e.value.code == EG_ERR_STATE
        assert lib.eg_batch_inverse(group.handle, rows.ctypes.data, h_out.ctypes.data, 9) == EG_ERR_STATE
        assert lib.eg_batch_inverse_dev(group.handle, d_in.ptr, d_out.ptr, 9) == EG_ERR_STATE
        assert b"decode" in lib.eg_last_error() and b"variable time" in lib.eg_last_error()
    finally:
        group.ct_pow = False
    assert (h_out == 0xAB).all() and (d_out.download() == 0xAB).all()
    assert ints(dc.batch_inverse(group, rows)) == pool.inv[:9]


# ---- counts ----
MAX_COUNTS = [0, 1, 3, 100, 1_000_000]


@pytest.fixture(scope="module")
def texts(group):
    """Per max_count: the texts y of the issue's exponents and non-exponents with the wanted counts,
    and one column of 300 M rows g^r with the products y * M; never modified."""
    import math
    p, q, g = group.p, group.q, group.g
    rng = random.Random(67)
    M = group.gPowP_batch([rng.randrange(1, q) for _ in range(300)])
    out = {}
    for mc in MAX_COUNTS:
        m = math.isqrt(mc) + 1
        ts = [t for t in (0, 1, m - 1, m, m + 1, mc) if t <= mc]
        ys = [pow(g, t, p) for t in ts] + [pow(g, mc + 1, p), pow(g, q - 1, p), 0, p - 1]
        want = ts + [-1] * 4
        Y = np.stack([be(y) for y in ys])
        Y.setflags(write=False)
        out[mc] = SimpleNamespace(Y=Y, want=want)
    M.setflags(write=False)
    return SimpleNamespace(by=out, M=M)


def tiled(rows, want, n):
    reps = -(-n // len(rows))
    return np.ascontiguousarray(np.concatenate([rows] * reps)[:n]), (want * reps)[:n]


@pytest.mark.parametrize("fp_bits", [0, 8], ids=["fp64", "fp8"])
@pytest.mark.parametrize("max_count", MAX_COUNTS)
def test_counts_at_every_max_count(group, texts, max_count, fp_bits):
    """fp8 at 1,000,000: 1,001 baby steps share 256 fingerprints and home slots, so every probe
    meets fingerprint matches that the comparison must reject."""
    from electionguard import decode as dc
    tx = texts.by[max_count]
    tab = dc.DecodeTable(group, max_count, fp_bits)
    try:
        for n in (1, 9, 300):
            Y, want = tiled(tx.Y, tx.want, n)
            if n == 1:                                       # the largest exponent alone
                Y, want = np.ascontiguousarray(tx.Y[len(tx.want) - 5][None]), [max_count]
            got = tab.counts(Y)                              # M = NULL: a plain dLog
            assert got.dtype == np.int64 and got.shape == (n,) and got.tolist() == want, (n, "no M")
            # y = B / M with B = y * M by the existing multiply; a zero row of M decodes to -1
            M = texts.M[:n].copy()
            B = group.multP_batch(Y, M)
            z = n // 2
            M[z] = 0
            want_m = list(want)
            want_m[z] = -1
            assert tab.counts(B, M).tolist() == want_m, (n, "M")
            if n == 9:
                dev = tab.counts(group.to_device(B), group.to_device(M))
                assert not isinstance(dev, np.ndarray) and dev.download().tolist() == want_m
                assert tab.counts(group.to_device(Y)).download().tolist() == want
    finally:
        tab.close()


def test_decode_counts_keeps_its_table_and_values_above_p_are_reduced(group, texts):
    from electionguard import decode as dc
    tx = texts.by[100]
    Y = tx.Y.copy()
    Y[0] = be(group.p + 1)                                   # 1 mod p: t = 0 still
    assert dc.decode_counts(group, Y, None, 100).tolist() == tx.want
    tab = group._decode_tables[100]
    assert dc.decode_counts(group, tx.Y, None, 100).tolist() == tx.want and group._decode_tables[100] is tab
    dc.close_tables(group)


# ---- the mediator ----
def test_decryption2_with_the_device_decode(group):
    """A small tally (with a count above max_count: None on both routes) and a small Manifest2
    table: decode="device" gives the host route's record, and the record verifier accepts."""
    from electionguard import ballot2 as b2
    from electionguard import decode as dc
    from electionguard import decrypt2 as D
    from electionguard.ballot import ElectionKey
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=11)
    comm = {g.gid: g.commitments for g in gk}
    avail = [gk[0], gk[2]]
    share_keys = D.share_public_keys(group, comm, {g.gid: g.x for g in avail})
    dec = D.Decryption2(group, QBAR, K, [D.DecryptingTrustee2(group, g) for g in avail], share_keys)
    rng = random.Random(71)
    counts = [0, 7, 3, 10, 1, 9]
    rs = [rng.randrange(1, group.q) for _ in counts]
    data = group.multP_batch(group.powP_batch([K] * len(rs), rs), group.gPowP_batch(counts))
    T = np.ascontiguousarray(np.stack([group.gPowP_batch(rs), data], axis=1))
    host, dev = dec.decrypt_record(T, 10), dec.decrypt_record(T, 10, decode="device")
    assert dev.counts == host.counts == counts and all(type(c) is int for c in dev.counts)
    assert np.array_equal(dev.M, host.M)
    assert D.verify_decryption_record2(group, QBAR, K, dev, 10) == {"proofs": True, "tally": True}
    assert dec.decrypt(T, 8, decode="device") == dec.decrypt(T, 8) == [0, 7, 3, None, 1, None]
    # ballots without placeholders, option limit 3
    key, man = ElectionKey(group, K), b2.Manifest2([(2, 3, 3), (1, 1, 1)])
    votes = np.array([[3, 0, 1], [1, 2, 0]], U8)
    sn, cn = b2.random_nonces2(np.random.default_rng(4), man, 2, group.q)
    eb = b2.encrypt(group, key, QBAR, man, votes, sn, cn)
    assert np.array_equal(dec.decryptBallots(eb, man, decode="device"), dec.decryptBallots(eb, man))
    rec = dec.decrypt_ballots_record(eb, man, decode="device")
    assert rec.counts == votes.reshape(-1).tolist() == dec.decrypt_ballots_record(eb, man).counts
    assert D.verify_decryption_record2(group, QBAR, K, rec, 3) == {"proofs": True, "tally": True}
    dc.close_tables(group)


def test_multinv_batch_keeps_its_bytes(group, pool):
    """No workspace slot is shared: multInv_batch and multP_batch give after the new calls the
    bytes they gave before them."""
    from electionguard import decode as dc
    rows, want = case(pool, 40, placements(pool, 40))
    before = group.multInv_batch(rows), group.multP_batch(rows, pool.rows[40:80])
    assert ints(before[0]) == want
    dc.batch_inverse(group, pool.rows[:300])
    tab = dc.DecodeTable(group, 100)
    tab.counts(pool.rows[:20], pool.rows[20:40])
    tab.close()
    after = group.multInv_batch(rows), group.multP_batch(rows, pool.rows[40:80])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
