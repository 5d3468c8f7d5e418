"""CPU: the ContestData packing and the host mirrors of electionguard.contest_data, against the
restatement on hashlib, hmac and CPython pow (contest_data_ref.py) and against the bytes frozen in
tests/golden/Mode4096/contest_data.json (inputs expanded from the fixture's seed)."""
import json
from pathlib import Path

import numpy as np
import pytest

import contest_data_ref as R
import eg_oracle as O

GOLDEN = Path(__file__).resolve().parent / "golden" / "Mode4096" / "contest_data.json"
FORMATS = ("fixed", "minimal")


@pytest.fixture(scope="module")
def fx():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def og():
    return O.production_group()


def rows(hexes):
    return np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in hexes])


# ---------------------------------------------------------------------------------------------
# pack / unpack
# ---------------------------------------------------------------------------------------------
CASES = [
    (0, [], []),
    (2, [0, 7, 65535], []),
    (3, [], ["Ada Lovelace"]),
    (1, [4], ["Zoë", "王小明", ""]),
]


@pytest.mark.parametrize("status,overvotes,write_ins", CASES)
@pytest.mark.parametrize("nbytes", [40, 64, 1024])
def test_pack_round_trips_and_matches_the_reference_layout(status, overvotes, write_ins, nbytes):
    from electionguard.contest_data import ContestData
    cd = ContestData(status, overvotes, write_ins)
    b = cd.pack(nbytes)
    assert len(b) == nbytes and b == R.pack(status, overvotes, write_ins, nbytes)
    assert ContestData.unpack(b) == cd
    used = 2 + int.from_bytes(b[:2], "big")
    assert b[used:] == bytes(nbytes - used)          # zero padding
    assert ContestData.unpack(b[:used]) == cd        # the padding is not needed to read it


def test_pack_ballots_lays_items_out_ballot_major():
    from electionguard.contest_data import ContestData, pack_ballots
    data = [[ContestData(0, [], ["a"]), ContestData(2, [1, 2], [])], [ContestData(3), ContestData(0, [], ["b", "c"])]]
    a = pack_ballots(data, 24)
    assert a.shape == (2, 2, 24) and a.dtype == np.uint8
    for b in range(2):
        for k in range(2):
            assert ContestData.unpack(a[b, k]) == data[b][k]
    with pytest.raises(ValueError):
        pack_ballots([data[0], data[1][:1]], 24)


def test_write_ins_that_do_not_fit_are_dropped_whole_and_flagged():
    from electionguard.contest_data import TRUNCATED, ContestData
    cd = ContestData(0, [9], ["abcdefgh", "ij", "klmnopqrstuvwxyz", "k"])
    # 2 length + status + count + 2 overvote + count = 7; "abcdefgh" takes 9, "ij" 3, "k" 2
    full = cd.pack(7 + 9 + 3 + 17 + 2)
    assert ContestData.unpack(full) == cd
    got = ContestData.unpack(cd.pack(7 + 9 + 3 + 2))
    assert got.write_ins == ["abcdefgh", "ij", "k"] and got.status == TRUNCATED and got.overvotes == [9]
    got = ContestData.unpack(cd.pack(7 + 9 + 3 + 1))           # one byte short of "k"
    assert got.write_ins == ["abcdefgh", "ij"] and got.status == TRUNCATED
    got = ContestData.unpack(cd.pack(7 + 8))                   # one byte short of the first
    assert got.write_ins == ["ij", "k"] and got.status == TRUNCATED
    got = ContestData.unpack(ContestData(2, [9], ["abc"]).pack(7))
    assert got == ContestData(2 | TRUNCATED, [9], [])
    # a name longer than its length byte can say
    got = ContestData.unpack(ContestData(0, [], ["x" * 256, "y" * 255]).pack(1024))
    assert got.write_ins == ["y" * 255] and got.status == TRUNCATED
    # a multi-byte name is measured in UTF-8 bytes and never split
    got = ContestData.unpack(ContestData(0, [], ["王小明"]).pack(5 + 9))
    assert got.write_ins == [] and got.status == TRUNCATED
    assert ContestData.unpack(ContestData(0, [], ["王小明"]).pack(5 + 10)).write_ins == ["王小明"]


def test_pack_rejects_what_it_cannot_represent():
    from electionguard.contest_data import ContestData
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            ContestData().pack(bad)
    with pytest.raises(ValueError):
        ContestData(0, [1, 2], []).pack(8)       # the overvotes always go in: 9 bytes needed
    assert len(ContestData(0, [1, 2], []).pack(9)) == 9
    with pytest.raises(ValueError):
        ContestData(128).pack(32)                # the truncation bit is pack's
    with pytest.raises(ValueError):
        ContestData(0, [65536]).pack(32)


def test_unpack_rejects_a_length_that_overruns_the_buffer():
    from electionguard.contest_data import ContestData
    good = ContestData(0, [3], ["abc"]).pack(32)
    used = 2 + int.from_bytes(good[:2], "big")
    assert ContestData.unpack(good[:used]).write_ins == ["abc"]
    with pytest.raises(ValueError, match="overruns"):
        ContestData.unpack(good[:used - 1])                      # the buffer ends before the recorded length
    with pytest.raises(ValueError, match="overruns"):
        ContestData.unpack((31).to_bytes(2, "big") + good[2:])   # 2 + 31 > 32
    with pytest.raises(ValueError, match="overruns"):
        ContestData.unpack(b"\xff\xff" + good[2:])
    with pytest.raises(ValueError):
        ContestData.unpack(b"\x00")
    # counts and name lengths inside a valid outer length
    body = bytes([0, 0, 1, 200]) + b"ab"
    with pytest.raises(ValueError, match="overruns"):
        ContestData.unpack(len(body).to_bytes(2, "big") + body + bytes(300))
    body = bytes([0, 9])
    with pytest.raises(ValueError, match="overruns"):
        ContestData.unpack(len(body).to_bytes(2, "big") + body + bytes(64))
    body = bytes([0, 0, 0, 7])                                   # a byte the fields do not account for
    with pytest.raises(ValueError):
        ContestData.unpack(len(body).to_bytes(2, "big") + body)


# ---------------------------------------------------------------------------------------------
# host mirrors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_nonce_mirror_equals_the_reference_and_keeps_clear_of_the_ballot_nonces(og, fmt):
    import codes_ref
    from electionguard import contest_data as CD
    bn = np.random.default_rng(5).integers(0, 256, size=(3, 32), dtype=np.uint8)
    bn[1, :20] = 0                                   # leading zero bytes: the formats differ
    r = CD.derive_nonces_host(og.q, 4, bn, fmt=fmt)
    assert r.shape == (3, 4, 32) and np.array_equal(r, R.nonces(og.q, fmt, 4, bn))
    _, cn = codes_ref.nonces(og.q, fmt, [2, 2, 2, 2], bn)
    assert not (r == cn).all(axis=2).any()           # tag 3 against tag 2


@pytest.mark.parametrize("nbytes", [1, 31, 32, 33, 64, 100])
def test_seal_and_open_mirrors_equal_the_reference(nbytes):
    from electionguard import contest_data as CD
    rng = np.random.default_rng(nbytes)
    nb, nc = 2, 3
    r = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)
    ids, c0, kappa, data = r(nb, 32), r(nb * nc, 512), r(nb * nc, 512), r(nb * nc, nbytes)
    c1, c2 = CD.seal_host(nc, ids, c0, kappa, data)
    rc1, rc2 = R.seal_with_kappa(nc, ids, c0, kappa, data)
    assert np.array_equal(c1, rc1) and np.array_equal(c2, rc2)
    got, ok = CD.open_host(nc, ids, c0, kappa, c1, c2)
    assert ok.all() and np.array_equal(got, data)
    bad = c2.copy()
    bad[4, 0] ^= 0x80
    got, ok = CD.open_host(nc, ids, c0, kappa, c1, bad)
    rgot, rok = R.open_all(nc, ids, c0, kappa, c1, bad)
    assert ok.tolist() == [True] * 4 + [False, True] == rok.tolist()
    assert np.array_equal(got, rgot) and not got[4].any() and np.array_equal(got[5], data[5])


def test_the_contest_keys_are_apart_from_the_share_keys():
    """the same kk and label under "share" give another stream: the tag enters every HMAC"""
    import hashlib
    import hmac
    from electionguard import contest_data as CD
    kk, mk, label = CD.item_keys_host(bytes(512), bytes(512), bytes(32), 1)
    assert label == bytes(32) + b"\x00\x00\x00\x01"
    assert kk == hashlib.sha256(bytes(1024)).digest()
    assert mk == hmac.new(kk, b"\x02contest" + label, hashlib.sha256).digest()
    assert CD.stream_host(kk, label, 40)[:32] == hmac.new(kk, b"\x01contest" + label + bytes(4), hashlib.sha256).digest()
    assert CD.stream_host(kk, label, 40)[:32] != hmac.new(kk, b"\x01share" + label + bytes(4), hashlib.sha256).digest()


@pytest.mark.parametrize("fmt", FORMATS)
def test_golden_fixture(og, fx, fmt):
    """the frozen bytes equal the reference's and the host mirrors': a later change of the format
    is caught here"""
    from electionguard import contest_data as CD
    assert R.fixture_outputs(og.p, og.q, og.g, fx, fmt) == fx[fmt]
    inp = R.fixture_inputs(fx)
    cds = [[CD.ContestData(c["status"], c["overvotes"], c["write_ins"]) for c in row] for row in fx["contest_data"]]
    data = CD.pack_ballots(cds, inp["nbytes"])
    assert np.array_equal(data.reshape(-1, inp["nbytes"]), inp["data"])
    K = pow(og.g, inp["secret"] % og.q, og.p)
    want = {k: rows(v) for k, v in fx[fmt].items()}
    assert np.array_equal(CD.derive_nonces_host(og.q, inp["nc"], inp["bn"], fmt=fmt).reshape(-1, 32), want["r"])
    c0, c1, c2 = CD.seal_contest_data_host(og.p, og.q, og.g, K, inp["nc"], inp["bn"], inp["ids"], data, fmt=fmt)
    assert np.array_equal(c0, want["c0"]) and np.array_equal(c1, want["c1"]) and np.array_equal(c2, want["c2"])
    # the joint secret opens it: kappa = c0^s
    kappa = rows([pow(int(h, 16), inp["secret"] % og.q, og.p).to_bytes(512, "big").hex() for h in fx[fmt]["c0"]])
    got, ok = CD.open_host(inp["nc"], inp["ids"], c0, kappa, c1, c2)
    assert ok.all()
    assert [[CD.ContestData.unpack(got[b * inp["nc"] + k]) for k in range(inp["nc"])] for b in range(inp["nb"])] == cds


def test_the_fixture_covers_both_formats_and_its_shape(fx):
    assert all(a != b for a, b in zip(fx["fixed"]["r"], fx["minimal"]["r"]))   # the small tags' hex differs
    assert all(len(fx[f][k]) == fx["nballots"] * fx["ncontest"] for f in FORMATS for k in ("r", "c0", "c1", "c2"))
    assert len(fx["fixed"]["c1"][0]) == 2 * fx["nbytes"] and len(fx["fixed"]["c2"][0]) == 64
