"""GPU: seeded nonces, confirmation codes, the opening and the spoiled-ballot decryption of
placeholder-free ballots (include/eg_hip_codes2.h, electionguard.codes2) against the package's host
mirror (itself pinned to tests/codes2_ref.py on the CPU) and tests/golden/Mode4096/
ballots2_seeded.json.  M0 has SN = 72, CN = 30, NS = 10: five ballots' 510 nonce threads cross a
256-thread block and the selection / contest split at thread 360 falls inside one."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest

import ballot2_ref as B2
import codes2_ref as R
import eg_oracle as O
from range_proof_ref import be2i, rows

pytestmark = pytest.mark.gpu


def down(x):
    return x if isinstance(x, np.ndarray) else x.download()


@pytest.fixture(scope="module")
def fx(group):
    """The fixture's inputs, the host mirror's nonces and the GPU's seeded ballots (never modified)."""
    from electionguard import ballot2 as b2
    from electionguard import codes as C
    from electionguard import codes2 as c2
    from electionguard.ballot import ElectionKey
    og = O.production_group()
    f = json.loads(R.FIXTURE.read_text())
    i = R.fixture_inputs(og, f)
    man = b2.Manifest2(i["man"])
    hashes = C.ManifestHashes(i["dsel"], i["dcon"], i["mh"])
    key = ElectionKey(group, i["K"])
    eb, B, codes = c2.encrypt_ballots_seeded2(group, key, i["qbar"], man, hashes, i["votes"], i["bn"], i["ids"], i["ts"],
                                              i["code_seed"])
    out = SimpleNamespace(og=og, json=f, man=man, hashes=hashes, key=key, eb=eb, B=B, codes=codes, K=i["K"],
                          qbar=i["qbar"], votes=i["votes"], bn=i["bn"], ids=i["ids"], ts=i["ts"], seed=i["code_seed"])
    for a in (eb.cts, eb.sproof, eb.cproof, B, codes, out.votes, out.bn, out.ids):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# derive
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("mode", ["Mode4096", "Mode4096_V2"])
def test_derived_nonces_equal_the_host_mirror(fx, mode, fmt):
    from electionguard import codes2 as c2
    from electionguard.core import productionGroup
    g = productionGroup(0, mode)
    sn, cn = c2.derive_nonces2_host(g.q, fx.man, fx.bn, fmt=fmt)
    assert sn.shape == (5, 72, 32) and cn.shape == (5, 30, 32)
    try:
        g.hash_format = fmt
        for nb in (1, 5):
            h_sn, h_cn = c2.derive_nonces2(g, fx.man, fx.bn[:nb])
            d_sn, d_cn = c2.derive_nonces2(g, fx.man, g.to_device(fx.bn[:nb]))
            assert isinstance(h_sn, np.ndarray) and not isinstance(d_sn, np.ndarray)
            for got_s, got_c in ((h_sn, h_cn), (down(d_sn), down(d_cn))):
                assert np.array_equal(got_s, sn[:nb]) and np.array_equal(got_c, cn[:nb]), (nb, mode, fmt)
    finally:
        g.hash_format = "fixed"
    if mode == "Mode4096":
        assert [bytes(b[0]).hex() for b in sn] == fx.json[fmt]["sel_nonces_first"]
        assert [bytes(b[-1]).hex() for b in cn] == fx.json[fmt]["contest_nonces_last"]


# ---------------------------------------------------------------------------------------------
# seeded encryption, hashes and the chain
# ---------------------------------------------------------------------------------------------
def test_seeded_encryption_reproduces_the_fixture(group, fx):
    from electionguard import ballot2 as b2
    want = fx.json["fixed"]
    assert (R.sha(fx.eb.cts), R.sha(fx.eb.sproof), R.sha(fx.eb.cproof)) == \
        (want["cts_sha256"], want["sproof_sha256"], want["cproof_sha256"])
    assert [bytes(r).hex() for r in fx.B] == want["ballot_hashes"]
    assert [bytes(r).hex() for r in fx.codes] == want["codes"]
    ok_s, ok_c, _ = b2.Verifier2(group, fx.key, fx.qbar, fx.man).verify(fx.eb, with_tally=False)
    assert ok_s.shape == (5, 10) and ok_c.shape == (5, 4) and ok_s.all() and ok_c.all()


def test_seeded_encryption_in_the_minimal_format(group, fx):
    from electionguard import codes2 as c2
    want = fx.json["minimal"]
    try:
        group.hash_format = "minimal"
        eb, B, codes = c2.encrypt_ballots_seeded2(group, fx.key, fx.qbar, fx.man, fx.hashes, fx.votes, fx.bn, fx.ids,
                                                  fx.ts, fx.seed)
    finally:
        group.hash_format = "fixed"
    assert (R.sha(eb.cts), R.sha(eb.sproof), R.sha(eb.cproof)) == \
        (want["cts_sha256"], want["sproof_sha256"], want["cproof_sha256"])
    assert [bytes(r).hex() for r in B] == want["ballot_hashes"] and [bytes(r).hex() for r in codes] == want["codes"]


def test_code_chain_of_seeded_ballots(group, fx):
    from electionguard import codes2 as c2
    args = (group, fx.man, fx.hashes, fx.ids)
    ok = c2.verify_ballot_codes2(*args, fx.eb.cts, fx.ts, fx.seed, fx.codes)
    assert ok.dtype == bool and ok.shape == (5,) and ok.all()
    bad = fx.codes.copy()
    bad[2, 7] ^= 0x10      # ballot 2's own link, and ballot 3's: a link reads the recorded predecessor
    assert c2.verify_ballot_codes2(*args, fx.eb.cts, fx.ts, fx.seed, bad).tolist() == [True, True, False, False, True]
    cts = fx.eb.cts.copy()
    cts[1, 9, 1, 300] ^= 1
    assert c2.verify_ballot_codes2(*args, cts, fx.ts, fx.seed, fx.codes).tolist() == [True, False, True, True, True]


def test_a_vote_over_its_option_limit_raises(group, fx):
    from electionguard import codes2 as c2
    votes = fx.votes.copy()
    votes[4, 0] = 2
    with pytest.raises(ValueError, match="ballot 4 contest 0 selection 0 holds 2, above its option limit 1"):
        c2.encrypt_ballots_seeded2(group, fx.key, fx.qbar, fx.man, fx.hashes, votes, fx.bn, fx.ids, fx.ts, fx.seed)


def test_ballot_hashes_dev_with_spc_nsel_equal_the_host_mirror(group, fx):
    from electionguard import codes2 as c2
    want = c2.ballot_hashes2_host(group.q, fx.man, fx.hashes, fx.ids, fx.eb.cts)
    got = c2.ballot_hashes2(group, fx.man, fx.hashes, group.to_device(fx.ids), group.to_device(fx.eb.cts), parts=True)
    host = c2.ballot_hashes2(group, fx.man, fx.hashes, fx.ids, fx.eb, parts=True)
    for w, d, h in zip(want, got, host):
        assert not isinstance(d, np.ndarray) and np.array_equal(down(d), w) and np.array_equal(h, w)
    assert np.array_equal(want[0], fx.B) and want[1].shape == (5, 10, 32) and want[2].shape == (5, 4, 32)


# ---------------------------------------------------------------------------------------------
# open
# ---------------------------------------------------------------------------------------------
def opened(group, key, man, cts, bn, dev):
    from electionguard import codes2 as c2
    if dev:
        cts, bn = group.to_device(np.ascontiguousarray(cts)), group.to_device(np.ascontiguousarray(bn))
    votes, ok = c2.open_ballots2(group, key, man, cts, bn)
    return down(votes), down(ok).astype(bool)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_open_returns_the_votes(group, fx, dev):
    votes, ok = opened(group, fx.key, fx.man, fx.eb.cts, fx.bn, dev)
    assert votes.dtype == np.uint8 and votes.shape == (5, 10) and ok.shape == (5, 10)
    assert ok.all() and np.array_equal(votes, fx.votes)
    votes, ok = opened(group, fx.key, fx.man, fx.eb.cts[3:4], fx.bn[3:4], dev)      # one ballot: 10 of a block's 32 groups
    assert ok.all() and np.array_equal(votes, fx.votes[3:4])


@pytest.mark.parametrize("ct", [False, True], ids=["radix", "ct_pow"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_open_tamper_matrix(group, fx, dev, ct):
    cts, bn, want_v, want_ok = R.tamper_matrix(fx.og, fx.eb.cts, fx.bn, fx.votes)
    group.ct_pow = ct
    try:
        votes, ok = opened(group, fx.key, fx.man, cts, bn, dev)
    finally:
        group.ct_pow = False
    assert np.array_equal(ok, want_ok), np.argwhere(ok != want_ok).tolist()
    assert np.array_equal(votes, want_v)


def encrypted_for(group, fx, man, votes, seed):
    """Ciphertexts of votes under nonces derived from fresh ballot nonces, by the device encryptor
    (it encrypts any byte; a vote over a limit only costs its proof rows) -> cts, bn, sn, cn."""
    from electionguard import ballot2 as b2
    from electionguard import codes2 as c2
    votes = np.asarray(votes, np.uint8).reshape(-1, man.NS)
    bn = np.random.default_rng(seed).integers(0, 256, (len(votes), 32), np.uint8)
    sn, cn = c2.derive_nonces2_host(group.q, man, bn)
    eb = b2.encrypt(group, fx.key, fx.qbar, man, group.to_device(votes), group.to_device(sn), group.to_device(cn))
    return eb.cts.download(), bn, sn, cn


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_open_at_the_cap_and_per_selection_limits(group, fx, dev):
    from electionguard import ballot2 as b2
    man = b2.Manifest2([(2, 15, 15)])
    votes = np.array([[15, 0], [0, 15]], np.uint8)      # the last and the first iteration of the match loop
    cts, bn, _, _ = encrypted_for(group, fx, man, votes, 5)
    got, ok = opened(group, fx.key, man, cts, bn, dev)
    assert ok.all() and np.array_equal(got, votes)
    over = cts.copy()                                    # 16 = the cap + 1 never opens
    over[0, 0, 1] = rows([be2i(cts[0, 0, 1]) * fx.og.g % fx.og.p], 512)[0]
    got, ok = opened(group, fx.key, man, over, bn, dev)
    assert ok.tolist() == [[False, True], [True, True]] and got.tolist() == [[0, 0], [0, 15]]
    mixed = b2.Manifest2([(2, 1, 1), (2, 15, 15)])      # one wave holds limits 1 and 15
    votes = np.array([[2, 1, 2, 0]], np.uint8)
    cts, bn, _, _ = encrypted_for(group, fx, mixed, votes, 6)
    got, ok = opened(group, fx.key, mixed, cts, bn, dev)
    assert ok.tolist() == [[False, True, True, True]] and got.tolist() == [[0, 1, 2, 0]]


def test_open_and_derive_across_a_chunk_boundary(group, fx):
    from electionguard import ballot2 as b2
    from electionguard import codes2 as c2
    man = b2.Manifest2([(64, 15, 15)])
    assert b2.chunk_ballots(man) == 33
    nb = 34
    votes = b2.random_votes2(np.random.default_rng(9), man, nb)
    assert votes.max() <= 15 and votes[32].any() and votes[33].any()
    cts, bn, sn, cn = encrypted_for(group, fx, man, votes, 10)
    h_sn, h_cn = c2.derive_nonces2(group, man, bn)       # the host variant, staged in two chunks
    assert np.array_equal(h_sn, sn) and np.array_equal(h_cn, cn)
    for dev in (False, True):
        got, ok = opened(group, fx.key, man, cts, bn, dev)
        assert ok.all(), (dev, np.argwhere(~ok)[:4].tolist())
        assert np.array_equal(got, votes), dev
        assert np.array_equal(got[32:], votes[32:])      # either side of the boundary


# ---------------------------------------------------------------------------------------------
# spoiled ballots through the trustees
# ---------------------------------------------------------------------------------------------
def test_spoiled_ballots_through_three_trustees(group, fx):
    from electionguard import codes2 as c2
    from electionguard.ballot import ElectionKey
    from electionguard.decrypt import DecryptingTrustee, Decryption
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=16)
    key = ElectionKey(group, K)
    eb, _, _ = c2.encrypt_ballots_seeded2(group, key, fx.qbar, fx.man, fx.hashes, fx.votes, fx.bn, fx.ids, fx.ts, fx.seed)
    comm = {g.gid: g.commitments for g in gk}
    avail = [DecryptingTrustee(group, g, comm) for g in gk[:2]]
    dec = Decryption(group, fx.qbar, avail, [gk[2].gid], {g.gid: g.public_key for g in gk})
    # a sixth ballot: ballot 0 with selection 3 (2 of at most 2) times g, so it holds olimit + 1 = 3, which
    # the manifest's largest option limit (3) still finds
    cts = np.concatenate([eb.cts, eb.cts[:1]])
    cts[5, 3, 1] = rows([be2i(cts[5, 3, 1]) * fx.og.g % fx.og.p], 512)[0]
    got = c2.decrypt_ballots2(dec, cts, fx.man)
    want = np.concatenate([fx.votes, fx.votes[:1]]).astype(np.int64)
    want[5, 3] = -1
    assert got.dtype == np.int64 and np.array_equal(got, want)
    rec = c2.decrypt_ballots2_record(dec, cts[5:], fx.man)
    assert rec.counts[3] == 3 and len(rec.counts) == 10 and sorted(rec.direct) == sorted(g.gid for g in gk[:2])


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def test_argument_errors_name_ballot2(group, fx):
    from electionguard.core import native
    from electionguard.core.marshal import u32p
    lib, man = group._lib, fx.man
    shape = (man.n_contests, u32p(man.nsel), u32p(man.olimit), u32p(man.climit))
    K = native.buf(fx.key.K_be)
    d_bn, d_cts = group.to_device(fx.bn[:1]), group.to_device(fx.eb.cts[:1])
    d_sn, d_cn = group.device_empty((1, 72, 32)), group.device_empty((1, 30, 32))
    d_v, d_ok = group.device_empty((1, 10)), group.device_empty((1, 10))
    P = ctypes.c_void_p
    for name, args in (("eg_derive_ballot_nonces_v2_dev", (1, *shape, P(d_bn.ptr + 1), P(d_sn.ptr), P(d_cn.ptr))),
                       ("eg_derive_ballot_nonces_v2_dev", (1, *shape, P(d_bn.ptr), P(d_sn.ptr + 8), P(d_cn.ptr))),
                       ("eg_open_ballots_v2_dev", (K, 1, *shape, P(d_bn.ptr), P(d_cts.ptr + 4), P(d_v.ptr), P(d_ok.ptr)))):
        assert getattr(lib, name)(group.handle, *args) == 1, name
        assert b"ballot2" in lib.eg_last_error() and b"aligned" in lib.eg_last_error()
    # votes and ok are single bytes: any address
    assert lib.eg_open_ballots_v2_dev(group.handle, K, 1, *shape, P(d_bn.ptr), P(d_cts.ptr), P(d_v.ptr + 1),
                                      P(d_ok.ptr + 3)) == 0
    group.sync()
    wide = [np.array([x], np.uint32) for x in (2200, 15, 15)]        # J = 2 * 15 * 2200 + 30 > 2^16
    for name, args in (("eg_derive_ballot_nonces_v2", (1, 1, *map(u32p, wide), P(d_bn.ptr), P(d_sn.ptr), P(d_cn.ptr))),
                       ("eg_open_ballots_v2_dev", (K, 1, 1, *map(u32p, wide), P(d_bn.ptr), P(d_cts.ptr), P(d_v.ptr),
                                                   P(d_ok.ptr)))):
        assert getattr(lib, name)(group.handle, *args) == 1, name
        assert b"ballot2" in lib.eg_last_error() and b"2^16" in lib.eg_last_error()


def test_no_ballots_write_nothing(group, fx):
    from electionguard.core import native
    from electionguard.core.marshal import ptr, u32p
    lib, man = group._lib, fx.man
    shape = (man.n_contests, u32p(man.nsel), u32p(man.olimit), u32p(man.climit))
    K = native.buf(fx.key.K_be)
    sent = lambda n: np.full(n, 0xAB, np.uint8)
    sn, cn, v, ok = sent(72 * 32), sent(30 * 32), sent(10), sent(10)
    assert lib.eg_derive_ballot_nonces_v2(group.handle, 0, *shape, None, ptr(sn), ptr(cn)) == 0
    assert lib.eg_open_ballots_v2(group.handle, K, 0, *shape, None, None, ptr(v), ptr(ok)) == 0
    d = [group.to_device(a) for a in (sn, cn, v, ok)]
    P = ctypes.c_void_p
    assert lib.eg_derive_ballot_nonces_v2_dev(group.handle, 0, *shape, None, P(d[0].ptr), P(d[1].ptr)) == 0
    assert lib.eg_open_ballots_v2_dev(group.handle, K, 0, *shape, None, None, P(d[2].ptr), P(d[3].ptr)) == 0
    for a, b in zip((sn, cn, v, ok), d):
        assert (a == 0xAB).all() and (b.download() == 0xAB).all()
