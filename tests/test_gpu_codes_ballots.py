"""GPU: encryption from one nonce per ballot (codes.encrypt_ballots_seeded), opening a ballot
from that nonce without trustees (codes.open_ballots), and the record verifier's ballot_codes
check, on a ragged and on the uniform manifest."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAGGED = [(2, 1), (1, 1)]
NB = 4
QBAR = 0xC0DE5


def _inputs(group, man, seed):
    from electionguard.ballot import random_votes
    from electionguard.codes import ManifestHashes
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    return dict(man=man, votes=random_votes(rng, man, NB), bn=r(NB, 32), ids=r(NB, 32), seed=r(32),
                ts=[1700000000 + 5 * b for b in range(NB)],
                hashes=ManifestHashes(r(man.nsel, 32), r(man.n_contests, 32), r(32)))


@pytest.fixture(scope="module")
def ceremony(group):
    from electionguard.ballot import ElectionKey
    from electionguard.keyceremony import key_ceremony
    gk, K = key_ceremony(group, 3, 2, seed=91)
    return gk, K, ElectionKey(group, K)


@pytest.fixture(scope="module")
def ragged(group, ceremony):
    """4 seeded ballots on [(2,1),(1,1)], encrypted once and left unchanged"""
    from electionguard.ballot import ElectionManifest
    from electionguard.codes import encrypt_ballots_seeded
    _, _, key = ceremony
    d = _inputs(group, ElectionManifest(RAGGED), 31)
    d["eb"], d["B"], d["codes"] = encrypt_ballots_seeded(group, key, QBAR, d["man"], d["hashes"], d["votes"], d["bn"],
                                                        d["ids"], d["ts"], d["seed"])
    return d


def _check_seeded(group, key, d):
    from electionguard import codes as C
    from electionguard.ballot import Verifier, batch_encryption
    man = d["man"]
    sn, cn = C.derive_nonces_host(group.q, man, d["bn"])
    want = batch_encryption(group, key, QBAR, man, d["votes"], sn, cn)
    eb = d["eb"]
    assert eb.cts.shape == want.cts.shape and eb.rproof.shape == want.rproof.shape and eb.cproof.shape == want.cproof.shape
    assert np.array_equal(eb.cts, want.cts) and np.array_equal(eb.rproof, want.rproof)
    assert np.array_equal(eb.cproof, want.cproof)
    ok_s, ok_c, _ = Verifier(group, key, QBAR, man).verify(eb)
    assert ok_s.all() and ok_c.all()
    assert np.array_equal(d["B"], C.ballot_hashes_host(group.q, man, d["hashes"], d["ids"], eb.cts)[0])
    assert np.array_equal(d["codes"], C.chain_codes(group.q, d["seed"], d["ts"], d["B"]))
    assert C.verify_code_chain(group, d["seed"], d["ts"], C.ballot_hashes(group, man, d["hashes"], d["ids"], eb.cts),
                               d["codes"]).tolist() == [True] * NB


def test_seeded_encryption_equals_injected_nonces_ragged(group, ceremony, ragged):
    _check_seeded(group, ceremony[2], ragged)


def test_seeded_encryption_uniform_constant_time(group, ceremony):
    from electionguard.ballot import Manifest
    from electionguard.codes import encrypt_ballots_seeded
    key = ceremony[2]
    d = _inputs(group, Manifest(2, 2, 1), 32)
    group.ct_encrypt = True
    try:
        d["eb"], d["B"], d["codes"] = encrypt_ballots_seeded(group, key, QBAR, d["man"], d["hashes"], d["votes"],
                                                            d["bn"], d["ids"], d["ts"], d["seed"])
    finally:
        group.ct_encrypt = False
    _check_seeded(group, key, d)


def test_open_ballots_from_their_nonces(group, ceremony, ragged):
    from electionguard.codes import open_ballots
    key, d = ceremony[2], ragged
    votes, ok = open_ballots(group, key, d["man"], d["eb"], d["bn"])
    assert ok.shape == (NB, d["man"].nsel) and ok.all()
    assert np.array_equal(votes, d["votes"])
    bn = d["bn"].copy()
    bn[1, 9] ^= 0x20
    votes, ok = open_ballots(group, key, d["man"], d["eb"], bn)
    assert not ok[1].any()
    others = [0, 2, 3]
    assert ok[others].all() and np.array_equal(votes[others], d["votes"][others])


def test_record_with_codes(group, ceremony, ragged):
    from electionguard.ballot import Verifier
    from electionguard.decrypt import DecryptingTrustee, Decryption
    from electionguard.record import ElectionRecord, GuardianRecord, verify_election_record
    (gk, K, key), d = ceremony, ragged
    man, eb = d["man"], d["eb"]
    _, _, tally = Verifier(group, key, QBAR, man).verify(eb)
    comm = {g.gid: g.commitments for g in gk}
    drec = Decryption(group, QBAR, [DecryptingTrustee(group, g, comm) for g in gk[:2]], [g.gid for g in gk[2:]],
                      {g.gid: g.public_key for g in gk}).decrypt_record(tally, NB)
    guardians = [GuardianRecord(g.gid, g.x, list(g.commitments), list(g.proofs)) for g in gk]
    plain = ElectionRecord(man, QBAR, K, guardians, eb, tally, drec)
    base = verify_election_record(group, plain)
    assert all(base.values()) and "ballot_codes" not in base, base
    rec = ElectionRecord(man, QBAR, K, guardians, eb, tally, drec, ballot_ids=d["ids"], timestamps=d["ts"],
                         code_seed=d["seed"], codes=d["codes"], hashes=d["hashes"])
    res = verify_election_record(group, rec)
    assert sorted(res) == sorted(list(base) + ["ballot_codes"]) and all(res.values()), res
    bad = copy.copy(rec)
    bad.codes = d["codes"].copy()
    bad.codes[3, 17] ^= 0x02
    res = verify_election_record(group, bad)
    assert sorted(k for k, v in res.items() if not v) == ["ballot_codes"]
