"""CPU: the host mirrors of electionguard.codes (nonce derivation, ballot hashes, the code chain)
against a restatement in bare hashlib (codes_ref.py), against the oracle's hash_elems, and
against the digests frozen in tests/golden/Mode4096/ballot_codes.json (inputs expanded from the
fixture's seed by a hashlib counter); the record verifier's optional ballot_codes check."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import codes_ref as R
import eg_oracle as O

GOLDEN = Path(__file__).resolve().parent / "golden" / "Mode4096" / "ballot_codes.json"
FORMATS = ("fixed", "minimal")


def fixture_inputs(fx):
    from electionguard.ballot import ElectionManifest
    from electionguard.codes import ManifestHashes
    seed = bytes.fromhex(fx["seed"])
    man = ElectionManifest([tuple(c) for c in fx["manifest"]])
    nb, nsel, nc = fx["nballots"], man.nsel, man.n_contests
    x = lambda label, shape: R.expand(seed, label, int(np.prod(shape))).reshape(shape)
    return dict(man=man, bn=x("ballot_nonces", (nb, 32)), ids=x("ballot_ids", (nb, 32)),
                cts=x("cts", (nb, nsel, 2, 512)), code_seed=x("code_seed", (32,)), ts=fx["timestamps"],
                hashes=ManifestHashes(x("dsel", (nsel, 32)), x("dcon", (nc, 32)), x("manifest_hash", (32,))))


@pytest.fixture(scope="module")
def fx():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def inp(fx):
    return fixture_inputs(fx)


@pytest.fixture(scope="module")
def q():
    return O.production_group().q


def host_all(q, inp, fmt):
    from electionguard import codes as C
    sn, cn = C.derive_nonces_host(q, inp["man"], inp["bn"], fmt=fmt)
    B, hs, hc = C.ballot_hashes_host(q, inp["man"], inp["hashes"], inp["ids"], inp["cts"], fmt=fmt)
    codes = C.chain_codes(q, inp["code_seed"], inp["ts"], B, fmt=fmt)
    return sn, cn, B, hs, hc, codes


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_mirrors_equal_the_hashlib_restatement(q, inp, fmt):
    from electionguard import codes as C
    sn, cn, B, hs, hc, codes = host_all(q, inp, fmt)
    man, h = inp["man"], inp["hashes"]
    rsn, rcn = R.nonces(q, fmt, man.spc_list, inp["bn"])
    assert np.array_equal(sn, rsn) and np.array_equal(cn, rcn)
    rB, rhs, rhc = R.hashes(q, fmt, man.spc_list, h.dsel, h.dcon, h.manifest_hash, inp["ids"], inp["cts"])
    assert np.array_equal(hs, rhs) and np.array_equal(hc, rhc) and np.array_equal(B, rB)
    ts = C.timestamp_elements(inp["ts"])
    assert [int.from_bytes(bytes(t), "big") for t in ts] == inp["ts"]
    rcodes = R.chain(q, fmt, inp["code_seed"], ts, rB)
    assert np.array_equal(codes, rcodes)
    assert C.verify_code_chain_host(q, inp["code_seed"], inp["ts"], B, codes, fmt=fmt).all()
    bad = codes.copy()
    bad[0, 5] ^= 1   # the link into ballot 0 and the link out of it
    want = R.check(q, fmt, inp["code_seed"], ts, rB, bad)
    assert want.tolist() == [False, False]
    assert np.array_equal(C.verify_code_chain_host(q, inp["code_seed"], ts, B, bad, fmt=fmt), want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_mirrors_equal_the_oracle_hash(q, inp, fmt):
    """every definition once more on eg_oracle.hash_elems (imported read-only)"""
    sn, cn, B, hs, hc, codes = host_all(q, inp, fmt)
    man, h = inp["man"], inp["hashes"]
    iv = lambda row: int.from_bytes(bytes(row), "big")
    b32 = lambda v: np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)
    with O.hash_format(fmt):
        for b in range(len(B)):
            xi = iv(inp["bn"][b])
            for r in range(4 * man.nsel):
                assert np.array_equal(sn[b, r // 4, r % 4], b32(O.hash_elems(q, ("Q", xi), ("Q", 1), ("Q", r))))
            for k in range(man.n_contests):
                assert np.array_equal(cn[b, k], b32(O.hash_elems(q, ("Q", xi), ("Q", 2), ("Q", k))))
            for s in range(man.nsel):
                want = O.hash_elems(q, ("Q", iv(h.dsel[s])), ("P", iv(inp["cts"][b, s, 0])), ("P", iv(inp["cts"][b, s, 1])))
                assert np.array_equal(hs[b, s], b32(want))
            for k, (off, n) in enumerate(zip(man.offsets, man.spc_list)):
                run = [("Q", iv(hs[b, int(off) + s])) for s in range(int(n))]
                assert np.array_equal(hc[b, k], b32(O.hash_elems(q, ("Q", iv(h.dcon[k])), *run)))
            want = O.hash_elems(q, ("Q", iv(inp["ids"][b])), ("Q", iv(h.manifest_hash)),
                                *[("Q", iv(hc[b, k])) for k in range(man.n_contests)])
            assert np.array_equal(B[b], b32(want))
            prev = iv(codes[b - 1]) if b else iv(inp["code_seed"])
            assert np.array_equal(codes[b], b32(O.hash_elems(q, ("Q", prev), ("Q", inp["ts"][b]), ("Q", iv(B[b])))))


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_mirrors_equal_the_frozen_digests(fx, q, inp, fmt):
    assert fx["manifest"] == [[2, 1], [1, 1]] and fx["nballots"] == 2
    sn, cn, B, hs, hc, codes = host_all(q, inp, fmt)
    want = fx[fmt]
    hexrows = lambda a: [bytes(r).hex() for r in a.reshape(-1, 32)]
    assert hashlib.sha256(sn.tobytes()).hexdigest() == want["sel_nonces_sha256"]
    assert hexrows(cn) == want["contest_nonces"]
    assert hashlib.sha256(hs.tobytes()).hexdigest() == want["sel_hashes_sha256"]
    assert hexrows(hc) == want["contest_hashes"]
    assert hexrows(B) == want["ballot_hashes"]
    assert hexrows(codes) == want["codes"]
    assert fx["fixed"]["codes"] != fx["minimal"]["codes"]


def test_record_verifier_adds_only_ballot_codes(monkeypatch, q, inp):
    """verify_election_record without codes returns the keys it always did; with codes it adds
    ballot_codes and nothing else.  The GPU calls are replaced by stand-ins (this is a CPU test):
    what is under test is which checks the verifier reports."""
    from electionguard import codes as C
    from electionguard import record as Rec
    from electionguard.ballot import EncryptedBallots
    man, nb = inp["man"], 2

    class Group:
        q = O.production_group().q
        hash_format = "fixed"

        def prodP_groups(self, elems, groups, length):
            return np.zeros((groups, 512), np.uint8)

    class FakeVerifier:
        def __init__(self, *a):
            pass

        def verify(self, eb, cast=None):
            return np.ones((nb, man.nsel), bool), np.ones((nb, man.n_contests), bool), np.zeros((man.n_real, 2, 512), np.uint8)

    class Dec:
        texts = np.zeros((man.n_real, 2, 512), np.uint8)

    monkeypatch.setattr(Rec, "Verifier", FakeVerifier)
    monkeypatch.setattr(Rec, "ElectionKey", lambda *a, **k: None)
    monkeypatch.setattr(Rec, "verify_commitment_proofs", lambda g, comm, prf: [True] * len(comm))
    monkeypatch.setattr(Rec, "verify_decryption_record", lambda *a, **k: {"shares": True, "tally": True})
    monkeypatch.setattr(C, "ballot_hashes",
                        lambda g, m, h, ids, cts: C.ballot_hashes_host(g.q, m, h, ids, cts, fmt=g.hash_format)[0])
    monkeypatch.setattr(C, "verify_code_chain",
                        lambda g, seed, ts, B, codes: C.verify_code_chain_host(g.q, seed, ts, B, codes, fmt=g.hash_format))
    eb = EncryptedBallots(inp["cts"], np.zeros((nb, man.nsel, 4, 32), np.uint8), np.zeros((nb, man.n_contests, 2, 32), np.uint8))
    rec = Rec.ElectionRecord(man, 1, 0, [Rec.GuardianRecord("g1", 1, [1], [(0, 0)])], eb,
                             np.zeros((man.n_real, 2, 512), np.uint8), Dec())
    assert (rec.ballot_ids, rec.timestamps, rec.code_seed, rec.codes, rec.hashes) == (None,) * 5
    base = Rec.verify_election_record(Group(), rec)
    assert sorted(base) == ["ballots", "decryption.shares", "decryption.tally", "decryption.texts", "guardian_proofs",
                            "joint_key", "tally"]
    B = C.ballot_hashes_host(q, man, inp["hashes"], inp["ids"], inp["cts"])[0]
    rec.ballot_ids, rec.timestamps, rec.code_seed, rec.hashes = inp["ids"], inp["ts"], inp["code_seed"], inp["hashes"]
    rec.codes = C.chain_codes(q, inp["code_seed"], inp["ts"], B)
    res = Rec.verify_election_record(Group(), rec)
    assert sorted(set(res) - set(base)) == ["ballot_codes"] and res["ballot_codes"]
    assert {k: res[k] for k in base} == base
    rec.codes = rec.codes.copy()
    rec.codes[1, 0] ^= 0x80
    res = Rec.verify_election_record(Group(), rec)
    assert not res["ballot_codes"] and {k: res[k] for k in base} == base
    rec.hashes = None   # codes without what the check needs: reported, not raised
    assert Rec.verify_election_record(Group(), rec)["ballot_codes"] is False
