"""CPU: the host mirrors of the pre-encrypted ballots (electionguard.preencrypt.*_host) against the
restatement of tests/preencrypt_ref.py and the fixture tests/golden/Mode4096/preencrypt.json in
both hash formats, recording's product property on CPython integers, and the verify mirror's
verdicts on the tamper corpus."""
import json

import numpy as np
import pytest

import preencrypt_ref as ref
from preencrypt_ref import b2i, sha


@pytest.fixture(scope="module")
def env():
    from electionguard import preencrypt as pe
    from electionguard.ballot import ElectionManifest
    from electionguard.codes import ManifestHashes
    G = ref.group()
    fx = json.loads(ref.FIXTURE.read_text())
    K, dcon, mh, ids, bn, votes = ref.fixture_inputs(fx)
    man = ElectionManifest([tuple(c) for c in fx["manifest"]])
    hashes = ManifestHashes(np.zeros((man.nsel, 32), np.uint8), dcon, mh)
    return pe, G, fx, K, man, hashes, ids, bn, votes


@pytest.fixture(scope="module")
def mirrored(env):
    """The host mirror's pre-encryption and recording of the fixture's ballots, per format."""
    pe, (p, q, g), fx, K, man, hashes, ids, bn, votes = env
    out = {}
    for fmt in ref.FORMATS:
        pre = pe.preencrypt_host(p, q, g, K, man, 2, hashes, ids, bn, fmt=fmt)
        rec = pe.record_host(p, q, g, K, man, 2, hashes, bn, votes, pre.sorted, fmt=fmt)
        out[fmt] = (pre, rec)
    return out


def rows32(hexes, shape):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), np.uint8).reshape(shape)


def test_fixture_meets_its_conditions(env):
    _, _, fx, *_ = env
    assert [tuple(c) for c in fx["manifest"]] == ref.M
    assert fx["minimal"]["zero_top_elements"] >= 1     # a P element whose minimal hex is shorter
    u1 = fx["fixed"]["unique"]["1"]
    assert 0 in u1 and 1 in u1                         # a colliding and a non-colliding ballot at one byte
    assert ref.FIXTURE.stat().st_size < 64 * 1024


def test_layout_of_the_manifest(env):
    pe, _, _, _, man, *_ = env
    sh = pe.pre_shape(man)
    assert (sh.spc, sh.limits, sh.off) == ((2, 5, 3), (1, 2, 1), (0, 2, 7))
    assert (sh.voff, sh.soff, sh.toff) == ((0, 4, 29), (0, 2, 12), (0, 1, 3))
    assert (sh.nsel, sh.V, sh.S, sh.T) == (10, 38, 15, 4)
    r = ref.shape(ref.M)
    assert (r["V"], r["S"], r["T"], r["voff"], r["soff"], r["toff"]) == (38, 15, 4, [0, 4, 29], [0, 2, 12], [0, 1, 3])


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_mirror_equals_the_fixture(env, mirrored, fmt):
    pe, _, fx, *_ = env
    pre, rec = mirrored[fmt]
    f = fx[fmt]
    assert sha(pre.vec_cts) == f["vec_cts_sha256"]
    assert np.array_equal(pre.sorted, rows32(f["sorted"], (5, 10, 32)))
    assert pre.perm.reshape(-1).tolist() == f["perm"]
    assert pre.codes.reshape(-1).tolist() == f["codes2"]
    assert pre.unique.tolist() == f["unique"]["2"]
    assert np.array_equal(pre.chash, rows32(f["chash"], (5, 3, 32)))
    assert np.array_equal(pre.conf, rows32(f["conf"], (5, 32)))
    assert rec.ok.all()
    assert sha(rec.sel_vecs) == f["sel_vecs_sha256"]
    assert rec.sel_rank.reshape(-1).tolist() == f["sel_rank"]
    assert rec.sel_codes.reshape(-1).tolist() == f["sel_codes2"]
    assert sha(rec.sel_nonces) == f["sel_nonces_sha256"]
    assert sha(rec.contest_nonces) == f["contest_nonces_sha256"]


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_mirror_equals_the_reference_run_now(env, mirrored, fmt):
    """One ballot through the reference itself (the fixture is its frozen output), and the short
    codes and flags at every code width from the mirror's ciphertexts."""
    pe, G, fx, K, man, hashes, ids, bn, votes = env
    pre, rec = mirrored[fmt]
    q = G[1]
    cts = ref.vec_cts(G, K, fmt, ref.M, bn[:1])
    assert np.array_equal(cts, pre.vec_cts[:1])
    for cb in (1, 2, 3, 4):
        want = ref.derive(q, fmt, ref.M, cb, hashes.dcon, hashes.manifest_hash, ids, pre.vec_cts)
        got = pe.hashes_from_cts_host(q, man, cb, hashes, ids, pre.vec_cts, fmt=fmt)
        for name in ("sorted", "perm", "codes", "unique", "chash", "conf"):
            assert np.array_equal(getattr(got, name), want[name]), (cb, name)
        assert got.unique.tolist() == fx[fmt]["unique"][str(cb)]
    r = ref.record(G, K, fmt, ref.M, 2, hashes.dcon, bn[:1], votes[:1], pre.sorted[:1])
    for name in ("sel_vecs", "sel_rank", "sel_codes", "sel_nonces", "contest_nonces"):
        assert np.array_equal(getattr(rec, name)[:1], r[name]), name


def test_chosen_vectors_are_stored_in_ascending_rank(env, mirrored):
    pe, _, _, _, man, *_ = env
    sh = pe.pre_shape(man)
    _, rec = mirrored["fixed"]
    r = rec.sel_rank[:, sh.toff[1]: sh.toff[1] + 2].astype(int)
    assert (r[:, 0] < r[:, 1]).all()


def test_product_of_the_chosen_vectors_is_the_encryptors_ciphertext(env, mirrored):
    pe, (p, q, g), _, K, man, _, _, _, votes = env
    _, rec = mirrored["fixed"]
    prod = pe.vector_product_host(p, man, rec.sel_vecs)
    assert np.array_equal(prod, ref.product((p, q, g), ref.M, rec.sel_vecs))
    for b in range(2):
        for s in range(man.nsel):
            R = b2i(rec.sel_nonces[b, s, 0])
            assert b2i(prod[b, s, 0]) == pow(g, R, p)
            assert b2i(prod[b, s, 1]) == pow(K, R, p) * pow(g, int(votes[b, s]), p) % p


def test_bad_votes_fail_their_contest_only(env, mirrored):
    pe, (p, q, g), _, K, man, hashes, _, bn, votes = env
    pre, _ = mirrored["fixed"]
    v = votes[:2].copy()
    v[0, 2:7] = [1, 1, 1, 0, 0]   # contest 1 sums to 3
    v[1, 7:10] = [2, 0, 0]        # a 2 in contest 2
    rec = pe.record_host(p, q, g, K, man, 2, hashes, bn[:2], v, pre.sorted[:2])
    assert rec.ok.tolist() == [[1, 0, 1], [1, 1, 0]]


def test_verify_mirror_on_the_tamper_corpus(env, mirrored):
    pe, (p, q, g), _, K, man, hashes, ids, _, votes = env
    pre, rec = mirrored["fixed"]
    good = dict(sel_vecs=rec.sel_vecs, sel_rank=rec.sel_rank, sel_codes=rec.sel_codes, sorted=pre.sorted,
                cts=pe.vector_product_host(p, man, rec.sel_vecs), conf=pre.conf)

    def verdict(a):
        return pe.verify_recorded_host(p, q, man, 2, hashes, ids, a["sel_vecs"], a["sel_rank"], a["sel_codes"],
                                       a["sorted"], a["cts"], a["conf"])
    okc, okb = verdict(good)
    assert okc.all() and okb.all()
    corpus = ref.tamper_corpus(p, ref.M, good)
    assert len(corpus) == 9
    for name, a, contests, ballots in corpus:
        okc, okb = verdict(a)
        assert {(int(b), int(k)) for b, k in zip(*np.nonzero(~okc))} == contests, name
        assert set(np.flatnonzero(~okb).tolist()) == ballots, name
