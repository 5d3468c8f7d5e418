"""CPU: the host mirrors of electionguard.codes2 (seeded nonces, ballot hashes, the code chain, the
opening) against tests/codes2_ref.py's restatement on the oracle and the values frozen in
tests/golden/Mode4096/ballots2_seeded.json, in both hash formats; where a selection's R sits; the
opening's tamper matrix.  No GPU call.  The reference arrays and the mirror's are computed once
per module and never modified."""
import json

import numpy as np
import pytest

import ballot2_ref as B2
import codes2_ref as R
import eg_oracle as O
from range_proof_ref import be2i

from electionguard import ballot2 as b2
from electionguard import codes as C
from electionguard import codes2 as c2
from electionguard import range_proof as rp


@pytest.fixture(scope="module")
def fx():
    return json.loads(R.FIXTURE.read_text())


@pytest.fixture(scope="module")
def env(fx):
    og = O.production_group()
    i = R.fixture_inputs(og, fx)
    return dict(og=og, hg=rp.HostGroup(og.p, og.q, og.g), man=b2.Manifest2(i["man"]),
                hashes=C.ManifestHashes(i["dsel"], i["dcon"], i["mh"]), **{k: v for k, v in i.items() if k != "man"})


@pytest.fixture(scope="module")
def ref(fx, env):
    return {fmt: R.compute(env["og"], fx, fmt) for fmt in R.FORMATS}


@pytest.fixture(scope="module")
def host(env):
    out = {}
    for fmt in R.FORMATS:
        hg = rp.HostGroup(env["og"].p, env["og"].q, env["og"].g, hash_format=fmt)
        sn, cn = c2.derive_nonces2_host(hg.q, env["man"], env["bn"], fmt=fmt)
        eb = b2.encrypt_host(hg, env["K"], env["qbar"], env["man"], env["votes"], sn, cn)
        B, hs, hc = c2.ballot_hashes2_host(hg.q, env["man"], env["hashes"], env["ids"], eb, fmt=fmt)
        codes = C.chain_codes(hg.q, env["code_seed"], env["ts"], B, fmt=fmt)
        out[fmt] = dict(sn=sn, cn=cn, cts=eb.cts, sproof=eb.sproof, cproof=eb.cproof, B=B, hs=hs, hc=hc, codes=codes)
    return out


def test_the_fixture_names_its_inputs(fx):
    assert [tuple(c) for c in fx["manifest"]] == B2.M0 and fx["votes"] == B2.VOTES0
    assert len(fx["timestamps"]) == 5 and fx["fixed"]["codes"] != fx["minimal"]["codes"]
    man = b2.Manifest2(B2.M0)
    assert (man.SN, man.CN, man.NS) == (72, 30, 10)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_host_mirrors_reproduce_the_fixture_and_the_reference(fx, ref, host, fmt):
    h, r = host[fmt], ref[fmt]
    for name in ("sn", "cn", "cts", "sproof", "cproof", "B", "hs", "hc", "codes"):
        assert np.array_equal(h[name], r[name]), name
    assert R.record(h["sn"], h["cn"], h["cts"], h["sproof"], h["cproof"], h["B"], h["codes"]) == fx[fmt]
    assert h["sn"].shape == (5, 72, 32) and h["cn"].shape == (5, 30, 32)


def test_hash_format_of_the_group_decides_the_proofs_too(host):
    assert not np.array_equal(host["fixed"]["sn"], host["minimal"]["sn"])
    assert not np.array_equal(host["fixed"]["sproof"], host["minimal"]["sproof"])


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_a_selections_R_sits_where_sn_off_says(fx, env, host, fmt):
    og, man, lay = env["og"], env["man"], B2.layout(B2.M0)
    sn, cts = host[fmt]["sn"], host[fmt]["cts"]
    walk = [(k, s, nr) for k, s, _, _, nr in lay["sels"]]
    mine = [(k, s, int(man.sn_off[k]) + i * (2 * L + 4)) for k, i, s, L, _, _ in man.selections()]
    assert walk == mine
    assert mine[0][2] == 0 and bytes(sn[0, 0]).hex() == fx[fmt]["sel_nonces_first"][0]
    with O.hash_format(fmt):
        for b in (0, 4):
            for k, s, nr in mine:
                assert be2i(sn[b, nr]) == O.hash_elems(og.q, ("Q", be2i(env["bn"][b])), ("Q", 5), ("Q", nr))
                assert be2i(cts[b, s, 0]) == og.gPowP(be2i(sn[b, nr])), (b, s)     # alpha = g^R of that row
    assert all(be2i(r) < og.q for r in sn.reshape(-1, 32)) and all(be2i(r) < og.q for r in host[fmt]["cn"].reshape(-1, 32))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_open_host_returns_the_votes(env, host, fmt):
    votes, ok = c2.open_ballots2_host(env["hg"], env["K"], env["man"], host[fmt]["cts"], env["bn"], fmt=fmt)
    assert ok.all() and ok.dtype == bool and np.array_equal(votes, env["votes"])
    other = "minimal" if fmt == "fixed" else "fixed"      # the seed is read in the group's format
    votes, ok = c2.open_ballots2_host(env["hg"], env["K"], env["man"], host[fmt]["cts"], env["bn"], fmt=other)
    assert not ok.any() and not votes.any()


def test_tamper_matrix_on_the_host_mirror(env, host):
    og = env["og"]
    cts, bn, want_v, want_ok = R.tamper_matrix(og, host["fixed"]["cts"], env["bn"], env["votes"])
    assert int(want_ok.sum()) == 50 - 10 - 5
    votes, ok = c2.open_ballots2_host(env["hg"], env["K"], env["man"], cts, bn)
    assert np.array_equal(ok, want_ok) and np.array_equal(votes, want_v)
    r_votes, r_ok = R.open_ballots(og, env["K"], B2.M0, cts, bn)
    assert np.array_equal(r_ok, want_ok) and np.array_equal(r_votes, want_v)


def test_regenerating_the_fixture_gives_the_committed_file(fx, env, ref):
    assert R.build(env["og"], ref) == fx
    assert R.FIXTURE.read_text() == json.dumps(fx, indent=1) + "\n"
