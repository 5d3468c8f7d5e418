"""CPU: the host mirror of the 0..L range proof (electionguard.range_proof.prove_host /
verify_host) against the oracle at L = 1, against the reference of tests/range_proof_ref.py and
against the fixture tests/golden/Mode4096/range_proofs.json at every limit and format, and the
verifier's rejections."""
import json

import numpy as np
import pytest

import eg_oracle as O
import range_proof_ref as ref
from range_proof_ref import be2i, rows


@pytest.fixture(scope="module")
def env():
    from electionguard import range_proof as rp
    G = O.production_group()
    fx = json.loads(ref.FIXTURE.read_text())
    K, qbar = ref.fixture_key(G, fx)
    return rp, G, fx, K, qbar


def host_group(rp, G, case=None):
    if case is None:
        return rp.HostGroup(G.p, G.q, G.g)
    return rp.HostGroup(G.p, G.q, G.g, case["hash_format"], (case["response"], case["preimage"]))


def expected(case):
    L = case["limit"]
    return np.stack([np.frombuffer(bytes.fromhex(p), np.uint8).reshape(L + 1, 2, 32) for p in case["proofs"]])


def test_limit_1_is_the_oracle_selection_proof(env):
    rp, G, fx, K, qbar = env
    case = next(c for c in fx["cases"] if c["name"] == "L1")
    inp = ref.case_inputs(G, K, fx, case)
    hg = host_group(rp, G)
    mirror = rp.prove_host(hg, K, qbar, 1, inp["cts"], inp["values"], inp["R"], inp["nonces"])
    refp = ref.prove_arrays(G, K, qbar, 1, inp["cts"], inp["values"], inp["R"], inp["nonces"])
    for i, m in enumerate(inp["values"]):
        ct = O.Ciphertext(be2i(inp["cts"][i, 0]), be2i(inp["cts"][i, 1]))
        f = 1 - int(m)   # (c_fake, v_fake) are the nonces of the other branch
        pr = O.make_range_proof(G, K, qbar, ct, int(m), be2i(inp["R"][i]), be2i(inp["nonces"][i, 0]),
                                be2i(inp["nonces"][i, 1 + 2 * f]), be2i(inp["nonces"][i, 2 + 2 * f]))
        want = rows([pr.c0, pr.v0, pr.c1, pr.v1], 32).reshape(2, 2, 32)
        assert np.array_equal(mirror[i], want) and np.array_equal(refp[i], want)
        assert O.verify_range_proof(G, K, qbar, ct, pr)
    assert rp.verify_host(hg, K, qbar, 1, inp["cts"], mirror).all()
    assert ref.verify_arrays(G, K, qbar, 1, inp["cts"], refp).all()


def test_fixture_covers_the_stated_cases(env):
    _, _, fx, _, _ = env
    by = {c["name"]: c for c in fx["cases"]}
    assert {c["limit"] for c in fx["cases"]} == {1, 2, 3, 4, 15}
    for L in (1, 2, 3):
        assert by["L%d" % L]["values"] == list(range(L + 1))
    assert by["L15"]["values"] == [0, 7, 15]
    six = {(c["response"], c["preimage"]) for c in fx["cases"] if c["limit"] == 2 and c["hash_format"] == "fixed"}
    assert six == {(r, p) for r in O.RESPONSES for p in O.PREIMAGES}
    assert ref.FIXTURE.stat().st_size < 64 * 1024


def test_mirror_equals_reference_and_fixture_at_every_limit_and_format(env):
    rp, G, fx, K, qbar = env
    for case in fx["cases"]:
        L, want = case["limit"], expected(case)
        inp = ref.case_inputs(G, K, fx, case)
        hg = host_group(rp, G, case)
        got = rp.prove_host(hg, K, qbar, L, inp["cts"], inp["values"], inp["R"], inp["nonces"])
        assert np.array_equal(got, want), case["name"]
        # the reference again (it wrote the fixture), on the first and the last item of the case
        pick = [0, len(want) - 1]
        with O.hash_format(case["hash_format"]), O.proof_format(case["response"], case["preimage"]):
            again = ref.prove_arrays(G, K, qbar, L, inp["cts"][pick], inp["values"][pick], inp["R"][pick],
                                     inp["nonces"][pick])
            assert np.array_equal(again, want[pick]), case["name"]
            # both verifiers accept, on the last item (the largest value)
            assert ref.verify_arrays(G, K, qbar, L, inp["cts"][-1:], want[-1:]).all(), case["name"]
        assert rp.verify_host(hg, K, qbar, L, inp["cts"][-1:], want[-1:]).all(), case["name"]


def test_own_format_only(env):
    """An L = 2 proof verifies under its own format and under no other (mirror)."""
    rp, G, fx, K, qbar = env
    cases = [c for c in fx["cases"] if c["limit"] == 2]
    inp = ref.case_inputs(G, K, fx, cases[0])
    proofs = {c["name"]: expected(c)[1:2] for c in cases}
    for c in cases:
        hg = host_group(rp, G, c)
        for name, pr in proofs.items():
            same = np.array_equal(pr, proofs[c["name"]])  # the hex forms differ only on a leading zero byte
            assert bool(rp.verify_host(hg, K, qbar, 2, inp["cts"][1:2], pr)[0]) == same, (c["name"], name)


def _both(env, L, cts, proofs):
    rp, G, _, K, qbar = env
    a = rp.verify_host(host_group(rp, G), K, qbar, L, cts, proofs)
    b = ref.verify_arrays(G, K, qbar, L, cts, proofs)
    assert np.array_equal(a, b)
    return a


def test_rejections(env):
    rp, G, fx, K, qbar = env
    case = next(c for c in fx["cases"] if c["name"] == "L2")
    inp = ref.case_inputs(G, K, fx, case)
    L, i = 2, 1
    ct, pr = inp["cts"][i:i + 1], expected(case)[i:i + 1]
    assert _both(env, L, ct, pr).all()
    bad_cts, bad_prs = [], []
    for j in range(L + 1):           # each c_j and v_j changed
        for w in range(2):
            t = pr.copy()
            t[0, j, w, 31] ^= 1
            bad_cts.append(ct)
            bad_prs.append(t)
    for comp in range(2):            # alpha and beta changed (multiplied by g: still valid residues)
        t = ct.copy()
        t[0, comp] = rows([G.multP(be2i(ct[0, comp]), G.g)], 512)[0]
        bad_cts.append(t)
        bad_prs.append(pr)
    t = pr.copy()                    # v_1 = q
    t[0, 1, 1] = rows([G.q], 32)[0]
    bad_cts.append(ct)
    bad_prs.append(t)
    t = ct.copy()                    # alpha -> p - alpha, a non-residue
    t[0, 0] = rows([G.p - be2i(ct[0, 0])], 512)[0]
    assert not O.is_valid_residue(G, G.p - be2i(ct[0, 0]))
    bad_cts.append(t)
    bad_prs.append(pr)
    got = _both(env, L, np.concatenate(bad_cts), np.concatenate(bad_prs))
    assert not got.any(), got


def test_a_value_above_the_limit_cannot_be_proved(env):
    """beta = K^R g^(L+1), proved by claiming m = L: the mirror and the reference build the same
    proof, and neither verifier accepts it."""
    rp, G, fx, K, qbar = env
    case = next(c for c in fx["cases"] if c["name"] == "L2")
    inp = ref.case_inputs(G, K, fx, case)
    L = 2
    R, nonces = inp["R"][:1], inp["nonces"][:1]
    cts = ref.encrypt_arrays(G, K, [L + 1], R)
    lie = np.array([L], np.uint8)
    a = rp.prove_host(host_group(rp, G), K, qbar, L, cts, lie, R, nonces)
    b = ref.prove_arrays(G, K, qbar, L, cts, lie, R, nonces)
    assert np.array_equal(a, b)
    assert not _both(env, L, cts, a).any()
    with pytest.raises(ValueError):
        rp.prove_host(host_group(rp, G), K, qbar, L, cts, np.array([L + 1], np.uint8), R, nonces)
