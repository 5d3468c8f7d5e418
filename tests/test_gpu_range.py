"""GPU: the 0..L range proofs (include/eg_hip_range.h, electionguard.range_proof) against the
reference of tests/range_proof_ref.py: the prover's bytes, the verifier's verdicts on honest and
tampered items, the formats, the constant-time prover, other groups, the argument checks, the host
variants' chunk boundary, contest limits without placeholders and selections of several votes."""
import json
from pathlib import Path

import numpy as np
import pytest

import eg_oracle as O
import range_proof_ref as ref
from range_proof_ref import be2i, rows

pytestmark = pytest.mark.gpu

SECRET = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
QBAR = int.from_bytes(bytes([0]) + bytes(range(1, 32)), "big")   # a leading zero byte: the hex forms differ
HASHES = ("fixed", "minimal")
FORMATS = [(h, r, p) for h in HASHES for r in O.RESPONSES for p in O.PREIMAGES]


@pytest.fixture(scope="module")
def env(group):
    from electionguard.ballot import ElectionKey
    og = O.production_group()
    K = og.gPowP(SECRET)
    return og, K, ElectionKey(group, K)


def encrypt_gpu(group, K, values, R):
    """(g^R, K^R g^m) through the fixed-base batch calls -> (n, 2, 512)"""
    from electionguard.core.group import FixedBase
    n = len(values)
    m32 = np.zeros((n, 32), np.uint8)
    m32[:, 31] = values
    kt = FixedBase(group, K)
    try:
        beta = group.multP_batch(kt.pow_batch(R), group.gPowP_batch(m32))
    finally:
        kt.close()
    return np.ascontiguousarray(np.stack([group.gPowP_batch(R), beta], axis=1))


def make_items(group, K, q, L, n, seed, values=None):
    from electionguard.ballot import random_scalars
    rng = np.random.default_rng(seed)
    if values is None:
        values = (np.arange(n) % (L + 1)).astype(np.uint8)   # every value 0..L once n > L
        if n == 1:
            values[:] = L
    values = np.asarray(values, np.uint8)
    R = random_scalars(rng, (n,), q)
    nonces = random_scalars(rng, (n, 2 * L + 3), q)
    return dict(L=L, n=n, values=values, R=R, nonces=nonces, cts=encrypt_gpu(group, K, values, R))


_CACHE = {}


def honest(group, env, L, n):
    """Items and their GPU proofs at (L, n), made once and shared by the tests (never modified)."""
    from electionguard import range_proof as rp
    og, K, key = env
    if (L, n) not in _CACHE:
        it = make_items(group, K, og.q, L, n, 1000 * L + n)
        it["proofs"] = rp.prove(group, key, QBAR, L, it["cts"], it["values"], it["R"], it["nonces"])
        for a in it.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[(L, n)] = it
    return _CACHE[(L, n)]


# ---------------------------------------------------------------------------------------------
# prover
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_prover_bytes_equal_the_reference(group, env, L, n):
    og, K, _ = env
    it = honest(group, env, L, n)
    if n > L:
        assert set(it["values"].tolist()) == set(range(L + 1))
    want = ref.prove_arrays(og, K, QBAR, L, it["cts"], it["values"], it["R"], it["nonces"])
    assert np.array_equal(it["proofs"], want)


def test_limit_1_equals_the_oracle_selection_proof(group, env):
    og, K, _ = env
    it = honest(group, env, 1, 33)
    for i in (0, 1, 32):
        m, f = int(it["values"][i]), 1 - int(it["values"][i])
        ct = O.Ciphertext(be2i(it["cts"][i, 0]), be2i(it["cts"][i, 1]))
        pr = O.make_range_proof(og, K, QBAR, ct, m, be2i(it["R"][i]), be2i(it["nonces"][i, 0]),
                                be2i(it["nonces"][i, 1 + 2 * f]), be2i(it["nonces"][i, 2 + 2 * f]))
        assert np.array_equal(it["proofs"][i], rows([pr.c0, pr.v0, pr.c1, pr.v1], 32).reshape(2, 2, 32)), i


def test_fixture_bytes_including_limit_15(group):
    """Every case of tests/golden/Mode4096/range_proofs.json (L = 15 at n = 3 among them, and the
    seven format variants at L = 2): the prover reproduces the bytes, both verifier variants accept."""
    from electionguard import range_proof as rp
    from electionguard.ballot import ElectionKey
    og = O.production_group()
    fx = json.loads(ref.FIXTURE.read_text())
    K, qbar = ref.fixture_key(og, fx)
    key = ElectionKey(group, K)
    try:
        for case in fx["cases"]:
            L = case["limit"]
            inp = ref.case_inputs(og, K, fx, case)
            want = np.stack([np.frombuffer(bytes.fromhex(p), np.uint8).reshape(L + 1, 2, 32) for p in case["proofs"]])
            group.hash_format, group.proof_format = case["hash_format"], (case["response"], case["preimage"])
            got = rp.prove(group, key, qbar, L, inp["cts"], inp["values"], inp["R"], inp["nonces"])
            assert np.array_equal(got, want), case["name"]
            assert rp.verify(group, key, qbar, L, inp["cts"], got).all(), case["name"]
            d_ok = rp.verify(group, key, qbar, L, group.to_device(inp["cts"]), group.to_device(got))
            assert d_ok.download().all(), case["name"]
    finally:
        group.hash_format, group.proof_format = "fixed", ("minus", "message_first")


# ---------------------------------------------------------------------------------------------
# verifier
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_honest_proofs_are_accepted_host_and_dev(group, env, L, n):
    from electionguard import range_proof as rp
    _, _, key = env
    it = honest(group, env, L, n)
    assert rp.verify(group, key, QBAR, L, it["cts"], it["proofs"]).all()
    d_cts, d_val = group.to_device(it["cts"]), group.to_device(it["values"])
    d_pr = rp.prove(group, key, QBAR, L, d_cts, d_val, group.to_device(it["R"]), group.to_device(it["nonces"]))
    assert np.array_equal(d_pr.download(), it["proofs"])
    assert rp.verify(group, key, QBAR, L, d_cts, d_pr).download().all()


def test_tampered_items_and_only_they_are_rejected(group, env):
    from electionguard import range_proof as rp
    og, K, key = env
    L, n = 3, 33
    it = honest(group, env, L, n)
    cts, pr = it["cts"].copy(), it["proofs"].copy()
    bad = {}
    pr[2, 1, 0, 31] ^= 1; bad[2] = "c_1 changed"
    pr[5, 3, 1, 0] ^= 0x40; bad[5] = "v_3 changed"
    pr[9, [0, 2]] = pr[9, [2, 0]]; bad[9] = "branches 0 and 2 swapped"
    pr[12, 2, 1] = rows([og.q], 32)[0]; bad[12] = "v_2 = q"
    assert it["values"][19] == L   # beta g: the ciphertext then holds L + 1
    cts[19, 1] = rows([og.multP(be2i(cts[19, 1]), og.g)], 512)[0]; bad[19] = "beta -> beta g"
    cts[20, 0] = rows([og.p - be2i(cts[20, 0])], 512)[0]; bad[20] = "alpha -> p - alpha"
    cts[31, 1] = rows([og.p + 1], 512)[0]; bad[31] = "beta >= p"
    want = np.ones(n, bool)
    want[list(bad)] = False
    assert len(bad) == 7
    got = rp.verify(group, key, QBAR, L, cts, pr)
    assert got.tolist() == want.tolist(), [bad.get(k, "honest") for k in np.flatnonzero(got != want)]
    got_dev = rp.verify(group, key, QBAR, L, group.to_device(cts), group.to_device(pr)).download().astype(bool)
    assert got_dev.tolist() == want.tolist()
    assert ref.verify_arrays(og, K, QBAR, L, cts, pr).tolist() == want.tolist()


@pytest.mark.parametrize("own", FORMATS, ids=["-".join(f) for f in FORMATS])
def test_formats(group, env, own):
    """Own-format proofs are accepted, and the same bytes rejected under every other format."""
    from electionguard import range_proof as rp
    og, K, key = env
    L, n = 2, 5
    base = honest(group, env, L, n)
    try:
        group.hash_format, group.proof_format = own[0], own[1:]
        pr = rp.prove(group, key, QBAR, L, base["cts"], base["values"], base["R"], base["nonces"])
        if own == ("minimal", "plus", "with_key"):   # one variant against the reference under the oracle's switches
            with O.hash_format(own[0]), O.proof_format(*own[1:]):
                assert np.array_equal(pr, ref.prove_arrays(og, K, QBAR, L, base["cts"], base["values"], base["R"],
                                                           base["nonces"]))
        for other in FORMATS:
            group.hash_format, group.proof_format = other[0], other[1:]
            ok = rp.verify(group, key, QBAR, L, base["cts"], pr)
            assert ok.all() if other == own else not ok.any(), (own, other)
    finally:
        group.hash_format, group.proof_format = "fixed", ("minus", "message_first")


def test_constant_time_prover_gives_the_same_bytes(group, env):
    from electionguard import range_proof as rp
    _, _, key = env
    it = honest(group, env, 3, 33)
    group.ct_encrypt = True
    try:
        pr = rp.prove(group, key, QBAR, 3, it["cts"], it["values"], it["R"], it["nonces"])
    finally:
        group.ct_encrypt = False
    assert np.array_equal(pr, it["proofs"])


def _other_groups():
    gs = json.loads((Path(__file__).resolve().parent / "golden" / "test_groups.json").read_text())["groups"]
    return ["Mode4096_V2", gs[0]["name"]]


@pytest.mark.parametrize("name", _other_groups())
def test_other_groups(name):
    from electionguard import range_proof as rp
    from electionguard.ballot import ElectionKey
    from electionguard.core import GroupContext, productionGroup
    if name == "Mode4096_V2":
        og, G, own = O.production_group(O.MODE4096_V2), productionGroup(0, "Mode4096_V2"), False
    else:
        gd = next(g for g in json.loads((Path(__file__).resolve().parent / "golden" / "test_groups.json")
                                        .read_text())["groups"] if g["name"] == name)
        og = O.Group(int(gd["p"], 16), int(gd["q"], 16), int(gd["g"], 16))
        G, own = GroupContext(og.p, og.q, og.g), True
    try:
        K = og.gPowP(SECRET % og.q)
        key = ElectionKey(G, K)
        L, n = 2, 5
        it = make_items(G, K, og.q, L, n, 77)
        qbar = QBAR % og.q
        pr = rp.prove(G, key, qbar, L, it["cts"], it["values"], it["R"], it["nonces"])
        assert np.array_equal(pr, ref.prove_arrays(og, K, qbar, L, it["cts"], it["values"], it["R"], it["nonces"]))
        bad = pr.copy()
        bad[3, 2, 0, 31] ^= 1
        ok = rp.verify(G, key, qbar, L, it["cts"], bad)
        assert ok.tolist() == [True, True, True, False, True]
        assert ref.verify_arrays(og, K, qbar, L, it["cts"], bad).tolist() == ok.tolist()
    finally:
        if own:
            G.close()


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def test_arguments_on_a_live_context(group, env):
    from electionguard import range_proof as rp
    from electionguard.core import native
    _, _, key = env
    lib, h = group._lib, group.handle
    it = honest(group, env, 2, 5)
    K, qb = native.buf(key.K_be), native.buf(QBAR.to_bytes(32, "big"))
    p = lambda a: a.ctypes.data_as(native.c_vp)
    ok = np.zeros(5, np.uint8)
    out = np.zeros_like(it["proofs"])
    cts, pr, val, R, non = (np.array(it[k]) for k in ("cts", "proofs", "values", "R", "nonces"))
    for bad_limit in (0, 16):
        assert lib.eg_range_verify(h, K, qb, 5, bad_limit, p(cts), p(pr), p(ok)) == 1
        assert b"range" in lib.eg_last_error() and b"limit" in lib.eg_last_error()
        assert lib.eg_range_prove(h, K, qb, 5, bad_limit, p(cts), p(val), p(R), p(non), p(out)) == 1
        assert b"range" in lib.eg_last_error()
    assert lib.eg_range_verify(h, K, qb, 5, 2, None, p(pr), p(ok)) == 1 and b"range" in lib.eg_last_error()
    # n == 0 is fine and touches nothing
    assert lib.eg_range_verify(h, K, qb, 0, 2, None, None, None) == 0
    assert lib.eg_range_prove_dev(h, K, qb, 0, 2, None, None, None, None, None) == 0
    # a misaligned device pointer
    d_cts, d_pr, d_ok = group.to_device(cts), group.to_device(pr), group.device_empty((5,))
    raw = group.device_empty((5 * 1024 + 16,))
    assert lib.eg_range_verify_dev(h, K, qb, 5, 2, raw[8:].ptr, d_pr.ptr, d_ok.ptr) == 1
    assert b"range" in lib.eg_last_error() and b"aligned" in lib.eg_last_error()
    assert lib.eg_range_prove_dev(h, K, qb, 5, 2, d_cts.ptr, group.to_device(val).ptr, raw[8:].ptr,
                                  group.to_device(non).ptr, d_pr.ptr) == 1
    assert b"aligned" in lib.eg_last_error()
    # a value above L: the host prover names the item, the device prover writes a zero row
    val2 = val.copy()
    val2[3] = 3
    with pytest.raises(native.EgError, match=r"range: values\[3\]"):
        rp.prove(group, key, QBAR, 2, cts, val2, R, non)
    d_out = rp.prove(group, key, QBAR, 2, d_cts, group.to_device(val2), group.to_device(R), group.to_device(non))
    got = d_out.download()
    assert not got[3].any() and np.array_equal(np.delete(got, 3, 0), np.delete(pr, 3, 0))
    assert rp.verify(group, key, QBAR, 2, cts, got).tolist() == [True, True, True, False, True]


# ---------------------------------------------------------------------------------------------
# the host variants' chunk boundary
# ---------------------------------------------------------------------------------------------
def test_chunk_boundary(group, env):
    """One item more than a host-variant chunk, at L = 2: 16,385 items.  L = 1 would halve the
    reference's work on the four checked items (8 simulated branches here) but double the items
    the host prepares, and its rows are the rproof layout, whose chunk offsets a wrong stride could
    still get right; the whole test takes about half a second.  Proofs made on the device,
    verified by the host variant."""
    from electionguard import range_proof as rp
    og, K, key = env
    L = 2
    chunk = rp.chunk_items(L)
    n = chunk + 1
    it = make_items(group, K, og.q, L, n, 4242)
    d_pr = rp.prove(group, key, QBAR, L, group.to_device(it["cts"]), group.to_device(it["values"]),
                    group.to_device(it["R"]), group.to_device(it["nonces"]))
    pr = d_pr.download()
    pick = [0, chunk - 1, chunk, n - 1]
    want = ref.prove_arrays(og, K, QBAR, L, it["cts"][pick], it["values"][pick], it["R"][pick], it["nonces"][pick])
    assert np.array_equal(pr[pick], want)
    pr[chunk - 1, 0, 1, 31] ^= 1
    pr[chunk, 2, 0, 31] ^= 1
    ok = rp.verify(group, key, QBAR, L, it["cts"], pr)
    assert np.flatnonzero(~ok).tolist() == [chunk - 1, chunk]


# ---------------------------------------------------------------------------------------------
# contest limits without placeholders; selections of several votes
# ---------------------------------------------------------------------------------------------
def test_contest_limits_without_placeholders(group, env):
    from electionguard import range_proof as rp
    from electionguard.ballot import ElectionManifest, Verifier, batch_encryption, random_scalars
    og, K, key = env
    man = ElectionManifest([(3, 1), (8, 3), (1, 1)])
    nb, nc = 6, man.n_contests
    o1 = int(man.offsets[1])
    votes = np.zeros((nb, man.nsel), np.uint8)    # placeholders never set
    votes[0, [0, o1 + 1, o1 + 4, o1 + 7, int(man.offsets[2])]] = 1   # every contest at its limit (exact votes)
    votes[1, [1, o1 + 2]] = 1                                         # contest 1 undervoted, contest 2 empty
    votes[2, [o1, o1 + 3, o1 + 5]] = 1                                # contest 0 empty
    votes[3, [2, o1 + 6, int(man.offsets[2])]] = 1
    votes[5, [0, o1 + 0, o1 + 1]] = 1                                 # ballot 4 is blank
    rng = np.random.default_rng(99)
    sn = random_scalars(rng, (nb, man.nsel, 4), og.q)
    cn = random_scalars(rng, (nb, nc), og.q)
    nonces = random_scalars(rng, (nb, nc, 2 * man.max_votes_allowed + 3), og.q)
    eb = batch_encryption(group, key, QBAR, man, votes, sn, cn)
    proofs = rp.contest_limit_prove(group, key, QBAR, man, eb, votes, sn, nonces)
    assert proofs.shape == (nb, nc, 4, 2, 32)
    assert not proofs[:, [0, 2], 2:].any() and proofs[:, 1, 3].any()
    assert rp.contest_limit_verify(group, key, QBAR, man, eb, proofs).all()
    ok_sel, ok_con, tally = Verifier(group, key, QBAR, man).verify(eb)
    assert ok_sel.all()
    # the constant proof of the padded sum cannot hold for an undervoted or an empty contest
    assert ok_con[1].tolist() == [True, False, False]
    for t, s in enumerate(man.real_index):
        assert be2i(tally[t, 0]) == og.prodP([be2i(eb.cts[b, s, 0]) for b in range(nb)])
        assert be2i(tally[t, 1]) == og.prodP([be2i(eb.cts[b, s, 1]) for b in range(nb)])
    # one reference check: ballot 0's vote-for-3 contest, at its limit
    A = og.prodP([be2i(eb.cts[0, o1 + s, 0]) for s in range(8)])
    B = og.prodP([be2i(eb.cts[0, o1 + s, 1]) for s in range(8)])
    br = [(be2i(proofs[0, 1, j, 0]), be2i(proofs[0, 1, j, 1])) for j in range(4)]
    assert ref.verify(og, K, QBAR, 3, O.Ciphertext(A, B), br)
    # ballot 2 overvotes contest 1 (4 of 8) and claims 3
    over, claim = votes.copy(), votes.copy()
    over[2, o1 + 7] = 1
    eb2 = batch_encryption(group, key, QBAR, man, over, sn, cn)
    proofs2 = rp.contest_limit_prove(group, key, QBAR, man, eb2, claim, sn, nonces)
    ok2 = rp.contest_limit_verify(group, key, QBAR, man, eb2, proofs2)
    want = np.ones((nb, nc), bool)
    want[2, 1] = False
    assert ok2.tolist() == want.tolist()


def test_selections_of_several_votes(group, env):
    from electionguard import range_proof as rp
    from electionguard.core.group import ElementModP
    og, K, key = env
    nb, ns, L = 5, 4, 3
    values = np.array([[0, 1, 2, 3], [3, 3, 0, 1], [2, 0, 0, 3], [1, 1, 1, 3], [0, 2, 3, 3]], np.uint8)
    it = make_items(group, K, og.q, L, nb * ns, 5, values=values.reshape(-1))
    pr = rp.prove(group, key, QBAR, L, it["cts"], it["values"], it["R"], it["nonces"])
    assert rp.verify(group, key, QBAR, L, it["cts"], pr).all()
    # the tally: per selection the product over the ballots, opened with the secret
    cts = it["cts"].reshape(nb, ns, 2, 512)
    g = np.ascontiguousarray(np.transpose(cts, (1, 2, 0, 3))).reshape(-1, 512)
    tally = group.prodP_groups(g, ns * 2, nb).reshape(ns, 2, 512)
    for s in range(ns):
        A, B = be2i(tally[s, 0]), be2i(tally[s, 1])
        gm = og.multP(B, og.multInv(og.powP(A, SECRET)))
        assert group.dLogG(ElementModP(gm, group), nb * L) == int(values[:, s].sum())
