"""CPU: the C ABI for manifests of unequal contests (include/eg_hip_manifest.h) and its Python
side: the header declares exactly the four entry points, the built library exports them,
native.EXPORTED_MANIFEST lists them, each rejects a null context without touching a device;
ElectionManifest's index arithmetic; the record format's pair-list manifest."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

FOUR = ["eg_encrypt_ballots_manifest", "eg_encrypt_ballots_manifest_dev",
        "eg_verify_ballots_manifest", "eg_verify_ballots_manifest_dev"]
# (real selections, votes_allowed): spc 3, 6, 2, 3
M = [(2, 1), (4, 2), (1, 1), (2, 1)]


def header_functions():
    src = (ROOT / "include" / "eg_hip_manifest.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_four_entry_points():
    assert header_functions() == FOUR
    src = (ROOT / "include" / "eg_hip_manifest.h").read_text()
    assert '#include "eg_hip.h"' in src


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_MANIFEST) == header_functions()
    assert not set(native.EXPORTED_MANIFEST) & set(native.EXPORTED)
    for name in FOUR:
        assert hasattr(lib, name), name


def test_null_ctx_is_an_argument_error(lib):
    shape = np.array([3, 6, 2, 3], np.uint32)
    spc = shape.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.eg_verify_ballots_manifest(None, None, None, 0, 4, spc, spc, spc, None, None, None, None, None, None,
                                          None) == 1
    assert lib.eg_verify_ballots_manifest_dev(None, None, None, 0, 4, spc, spc, spc, None, None, None, None, None,
                                              None, None) == 1
    assert lib.eg_encrypt_ballots_manifest(None, None, None, 0, 4, spc, None, None, None, None, None, None) == 1
    assert lib.eg_encrypt_ballots_manifest_dev(None, None, None, 0, 4, spc, None, None, None, None, None, None) == 1
    assert b"null" in lib.eg_last_error()


def test_election_manifest_indices():
    from electionguard.ballot import Contest, ElectionManifest, Manifest
    man = ElectionManifest(M)
    assert man.contests[1] == Contest(4, 2)
    assert man.n_contests == 4 and man.nsel == 14 and man.n_real == 9 and man.max_votes_allowed == 2
    assert man.spc_list.tolist() == [3, 6, 2, 3] and man.spc_list.dtype == np.uint32
    assert man.placeholders.tolist() == [1, 2, 1, 1] and man.limits.tolist() == [1, 2, 1, 1]
    assert man.offsets.tolist() == [0, 3, 9, 11]
    assert man.real_index.tolist() == [0, 1, 3, 4, 5, 6, 9, 11, 12]
    # a style is the sub-manifest of the listed contests
    st = man.style([1, 2])
    assert st == ElectionManifest([(4, 2), (1, 1)]) and st.nsel == 8 and st.real_index.tolist() == [0, 1, 2, 3, 6]
    # the uniform Manifest answers the same questions
    u = Manifest(2, 3, 2)
    assert u.offsets.tolist() == [0, 5] and u.real_index.tolist() == [0, 1, 2, 5, 6, 7]
    assert u.contests == (Contest(3, 2), Contest(3, 2)) and u.max_votes_allowed == 2
    assert ElectionManifest(u.contests).real_index.tolist() == u.real_index.tolist()
    with pytest.raises(ValueError):
        ElectionManifest([])


def test_random_votes_fill_each_contest_to_its_limit():
    from electionguard.ballot import ElectionManifest, random_votes
    man = ElectionManifest(M)
    v = random_votes(np.random.default_rng(3), man, 40)
    assert v.shape == (40, 14) and v.dtype == np.uint8 and v.max() == 1
    seen = set()
    for o, c in zip(man.offsets, man.contests):
        blk = v[:, o:o + c.spc]
        assert (blk.sum(axis=1) == c.votes_allowed).all()
        seen |= set(blk[:, :c.n_selections].sum(axis=1).tolist())
    assert seen == {0, 1, 2}


def test_formats_round_trips_the_pair_list_manifest():
    from electionguard.ballot import ElectionManifest, Manifest
    from electionguard.formats import manifest_field, record_arrays, record_manifest
    man = ElectionManifest(M)
    field = manifest_field(man)
    assert field == [[2, 1], [4, 2], [1, 1], [2, 1]]
    assert record_manifest({"manifest": field}) == man
    assert record_manifest({"manifest": [4, 5, 1]}) == Manifest(4, 5, 1)     # the three-integer form
    assert manifest_field(Manifest(4, 5, 1)) == [4, 5, 1]
    bal = {"cts": [[f"{i:02x}", f"{i + 100:02x}"] for i in range(14)],
           "rproofs": [[f"{i:02x}"] * 4 for i in range(14)], "cproofs": [[f"{k:02x}"] * 2 for k in range(4)]}
    (cts, rp, cp), shares = record_arrays({"manifest": field, "ballots": [bal, bal]})
    assert shares is None and cts.shape == (2, 14, 2, 512) and rp.shape == (2, 14, 4, 32) and cp.shape == (2, 4, 2, 32)
    assert cts[1, 13, 1, 511] == 113 and cts[1, 13, 1, :511].sum() == 0 and cp[0, 3, 1, 31] == 3


def test_spoiled_texts_take_the_real_selections():
    from electionguard.ballot import ElectionManifest, Manifest
    from electionguard.decrypt import spoiled_texts
    man = ElectionManifest(M)
    cts = np.random.default_rng(1).integers(0, 256, size=(3, 14, 2, 512), dtype=np.uint8)
    t = spoiled_texts(man, cts)
    assert t.shape == (3 * 9, 2, 512)
    assert np.array_equal(t.reshape(3, 9, 2, 512), cts[:, [0, 1, 3, 4, 5, 6, 9, 11, 12]])
    u = Manifest(2, 3, 2)
    cu = cts[:, :10]
    want = cu.reshape(3, 2, 5, 2, 512)[:, :, :3].reshape(18, 2, 512)
    assert np.array_equal(spoiled_texts(u, cu), want)
    assert np.array_equal(spoiled_texts(ElectionManifest(u.contests), cu), want)
