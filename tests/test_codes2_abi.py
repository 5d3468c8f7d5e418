"""CPU: the C ABI of the seeded nonces and the opening of placeholder-free ballots
(include/eg_hip_codes2.h): the header declares exactly the four entry points,
native.EXPORTED_CODES2 lists them and nothing another list holds, the built library exports them,
each rejects a null context without touching a device, and the build's source list names the
header and the includes in their order."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_codes2.h"

FOUR = ["eg_derive_ballot_nonces_v2", "eg_derive_ballot_nonces_v2_dev", "eg_open_ballots_v2", "eg_open_ballots_v2_dev"]


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def test_header_declares_exactly_the_four_entry_points():
    assert header_functions() == FOUR
    text = HEADER.read_text()
    assert '#include "eg_hip_ballot2.h"' in text     # the manifest and the row layouts are ballot2's
    for word in ("sn_off", "cn_off", "eg_ctx_set_ct_pow", "2^16", "Q 5", "Q 6", "eg_ballot_hashes"):
        assert word in text, word


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_CODES2) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES) | \
        set(native.EXPORTED_CONTEST_DATA) | set(native.EXPORTED_RANGE) | set(native.EXPORTED_PREENCRYPT) | \
        set(native.EXPORTED_BALLOT2)
    assert not set(native.EXPORTED_CODES2) & others
    for name in FOUR:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == (9 if "derive" in name else 11), name


def test_null_ctx_is_an_argument_error(lib):
    one = (ctypes.c_uint32 * 1)(1)
    for name in FOUR:
        head = (0, 1, one, one, one) if "derive" in name else (bytes(512), 0, 1, one, one, one)
        n = 3 if "derive" in name else 4
        assert getattr(lib, name)(None, *head, *[None] * n) == 1, name
        assert b"ballot2" in lib.eg_last_error() and b"null" in lib.eg_last_error()


def test_the_source_list_of_the_build_names_the_header_and_the_includes():
    src = (ROOT / "__graft_entry__.py").read_text()
    assert '"eg_hip_codes2.h"' in src
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert capi.index('#include "eg_capi_ballot2.inc"') < capi.index('#include "eg_capi_codes2.inc"')
    assert capi.index('#include "eg_capi_contestdata.inc"') < capi.index('#include "eg_capi_codes2.inc"')
    assert '#include "eg_codes2.hpp"' in capi
