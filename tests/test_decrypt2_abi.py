"""CPU: the C ABI of the threshold decryption with one combined proof per text
(include/eg_hip_decrypt2.h): the header declares exactly the eight entry points,
native.EXPORTED_DECRYPT2 lists them and nothing another list holds, the built library exports
them, and every refusal of the header is an argument error naming decrypt2 before the context is
read: a pointer that is merely not NULL stands in for it."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "eg_hip_decrypt2.h"

EIGHT = sorted(["eg_decrypt2_commit", "eg_decrypt2_respond", "eg_decrypt2_combine", "eg_decrypt2_combine_dev",
                "eg_decrypt2_check", "eg_decrypt2_check_dev", "eg_decrypt2_verify", "eg_decrypt2_verify_dev"])
NARGS = {"commit": 8, "respond": 6, "combine": 12, "check": 11, "verify": 8}
EG_ERR_ARG = 1
CTX = ctypes.c_void_p(0x1000)
BUF = ctypes.c_void_p(0x2000)
ODD = ctypes.c_void_p(0x2008)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build_hip()
    from electionguard.core import native
    return native.load()


def refused(lib, rc):
    return rc == EG_ERR_ARG and b"decrypt2" in lib.eg_last_error()


def test_header_declares_exactly_the_eight_entry_points():
    assert header_functions() == EIGHT
    text = HEADER.read_text()
    assert '#include "eg_hip.h"' in text
    for word in ("EG_DECRYPT2_MAX_GUARDIANS 64", "EG_DECRYPT2_CHUNK_JOBS", "EG_DECRYPT2_CHUNK_JOBS / (4 * k)",
                 "0x30", "eg_ctx_set_proof_format does NOT apply", "eg_ctx_set_hash_format", "constant time",
                 "text-major", "16-byte aligned", "ONCE"):
        assert word in text, word


def test_library_exports_and_native_list(lib):
    from electionguard.core import native
    assert sorted(native.EXPORTED_DECRYPT2) == header_functions()
    others = set(native.EXPORTED) | set(native.EXPORTED_MANIFEST) | set(native.EXPORTED_CODES) | \
        set(native.EXPORTED_CONTEST_DATA) | set(native.EXPORTED_RANGE) | set(native.EXPORTED_PREENCRYPT) | \
        set(native.EXPORTED_BALLOT2) | set(native.EXPORTED_CODES2) | set(native.EXPORTED_PRODPOW)
    assert not set(native.EXPORTED_DECRYPT2) & others
    for name in EIGHT:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == NARGS[name.split("_")[2]], name


def test_the_python_constants_are_the_headers():
    from electionguard import decrypt2 as D
    text = HEADER.read_text()
    assert re.search(r"#define EG_DECRYPT2_CHUNK_JOBS \(\(size_t\)1 << 16\)", text) and D.CHUNK_JOBS == 1 << 16
    assert re.search(r"#define EG_DECRYPT2_MAX_ITEMS \(\(size_t\)1 << 24\)", text) and D.MAX_ITEMS == 1 << 24
    assert D.MAX_GUARDIANS == 64 and D.TAG == 0x30
    assert [D.chunk_texts(k) for k in (1, 2, 3, 64)] == [16384, 8192, 5461, 256]


def test_the_build_names_the_header_and_the_include():
    assert '"eg_hip_decrypt2.h"' in (ROOT / "__graft_entry__.py").read_text()
    capi = (ROOT / "electionguard-remote_amd" / "csrc" / "eg_capi.hip").read_text()
    assert '#include "eg_decrypt2.hpp"' in capi
    assert re.search(r'#include "eg_capi_prodpow.inc"\s*\n#include "eg_capi_decrypt2.inc"', capi)
    assert re.search(r"W_PP_ACC,\s*(//[^\n]*\n\s*)*W_D2_", capi), "the new workspace slots follow the W_PP_ slots"


# ---- the calls, with BUF for every pointer unless told otherwise ----------------------------------
def commit(lib, ctx=CTX, secret=BUF, n=1, data=BUF):
    return lib.eg_decrypt2_commit(ctx, secret, data, BUF, n, BUF, BUF, BUF)


def respond(lib, ctx=CTX, secret=BUF, n=1, data=BUF):
    return lib.eg_decrypt2_respond(ctx, secret, BUF, data, n, BUF)


def combine(lib, dev, ctx=CTX, K=BUF, qbar=BUF, n=1, k=1, w=BUF, ptrs=None):
    fn = lib.eg_decrypt2_combine_dev if dev else lib.eg_decrypt2_combine
    return fn(ctx, K, qbar, n, k, w, *(ptrs or [BUF] * 6))


def check(lib, dev, ctx=CTX, n=1, k=1, Z=BUF, ptrs=None):
    fn = lib.eg_decrypt2_check_dev if dev else lib.eg_decrypt2_check
    return fn(ctx, n, k, Z, *(ptrs or [BUF] * 7))


def verify(lib, dev, ctx=CTX, K=BUF, qbar=BUF, n=1, ptrs=None):
    fn = lib.eg_decrypt2_verify_dev if dev else lib.eg_decrypt2_verify
    return fn(ctx, K, qbar, n, *(ptrs or [BUF] * 4))


def swap(count, at, value):
    return [value if j == at else BUF for j in range(count)]


def test_null_arguments_of_the_trustee_calls(lib):
    assert refused(lib, commit(lib, ctx=None)) and b"null" in lib.eg_last_error()
    assert refused(lib, commit(lib, secret=None))
    assert refused(lib, commit(lib, data=None))
    assert refused(lib, lib.eg_decrypt2_commit(CTX, BUF, BUF, None, 1, BUF, BUF, BUF))
    for at in range(3):
        assert refused(lib, lib.eg_decrypt2_commit(CTX, BUF, BUF, BUF, 1, *swap(3, at, None)))
    assert refused(lib, respond(lib, ctx=None)) and refused(lib, respond(lib, secret=None))
    assert refused(lib, respond(lib, data=None))
    assert refused(lib, lib.eg_decrypt2_respond(CTX, BUF, None, BUF, 1, BUF))
    assert refused(lib, lib.eg_decrypt2_respond(CTX, BUF, BUF, BUF, 1, None))
    assert refused(lib, commit(lib, n=(1 << 24) + 1)) and refused(lib, respond(lib, n=(1 << 24) + 1))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_null_arguments_of_the_pairs(lib, dev):
    assert refused(lib, combine(lib, dev, ctx=None)) and b"null" in lib.eg_last_error()
    for kw in ({"K": None}, {"qbar": None}, {"w": None}):
        assert refused(lib, combine(lib, dev, **kw)), kw
    for at in range(6):
        assert refused(lib, combine(lib, dev, ptrs=swap(6, at, None))), at
    assert refused(lib, check(lib, dev, ctx=None)) and refused(lib, check(lib, dev, Z=None))
    for at in range(7):
        assert refused(lib, check(lib, dev, ptrs=swap(7, at, None))), at
    assert refused(lib, verify(lib, dev, ctx=None))
    assert refused(lib, verify(lib, dev, K=None)) and refused(lib, verify(lib, dev, qbar=None))
    for at in range(4):
        assert refused(lib, verify(lib, dev, ptrs=swap(4, at, None))), at


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_every_limit_is_refused(lib, dev):
    for call in (combine, check):
        assert refused(lib, call(lib, dev, k=0)) and b"k == 0" in lib.eg_last_error()
        assert refused(lib, call(lib, dev, k=65)) and b"64" in lib.eg_last_error()
        assert refused(lib, call(lib, dev, n=(1 << 24) // 3 + 1, k=3)) and b"2^24" in lib.eg_last_error()
        assert refused(lib, call(lib, dev, n=(1 << 18) + 1, k=64))
        assert refused(lib, call(lib, dev, n=0, k=0))          # the guardian count is checked whatever n is
    assert refused(lib, verify(lib, dev, n=(1 << 24) + 1))


def test_n_zero_is_ok_and_touches_nothing(lib):
    assert commit(lib, n=0, data=None) == 0 and respond(lib, n=0, data=None) == 0
    for dev in (False, True):
        assert combine(lib, dev, n=0, k=3, ptrs=[None] * 6) == 0
        assert check(lib, dev, n=0, k=3, ptrs=[None] * 7) == 0
        assert verify(lib, dev, n=0, ptrs=[None] * 4) == 0


def test_a_misaligned_device_pointer_to_rows_is_refused(lib):
    for at in range(6):
        assert refused(lib, combine(lib, True, ptrs=swap(6, at, ODD))), at
        assert b"aligned" in lib.eg_last_error()
    for at in (0, 1, 2, 3, 4, 6):                               # ok (index 5) holds single bytes
        assert refused(lib, check(lib, True, ptrs=swap(7, at, ODD))), at
    for at in (0, 1, 2):                                        # ok (index 3) holds single bytes
        assert refused(lib, verify(lib, True, ptrs=swap(4, at, ODD))), at
