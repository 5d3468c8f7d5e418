"""ctypes binding of libeg_hip.so (the C ABI in include/eg_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc,
``--offload-arch=gfx950``) into ``electionguard-remote_amd/electionguard/lib/``.
There is deliberately NO CPU fallback: if the library (or a GPU) is missing,
every group operation raises :class:`NativeUnavailable`.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

LIB_DIR = Path(__file__).resolve().parent.parent / "lib"
LIB_PATH = LIB_DIR / "libeg_hip.so"

# Every symbol declared in include/eg_hip.h (tests check the library exports them).
EXPORTED = [
    "eg_last_error", "eg_version", "eg_ctx_create", "eg_ctx_destroy", "eg_ctx_sync",
    "eg_ctx_profile_begin", "eg_ctx_profile_end", "eg_ctx_profile_clock", "eg_ctx_g_table", "eg_ctx_set_hash_format",
    "eg_fixed_base_create", "eg_fixed_base_destroy", "eg_powp_batch", "eg_fb_pow_batch",
    "eg_powp_batch_dev", "eg_fb_pow_batch_dev",
    "eg_multp_batch", "eg_prod_reduce", "eg_multinv_batch", "eg_verify_ballots",
    "eg_set_election_key", "eg_verify_ballots_dev", "eg_encrypt_ballots", "eg_encrypt_ballots_dev",
    "eg_trustee_decrypt_batch", "eg_verify_shares", "eg_clock_median",
    "eg_ctx_set_coalescing", "eg_powp_submit", "eg_gpowp_submit", "eg_multp_submit", "eg_ticket_wait",
    "eg_powp_one", "eg_gpowp_one", "eg_multp_one", "eg_ctx_set_ct_encrypt",
    "eg_dev_alloc", "eg_dev_free", "eg_memcpy_htod", "eg_memcpy_dtoh", "eg_memset_dev", "eg_all_nonzero_dev",
    "eg_comm_unique_id", "eg_comm_init", "eg_comm_destroy", "eg_comm_all_valid", "eg_tally_allgather_fold",
    "eg_ctx_set_proof_format",
    "eg_mexp_submit", "eg_mexp_one", "eg_fb_pow_submit", "eg_fb_pow_one", "eg_ctx_set_ct_pow", "eg_comm_info",
]


# Every symbol declared in include/eg_hip_manifest.h (manifests of unequal contests).
EXPORTED_MANIFEST = [
    "eg_verify_ballots_manifest", "eg_verify_ballots_manifest_dev",
    "eg_encrypt_ballots_manifest", "eg_encrypt_ballots_manifest_dev",
]


# Every symbol declared in include/eg_hip_codes.h (ballot nonces, ballot hashes, code chain).
EXPORTED_CODES = [
    "eg_derive_ballot_nonces", "eg_derive_ballot_nonces_dev",
    "eg_ballot_hashes", "eg_ballot_hashes_dev",
    "eg_verify_code_chain", "eg_verify_code_chain_dev",
]


# Every symbol declared in include/eg_hip_contestdata.h (contest data under HashedElGamal).
EXPORTED_CONTEST_DATA = [
    "eg_derive_contest_data_nonces", "eg_derive_contest_data_nonces_dev",
    "eg_seal_contest_data", "eg_seal_contest_data_dev",
    "eg_open_contest_data", "eg_open_contest_data_dev",
]


# Every symbol declared in include/eg_hip_range.h (0..L range proofs of ciphertexts).
EXPORTED_RANGE = [
    "eg_range_prove", "eg_range_prove_dev",
    "eg_range_verify", "eg_range_verify_dev",
]


# Every symbol declared in include/eg_hip_preencrypt.h (pre-encrypted ballots).
EXPORTED_PREENCRYPT = [
    "eg_preencrypt_ballots", "eg_preencrypt_ballots_dev",
    "eg_preencrypt_record", "eg_preencrypt_record_dev",
    "eg_preencrypt_verify", "eg_preencrypt_verify_dev",
]


# Every symbol declared in include/eg_hip_ballot2.h (ballots without placeholder selections).
EXPORTED_BALLOT2 = [
    "eg_encrypt_ballots_v2", "eg_encrypt_ballots_v2_dev",
    "eg_verify_ballots_v2", "eg_verify_ballots_v2_dev",
]


# Every symbol declared in include/eg_hip_codes2.h (seeded nonces and opening of those ballots).
EXPORTED_CODES2 = [
    "eg_derive_ballot_nonces_v2", "eg_derive_ballot_nonces_v2_dev",
    "eg_open_ballots_v2", "eg_open_ballots_v2_dev",
]

# Every symbol declared in include/eg_hip_prodpow.h (products of powers over one shared exponent vector).
EXPORTED_PRODPOW = [
    "eg_prod_pow", "eg_prod_pow_dev", "eg_prod_pow_plan",
]

# Every symbol declared in include/eg_hip_decrypt2.h (threshold decryption with one combined proof per text).
EXPORTED_DECRYPT2 = [
    "eg_decrypt2_commit", "eg_decrypt2_respond",
    "eg_decrypt2_combine", "eg_decrypt2_combine_dev",
    "eg_decrypt2_check", "eg_decrypt2_check_dev",
    "eg_decrypt2_verify", "eg_decrypt2_verify_dev",
]

# Every symbol declared in include/eg_hip_shuffle.h (the verifiable shuffle: generators, mix, prover, verifier).
EXPORTED_SHUFFLE = [
    "eg_shuffle_generators", "eg_shuffle_generators_dev",
    "eg_shuffle_mix", "eg_shuffle_mix_dev",
    "eg_shuffle_prove", "eg_shuffle_prove_dev",
    "eg_shuffle_verify", "eg_shuffle_verify_dev",
]

# Every symbol declared in include/eg_hip_decode.h (decoding decrypted texts: batch inverse and dLog on the device).
EXPORTED_DECODE = [
    "eg_batch_inverse", "eg_batch_inverse_dev",
    "eg_decode_table_create", "eg_decode_table_destroy",
    "eg_decode_counts", "eg_decode_counts_dev",
    "eg_decode_plan",
]


class NativeUnavailable(RuntimeError):
    pass


class EgError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed (status {code}): {msg}")
        self.code = code


_lib: Optional[ctypes.CDLL] = None

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_vp = ctypes.c_void_p
c_sz = ctypes.c_size_t


def _sig(lib: ctypes.CDLL) -> None:
    I = ctypes.c_int
    P = c_vp
    S = c_sz
    U32 = ctypes.c_uint32
    D = ctypes.POINTER(ctypes.c_double)
    U32P = ctypes.POINTER(U32)
    sigs = {
        "eg_last_error": ([], ctypes.c_char_p),
        "eg_version": ([ctypes.c_char_p, S], I),
        "eg_ctx_create": ([P, P, P, I, ctypes.POINTER(c_vp)], I),
        "eg_ctx_destroy": ([P], I),
        "eg_ctx_sync": ([P], I),
        "eg_ctx_profile_begin": ([P], I),
        "eg_ctx_profile_end": ([P, D, D, D, ctypes.POINTER(I)], I),
        "eg_ctx_profile_clock": ([P, D, ctypes.POINTER(U32), ctypes.POINTER(U32)], I),
        "eg_clock_median": ([P, S, D, ctypes.POINTER(U32), ctypes.POINTER(U32)], I),
        "eg_ctx_g_table": ([P], P),
        "eg_ctx_set_hash_format": ([P, I], I),
        "eg_ctx_set_proof_format": ([P, I, I], I),
        "eg_fixed_base_create": ([P, P, I, ctypes.POINTER(c_vp)], I),
        "eg_fixed_base_destroy": ([P], I),
        "eg_multp_batch": ([P, P, P, P, S], I),
        "eg_prod_reduce": ([P, P, S, S, P], I),
        "eg_multinv_batch": ([P, P, P, S], I),
        "eg_set_election_key": ([P, P, I], I),
        "eg_ctx_set_ct_encrypt": ([P, I], I),
        "eg_ctx_set_coalescing": ([P, S, U32], I),
        "eg_powp_submit": ([P, P, P, P, ctypes.POINTER(c_vp)], I),
        "eg_gpowp_submit": ([P, P, P, ctypes.POINTER(c_vp)], I),
        "eg_multp_submit": ([P, P, P, P, ctypes.POINTER(c_vp)], I),
        "eg_ticket_wait": ([P], I),
        "eg_powp_one": ([P, P, P, P], I),
        "eg_gpowp_one": ([P, P, P], I),
        "eg_multp_one": ([P, P, P, P], I),
        "eg_trustee_decrypt_batch": ([P, P, P, P, P, S, P, P], I),
        "eg_verify_shares": ([P, P, P, P, P, P, S, P], I),
        "eg_dev_alloc": ([P, S, ctypes.POINTER(c_vp)], I),
        "eg_dev_free": ([P, P], I),
        "eg_memcpy_htod": ([P, P, P, S], I),
        "eg_memcpy_dtoh": ([P, P, P, S], I),
        "eg_memset_dev": ([P, P, I, S], I),
        "eg_all_nonzero_dev": ([P, P, S, ctypes.POINTER(I)], I),
        "eg_comm_unique_id": ([P], I),
        "eg_comm_init": ([P, P, I, I], I),
        "eg_comm_destroy": ([P], I),
        "eg_comm_all_valid": ([P, I, ctypes.POINTER(I)], I),
        "eg_tally_allgather_fold": ([P, P, S, S, I, P], I),
        "eg_comm_info": ([P, ctypes.POINTER(I), ctypes.POINTER(I)], I),
        "eg_mexp_submit": ([P, P, S, P, P, P, P, P, P, ctypes.POINTER(c_vp)], I),
        "eg_mexp_one": ([P, P, S, P, P, P, P, P, P], I),
        "eg_fb_pow_submit": ([P, P, P, ctypes.POINTER(c_vp)], I),
        "eg_fb_pow_one": ([P, P, P], I),
        "eg_ctx_set_ct_pow": ([P, I], I),
        "eg_prod_pow_plan": ([S, S, I, I, ctypes.POINTER(I), ctypes.POINTER(I), D], I),
        "eg_decrypt2_commit": ([P, P, P, P, S, P, P, P], I),
        "eg_decrypt2_respond": ([P, P, P, P, S, P], I),
        "eg_decode_table_create": ([P, ctypes.c_uint64, I, ctypes.POINTER(c_vp)], I),
        "eg_decode_table_destroy": ([P], I),
        "eg_decode_plan": ([S, ctypes.c_uint64, U32P, U32P, U32P, U32P, U32P, D, D, D], I),
    }
    # declared once, bound twice: name takes host pointers, name_dev device pointers
    pairs = {
        "eg_powp_batch": ([P, P, P, P, S], I),
        "eg_fb_pow_batch": ([P, P, P, S], I),
        "eg_verify_ballots": ([P, P, P, S, S, S, S, U32, P, P, P, P, P, P, P], I),
        "eg_encrypt_ballots": ([P, P, P, S, S, S, P, P, P, P, P, P], I),
        "eg_verify_ballots_manifest": ([P, P, P, S, S, U32P, U32P, U32P, P, P, P, P, P, P, P], I),
        "eg_encrypt_ballots_manifest": ([P, P, P, S, S, U32P, P, P, P, P, P, P], I),
        "eg_derive_ballot_nonces": ([P, S, S, U32P, P, P, P], I),
        "eg_ballot_hashes": ([P, S, S, U32P, P, P, P, P, P, P, P, P], I),
        "eg_verify_code_chain": ([P, S, P, P, P, P, P], I),
        "eg_derive_contest_data_nonces": ([P, S, S, P, P], I),
        "eg_seal_contest_data": ([P, P, S, S, S, P, P, P, P, P, P], I),
        "eg_open_contest_data": ([P, S, S, S, P, P, P, P, P, P, P], I),
        "eg_range_prove": ([P, P, P, S, U32, P, P, P, P, P], I),
        "eg_range_verify": ([P, P, P, S, U32, P, P, P], I),
        "eg_preencrypt_ballots": ([P, P, S, S, P, U32] + [P] * 11, I),
        "eg_preencrypt_record": ([P, P, S, S, P, P, U32] + [P] * 10, I),
        "eg_preencrypt_verify": ([P, S, S, P, P, U32] + [P] * 11, I),
        "eg_encrypt_ballots_v2": ([P, P, P, S, S, U32P, U32P, U32P] + [P] * 6, I),
        "eg_verify_ballots_v2": ([P, P, P, S, S, U32P, U32P, U32P] + [P] * 7, I),
        "eg_derive_ballot_nonces_v2": ([P, S, S, U32P, U32P, U32P, P, P, P], I),
        "eg_open_ballots_v2": ([P, P, S, S, U32P, U32P, U32P, P, P, P, P], I),
        "eg_prod_pow": ([P, P, S, S, P, S, S, I, I, P], I),
        "eg_decrypt2_combine": ([P, P, P, S, S, P, P, P, P, P, P, P], I),
        "eg_decrypt2_check": ([P, S, S, P, P, P, P, P, P, P, P], I),
        "eg_decrypt2_verify": ([P, P, P, S, P, P, P, P], I),
        "eg_shuffle_generators": ([P, P, P, S, P], I),
        "eg_shuffle_mix": ([P, P, S, S, P, P, P, P], I),
        "eg_shuffle_prove": ([P, P, P, P, S, S] + [P] * 12, I),
        "eg_shuffle_verify": ([P, P, P, P, S, S] + [P] * 9 + [I, P, P], I),
        "eg_batch_inverse": ([P, P, P, S], I),
        "eg_decode_counts": ([P, P, P, S, P], I),
    }
    sigs.update({name + dev: sig for name, sig in pairs.items() for dev in ("", "_dev")})
    for name, (args, res) in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res


def load(path: Optional[os.PathLike] = None) -> ctypes.CDLL:
    """Load libeg_hip.so (no GPU needed to load; compute calls need one)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("EG_LIB"):
        path = os.environ["EG_LIB"]  # A/B builds (tools/ab_mm.py); production uses the in-tree default
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise NativeUnavailable(
            f"{p} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP extension is required; there is no CPU fallback)")
    lib = ctypes.CDLL(str(p))
    _sig(lib)
    if path is None:
        _lib = lib
    return lib


def check(lib: ctypes.CDLL, fn: str, rc: int) -> None:
    if rc != 0:
        raise EgError(fn, rc, lib.eg_last_error().decode(errors="replace"))


def buf(b: bytes | bytearray | memoryview):
    """Pointer to the bytes of b (kept alive by the caller)."""
    if isinstance(b, (bytes,)):
        return ctypes.cast(ctypes.c_char_p(b), c_vp)
    arr = (ctypes.c_uint8 * len(b)).from_buffer(b)
    return ctypes.cast(arr, c_vp)


def out_buf(n: int) -> bytearray:
    return bytearray(max(n, 1))


def version() -> str:
    """Build string of the loaded library, e.g. 'eg_hip gfx950 radix2^29 limbs=144 ...'."""
    lib = load()
    b = ctypes.create_string_buffer(160)
    check(lib, "eg_version", lib.eg_version(b, len(b)))
    return b.value.decode()


def lib_path() -> Path:
    """Path of the library load() uses (EG_LIB override or the in-tree build)."""
    return Path(os.environ["EG_LIB"]) if os.environ.get("EG_LIB") else LIB_PATH
