"""Ballot nonces from one per-ballot seed, ballot hashes and confirmation (tracking) codes.

What batchEncryption (RunRemoteWorkflowTest.java:140-141) produces besides ciphertexts and
proofs: every nonce of a ballot comes from one 32-byte ballot nonce xi_b (so a challenged ballot
is opened from xi_b alone, without trustees), each ballot has a hash, and the hashes are chained
into the confirmation codes a voter sees and the verifier checks ("ballot chaining").

With H = core.hashing.hash_elems (no Q-bar prefix), "Q" elements 32 bytes as given, s the
position of a selection in its ballot and k the contest index (include/eg_hip_codes.h):

  N_sel(xi_b, s, t) = H(Q xi_b, Q 1, Q 4s+t)     t = 0..3: R, u, c_fake, v_fake
  N_con(xi_b, k)    = H(Q xi_b, Q 2, Q k)
  h_sel[b,s] = H(Q dsel[s], P alpha, P beta)
  h_con[b,k] = H(Q dcon[k], Q h_sel[b,off_k], ..., Q h_sel[b,off_k+spc_k-1])
  B[b]       = H(Q ballot_id[b], Q manifest_hash, Q h_con[b,0], ..., Q h_con[b,nc-1])
  code[b]    = H(Q code[b-1], Q ts[b], Q B[b]),  code[-1] = seed

The pre-image formats are the project's own (the upstream one is unpinned).  The
``*_host`` functions restate the definitions on the host; derive_nonces, ballot_hashes and
verify_code_chain run them on the GPU (csrc/eg_codes.hpp), on numpy arrays or DeviceBuffers.
Building the chain is sequential, one short hash per ballot: chain_codes, on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple, Union

import numpy as np

from .ballot import AnyManifest, ElectionKey, EncryptedBallots, batch_encryption_device
from .core.group import FixedBase, GroupContext
from .core.hashing import hash_elems
from .core.marshal import Columns, be32_row as _b32, be_int as _i, q_row, rows32, u32p

Q32 = Union[int, bytes, bytearray, np.ndarray]


@dataclass
class ManifestHashes:
    """The manifest's description hashes: dsel (nsel, 32), dcon (nc, 32), manifest_hash (32,)."""
    dsel: np.ndarray
    dcon: np.ndarray
    manifest_hash: np.ndarray


# ---------------------------------------------------------------------------------------------
# small conversions
# ---------------------------------------------------------------------------------------------
def timestamp_elements(seconds: Sequence[int]) -> np.ndarray:
    """Integer seconds -> the (nb, 32) big-endian ts elements of the code chain."""
    return np.frombuffer(b"".join(int(t).to_bytes(32, "big") for t in seconds), np.uint8).reshape(-1, 32)


def _ts_elements(timestamps) -> np.ndarray:
    a = np.asarray(timestamps)
    if a.dtype != np.uint8 or a.ndim != 2:
        a = timestamp_elements([int(t) for t in a.reshape(-1)])
    return a


def _ts_rows(timestamps, nb: int) -> np.ndarray:
    return rows32(_ts_elements(timestamps), nb, "timestamps")


def _hashes_rows(man: AnyManifest, hashes: ManifestHashes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    return (rows32(hashes.dsel, man.nsel, "dsel"), rows32(hashes.dcon, man.n_contests, "dcon"),
            q_row(hashes.manifest_hash))


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions
# ---------------------------------------------------------------------------------------------
def derive_nonces_host(q: int, man: AnyManifest, ballot_nonces, fmt: str = "fixed") -> Tuple[np.ndarray, np.ndarray]:
    """-> sel_nonces (nb, nsel, 4, 32), contest_nonces (nb, nc, 32): batch_encryption's inputs."""
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    nb, nsel, nc = len(bn), man.nsel, man.n_contests
    sn = np.empty((nb, nsel, 4, 32), np.uint8)
    cn = np.empty((nb, nc, 32), np.uint8)
    for b in range(nb):
        xi = _i(bn[b])
        for r in range(nsel * 4):
            sn[b, r // 4, r % 4] = _b32(hash_elems(q, ("Q", xi), ("Q", 1), ("Q", r), fmt=fmt))
        for k in range(nc):
            cn[b, k] = _b32(hash_elems(q, ("Q", xi), ("Q", 2), ("Q", k), fmt=fmt))
    return sn, cn


def ballot_hashes_host(q: int, man: AnyManifest, hashes: ManifestHashes, ballot_ids, cts,
                       fmt: str = "fixed") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> B (nb, 32), h_sel (nb, nsel, 32), h_con (nb, nc, 32)."""
    nsel, nc = man.nsel, man.n_contests
    cts = np.ascontiguousarray(cts, dtype=np.uint8).reshape(-1, nsel, 2, 512)
    nb = len(cts)
    ids = rows32(ballot_ids, nb, "ballot_ids")
    dsel, dcon, mh = _hashes_rows(man, hashes)
    B = np.empty((nb, 32), np.uint8)
    hs = np.empty((nb, nsel, 32), np.uint8)
    hc = np.empty((nb, nc, 32), np.uint8)
    for b in range(nb):
        for s in range(nsel):
            hs[b, s] = _b32(hash_elems(q, ("Q", _i(dsel[s])), ("P", _i(cts[b, s, 0])), ("P", _i(cts[b, s, 1])),
                                       fmt=fmt))
        for k, (off, n) in enumerate(zip(man.offsets, man.spc_list)):
            run = [("Q", _i(hs[b, int(off) + s])) for s in range(int(n))]
            hc[b, k] = _b32(hash_elems(q, ("Q", _i(dcon[k])), *run, fmt=fmt))
        B[b] = _b32(hash_elems(q, ("Q", _i(ids[b])), ("Q", _i(mh)), *[("Q", _i(hc[b, k])) for k in range(nc)],
                               fmt=fmt))
    return B, hs, hc


def chain_codes(q: int, seed: Q32, timestamps, ballot_hashes, fmt: str = "fixed") -> np.ndarray:
    """The confirmation codes (nb, 32) of ballots in order: code[b] = H(code[b-1], ts[b], B[b])."""
    B = np.ascontiguousarray(ballot_hashes, dtype=np.uint8).reshape(-1, 32)
    ts = _ts_rows(timestamps, len(B))
    codes = np.empty((len(B), 32), np.uint8)
    prev = _i(q_row(seed))
    for b in range(len(B)):
        prev = hash_elems(q, ("Q", prev), ("Q", _i(ts[b])), ("Q", _i(B[b])), fmt=fmt)
        codes[b] = _b32(prev)
    return codes


def verify_code_chain_host(q: int, seed: Q32, timestamps, ballot_hashes, codes, fmt: str = "fixed") -> np.ndarray:
    """-> ok (nb,) bool: codes[b] == H(codes[b-1] or seed, ts[b], B[b]) with the RECORDED codes[b-1]."""
    B = np.ascontiguousarray(ballot_hashes, dtype=np.uint8).reshape(-1, 32)
    nb = len(B)
    ts, cd = _ts_rows(timestamps, nb), rows32(codes, nb, "codes")
    ok = np.zeros(nb, bool)
    for b in range(nb):
        prev = _i(cd[b - 1]) if b else _i(q_row(seed))
        ok[b] = bytes(cd[b]) == bytes(_b32(hash_elems(q, ("Q", prev), ("Q", _i(ts[b])), ("Q", _i(B[b])), fmt=fmt)))
    return ok


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def derive_nonces(group: GroupContext, man: AnyManifest, ballot_nonces):
    """-> (sel_nonces (nb, nsel, 4, 32), contest_nonces (nb, nc, 32)) of the ballot nonces (nb, 32);
    DeviceBuffers in, DeviceBuffers out (asynchronous on the context's stream)."""
    cols = Columns(group)
    bn = cols.item(ballot_nonces, (32,), "ballot_nonces")
    sn, cn = cols.out((man.nsel, 4, 32)), cols.out((man.n_contests, 32))
    return tuple(cols.call("eg_derive_ballot_nonces", cols.n, man.n_contests, u32p(man.spc_list), bn, sn, cn))


def ballot_hashes(group: GroupContext, man: AnyManifest, hashes: ManifestHashes, ballot_ids, cts, parts: bool = False):
    """-> B (nb, 32), or (B, h_sel (nb, nsel, 32), h_con (nb, nc, 32)) with parts.  With cts and
    ballot_ids DeviceBuffers the ciphertexts are hashed where they lie and the results are
    DeviceBuffers (asynchronous on the context's stream)."""
    nsel, nc = man.nsel, man.n_contests
    cols = Columns(group)
    dsel, dcon, mh = map(cols.once, _hashes_rows(man, hashes))
    cts = cols.item(cts, (nsel, 2, 512), "cts")
    ids = cols.item(ballot_ids, (32,), "ballot_ids")
    B, hs, hc = cols.out((32,)), cols.out((nsel, 32), want=parts), cols.out((nc, 32), want=parts)
    out = cols.call("eg_ballot_hashes", cols.n, nc, u32p(man.spc_list), dsel, dcon, mh, ids, cts, B, hs, hc)
    return tuple(out) if parts else out[0]


def verify_code_chain(group: GroupContext, seed: Q32, timestamps, ballot_hashes, codes):
    """-> ok (nb,) bool: every link of the chain recomputed from the recorded previous code.  With
    DeviceBuffers for all four (seed too) -> a DeviceBuffer of nb flag bytes, asynchronous."""
    cols = Columns(group)
    B = cols.item(ballot_hashes, (32,), "ballot_hashes")
    ts = cols.item(timestamps, (32,), "timestamps", host=_ts_elements)
    cd = cols.item(codes, (32,), "codes")
    sd = cols.given(seed, "seed")
    return cols.call("eg_verify_code_chain", cols.n, sd, ts, B, cd, cols.out((), flag=True))[0]


# ---------------------------------------------------------------------------------------------
# encryption from ballot nonces, and opening a challenged ballot
# ---------------------------------------------------------------------------------------------
def encrypt_ballots_seeded(group: GroupContext, key: ElectionKey, qbar: int, man: AnyManifest,
                           hashes: ManifestHashes, votes, ballot_nonces, ballot_ids, timestamps,
                           seed: Q32) -> Tuple[EncryptedBallots, np.ndarray, np.ndarray]:
    """Encrypt nb ballots from their ballot nonces -> (EncryptedBallots, ballot_hashes (nb, 32),
    codes (nb, 32)).  Only the ballot nonces go up: the selection and contest nonces are derived in
    HBM and handed to the device encryptor, and the hashes are taken from the ciphertexts still
    there; the ciphertexts, proofs and B come back, and the chain is built on the host."""
    nsel, nc = man.nsel, man.n_contests
    votes = np.ascontiguousarray(votes, dtype=np.uint8).reshape(-1, nsel)
    nb = len(votes)
    bn = rows32(ballot_nonces, nb, "ballot_nonces")
    ids = rows32(ballot_ids, nb, "ballot_ids")
    if not nb:
        eb = EncryptedBallots(np.empty((0, nsel, 2, 512), np.uint8), np.empty((0, nsel, 4, 32), np.uint8),
                              np.empty((0, nc, 2, 32), np.uint8))
        return eb, np.empty((0, 32), np.uint8), np.empty((0, 32), np.uint8)
    d_sn, d_cn = derive_nonces(group, man, group.to_device(bn))
    d_votes = group.to_device(votes)
    d_cts = group.device_empty((nb, nsel, 2, 512))
    d_rp, d_cp = group.device_empty((nb, nsel, 4, 32)), group.device_empty((nb, nc, 2, 32))
    batch_encryption_device(group, key, qbar, man, nb, d_votes.ptr, d_sn.ptr, d_cn.ptr, d_cts.ptr, d_rp.ptr, d_cp.ptr)
    d_B = ballot_hashes(group, man, hashes, group.to_device(ids), d_cts)
    eb = EncryptedBallots(d_cts.download(), d_rp.download(), d_cp.download())
    B = d_B.download()
    return eb, B, chain_codes(group.q, seed, timestamps, B, fmt=group.hash_format)


def open_ballots(group: GroupContext, key: ElectionKey, man: AnyManifest, eb: EncryptedBallots,
                 ballot_nonces) -> Tuple[np.ndarray, np.ndarray]:
    """Open ballots from their ballot nonces, without trustees -> (votes (nb, nsel) uint8, ok
    (nb, nsel) bool).  Every R is re-derived on the device; a selection is ok when alpha = g^R and
    beta (K^R)^-1 is 1 (vote 0) or g (vote 1).  votes is 0 where ok is False."""
    nsel = man.nsel
    cts = np.ascontiguousarray(eb.cts, dtype=np.uint8).reshape(-1, nsel, 2, 512)
    nb = len(cts)
    bn = rows32(ballot_nonces, nb, "ballot_nonces")
    if not nb:
        return np.zeros((0, nsel), np.uint8), np.zeros((0, nsel), bool)
    sn, _ = derive_nonces(group, man, bn)
    R = np.ascontiguousarray(sn[:, :, 0]).reshape(-1, 32)
    alpha = np.ascontiguousarray(cts[:, :, 0]).reshape(-1, 512)
    beta = np.ascontiguousarray(cts[:, :, 1]).reshape(-1, 512)
    ktab = FixedBase(group, key.K, key.window_bits)
    try:
        KR = ktab.pow_batch(R)
    finally:
        ktab.close()
    m = group.multP_batch(beta, group.multInv_batch(KR))
    one = np.zeros(512, np.uint8)
    one[511] = 1
    g = np.frombuffer(group._g_be, np.uint8)
    is0, is1 = (m == one).all(axis=1), (m == g).all(axis=1)
    ok = (group.gPowP_batch(R) == alpha).all(axis=1) & (is0 | is1)
    return (is1 & ok).astype(np.uint8).reshape(nb, nsel), ok.reshape(nb, nsel)
