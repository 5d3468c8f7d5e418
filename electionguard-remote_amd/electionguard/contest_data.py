"""A contest's write-in names and overvote / undervote status, encrypted with the ballot.

Upstream keeps them in ``EncryptedBallot.Contest.contestData``, a HashedElGamalCiphertext
(c0, c1, c2, numBytes; common.proto) that batchEncryption writes for every contest of every ballot,
padded to a fixed length, and that decryptBallot opens through the trustees.  Here an item is one
(ballot b, contest k) pair in ballot-major order and every item of a call has the same padded
length nbytes <= MAX_BYTES (include/eg_hip_contestdata.h):

  r[b,k]  = H(Q xi_b, Q 3, Q k)                      core.hashing.hash_elems, mod q
  c0      = g^r,  kappa = K^r
  label   = ballot_id[b] || be32(k)
  kk      = SHA256(c0 || kappa)
  block j = HMAC(kk, 0x01 || "contest" || label || be32(j))
  mk      = HMAC(kk, 0x02 || "contest" || label)
  c1      = data XOR stream,  c2 = HMAC(mk, c0 || c1)

The KDF layout is the project's own (the upstream one is unpinned, as for the key ceremony's
backups, whose keys carry "share" where these carry "contest").  Contest data does not enter the
contest hash, the ballot hash or the confirmation codes.

``ContestData`` is the plaintext and its packing; the ``*_host`` functions restate the definitions
on the host and never call the GPU; derive_nonces, seal and open_sealed run them on the GPU
(csrc/eg_hmac.hpp) on numpy arrays or DeviceBuffers; seal_contest_data_seeded and
open_contest_data_seeded work from the ballot nonces, as codes.encrypt_ballots_seeded and
codes.open_ballots do for the selections.
"""
from __future__ import annotations

import hashlib
import hmac
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .ballot import AnyManifest, ElectionKey
from .core import native
from .core.group import FixedBase, GroupContext
from .core.hashing import hash_elems
from .core.marshal import Columns, be_int as _i, rows32

MAX_BYTES = 1024   # EG_CD_MAX_BYTES
TAG = b"contest"

# ContestData.status: the low bits are upstream's ContestDataStatus, TRUNCATED is set by pack()
NORMAL, NULL_VOTE, OVER_VOTE, UNDER_VOTE = 0, 1, 2, 3
TRUNCATED = 0x80


# ---------------------------------------------------------------------------------------------
# the plaintext
# ---------------------------------------------------------------------------------------------
@dataclass
class ContestData:
    """What a contest records besides its selections.  Packed layout (pack / unpack):

      be16 length of everything after these two bytes | status byte |
      count byte, the overvoted selection indices (be16 each) |
      count byte, the write-ins (a length byte plus UTF-8 each) | zero padding to nbytes

    The status and the overvotes always go in (pack raises when nbytes cannot hold them); a
    write-in that does not fit -- the buffer, its length byte or the count byte -- is dropped
    whole, and TRUNCATED is set in the packed status."""
    status: int = NORMAL
    overvotes: List[int] = field(default_factory=list)
    write_ins: List[str] = field(default_factory=list)

    def pack(self, nbytes: int) -> bytes:
        if not 1 <= nbytes <= MAX_BYTES:
            raise ValueError(f"nbytes outside [1, {MAX_BYTES}]")
        if not 0 <= self.status < TRUNCATED:
            raise ValueError("status outside [0, 128)")
        if len(self.overvotes) > 255 or any(not 0 <= int(v) < 65536 for v in self.overvotes):
            raise ValueError("at most 255 overvotes, each below 65536")
        ov = b"".join(int(v).to_bytes(2, "big") for v in self.overvotes)
        room = nbytes - (2 + 2 + len(ov) + 1)
        if room < 0:
            raise ValueError(f"{nbytes} bytes cannot hold the status and {len(self.overvotes)} overvotes")
        kept, status = [], self.status
        for w in self.write_ins:
            e = w.encode("utf-8")
            if len(e) > 255 or len(kept) == 255 or 1 + len(e) > room:
                status |= TRUNCATED
                continue
            kept.append(bytes([len(e)]) + e)
            room -= 1 + len(e)
        body = bytes([status, len(self.overvotes)]) + ov + bytes([len(kept)]) + b"".join(kept)
        out = len(body).to_bytes(2, "big") + body
        return out + bytes(nbytes - len(out))

    @staticmethod
    def unpack(buf) -> "ContestData":
        """The ContestData of a packed buffer (the status as packed, TRUNCATED included).  A length
        or a count that runs past the buffer or past the recorded length is a ValueError."""
        b = bytes(buf)
        if len(b) < 2:
            raise ValueError("contest data shorter than its length field")
        end = 2 + int.from_bytes(b[:2], "big")
        if end > len(b):
            raise ValueError(f"contest data length {end - 2} overruns the {len(b)}-byte buffer")
        pos = 2

        def take(n: int) -> bytes:
            nonlocal pos
            if pos + n > end:
                raise ValueError("contest data field overruns its recorded length")
            pos += n
            return b[pos - n:pos]

        status = take(1)[0]
        overvotes = [int.from_bytes(take(2), "big") for _ in range(take(1)[0])]
        write_ins = [take(take(1)[0]).decode("utf-8") for _ in range(take(1)[0])]
        if pos != end:
            raise ValueError("contest data length does not match its fields")
        return ContestData(status, overvotes, write_ins)


def pack_ballots(data: Sequence[Sequence[ContestData]], nbytes: int) -> np.ndarray:
    """data[b][k] -> (nb, nc, nbytes) uint8"""
    nb, nc = len(data), len(data[0]) if len(data) else 0
    if any(len(row) != nc for row in data):
        raise ValueError("every ballot carries one ContestData per contest")
    out = np.frombuffer(b"".join(cd.pack(nbytes) for row in data for cd in row), np.uint8)
    return out.reshape(nb, nc, nbytes).copy()


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions (no GPU call)
# ---------------------------------------------------------------------------------------------
def _be32(x: int) -> bytes:
    return int(x).to_bytes(4, "big")


def derive_nonces_host(q: int, ncontest: int, ballot_nonces, fmt: str = "fixed") -> np.ndarray:
    """-> r (nb, nc, 32)"""
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    rows = [hash_elems(q, ("Q", _i(bn[b])), ("Q", 3), ("Q", k), fmt=fmt).to_bytes(32, "big")
            for b in range(len(bn)) for k in range(ncontest)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(bn), ncontest, 32).copy()


def item_keys_host(c0, kappa, ballot_id, k: int) -> Tuple[bytes, bytes, bytes]:
    """-> (kk, mk, label) of the item (ballot_id, k)"""
    label = bytes(ballot_id) + _be32(k)
    kk = hashlib.sha256(bytes(c0) + bytes(kappa)).digest()
    return kk, hmac.new(kk, b"\x02" + TAG + label, hashlib.sha256).digest(), label


def stream_host(kk: bytes, label: bytes, nbytes: int) -> bytes:
    blocks = [hmac.new(kk, b"\x01" + TAG + label + _be32(j), hashlib.sha256).digest()
              for j in range((nbytes + 31) // 32)]
    return b"".join(blocks)[:nbytes]


def _xor(a: bytes, b: bytes) -> bytes:
    return (int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).to_bytes(len(a), "big")


def _shapes(ncontest: int, ballot_ids, c0, kappa, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    c0 = np.ascontiguousarray(c0, dtype=np.uint8).reshape(-1, 512)
    n = len(c0)
    if ncontest < 1 or n == 0 or n % ncontest:
        raise ValueError("items are (ballot, contest) pairs, at least one")
    rows = rows.reshape(n, -1)
    if not 1 <= rows.shape[1] <= MAX_BYTES:
        raise ValueError(f"nbytes outside [1, {MAX_BYTES}]")
    kappa = np.ascontiguousarray(kappa, dtype=np.uint8).reshape(-1, 512)
    if len(kappa) != n:
        raise ValueError("one kappa per item")
    return rows32(ballot_ids, n // ncontest, "ballot_ids"), c0, kappa, rows


def seal_host(ncontest: int, ballot_ids, c0, kappa, data) -> Tuple[np.ndarray, np.ndarray]:
    """The hash half of a seal: c0 / kappa (n, 512), data (n, nbytes) -> c1 (n, nbytes), c2 (n, 32)"""
    ids, c0, kappa, data = _shapes(ncontest, ballot_ids, c0, kappa, data)
    c1, c2 = np.empty_like(data), np.empty((len(data), 32), np.uint8)
    for i in range(len(data)):
        kk, mk, label = item_keys_host(c0[i], kappa[i], ids[i // ncontest], i % ncontest)
        ct = _xor(bytes(data[i]), stream_host(kk, label, data.shape[1]))
        c1[i] = np.frombuffer(ct, np.uint8)
        c2[i] = np.frombuffer(hmac.new(mk, bytes(c0[i]) + ct, hashlib.sha256).digest(), np.uint8)
    return c1, c2


def open_host(ncontest: int, ballot_ids, c0, kappa, c1, c2) -> Tuple[np.ndarray, np.ndarray]:
    """-> data (n, nbytes), ok (n,) bool; a failed item's row is zero"""
    ids, c0, kappa, c1 = _shapes(ncontest, ballot_ids, c0, kappa, c1)
    c2 = rows32(c2, len(c1), "c2")
    data, ok = np.zeros_like(c1), np.zeros(len(c1), bool)
    for i in range(len(c1)):
        kk, mk, label = item_keys_host(c0[i], kappa[i], ids[i // ncontest], i % ncontest)
        ct = bytes(c1[i])
        ok[i] = hmac.compare_digest(hmac.new(mk, bytes(c0[i]) + ct, hashlib.sha256).digest(), bytes(c2[i]))
        if ok[i]:
            data[i] = np.frombuffer(_xor(ct, stream_host(kk, label, len(ct))), np.uint8)
    return data, ok


def seal_contest_data_host(p: int, q: int, g: int, K: int, ncontest: int, ballot_nonces, ballot_ids, data,
                           fmt: str = "fixed") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The whole seal on the host (CPython pow): -> c0 (n, 512), c1 (n, nbytes), c2 (n, 32)"""
    r = derive_nonces_host(q, ncontest, ballot_nonces, fmt).reshape(-1, 32)
    c0 = np.frombuffer(b"".join(pow(g, _i(e), p).to_bytes(512, "big") for e in r), np.uint8).reshape(-1, 512)
    kappa = np.frombuffer(b"".join(pow(K, _i(e), p).to_bytes(512, "big") for e in r), np.uint8).reshape(-1, 512)
    c1, c2 = seal_host(ncontest, ballot_ids, c0, kappa, np.asarray(data, np.uint8).reshape(len(r), -1))
    return c0.copy(), c1, c2


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def _nbytes(nbytes: int) -> int:
    if not 1 <= int(nbytes) <= MAX_BYTES:
        raise ValueError(f"nbytes outside [1, {MAX_BYTES}]")
    return int(nbytes)


def derive_nonces(group: GroupContext, ncontest: int, ballot_nonces):
    """-> r (nb, nc, 32) of the ballot nonces (nb, 32); a DeviceBuffer in, a DeviceBuffer out
    (asynchronous on the context's stream)."""
    cols = Columns(group)
    bn = cols.item(ballot_nonces, (32,), "ballot_nonces")
    return cols.call("eg_derive_contest_data_nonces", cols.n, ncontest, bn, cols.out((ncontest, 32)))[0]


def seal(group: GroupContext, key: ElectionKey, ncontest: int, nbytes: int, ballot_ids, nonces_r, data):
    """-> (c0 (n, 512), c1 (n, nbytes), c2 (n, 32)) of data (n, nbytes) under the nonces r (n, 32).
    With DeviceBuffers for the three inputs the results are DeviceBuffers (asynchronous).  The two
    exponentiations follow group.ct_pow."""
    nbytes = _nbytes(nbytes)
    cols = Columns(group)
    ids = cols.item(ballot_ids, (32,), "ballot_ids")
    r = cols.item(nonces_r, (ncontest, 32), "nonces_r")
    data = cols.item(data, (ncontest, nbytes), "data")
    c0, c1, c2 = (cols.out((w,), per=ncontest) for w in (512, nbytes, 32))
    return tuple(cols.call("eg_seal_contest_data", native.buf(key.K_be), cols.n, ncontest, nbytes, ids, r, data,
                           c0, c1, c2))


def open_sealed(group: GroupContext, ncontest: int, nbytes: int, ballot_ids, c0, kappa, c1, c2):
    """-> (data (n, nbytes), ok (n,) bool) from the caller's kappa (n, 512).  An item whose MAC
    fails has ok False and a zero row; the others are not affected.  With DeviceBuffers for all
    five inputs -> DeviceBuffers (ok as flag bytes), asynchronous."""
    nbytes = _nbytes(nbytes)
    cols = Columns(group)
    ids = cols.item(ballot_ids, (32,), "ballot_ids")
    c0, kappa = cols.item(c0, (ncontest, 512), "c0"), cols.item(kappa, (ncontest, 512), "kappa")
    c1, c2 = cols.item(c1, (ncontest, nbytes), "c1"), cols.item(c2, (ncontest, 32), "c2")
    data, ok = cols.out((nbytes,), per=ncontest), cols.out((), per=ncontest, flag=True)
    return tuple(cols.call("eg_open_contest_data", cols.n, ncontest, nbytes, ids, c0, kappa, c1, c2, data, ok))


# ---------------------------------------------------------------------------------------------
# from the ballot nonces
# ---------------------------------------------------------------------------------------------
@dataclass
class SealedContestData:
    """The HashedElGamalCiphertexts of nb ballots: c0 (nb, nc, 512), c1 (nb, nc, nbytes), c2
    (nb, nc, 32), and the recorded numBytes (None: whatever c1 holds)."""
    c0: np.ndarray
    c1: np.ndarray
    c2: np.ndarray
    num_bytes: Optional[int] = None

    @property
    def nbytes(self) -> int:
        return int(self.c1.shape[-1])


def _data_rows(man: AnyManifest, data, nb: int) -> np.ndarray:
    nc = man.n_contests
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if nb * nc == 0 or data.size % (nb * nc):
        raise ValueError("data: one row per (ballot, contest)")
    return data.reshape(nb, nc, data.size // (nb * nc))


def seal_contest_data_seeded(group: GroupContext, key: ElectionKey, man: AnyManifest, ballot_nonces, ballot_ids,
                             data) -> SealedContestData:
    """Seal data (nb, nc, nbytes) -- pack_ballots' output -- from the ballot nonces.  Only the
    nonces, the ids and the plaintexts go up: every r is derived in HBM and handed to the device
    seal, and kappa never leaves the device."""
    nc = man.n_contests
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    nb = len(bn)
    ids = rows32(ballot_ids, nb, "ballot_ids")
    if not nb:
        w = np.asarray(data).shape[-1] if np.asarray(data).ndim else 0
        return SealedContestData(np.empty((0, nc, 512), np.uint8), np.empty((0, nc, w), np.uint8),
                                 np.empty((0, nc, 32), np.uint8))
    data = _data_rows(man, data, nb)
    nbytes = data.shape[2]
    d_r = derive_nonces(group, nc, group.to_device(bn))
    c0, c1, c2 = seal(group, key, nc, nbytes, group.to_device(ids), d_r, group.to_device(data))
    return SealedContestData(c0.download().reshape(nb, nc, 512), c1.download().reshape(nb, nc, nbytes),
                             c2.download().reshape(nb, nc, 32), nbytes)


def open_contest_data_seeded(group: GroupContext, key: ElectionKey, man: AnyManifest, sealed: SealedContestData,
                             ballot_nonces, ballot_ids) -> Tuple[np.ndarray, np.ndarray]:
    """Open challenged ballots from their ballot nonces, without trustees -> (data (nb, nc, nbytes),
    ok (nb, nc) bool).  Every r is re-derived on the device and kappa = K^r comes from
    FixedBase.pow_batch; an item is ok when c0 == g^r and its MAC holds, and its row is zero
    otherwise.  ContestData.unpack reads an ok row."""
    nc = man.n_contests
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    nb = len(bn)
    ids = rows32(ballot_ids, nb, "ballot_ids")
    nbytes = sealed.nbytes
    if not nb:
        return np.zeros((0, nc, nbytes), np.uint8), np.zeros((0, nc), bool)
    c0 = np.ascontiguousarray(sealed.c0, dtype=np.uint8).reshape(nb * nc, 512)
    r = derive_nonces(group, nc, bn).reshape(-1, 32)
    ktab = FixedBase(group, key.K, key.window_bits)
    try:
        kappa = ktab.pow_batch(r)
    finally:
        ktab.close()
    data, ok = open_sealed(group, nc, nbytes, ids, c0, kappa, sealed.c1, sealed.c2)
    ok &= (group.gPowP_batch(r) == c0).all(axis=1)
    data[~ok] = 0
    return data.reshape(nb, nc, nbytes), ok.reshape(nb, nc)


# ---------------------------------------------------------------------------------------------
# the public check of a record
# ---------------------------------------------------------------------------------------------
def verify_public(group: GroupContext, man: AnyManifest, nb: int, sealed: SealedContestData) -> bool:
    """What anyone can check without a key: one ciphertext per (ballot, contest), every c0 in
    [1, p) with c0^q = 1 (a subgroup element), every c1 as long as the recorded numBytes, every
    c2 32 bytes."""
    nc = man.n_contests
    try:
        c0 = np.ascontiguousarray(sealed.c0, dtype=np.uint8)
        c1, c2 = np.asarray(sealed.c1), np.asarray(sealed.c2)
        nbytes = int(c1.shape[-1] if sealed.num_bytes is None else sealed.num_bytes)
    except (TypeError, ValueError, IndexError):
        return False
    if c0.shape != (nb, nc, 512) or c1.shape != (nb, nc, nbytes) or c2.shape != (nb, nc, 32):
        return False
    if not nb:
        return True
    c0 = c0.reshape(-1, 512)
    p_be = np.frombuffer(group.p.to_bytes(512, "big"), np.uint8)
    # big-endian rows compare like integers: the first differing byte decides
    diff = c0 != p_be
    first = diff.argmax(axis=1)
    below_p = diff.any(axis=1) & (c0[np.arange(len(c0)), first] < p_be[first])
    if not (below_p.all() and c0.any(axis=1).all()):
        return False
    one = np.zeros(512, np.uint8)
    one[511] = 1
    return bool((group.powP_batch(c0, [group.q] * len(c0)) == one).all())
