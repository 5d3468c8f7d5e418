"""A per-ballot seed, confirmation codes and the opening of challenged ballots for the ballots
without placeholder selections of ``ballot2`` (include/eg_hip_codes2.h): what
``codes`` gives the ElectionGuard 1.0 form.

With H = core.hashing.hash_elems (no Q-bar prefix), xi_b a ballot's 32-byte seed and the row
layouts of ``ballot2.Manifest2``:

  sel_nonces[b, r]     = H(Q xi_b, Q 5, Q r)      0 <= r < SN
  contest_nonces[b, r] = H(Q xi_b, Q 6, Q r)      0 <= r < CN
  R of selection i of contest k = sel_nonces[b, sn_off[k] + i (2 olimit[k] + 4)]
  h_sel, h_con, B, code: codes' definitions with spc[k] = nsel[k]; the proofs do not enter
  open: ok = (alpha == g^R) and (beta == K^R g^m for one m in 0..olimit[k]); votes = m, else 0

The ``*_host`` functions restate the definitions on CPython ints and never call the GPU; the others
run the library on numpy arrays or DeviceBuffers.  Ballot hashes and the code chain are ``codes``'
own entry points (a placeholder-free ballot is a manifest whose every selection is real)."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import ballot2 as b2
from . import codes as _codes
from . import range_proof as rp
from .ballot2 import EncryptedBallots2, Manifest2
from .codes import ManifestHashes, Q32
from .core import native
from .core.hashing import hash_elems
from .core.marshal import Columns, be32_row as _b32, be_int as _i, rows32

TAG_SEL, TAG_CON = 5, 6


class _CodesManifest:
    """What codes.ballot_hashes reads of a manifest, for a Manifest2: every selection is real."""

    def __init__(self, man: Manifest2):
        self.nsel, self.n_contests = man.NS, man.n_contests
        self.spc_list = np.ascontiguousarray(man.nsel, np.uint32)
        self.offsets = man.first


def _cts_of(eb_or_cts):
    return eb_or_cts.cts if hasattr(eb_or_cts, "cts") else eb_or_cts


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions (no GPU call)
# ---------------------------------------------------------------------------------------------
def derive_nonces2_host(q: int, man: Manifest2, ballot_nonces, fmt: str = "fixed") -> Tuple[np.ndarray, np.ndarray]:
    """-> sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32): ballot2.encrypt's inputs."""
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    sn = np.empty((len(bn), man.SN, 32), np.uint8)
    cn = np.empty((len(bn), man.CN, 32), np.uint8)
    for b in range(len(bn)):
        xi = _i(bn[b])
        for r in range(man.SN):
            sn[b, r] = _b32(hash_elems(q, ("Q", xi), ("Q", TAG_SEL), ("Q", r), fmt=fmt))
        for r in range(man.CN):
            cn[b, r] = _b32(hash_elems(q, ("Q", xi), ("Q", TAG_CON), ("Q", r), fmt=fmt))
    return sn, cn


def ballot_hashes2_host(q: int, man: Manifest2, hashes: ManifestHashes, ballot_ids, cts, fmt: str = "fixed"):
    """-> B (nb, 32), h_sel (nb, NS, 32), h_con (nb, nc, 32)."""
    return _codes.ballot_hashes_host(q, _CodesManifest(man), hashes, ballot_ids, _cts_of(cts), fmt=fmt)


def open_ballots2_host(group, key, man: Manifest2, eb_or_cts, ballot_nonces, fmt: str = None):
    """open_ballots2 on the host -> (votes (nb, NS) uint8, ok (nb, NS) bool).  group needs p, q and
    g only (fmt: its hash_format when not given)."""
    p, q, g, K = group.p, group.q, group.g, rp._key_int(key)
    fmt = fmt or getattr(group, "hash_format", "fixed")
    cts = np.ascontiguousarray(_cts_of(eb_or_cts), np.uint8).reshape(-1, man.NS, 2, 512)
    nb = len(cts)
    bn = rows32(ballot_nonces, nb, "ballot_nonces")
    votes, ok = np.zeros((nb, man.NS), np.uint8), np.zeros((nb, man.NS), bool)
    for b in range(nb):
        xi = _i(bn[b])
        for _, _, s, L, _, nr in man.selections():
            R = hash_elems(q, ("Q", xi), ("Q", TAG_SEL), ("Q", nr), fmt=fmt)
            alpha, beta = _i(cts[b, s, 0]), _i(cts[b, s, 1])
            if alpha != pow(g, R, p):
                continue
            T = pow(K, R, p)
            for m in range(L + 1):
                if T == beta:
                    votes[b, s], ok[b, s] = m, True
                    break
                T = T * g % p
    return votes, ok


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def derive_nonces2(group, man: Manifest2, ballot_nonces):
    """-> (sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32)) of the ballot nonces (nb, 32);
    DeviceBuffers in, DeviceBuffers out (asynchronous on the context's stream)."""
    cols = Columns(group)
    bn = cols.item(ballot_nonces, (32,), "ballot_nonces")
    return tuple(cols.call("eg_derive_ballot_nonces_v2", cols.n, *man._shape_args(), bn, cols.out((man.SN, 32)),
                           cols.out((man.CN, 32))))


def ballot_hashes2(group, man: Manifest2, hashes: ManifestHashes, ballot_ids, cts, parts: bool = False):
    """codes.ballot_hashes for placeholder-free ballots: B (nb, 32), or (B, h_sel (nb, NS, 32),
    h_con (nb, nc, 32)) with parts; DeviceBuffers are hashed where they lie."""
    return _codes.ballot_hashes(group, _CodesManifest(man), hashes, ballot_ids, _cts_of(cts), parts=parts)


def open_ballots2(group, key, man: Manifest2, eb_or_cts, ballot_nonces):
    """Open ballots from their ballot nonces, without trustees -> (votes (nb, NS) uint8, ok
    (nb, NS) bool; DeviceBuffers of bytes for DeviceBuffer ballots, asynchronous).  Every R is
    re-derived on the device, g^R and K^R follow group.ct_pow, and the match against
    K^R g^m, m = 0..option limit, runs on the device; votes is 0 where ok is False."""
    cols = Columns(group)
    cts = cols.item(_cts_of(eb_or_cts), (man.NS, 2, 512), "cts")
    bn = cols.item(ballot_nonces, (32,), "ballot_nonces")
    votes, ok = cols.call("eg_open_ballots_v2", native.buf(key.K_be), cols.n, *man._shape_args(), bn, cts,
                          cols.out((man.NS,)), cols.out((man.NS,), flag=True))
    return votes, ok


def encrypt_ballots_seeded2(group, key, qbar: int, man: Manifest2, hashes: ManifestHashes, votes, ballot_nonces,
                            ballot_ids, timestamps, seed: Q32) -> Tuple[EncryptedBallots2, np.ndarray, np.ndarray]:
    """Encrypt nb ballots from their ballot nonces -> (EncryptedBallots2, ballot_hashes (nb, 32),
    codes (nb, 32)).  Only the seeds, votes and ids go up: the nonce rows are derived in HBM and
    handed to the device encryptor, and the hashes are taken from the ciphertexts still there; the
    chain is built on the host.  A vote or a contest sum over its limit raises ValueError before
    anything is uploaded."""
    votes = np.ascontiguousarray(votes, dtype=np.uint8).reshape(-1, man.NS)
    nb = len(votes)
    b2.check_votes(man, votes)
    bn = rows32(ballot_nonces, nb, "ballot_nonces")
    ids = rows32(ballot_ids, nb, "ballot_ids")
    if not nb:
        eb = EncryptedBallots2(np.empty((0, man.NS, 2, 512), np.uint8), np.empty((0, man.SP, 2, 32), np.uint8),
                               np.empty((0, man.CP, 2, 32), np.uint8))
        return eb, np.empty((0, 32), np.uint8), np.empty((0, 32), np.uint8)
    d_sn, d_cn = derive_nonces2(group, man, group.to_device(bn))
    d_eb = b2.encrypt(group, key, qbar, man, group.to_device(votes), d_sn, d_cn)
    d_B = ballot_hashes2(group, man, hashes, group.to_device(ids), d_eb.cts)
    eb = EncryptedBallots2(d_eb.cts.download(), d_eb.sproof.download(), d_eb.cproof.download())
    B = d_B.download()
    return eb, B, _codes.chain_codes(group.q, seed, timestamps, B, fmt=group.hash_format)


def verify_ballot_codes2(group, man: Manifest2, hashes: ManifestHashes, ballot_ids, cts, timestamps, seed: Q32,
                         codes) -> np.ndarray:
    """-> ok (nb,) bool: codes[b] == H(codes[b-1] or seed, ts[b], B[b]) with B[b] recomputed from
    the ciphertexts on the device and the RECORDED codes[b-1]."""
    B = ballot_hashes2(group, man, hashes, ballot_ids, cts)
    B = B.download() if hasattr(B, "download") else B
    return _codes.verify_code_chain(group, seed, timestamps, B, codes)


# ---------------------------------------------------------------------------------------------
# spoiled ballots through the trustees
# ---------------------------------------------------------------------------------------------
def decrypt_ballots2_record(decryption, ballots, man: Manifest2):
    """The DecryptionRecord of a batch of spoiled ballots: every selection is a text (there are no
    placeholders to drop), ballot-major, in ONE trustee batch per guardian; counts are looked up
    to the manifest's largest option limit."""
    cts = np.ascontiguousarray(_cts_of(ballots), np.uint8).reshape(-1, 2, 512)
    return decryption.decrypt_record(cts, int(man.olimit.max()))


def decrypt_ballots2(decryption, ballots, man: Manifest2) -> np.ndarray:
    """-> (nb, NS) int64 decrypted selections of spoiled ballots (EncryptedBallots2 or their
    (nb, NS, 2, 512) ciphertexts); -1 where a value has no discrete log up to the largest option
    limit or exceeds its own contest's, which an honest ballot never has."""
    cts = np.ascontiguousarray(_cts_of(ballots), np.uint8).reshape(-1, man.NS, 2, 512)
    if not len(cts):
        return np.zeros((0, man.NS), np.int64)
    counts = decrypt_ballots2_record(decryption, cts, man).counts
    out = np.array([-1 if c is None else int(c) for c in counts], np.int64).reshape(len(cts), man.NS)
    limit = np.repeat(man.olimit.astype(np.int64), man.nsel)
    out[out > limit] = -1
    return out
