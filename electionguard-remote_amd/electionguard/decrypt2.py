"""Threshold decryption with ONE combined Chaum-Pedersen proof per text (ElectionGuard 2.0 style),
GPU-backed (include/eg_hip_decrypt2.h).  ``decrypt.py`` (the 1.0 path: a direct
share and a proof per guardian, compensated shares for the missing ones) is untouched.

  key share   z_i = sum_j P_j(x_i) mod q          share public key   Z_i = g^{z_i}
  round 1     M_i = A^{z_i}, a_i = g^u, b_i = A^u  (DecryptingTrustee2.commit)
  combine     M = prod M_i^{w_i}, a = prod a_i, b = prod b_i,
              c = H(qbar, 0x30, K, A, B, a, b, M), c_i = c w_i
  round 2     v_i = u - c_i z_i                    (DecryptingTrustee2.respond, ONCE per commit)
  check       g^{v_i} Z_i^{c_i} == a_i, A^{v_i} M_i^{c_i} == b_i;  v = sum v_i
  record      M, (c, v) per text, T = B / M, count = dLog_g T
  verifier    a' = g^v K^c, b' = A^v M^c, c == H(qbar, 0x30, K, A, B, a', b', M)

The pre-image order and the minus response are fixed (``group.set_proof_format`` does not apply);
the hex format of the hash is the context's.  All arrays are text-major with the guardian inner:
texts (n, 2, 512), shares (n, k, 512), comm (n, k, 2, 512), ci / vi (n, k, 32), proofs (n, 2, 32).
``combine``, ``check`` and ``verify`` take numpy arrays (host entry points) or DeviceBuffers (the
``_dev`` twins, asynchronous on the context's stream); the ``*_host`` functions restate every step
on CPython ints and never call the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import contest_data as _cd
from . import prodpow as _pp
from .core import native
from .core.group import as_p_array, as_q_array, p_bytes
from .core.hashing import hash_elems
from .core.marshal import Columns, be32, be_int, call as _call, ptr
from .decode import decode_counts
from .decrypt import _concurrently, _nonces, _texts_array, dlog_g_batch, lagrange, spoiled_texts
from .keyceremony import GuardianKeys, poly_eval

TAG = 0x30
MAX_GUARDIANS = 64
MAX_ITEMS = 1 << 24
CHUNK_JOBS = 1 << 16   # EG_DECRYPT2_CHUNK_JOBS: exponentiation jobs per chunk of the library's calls
DECODES = ("host", "device")   # where decrypt_record takes the dLog of B / M


def chunk_texts(k: int = 1) -> int:
    """Texts per chunk of combine / check with k guardians (k = 1: commit, respond, verify)."""
    return max(1, CHUNK_JOBS // (4 * int(k)))


# ---------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------
def key_share(keys: GuardianKeys, q: int) -> int:
    """z_i = sum_j P_j(x_i) mod q: the guardian's own polynomial at its x plus every share it holds."""
    return (poly_eval(keys.coeffs, keys.x, q) + sum(keys.shares_from.values())) % q


def _share_key_terms(commitments: Dict[str, List[int]], x: int, q: int):
    flat = [K for gid in sorted(commitments) for K in commitments[gid]]
    exps = [pow(x, m, q) for gid in sorted(commitments) for m in range(len(commitments[gid]))]
    return flat, exps


def share_public_keys(group, commitments: Dict[str, List[int]], xs: Dict[str, int]) -> Dict[str, int]:
    """Z_i = prod_j prod_m K_{j,m}^(x_i^m mod q) for every guardian of xs, from the public
    commitments alone: one multi-exponentiation (prodpow.prod_pow) per guardian."""
    out = {}
    for gid, x in xs.items():
        flat, exps = _share_key_terms(commitments, x, group.q)
        out[gid] = be_int(_pp.prod_pow(group, as_p_array(flat).reshape(1, len(flat), 512), exps)[0])
    return out


def share_public_keys_host(group, commitments: Dict[str, List[int]], xs: Dict[str, int]) -> Dict[str, int]:
    out = {}
    for gid, x in xs.items():
        flat, exps = _share_key_terms(commitments, x, group.q)
        out[gid] = _pp.prod_pow_host(group.p, [flat], exps)[0]
    return out


# ---------------------------------------------------------------------------------------------
# the five steps on CPython ints (never the GPU)
# ---------------------------------------------------------------------------------------------
def challenge_host(group, qbar: int, K: int, A: int, B: int, a: int, b: int, M: int) -> int:
    return hash_elems(group.q, ("Q", qbar), ("Q", TAG), ("P", K), ("P", A), ("P", B), ("P", a), ("P", b), ("P", M),
                      fmt=group.hash_format)


def commit_host(group, z: int, pads: Sequence[int], nonces: Sequence[int]):
    """-> (M, a, b) lists of ints."""
    p, g = group.p, group.g
    return ([pow(A % p, z, p) for A in pads], [pow(g, u, p) for u in nonces],
            [pow(A % p, u, p) for A, u in zip(pads, nonces)])


def respond_host(group, z: int, nonces: Sequence[int], ci: Sequence[int]) -> List[int]:
    q = group.q
    return [(u % q - (c % q) * (z % q)) % q for u, c in zip(nonces, ci)]


def combine_host(group, K: int, qbar: int, weights: Sequence[int], texts, shares, comm):
    """texts [(A, B)], shares [t][i], comm [t][i] = (a_i, b_i) -> (M [t], c [t], ci [t][i])."""
    p, q = group.p, group.q
    Ms, cs, cis = [], [], []
    for (A, B), sh, cm in zip(texts, shares, comm):
        M = _pp.prod_pow_host(p, [sh], weights)[0]
        a = b = 1 % p
        for ai, bi in cm:
            a, b = a * (ai % p) % p, b * (bi % p) % p
        c = challenge_host(group, qbar, K, A, B, a, b, M)
        Ms.append(M)
        cs.append(c)
        cis.append([c * (w % q) % q for w in weights])
    return Ms, cs, cis


def check_host(group, Z: Sequence[int], texts, shares, comm, ci, vi):
    """-> (ok [t][i], v [t])."""
    p, q, g = group.p, group.q, group.g
    oks, vs = [], []
    for (A, _), sh, cm, cr, vr in zip(texts, shares, comm, ci, vi):
        oks.append([c < q and v < q and pow(g, v, p) * pow(Zi % p, c, p) % p == ai and
                    pow(A % p, v, p) * pow(Mi % p, c, p) % p == bi
                    for Zi, Mi, (ai, bi), c, v in zip(Z, sh, cm, cr, vr)])
        vs.append(sum(v % q for v in vr) % q)
    return oks, vs


def verify_host(group, K: int, qbar: int, texts, M: Sequence[int], proofs) -> List[bool]:
    p, q, g = group.p, group.q, group.g
    out = []
    for (A, B), Mt, (c, v) in zip(texts, M, proofs):
        a = pow(g, v, p) * pow(K % p, c, p) % p
        b = pow(A % p, v, p) * pow(Mt % p, c, p) % p
        out.append(c < q and v < q and c == challenge_host(group, qbar, K, A, B, a, b, Mt))
    return out


# ---------------------------------------------------------------------------------------------
# the five steps on the GPU
# ---------------------------------------------------------------------------------------------
def _limits(n: int, k: int) -> None:
    if not 1 <= k <= MAX_GUARDIANS:
        raise ValueError(f"decrypt2: {k} guardians, expected 1..{MAX_GUARDIANS}")
    if n * k > MAX_ITEMS:
        raise ValueError(f"decrypt2: {n} texts x {k} guardians exceed 2^24 in all")


def _q_rows(xs, k: Optional[int], what: str) -> np.ndarray:
    a = xs if isinstance(xs, np.ndarray) and xs.dtype == np.uint8 else as_q_array([int(x) for x in xs])
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    if k is not None and len(a) != k:
        raise ValueError(f"{what}: expected {k} x 32 bytes, got {a.size}")
    return a


def commit(group, secret: int, pads, nonces) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Round 1 of one guardian, constant time: pads (n, 512), nonces (n, 32) -> M, a, b (n, 512)."""
    pads = as_p_array(pads if isinstance(pads, np.ndarray) else list(pads))
    n = len(pads)
    U = _q_rows(nonces, n, "nonces")
    _limits(n, 1)
    M, a, b = (np.zeros((n, 512), np.uint8) for _ in range(3))
    _call(group, "eg_decrypt2_commit", native.buf(be32(secret)), ptr(pads), ptr(U), n, ptr(M), ptr(a), ptr(b))
    return M, a, b


def respond(group, secret: int, nonces, challenges) -> np.ndarray:
    """Round 2 of one guardian: v (n, 32) = u - c z mod q, every scalar reduced mod q first."""
    U = _q_rows(nonces, None, "nonces")
    n = len(U)
    C = _q_rows(challenges, n, "challenges")
    _limits(n, 1)
    v = np.zeros((n, 32), np.uint8)
    _call(group, "eg_decrypt2_respond", native.buf(be32(secret)), ptr(U), ptr(C), n, ptr(v))
    return v


def combine(group, K: int, qbar: int, weights, texts, shares, comm):
    """-> (M (n, 512), c (n, 32), ci (n * k, 32) as (n, k, 32) on the host)."""
    w = _q_rows(weights, None, "weights")
    k = len(w)
    cols = Columns(group)
    t = cols.item(texts, (2, 512), "texts")
    s, cm = cols.item(shares, (k, 512), "shares"), cols.item(comm, (k, 2, 512), "comm")
    _limits(cols.n, k)
    M, c, ci = cols.call("eg_decrypt2_combine", native.buf(p_bytes(K)), native.buf(be32(qbar)), cols.n, k, ptr(w),
                         t, s, cm, cols.out((512,)), cols.out((32,)), cols.out((k, 32)))
    return M, c, ci


def check(group, Z, texts, shares, comm, ci, vi):
    """-> (ok (n, k) bool, v (n, 32)): the mediator's check of every (text, guardian) and the
    texts' summed responses."""
    Zb = as_p_array(Z if isinstance(Z, np.ndarray) else [int(z) for z in Z])
    k = len(Zb)
    cols = Columns(group)
    t = cols.item(texts, (2, 512), "texts")
    s, cm = cols.item(shares, (k, 512), "shares"), cols.item(comm, (k, 2, 512), "comm")
    c, v = cols.item(ci, (k, 32), "ci"), cols.item(vi, (k, 32), "vi")
    _limits(cols.n, k)
    ok, vs = cols.call("eg_decrypt2_check", cols.n, k, ptr(Zb), t, s, cm, c, v, cols.out((k,), flag=True),
                       cols.out((32,)))
    return ok, vs


def verify(group, K: int, qbar: int, texts, M, proofs):
    """-> ok (n,) bool: the record verifier's check of every (c, v)."""
    cols = Columns(group)
    t = cols.item(texts, (2, 512), "texts")
    m, pr = cols.item(M, (512,), "M"), cols.item(proofs, (2, 32), "proofs")
    _limits(cols.n, 1)
    return cols.call("eg_decrypt2_verify", native.buf(p_bytes(K)), native.buf(be32(qbar)), cols.n, t, m, pr,
                     cols.out((), flag=True))[0]


# ---------------------------------------------------------------------------------------------
# trustee and mediator
# ---------------------------------------------------------------------------------------------
class DecryptingTrustee2:
    """One guardian of the two-round decryption.  ``commit`` keeps the nonces under a handle;
    ``respond`` releases them ONCE: a nonce answered for two challenges gives away z_i, so a second
    ``respond`` on a handle raises.  host: run on CPython ints (the ``*_host`` mirrors; ``group``
    then only needs p, q, g)."""

    def __init__(self, group, keys: GuardianKeys, host: bool = False):
        self.group, self.keys, self.host = group, keys, host
        self.z = key_share(keys, group.q)
        self._open: Dict[int, np.ndarray] = {}
        self._next = 0

    def id(self) -> str:
        return self.keys.gid

    def xCoordinate(self) -> int:
        return self.keys.x

    def commit(self, texts, nonces=None):
        """texts (n, 2, 512) or (A, B) pairs -> (handle, M, a, b), each (n, 512)."""
        T = _texts_array(texts)
        U = _nonces(self.group, len(T), nonces)
        pads = np.ascontiguousarray(T[:, 0])
        if self.host:
            M, a, b = (as_p_array(x) if x else np.zeros((0, 512), np.uint8) for x in commit_host(
                self.group, self.z, [be_int(r) for r in pads], [be_int(r) for r in U]))
        else:
            M, a, b = commit(self.group, self.z, pads, U)
        handle, self._next = self._next, self._next + 1
        self._open[handle] = U
        return handle, M, a, b

    def respond(self, handle, ci) -> np.ndarray:
        """ci (n, 32) -> v_i (n, 32); the handle's nonces are gone afterwards, whatever happens."""
        U = self._open.pop(handle, None)
        if U is None:
            raise ValueError(f"trustee {self.id()}: no open commitment {handle!r} (a commitment is answered once)")
        C = _q_rows(ci, len(U), "ci")
        if self.host:
            v = respond_host(self.group, self.z, [be_int(r) for r in U], [be_int(r) for r in C])
            return as_q_array(v) if v else np.zeros((0, 32), np.uint8)
        return respond(self.group, self.z, U, C)


@dataclass
class DecryptionRecord2:
    """What the mediator publishes: per text the combined M and ONE proof (c, v), and the counts."""
    texts: np.ndarray              # (n, 2, 512)
    xs: Dict[str, int]             # available guardian -> x coordinate
    M: np.ndarray                  # (n, 512)
    proofs: np.ndarray             # (n, 2, 32) = (c, v)
    counts: List[Optional[int]]


class Decryption2:
    """The mediator: ``Decryption2(group, qbar, K, trustees, share_keys).decrypt(tally, max_count)``.
    trustees: the available guardians (at least the quorum); share_keys: guardian id -> Z_i
    (``share_public_keys``)."""

    def __init__(self, group, qbar: int, K: int, trustees: Sequence, share_keys: Dict[str, int]):
        self.group, self.qbar, self.K = group, int(qbar), int(K)
        self.trustees = list(trustees)
        self.share_keys = share_keys
        _limits(0, len(self.trustees))

    def rounds(self, T: np.ndarray):
        """Both rounds over the texts T (n, 2, 512) -> (shares, comm, ci, vi), unchecked."""
        G = self.group
        xs = [t.xCoordinate() for t in self.trustees]
        w = [lagrange(xs, x, G.q) for x in xs]
        r1 = _concurrently(lambda tr: tr.commit(T), self.trustees)
        shares = np.ascontiguousarray(np.stack([r[1] for r in r1], axis=1))
        comm = np.ascontiguousarray(np.stack([np.stack([r[2], r[3]], axis=1) for r in r1], axis=1))
        M, c, ci = combine(G, self.K, self.qbar, w, T, shares, comm)
        ci = ci.reshape(len(T), len(xs), 32)
        r2 = _concurrently(lambda it: it[1].respond(r1[it[0]][0], np.ascontiguousarray(ci[:, it[0]])),
                           list(enumerate(self.trustees)))
        vi = np.ascontiguousarray(np.stack(r2, axis=1))
        return shares, comm, M, c, ci, vi

    def checked(self, T, shares, comm, c, ci, vi) -> np.ndarray:
        """The mediator's check -> proofs (n, 2, 32); a guardian whose check fails raises, naming it."""
        ok, v = check(self.group, [self.share_keys[t.id()] for t in self.trustees], T, shares, comm, ci, vi)
        for i, tr in enumerate(self.trustees):
            if not ok[:, i].all():
                raise ValueError(f"invalid decryption share or response from {tr.id()}")
        return np.ascontiguousarray(np.stack([c, v], axis=1))

    def _combined(self, T: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        if not len(T):
            return np.zeros((0, 512), np.uint8), np.zeros((0, 2, 32), np.uint8)
        shares, comm, M, c, ci, vi = self.rounds(T)
        return M, self.checked(T, shares, comm, c, ci, vi)

    def decrypt_record(self, tally, max_count: int, decode: str = "host") -> DecryptionRecord2:
        """decode: "host" takes t = dLog_g(B / M) through multInv_batch, multP_batch and the host's
        baby-step giant-step; "device" through decode.decode_counts (inverse, table and giant steps on
        the GPU).  The counts are the same list either way: None where there is no t <= max_count."""
        if decode not in DECODES:
            raise ValueError(f"decode: one of {DECODES}, got {decode!r}")
        G = self.group
        T = _texts_array(tally)
        M, proofs = self._combined(T)
        counts = []
        if len(T) and decode == "device":
            t = decode_counts(G, np.ascontiguousarray(T[:, 1]), M, max_count)
            counts = [None if c < 0 else int(c) for c in t]
        elif len(T):
            counts = dlog_g_batch(G, G.multP_batch(np.ascontiguousarray(T[:, 1]), G.multInv_batch(M)), max_count)
        return DecryptionRecord2(T, {t.id(): t.xCoordinate() for t in self.trustees}, M, proofs, counts)

    def decrypt(self, tally, max_count: int, decode: str = "host") -> List[Optional[int]]:
        return self.decrypt_record(tally, max_count, decode).counts

    # ---- spoiled ballots ----
    @staticmethod
    def _ballot_texts(ballots, man):
        """-> (texts, selections per ballot, largest count) for an ElectionManifest (the real
        selections, decrypt.spoiled_texts) or a ballot2.Manifest2 (every selection)."""
        cts = ballots.cts if hasattr(ballots, "cts") else ballots
        cts = np.asarray(cts.download() if hasattr(cts, "download") else cts)
        if hasattr(man, "olimit"):
            return np.ascontiguousarray(cts).reshape(-1, 2, 512), int(man.NS), int(man.olimit.max())
        return spoiled_texts(man, cts), int(man.n_real), int(man.max_votes_allowed)

    def decrypt_ballots_record(self, ballots, man, decode: str = "host") -> DecryptionRecord2:
        T, _, limit = self._ballot_texts(ballots, man)
        return self.decrypt_record(T, limit, decode)

    def decryptBallots(self, ballots, man, decode: str = "host") -> np.ndarray:
        """-> (nb, selections) plaintext selections; -1 where a value is not a valid count."""
        T, per, limit = self._ballot_texts(ballots, man)
        counts = self.decrypt_record(T, limit, decode).counts
        return np.array([-1 if c is None else int(c) for c in counts], dtype=np.int64).reshape(-1, per)

    # ---- contest data ----
    def decryptContestData(self, c0, c1, c2, ballot_ids, ncontest: int) -> Tuple[np.ndarray, np.ndarray]:
        """As Decryption.decryptContestData: texts (c0, 1), kappa = the combined M."""
        ids = np.ascontiguousarray(ballot_ids, dtype=np.uint8).reshape(-1, 32)
        nb = len(ids)
        n = nb * ncontest
        c1 = np.ascontiguousarray(c1, dtype=np.uint8)
        if n == 0 or c1.size % n:
            raise ValueError("c1: one row per (ballot, contest)")
        nbytes = c1.size // n
        T = np.zeros((n, 2, 512), dtype=np.uint8)
        T[:, 0] = np.ascontiguousarray(c0, dtype=np.uint8).reshape(n, 512)
        T[:, 1, 511] = 1
        kappa, _ = self._combined(T)
        data, ok = _cd.open_sealed(self.group, ncontest, nbytes, ids, T[:, 0], kappa, c1, c2)
        return data.reshape(nb, ncontest, nbytes), ok.reshape(nb, ncontest)


def verify_decryption_record2(group, qbar: int, K: int, rec: DecryptionRecord2,
                              max_count: Optional[int] = None) -> Dict[str, bool]:
    """The record verifier: ``proofs`` every (c, v) through eg_decrypt2_verify; ``tally``
    B == M * g^t per text on the GPU with every count an integer in [0, max_count]."""
    T = _texts_array(rec.texts)
    n = len(T)
    out = {"proofs": True, "tally": True}
    M = np.ascontiguousarray(rec.M, np.uint8).reshape(-1, 512)
    pr = np.ascontiguousarray(rec.proofs, np.uint8).reshape(-1, 2, 32)
    if len(M) != n or len(pr) != n:
        return {"proofs": False, "tally": False}
    if len(rec.counts) != n or any(
            c is None or not isinstance(c, (int, np.integer)) or c < 0 or (max_count is not None and c > max_count)
            for c in rec.counts):
        out["tally"] = False
    if not n:
        return out
    out["proofs"] = bool(verify(group, K, qbar, T, M, pr).all())
    if out["tally"]:
        lhs = group.multP_batch(M, group.gPowP_batch([int(c) for c in rec.counts]))
        out["tally"] = bool(np.array_equal(lhs, np.ascontiguousarray(T[:, 1])))
    return out
