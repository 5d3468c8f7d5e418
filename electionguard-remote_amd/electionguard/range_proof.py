"""Proofs that a ciphertext encrypts a value in 0..L, made and checked in batches on the GPU.

The selection proofs of ``ballot`` are 0-or-1 disjunctions.  This is the (L+1)-branch disjunctive
Chaum-Pedersen proof (include/eg_hip_range.h): a selection that takes up to L marks (cumulative
and score voting, ElectionGuard 2.0's option selection limit), or a contest's "at most L of these"
shown on the contest aggregate with no placeholder selection.  At L = 1 it is the selection proof
byte for byte.

An item is a ciphertext (alpha, beta) = (g^R, K^R g^m), a limit L in 1..MAX_LIMIT (one per call)
and a proof (c_0, v_0, ..., c_L, v_L).  With e_j = c_j (response "minus") or -c_j ("plus"):

  verifier  a_j = g^v_j alpha^e_j,  b_j = K^v_j beta^e_j g^(-j e_j)
            c = H(Q-bar; (alpha, beta); (a_0, b_0, ..., a_L, b_L))   in the pre-image order
            ok = alpha, beta valid residues, every c_j, v_j < q, sum c_j = c (mod q)
  prover    nonces (u, c_0, v_0, ..., c_L, v_L): a_m = g^u, b_m = K^u, the other branches the
            verifier's values; c_m = c - sum_{j != m} c_j, v_m = u -+ c_m R.  The supplied
            (c_m, v_m) is ignored, so the nonce layout does not depend on the value.

Layouts (uint8, big-endian, item-major): cts (n, 2, 512), proofs (n, L+1, 2, 32), values (n,),
R (n, 32), nonces (n, 2L+3, 32), ok (n,).

``prove_host`` / ``verify_host`` restate the definitions on CPython ints and never call the GPU;
``prove`` / ``verify`` run on the GPU (csrc/eg_range.hpp and the k_pow jobs of
csrc/eg_capi_range.inc) on numpy arrays or DeviceBuffers; ``contest_limit_prove`` /
``contest_limit_verify`` put a 0..votes_allowed proof on every contest's aggregate, composed on the
host from numpy arrays.  Whole ballots of that form (no placeholders, a range proof per selection
and per contest) are encrypted, verified and tallied in one batch call by ``ballot2``
(include/eg_hip_ballot2.h), which also takes device-resident ballots.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

from .core import native
from .core.hashing import hash_elems
from .core.marshal import Columns, be32, be_int as _i

MAX_LIMIT = 15   # EG_RANGE_MAX_LIMIT
CHUNK_JOBS = 1 << 16   # kRangeChunkJobs (csrc/eg_capi_range.inc)


def chunk_items(limit: int) -> int:
    """Items per chunk of the library's calls at this limit: a chunk holds at most CHUNK_JOBS
    verifier jobs, 2 L per item (32,768 items at L = 1, 2,184 at L = 15)."""
    return max(1, CHUNK_JOBS // (2 * int(limit)))


@dataclass(frozen=True)
class HostGroup:
    """What the host mirrors read of a group: a GroupContext stands for one as well."""
    p: int
    q: int
    g: int
    hash_format: str = "fixed"
    proof_format: Tuple[str, str] = ("minus", "message_first")


def _limit(limit: int) -> int:
    if not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"limit outside [1, {MAX_LIMIT}]")
    return int(limit)


def _key_int(key) -> int:
    return int(key.K) if hasattr(key, "K") else int(key)


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions (no GPU call)
# ---------------------------------------------------------------------------------------------
def resp_exp_host(group, c: int) -> int:
    """The exponent alpha and beta are raised to: c ("minus") or -c ("plus")."""
    return c % group.q if group.proof_format[0] == "minus" else (-c) % group.q


def response_host(group, u: int, c: int, x: int) -> int:
    return (u - c * x) % group.q if group.proof_format[0] == "minus" else (u + c * x) % group.q


def challenge_host(group, K: int, qbar: int, msg, comm) -> int:
    order = group.proof_format[1]
    if order == "message_first":
        els = [*msg, *comm]
    elif order == "commitments_first":
        els = [*comm, *msg]
    else:
        els = [K, *msg, *comm]
    return hash_elems(group.q, ("Q", qbar), *(("P", e) for e in els), fmt=group.hash_format)


def valid_residue_host(group, x: int) -> bool:
    return 0 < x < group.p and pow(x, group.q, group.p) == 1


def commitments_host(group, K: int, alpha: int, beta: int, branches) -> list:
    """The verifier's (a_0, b_0, ..., a_L, b_L) of the branches [(c_j, v_j)]."""
    p, q, g = group.p, group.q, group.g
    out = []
    for j, (c, v) in enumerate(branches):
        e = resp_exp_host(group, c)
        out.append(pow(g, v, p) * pow(alpha % p, e, p) % p)
        out.append(pow(K, v, p) * pow(beta % p, e, p) * pow(g, (-j * e) % q, p) % p)
    return out


def prove_item_host(group, K: int, qbar: int, limit: int, alpha: int, beta: int, m: int, R: int, u: int,
                    branches) -> list:
    """One item: branches [(c_j, v_j)] for every j (entry m is ignored) -> the proof's
    [(c_j, v_j)].  m may lie about the ciphertext (the proof then fails to verify)."""
    p, q, g = group.p, group.q, group.g
    if len(branches) != limit + 1 or not 0 <= m <= limit:
        raise ValueError("one (c, v) pair per branch and a value in 0..limit")
    comm = []
    for j, (c, v) in enumerate(branches):
        if j == m:
            comm += [pow(g, u, p), pow(K, u, p)]
        else:
            e = resp_exp_host(group, c)
            s = (v + R * e) % q
            comm += [pow(g, s, p), pow(K, s, p) * pow(g, ((m - j) * e) % q, p) % p]
    c = challenge_host(group, K, qbar, (alpha, beta), comm)
    cm = (c - sum(cj for j, (cj, _) in enumerate(branches) if j != m)) % q
    out = [(int(cj), int(vj)) for cj, vj in branches]
    out[m] = (cm, response_host(group, u, cm, R))
    return out


def verify_item_host(group, K: int, qbar: int, limit: int, alpha: int, beta: int, branches) -> bool:
    q = group.q
    if len(branches) != limit + 1:
        return False
    if not (valid_residue_host(group, alpha) and valid_residue_host(group, beta)):
        return False
    if not all(0 <= c < q and 0 <= v < q for c, v in branches):
        return False
    comm = commitments_host(group, K, alpha, beta, branches)
    return sum(c for c, _ in branches) % q == challenge_host(group, K, qbar, (alpha, beta), comm)


def prove_host(group, key, qbar: int, limit: int, cts, values, R, nonces) -> np.ndarray:
    """prove() on the host, same layouts -> proofs (n, L+1, 2, 32)."""
    L = _limit(limit)
    K = _key_int(key)
    cts = np.ascontiguousarray(cts, dtype=np.uint8).reshape(-1, 2, 512)
    n = len(cts)
    values = np.ascontiguousarray(values, dtype=np.uint8).reshape(n)
    R = np.ascontiguousarray(R, dtype=np.uint8).reshape(n, 32)
    nonces = np.ascontiguousarray(nonces, dtype=np.uint8).reshape(n, 2 * L + 3, 32)
    out = np.zeros((n, L + 1, 2, 32), np.uint8)
    for i in range(n):
        br = [(_i(nonces[i, 1 + 2 * j]), _i(nonces[i, 2 + 2 * j])) for j in range(L + 1)]
        pr = prove_item_host(group, K, int(qbar), L, _i(cts[i, 0]), _i(cts[i, 1]), int(values[i]), _i(R[i]),
                             _i(nonces[i, 0]), br)
        out[i] = np.frombuffer(b"".join(c.to_bytes(32, "big") + v.to_bytes(32, "big") for c, v in pr),
                               np.uint8).reshape(L + 1, 2, 32)
    return out


def verify_host(group, key, qbar: int, limit: int, cts, proofs) -> np.ndarray:
    """verify() on the host -> ok (n,) bool."""
    L = _limit(limit)
    K = _key_int(key)
    cts = np.ascontiguousarray(cts, dtype=np.uint8).reshape(-1, 2, 512)
    n = len(cts)
    proofs = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(n, L + 1, 2, 32)
    return np.array([verify_item_host(group, K, int(qbar), L, _i(cts[i, 0]), _i(cts[i, 1]),
                                      [(_i(proofs[i, j, 0]), _i(proofs[i, j, 1])) for j in range(L + 1)])
                     for i in range(n)], dtype=bool)


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def prove(group, key, qbar: int, limit: int, cts, values, R, nonces):
    """-> proofs (n, L+1, 2, 32) for cts (n, 2, 512), values (n,) in 0..L, R (n, 32) and nonces
    (n, 2L+3, 32).  With DeviceBuffers for all four the result is a DeviceBuffer (asynchronous on
    the context's stream), and an item whose value exceeds L gets an all-zero proof, which verify
    rejects; with arrays such a value raises EgError naming the item.  group.ct_encrypt makes the
    fixed-base reads masked scans (same bytes)."""
    L = _limit(limit)
    cols = Columns(group)
    cts = cols.item(cts, (2, 512), "cts")
    values, R = cols.item(values, (), "values"), cols.item(R, (32,), "R")
    nonces = cols.item(nonces, (2 * L + 3, 32), "nonces")
    return cols.call("eg_range_prove", native.buf(key.K_be), native.buf(be32(qbar)), cols.n, L, cts, values, R,
                     nonces, cols.out((L + 1, 2, 32)))[0]


def verify(group, key, qbar: int, limit: int, cts, proofs):
    """-> ok (n,) bool for cts (n, 2, 512) and proofs (n, L+1, 2, 32); DeviceBuffers in, a
    DeviceBuffer of flag bytes out (asynchronous)."""
    L = _limit(limit)
    cols = Columns(group)
    cts, proofs = cols.item(cts, (2, 512), "cts"), cols.item(proofs, (L + 1, 2, 32), "proofs")
    return cols.call("eg_range_verify", native.buf(key.K_be), native.buf(be32(qbar)), cols.n, L, cts, proofs,
                     cols.out((), flag=True))[0]


# ---------------------------------------------------------------------------------------------
# a contest's selection limit on its aggregate, without placeholders
# ---------------------------------------------------------------------------------------------
def _contest_aggregates(group, man, cts: np.ndarray) -> np.ndarray:
    """(nb, nc, 2, 512): (prod alpha, prod beta) over each contest's real selections, one
    prodP_groups call per contest size."""
    nb, nc = cts.shape[0], man.n_contests
    out = np.empty((nb, nc, 2, 512), np.uint8)
    sizes = np.array([c.n_selections for c in man.contests])
    for size in np.unique(sizes):
        ks = np.flatnonzero(sizes == size)
        idx = np.asarray(man.offsets)[ks][:, None] + np.arange(size)[None, :]       # (nk, size)
        sel = cts[:, idx]                                                             # (nb, nk, size, 2, 512)
        g = np.ascontiguousarray(np.transpose(sel, (0, 1, 3, 2, 4))).reshape(-1, 512)  # groups (b, k, comp)
        out[:, ks] = group.prodP_groups(g, nb * len(ks) * 2, int(size)).reshape(nb, len(ks), 2, 512)
    return out


def contest_limit_prove(group, key, qbar: int, man, eb, votes, sel_nonces, nonces) -> np.ndarray:
    """A 0..votes_allowed proof on every contest's aggregate ciphertext (prod alpha, prod beta) over
    its real selections: the contest holds at most votes_allowed votes, undervotes and empty
    contests included, and no placeholder selection takes part (a manifest layout's placeholder
    slots stay out of the aggregate, as they stay out of the tally).

    eb: the EncryptedBallots of man; votes (nb, nsel) the plaintexts the prover claims (the value
    is their sum over the contest's real selections); sel_nonces (nb, nsel, 4, 32) as given to
    batch_encryption (the aggregate's nonce is the sum of the selections' R mod q); nonces
    (nb, nc, 2 Lmax + 3, 32), contest k reading its first 2 L_k + 3 rows, Lmax =
    man.max_votes_allowed.  -> proofs (nb, nc, Lmax + 1, 2, 32), contest k's first L_k + 1 branches
    filled and the rest zero.  Contests are grouped by limit, one prove() call per limit.
    ballot2.encrypt makes whole placeholder-free ballots, these proofs included, in one batch call."""
    nb, nc, Lmax = eb.n, man.n_contests, _limit(man.max_votes_allowed)
    cts = np.ascontiguousarray(eb.cts, dtype=np.uint8).reshape(nb, man.nsel, 2, 512)
    votes = np.ascontiguousarray(votes, dtype=np.uint8).reshape(nb, man.nsel)
    sn = np.ascontiguousarray(sel_nonces, dtype=np.uint8).reshape(nb, man.nsel, 4, 32)
    nonces = np.ascontiguousarray(nonces, dtype=np.uint8).reshape(nb, nc, 2 * Lmax + 3, 32)
    agg = _contest_aggregates(group, man, cts)
    values = np.zeros((nb, nc), np.uint8)
    rsum = np.zeros((nb, nc, 32), np.uint8)
    for k, (o, c) in enumerate(zip(man.offsets, man.contests)):
        values[:, k] = votes[:, o:o + c.n_selections].sum(axis=1)
        for b in range(nb):
            r = sum(_i(sn[b, o + s, 0]) for s in range(c.n_selections)) % group.q
            rsum[b, k] = np.frombuffer(be32(r), np.uint8)
    out = np.zeros((nb, nc, Lmax + 1, 2, 32), np.uint8)
    limits = np.array([_limit(c.votes_allowed) for c in man.contests])
    for L in np.unique(limits):
        ks = np.flatnonzero(limits == L)
        pr = prove(group, key, qbar, int(L), agg[:, ks].reshape(-1, 2, 512), values[:, ks].reshape(-1),
                   rsum[:, ks].reshape(-1, 32), nonces[:, ks, :2 * L + 3].reshape(-1, 2 * L + 3, 32))
        out[:, ks, :L + 1] = pr.reshape(nb, len(ks), L + 1, 2, 32)
    return out


def contest_limit_verify(group, key, qbar: int, man, eb, proofs) -> np.ndarray:
    """-> ok (nb, nc) bool: contest k of ballot b holds at most votes_allowed votes (its aggregate
    over the real selections carries a valid 0..votes_allowed proof).

    For manifests whose ballots set no placeholders this supersedes the fused verifier's
    ok_contest (the constant proof of the padded sum, which an undervoted contest cannot pass);
    ok_sel and the tally still come from Verifier.verify on the same ballots.  Ballots made
    without placeholders from the start are verified and tallied in one batch call, device-resident
    ones included, by ballot2.Verifier2 (include/eg_hip_ballot2.h)."""
    nb, nc, Lmax = eb.n, man.n_contests, _limit(man.max_votes_allowed)
    cts = np.ascontiguousarray(eb.cts, dtype=np.uint8).reshape(nb, man.nsel, 2, 512)
    proofs = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(nb, nc, Lmax + 1, 2, 32)
    agg = _contest_aggregates(group, man, cts)
    ok = np.zeros((nb, nc), bool)
    limits = np.array([_limit(c.votes_allowed) for c in man.contests])
    for L in np.unique(limits):
        ks = np.flatnonzero(limits == L)
        pr = np.ascontiguousarray(proofs[:, ks, :L + 1])
        ok[:, ks] = verify(group, key, qbar, int(L), agg[:, ks].reshape(-1, 2, 512), pr).reshape(nb, len(ks))
    return ok
