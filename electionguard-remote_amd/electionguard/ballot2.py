"""Ballots without placeholder selections (the ElectionGuard 2.0 form): batch encryption,
verification and tally on the GPU (include/eg_hip_ballot2.h).

``ballot`` holds ElectionGuard 1.0's form: every contest padded with votes_allowed placeholder
selections, every selection 0 or 1, the contest's limit a constant proof of the padded sum.  Here
nothing is padded: selection s of contest k carries a 0..option_limit range proof
(``range_proof``), the contest a 0..contest_limit range proof on its aggregate
(prod alpha, prod beta).  Cumulative and score voting, undervotes and empty contests are plain
ballots of this form.

A Manifest2 is a list of (nsel, option_limit, contest_limit) per contest.  With NS = sum nsel, the
per-ballot rows (uint8, big-endian, ballot-major):

  votes (nb, NS)   sel_nonces (nb, SN, 32)   contest_nonces (nb, CN, 32)
  cts (nb, NS, 2, 512)   sproof (nb, SP, 2, 32)   cproof (nb, CP, 2, 32)
  ok_sel (nb, NS)   ok_contest (nb, nc)   tally (NS, 2, 512)

  SP = sum nsel (olimit + 1): selection i of contest k at sp_off[k] + i (olimit[k] + 1)
  SN = sum nsel (2 olimit + 4): at sn_off[k] + i (2 olimit[k] + 4); rows R, u, c_0, v_0, ..., c_L, v_L
  CP = sum (climit + 1): contest k at cp_off[k]
  CN = sum (2 climit + 3): contest k at cn_off[k]; rows u, c_0, v_0, ..., c_L, v_L

``encrypt_host`` / ``verify_host`` restate the header's definitions on CPython ints with
range_proof's host functions and never call the GPU; ``encrypt`` / ``Verifier2.verify`` run the
library on numpy arrays or DeviceBuffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import range_proof as rp
from .core import native
from .core.marshal import Columns, _Col, be32, be_int as _i, ptr, u32p


class Manifest2:
    """Contests (nsel, option_limit, contest_limit); every selection is real and tallied."""

    def __init__(self, contests: Sequence[Tuple[int, int, int]]):
        self.contests = tuple((int(n), int(o), int(c)) for n, o, c in contests)
        if not self.contests:
            raise ValueError("a manifest needs at least one contest")
        for k, (n, o, c) in enumerate(self.contests):
            if n < 1:
                raise ValueError(f"contest {k} has no selections")
            if not (1 <= o <= rp.MAX_LIMIT and 1 <= c <= rp.MAX_LIMIT):
                raise ValueError(f"contest {k}: a limit outside [1, {rp.MAX_LIMIT}]")
        self.nsel = np.array([n for n, _, _ in self.contests], np.uint32)
        self.olimit = np.array([o for _, o, _ in self.contests], np.uint32)
        self.climit = np.array([c for _, _, c in self.contests], np.uint32)

        i64 = lambda a: np.asarray(a, np.int64)
        prefix = lambda counts: np.concatenate([[0], np.cumsum(i64(counts))[:-1]]).astype(np.int64)
        sp, sn = i64(self.nsel) * (i64(self.olimit) + 1), i64(self.nsel) * (2 * i64(self.olimit) + 4)
        cp, cn = i64(self.climit) + 1, 2 * i64(self.climit) + 3
        self._sums = tuple(int(x.sum()) for x in (i64(self.nsel), sp, sn, cp, cn))
        self._offs = tuple(prefix(x) for x in (self.nsel, sp, sn, cp, cn))

    n_contests = property(lambda self: len(self.contests))
    NS = property(lambda self: self._sums[0])
    SP = property(lambda self: self._sums[1])
    SN = property(lambda self: self._sums[2])
    CP = property(lambda self: self._sums[3])
    CN = property(lambda self: self._sums[4])
    first = property(lambda self: self._offs[0])
    sp_off = property(lambda self: self._offs[1])
    sn_off = property(lambda self: self._offs[2])
    cp_off = property(lambda self: self._offs[3])
    cn_off = property(lambda self: self._offs[4])

    @property
    def jobs(self) -> int:
        """One ballot's verifier jobs J = sum (2 olimit nsel + 2 climit)."""
        return int((2 * self.olimit.astype(np.int64) * self.nsel + 2 * self.climit.astype(np.int64)).sum())

    def selections(self):
        """(k, i, s, L, proof row, nonce row) of every selection, in ballot order."""
        for k, (n, o, _) in enumerate(self.contests):
            for i in range(n):
                yield (k, i, int(self.first[k]) + i, o, int(self.sp_off[k]) + i * (o + 1),
                       int(self.sn_off[k]) + i * (2 * o + 4))

    def style(self, indices: Sequence[int]) -> "Manifest2":
        """The sub-manifest of a ballot style: the listed contests, in the order given."""
        return Manifest2([self.contests[int(k)] for k in indices])

    def __eq__(self, other) -> bool:
        return isinstance(other, Manifest2) and self.contests == other.contests

    def __hash__(self) -> int:
        return hash(self.contests)

    def __repr__(self) -> str:
        return f"Manifest2({list(self.contests)})"

    def _shape_args(self):
        return self.n_contests, u32p(self.nsel), u32p(self.olimit), u32p(self.climit)


def chunk_ballots(man: Manifest2) -> int:
    """Ballots per chunk of the library's calls: a chunk holds at most range_proof.CHUNK_JOBS
    verifier jobs (a ballot whose own jobs exceed that is refused)."""
    return max(1, rp.CHUNK_JOBS // man.jobs)


@dataclass
class EncryptedBallots2:
    cts: object     # (nb, NS, 2, 512) uint8, or a DeviceBuffer
    sproof: object  # (nb, SP, 2, 32)
    cproof: object  # (nb, CP, 2, 32)

    @property
    def n(self) -> int:
        return self.cts.shape[0]


def random_votes2(rng: np.random.Generator, man: Manifest2, nb: int) -> np.ndarray:
    """(nb, NS) votes within every limit: per contest a total 0..climit dealt out one mark at a
    time over selections that still have room (undervotes and empty contests included)."""
    v = np.zeros((nb, man.NS), np.uint8)
    for k, (n, o, c) in enumerate(man.contests):
        f = int(man.first[k])
        for b in range(nb):
            for _ in range(int(rng.integers(0, min(c, n * o) + 1))):
                room = np.flatnonzero(v[b, f:f + n] < o)
                v[b, f + int(rng.choice(room))] += 1
    return v


def random_nonces2(rng: np.random.Generator, man: Manifest2, nb: int, q: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32), uniform below q."""
    from .ballot import random_scalars
    return random_scalars(rng, (nb, man.SN), q), random_scalars(rng, (nb, man.CN), q)


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions (no GPU call)
# ---------------------------------------------------------------------------------------------
def _branches(rows, L: int):
    return [(_i(rows[2 * j]), _i(rows[2 * j + 1])) for j in range(L + 1)]


def _pairs(pr) -> np.ndarray:
    return np.frombuffer(b"".join(be32(c) + be32(v) for c, v in pr), np.uint8).reshape(-1, 2, 32)


def _elem(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(512, "big"), np.uint8)


def check_votes(man: Manifest2, votes: np.ndarray) -> None:
    """ValueError naming the first ballot and contest over a limit (and the selection, when a
    vote is the cause), as eg_encrypt_ballots_v2 does."""
    votes = np.asarray(votes).reshape(-1, man.NS)
    for b in range(len(votes)):
        for k, (n, o, c) in enumerate(man.contests):
            f = int(man.first[k])
            for i in range(n):
                if votes[b, f + i] > o:
                    raise ValueError(f"ballot {b} contest {k} selection {i} holds {int(votes[b, f + i])}, "
                                     f"above its option limit {o}")
            if int(votes[b, f:f + n].sum()) > c:
                raise ValueError(f"ballot {b} contest {k} holds {int(votes[b, f:f + n].sum())}, "
                                 f"above its contest limit {c}")


def encrypt_host(group, key, qbar: int, man: Manifest2, votes, sel_nonces, contest_nonces) -> EncryptedBallots2:
    """encrypt() on the host, same layouts; raises ValueError on a vote or a sum over its limit."""
    p, q, g, K = group.p, group.q, group.g, rp._key_int(key)
    votes = np.ascontiguousarray(votes, np.uint8).reshape(-1, man.NS)
    nb = len(votes)
    check_votes(man, votes)
    sn = np.ascontiguousarray(sel_nonces, np.uint8).reshape(nb, man.SN, 32)
    cn = np.ascontiguousarray(contest_nonces, np.uint8).reshape(nb, man.CN, 32)
    cts = np.zeros((nb, man.NS, 2, 512), np.uint8)
    sproof = np.zeros((nb, man.SP, 2, 32), np.uint8)
    cproof = np.zeros((nb, man.CP, 2, 32), np.uint8)
    for b in range(nb):
        A, B = [1] * man.n_contests, [1] * man.n_contests
        Rs, Ms = [0] * man.n_contests, [0] * man.n_contests
        for k, i, s, L, pr, nr in man.selections():
            m, R = int(votes[b, s]), _i(sn[b, nr])
            alpha, beta = pow(g, R, p), pow(K, R, p) * pow(g, m, p) % p
            cts[b, s, 0], cts[b, s, 1] = _elem(alpha), _elem(beta)
            proof = rp.prove_item_host(group, K, int(qbar), L, alpha, beta, m, R, _i(sn[b, nr + 1]),
                                       _branches(sn[b, nr + 2:nr + 2 * L + 4], L))
            sproof[b, pr:pr + L + 1] = _pairs(proof)
            A[k], B[k], Rs[k], Ms[k] = A[k] * alpha % p, B[k] * beta % p, (Rs[k] + R) % q, Ms[k] + m
        for k, (_, _, L) in enumerate(man.contests):
            cr, nr = int(man.cp_off[k]), int(man.cn_off[k])
            proof = rp.prove_item_host(group, K, int(qbar), L, A[k], B[k], Ms[k], Rs[k], _i(cn[b, nr]),
                                       _branches(cn[b, nr + 1:nr + 2 * L + 3], L))
            cproof[b, cr:cr + L + 1] = _pairs(proof)
    return EncryptedBallots2(cts, sproof, cproof)


def verify_host(group, key, qbar: int, man: Manifest2, eb: EncryptedBallots2, cast=None, with_tally: bool = True):
    """Verifier2.verify on the host -> ok_sel (nb, NS) bool, ok_contest (nb, nc) bool, tally
    (NS, 2, 512) or None."""
    p, K = group.p, rp._key_int(key)
    cts = np.ascontiguousarray(eb.cts, np.uint8).reshape(-1, man.NS, 2, 512)
    nb = len(cts)
    sproof = np.ascontiguousarray(eb.sproof, np.uint8).reshape(nb, man.SP, 2, 32)
    cproof = np.ascontiguousarray(eb.cproof, np.uint8).reshape(nb, man.CP, 2, 32)
    cast = np.ones(nb, bool) if cast is None else np.asarray(cast).reshape(nb) != 0
    ok_sel, ok_con = np.zeros((nb, man.NS), bool), np.zeros((nb, man.n_contests), bool)
    tally = [[1, 1] for _ in range(man.NS)]
    for b in range(nb):
        A, B = [1] * man.n_contests, [1] * man.n_contests
        valid = [True] * man.n_contests
        for k, i, s, L, pr, _ in man.selections():
            alpha, beta = _i(cts[b, s, 0]), _i(cts[b, s, 1])
            ok_sel[b, s] = rp.verify_item_host(group, K, int(qbar), L, alpha, beta,
                                               _branches(sproof[b, pr:pr + L + 1].reshape(-1, 32), L))
            valid[k] &= rp.valid_residue_host(group, alpha) and rp.valid_residue_host(group, beta)
            A[k], B[k] = A[k] * alpha % p, B[k] * beta % p
            if cast[b]:
                tally[s] = [tally[s][0] * alpha % p, tally[s][1] * beta % p]
        for k, (_, _, L) in enumerate(man.contests):
            cr = int(man.cp_off[k])
            ok_con[b, k] = valid[k] and rp.verify_item_host(group, K, int(qbar), L, A[k], B[k],
                                                            _branches(cproof[b, cr:cr + L + 1].reshape(-1, 32), L))
    out = np.stack([np.stack([_elem(a), _elem(bb)]) for a, bb in tally]) if with_tally else None
    return ok_sel, ok_con, out


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def encrypt(group, key, qbar: int, man: Manifest2, votes, sel_nonces, contest_nonces) -> EncryptedBallots2:
    """votes (nb, NS), sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32) -> EncryptedBallots2.
    With DeviceBuffers for all three the results are DeviceBuffers (asynchronous on the context's
    stream) and a vote or a contest sum over its limit gives all-zero proof rows for that
    selection or contest, which the verifier rejects; with arrays it raises EgError naming the
    ballot and contest.  group.ct_encrypt makes the fixed-base reads masked scans (same bytes)."""
    cols = Columns(group)
    votes = cols.item(votes, (man.NS,), "votes")
    sn = cols.item(sel_nonces, (man.SN, 32), "sel_nonces")
    cn = cols.item(contest_nonces, (man.CN, 32), "contest_nonces")
    cts, sp, cp = cols.call("eg_encrypt_ballots_v2", native.buf(key.K_be), native.buf(be32(qbar)), cols.n,
                            *man._shape_args(), votes, sn, cn, cols.out((man.NS, 2, 512)), cols.out((man.SP, 2, 32)),
                            cols.out((man.CP, 2, 32)))
    return EncryptedBallots2(cts, sp, cp)


class Verifier2:
    """Proof verification + homomorphic tally of placeholder-free ballots."""

    def __init__(self, group, key, qbar: int, man: Manifest2):
        self.group, self.key, self.qbar, self.man = group, key, int(qbar), man

    def verify(self, eb: EncryptedBallots2, cast=None, with_tally: bool = True):
        """-> ok_sel (nb, NS), ok_contest (nb, nc), tally (NS, 2, 512) or None: bool arrays and a
        uint8 array for array ballots, DeviceBuffers (flag bytes; asynchronous) for DeviceBuffer
        ballots.  cast (nb,) flags (None: all cast): every ballot is verified, only the cast ones
        are tallied."""
        man, g = self.man, self.group
        cols = Columns(g)
        cts = cols.item(eb.cts, (man.NS, 2, 512), "cts")
        sp = cols.item(eb.sproof, (man.SP, 2, 32), "sproof")
        cp = cols.item(eb.cproof, (man.CP, 2, 32), "cproof")
        cm = _Col() if cast is None else cols.item(cast, (), "cast", host=lambda c: np.asarray(c).reshape(-1) != 0)
        tally = _Col()   # one per call, not per item: allocated here
        if with_tally:
            shape = (man.NS, 2, 512)
            tally.value = g.device_empty(shape, np.uint8) if cols.device else np.zeros(shape, np.uint8)
            tally.arg = tally.value.ptr if cols.device else ptr(tally.value)
        ok_s, ok_c = cols.call("eg_verify_ballots_v2", native.buf(self.key.K_be), native.buf(be32(self.qbar)), cols.n,
                               *man._shape_args(), cts, sp, cp, cm, cols.out((man.NS,), flag=True),
                               cols.out((man.n_contests,), flag=True), tally)
        return ok_s, ok_c, tally.value
