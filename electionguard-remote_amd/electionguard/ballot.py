"""Batched ballot encryption, verification and tally accumulation on the GPU.

Replaces the three in-process hot loops of the reference's end-to-end driver
(src/test/java/electionguard/workflow/RunRemoteWorkflowTest.java):

  * ``batchEncryption(group, ..., true, 11, "createdBy", CheckType.None)``   :140-141
  * ``runAccumulateBallots(group, ...)``                                     :151
  * ``new Verifier(record, 11).verify()``                                   :179-182

Data layout (device and host, big-endian bytes, ballot-major; see include/eg_hip.h):
  cts    (nb, nsel, 2, 512)  ElGamal (pad alpha, data beta) per selection
  rproof (nb, nsel, 4, 32)   disjunctive 0/1 proof (c0, v0, c1, v1), compact form
  cproof (nb, nc, 2, 32)     contest selection-limit proof (c, v)
Selections are contest-major with the placeholder selection(s) last in each contest.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from .core import native
from .core.group import GroupContext, p_bytes, q_bytes
from .core.marshal import call, ptr, u32p


@dataclass(frozen=True)
class Manifest:
    """Synthetic manifest shape (RandomBallotProvider input, RunRemoteWorkflowTest.java:133)."""
    n_contests: int = 4
    n_selections: int = 5     # real selections per contest
    votes_allowed: int = 1    # = number of placeholder selections per contest

    @property
    def spc(self) -> int:
        return self.n_selections + self.votes_allowed

    @property
    def nsel(self) -> int:
        return self.n_contests * self.spc

    @property
    def n_real(self) -> int:
        return self.n_contests * self.n_selections

    # what lets a Manifest stand wherever an ElectionManifest does
    @property
    def contests(self) -> Tuple["Contest", ...]:
        return (Contest(self.n_selections, self.votes_allowed),) * self.n_contests

    @property
    def offsets(self) -> np.ndarray:
        return np.arange(self.n_contests, dtype=np.int64) * self.spc

    @property
    def real_index(self) -> np.ndarray:
        return (self.offsets[:, None] + np.arange(self.n_selections, dtype=np.int64)[None, :]).reshape(-1)

    @property
    def max_votes_allowed(self) -> int:
        return self.votes_allowed

    @property
    def spc_list(self) -> np.ndarray:
        return np.full(self.n_contests, self.spc, dtype=np.uint32)

    @property
    def placeholders(self) -> np.ndarray:
        return np.full(self.n_contests, self.votes_allowed, dtype=np.uint32)

    @property
    def limits(self) -> np.ndarray:
        return self.placeholders


@dataclass(frozen=True)
class Contest:
    """One contest of an ElectionManifest: n_selections real selections followed by
    votes_allowed placeholder selections; its constant proof's limit is votes_allowed."""
    n_selections: int
    votes_allowed: int = 1

    @property
    def spc(self) -> int:
        return self.n_selections + self.votes_allowed


class ElectionManifest:
    """A manifest whose contests differ in size (a vote-for-1 race among 3, a vote-for-3 board
    race among 8, a yes/no measure).  Contest k's selections start at offsets[k] of a ballot's
    nsel selections, its real selections first; real_index lists the real selections' positions
    in tally order (contest-major).  Ballots of an ElectionManifest go through the
    eg_*_ballots_manifest entry points (include/eg_hip_manifest.h)."""

    def __init__(self, contests: Sequence[Union[Contest, Tuple[int, int]]]):
        self.contests: Tuple[Contest, ...] = tuple(c if isinstance(c, Contest) else Contest(*c) for c in contests)
        if not self.contests:
            raise ValueError("a manifest needs at least one contest")
        for c in self.contests:
            if c.n_selections < 1 or c.votes_allowed < 0:
                raise ValueError(f"bad contest {c}")
        self.spc_list = np.array([c.spc for c in self.contests], dtype=np.uint32)
        self.placeholders = np.array([c.votes_allowed for c in self.contests], dtype=np.uint32)
        self.limits = self.placeholders.copy()
        self.offsets = np.concatenate([[0], np.cumsum(self.spc_list.astype(np.int64))[:-1]]).astype(np.int64)
        self.real_index = np.concatenate([o + np.arange(c.n_selections, dtype=np.int64)
                                          for o, c in zip(self.offsets, self.contests)])

    @property
    def n_contests(self) -> int:
        return len(self.contests)

    @property
    def nsel(self) -> int:
        return int(self.spc_list.sum())

    @property
    def n_real(self) -> int:
        return len(self.real_index)

    @property
    def max_votes_allowed(self) -> int:
        return max(c.votes_allowed for c in self.contests)

    def style(self, contest_indices: Sequence[int]) -> "ElectionManifest":
        """The sub-manifest of a ballot style: the listed contests of this manifest, in the
        order given.  A style's ballots are verified as their own batch and the per-style
        tallies joined by merge_style_tallies."""
        return ElectionManifest([self.contests[int(k)] for k in contest_indices])

    def __eq__(self, other) -> bool:
        return isinstance(other, ElectionManifest) and self.contests == other.contests

    def __hash__(self) -> int:
        return hash(self.contests)

    def __repr__(self) -> str:
        return f"ElectionManifest({[(c.n_selections, c.votes_allowed) for c in self.contests]})"


AnyManifest = Union[Manifest, ElectionManifest]


def _entry(man: AnyManifest, base: str, verify: bool) -> Tuple[str, tuple]:
    """The ballot entry point of man's type (a host name; its device variant adds "_dev") and the
    shape arguments that follow nballots: scalars for a Manifest, per-contest tables for an
    ElectionManifest."""
    if isinstance(man, ElectionManifest):
        tables = (man.placeholders, man.limits) if verify else ()
        return base + "_manifest", (man.n_contests, u32p(man.spc_list), *map(u32p, tables))
    return base, (man.n_contests, man.spc) + ((man.votes_allowed, man.votes_allowed) if verify else ())


@dataclass
class EncryptedBallots:
    cts: np.ndarray     # (nb, nsel, 2, 512) uint8
    rproof: np.ndarray  # (nb, nsel, 4, 32) uint8
    cproof: np.ndarray  # (nb, nc, 2, 32) uint8

    @property
    def n(self) -> int:
        return self.cts.shape[0]

    def slice(self, a: int, b: int) -> "EncryptedBallots":
        return EncryptedBallots(self.cts[a:b], self.rproof[a:b], self.cproof[a:b])


def random_scalars(rng: np.random.Generator, shape, q: int) -> np.ndarray:
    """Uniform 256-bit big-endian scalars in [0, q) (q = 2^256 - 189 for EG)."""
    out = rng.integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)
    flat = out.reshape(-1, 32)
    qb = np.frombuffer(q_bytes(q), dtype=np.uint8)
    q_top = int.from_bytes(bytes(qb[:8]), "big")
    # rows >= q are re-drawn (probability ~2^-248 for the EG q).  The top 64 bits decide every
    # row except those equal to q's top word, which are compared byte by byte.
    while True:
        top = flat[:, :8].copy().view(">u8").ravel()
        ge = top > q_top
        for i in np.flatnonzero(top == q_top):
            ge[i] = bytes(flat[i]) >= bytes(qb)
        if not ge.any():
            return out
        flat[ge] = rng.integers(0, 256, size=(int(ge.sum()), 32), dtype=np.uint8)


def random_votes(rng: np.random.Generator, man: AnyManifest, nb: int) -> np.ndarray:
    """Manifest: one-hot vote over the real selections of each contest (placeholders 0).
    ElectionManifest: per contest 0..votes_allowed distinct real selections voted, and as many
    placeholders set as votes were left unused, so every contest sums to its limit."""
    if isinstance(man, ElectionManifest):
        v = np.zeros((nb, man.nsel), dtype=np.uint8)
        for o, c in zip(man.offsets, man.contests):
            for b in range(nb):
                k = int(rng.integers(0, min(c.votes_allowed, c.n_selections) + 1))
                v[b, o + rng.choice(c.n_selections, size=k, replace=False)] = 1
                v[b, o + c.n_selections: o + c.n_selections + (c.votes_allowed - k)] = 1
        return v
    v = np.zeros((nb, man.n_contests, man.spc), dtype=np.uint8)
    pick = rng.integers(0, man.n_selections, size=(nb, man.n_contests))
    np.put_along_axis(v, pick[..., None], 1, axis=2)
    return v.reshape(nb, man.nsel)


class ElectionKey:
    """The joint election key K: registers its fixed-base table (window_bits wide) on a
    GroupContext.  Every ballot call passes K itself, and the library sets it under the ctx lock
    for that call, so threads using different keys on one shared context cannot mix them up."""

    def __init__(self, group: GroupContext, K: int, window_bits: int = 8):
        self.group, self.K, self.window_bits = group, int(K), window_bits
        self._K_be = p_bytes(K)
        self.ensure()

    @property
    def K_be(self) -> bytes:
        return self._K_be

    def ensure(self) -> None:
        """(Re)build K's table at this key's width (a no-op when the ctx already holds it)."""
        native.check(self.group._lib, "eg_set_election_key",
                     self.group._lib.eg_set_election_key(self.group.handle, native.buf(self._K_be),
                                                         self.window_bits))


def batch_encryption(group: GroupContext, key: ElectionKey, qbar: int, man: AnyManifest, votes: np.ndarray,
                     sel_nonces: np.ndarray, contest_nonces: np.ndarray) -> EncryptedBallots:
    """Encrypt nb ballots with injected nonces (batchEncryption, RunRemoteWorkflowTest.java:140-141).

    votes (nb, nsel) in {0,1}; sel_nonces (nb, nsel, 4, 32) = (R, u, c_fake, v_fake);
    contest_nonces (nb, nc, 32).  Deterministic given the nonces.
    """
    nb = votes.shape[0]
    votes = np.ascontiguousarray(votes, dtype=np.uint8).reshape(nb, man.nsel)
    sn = np.ascontiguousarray(sel_nonces, dtype=np.uint8).reshape(nb, man.nsel, 4, 32)
    cn = np.ascontiguousarray(contest_nonces, dtype=np.uint8).reshape(nb, man.n_contests, 32)
    cts = np.empty((nb, man.nsel, 2, 512), dtype=np.uint8)
    rp = np.empty((nb, man.nsel, 4, 32), dtype=np.uint8)
    cp = np.empty((nb, man.n_contests, 2, 32), dtype=np.uint8)
    if nb:
        name, shape = _entry(man, "eg_encrypt_ballots", verify=False)
        call(group, name, native.buf(key.K_be), native.buf(q_bytes(qbar)), nb, *shape, ptr(votes), ptr(sn), ptr(cn),
             ptr(cts), ptr(rp), ptr(cp))
    return EncryptedBallots(cts, rp, cp)


def batch_encryption_device(group: GroupContext, key: ElectionKey, qbar: int, man: AnyManifest, nb: int, d_votes: int,
                            d_sel_nonces: int, d_contest_nonces: int, d_cts: int, d_rproof: int,
                            d_cproof: int) -> None:
    """batch_encryption on device pointers (e.g. torch tensors' data_ptr()): the same
    layouts, inputs and outputs resident in HBM (eg_encrypt_ballots_dev)."""
    if nb:
        name, shape = _entry(man, "eg_encrypt_ballots", verify=False)
        call(group, name + "_dev", native.buf(key.K_be), native.buf(q_bytes(qbar)), nb, *shape, d_votes, d_sel_nonces,
             d_contest_nonces, d_cts, d_rproof, d_cproof)


class Verifier:
    """Ballot-proof verification + homomorphic tally (Verifier.verify / runAccumulateBallots)."""

    def __init__(self, group: GroupContext, key: ElectionKey, qbar: int, man: AnyManifest):
        self.group, self.key, self.qbar, self.man = group, key, int(qbar), man
        self._qb = q_bytes(qbar)

    def verify(self, eb: EncryptedBallots, with_tally: bool = True,
               cast: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """-> ok_sel (nb, nsel) bool, ok_contest (nb, nc) bool, tally (n_real, 2, 512) or None.

        cast (nb,) bool (None = all cast): every ballot is verified, only the cast ones are
        tallied (runAccumulateBallots counts cast ballots; spoiled ones are decrypted one by one,
        RunRemoteDecryptor.java:264-269)."""
        man, g = self.man, self.group
        nb = eb.n
        cts = np.ascontiguousarray(eb.cts, dtype=np.uint8)
        rp = np.ascontiguousarray(eb.rproof, dtype=np.uint8)
        cp = np.ascontiguousarray(eb.cproof, dtype=np.uint8)
        cm = None if cast is None else np.ascontiguousarray(np.asarray(cast).reshape(nb) != 0, dtype=np.uint8)
        ok_s = np.zeros((nb, man.nsel), dtype=np.uint8)
        ok_c = np.zeros((nb, man.n_contests), dtype=np.uint8)
        tally = np.empty((man.n_real, 2, 512), dtype=np.uint8) if with_tally else None
        name, shape = _entry(man, "eg_verify_ballots", verify=True)
        call(g, name, native.buf(self.key.K_be), native.buf(self._qb), nb, *shape, ptr(cts), ptr(rp), ptr(cp),
             ptr(cm) if cm is not None else None, ptr(ok_s), ptr(ok_c), ptr(tally) if tally is not None else None)
        return ok_s.astype(bool), ok_c.astype(bool), tally

    def verify_device(self, d_cts: int, d_rproof: int, d_cproof: int, nb: int, d_ok_sel: int, d_ok_con: int,
                      d_tally: Optional[int], d_cast: Optional[int] = None) -> None:
        """Asynchronous verify on device pointers (e.g. torch CUDA tensors' data_ptr()); d_cast
        (nb bytes, 0 = spoiled) as verify's cast."""
        name, shape = _entry(self.man, "eg_verify_ballots", verify=True)
        call(self.group, name + "_dev", native.buf(self.key.K_be), native.buf(self._qb), nb, *shape, d_cts, d_rproof,
             d_cproof, d_cast, d_ok_sel, d_ok_con, d_tally)


def accumulate_tally(group: GroupContext, man: AnyManifest, eb: EncryptedBallots,
                     cast: Optional[np.ndarray] = None) -> np.ndarray:
    """runAccumulateBallots without verification: per real selection, prod pad / prod data over the
    cast ballots (cast (nb,) bool, None = all)."""
    if cast is not None:
        eb = EncryptedBallots(eb.cts[np.asarray(cast, bool)], eb.rproof[np.asarray(cast, bool)],
                              eb.cproof[np.asarray(cast, bool)])
    nb = eb.n
    sel = eb.cts.reshape(nb, man.nsel, 2, 512)[:, man.real_index]
    # groups ordered (contest, selection, component), elements over ballots
    g = np.ascontiguousarray(np.transpose(sel, (1, 2, 0, 3))).reshape(-1, 512)
    out = group.prodP_groups(g, man.n_real * 2, nb)
    return out.reshape(man.n_real, 2, 512)


def merge_style_tallies(group: GroupContext, man: ElectionManifest,
                        parts: Sequence[Tuple[Sequence[int], np.ndarray]]) -> np.ndarray:
    """Join per-style tallies into the full manifest's (n_real, 2, 512) tally.  parts holds, per
    ballot style, the contest indices given to man.style() and the tally of that style's batch;
    a contest's selections are multiplied over every style that carries it (multP_batch), and
    contests that no style covers stay 1 (the empty product)."""
    real_off = np.concatenate([[0], np.cumsum([c.n_selections for c in man.contests])]).astype(np.int64)
    out = np.zeros((man.n_real, 2, 512), dtype=np.uint8)
    out[:, :, 511] = 1
    for contest_indices, tally in parts:
        rows = np.concatenate([np.arange(real_off[int(k)], real_off[int(k) + 1]) for k in contest_indices]) \
            if len(contest_indices) else np.zeros(0, np.int64)
        t = np.ascontiguousarray(tally, dtype=np.uint8).reshape(-1, 2, 512)
        if t.shape[0] != len(rows):
            raise ValueError(f"style {list(contest_indices)} has {len(rows)} real selections, its tally {t.shape[0]}")
        if len(rows):
            prod = group.multP_batch(np.ascontiguousarray(out[rows]).reshape(-1, 512), t.reshape(-1, 512))
            out[rows] = np.asarray(prod).reshape(-1, 2, 512)
    return out
