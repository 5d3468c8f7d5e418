"""Pre-encrypted (print-at-home, vote-by-mail) ballots: made before anyone votes, recorded from
the codes a voter marked, and checked against the published hashes (include/eg_hip_preencrypt.h).

Contest k owns spc_k = m_k + limit_k slots from off_k, real selections first.  It has spc_k
selection vectors of spc_k components: vector i < m_k is the choice "selection i", vector
i >= m_k null vector i - m_k (the unused vote that sets placeholder i - m_k); vector i encrypts
the unit vector e_i over the contest's slots.  With H = core.hashing.hash_elems (no Q-bar
prefix), V = sum spc_k^2 and voff_k = sum_{k' < k} spc_k'^2:

  w(k,i,j)   = voff_k + i spc_k + j
  rho[b,w]   = H(Q xi_b, Q 4, Q w)
  component  = (g^rho, K^rho g^[i = j])
  e[b,w]     = H(P alpha, P beta)
  psi[b,k,i] = H(Q dcon[k], Q e[b,w(k,i,0)], ..., Q e[b,w(k,i,spc_k-1)])
  Omega(psi) = the last code_bytes bytes of psi
  sorted     = the contest's psi ascending (ties to the lower i); perm[b, off_k + r] the vector at rank r
  unique[b]  = no contest of the ballot has two vectors with one short code
  chi[b,k]   = H(Q dcon[k], Q sorted[b,off_k], ..., Q sorted[b,off_k+spc_k-1])
  C[b]       = H(Q ballot_id[b], Q manifest_hash, Q chi[b,0], ..., Q chi[b,nc-1])

C enters codes.chain_codes where the ballot hash B does.  Recording takes the encryptor's votes
(slot off_k + i set: vector i chosen, null vectors included): the ballot's encryption nonce of slot
off_k + j is the sum of the chosen vectors' rho[b, w(k,i,j)], its other nonces are codes' N_sel /
N_con, so the unchanged encryptor yields a ballot whose ciphertexts are the slot-wise products of
the chosen vectors.  Published per contest: the sorted list and the limit_k chosen vectors in
ascending rank with their ranks and short codes.

The ``*_host`` functions restate the definitions on CPython integers and never touch the GPU;
preencrypt_ballots, record_ballots and verify_recorded run them on the device
(csrc/eg_preencrypt.hpp), on numpy arrays or DeviceBuffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .ballot import AnyManifest, ElectionKey, EncryptedBallots, batch_encryption, batch_encryption_device
from .codes import ManifestHashes
from .core import native
from .core.group import DeviceBuffer, GroupContext
from .core.hashing import hash_elems
from .core.marshal import Columns, be32_row as _b32, be_int as _i, q_row, rows32, u32p

MAX_SPC = 64           # EG_PRE_MAX_SPC
CHUNK_CTS = 1 << 18    # EG_PRE_CHUNK_CTS: component ciphertexts per chunk


@dataclass(frozen=True)
class PreShape:
    """Per-contest layout of a manifest's pre-encrypted ballots."""
    spc: Tuple[int, ...]
    limits: Tuple[int, ...]
    off: Tuple[int, ...]    # first slot (= first vector)
    voff: Tuple[int, ...]   # first component
    soff: Tuple[int, ...]   # first chosen component of a recorded ballot
    toff: Tuple[int, ...]   # first chosen vector of a recorded ballot
    nsel: int
    V: int
    S: int
    T: int

    @property
    def nc(self) -> int:
        return len(self.spc)


def pre_shape(man: AnyManifest) -> PreShape:
    spc = tuple(int(x) for x in man.spc_list)
    lim = tuple(int(x) for x in man.limits)
    off, voff, soff, toff = [], [], [], []
    o = v = s = t = 0
    for m, L in zip(spc, lim):
        off.append(o), voff.append(v), soff.append(s), toff.append(t)
        o, v, s, t = o + m, v + m * m, s + L * m, t + L
    return PreShape(spc, lim, tuple(off), tuple(voff), tuple(soff), tuple(toff), o, v, s, t)


def ballots_per_chunk(man: AnyManifest) -> int:
    """Ballots eg_preencrypt_ballots handles per chunk."""
    return max(1, CHUNK_CTS // pre_shape(man).V)


@dataclass
class PreEncrypted:
    """What eg_preencrypt_ballots yields for nb ballots."""
    sorted: np.ndarray                   # (nb, nsel, 32) the contests' sorted vector hashes
    perm: np.ndarray                     # (nb, nsel) u32: the vector at each rank
    codes: np.ndarray                    # (nb, nsel) u32: each vector's short code, in vector order
    unique: np.ndarray                   # (nb,) u8: 0 = re-seed this ballot
    conf: np.ndarray                     # (nb, 32) confirmation hashes C
    chash: Optional[np.ndarray] = None   # (nb, nc, 32) contest hashes chi
    vec_cts: Optional[np.ndarray] = None  # (nb, V, 2, 512) the component ciphertexts


@dataclass
class RecordedBallots:
    """A recorded pre-encrypted ballot batch: the ballots and what is published with them."""
    ballots: Optional[EncryptedBallots]
    sel_vecs: np.ndarray     # (nb, S, 2, 512) the chosen vectors, ascending rank per contest
    sel_rank: np.ndarray     # (nb, T) u32
    sel_codes: np.ndarray    # (nb, T) u32
    ok: np.ndarray           # (nb, nc) u8: 0 = the contest's votes could not be recorded
    sorted: np.ndarray       # (nb, nsel, 32)
    sel_nonces: Optional[np.ndarray] = None       # (nb, nsel, 4, 32) private: the encryptor's input
    contest_nonces: Optional[np.ndarray] = None   # (nb, nc, 32)


@dataclass
class PreencryptedRecord:
    """The pre-encryption part of an election record (verify_election_record(preencrypted=...))."""
    sel_vecs: np.ndarray
    sel_rank: np.ndarray
    sel_codes: np.ndarray
    sorted: np.ndarray
    conf: np.ndarray
    code_bytes: int = 2


# ---------------------------------------------------------------------------------------------
# host mirrors of the definitions
# ---------------------------------------------------------------------------------------------
def _p512(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(512, "big"), np.uint8)


def short_code(psi: int, code_bytes: int) -> int:
    return int(psi) & ((1 << (8 * code_bytes)) - 1)


def component_nonce_host(q: int, xi: int, w: int, fmt: str = "fixed") -> int:
    return hash_elems(q, ("Q", xi), ("Q", 4), ("Q", w), fmt=fmt)


def vector_cts_host(p: int, q: int, g: int, K: int, man: AnyManifest, ballot_nonces, fmt: str = "fixed") -> np.ndarray:
    """-> (nb, V, 2, 512): every component ciphertext of every ballot."""
    sh = pre_shape(man)
    bn = np.ascontiguousarray(ballot_nonces, dtype=np.uint8).reshape(-1, 32)
    out = np.empty((len(bn), sh.V, 2, 512), np.uint8)
    for b in range(len(bn)):
        xi = _i(bn[b])
        for m, vo in zip(sh.spc, sh.voff):
            for i in range(m):
                for j in range(m):
                    w = vo + i * m + j
                    rho = component_nonce_host(q, xi, w, fmt)
                    out[b, w, 0] = _p512(pow(g, rho, p))
                    out[b, w, 1] = _p512(pow(K, rho, p) * (g if i == j else 1) % p)
    return out


def _psi_host(q: int, dcon_k: int, rows, fmt: str) -> int:
    """psi of one vector from its component ciphertext rows (m, 2, 512)."""
    es = [("Q", hash_elems(q, ("P", _i(r[0])), ("P", _i(r[1])), fmt=fmt)) for r in rows]
    return hash_elems(q, ("Q", dcon_k), *es, fmt=fmt)


def _conf_host(q: int, sh: PreShape, dcon, mh: int, bid: int, sorted_b, fmt: str) -> Tuple[List[int], int]:
    chi = [hash_elems(q, ("Q", _i(dcon[k])), *[("Q", _i(sorted_b[o + r])) for r in range(m)], fmt=fmt)
           for k, (m, o) in enumerate(zip(sh.spc, sh.off))]
    return chi, hash_elems(q, ("Q", bid), ("Q", mh), *[("Q", x) for x in chi], fmt=fmt)


def hashes_from_cts_host(q: int, man: AnyManifest, code_bytes: int, hashes: ManifestHashes, ballot_ids, vec_cts,
                         fmt: str = "fixed") -> PreEncrypted:
    """Everything eg_preencrypt_ballots derives from the component ciphertexts (nb, V, 2, 512)."""
    sh = pre_shape(man)
    cts = np.ascontiguousarray(vec_cts, dtype=np.uint8).reshape(-1, sh.V, 2, 512)
    nb = len(cts)
    ids = rows32(ballot_ids, nb, "ballot_ids")
    dcon, mh = rows32(hashes.dcon, sh.nc, "dcon"), _i(q_row(hashes.manifest_hash))
    srt = np.empty((nb, sh.nsel, 32), np.uint8)
    perm = np.empty((nb, sh.nsel), np.uint32)
    codes = np.empty((nb, sh.nsel), np.uint32)
    unique = np.ones(nb, np.uint8)
    conf = np.empty((nb, 32), np.uint8)
    chash = np.empty((nb, sh.nc, 32), np.uint8)
    for b in range(nb):
        for k, (m, o, vo) in enumerate(zip(sh.spc, sh.off, sh.voff)):
            psi = [_psi_host(q, _i(dcon[k]), cts[b, vo + i * m: vo + (i + 1) * m], fmt) for i in range(m)]
            order = sorted(range(m), key=lambda i: (psi[i], i))
            for r, i in enumerate(order):
                srt[b, o + r] = _b32(psi[i])
                perm[b, o + r] = i
            cs = [short_code(x, code_bytes) for x in psi]
            codes[b, o:o + m] = cs
            if len(set(cs)) != m:
                unique[b] = 0
        chi, C = _conf_host(q, sh, dcon, mh, _i(ids[b]), srt[b], fmt)
        chash[b] = np.stack([_b32(x) for x in chi])
        conf[b] = _b32(C)
    return PreEncrypted(srt, perm, codes, unique, conf, chash, cts)


def preencrypt_host(p: int, q: int, g: int, K: int, man: AnyManifest, code_bytes: int, hashes: ManifestHashes,
                    ballot_ids, ballot_nonces, fmt: str = "fixed") -> PreEncrypted:
    return hashes_from_cts_host(q, man, code_bytes, hashes, ballot_ids,
                                vector_cts_host(p, q, g, K, man, ballot_nonces, fmt), fmt)


def chosen_vectors(votes_k, limit: int) -> List[int]:
    """Chosen slot t of a contest: its (t+1)-th set vote; vector 0 where the votes hold fewer
    (the contest is then not ok)."""
    nz = [i for i, v in enumerate(votes_k) if v]
    return [nz[t] if t < len(nz) else 0 for t in range(limit)]


def record_host(p: int, q: int, g: int, K: int, man: AnyManifest, code_bytes: int, hashes: ManifestHashes,
                ballot_nonces, votes, sorted_hashes, fmt: str = "fixed") -> RecordedBallots:
    """eg_preencrypt_record on the host (ballots is None: the encryptor is not restated here)."""
    sh = pre_shape(man)
    votes = np.ascontiguousarray(votes, dtype=np.uint8).reshape(-1, sh.nsel)
    nb = len(votes)
    bn = rows32(ballot_nonces, nb, "ballot_nonces")
    srt = np.ascontiguousarray(sorted_hashes, dtype=np.uint8).reshape(nb, sh.nsel, 32)
    dcon = rows32(hashes.dcon, sh.nc, "dcon")
    sv = np.empty((nb, sh.S, 2, 512), np.uint8)
    rank = np.empty((nb, sh.T), np.uint32)
    codes = np.empty((nb, sh.T), np.uint32)
    sn = np.empty((nb, sh.nsel, 4, 32), np.uint8)
    cn = np.empty((nb, sh.nc, 32), np.uint8)
    ok = np.ones((nb, sh.nc), np.uint8)
    for b in range(nb):
        xi = _i(bn[b])
        for k, (m, L, o, vo, so, to) in enumerate(zip(sh.spc, sh.limits, sh.off, sh.voff, sh.soff, sh.toff)):
            vk = votes[b, o:o + m]
            if int(vk.max()) > 1 or int(vk.sum()) != L:
                ok[b, k] = 0
            lst = [_i(srt[b, o + r]) for r in range(m)]
            rows, psis, ranks, rsum = [], [], [], [0] * m
            for i in chosen_vectors(vk, L):
                rho = [component_nonce_host(q, xi, vo + i * m + j, fmt) for j in range(m)]
                rsum = [(a + r) % q for a, r in zip(rsum, rho)]
                vec = np.stack([np.stack([_p512(pow(g, r, p)), _p512(pow(K, r, p) * (g if i == j else 1) % p)])
                                for j, r in enumerate(rho)])
                psi = _psi_host(q, _i(dcon[k]), vec, fmt)
                rows.append(vec), psis.append(psi)
                ranks.append(lst.index(psi) if psi in lst else m)
            if any(r >= m for r in ranks):
                ok[b, k] = 0
            for pos, t in enumerate(sorted(range(L), key=lambda t: (ranks[t], t))):
                sv[b, so + pos * m: so + (pos + 1) * m] = rows[t]
                rank[b, to + pos] = ranks[t]
                codes[b, to + pos] = short_code(psis[t], code_bytes)
            for j in range(m):
                s = o + j
                sn[b, s, 0] = _b32(rsum[j])
                for t in (1, 2, 3):
                    sn[b, s, t] = _b32(hash_elems(q, ("Q", xi), ("Q", 1), ("Q", 4 * s + t), fmt=fmt))
            cn[b, k] = _b32(hash_elems(q, ("Q", xi), ("Q", 2), ("Q", k), fmt=fmt))
    return RecordedBallots(None, sv, rank, codes, ok, srt, sn, cn)


def vector_product_host(p: int, man: AnyManifest, sel_vecs) -> np.ndarray:
    """-> (nb, nsel, 2, 512): the slot-wise products of each contest's chosen vectors."""
    sh = pre_shape(man)
    sv = np.ascontiguousarray(sel_vecs, dtype=np.uint8).reshape(-1, sh.S, 2, 512)
    out = np.empty((len(sv), sh.nsel, 2, 512), np.uint8)
    for b in range(len(sv)):
        for m, L, o, so in zip(sh.spc, sh.limits, sh.off, sh.soff):
            for j in range(m):
                for c in (0, 1):
                    x = 1
                    for t in range(L):
                        x = x * _i(sv[b, so + t * m + j, c]) % p
                    out[b, o + j, c] = _p512(x)
    return out


def verify_recorded_host(p: int, q: int, man: AnyManifest, code_bytes: int, hashes: ManifestHashes, ballot_ids,
                         sel_vecs, sel_rank, sel_codes, sorted_hashes, cts, conf,
                         fmt: str = "fixed") -> Tuple[np.ndarray, np.ndarray]:
    """The verdict of the pre-encryption check -> ok_contest (nb, nc) bool, ok_conf (nb,) bool."""
    sh = pre_shape(man)
    sv = np.ascontiguousarray(sel_vecs, dtype=np.uint8).reshape(-1, sh.S, 2, 512)
    nb = len(sv)
    rank = np.asarray(sel_rank, np.uint32).reshape(nb, sh.T)
    codes = np.asarray(sel_codes, np.uint32).reshape(nb, sh.T)
    srt = np.ascontiguousarray(sorted_hashes, dtype=np.uint8).reshape(nb, sh.nsel, 32)
    cts = np.ascontiguousarray(cts, dtype=np.uint8).reshape(nb, sh.nsel, 2, 512)
    cf = rows32(conf, nb, "conf")
    ids = rows32(ballot_ids, nb, "ballot_ids")
    dcon, mh = rows32(hashes.dcon, sh.nc, "dcon"), _i(q_row(hashes.manifest_hash))
    okc = np.zeros((nb, sh.nc), bool)
    okb = np.zeros(nb, bool)
    for b in range(nb):
        for k, (m, L, o, so, to) in enumerate(zip(sh.spc, sh.limits, sh.off, sh.soff, sh.toff)):
            good = all(1 <= _i(sv[b, so + x, c]) < p for x in range(L * m) for c in (0, 1))
            lst = [_i(srt[b, o + r]) for r in range(m)]
            good &= all(lst[r - 1] < lst[r] for r in range(1, m))
            rk = [int(rank[b, to + t]) for t in range(L)]
            good &= all(r < m for r in rk) and all(rk[t - 1] < rk[t] for t in range(1, L))
            for t in range(L):
                psi = _psi_host(q, _i(dcon[k]), sv[b, so + t * m: so + (t + 1) * m], fmt)
                good &= rk[t] < m and psi == lst[rk[t]]
                good &= int(codes[b, to + t]) == short_code(psi, code_bytes)
            for j in range(m):
                for c in (0, 1):
                    x = 1
                    for t in range(L):
                        x = x * _i(sv[b, so + t * m + j, c]) % p
                    good &= bytes(_p512(x)) == bytes(cts[b, o + j, c])
            okc[b, k] = good
        okb[b] = _conf_host(q, sh, dcon, mh, _i(ids[b]), srt[b], fmt)[1] == _i(cf[b])
    return okc, okb


# ---------------------------------------------------------------------------------------------
# GPU calls (numpy arrays through the host entry points, DeviceBuffers through the _dev ones)
# ---------------------------------------------------------------------------------------------
def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def preencrypt_ballots(group: GroupContext, key: ElectionKey, man: AnyManifest, hashes: ManifestHashes, ballot_ids,
                       ballot_nonces, code_bytes: int = 2, with_cts: bool = False) -> PreEncrypted:
    """Pre-encrypt nb ballots from their seeds.  Only hashes, orders and codes come back unless
    with_cts asks for the component ciphertexts too.  With ballot_ids and ballot_nonces
    DeviceBuffers every field of the result is a DeviceBuffer (asynchronous on the context's stream)."""
    sh = pre_shape(man)
    nc, nsel = sh.nc, sh.nsel
    cols = Columns(group)
    dcon, mh = cols.once(rows32(hashes.dcon, nc, "dcon")), cols.once(q_row(hashes.manifest_hash))
    bn, ids = cols.item(ballot_nonces, (32,), "ballot_nonces"), cols.item(ballot_ids, (32,), "ballot_ids")
    outs = [cols.out((nsel, 32)), cols.out((nsel,), np.uint32), cols.out((nsel,), np.uint32), cols.out(()),
            cols.out((32,)), cols.out((nc, 32)), cols.out((sh.V, 2, 512), want=with_cts)]
    return PreEncrypted(*cols.call("eg_preencrypt_ballots", native.buf(key.K_be), cols.n, nc, u32p(_u32(man.spc_list)),
                                   code_bytes, dcon, mh, ids, bn, *outs))


def record_parts(group: GroupContext, key: ElectionKey, man: AnyManifest, hashes: ManifestHashes, ballot_nonces,
                 votes, sorted_hashes, code_bytes: int = 2) -> RecordedBallots:
    """eg_preencrypt_record[_dev]: the published parts and the encryptor's nonces (ballots is None)."""
    sh = pre_shape(man)
    nc, nsel = sh.nc, sh.nsel
    cols = Columns(group)
    dcon = cols.once(rows32(hashes.dcon, nc, "dcon"))
    votes = cols.item(votes, (nsel,), "votes")
    bn, srt = cols.item(ballot_nonces, (32,), "ballot_nonces"), cols.item(sorted_hashes, (nsel, 32), "sorted_hashes")
    sv, rank, codes = cols.out((sh.S, 2, 512)), cols.out((sh.T,), np.uint32), cols.out((sh.T,), np.uint32)
    sn, cn, ok = cols.out((nsel, 4, 32)), cols.out((nc, 32)), cols.out((nc,))
    sv, rank, codes, sn, cn, ok = cols.call(
        "eg_preencrypt_record", native.buf(key.K_be), cols.n, nc, u32p(_u32(man.spc_list)), u32p(_u32(man.limits)),
        code_bytes, dcon, bn, votes, srt, sv, rank, codes, sn, cn, ok)
    return RecordedBallots(None, sv, rank, codes, ok, srt.value, sn, cn)


def record_ballots(group: GroupContext, key: ElectionKey, qbar: int, man: AnyManifest, hashes: ManifestHashes,
                   ballot_nonces, votes, sorted_hashes, code_bytes: int = 2) -> RecordedBallots:
    """Record returned ballots: the record entry, then the unchanged encryptor on its nonces.
    DeviceBuffers in (votes, ballot_nonces, sorted_hashes): everything stays in HBM and the
    EncryptedBallots holds DeviceBuffers."""
    sh = pre_shape(man)
    rec = record_parts(group, key, man, hashes, ballot_nonces, votes, sorted_hashes, code_bytes)
    if isinstance(votes, DeviceBuffer):
        nb = votes.nbytes // sh.nsel
        eb = EncryptedBallots(group.device_empty((nb, sh.nsel, 2, 512)), group.device_empty((nb, sh.nsel, 4, 32)),
                              group.device_empty((nb, sh.nc, 2, 32)))
        batch_encryption_device(group, key, qbar, man, nb, votes.ptr, rec.sel_nonces.ptr, rec.contest_nonces.ptr,
                                eb.cts.ptr, eb.rproof.ptr, eb.cproof.ptr)
    else:
        v = np.ascontiguousarray(votes, dtype=np.uint8).reshape(-1, sh.nsel)
        eb = batch_encryption(group, key, qbar, man, v, rec.sel_nonces, rec.contest_nonces)
    rec.ballots = eb
    return rec


def verify_recorded(group: GroupContext, man: AnyManifest, hashes: ManifestHashes, ballot_ids, sel_vecs, sel_rank,
                    sel_codes, sorted_hashes, cts, conf, code_bytes: int = 2):
    """The pre-encryption check -> (ok_contest (nb, nc) bool, ok_conf (nb,) bool); with
    DeviceBuffers for every array -> two DeviceBuffers of flag bytes, asynchronous."""
    sh = pre_shape(man)
    nc, nsel = sh.nc, sh.nsel
    cols = Columns(group)
    dcon, mh = cols.once(rows32(hashes.dcon, nc, "dcon")), cols.once(q_row(hashes.manifest_hash))
    cf, ids = cols.item(conf, (32,), "conf"), cols.item(ballot_ids, (32,), "ballot_ids")
    sv = cols.item(sel_vecs, (sh.S, 2, 512), "sel_vecs")
    rk = cols.item(sel_rank, (sh.T,), "sel_rank", np.uint32)
    cd = cols.item(sel_codes, (sh.T,), "sel_codes", np.uint32)
    srt, ct = cols.item(sorted_hashes, (nsel, 32), "sorted_hashes"), cols.item(cts, (nsel, 2, 512), "cts")
    okc, okb = cols.out((nc,), flag=True), cols.out((), flag=True)
    return tuple(cols.call("eg_preencrypt_verify", cols.n, nc, u32p(_u32(man.spc_list)), u32p(_u32(man.limits)),
                           code_bytes, dcon, mh, ids, sv, rk, cd, srt, ct, cf, okc, okb))
