"""The mixer's side of a verifiable re-encryption shuffle of ciphertext rows
(include/eg_hip_shuffle.h): the independent generators of the Terelius-Wikstrom
proof and the mix itself on the GPU, and the whole protocol restated on CPython ints.

  rows  (N, w, 2, 512): alpha[i,j], beta[i,j], exactly ``ballot2``'s ``eb.cts``
  mix   alpha'[i,j] = alpha[psi(i),j] g^{r[i,j]},  beta'[i,j] = beta[psi(i),j] K^{r[i,j]}
  G     (N + 2, 512): h, h_0 .. h_{N-1}, prod h_i;  gen(k) = X_k^{(p-1)/q} with X_k sixteen raw
        SHA-256 digests of (Q gseed, Q 0x43, Q k, Q t) side by side

  proof (N, 512) pc and chain, c (32), s (3 + w, 32), s_hat and s_prime (N, 32): compact, no commitment
        is published; the verifier recomputes them and the challenge

``generators``, ``mix``, ``prove`` and ``verify`` take numpy arrays (host entry points, which upload
the whole arrays) or DeviceBuffers (the ``_dev`` twins, asynchronous on the context's stream);
``shuffle`` draws psi and every nonce and returns the mixed rows with their proof.  A cascade of
mixers is one ``verify`` call per stage.  The ``*_host`` functions restate the protocol of DESIGN §19
on CPython ints and never call the GPU.  ``mix`` and ``prove`` are variable time and are refused while
``group.ct_pow`` is on; ``generators`` and ``verify`` work on public values and run either way.
"""
from __future__ import annotations

import hashlib
import secrets
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .core import native
from .core.group import p_bytes
from .core.hashing import hash_elems
from .core.marshal import Columns, _is_device, be32, call as _call, ptr

MAX_ROWS, MAX_CELLS = 1 << 20, 1 << 21
TAG_LEAF, TAG_NODE, TAG_SEED, TAG_GEN, TAG_U, TAG_C = 0x40, 0x41, 0x42, 0x43, 0x44, 0x45
FAN = 256
RANGE, RESIDUE, CHALLENGE = 1, 2, 4   # the bits of verify's failed mask


def cofactor(group) -> int:
    return (group.p - 1) // group.q


def _limits(N: int, w: int) -> None:
    if not 0 < N <= MAX_ROWS or w <= 0 or N * w > MAX_CELLS:
        raise ValueError(f"shuffle: {N} rows of width {w}: 1 <= N <= 2^20, w >= 1 and N w <= 2^21 are needed")


# ---------------------------------------------------------------------------------------------
# the GPU calls
# ---------------------------------------------------------------------------------------------
def generators(group, gseed: int, N: int, device: bool = False):
    """G (N + 2, 512) = h, h_0 .. h_{N-1}, prod h_i from the 32-byte seed: a numpy array through
    eg_shuffle_generators, or with ``device`` a DeviceBuffer through eg_shuffle_generators_dev."""
    N = int(N)
    _limits(N, 1)
    cof = native.buf(int(cofactor(group)).to_bytes(512, "big"))
    out = group.device_empty((N + 2, 512)) if device else np.zeros((N + 2, 512), np.uint8)
    _call(group, "eg_shuffle_generators_dev" if device else "eg_shuffle_generators", cof, native.buf(be32(gseed)), N,
          out.ptr if device else ptr(out))
    return out


def _nonce_rows(r):
    if isinstance(r, np.ndarray) and r.dtype == np.uint8:
        return r
    return np.frombuffer(b"".join(be32(x) for row in r for x in row), np.uint8)


def mix(group, K: int, rows, psi, r):
    """rows' (N, w, 2, 512) with row i the re-encryption of row psi(i) under the nonces r (N, w, 32):
    numpy arrays through eg_shuffle_mix (which refuses a psi that is no permutation), DeviceBuffers
    through eg_shuffle_mix_dev (asynchronous on the context's stream; psi is trusted there).  psi: N
    uint32; r on the host may be rows of ints."""
    N, w = _shape_of(rows)
    cols = Columns(group)
    e = cols.item(rows, (w, 2, 512), "rows")
    ps = cols.item(psi, (), "psi", dtype=np.uint32)
    rr = cols.item(r, (w, 32), "r", host=_nonce_rows)
    out, = cols.call("eg_shuffle_mix", native.buf(p_bytes(K)), N, w, e, ps, rr, cols.out((w, 2, 512)))
    return out


def _whole(cols, value, nbytes: int, name: str):
    """An input of the call's kind that is not one row per item: -> (value, pointer)."""
    dev = _is_device(value)
    if dev != bool(cols.device):
        raise TypeError(f"{name}: {'a DeviceBuffer' if cols.device else 'a host array'} is needed here, "
                        "host and device columns do not mix")
    if not dev:
        value = np.ascontiguousarray(value, dtype=np.uint8)
    if value.nbytes != nbytes:
        raise ValueError(f"{name}: expected {nbytes} bytes, got {value.nbytes}")
    return value, (value.ptr if dev else ptr(value))


def _fresh(cols, shape, dtype=np.uint8):
    value = cols.group.device_empty(shape, dtype) if cols.device else np.zeros(shape, dtype)
    return value, (value.ptr if cols.device else ptr(value))


def _shape_of(rows):
    shape = tuple(getattr(rows, "shape", ()))
    if len(shape) != 4 or shape[2:] != (2, 512):
        raise ValueError(f"rows: expected a (N, w, 2, 512) array, got shape {shape}")
    _limits(shape[0], shape[1])
    return shape[0], shape[1]


def _q_rows(x):
    if isinstance(x, np.ndarray) and x.dtype == np.uint8:
        return x
    return np.frombuffer(b"".join(be32(v) for v in np.asarray(x, object).reshape(-1)), np.uint8)


def prove(group, K: int, qbar: int, gseed: int, G, rows, rows2, psi, r, nonces) -> "ShuffleProof":
    """The proof that rows2 is a mix of rows under psi and r (eg_shuffle_prove / _dev).  nonces:
    (4 N + 3 + w, 32) in the order rho, rho^, omega^, omega', omega1, omega2, omega3, omega4, each
    reduced mod q on use; each set must be used for ONE proof.  -> a ShuffleProof of arrays, or of
    DeviceBuffers when the inputs are."""
    N, w = _shape_of(rows)
    cols = Columns(group)
    e = cols.item(rows, (w, 2, 512), "rows")
    e2 = cols.item(rows2, (w, 2, 512), "rows2")
    ps = cols.item(psi, (), "psi", dtype=np.uint32)
    rr = cols.item(r, (w, 32), "r", host=_nonce_rows)
    _, g_arg = _whole(cols, G, (N + 2) * 512, "G")
    _, n_arg = _whole(cols, nonces if _is_device(nonces) else _q_rows(nonces), (4 * N + 3 + w) * 32, "nonces")
    c, c_arg = _fresh(cols, (32,))
    sv, s_arg = _fresh(cols, (3 + w, 32))
    pc, chain, s_hat, s_prime = cols.call("eg_shuffle_prove", native.buf(p_bytes(K)), native.buf(be32(qbar)),
                                          native.buf(be32(gseed)), N, w, g_arg, e, e2, ps, rr, n_arg,
                                          cols.out((512,)), cols.out((512,)), c_arg, s_arg, cols.out((32,)),
                                          cols.out((32,)))
    return ShuffleProof(pc, chain, c, sv, s_hat, s_prime)


def verify(group, K: int, qbar: int, gseed: int, G, rows, rows2, proof: "ShuffleProof", check_inputs: bool = False):
    """-> (ok, failed): a bool and a mask of RANGE, RESIDUE and CHALLENGE for arrays; for DeviceBuffers a
    one-byte and a uint32 DeviceBuffer, asynchronous on the context's stream.  check_inputs: the
    residue test also covers rows (a stage of a cascade that checked its input as the stage before's
    output may leave it out)."""
    N, w = _shape_of(rows)
    cols = Columns(group)
    e = cols.item(rows, (w, 2, 512), "rows")
    e2 = cols.item(rows2, (w, 2, 512), "rows2")
    pc, chain = cols.item(proof.pc, (512,), "pc"), cols.item(proof.chain, (512,), "chain")
    sh, sp = cols.item(proof.s_hat, (32,), "s_hat"), cols.item(proof.s_prime, (32,), "s_prime")
    _, g_arg = _whole(cols, G, (N + 2) * 512, "G")
    _, c_arg = _whole(cols, proof.c, 32, "c")
    _, s_arg = _whole(cols, proof.s, (3 + w) * 32, "s")
    ok, ok_arg = _fresh(cols, (1,))
    failed, f_arg = _fresh(cols, (1,), np.uint32)
    cols.call("eg_shuffle_verify", native.buf(p_bytes(K)), native.buf(be32(qbar)), native.buf(be32(gseed)), N, w,
              g_arg, e, e2, pc, chain, c_arg, s_arg, sh, sp, int(bool(check_inputs)), ok_arg, f_arg)
    if cols.device:
        return ok, failed
    return bool(ok[0]), int(failed[0])


def shuffle(group, K: int, qbar: int, rows, gseed: int, rng=secrets):
    """One mixer's stage: draws psi and every nonce from rng (``secrets``: randbelow and token_bytes),
    derives the generators, mixes and proves.  rows: ``eb.cts`` as it stands, an array or a
    DeviceBuffer.  -> (rows', proof).  The 256-bit nonces are reduced mod q on use."""
    N, w = _shape_of(rows)
    device = _is_device(rows)
    psi = np.arange(N, dtype=np.uint32)
    for i in range(N - 1, 0, -1):
        j = rng.randbelow(i + 1)
        psi[i], psi[j] = psi[j], psi[i]
    r = np.frombuffer(rng.token_bytes(N * w * 32), np.uint8).reshape(N, w, 32)
    nonces = np.frombuffer(rng.token_bytes((4 * N + 3 + w) * 32), np.uint8).reshape(-1, 32)
    if device:
        psi, r, nonces = group.to_device(psi), group.to_device(r), group.to_device(nonces)
    G = generators(group, gseed, N, device=device)
    rows2 = mix(group, K, rows, psi, r)
    return rows2, prove(group, K, qbar, gseed, G, rows, rows2, psi, r, nonces)


# ---------------------------------------------------------------------------------------------
# the protocol on CPython ints (E: N rows of w (alpha, beta) pairs)
# ---------------------------------------------------------------------------------------------
@dataclass
class ShuffleProof:
    """The compact proof: no commitment t is published.  prove and verify hold arrays or
    DeviceBuffers in it, the *_host functions CPython ints."""
    pc: object        # the permutation commitment: (N, 512), or N ints
    chain: object     # the commitment chain: (N, 512), or N ints
    c: object         # (32,), or an int
    s: object         # s1, s2, s3, s4[0..w-1]: (3 + w, 32)
    s_hat: object     # (N, 32)
    s_prime: object   # (N, 32)

    def to_ints(self) -> "ShuffleProof":
        f = lambda a: [int.from_bytes(bytes(x), "big") for x in np.asarray(a).reshape(-1, np.asarray(a).shape[-1])]
        return ShuffleProof(f(self.pc), f(self.chain), f(self.c)[0], f(self.s), f(self.s_hat), f(self.s_prime))

    def to_arrays(self) -> "ShuffleProof":
        f = lambda xs, n: np.frombuffer(b"".join(int(x).to_bytes(n, "big") for x in xs), np.uint8).reshape(-1, n)
        return ShuffleProof(f(self.pc, 512), f(self.chain, 512), f([self.c], 32)[0], f(self.s, 32), f(self.s_hat, 32),
                            f(self.s_prime, 32))


def rows_to_ints(rows) -> list:
    """(N, w, 2, 512) bytes -> N rows of w (alpha, beta) pairs."""
    a = np.asarray(rows, np.uint8)
    return [[tuple(int.from_bytes(bytes(a[i, j, k]), "big") for k in (0, 1)) for j in range(a.shape[1])]
            for i in range(a.shape[0])]


def ints_to_rows(E) -> np.ndarray:
    return np.frombuffer(b"".join(p_bytes(x) for row in E for pair in row for x in pair),
                         np.uint8).reshape(len(E), len(E[0]), 2, 512)


def _H(group, *elems) -> int:
    return hash_elems(group.q, *elems, fmt=group.hash_format)


def _leaf(group, xs) -> int:
    return _H(group, ("Q", TAG_LEAF), *[("P", x) for x in xs])


def tree_host(group, vs: Sequence[int]) -> int:
    """T(v_0 .. v_{n-1}): one tagged hash of up to 256 values, of more the T of the Ts of
    consecutive chunks of 256."""
    vs = list(vs)
    while len(vs) > FAN:
        vs = [tree_host(group, vs[i:i + FAN]) for i in range(0, len(vs), FAN)]
    return _H(group, ("Q", TAG_NODE), ("Q", len(vs)), *[("Q", v) for v in vs])


def _tree_rows(group, rows) -> int:
    return tree_host(group, [_leaf(group, row) for row in rows])


def _flat(E):
    return [[x for pair in row for x in pair] for row in E]


def generators_host(group, gseed: int, N: int) -> List[int]:
    p, q = group.p, group.q
    G = []
    for k in range(N + 1):
        X = b""
        for t in range(16):
            parts = [be32(gseed), be32(TAG_GEN), be32(k), be32(t)]
            if group.hash_format == "minimal":
                parts = [b.lstrip(b"\0") or b"\0" for b in parts]
            X += hashlib.sha256(("|" + "|".join(b.hex().upper() for b in parts) + "|").encode("ascii")).digest()
        G.append(pow(int.from_bytes(X, "big") % p, (p - 1) // q, p))
    if any(x in (0, 1) for x in G):
        raise ValueError("shuffle: a generator is 0 or 1 (take another gseed)")
    prod = 1
    for x in G[1:]:
        prod = prod * x % p
    return G + [prod]


def mix_host(group, K: int, E, psi, r) -> list:
    p, q, g = group.p, group.q, group.g
    if sorted(int(x) for x in psi) != list(range(len(E))):
        raise ValueError("shuffle: psi is no permutation")
    return [[(E[psi[i]][j][0] % p * pow(g, r[i][j] % q, p) % p, E[psi[i]][j][1] % p * pow(K, r[i][j] % q, p) % p)
             for j in range(len(E[0]))] for i in range(len(E))]


def _seed(group, K, qbar, gseed, E, E2, pc) -> int:
    return _H(group, ("Q", qbar), ("Q", TAG_SEED), ("Q", len(E)), ("Q", len(E[0])), ("P", K), ("Q", gseed),
              ("Q", _tree_rows(group, _flat(E))), ("Q", _tree_rows(group, _flat(E2))),
              ("Q", _tree_rows(group, [[x] for x in pc])))


def _challenge(group, y, t1, t2, t3, t4, that, chain) -> int:
    return _H(group, ("Q", y), ("Q", TAG_C), ("P", t1), ("P", t2), ("P", t3),
              ("Q", _tree_rows(group, [list(t) for t in t4])), ("Q", _tree_rows(group, [[x] for x in that])),
              ("Q", _tree_rows(group, [[x] for x in chain])))


def prove_host(group, K: int, qbar: int, gseed: int, G, E, E2, psi, r, nonces) -> ShuffleProof:
    """The prover of DESIGN §19.  nonces: 4 N + 3 + w values in the order rho, rho^, omega^, omega',
    omega1, omega2, omega3, omega4, each reduced mod q on use."""
    p, q, g = group.p, group.q, group.g
    N, w = len(E), len(E[0])
    if len(nonces) != 4 * N + 3 + w or len(G) != N + 2:
        raise ValueError("shuffle: 4 N + 3 + w nonces and N + 2 generators are needed")
    h, hs = G[0] % p, [x % p for x in G[1:N + 1]]
    nn = [int(x) % q for x in nonces]
    rho, rho_hat, om_hat, om_p = nn[:N], nn[N:2 * N], nn[2 * N:3 * N], nn[3 * N:4 * N]
    om1, om2, om3 = nn[4 * N:4 * N + 3]
    om4 = nn[4 * N + 3:]
    pc = [1 % p] * N
    for i in range(N):
        pc[psi[i]] = pow(g, rho[psi[i]], p) * hs[i] % p
    y = _seed(group, K, qbar, gseed, E, E2, pc)
    u = [_H(group, ("Q", y), ("Q", TAG_U), ("Q", j)) for j in range(N)]
    up = [u[psi[i]] for i in range(N)]
    R, U, Rs, chain = 0, 1, [], []
    for i in range(N):
        R, U = (rho_hat[i] + up[i] * R) % q, up[i] * U % q
        Rs.append(R)
        chain.append(pow(g, R, p) * pow(h, U, p) % p)
    rbar, rhat = sum(rho) % q, Rs[-1]
    rtil = sum(a * b for a, b in zip(rho, u)) % q
    rstar = [sum((r[i][j] % q) * up[i] for i in range(N)) % q for j in range(w)]
    t1, t2, t3 = pow(g, om1, p), pow(g, om2, p), pow(g, om3, p)
    for i in range(N):
        t3 = t3 * pow(hs[i], om_p[i], p) % p
    t4 = []
    for j in range(w):
        a, b = pow(g, (q - om4[j]) % q, p), pow(K, (q - om4[j]) % q, p)
        for i in range(N):
            a = a * pow(E2[i][j][0] % p, om_p[i], p) % p
            b = b * pow(E2[i][j][1] % p, om_p[i], p) % p
        t4.append((a, b))
    that = [pow(g, om_hat[i], p) * pow(chain[i - 1] if i else h, om_p[i], p) % p for i in range(N)]
    c = _challenge(group, y, t1, t2, t3, t4, that, chain)
    s = [(om1 + c * rbar) % q, (om2 + c * rhat) % q, (om3 + c * rtil) % q] + \
        [(om4[j] + c * rstar[j]) % q for j in range(w)]
    return ShuffleProof(pc, chain, c, s, [(om_hat[i] + c * rho_hat[i]) % q for i in range(N)],
                        [(om_p[i] + c * up[i]) % q for i in range(N)])


def verify_host(group, K: int, qbar: int, gseed: int, G, E, E2, proof: ShuffleProof, check_inputs: bool = False):
    """-> (ok, failed): failed is a mask of RANGE (c or a response >= q), RESIDUE (an element of E',
    pc or chain, with check_inputs also of E, outside (0, p) or not of order q) and CHALLENGE.  All
    three tests are always made."""
    p, q, g = group.p, group.q, group.g
    N, w = len(E), len(E[0])
    failed = 0
    pc, chain, c = proof.pc, proof.chain, proof.c
    if c >= q or any(x >= q for x in list(proof.s) + list(proof.s_hat) + list(proof.s_prime)):
        failed |= RANGE
    els = [x for row in _flat(E2) for x in row] + list(pc) + list(chain)
    if check_inputs:
        els += [x for row in _flat(E) for x in row]
    if not all(0 < x < p and pow(x, q, p) == 1 for x in els):
        failed |= RESIDUE
    h, hs, hprod = G[0] % p, [x % p for x in G[1:N + 1]], G[N + 1] % p
    s = [x % q for x in proof.s]
    s_hat, s_prime = [x % q for x in proof.s_hat], [x % q for x in proof.s_prime]
    nc = (q - c % q) % q
    y = _seed(group, K, qbar, gseed, E, E2, pc)
    u = [_H(group, ("Q", y), ("Q", TAG_U), ("Q", j)) for j in range(N)]
    U = 1
    for x in u:
        U = U * x % q
    cbar, ctil = pow(hprod, q - 1, p), 1
    for j in range(N):
        cbar = cbar * (pc[j] % p) % p
        ctil = ctil * pow(pc[j] % p, u[j], p) % p
    chat = chain[N - 1] % p * pow(h, (q - U) % q, p) % p
    t1 = pow(cbar, nc, p) * pow(g, s[0], p) % p
    t2 = pow(chat, nc, p) * pow(g, s[1], p) % p
    t3 = pow(ctil, nc, p) * pow(g, s[2], p) % p
    for i in range(N):
        t3 = t3 * pow(hs[i], s_prime[i], p) % p
    t4 = []
    for j in range(w):
        ea = eb = 1
        for k in range(N):
            ea = ea * pow(E[k][j][0] % p, u[k], p) % p
            eb = eb * pow(E[k][j][1] % p, u[k], p) % p
        ns4 = (q - s[3 + j]) % q
        a, b = pow(ea, nc, p) * pow(g, ns4, p) % p, pow(eb, nc, p) * pow(K, ns4, p) % p
        for i in range(N):
            a = a * pow(E2[i][j][0] % p, s_prime[i], p) % p
            b = b * pow(E2[i][j][1] % p, s_prime[i], p) % p
        t4.append((a, b))
    that = [pow(chain[i] % p, nc, p) * pow(g, s_hat[i], p) * pow(chain[i - 1] % p if i else h, s_prime[i], p) % p
            for i in range(N)]
    if _challenge(group, y, t1, t2, t3, t4, that, chain) != c:
        failed |= CHALLENGE
    return failed == 0, failed
