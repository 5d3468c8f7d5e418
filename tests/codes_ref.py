"""The definitions of include/eg_hip_codes.h restated with bare hashlib, for the codes tests (no
import of the package): elements are bytes objects, 32 ("Q") or 512 ("P") long, hashed as given."""
import hashlib

import numpy as np


def H(q, fmt, *elems):
    """SHA-256("|" + "|".join(upper hex) + "|") mod q -> 32 bytes; minimal drops leading zero bytes."""
    assert fmt in ("fixed", "minimal")
    parts = []
    for e in elems:
        e = bytes(e)
        assert len(e) in (32, 512)
        if fmt == "minimal":
            e = e.lstrip(b"\0") or b"\0"
        parts.append(e.hex().upper())
    msg = ("|" + "|".join(parts) + "|").encode("ascii")
    return (int.from_bytes(hashlib.sha256(msg).digest(), "big") % q).to_bytes(32, "big")


def i32(x):
    return int(x).to_bytes(32, "big")


def arr(rows, shape):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(shape)


def nonces(q, fmt, spc, bn):
    """bn (nb, 32) -> sel_nonces (nb, nsel, 4, 32), contest_nonces (nb, nc, 32)"""
    nsel, nc, nb = int(sum(spc)), len(spc), len(bn)
    sn = [H(q, fmt, bn[b], i32(1), i32(r)) for b in range(nb) for r in range(4 * nsel)]
    cn = [H(q, fmt, bn[b], i32(2), i32(k)) for b in range(nb) for k in range(nc)]
    return arr(sn, (nb, nsel, 4, 32)), arr(cn, (nb, nc, 32))


def hashes(q, fmt, spc, dsel, dcon, mh, ids, cts):
    """-> B (nb, 32), h_sel (nb, nsel, 32), h_con (nb, nc, 32)"""
    nsel, nc, nb = int(sum(spc)), len(spc), len(cts)
    hs = [[H(q, fmt, dsel[s], cts[b, s, 0], cts[b, s, 1]) for s in range(nsel)] for b in range(nb)]
    hc, off = [[] for _ in range(nb)], 0
    for k, n in enumerate(spc):
        for b in range(nb):
            hc[b].append(H(q, fmt, dcon[k], *hs[b][off:off + int(n)]))
        off += int(n)
    B = [H(q, fmt, ids[b], mh, *hc[b]) for b in range(nb)]
    return (arr(B, (nb, 32)), arr([h for r in hs for h in r], (nb, nsel, 32)),
            arr([h for r in hc for h in r], (nb, nc, 32)))


def chain(q, fmt, seed, ts, B):
    codes, prev = [], bytes(seed)
    for b in range(len(B)):
        prev = H(q, fmt, prev, ts[b], B[b])
        codes.append(prev)
    return arr(codes, (len(B), 32))


def check(q, fmt, seed, ts, B, codes):
    return np.array([bytes(codes[b]) == H(q, fmt, codes[b - 1] if b else seed, ts[b], B[b])
                     for b in range(len(B))], bool)


def expand(seed: bytes, label: str, nbytes: int) -> np.ndarray:
    """nbytes of SHA-256(seed | label | counter) output: the fixture's inputs from its seed."""
    out, i = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(seed + b"|" + label.encode() + b"|" + str(i).encode()).digest()
        i += 1
    return np.frombuffer(out[:nbytes], np.uint8).copy()
