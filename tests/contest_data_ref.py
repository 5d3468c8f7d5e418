"""The definitions of include/eg_hip_contestdata.h restated with bare hashlib, hmac and CPython
pow, for the contest-data tests (no import of the package).  Elements are bytes objects; an item
is one (ballot b, contest k) pair, ballot-major."""
import hashlib
import hmac

import numpy as np

from codes_ref import H, expand, i32  # noqa: F401  (hash_elems restated; the fixtures' inputs)

TAG = b"contest"


def be32(x):
    return int(x).to_bytes(4, "big")


def nonces(q, fmt, nc, bn):
    """bn (nb, 32) -> r (nb, nc, 32): r[b,k] = H(xi_b, 3, k)"""
    rows = [H(q, fmt, bytes(bn[b]), i32(3), i32(k)) for b in range(len(bn)) for k in range(nc)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(bn), nc, 32)


def _mac(key, msg):
    return hmac.new(key, msg, hashlib.sha256).digest()


def keys(c0, kappa, ballot_id, k):
    """-> (kk, mk, label) of one item; c0 and kappa 512 bytes, ballot_id 32"""
    c0, kappa, label = bytes(c0), bytes(kappa), bytes(ballot_id) + be32(k)
    assert len(c0) == 512 and len(kappa) == 512 and len(label) == 36
    kk = hashlib.sha256(c0 + kappa).digest()
    return kk, _mac(kk, b"\x02" + TAG + label), label


def stream(kk, label, nbytes):
    out = b"".join(_mac(kk, b"\x01" + TAG + label + be32(j)) for j in range((nbytes + 31) // 32))
    return out[:nbytes]


def seal_item(c0, kappa, ballot_id, k, data):
    """-> (c1, c2) of one item"""
    data = bytes(data)
    kk, mk, label = keys(c0, kappa, ballot_id, k)
    c1 = bytes(a ^ b for a, b in zip(data, stream(kk, label, len(data))))
    return c1, _mac(mk, bytes(c0) + c1)


def open_item(c0, kappa, ballot_id, k, c1, c2):
    """-> (data, ok): data all zero when the MAC fails"""
    c1 = bytes(c1)
    kk, mk, label = keys(c0, kappa, ballot_id, k)
    if not hmac.compare_digest(_mac(mk, bytes(c0) + c1), bytes(c2)):
        return bytes(len(c1)), False
    return bytes(a ^ b for a, b in zip(c1, stream(kk, label, len(c1)))), True


def seal_with_kappa(nc, ids, c0, kappa, data):
    """The hash half over arrays: ids (nb, 32), c0 / kappa (n, 512), data (n, nbytes) -> c1, c2"""
    n, nbytes = len(data), data.shape[1]
    c1 = np.empty((n, nbytes), np.uint8)
    c2 = np.empty((n, 32), np.uint8)
    for i in range(n):
        a, m = seal_item(c0[i], kappa[i], ids[i // nc], i % nc, data[i])
        c1[i] = np.frombuffer(a, np.uint8)
        c2[i] = np.frombuffer(m, np.uint8)
    return c1, c2


def seal(p, g, K, nc, ids, r, data):
    """Both halves with CPython pow: r (n, 32) -> c0 (n, 512), c1, c2"""
    n = len(data)
    rs = [int.from_bytes(bytes(r[i]), "big") for i in range(n)]
    c0 = np.frombuffer(b"".join(pow(g, e, p).to_bytes(512, "big") for e in rs), np.uint8).reshape(n, 512)
    kappa = np.frombuffer(b"".join(pow(K, e, p).to_bytes(512, "big") for e in rs), np.uint8).reshape(n, 512)
    c1, c2 = seal_with_kappa(nc, ids, c0, kappa, data)
    return c0, c1, c2


def open_all(nc, ids, c0, kappa, c1, c2):
    """-> data (n, nbytes), ok (n,) bool"""
    n = len(c1)
    data = np.zeros(c1.shape, np.uint8)
    ok = np.zeros(n, bool)
    for i in range(n):
        d, ok[i] = open_item(c0[i], kappa[i], ids[i // nc], i % nc, c1[i], c2[i])
        data[i] = np.frombuffer(d, np.uint8)
    return data, ok


def pack(status, overvotes, write_ins, nbytes):
    """The ContestData layout: be16 length of what follows it, a status byte, a count byte and the
    overvoted selection indices (be16 each), a count byte and the write-ins (a length byte plus
    UTF-8 each), zero padding.  No truncation here: the caller passes what fits."""
    body = bytes([status, len(overvotes)]) + b"".join(int(v).to_bytes(2, "big") for v in overvotes)
    body += bytes([len(write_ins)]) + b"".join(bytes([len(w.encode())]) + w.encode() for w in write_ins)
    out = len(body).to_bytes(2, "big") + body
    assert len(out) <= nbytes
    return out + bytes(nbytes - len(out))


def fixture_inputs(fx):
    """The inputs of tests/golden/Mode4096/contest_data.json, expanded from its seed"""
    seed = bytes.fromhex(fx["seed"])
    nb, nc, nbytes = fx["nballots"], fx["ncontest"], fx["nbytes"]
    data = [pack(cd["status"], cd["overvotes"], cd["write_ins"], nbytes) for row in fx["contest_data"] for cd in row]
    return dict(nb=nb, nc=nc, nbytes=nbytes, bn=expand(seed, "ballot_nonces", nb * 32).reshape(nb, 32),
                ids=expand(seed, "ballot_ids", nb * 32).reshape(nb, 32),
                secret=int.from_bytes(bytes(expand(seed, "secret", 32)), "big"),
                data=np.frombuffer(b"".join(data), np.uint8).reshape(nb * nc, nbytes))


def fixture_outputs(p, q, g, fx, fmt):
    """-> {"r", "c0", "c1", "c2"}: lists of hex strings, one per item"""
    inp = fixture_inputs(fx)
    K = pow(g, inp["secret"] % q, p)
    r = nonces(q, fmt, inp["nc"], inp["bn"]).reshape(-1, 32)
    c0, c1, c2 = seal(p, g, K, inp["nc"], inp["ids"], r, inp["data"])
    return {name: [bytes(row).hex() for row in a] for name, a in (("r", r), ("c0", c0), ("c1", c1), ("c2", c2))}
