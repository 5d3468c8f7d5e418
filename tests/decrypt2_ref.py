"""A CPython restatement of the threshold decryption with one combined proof per text
(include/eg_hip_decrypt2.h), for the tests: CPython ints and hashlib only, no
import of the package.  It is the reference of every decrypt2 test.

  ceremony(p, q, g, n_g, quorum, rng)      -> Ceremony (coefficients, commitments, K, s)
  key_share / share_public_key / lagrange  -> z_i, Z_i from the PUBLIC commitments, w_i
  commit / combine / respond / check / verify   the five steps, on lists of ints
  run(...)                                 -> an honest Run of all of them
  dlog(p, g, y, limit)                     -> t with g^t = y, 0 <= t <= limit, or None

Semantics (the header's): bases are reduced mod p, pow(0, 0) = 1; the exponents of commit, check
and verify are used as the values given; respond reduces its scalars mod q; the hash takes A, B, K
and M as the values given; check compares the recomputed values with a_i and b_i as given.
"""
import hashlib
from types import SimpleNamespace

TAG = 0x30

_MEMO = {}


def powm(b, e, p):
    """pow(b mod p, e, p), remembered: the tests' texts and nonces repeat."""
    key = (b % p, e, p)
    r = _MEMO.get(key)
    if r is None:
        r = _MEMO[key] = pow(b % p, e, p)
    return r


def _hex(x, width, fmt):
    b = int(x).to_bytes(width, "big")
    if fmt == "minimal":
        b = b.lstrip(b"\0") or b"\0"
    elif fmt != "fixed":
        raise ValueError(fmt)
    return b.hex().upper()


def hash_elems(q, elems, fmt="fixed"):
    """elems: ("P" | "Q", int) pairs -> SHA-256("|hex|...|") mod q."""
    parts = [_hex(v, 512 if kind == "P" else 32, fmt) for kind, v in elems]
    return int.from_bytes(hashlib.sha256(("|" + "|".join(parts) + "|").encode("ascii")).digest(), "big") % q


def challenge(q, qbar, K, A, B, a, b, M, fmt="fixed"):
    return hash_elems(q, [("Q", qbar), ("Q", TAG), ("P", K), ("P", A), ("P", B), ("P", a), ("P", b), ("P", M)], fmt)


def poly_eval(coeffs, x, q):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % q
    return acc


def lagrange(xs, xi, q):
    num = den = 1
    for xj in xs:
        if xj != xi:
            num = num * xj % q
            den = den * (xj - xi) % q
    return num * pow(den, -1, q) % q


def ceremony(p, q, g, n_g, quorum, rng):
    coeffs = [[rng.randrange(1, q) for _ in range(quorum)] for _ in range(n_g)]
    comm = [[pow(g, a, p) for a in co] for co in coeffs]
    K = 1
    for cm in comm:
        K = K * cm[0] % p
    return SimpleNamespace(p=p, q=q, g=g, n=n_g, quorum=quorum, xs=list(range(1, n_g + 1)), coeffs=coeffs,
                           commitments=comm, K=K, s=sum(co[0] for co in coeffs) % q)


def key_share(cer, x):
    """z = SUM_j P_j(x) mod q."""
    return sum(poly_eval(co, x, cer.q) for co in cer.coeffs) % cer.q


def share_public_key(cer, x):
    """Z = PROD_j PROD_m K_{j,m}^(x^m mod q), from the public commitments alone."""
    Z = 1
    for cm in cer.commitments:
        for m, Kjm in enumerate(cm):
            Z = Z * pow(Kjm, pow(x, m, cer.q), cer.p) % cer.p
    return Z


# ---- the five steps --------------------------------------------------------------------------
def commit(p, g, z, pads, nonces):
    """-> (M, a, b) lists: M = A^z, a = g^u, b = A^u."""
    return ([powm(A, z, p) for A in pads], [powm(g, u, p) for u in nonces],
            [powm(A, u, p) for A, u in zip(pads, nonces)])


def respond(q, z, nonces, ci):
    return [(u % q - (c % q) * (z % q)) % q for u, c in zip(nonces, ci)]


def combine(p, q, K, qbar, weights, texts, shares, comm, fmt="fixed"):
    """texts [(A, B)], shares [t][i], comm [t][i] = (a_i, b_i) -> (M [t], c [t], ci [t][i])."""
    Ms, cs, cis = [], [], []
    for (A, B), sh, cm in zip(texts, shares, comm):
        M = a = b = 1 % p
        for w, Mi, (ai, bi) in zip(weights, sh, cm):
            M = M * powm(Mi, w, p) % p
            a = a * (ai % p) % p
            b = b * (bi % p) % p
        c = challenge(q, qbar, K, A, B, a, b, M, fmt)
        Ms.append(M)
        cs.append(c)
        cis.append([c * (w % q) % q for w in weights])
    return Ms, cs, cis


def check(p, q, g, Z, texts, shares, comm, ci, vi):
    """-> (ok [t][i], v [t])."""
    oks, vs = [], []
    for (A, _), sh, cm, cr, vr in zip(texts, shares, comm, ci, vi):
        row = []
        for Zi, Mi, (ai, bi), c, v in zip(Z, sh, cm, cr, vr):
            ga = powm(g, v, p) * powm(Zi, c, p) % p
            gb = powm(A, v, p) * powm(Mi, c, p) % p
            row.append(c < q and v < q and ga == ai and gb == bi)
        oks.append(row)
        vs.append(sum(v % q for v in vr) % q)
    return oks, vs


def verify(p, q, g, K, qbar, texts, M, proofs, fmt="fixed"):
    """proofs [(c, v)] -> ok [t]."""
    out = []
    for (A, B), Mt, (c, v) in zip(texts, M, proofs):
        a = powm(g, v, p) * powm(K, c, p) % p
        b = powm(A, v, p) * powm(Mt, c, p) % p
        out.append(c < q and v < q and c == challenge(q, qbar, K, A, B, a, b, Mt, fmt))
    return out


def dlog(p, g, y, limit):
    acc = 1 % p
    for t in range(limit + 1):
        if acc == y:
            return t
        acc = acc * g % p
    return None


def run(cer, qbar, avail_xs, texts, nonces, fmt="fixed", limit=None, zs=None, after_commit=None, after_respond=None,
        publish=None):
    """A run by the guardians at avail_xs; nonces [i][t].  Honest unless told otherwise: zs overrides
    the key shares the guardians USE (the published Z stay the ceremony's); after_commit(shares,
    comm), after_respond(ci, vi) and publish(M, c, v) may alter those lists in place on their way
    to the mediator, to the check, and into the record."""
    p, q, g = cer.p, cer.q, cer.g
    k, n = len(avail_xs), len(texts)
    true_z = [key_share(cer, x) for x in avail_xs]
    zs = list(true_z) if zs is None else zs
    Z = [powm(g, z, p) for z in true_z]   # == share_public_key(cer, x): tests/test_decrypt2_host.py
    w = [lagrange(avail_xs, x, q) for x in avail_xs]
    pads = [A for A, _ in texts]
    r1 = [commit(p, g, z, pads, nonces[i]) for i, z in enumerate(zs)]
    shares = [[r1[i][0][t] for i in range(k)] for t in range(n)]
    comm = [[[r1[i][1][t], r1[i][2][t]] for i in range(k)] for t in range(n)]
    if after_commit:
        after_commit(shares, comm)
    M, c, ci = combine(p, q, cer.K, qbar, w, texts, shares, comm, fmt)
    r2 = [respond(q, z, nonces[i], [ci[t][i] for t in range(n)]) for i, z in enumerate(zs)]
    vi = [[r2[i][t] for i in range(k)] for t in range(n)]
    if after_respond:
        after_respond(ci, vi)
    ok, v = check(p, q, g, Z, texts, shares, comm, ci, vi)
    if publish:
        publish(M, c, v)
    proofs = list(zip(c, v))
    counts = None
    if limit is not None:
        counts = [dlog(p, g, (B % p) * pow(Mt, -1, p) % p, limit) if Mt else None for (_, B), Mt in zip(texts, M)]
    return SimpleNamespace(xs=avail_xs, z=zs, Z=Z, w=w, texts=texts, nonces=nonces, shares=shares, comm=comm, M=M, c=c,
                           ci=ci, vi=vi, ok=ok, v=v, proofs=proofs, counts=counts,
                           verified=verify(p, q, g, cer.K, qbar, texts, M, proofs, fmt))


# ---- tamperings ------------------------------------------------------------------------------
# kind -> what fails: "item" the check's flag (t, i) alone, "guardian" guardian i at every text;
# and the texts whose published proof no longer verifies: "text" t alone, "all", or "none".
TAMPERINGS = {
    "vi": ("item", "text"), "ci": ("item", "none"), "ai": ("item", "text"), "bi": ("item", "text"),
    "Mi": ("item", "text"), "wrong_z": ("guardian", "all"),
    "pub_M": ("none", "text"), "pub_c": ("none", "text"), "pub_v": ("none", "text"),
}


def tampered(cer, qbar, avail_xs, texts, nonces, kind, t, i, fmt="fixed"):
    """run() with one tampering at text t, guardian i -> (Run, expected failing (t, i) of the
    check, expected failing texts of the verifier)."""
    p, q, g = cer.p, cer.q, cer.g
    n, k = len(texts), len(avail_xs)
    kw = {}
    if kind == "vi":
        kw["after_respond"] = lambda ci, vi: vi[t].__setitem__(i, (vi[t][i] + 1) % q)
    elif kind == "ci":
        kw["after_respond"] = lambda ci, vi: ci[t].__setitem__(i, (ci[t][i] + 1) % q)
    elif kind == "ai":
        kw["after_commit"] = lambda sh, cm: cm[t][i].__setitem__(0, cm[t][i][0] * g % p)
    elif kind == "bi":
        kw["after_commit"] = lambda sh, cm: cm[t][i].__setitem__(1, cm[t][i][1] * g % p)
    elif kind == "Mi":
        kw["after_commit"] = lambda sh, cm: sh[t].__setitem__(i, sh[t][i] * g % p)
    elif kind == "wrong_z":
        zs = [key_share(cer, x) for x in avail_xs]
        zs[i] = (zs[i] + 1) % q
        kw["zs"] = zs
    elif kind == "pub_M":
        kw["publish"] = lambda M, c, v: M.__setitem__(t, M[t] * g % p)
    elif kind == "pub_c":
        kw["publish"] = lambda M, c, v: c.__setitem__(t, (c[t] + 1) % q)
    elif kind == "pub_v":
        kw["publish"] = lambda M, c, v: v.__setitem__(t, (v[t] + 1) % q)
    else:
        raise ValueError(kind)
    what, texts_out = TAMPERINGS[kind]
    bad_items = {"item": {(t, i)}, "guardian": {(tt, i) for tt in range(n)}, "none": set()}[what]
    bad_texts = {"text": {t}, "all": set(range(n)), "none": set()}[texts_out]
    return run(cer, qbar, avail_xs, texts, nonces, fmt, **kw), bad_items, bad_texts
