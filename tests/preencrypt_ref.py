"""The definitions of include/eg_hip_preencrypt.h restated with bare hashlib and pow, for the
pre-encryption tests (no import of electionguard.preencrypt): elements are bytes objects, 32 ("Q")
or 512 ("P") long, hashed as given.  Run as a script it freezes the fixture
tests/golden/Mode4096/preencrypt.json.

A manifest is a list of (real selections, votes allowed): contest k has spc_k = real + allowed
slots and limit_k = allowed."""
import hashlib
import json
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden" / "Mode4096"
FIXTURE = GOLD / "preencrypt.json"
M = [(1, 1), (3, 2), (2, 1)]   # spc 2, 5, 3; V = 38; nsel = 10
FORMATS = ("fixed", "minimal")


def group():
    c = json.loads((GOLD / "constants.json").read_text())
    return int(c["p"], 16), int(c["q"], 16), int(c["g"], 16)


def H(q, fmt, *elems):
    """SHA-256("|" + "|".join(upper hex) + "|") mod q -> 32 bytes; minimal drops leading zero bytes."""
    assert fmt in FORMATS
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


def b2i(x):
    return int.from_bytes(bytes(x), "big")


def arr(rows, shape):
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(shape)


def shape(man):
    spc = [a + b for a, b in man]
    lim = [b for _, b in man]
    off, voff, soff, toff = [], [], [], []
    o = v = s = t = 0
    for m, L in zip(spc, lim):
        off.append(o), voff.append(v), soff.append(s), toff.append(t)
        o, v, s, t = o + m, v + m * m, s + L * m, t + L
    return dict(spc=spc, lim=lim, off=off, voff=voff, soff=soff, toff=toff, nc=len(man), nsel=o, V=v, S=s, T=t)


def component(G, K, fmt, xi, w, diag):
    """-> (alpha, beta) 512-byte rows of component w of the ballot with seed xi"""
    p, q, g = G
    rho = b2i(H(q, fmt, xi, i32(4), i32(w)))
    return pow(g, rho, p).to_bytes(512, "big"), (pow(K, rho, p) * (g if diag else 1) % p).to_bytes(512, "big")


def vec_cts(G, K, fmt, man, bn):
    """bn (nb, 32) -> (nb, V, 2, 512)"""
    sh = shape(man)
    rows = []
    for b in range(len(bn)):
        for m in sh["spc"]:
            for i in range(m):
                for j in range(m):
                    rows.extend(component(G, K, fmt, bytes(bn[b]), len(rows) // 2 - b * sh["V"], i == j))
    return arr(rows, (len(bn), sh["V"], 2, 512))


def psi(q, fmt, dcon_k, rows):
    """vector hash from the vector's component rows (m, 2, 512)"""
    return H(q, fmt, dcon_k, *[H(q, fmt, r[0], r[1]) for r in rows])


def omega(h, cb):
    return b2i(bytes(h)[32 - cb:])


def derive(q, fmt, man, cb, dcon, mh, ids, cts):
    """Everything pre-encryption publishes, from the component ciphertexts (nb, V, 2, 512)."""
    sh = shape(man)
    nb = len(cts)
    srt, perm, codes, unique, chash, conf = [], [], [], [], [], []
    for b in range(nb):
        uniq, chis = 1, []
        for k, (m, vo) in enumerate(zip(sh["spc"], sh["voff"])):
            ps = [psi(q, fmt, dcon[k], cts[b, vo + i * m: vo + (i + 1) * m]) for i in range(m)]
            order = sorted(range(m), key=lambda i: (b2i(ps[i]), i))
            lst = [ps[i] for i in order]
            srt.extend(lst)
            perm.extend(order)
            cs = [omega(x, cb) for x in ps]
            codes.extend(cs)
            if len(set(cs)) < m:
                uniq = 0
            chis.append(H(q, fmt, dcon[k], *lst))
        unique.append(uniq)
        chash.extend(chis)
        conf.append(H(q, fmt, ids[b], mh, *chis))
    return dict(sorted=arr(srt, (nb, sh["nsel"], 32)), perm=np.array(perm, np.uint32).reshape(nb, sh["nsel"]),
                codes=np.array(codes, np.uint32).reshape(nb, sh["nsel"]), unique=np.array(unique, np.uint8),
                chash=arr(chash, (nb, sh["nc"], 32)), conf=arr(conf, (nb, 32)))


def record(G, K, fmt, man, cb, dcon, bn, votes, srt):
    """Recording of well-formed votes (every contest sums to its limit, every psi is in srt)."""
    p, q, g = G
    sh = shape(man)
    nb = len(votes)
    sv, rank, codes, sn, cn = [], [], [], [], []
    for b in range(nb):
        xi = bytes(bn[b])
        R = {}
        for k, (m, L, o, vo) in enumerate(zip(sh["spc"], sh["lim"], sh["off"], sh["voff"])):
            chosen = [i for i in range(m) if votes[b, o + i]]
            assert len(chosen) == L and all(votes[b, o + i] == 1 for i in chosen)
            lst = [bytes(srt[b, o + r]) for r in range(m)]
            vecs = []
            for i in chosen:
                rows = [component(G, K, fmt, xi, vo + i * m + j, i == j) for j in range(m)]
                h = psi(q, fmt, dcon[k], rows)
                vecs.append((lst.index(h), h, rows))
            for r, h, rows in sorted(vecs, key=lambda v: v[0]):   # ascending rank
                sv.extend(x for row in rows for x in row)
                rank.append(r)
                codes.append(omega(h, cb))
            for j in range(m):
                R[o + j] = sum(b2i(H(q, fmt, xi, i32(4), i32(vo + i * m + j))) for i in chosen) % q
            cn.append(H(q, fmt, xi, i32(2), i32(k)))
        for s in range(sh["nsel"]):
            sn.append(i32(R[s]))
            sn.extend(H(q, fmt, xi, i32(1), i32(4 * s + t)) for t in (1, 2, 3))
    return dict(sel_vecs=arr(sv, (nb, sh["S"], 2, 512)), sel_rank=np.array(rank, np.uint32).reshape(nb, sh["T"]),
                sel_codes=np.array(codes, np.uint32).reshape(nb, sh["T"]),
                sel_nonces=arr(sn, (nb, sh["nsel"], 4, 32)), contest_nonces=arr(cn, (nb, sh["nc"], 32)))


def product(G, man, sel_vecs):
    """-> (nb, nsel, 2, 512): slot-wise products of each contest's chosen vectors"""
    p = G[0]
    sh = shape(man)
    rows = []
    for b in range(len(sel_vecs)):
        for m, L, so in zip(sh["spc"], sh["lim"], sh["soff"]):
            for j in range(m):
                for c in (0, 1):
                    x = 1
                    for t in range(L):
                        x = x * b2i(sel_vecs[b, so + t * m + j, c]) % p
                    rows.append(x.to_bytes(512, "big"))
    return arr(rows, (len(sel_vecs), sh["nsel"], 2, 512))


def tamper_corpus(p, man, good):
    """Tampered copies of a good record of >= 5 ballots.  good: dict of sel_vecs, sel_rank,
    sel_codes, sorted, cts, conf (arrays).  -> list of (name, arrays, contests {(b, k)} whose
    verdict must turn false, ballots {b} whose confirmation verdict must turn false); nothing else
    may change."""
    sh = shape(man)
    off, so, to, spc = sh["off"], sh["soff"], sh["toff"], sh["spc"]
    out = []

    def case(name, contests, ballots=()):
        a = {k: np.array(v, copy=True) for k, v in good.items()}
        out.append((name, a, set(contests), set(ballots)))
        return a

    a = case("two sorted hashes swapped", {(0, 1)}, {0})
    a["sorted"][0, [off[1], off[1] + 1]] = a["sorted"][0, [off[1] + 1, off[1]]]
    a = case("one byte of a chosen vector changed", {(1, 1)})
    a["sel_vecs"][1, so[1] + 3, 1, 511] ^= 1
    a = case("a rank off by one", {(2, 0)})
    a["sel_rank"][2, to[0]] = (a["sel_rank"][2, to[0]] + 1) % spc[0]
    a = case("two chosen vectors exchanged", {(3, 1)})
    m = spc[1]
    a["sel_vecs"][3, so[1]: so[1] + 2 * m] = np.concatenate([good["sel_vecs"][3, so[1] + m: so[1] + 2 * m],
                                                              good["sel_vecs"][3, so[1]: so[1] + m]])
    a = case("a code changed", {(4, 2)})
    a["sel_codes"][4, to[2]] ^= 1
    a = case("conf changed", set(), {0})
    a["conf"][0, 31] ^= 1
    a = case("a ballot ciphertext replaced", {(1, 2)})
    a["cts"][1, off[2] + 1] = a["cts"][1, off[2]]
    a = case("a chosen element set to 0", {(2, 1)})
    a["sel_vecs"][2, so[1], 0] = 0
    a = case("a chosen element set to p + 1", {(3, 2)})
    a["sel_vecs"][3, so[2] + 1, 1] = np.frombuffer((p + 1).to_bytes(512, "big"), np.uint8)
    return out


# ---------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------
def expand(seed: bytes, label: str, nbytes: int) -> np.ndarray:
    out, i = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(seed + b"|" + label.encode() + b"|" + str(i).encode()).digest()
        i += 1
    return np.frombuffer(out[:nbytes], np.uint8).copy()


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture_inputs(fx):
    """-> K, dcon (nc, 32), mh (32,), ids (nb, 32), bn (nb, 32), votes (nb, nsel)"""
    p, q, g = group()
    seed = bytes.fromhex(fx["seed"])
    sh = shape([tuple(c) for c in fx["manifest"]])
    K = pow(g, b2i(expand(seed, "secret", 32)) % q, p)
    nb = len(fx["trials"])
    dcon = expand(seed, "dcon", sh["nc"] * 32).reshape(-1, 32)
    mh = expand(seed, "manifest_hash", 32)
    ids = expand(seed, "ballot_ids", nb * 32).reshape(nb, 32)
    bn = np.stack([trial_seed(seed, q, t) for t in fx["trials"]])
    votes = np.array(fx["votes"], np.uint8)
    return K, dcon, mh, ids, bn, votes


def trial_seed(seed: bytes, q: int, t: int) -> np.ndarray:
    return np.frombuffer(i32(b2i(expand(seed, "xi%d" % t, 32)) % q), np.uint8)


# votes with 0, 1 and 2 real choices in the limit-2 contest and an undervote in each limit-1 contest
VOTES = [
    [1, 0, 1, 1, 0, 0, 0, 1, 0, 0],
    [0, 1, 0, 1, 0, 1, 0, 0, 1, 0],
    [1, 0, 0, 0, 0, 1, 1, 0, 0, 1],
    [1, 0, 0, 0, 1, 0, 1, 1, 0, 0],
    [0, 1, 1, 0, 1, 0, 0, 0, 0, 1],
]


def make_fixture(seed_hex="707265656e63727970742d6669787475726521"):
    """Search trial seeds until, of 5 ballots, one has two vectors of a contest with the same
    1-byte code in the fixed format, one has none, and one has a ciphertext element with a zero
    top byte in the minimal format (its minimal hex is shorter)."""
    G = group()
    p, q, g = G
    seed = bytes.fromhex(seed_hex)
    sh = shape(M)
    K = pow(g, b2i(expand(seed, "secret", 32)) % q, p)
    dcon = expand(seed, "dcon", sh["nc"] * 32).reshape(-1, 32)
    mh = expand(seed, "manifest_hash", 32)
    ids5 = expand(seed, "ballot_ids", 5 * 32).reshape(5, 32)
    coll, plain, ztop = [], [], []
    t = 0
    while not (coll and ztop and len(plain) >= 5):
        bn = trial_seed(seed, q, t)[None]
        cf = vec_cts(G, K, "fixed", M, bn)
        if derive(q, "fixed", M, 1, dcon, mh, ids5[:1], cf)["unique"][0] == 0:
            coll.append(t)
        elif (vec_cts(G, K, "minimal", M, bn)[0, :, :, 0] == 0).any():
            ztop.append(t)
        else:
            plain.append(t)
        t += 1
    trials = [coll[0], ztop[0]] + plain[:3]
    fx = {"seed": seed_hex, "manifest": [list(c) for c in M], "trials": trials, "searched": t, "votes": VOTES}
    K, dcon, mh, ids, bn, votes = fixture_inputs(fx)
    for fmt in FORMATS:
        cts = vec_cts(G, K, fmt, M, bn)
        d = derive(q, fmt, M, 2, dcon, mh, ids, cts)
        r = record(G, K, fmt, M, 2, dcon, bn, votes, d["sorted"])
        fx[fmt] = {
            "vec_cts_sha256": sha(cts), "zero_top_elements": int((cts[:, :, :, 0] == 0).sum()),
            "sorted": [bytes(x).hex() for x in d["sorted"].reshape(-1, 32)],
            "perm": d["perm"].reshape(-1).tolist(), "codes2": d["codes"].reshape(-1).tolist(),
            "unique": {str(cb): derive(q, fmt, M, cb, dcon, mh, ids, cts)["unique"].tolist() for cb in (1, 2, 3, 4)},
            "chash": [bytes(x).hex() for x in d["chash"].reshape(-1, 32)],
            "conf": [bytes(x).hex() for x in d["conf"]],
            "sel_vecs_sha256": sha(r["sel_vecs"]), "sel_rank": r["sel_rank"].reshape(-1).tolist(),
            "sel_codes2": r["sel_codes"].reshape(-1).tolist(), "sel_nonces_sha256": sha(r["sel_nonces"]),
            "contest_nonces_sha256": sha(r["contest_nonces"]),
        }
    assert fx["minimal"]["zero_top_elements"] >= 1
    u1 = fx["fixed"]["unique"]["1"]
    assert 0 in u1 and 1 in u1
    FIXTURE.write_text(json.dumps(fx, indent=1) + "\n")
    print("wrote", FIXTURE, FIXTURE.stat().st_size, "bytes; searched", t, "seeds; trials", trials)


if __name__ == "__main__":
    make_fixture()
