"""The seed, hash and opening definitions of include/eg_hip_codes2.h restated on the oracle's own
pieces (eg_oracle.hash_elems and Group) and tests/ballot2_ref.py's layout and encrypt, for the
codes2 tests: written apart from the package's host mirror and with no import of the package.  The
oracle's format switches drive it.

Run as a script it writes tests/golden/Mode4096/ballots2_seeded.json: manifest M0 and VOTES0 of
ballot2_ref, five seeds, ids and timestamps, description hashes and a chain seed expanded from the
fixture's seed; per hash format the first and last row of each ballot's nonce arrays, SHA-256
digests of the whole arrays and of cts / sproof / cproof, and B and the codes in full."""
import hashlib
import json

import numpy as np

import ballot2_ref as B2
import eg_oracle as O
import range_proof_ref as R
from range_proof_ref import be2i, rows

FIXTURE = R.GOLD / O.MODE4096 / "ballots2_seeded.json"
FORMATS = ("fixed", "minimal")
TAG_SEL, TAG_CON = 5, 6
TS0 = 1_700_000_000


def nonces(q, man, ballot_nonces):
    """-> sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32)"""
    lay = B2.layout(man)
    bn = np.asarray(ballot_nonces, np.uint8).reshape(-1, 32)
    sn = np.stack([rows([O.hash_elems(q, ("Q", be2i(x)), ("Q", TAG_SEL), ("Q", r)) for r in range(lay["SN"])], 32)
                   for x in bn])
    cn = np.stack([rows([O.hash_elems(q, ("Q", be2i(x)), ("Q", TAG_CON), ("Q", r)) for r in range(lay["CN"])], 32)
                   for x in bn])
    return sn, cn


def hashes(q, man, dsel, dcon, mh, ids, cts):
    """-> B (nb, 32), h_sel (nb, NS, 32), h_con (nb, nc, 32): every selection of a contest enters"""
    lay = B2.layout(man)
    cts = np.asarray(cts, np.uint8).reshape(-1, lay["NS"], 2, 512)
    Bs, HS, HC = [], [], []
    for b in range(len(cts)):
        hs = [O.hash_elems(q, ("Q", be2i(dsel[s])), ("P", be2i(cts[b, s, 0])), ("P", be2i(cts[b, s, 1])))
              for s in range(lay["NS"])]
        hc = [O.hash_elems(q, ("Q", be2i(dcon[k])), *[("Q", h) for h in hs[f:f + n]]) for k, f, n, _, _, _ in lay["cons"]]
        Bs.append(O.hash_elems(q, ("Q", be2i(ids[b])), ("Q", be2i(mh)), *[("Q", h) for h in hc]))
        HS.append(rows(hs, 32))
        HC.append(rows(hc, 32))
    return rows(Bs, 32), np.stack(HS), np.stack(HC)


def chain(q, seed, ts, Bs):
    out, prev = [], be2i(seed)
    for t, b in zip(ts, Bs):
        prev = O.hash_elems(q, ("Q", prev), ("Q", int(t)), ("Q", be2i(b)))
        out.append(prev)
    return rows(out, 32)


def open_ballots(G, K, man, cts, ballot_nonces):
    """-> votes (nb, NS) uint8, ok (nb, NS) bool, by trying every m in 0..olimit"""
    lay = B2.layout(man)
    cts = np.asarray(cts, np.uint8).reshape(-1, lay["NS"], 2, 512)
    votes, ok = np.zeros((len(cts), lay["NS"]), np.uint8), np.zeros((len(cts), lay["NS"]), bool)
    for b in range(len(cts)):
        xi = be2i(np.asarray(ballot_nonces, np.uint8).reshape(-1, 32)[b])
        for _, s, L, _, nr in lay["sels"]:
            r = O.hash_elems(G.q, ("Q", xi), ("Q", TAG_SEL), ("Q", nr))
            alpha, beta = be2i(cts[b, s, 0]), be2i(cts[b, s, 1])
            ms = [m for m in range(L + 1) if beta == G.multP(G.powP(K, r), G.gPowP(m))]
            if alpha == G.gPowP(r) and ms:
                votes[b, s], ok[b, s] = ms[0], True
    return votes, ok


def tamper_matrix(G, cts, ballot_nonces, votes):
    """The opening's tamper matrix on the five M0 ballots of VOTES0 -> (cts, ballot_nonces, votes,
    ok) with exactly the targeted selections' flags down (and their votes 0):
      ballot 3: a wrong seed, every flag of the ballot      ballot 2, s 0: alpha g
      ballot 0, s 3: beta g on a selection at its option limit (it then holds L + 1)
      ballot 2, s 4: beta (p - 1)      ballot 4, s 6: beta = 0      ballot 4, s 8: beta = p
    and one change that must NOT fail: ballot 1, s 3: beta g below the limit opens as 1."""
    cts, bn = np.array(cts, np.uint8).reshape(5, 10, 2, 512), np.array(ballot_nonces, np.uint8).reshape(5, 32)
    votes, ok = np.array(votes, np.uint8).reshape(5, 10), np.ones((5, 10), bool)
    assert votes[0, 3] == 2 and B2.M0[1][1] == 2 and votes[1, 3] == 0
    put = lambda b, s, c, v: cts.__setitem__((b, s, c), rows([v], 512)[0])
    bn[3, 31] ^= 1
    votes[3], ok[3] = 0, False
    put(2, 0, 0, G.multP(be2i(cts[2, 0, 0]), G.g))
    put(0, 3, 1, G.multP(be2i(cts[0, 3, 1]), G.g))
    put(2, 4, 1, G.multP(be2i(cts[2, 4, 1]), G.p - 1))
    put(4, 6, 1, 0)
    put(4, 8, 1, G.p)
    for b, s in ((2, 0), (0, 3), (2, 4), (4, 6), (4, 8)):
        votes[b, s], ok[b, s] = 0, False
    put(1, 3, 1, G.multP(be2i(cts[1, 3, 1]), G.g))
    votes[1, 3] = 1
    return cts, bn, votes, ok


# ---- the fixture ----
def fixture_inputs(G, fx):
    """-> dict: K, qbar, man, votes (nb, NS), bn, ids (nb, 32), ts [int], dsel, dcon, mh, code_seed"""
    seed = bytes.fromhex(fx["seed"])
    K, qbar = R.fixture_key(G, fx)
    man = [tuple(c) for c in fx["manifest"]]
    lay = B2.layout(man)
    votes = np.array(fx["votes"], np.uint8)
    nb = len(votes)
    x = lambda label, shape: R.expand(seed, label, int(np.prod(shape))).reshape(shape)
    return dict(K=K, qbar=qbar, man=man, votes=votes, bn=x("ballot_nonces", (nb, 32)), ids=x("ballot_ids", (nb, 32)),
                ts=list(fx["timestamps"]), dsel=x("dsel", (lay["NS"], 32)), dcon=x("dcon", (len(man), 32)),
                mh=x("manifest_hash", (32,)), code_seed=x("code_seed", (32,)))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


def record(sn, cn, cts, sproof, cproof, Bs, codes):
    """What the fixture keeps of one hash format's results."""
    hexrow = lambda r: bytes(r).hex()
    return {"sel_nonces_first": [hexrow(b[0]) for b in sn], "sel_nonces_last": [hexrow(b[-1]) for b in sn],
            "contest_nonces_first": [hexrow(b[0]) for b in cn], "contest_nonces_last": [hexrow(b[-1]) for b in cn],
            "sel_nonces_sha256": sha(sn), "contest_nonces_sha256": sha(cn), "cts_sha256": sha(cts),
            "sproof_sha256": sha(sproof), "cproof_sha256": sha(cproof), "ballot_hashes": [hexrow(r) for r in Bs],
            "codes": [hexrow(r) for r in codes]}


def compute(G, fx, fmt):
    """-> dict of the arrays of one hash format: sn, cn, cts, sproof, cproof, B, hs, hc, codes"""
    i = fixture_inputs(G, fx)
    with O.hash_format(fmt):
        sn, cn = nonces(G.q, i["man"], i["bn"])
        cts, sproof, cproof = B2.encrypt(G, i["K"], i["qbar"], i["man"], i["votes"], sn, cn)
        Bs, hs, hc = hashes(G.q, i["man"], i["dsel"], i["dcon"], i["mh"], i["ids"], cts)
        codes = chain(G.q, i["code_seed"], i["ts"], Bs)
    return dict(sn=sn, cn=cn, cts=cts, sproof=sproof, cproof=cproof, B=Bs, hs=hs, hc=hc, codes=codes)


def head():
    return {"seed": hashlib.sha256(b"seeded ballots without placeholders").hexdigest(),
            "manifest": [list(c) for c in B2.M0], "votes": B2.VOTES0,
            "timestamps": [TS0 + 61 * b for b in range(len(B2.VOTES0))]}


def build(G, computed=None):
    """The fixture as a dict; computed: {fmt: compute(...)} already at hand."""
    fx = head()
    for fmt in FORMATS:
        c = computed[fmt] if computed else compute(G, fx, fmt)
        fx[fmt] = record(c["sn"], c["cn"], c["cts"], c["sproof"], c["cproof"], c["B"], c["codes"])
    return fx


def main():
    FIXTURE.write_text(json.dumps(build(O.production_group()), indent=1) + "\n")
    print("wrote", FIXTURE, FIXTURE.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
