"""The placeholder-free ballot of include/eg_hip_ballot2.h restated on the oracle's own pieces and
tests/range_proof_ref.py (the 0..L proof on eg_oracle.challenge, _resp_exp, _response,
is_valid_residue and Group), for the ballot2 tests: written apart from the package's host mirror
and with no import of the package.  The oracle's format switches drive it.

A manifest is a list of (nsel, option limit, contest limit).  Run as a script it writes
tests/golden/Mode4096/ballots2.json: the fixture's nonces come from its seed (expand), the file
keeps the seed, the manifest, the votes and the expected proof bytes."""
import hashlib
import json

import numpy as np

import eg_oracle as O
import range_proof_ref as R
from range_proof_ref import be2i, rows

FIXTURE = R.GOLD / O.MODE4096 / "ballots2.json"

M0 = [(3, 1, 1), (4, 2, 3), (1, 3, 3), (2, 1, 2)]
VOTES0 = [
    [0, 1, 0, 2, 1, 0, 0, 3, 1, 1],   # every contest exactly at its limit, a selection holding 2
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # every contest empty
    [1, 0, 0, 0, 2, 0, 0, 1, 0, 1],   # undervotes
    [0, 0, 1, 1, 1, 1, 0, 2, 1, 0],
    [0, 0, 0, 0, 0, 0, 2, 0, 1, 1],   # an empty contest beside voted ones
]


def layout(man):
    """-> dict: NS, SP, SN, CP, CN and per selection (k, s, L, proof row, nonce row), per contest
    (k, first, nsel, L, proof row, nonce row), by walking the manifest."""
    sels, cons = [], []
    s = sp = sn = cp = cn = 0
    for k, (n, o, c) in enumerate(man):
        cons.append((k, s, n, c, cp, cn))
        for _ in range(n):
            sels.append((k, s, o, sp, sn))
            s, sp, sn = s + 1, sp + o + 1, sn + 2 * o + 4
        cp, cn = cp + c + 1, cn + 2 * c + 3
    return dict(NS=s, SP=sp, SN=sn, CP=cp, CN=cn, sels=sels, cons=cons)


def _branches(rows32, L):
    return [(be2i(rows32[2 * j]), be2i(rows32[2 * j + 1])) for j in range(L + 1)]


def _pairs(pr):
    return rows([x for cv in pr for x in cv], 32).reshape(-1, 2, 32)


def encrypt(G, K, qbar, man, votes, sel_nonces, contest_nonces, only=None):
    """-> cts (nb, NS, 2, 512), sproof (nb, SP, 2, 32), cproof (nb, CP, 2, 32).  only: a set of
    ("s", s) / ("c", k) to prove, the other proof rows staying zero (spot checks of wide ballots);
    every ciphertext is computed."""
    lay = layout(man)
    votes = np.asarray(votes, np.uint8).reshape(-1, lay["NS"])
    nb = len(votes)
    sn = np.asarray(sel_nonces, np.uint8).reshape(nb, lay["SN"], 32)
    cn = np.asarray(contest_nonces, np.uint8).reshape(nb, lay["CN"], 32)
    cts = np.zeros((nb, lay["NS"], 2, 512), np.uint8)
    sproof = np.zeros((nb, lay["SP"], 2, 32), np.uint8)
    cproof = np.zeros((nb, lay["CP"], 2, 32), np.uint8)
    for b in range(nb):
        enc = []
        for k, s, L, pr, nr in lay["sels"]:
            m, r = int(votes[b, s]), be2i(sn[b, nr])
            ct = O.Ciphertext(G.gPowP(r), G.multP(G.powP(K, r), G.gPowP(m)))
            enc.append((ct, m, r))
            cts[b, s] = rows([ct.pad, ct.data], 512)
            if only is not None and ("s", s) not in only:
                continue
            sproof[b, pr:pr + L + 1] = _pairs(R.prove(G, K, qbar, L, ct, m, r, be2i(sn[b, nr + 1]),
                                                      _branches(sn[b, nr + 2:nr + 2 * L + 4], L)))
        for k, f, n, L, pr, nr in lay["cons"]:
            mine = enc[f:f + n]
            if only is not None and ("c", k) not in only:
                continue
            agg = O.Ciphertext(G.prodP([ct.pad for ct, _, _ in mine]), G.prodP([ct.data for ct, _, _ in mine]))
            cproof[b, pr:pr + L + 1] = _pairs(R.prove(G, K, qbar, L, agg, sum(m for _, m, _ in mine),
                                                      sum(r for _, _, r in mine) % G.q, be2i(cn[b, nr]),
                                                      _branches(cn[b, nr + 1:nr + 2 * L + 3], L)))
    return cts, sproof, cproof


def verify(G, K, qbar, man, cts, sproof, cproof, cast=None):
    """-> ok_sel (nb, NS) bool, ok_contest (nb, nc) bool, tally [(pad, data)] over the cast ballots"""
    lay = layout(man)
    cts = np.asarray(cts, np.uint8).reshape(-1, lay["NS"], 2, 512)
    nb = len(cts)
    sproof = np.asarray(sproof, np.uint8).reshape(nb, lay["SP"], 2, 32)
    cproof = np.asarray(cproof, np.uint8).reshape(nb, lay["CP"], 2, 32)
    cast = [True] * nb if cast is None else [bool(x) for x in cast]
    ok_sel, ok_con = np.zeros((nb, lay["NS"]), bool), np.zeros((nb, len(man)), bool)
    tally = [(1, 1)] * lay["NS"]
    for b in range(nb):
        ct = [O.Ciphertext(be2i(cts[b, s, 0]), be2i(cts[b, s, 1])) for s in range(lay["NS"])]
        for k, s, L, pr, _ in lay["sels"]:
            ok_sel[b, s] = R.verify(G, K, qbar, L, ct[s], _branches(sproof[b, pr:pr + L + 1].reshape(-1, 32), L))
            if cast[b]:
                tally[s] = (G.multP(tally[s][0], ct[s].pad % G.p), G.multP(tally[s][1], ct[s].data % G.p))
        for k, f, n, L, pr, _ in lay["cons"]:
            mine = ct[f:f + n]
            valid = all(O.is_valid_residue(G, x.pad) and O.is_valid_residue(G, x.data) for x in mine)
            agg = O.Ciphertext(G.prodP([x.pad % G.p for x in mine]), G.prodP([x.data % G.p for x in mine]))
            ok_con[b, k] = valid and R.verify(G, K, qbar, L, agg,
                                              _branches(cproof[b, pr:pr + L + 1].reshape(-1, 32), L))
    return ok_sel, ok_con, tally


# ---- the fixture ----
def fixture_inputs(G, fx):
    """-> K, qbar, man, votes (nb, NS), sel_nonces (nb, SN, 32), contest_nonces (nb, CN, 32)"""
    seed = bytes.fromhex(fx["seed"])
    K, qbar = R.fixture_key(G, fx)
    man = [tuple(c) for c in fx["manifest"]]
    lay = layout(man)
    votes = np.array(fx["votes"], np.uint8)
    nb = len(votes)
    sn = R.scalars(seed, "sel_nonces", nb * lay["SN"], G.q).reshape(nb, lay["SN"], 32)
    cn = R.scalars(seed, "contest_nonces", nb * lay["CN"], G.q).reshape(nb, lay["CN"], 32)
    return K, qbar, man, votes, sn, cn


def fixture_proofs(fx):
    nb = len(fx["votes"])
    un = lambda hexes: np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in hexes]).reshape(nb, -1, 2, 32)
    return un(fx["sproof"]), un(fx["cproof"])


def main():
    G = O.production_group()
    fx = {"seed": hashlib.sha256(b"ballots without placeholders").hexdigest(), "manifest": [list(c) for c in M0],
          "votes": VOTES0}
    K, qbar, man, votes, sn, cn = fixture_inputs(G, fx)
    _, sproof, cproof = encrypt(G, K, qbar, man, votes, sn, cn)
    fx["sproof"] = [bytes(p.reshape(-1)).hex() for p in sproof]
    fx["cproof"] = [bytes(p.reshape(-1)).hex() for p in cproof]
    FIXTURE.write_text(json.dumps(fx, indent=1) + "\n")
    print("wrote", FIXTURE, FIXTURE.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
