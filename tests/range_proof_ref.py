"""The 0..L range proof of include/eg_hip_range.h restated on the oracle's own pieces
(eg_oracle.challenge, _resp_exp, _response, is_valid_residue and Group), for the range-proof tests:
written apart from the package's host mirror and with no import of the package.  The oracle's
format switches (O.hash_format, O.proof_format) drive it.

Run as a script it writes tests/golden/Mode4096/range_proofs.json: the fixture's inputs come from
its seed (expand), the file keeps the seed, the cases and the expected proofs."""
import hashlib
import json
from pathlib import Path

import numpy as np

import eg_oracle as O

GOLD = Path(__file__).resolve().parent / "golden"
FIXTURE = GOLD / O.MODE4096 / "range_proofs.json"
MAX_LIMIT = 15


def commitments(G, K, ct, branches):
    """The verifier's [a_0, b_0, ..., a_L, b_L] of the branches [(c_j, v_j)]."""
    out = []
    for j, (c, v) in enumerate(branches):
        e = O._resp_exp(G.q, c)
        out.append(G.multP(G.gPowP(v), G.powP(ct.pad, e)))
        out.append(G.prodP([G.powP(K, v), G.powP(ct.data, e), G.gPowP((-j * e) % G.q)]))
    return out


def verify(G, K, qbar, L, ct, branches):
    q = G.q
    if len(branches) != L + 1 or not 1 <= L <= MAX_LIMIT:
        return False
    if not (O.is_valid_residue(G, ct.pad) and O.is_valid_residue(G, ct.data)):
        return False
    if not all(0 <= c < q and 0 <= v < q for c, v in branches):
        return False
    c = O.challenge(q, qbar, K, (ct.pad, ct.data), commitments(G, K, ct, branches))
    return sum(cj for cj, _ in branches) % q == c


def prove(G, K, qbar, L, ct, m, R, u, branches):
    """branches: (c_j, v_j) for every j, entry m ignored -> the proof's [(c_j, v_j)].  The
    simulated branches are the verifier's own values on the ciphertext; the prover's fixed-base
    form g^(v + R e) equals them only for alpha = g^R, which is what a test of a lying m relies on."""
    q = G.q
    assert len(branches) == L + 1 and 0 <= m <= L
    others = [(c, v) if j != m else (0, 0) for j, (c, v) in enumerate(branches)]  # branch m costs nothing here
    sim = commitments(G, K, ct, others)
    if ct.pad != G.gPowP(R) or ct.data != G.multP(G.powP(K, R), G.gPowP(m)):
        # a prover that lies about m: its simulated b_j carry g^((m - j) e_j) for the CLAIMED m
        for j, (c, v) in enumerate(branches):
            e = O._resp_exp(q, c)
            s = (v + R * e) % q
            sim[2 * j] = G.gPowP(s)
            sim[2 * j + 1] = G.multP(G.powP(K, s), G.gPowP(((m - j) * e) % q))
    sim[2 * m], sim[2 * m + 1] = G.gPowP(u), G.powP(K, u)
    c = O.challenge(q, qbar, K, (ct.pad, ct.data), sim)
    cm = (c - sum(cj for j, (cj, _) in enumerate(branches) if j != m)) % q
    out = list(branches)
    out[m] = (cm, O._response(q, u, cm, R))
    return out


# ---- array forms (the wire layouts of eg_hip_range.h) ----
def be2i(row):
    return int.from_bytes(bytes(row), "big")


def rows(ints, width):
    return np.frombuffer(b"".join(int(x).to_bytes(width, "big") for x in ints), np.uint8).reshape(-1, width).copy()


def prove_arrays(G, K, qbar, L, cts, values, R, nonces):
    cts, nonces = np.asarray(cts).reshape(-1, 2, 512), np.asarray(nonces).reshape(-1, 2 * L + 3, 32)
    out = np.zeros((len(cts), L + 1, 2, 32), np.uint8)
    for i in range(len(cts)):
        br = [(be2i(nonces[i, 1 + 2 * j]), be2i(nonces[i, 2 + 2 * j])) for j in range(L + 1)]
        pr = prove(G, K, qbar, L, O.Ciphertext(be2i(cts[i, 0]), be2i(cts[i, 1])), int(values[i]), be2i(R[i]),
                   be2i(nonces[i, 0]), br)
        out[i] = rows([x for cv in pr for x in cv], 32).reshape(L + 1, 2, 32)
    return out


def verify_arrays(G, K, qbar, L, cts, proofs):
    cts, proofs = np.asarray(cts).reshape(-1, 2, 512), np.asarray(proofs).reshape(-1, L + 1, 2, 32)
    return np.array([verify(G, K, qbar, L, O.Ciphertext(be2i(cts[i, 0]), be2i(cts[i, 1])),
                            [(be2i(proofs[i, j, 0]), be2i(proofs[i, j, 1])) for j in range(L + 1)])
                     for i in range(len(cts))], dtype=bool)


def encrypt_arrays(G, K, values, R):
    return np.stack([np.stack([rows([G.gPowP(be2i(r))], 512)[0],
                               rows([G.multP(G.powP(K, be2i(r)), G.gPowP(int(m)))], 512)[0]])
                     for m, r in zip(values, R)])


# ---- the fixture ----
def expand(seed: bytes, label: str, nbytes: int) -> np.ndarray:
    out, i = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(seed + b"|" + label.encode() + b"|" + str(i).encode()).digest()
        i += 1
    return np.frombuffer(out[:nbytes], np.uint8).copy()


def scalars(seed, label, n, q):
    """n scalars below q from the seed, (n, 32)"""
    raw = expand(seed, label, n * 32).reshape(n, 32)
    return rows([be2i(r) % q for r in raw], 32)


CASES = [  # (name, L, values, hash format, response, pre-image)
    ("L1", 1, [0, 1], "fixed", "minus", "message_first"),
    ("L2", 2, [0, 1, 2], "fixed", "minus", "message_first"),
    ("L3", 3, [0, 1, 2, 3], "fixed", "minus", "message_first"),
    ("L4", 4, [0, 1, 2, 3, 4], "fixed", "minus", "message_first"),
    ("L15", 15, [0, 7, 15], "fixed", "minus", "message_first"),
] + [("L2/%s/%s" % (r, p), 2, [0, 1, 2], "fixed", r, p) for r in O.RESPONSES for p in O.PREIMAGES
     if (r, p) != ("minus", "message_first")] + [("L2/minimal", 2, [0, 1, 2], "minimal", "minus", "message_first")]


def fixture_key(G, fx):
    seed = bytes.fromhex(fx["seed"])
    return G.gPowP(be2i(scalars(seed, "secret", 1, G.q)[0])), be2i(scalars(seed, "qbar", 1, G.q)[0])


def case_inputs(G, K, fx, case):
    """-> dict(L, values (n,), R (n, 32), nonces (n, 2L+3, 32), cts (n, 2, 512)) of a fixture case"""
    seed, L = bytes.fromhex(fx["seed"]), case["limit"]
    values = np.array(case["values"], np.uint8)
    n = len(values)
    tag = "L%d" % L   # cases of one limit share their inputs, whatever the format
    R = scalars(seed, tag + "/R", n, G.q)
    nonces = scalars(seed, tag + "/nonces", n * (2 * L + 3), G.q).reshape(n, 2 * L + 3, 32)
    return dict(L=L, values=values, R=R, nonces=nonces, cts=encrypt_arrays(G, K, values, R))


def case_proofs(G, K, qbar, fx, case):
    inp = case_inputs(G, K, fx, case)
    with O.hash_format(case["hash_format"]), O.proof_format(case["response"], case["preimage"]):
        return prove_arrays(G, K, qbar, inp["L"], inp["cts"], inp["values"], inp["R"], inp["nonces"])


def main():
    G = O.production_group()
    fx = {"seed": hashlib.sha256(b"range proofs 0..L").hexdigest(), "cases": []}
    K, qbar = fixture_key(G, fx)
    for name, L, values, hf, resp, pre in CASES:
        case = {"name": name, "limit": L, "values": values, "hash_format": hf, "response": resp, "preimage": pre}
        pr = case_proofs(G, K, qbar, fx, case)
        case["proofs"] = [bytes(p.reshape(-1)).hex() for p in pr]
        fx["cases"].append(case)
    FIXTURE.write_text(json.dumps(fx, indent=1) + "\n")
    print("wrote", FIXTURE, FIXTURE.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
