"""A CPython restatement of the verifiable shuffle (include/eg_hip_shuffle.h),
for the tests: CPython ints and hashlib only, no import of the package.  It is the reference of every
shuffle test: generators, mix, the Terelius-Wikstrom prover and its verifier, and the tagged hashes.

  find_group(pbits, qbits)                       -> a toy Schnorr group (p, q, g) with p = cof q + 1
  generators(p, q, gseed, N, fmt)                -> [h, h_0 .. h_{N-1}, PROD h_i]
  mix(p, q, g, K, E, psi, r)                     -> E'
  prove(p, q, g, K, qbar, gseed, G, E, E2, psi, r, nonces, fmt) -> Proof (and its inner values)
  verify(p, q, g, K, qbar, gseed, G, E, E2, proof, check_inputs, fmt) -> (ok, failed mask)

E is a list of N rows, a row a list of w pairs (alpha, beta); psi a list of N indices; r a list of N
lists of w nonces; nonces a flat list of 4 N + 3 + w values in the order rho, rho^, omega^, omega',
omega1, omega2, omega3, omega4.  Indices are 0-based.  Bases are reduced mod p, the prover's nonces
mod q; the hashes take E and E' as the values given (512-byte P elements, 32-byte Q elements).
"""
import hashlib
from types import SimpleNamespace

TAG_LEAF, TAG_NODE, TAG_SEED, TAG_GEN, TAG_U, TAG_C = 0x40, 0x41, 0x42, 0x43, 0x44, 0x45
FAN = 256
RANGE, RESIDUE, CHALLENGE = 1, 2, 4


# ---- hashes ------------------------------------------------------------------------------------
def _hex(x, width, fmt):
    b = int(x).to_bytes(width, "big")
    if fmt == "minimal":
        b = b.lstrip(b"\0") or b"\0"
    elif fmt != "fixed":
        raise ValueError(fmt)
    return b.hex().upper()


def digest(elems, fmt="fixed"):
    """elems: ("P" | "Q", int) pairs -> the raw SHA-256 of "|hex|...|"."""
    parts = [_hex(v, 512 if kind == "P" else 32, fmt) for kind, v in elems]
    return hashlib.sha256(("|" + "|".join(parts) + "|").encode("ascii")).digest()


def hash_elems(q, elems, fmt="fixed"):
    return int.from_bytes(digest(elems, fmt), "big") % q


def leaf(q, xs, fmt="fixed"):
    return hash_elems(q, [("Q", TAG_LEAF)] + [("P", x) for x in xs], fmt)


def tree(q, vs, fmt="fixed"):
    """T: one hash of up to 256 values; of more, T of the Ts of consecutive chunks of 256."""
    vs = list(vs)
    while len(vs) > FAN:
        vs = [tree(q, vs[i:i + FAN], fmt) for i in range(0, len(vs), FAN)]
    return hash_elems(q, [("Q", TAG_NODE), ("Q", len(vs))] + [("Q", v) for v in vs], fmt)


def tree_rows(q, rows, fmt="fixed"):
    return tree(q, [leaf(q, row, fmt) for row in rows], fmt)


def flat(E):
    """Rows of (alpha, beta) pairs -> rows of 2 w elements."""
    return [[x for pair in row for x in pair] for row in E]


# ---- groups ------------------------------------------------------------------------------------
def _is_prime(n):
    if n < 2:
        return False
    for s in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % s == 0:
            return n == s
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def find_group(pbits=64, qbits=32):
    """The first Schnorr group p = cof q + 1 with a qbits prime q and a pbits prime p, g of order q."""
    q = (1 << (qbits - 1)) + 1
    while not _is_prime(q):
        q += 2
    cof = (1 << (pbits - 1)) // q + 1
    cof += cof & 1
    while not _is_prime(cof * q + 1):
        cof += 2
    p = cof * q + 1
    a = 2
    while pow(a, cof, p) in (0, 1):
        a += 1
    return p, q, pow(a, cof, p)


# ---- generators --------------------------------------------------------------------------------
def gen(p, q, gseed, k, fmt="fixed"):
    X = b"".join(digest([("Q", gseed), ("Q", TAG_GEN), ("Q", k), ("Q", t)], fmt) for t in range(16))
    return pow(int.from_bytes(X, "big") % p, (p - 1) // q, p)


def generators(p, q, gseed, N, fmt="fixed"):
    G = [gen(p, q, gseed, k, fmt) for k in range(N + 1)]
    if any(x in (0, 1) for x in G):
        raise ValueError("a generator is 0 or 1")
    prod = 1
    for x in G[1:]:
        prod = prod * x % p
    return G + [prod]


# ---- mix ---------------------------------------------------------------------------------------
def mix(p, q, g, K, E, psi, r):
    return [[(E[psi[i]][j][0] % p * pow(g, r[i][j] % q, p) % p, E[psi[i]][j][1] % p * pow(K, r[i][j] % q, p) % p)
             for j in range(len(E[0]))] for i in range(len(E))]


# ---- prove -------------------------------------------------------------------------------------
def seed(q, qbar, K, gseed, N, w, E, E2, pc, fmt="fixed"):
    return hash_elems(q, [("Q", qbar), ("Q", TAG_SEED), ("Q", N), ("Q", w), ("P", K), ("Q", gseed),
                          ("Q", tree_rows(q, flat(E), fmt)), ("Q", tree_rows(q, flat(E2), fmt)),
                          ("Q", tree_rows(q, [[x] for x in pc], fmt))], fmt)


def challenges(q, y, N, fmt="fixed"):
    return [hash_elems(q, [("Q", y), ("Q", TAG_U), ("Q", j)], fmt) for j in range(N)]


def challenge(q, y, t1, t2, t3, t4, that, chain, fmt="fixed"):
    return hash_elems(q, [("Q", y), ("Q", TAG_C), ("P", t1), ("P", t2), ("P", t3),
                          ("Q", tree_rows(q, [list(t) for t in t4], fmt)),
                          ("Q", tree_rows(q, [[x] for x in that], fmt)),
                          ("Q", tree_rows(q, [[x] for x in chain], fmt))], fmt)


def scan(q, rho_hat, up):
    """The chain recurrence, sequentially: R_i = rho^_i + u'_i R_{i-1}, U_i = u'_i U_{i-1}."""
    R, U, Rs, Us = 0, 1, [], []
    for a, b in zip(rho_hat, up):
        R, U = (a + b * R) % q, b * U % q
        Rs.append(R)
        Us.append(U)
    return Rs, Us


def prove(p, q, g, K, qbar, gseed, G, E, E2, psi, r, nonces, fmt="fixed"):
    N, w = len(E), len(E[0])
    if len(nonces) != 4 * N + 3 + w or len(G) != N + 2:
        raise ValueError("nonces: 4 N + 3 + w values; G: N + 2 elements")
    h, hs = G[0] % p, [x % p for x in G[1:N + 1]]
    nn = [x % q for x in nonces]
    rho, rho_hat, om_hat, om_p = nn[:N], nn[N:2 * N], nn[2 * N:3 * N], nn[3 * N:4 * N]
    om1, om2, om3 = nn[4 * N:4 * N + 3]
    om4 = nn[4 * N + 3:]
    pc = [None] * N
    for i in range(N):
        pc[psi[i]] = pow(g, rho[psi[i]], p) * hs[i] % p
    if any(x is None for x in pc):      # psi is no bijection: some commitment is never made
        pc = [1 % p if x is None else x for x in pc]
    y = seed(q, qbar, K, gseed, N, w, E, E2, pc, fmt)
    u = challenges(q, y, N, fmt)
    up = [u[psi[i]] for i in range(N)]
    Rs, Us = scan(q, rho_hat, up)
    chain = [pow(g, R, p) * pow(h, U, p) % p for R, U in zip(Rs, Us)]
    rbar, rhat = sum(rho) % q, Rs[-1]
    rtil = sum(a * b for a, b in zip(rho, u)) % q
    rstar = [sum((r[i][j] % q) * up[i] for i in range(N)) % q for j in range(w)]
    t1, t2 = pow(g, om1, p), pow(g, om2, p)
    t3 = pow(g, om3, p)
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
    c = challenge(q, y, t1, t2, t3, t4, that, chain, fmt)
    s = [(om1 + c * rbar) % q, (om2 + c * rhat) % q, (om3 + c * rtil) % q] + \
        [(om4[j] + c * rstar[j]) % q for j in range(w)]
    s_hat = [(om_hat[i] + c * rho_hat[i]) % q for i in range(N)]
    s_prime = [(om_p[i] + c * up[i]) % q for i in range(N)]
    return SimpleNamespace(pc=pc, chain=chain, c=c, s=s, s_hat=s_hat, s_prime=s_prime,
                           y=y, u=u, up=up, R=Rs, U=Us, t1=t1, t2=t2, t3=t3, t4=t4, that=that)


# ---- verify ------------------------------------------------------------------------------------
def _residue(p, q, x):
    return 0 < x < p and pow(x, q, p) == 1


def verify(p, q, g, K, qbar, gseed, G, E, E2, proof, check_inputs=False, fmt="fixed"):
    """-> (ok, failed): failed is a mask of RANGE, RESIDUE and CHALLENGE.  All three tests are always
    made; the recomputation reduces bases mod p and responses mod q."""
    N, w = len(E), len(E[0])
    failed = 0
    pc, chain, c = proof.pc, proof.chain, proof.c
    if c >= q or any(x >= q for x in list(proof.s) + list(proof.s_hat) + list(proof.s_prime)):
        failed |= RANGE
    els = [x for row in flat(E2) for x in row] + list(pc) + list(chain)
    if check_inputs:
        els += [x for row in flat(E) for x in row]
    if not all(_residue(p, q, x) for x in els):
        failed |= RESIDUE
    h, hs, hprod = G[0] % p, [x % p for x in G[1:N + 1]], G[N + 1] % p
    s = [x % q for x in proof.s]
    s_hat, s_prime = [x % q for x in proof.s_hat], [x % q for x in proof.s_prime]
    nc = (q - c % q) % q
    y = seed(q, qbar, K, gseed, N, w, E, E2, pc, fmt)
    u = challenges(q, y, N, fmt)
    U = 1
    for x in u:
        U = U * x % q
    cbar = pow(hprod, q - 1, p)
    ctil = 1
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
    if challenge(q, y, t1, t2, t3, t4, that, chain, fmt) != c:
        failed |= CHALLENGE
    return failed == 0, failed
