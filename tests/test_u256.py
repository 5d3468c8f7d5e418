"""CPU: the 256-bit scalar arithmetic of the proofs (electionguard-remote_amd/csrc/eg_u256.hpp), by
tests/cpp/u256_test.cpp: the header's functions, the bodies the device kernels inline, compiled as
host code and run on operands drawn here, against Python integers.  Every function is run for the
production q = 2^256 - 189 and, where its contract allows a small q, for a 32-bit prime; the
program is built with g++'s address and undefined-behaviour sanitizers when their runtimes are
installed (it is a stand-alone program), and without them otherwise."""
import random
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "electionguard-remote_amd" / "csrc"

M = 1 << 256
Q_TOP = M - 189
Q_SMALL = 4294967291  # 2^32 - 5, prime


def _h(x):
    assert 0 <= x < M
    return f"{x:064x}"


def _cases():
    """[(input line, expected output line)]"""
    rng = random.Random(0x256)
    out = []
    add = lambda line, want: out.append((line, want))

    def specials(q):
        return [0, 1, q - 1, q, q + 1, 1 << 255, M - 1]

    anyv = sorted(set(specials(Q_TOP) + specials(Q_SMALL)))
    rnd = [rng.randrange(M) for _ in range(40)] + [rng.randrange(1 << rng.randrange(1, 257)) for _ in range(40)]

    # no modulus: words in and out, constants, compare, select, add with carry, subtract with borrow
    for a in anyv + rnd[:8]:
        add(f"words {_h(a)}", _h(a))
        add(f"ldst {_h(a)}", _h(a))
    for v in (0, 1, 255, 256, (1 << 32) - 1):
        add(f"small {v:x}", _h(v))
    add("zero", _h(0))
    pairs = [(a, b) for a in anyv for b in anyv] + list(zip(rnd, reversed(rnd)))
    pairs += [(M - 1, 1), ((1 << 32) - 1, 1), ((1 << 224) - 1, 1)]        # carries out of add256, and along it
    pairs += [(0, 1), (1 << 32, 1), (1 << 255, (1 << 255) + 1), (5, M - 1)]  # borrows in sub256, and along it
    for a, b in pairs:
        add(f"eq {_h(a)} {_h(b)}", "1" if a == b else "0")
        add(f"lt {_h(a)} {_h(b)}", "1" if a < b else "0")
        add(f"add {_h(a)} {_h(b)}", f"{_h((a + b) % M)} {(a + b) // M}")
        add(f"sub {_h(a)} {_h(b)}", f"{_h((a - b) % M)} {1 if a < b else 0}")
    for a, b in pairs[:20]:
        add(f"sel ffffffff {_h(a)} {_h(b)}", _h(a))
        add(f"sel 0 {_h(a)} {_h(b)}", _h(b))

    for q in (Q_TOP, Q_SMALL):
        below = sorted({v for v in specials(q) if v < q})  # 0, 1, q - 1 and, for the top q, 2^255
        rq = [rng.randrange(q) for _ in range(150)]
        mod_pairs = [(a, b) for a in below for b in below] + list(zip(rq, reversed(rq)))
        for a, b in mod_pairs:
            add(f"addmod {_h(a)} {_h(b)} {_h(q)}", _h((a + b) % q))
            add(f"submod {_h(a)} {_h(b)} {_h(q)}", _h((a - b) % q))
            add(f"mulmod {_h(a)} {_h(b)} {_h(q)}", _h(a * b % q))
        for a in below + rq[:40]:
            add(f"negmod {_h(a)} {_h(q)}", _h(-a % q))
            for k in (0, 1, 2, 128, 255, rng.randrange(256)):
                add(f"mulbyte {_h(a)} {k:x} {_h(q)}", _h(k * a % q))
        # the any-q reduction takes every 256-bit x
        for x in anyv + rnd + rq[:20]:
            add(f"modany {_h(x)} {_h(q)}", _h(x % q))
        # mulsmall_mod subtracts q floor(L a / q) times (it is for public values), so the operands
        # keep that count bounded: any a with L <= 1 and a small L, and L = 2^32 - 1 with an a
        # that makes the product a few q, a thousand q and 65,535 q (the top word `hi` then
        # takes that many borrows, one every few subtractions or every one)
        few = [0, 1, 2, 3 * q >> 32, 7 * q >> 32, (1000 * q >> 32) + 12345, 65535 * q >> 32]
        for a in below + rq[:40]:
            for L in (0, 1, 2, rng.randrange(3, 4096)):
                add(f"mulsmall {_h(a)} {L:x} {_h(q)}", _h(L * a % q))
        for a in few:
            add(f"mulsmall {_h(a)} ffffffff {_h(q)}", _h(((1 << 32) - 1) * a % q))
    add(f"modany {_h(M - 1)} {_h(Q_SMALL)}", _h((M - 1) % Q_SMALL))
    return out


def _sanitizers(tmp_path):
    """the sanitizer flags if g++ can link a program with them here, else none"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True)
    if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
        return flags
    print("g++'s sanitizer runtimes are not installed: u256_test runs without them")
    return []


def test_u256_functions_against_python_integers(tmp_path):
    exe = tmp_path / "u256_test"
    # -Wno-unknown-pragmas: the header's "#pragma unroll" is hipcc's
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    *_sanitizers(tmp_path), "-I", str(CSRC), "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "u256_test.cpp")], check=True)
    cases = _cases()
    inp = tmp_path / "cases.txt"
    inp.write_text("".join(line + "\n" for line, _ in cases))
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases), (len(got), len(cases), r.stderr[-2000:])
    bad = [(line, want, g) for (line, want), g in zip(cases, got) if g != want]
    assert not bad, (len(bad), bad[:5])
    ops = {line.split()[0] for line, _ in cases}
    assert ops == {"words", "ldst", "small", "zero", "eq", "lt", "sel", "add", "sub", "addmod", "submod", "negmod",
                   "mulsmall", "mulmod", "mulbyte", "modany"}
