#!/usr/bin/env python3
"""What does a verifiable shuffle of a ballot table cost on the GPU?

One process, one context, device-resident inputs: N = 65,536 rows of w = 20 ciphertexts (a 4 x 5
ballot table without placeholders).  Five steps, interleaved over the repetitions, each timed by a
host clock around a call that ends in a stream synchronise:

  generators   eg_shuffle_generators_dev     N + 1 cofactor powers and their product
  mix          eg_shuffle_mix_dev
  prove        eg_shuffle_prove_dev
  verify       eg_shuffle_verify_dev         residue test of E', pc and chain
  verify+E     ... with check_inputs         and of E

Before timing, the proof must verify (ok = 1, mask = 0).  Next to each time: a Montgomery-multiply
model of the step, squarings included: the op programs' counts for the powers (a 32-byte variable
exponent 14 + 63 x 5 = 329, a 512-byte one 14 + 1023 x 5 = 5,129, a fixed-base term one multiply per
radix window), the plan's bounds for the products over N (eg_prod_pow_plan), N (2 w + 2) residue
tests of 329.  Not separated: the hashes, the scalar kernels, imports and exports, which the model
leaves out and the times include.  Prints one line per timing and one JSON summary line; --log also
appends them to a file.

--ab-tree PATH, a built checkout of the parent commit, also alternates bench.py between this tree
and that one, --ab-rounds runs each, the order swapped from round to round.

    python tools/bench_shuffle.py [--reps 5] [--rows 65536] [--width 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "electionguard-remote_amd"))

LOG = None
POW32, POW512 = 14 + 63 * 5, 14 + 1023 * 5


def say(line):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def flagship_ab(a):
    """bench.py alternated between the two trees, the order swapped each round -> summary dict"""
    runs = {"this": [], "parent": []}
    for rnd in range(a.ab_rounds):
        for arm in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):
            env = dict(os.environ)
            env.pop("EG_LIB", None)
            tree = ROOT if arm == "this" else Path(a.ab_tree).resolve()
            r = subprocess.run([sys.executable, str(tree / "bench.py"), "--gpus", "1", "--steps", str(a.ab_steps),
                                "--warmup", str(a.ab_warmup)], env=env, cwd=tree, capture_output=True, text=True,
                               timeout=900)
            if r.returncode != 0:
                sys.exit(f"bench.py ({arm}) failed with status {r.returncode}:\n{r.stderr[-2000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            runs[arm].append(json.loads(line)["value"])
            say(f"flagship round {rnd} {arm:6s} {line}")
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {"tool": "bench_shuffle flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def model(pp, N, w, F):
    """Montgomery multiplies per step (F: radix windows of g's and K's tables)."""
    over_n = pp.plan(1, N).mont_ops + sum(pp.plan(min(2 * w - r0, 1 << 16, (1 << 24) // N), N).mont_ops
                                          for r0 in range(0, 2 * w, min(1 << 16, (1 << 24) // N)))
    resid = N * (2 * w + 2) * POW32
    verify = resid + (N - 1) + 2 * POW32 + 2 + over_n + (3 + 2 * w) * (POW32 + F) + over_n + (1 + 2 * w) + \
        N * (POW32 + F) + N * POW32 + N
    return {
        "generators": (N + 1) * POW512 + (N - 1),
        "mix": 2 * N * w * (F - 1) + 2 * N * w,
        "prove": N * (F - 1) + N + 2 * N * (POW32 + F) + (3 + 2 * w) * (F - 1) + over_n + (1 + 2 * w),
        "verify": verify,
        "verify+E": verify + 2 * N * w * POW32,
        "residue tests": resid,
    }


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--width", type=int, default=20)
    ap.add_argument("--mm-rate", type=float, default=836e6, help="the flagship's multiplies per second (DESIGN §17)")
    ap.add_argument("--log", default=None, help="append every printed line to this file")
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: alternate bench.py")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--ab-steps", type=int, default=3)
    ap.add_argument("--ab-warmup", type=int, default=1)
    a = ap.parse_args()
    LOG = a.log
    if a.ab_tree:
        say(json.dumps(flagship_ab(a)))
        return

    from electionguard import prodpow as pp
    from electionguard import shuffle as S
    from electionguard.core import productionGroup

    group = productionGroup(0)
    N, w = a.rows, a.width
    rng = np.random.default_rng(19)
    q = group.q
    K = pow(group.g, int.from_bytes(rng.bytes(32), "big") % q, group.p)
    qbar, gseed = 0x1234567, 0xABCDEF
    # rows of subgroup elements g^e, made on the device
    exps = group.to_device(np.frombuffer(rng.bytes(N * w * 2 * 32), np.uint8).reshape(-1, 32))
    rows = group.device_empty((N, w, 2, 512))
    group.gPowP_batch_dev(exps.ptr, rows.ptr, N * w * 2)
    psi = group.to_device(rng.permutation(N).astype(np.uint32))
    r = group.to_device(np.frombuffer(rng.bytes(N * w * 32), np.uint8).reshape(N, w, 32))
    nonces = group.to_device(np.frombuffer(rng.bytes((4 * N + 3 + w) * 32), np.uint8).reshape(-1, 32))
    group.sync()

    state = {}

    def generators():
        state["G"] = S.generators(group, gseed, N, device=True)

    def mix():
        state["rows2"] = S.mix(group, K, rows, psi, r)

    def prove():
        state["proof"] = S.prove(group, K, qbar, gseed, state["G"], rows, state["rows2"], psi, r, nonces)

    def verify(check_inputs=False):
        state["verdict"] = S.verify(group, K, qbar, gseed, state["G"], rows, state["rows2"], state["proof"], check_inputs)

    steps = [("generators", generators), ("mix", mix), ("prove", prove), ("verify", verify),
             ("verify+E", lambda: verify(True))]
    for _, fn in steps:          # warm-up: tables, workspace, op programs; and the proof must verify
        fn()
    group.sync()
    ok, failed = state["verdict"]
    if (int(ok.download()[0]), int(failed.download()[0])) != (1, 0):
        sys.exit("the proof does not verify")
    times = {name: [] for name, _ in steps}
    for rep in range(a.reps):
        for name, fn in steps:
            group.sync()
            t0 = time.perf_counter()
            fn()
            group.sync()
            times[name].append(time.perf_counter() - t0)
            say(f"rep {rep} {name:10s} {times[name][-1] * 1e3:9.1f} ms")
    wb = getattr(group, "_fb_window_bits", 8)
    F = (256 + wb - 1) // wb
    mm = model(pp, N, w, F)
    out = {"tool": "bench_shuffle", "rows": N, "width": w, "reps": a.reps, "fb_windows": F, "mm_rate": a.mm_rate,
           "steps": {}}
    for name, _ in steps:
        med = statistics.median(times[name])
        out["steps"][name] = {"ms_median": round(med * 1e3, 1), "ms_min": round(min(times[name]) * 1e3, 1),
                              "ms_max": round(max(times[name]) * 1e3, 1), "model_mm": round(mm[name]),
                              "model_ms": round(mm[name] / a.mm_rate * 1e3, 1),
                              "time_over_model": round(med / (mm[name] / a.mm_rate), 2)}
    out["residue_tests_mm"] = round(mm["residue tests"])
    say(json.dumps(out))


if __name__ == "__main__":
    main()
