#!/usr/bin/env python3
"""What does the device-side decode cost against the present route?

One process, one context.  Two routes from the same host arrays B and M (texts B = M * g^t with
M = g^r) to the counts t, interleaved over the repetitions, each timed by a host clock around
calls that end in a stream synchronise:

  host    group.multInv_batch(M), group.multP_batch(B, .), decrypt.dlog_g_batch(., max_count): the
          tail of Decryption.decrypt_record and Decryption2.decrypt_record, unchanged code.
  device  decode.decode_counts(group, B, M, max_count) on the same host arrays (uploads included),
          and `resident`, the same call on DeviceBuffers followed by a synchronise.

Three shapes: 10,000 texts of counts 0..100; 1,000 texts of counts up to 1,000,000; 65,536 x 20
texts of values 0..3.  Where a shape has more texts than --host-sample, the host route is timed on
the first --host-sample texts only and its figure for the whole shape is that time scaled by the
number of texts (said in the output: `host_sampled`).  Before anything is timed the routes' counts
must be equal, and equal to the t the texts were made from.

`model` is eg_decode_plan's mont_ops (an upper bound: inversion, B / M, giant steps) at --rate
Montgomery multiplies per second, the flagship's rate.  Prints one line per timing and one JSON
summary line per shape; --log also appends them to a file.

--ab-tree PATH, a built checkout of the parent commit, also alternates bench.py between this tree
and that one, --ab-rounds runs each, the order swapped between rounds.

    python tools/bench_decode.py [--reps 5] [--shapes 10000:100,1000:1000000,1310720:3]
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


def say(line):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def flagship_ab(a):
    """bench.py alternated between the two trees -> summary dict"""
    runs = {"this": [], "parent": []}
    for rnd in range(a.ab_rounds):
        for arm in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):   # neither tree always goes first
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
    return {"tool": "bench_decode flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def make_texts(group, n, max_count, rng):
    """-> (B, M, t): M = g^r, B = M * g^t for t uniform in 0..max_count."""
    q_be = np.frombuffer(group.q.to_bytes(32, "big"), np.uint8)
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 0] = np.minimum(r[:, 0], q_be[0] - 1)
    t = rng.integers(0, max_count + 1, n)
    uniq, where = np.unique(t, return_inverse=True)
    gt = group.gPowP_batch([int(x) for x in uniq])[where]
    M = group.gPowP_batch(r)
    return group.multP_batch(M, gt), M, t.astype(np.int64)


def timed(group, fn):
    group.sync()
    t0 = time.perf_counter()
    out = fn()
    group.sync()
    return time.perf_counter() - t0, out


def run_shape(group, a, n, max_count, seed):
    from electionguard import decode as dc
    from electionguard.decrypt import dlog_g_batch

    rng = np.random.default_rng(seed)
    B, M, t = make_texts(group, n, max_count, rng)
    ns = min(n, a.host_sample)
    Bs, Ms = np.ascontiguousarray(B[:ns]), np.ascontiguousarray(M[:ns])
    host = lambda: dlog_g_batch(group, group.multP_batch(Bs, group.multInv_batch(Ms)), max_count)
    device = lambda: dc.decode_counts(group, B, M, max_count)
    dB, dM = group.to_device(B), group.to_device(M)
    resident = lambda: dc.decode_counts(group, dB, dM, max_count)

    # warm-up (table, workspaces) and agreement
    got_h, got_d, got_r = host(), device(), resident().download()
    assert [-1 if c is None else c for c in got_h] == t[:ns].tolist(), "the host route's counts are not the texts'"
    assert np.array_equal(got_d, t) and np.array_equal(got_r, t), "the device route's counts are not the texts'"
    tag = f"{n}:{max_count}"
    say(f"shape {tag}: agreement on {n} texts (host route on {ns})")

    times = {"host": [], "device": [], "resident": []}
    for rep in range(a.reps):
        for name, fn in (("host", host), ("device", device), ("resident", resident)):
            dt, _ = timed(group, fn)
            times[name].append(dt)
            say(f"shape {tag} rep {rep} {name:8s} {dt * 1e3:10.3f} ms")
    p = dc.plan(n, max_count)
    med = {k: statistics.median(v) for k, v in times.items()}
    host_whole = med["host"] * n / ns
    model_ms = p.mont_ops / a.rate * 1e3
    out = {
        "tool": "bench_decode", "reps": a.reps, "texts": n, "max_count": max_count, "host_texts": ns,
        "host_sampled": ns < n, "plan": p._asdict(),
        "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
        "host_ms_scaled_to_all_texts": round(host_whole * 1e3, 3),
        "host_over_device": round(host_whole / med["device"], 3),
        "host_over_resident": round(host_whole / med["resident"], 3),
        "model_M_multiplies": round(p.mont_ops / 1e6, 3), "model_ms": round(model_ms, 3),
        "resident_over_model": round(med["resident"] * 1e3 / model_ms, 2),
    }
    say(json.dumps(out))
    dB.free()
    dM.free()
    dc.close_tables(group)


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="10000:100,1000:1000000,1310720:3", help="texts:max_count, comma separated")
    ap.add_argument("--host-sample", type=int, default=65536, help="most texts the host route is timed on")
    ap.add_argument("--rate", type=float, default=836e6, help="Montgomery multiplies per second of the model")
    ap.add_argument("--log", default=None, help="append every printed line to this file")
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: also run the flagship A/B")
    ap.add_argument("--ab-only", action="store_true", help="skip the shapes: the flagship A/B alone")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--ab-steps", type=int, default=3)
    ap.add_argument("--ab-warmup", type=int, default=1)
    a = ap.parse_args()
    LOG = a.log
    if a.reps < 5:
        sys.exit("at least five repetitions")
    if a.ab_only:
        if not a.ab_tree:
            sys.exit("--ab-only needs --ab-tree")
        say(json.dumps(flagship_ab(a)))
        return

    from electionguard.core import productionGroup

    group = productionGroup(0)
    for k, shape in enumerate(a.shapes.split(",")):
        n, max_count = (int(x) for x in shape.split(":"))
        run_shape(group, a, n, max_count, 20 + k)
    if a.ab_tree:
        group.close()   # the flagship runs get the device to themselves
        say(json.dumps(flagship_ab(a)))


if __name__ == "__main__":
    main()
