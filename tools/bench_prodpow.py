#!/usr/bin/env python3
"""What does the multi-exponentiation save over one exponentiation per term?

One process, one context, device-resident inputs, two shapes:

  combine          100,000 rows x 5 terms, layout "rows"   (the mediator's Lagrange combine)
  shuffle column   8 rows x 2^18 terms, layout "terms"     (one exponent vector over 8 columns)

Two arms per shape on the same elements, interleaved over the repetitions, each timed by a host
clock around calls that end in a stream synchronise:

  prod_pow   eg_prod_pow_dev, method and width chosen by its plan (at most 2^16 rows per call)
  yardstick  eg_powp_batch_dev into a scratch array, then eg_prod_reduce: unchanged code, the only
             route before.  It gets the layout it needs (each row's terms side by side), so no
             transposing copy is charged to it; eg_prod_reduce takes host pointers, so its scratch
             comes down first, as any caller of that route has to do.

Before timing, the arms' results must be byte-identical.  Next to the times: the yardstick's k_pow
multiply count from eg_ctx_profile_begin / end and the plan's bound for the new arm.  Prints one
line per timing and one JSON summary line; --log also appends them to a file.

--ab-tree PATH, a built checkout of the parent commit, also alternates bench.py between this tree
and that one, --ab-rounds runs each.

    python tools/bench_prodpow.py [--reps 5] [--texts 100000] [--k 5] [--columns 8] [--terms 262144]
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
        for arm in ("this", "parent"):
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
    return {"tool": "bench_prodpow flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--texts", type=int, default=100000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--terms", type=int, default=1 << 18)
    ap.add_argument("--log", default=None, help="append every printed line to this file")
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: also run the flagship A/B")
    ap.add_argument("--ab-only", action="store_true", help="skip the arms: the flagship A/B alone")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--ab-steps", type=int, default=3)
    ap.add_argument("--ab-warmup", type=int, default=1)
    a = ap.parse_args()
    LOG = a.log
    if a.ab_only:
        if not a.ab_tree:
            sys.exit("--ab-only needs --ab-tree")
        say(json.dumps(flagship_ab(a)))
        return

    from electionguard import prodpow as pp
    from electionguard.core import productionGroup

    group = productionGroup(0)
    rng = np.random.default_rng(17)
    q_be = np.frombuffer(group.q.to_bytes(32, "big"), np.uint8)

    def below_q(n):
        e = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        e[:, 0] = np.minimum(e[:, 0], q_be[0] - 1)
        return e

    def elements(n):
        """n random members of the subgroup, made on the device: g^x for random x."""
        d_x, d = group.to_device(below_q(n)), group.device_empty((n, 512))
        group.gPowP_batch_dev(d_x.ptr, d.ptr, n)
        group.sync()
        d_x.free()
        return d

    shapes, keep = {}, []
    for tag, rows, n, layout in (("combine", a.texts, a.k, "rows"), ("column", a.columns, a.terms, "terms")):
        exps = below_q(n) if tag == "combine" else rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        d_rows = elements(rows * n)                      # (rows, n, 512): each row's terms side by side
        d_rows.shape = (rows, n, 512)
        if layout == "rows":
            d_new = d_rows
        else:                                            # the same elements as (n, rows, 512)
            d_new = group.to_device(np.ascontiguousarray(d_rows.download().transpose(1, 0, 2)))
        d_e = group.to_device(exps)
        d_e_all = group.to_device(np.ascontiguousarray(np.broadcast_to(exps, (rows, n, 32))))   # one exponent per element
        d_scratch, d_out = group.device_empty((rows * n, 512)), group.device_empty((rows, 512))

        def new(d_new=d_new, d_e=d_e, d_out=d_out, rows=rows, layout=layout):
            if layout == "rows":
                for r0 in range(0, rows, pp.MAX_ROWS):
                    pp.prod_pow(group, d_new[r0:r0 + pp.MAX_ROWS], d_e, layout="rows", out=d_out[r0:r0 + pp.MAX_ROWS])
            else:
                pp.prod_pow(group, d_new, d_e, layout="terms", out=d_out)
            group.sync()

        def old(d_rows=d_rows, d_e_all=d_e_all, d_scratch=d_scratch, rows=rows, n=n):
            group.powP_batch_dev(d_rows.ptr, d_e_all.ptr, d_scratch.ptr, rows * n)
            return group.prodP_groups(d_scratch.download(), rows, n)      # ends in a stream synchronise

        new()
        group.profile_begin()
        want = old()
        prof = group.profile_end()
        assert np.array_equal(d_out.download(), want), f"{tag}: the arms differ"
        bound = sum(pp.plan(min(pp.MAX_ROWS, rows - r0), n).mont_ops for r0 in range(0, rows, pp.MAX_ROWS))
        pl = pp.plan(min(rows, pp.MAX_ROWS), n)
        shapes[tag] = {"rows": rows, "n": n, "layout": layout, "method": pl.method, "window_bits": pl.window_bits,
                       "plan_mont_ops": bound, "yardstick_kpow_mont_ops": prof.mont_ops,
                       "yardstick_prod_multiplies": rows * (n - 1),
                       "multiply_ratio": round(bound / (prof.mont_ops + rows * (n - 1)), 4)}
        say(f"{tag}: byte-identical; {json.dumps(shapes[tag])}")
        keep.append((tag, new, old, [d_rows, d_new, d_e, d_e_all, d_scratch, d_out]))

    times = {f"{tag}_{arm}": [] for tag, *_ in keep for arm in ("prod_pow", "yardstick")}
    for rep in range(a.reps):
        for tag, new, old, _ in keep:
            for arm, fn in (("prod_pow", new), ("yardstick", old)):
                group.sync()
                t0 = time.perf_counter()
                fn()
                group.sync()
                dt = time.perf_counter() - t0
                times[f"{tag}_{arm}"].append(dt)
                say(f"rep {rep} {tag:8s} {arm:10s} {dt * 1e3:10.3f} ms")
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_prodpow", "reps": a.reps, "shapes": shapes,
        "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
        "time_ratio": {tag: round(med[tag + "_prod_pow"] / med[tag + "_yardstick"], 4) for tag, *_ in keep},
        "slowest_new_below_fastest_yardstick": {tag: max(times[tag + "_prod_pow"]) < min(times[tag + "_yardstick"])
                                                for tag, *_ in keep},
    }
    say(json.dumps(out))
    if a.ab_tree:
        for *_, bufs in keep:
            for x in set(bufs):
                x.free()
        group.close()   # the flagship runs get the device to themselves
        say(json.dumps(flagship_ab(a)))


if __name__ == "__main__":
    main()
