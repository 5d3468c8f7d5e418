#!/usr/bin/env python3
"""What does the manifest path (eg_verify_ballots_manifest) cost beside the uniform one?

One process, one context, GPU-made ballots.  Three arms, each verifying + tallying the same
number of ballots from host memory, interleaved over the repetitions:

  uniform   eg_verify_ballots            at 4 x (5+1)
  same      eg_verify_ballots_manifest   given that same shape as four equal contests
  ragged    eg_verify_ballots_manifest   at [(2,1), (8,1), (5,1), (5,1)]: the same 24 selections
                                         and 4 contests in three size classes

Prints one line per timed call and one JSON summary line (medians, the uniform arm's min-max
spread, the ratios to the uniform median).

    python tools/bench_manifest.py [--ballots 10000] [--reps 5] [--fb-window 12]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "electionguard-remote_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ballots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fb-window", type=int, default=12)
    a = ap.parse_args()

    from electionguard.ballot import (ElectionKey, ElectionManifest, Manifest, Verifier, batch_encryption,
                                      random_scalars, random_votes)
    from electionguard.core import productionGroup
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar = 0xBEEF
    nb = a.ballots
    arms = {
        "uniform": Manifest(4, 5, 1),
        "same": ElectionManifest([(5, 1)] * 4),
        "ragged": ElectionManifest([(2, 1), (8, 1), (5, 1), (5, 1)]),
    }
    work = {}
    for name, man in arms.items():
        rng = np.random.default_rng(9)
        eb = batch_encryption(group, key, qbar, man, random_votes(rng, man, nb),
                              random_scalars(rng, (nb, man.nsel, 4), group.q),
                              random_scalars(rng, (nb, man.n_contests), group.q))
        V = Verifier(group, key, qbar, man)
        ok_s, ok_c, _ = V.verify(eb)  # warm-up: tables, workspaces, op programs
        assert ok_s.all() and ok_c.all(), name
        work[name] = (V, eb)
    times = {name: [] for name in arms}
    for rep in range(a.reps):
        for name, (V, eb) in work.items():
            t0 = time.perf_counter()
            ok_s, ok_c, _ = V.verify(eb)
            dt = time.perf_counter() - t0
            assert ok_s.all() and ok_c.all(), name
            times[name].append(dt)
            print(f"rep {rep} {name:8s} {dt * 1e3:9.2f} ms  {nb / dt:10.0f} ballots/s", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_manifest", "ballots": nb, "reps": a.reps, "fb_window": a.fb_window,
        "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "uniform_min_max_ms": [round(min(times["uniform"]) * 1e3, 3), round(max(times["uniform"]) * 1e3, 3)],
        "ratio_to_uniform": {k: round(med[k] / med["uniform"], 4) for k in ("same", "ragged")},
        "all_ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
