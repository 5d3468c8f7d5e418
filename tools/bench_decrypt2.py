#!/usr/bin/env python3
"""What does one combined proof per text cost against a proof per share?

One process, one context, in-process trustees: 5 guardians, quorum 3, 3 available (2 missing),
10,000 texts.  Two routes over the same texts, interleaved over the repetitions, each timed by a
host clock around calls that end in a stream synchronise:

  1.0  Decryption.decrypt_record and verify_decryption_record: unchanged code, the yardstick.
       Per text 9 exponentiations in each trustee, 36 in the mediator, 36 in the record verifier.
  2.0  Decryption2.decrypt_record and verify_decryption_record2: 3, 12 and 4.

Per route and repetition three phases:
  trustees  the time inside the trustees' calls (direct + compensated decrypt; commit + respond),
            taken by a proxy that lets one call run at a time, so a call never waits in its own
            measurement;
  mediator  decrypt_record minus the trustees: the checks and the combine, and in BOTH routes the
            same tail T = B / M and dLog, which `tail` times once on its own;
  verifier  the record verifier's call.
Before timing, both routes must give the same M bytes and the same counts.  Prints one line per
timing and one JSON summary line; --log also appends them to a file.

--ab-tree PATH, a built checkout of the parent commit, also alternates bench.py between this tree
and that one, --ab-rounds runs each.

    python tools/bench_decrypt2.py [--reps 5] [--texts 10000]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "electionguard-remote_amd"))

LOG = None
COUNTS = {"trustee": {"1.0": 9, "2.0": 3}, "mediator": {"1.0": 36, "2.0": 12}, "verifier": {"1.0": 36, "2.0": 4}}


def say(line):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


class Timed:
    """A trustee whose listed calls run one at a time and add their time to clock[0]."""
    lock = threading.Lock()

    def __init__(self, inner, names, clock):
        self._inner, self._names, self._clock = inner, names, clock

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name not in self._names:
            return attr

        def call(*args, **kw):
            with Timed.lock:
                t0 = time.perf_counter()
                try:
                    return attr(*args, **kw)
                finally:
                    self._clock[0] += time.perf_counter() - t0
        return call


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
    return {"tool": "bench_decrypt2 flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--texts", type=int, default=10000)
    ap.add_argument("--max-count", type=int, default=100)
    ap.add_argument("--log", default=None, help="append every printed line to this file")
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: also run the flagship A/B")
    ap.add_argument("--ab-only", action="store_true", help="skip the routes: the flagship A/B alone")
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

    from electionguard import decrypt as d1
    from electionguard import decrypt2 as d2
    from electionguard.core import productionGroup
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    n, qbar, n_g, quorum, n_avail = a.texts, 0xBE2C, 5, 3, 3
    gk, K = key_ceremony(group, n_g, quorum, seed=18)
    rng = np.random.default_rng(18)
    q_be = np.frombuffer(group.q.to_bytes(32, "big"), np.uint8)
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 0] = np.minimum(r[:, 0], q_be[0] - 1)
    votes = [int(x) for x in rng.integers(0, a.max_count + 1, n)]
    data = group.multP_batch(group.powP_batch(np.broadcast_to(np.frombuffer(K.to_bytes(512, "big"), np.uint8), (n, 512)),
                                              r), group.gPowP_batch(votes))
    T = np.ascontiguousarray(np.stack([group.gPowP_batch(r), data], axis=1))

    comm = {g.gid: g.commitments for g in gk}
    pub = {g.gid: g.public_key for g in gk}
    xs = {g.gid: g.x for g in gk}
    avail, missing = gk[:n_avail], [g.gid for g in gk[n_avail:]]
    clock = [0.0]
    old = d1.Decryption(group, qbar, [Timed(d1.DecryptingTrustee(group, g, comm), ("directDecrypt", "compensatedDecrypt"),
                                            clock) for g in avail], missing, pub)
    share_keys = d2.share_public_keys(group, comm, {g.gid: g.x for g in avail})
    new = d2.Decryption2(group, qbar, K, [Timed(d2.DecryptingTrustee2(group, g), ("commit", "respond"), clock)
                                          for g in avail], share_keys)
    routes = {
        "1.0": (lambda: old.decrypt_record(T, a.max_count),
                lambda rec: d1.verify_decryption_record(group, qbar, rec, pub, comm, xs, quorum, a.max_count)),
        "2.0": (lambda: new.decrypt_record(T, a.max_count),
                lambda rec: d2.verify_decryption_record2(group, qbar, K, rec, a.max_count)),
    }

    # warm-up (tables, workspaces) and agreement
    recs = {tag: run() for tag, (run, _) in routes.items()}
    assert recs["1.0"].counts == recs["2.0"].counts == votes, "the routes' counts differ"
    assert np.array_equal(old._shares_and_combine(T)[1], recs["2.0"].M), "the routes' M differ"
    for tag, (_, check) in routes.items():
        assert all(check(recs[tag]).values()), f"the {tag} record does not verify"
    say(f"agreement: {n} texts, byte-identical M, equal counts, both records verify")

    def tail():
        M = recs["2.0"].M
        d1.dlog_g_batch(group, group.multP_batch(np.ascontiguousarray(T[:, 1]), group.multInv_batch(M)), a.max_count)

    times = {f"{tag}_{ph}": [] for tag in routes for ph in ("trustees", "mediator", "verifier", "total")}
    times["tail"] = []
    for rep in range(a.reps):
        for tag, (run, check) in routes.items():
            clock[0] = 0.0
            group.sync()
            t0 = time.perf_counter()
            rec = run()
            group.sync()
            total = time.perf_counter() - t0
            t0 = time.perf_counter()
            check(rec)
            group.sync()
            ver = time.perf_counter() - t0
            for ph, dt in (("trustees", clock[0]), ("mediator", total - clock[0]), ("verifier", ver), ("total", total)):
                times[f"{tag}_{ph}"].append(dt)
                say(f"rep {rep} {tag} {ph:9s} {dt * 1e3:10.3f} ms")
        group.sync()
        t0 = time.perf_counter()
        tail()
        group.sync()
        times["tail"].append(time.perf_counter() - t0)
        say(f"rep {rep} tail (T = B / M, dLog; in both mediators) {times['tail'][-1] * 1e3:10.3f} ms")
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_decrypt2", "reps": a.reps, "texts": n, "guardians": n_g, "quorum": quorum, "available": n_avail,
        "exponentiations_per_text": COUNTS,
        "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
        "time_ratio_2_0_over_1_0": {ph: round(med["2.0_" + ph] / med["1.0_" + ph], 4)
                                    for ph in ("trustees", "mediator", "verifier", "total")},
        "mediator_without_tail_ms": {tag: round((med[tag + "_mediator"] - med["tail"]) * 1e3, 3) for tag in routes},
    }
    say(json.dumps(out))
    if a.ab_tree:
        group.close()   # the flagship runs get the device to themselves
        say(json.dumps(flagship_ab(a)))


if __name__ == "__main__":
    main()
