#!/usr/bin/env python3
"""What does a ballot without placeholders cost beside the same election in the 1.0 form?

One process, one context, device-resident ballots.  Arms interleaved over the repetitions, each
timed by a host clock around one call that ends in a stream synchronise:

  v1     eg_encrypt_ballots_manifest_dev / eg_verify_ballots_manifest_dev on 4 x (5+1), limit 1:
         unchanged code, the yardstick (24 selection proofs and 4 constant proofs per ballot)
  v2 L1  eg_encrypt_ballots_v2_dev / eg_verify_ballots_v2_dev on 4 x (5, 1, 1): the same votes on the
         same real selections (24 range items per ballot: 20 selections and 4 contests)
  v2 L3  the same on 4 x (5, 3, 3), votes up to 3 per selection and contest

Before timing every ballot is verified once and the k_pow multiplies per ballot are read from the
context's profile.  Prints one line per timing and one JSON summary line: medians, min-max spreads,
ballots per second and the ratios to the yardstick.

With --ab-tree PARENT it then runs the flagship line, bench.py --gpus 1, alternated between this
tree and a built checkout of the parent commit (its own bench.py, package and library), one fresh
process per run, and prints each run's JSON line and the ratio of the medians.

    python tools/bench_ballot2.py [--ballots 10000] [--reps 5] [--fb-window 12]
                                  [--ab-tree PATH [--ab-only] --ab-rounds 3 --ab-steps 3 --ab-warmup 1]
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
            print(f"flagship round {rnd} {arm:6s} {line}", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {"tool": "bench_ballot2 flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ballots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fb-window", type=int, default=12)
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: also run the flagship A/B")
    ap.add_argument("--ab-only", action="store_true", help="skip the ballot arms: the flagship A/B alone")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=3)
    ap.add_argument("--ab-warmup", type=int, default=1)
    a = ap.parse_args()
    if a.ab_only:
        if not a.ab_tree:
            sys.exit("--ab-only needs --ab-tree")
        print(json.dumps(flagship_ab(a)), flush=True)
        return

    from electionguard import ballot2 as B2
    from electionguard.ballot import (ElectionKey, ElectionManifest, Verifier, batch_encryption_device, random_scalars,
                                      random_votes)
    from electionguard.core import native, productionGroup
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, nb = 0xBEEF, a.ballots
    rng = np.random.default_rng(12)
    lib, h = group._lib, group.handle
    Kb, qb = native.buf(key.K_be), native.buf(qbar.to_bytes(32, "big"))
    arms, mm, keep = {}, {}, []

    # ---- the yardstick: the 1.0 form, 4 x (5 real + 1 placeholder), limit 1 ----
    man1 = ElectionManifest([(5, 1)] * 4)
    votes1 = random_votes(rng, man1, nb)
    d_v1 = group.to_device(votes1)
    d_sn1 = group.to_device(random_scalars(rng, (nb, man1.nsel, 4), group.q))
    d_cn1 = group.to_device(random_scalars(rng, (nb, man1.n_contests), group.q))
    d_c1, d_r1, d_p1 = (group.device_empty(s) for s in ((nb, man1.nsel, 2, 512), (nb, man1.nsel, 4, 32),
                                                        (nb, man1.n_contests, 2, 32)))
    d_os1, d_oc1 = group.device_empty((nb, man1.nsel)), group.device_empty((nb, man1.n_contests))
    d_t1 = group.device_empty((man1.n_real, 2, 512))
    V1 = Verifier(group, key, qbar, man1)

    def enc1():
        batch_encryption_device(group, key, qbar, man1, nb, d_v1.ptr, d_sn1.ptr, d_cn1.ptr, d_c1.ptr, d_r1.ptr, d_p1.ptr)

    def ver1():
        V1.verify_device(d_c1.ptr, d_r1.ptr, d_p1.ptr, nb, d_os1.ptr, d_oc1.ptr, d_t1.ptr)

    arms["v1_encrypt"], arms["v1_verify"] = enc1, ver1

    # ---- the 2.0 form: the same votes on the real selections, then limits of 3 ----
    real = votes1[:, man1.real_index]
    for tag, L in (("v2_L1", 1), ("v2_L3", 3)):
        man = B2.Manifest2([(5, L, L)] * 4)
        votes = real if L == 1 else B2.random_votes2(rng, man, nb)
        sn, cn = B2.random_nonces2(rng, man, nb, group.q)
        d = [group.to_device(x) for x in (votes, sn, cn)]
        out = [group.device_empty(s) for s in ((nb, man.NS, 2, 512), (nb, man.SP, 2, 32), (nb, man.CP, 2, 32),
                                               (nb, man.NS), (nb, man.n_contests), (man.NS, 2, 512))]
        keep.append((man, d, out))
        shape = man._shape_args()

        def enc(shape=shape, d=d, out=out):
            native.check(lib, "eg_encrypt_ballots_v2_dev",
                         lib.eg_encrypt_ballots_v2_dev(h, Kb, qb, nb, *shape, d[0].ptr, d[1].ptr, d[2].ptr, out[0].ptr,
                                                       out[1].ptr, out[2].ptr))

        def ver(shape=shape, out=out):
            native.check(lib, "eg_verify_ballots_v2_dev",
                         lib.eg_verify_ballots_v2_dev(h, Kb, qb, nb, *shape, out[0].ptr, out[1].ptr, out[2].ptr, None,
                                                      out[3].ptr, out[4].ptr, out[5].ptr))

        arms[tag + "_encrypt"], arms[tag + "_verify"] = enc, ver

    # ---- once untimed (tables, op programs), every verdict checked, multiplies from the profile ----
    for name, fn in arms.items():
        fn()
        group.sync()
        group.profile_begin()
        fn()
        p = group.profile_end()
        mm[name] = {"mm_per_ballot": round(p.mont_ops / nb, 1), "k_pow_launches": p.launches}
        print(f"{name:14s} {mm[name]['mm_per_ballot']:9.1f} k_pow multiplies per ballot, {p.launches} k_pow launches",
              flush=True)
    assert group.all_nonzero(d_os1) and group.all_nonzero(d_oc1), "the yardstick's ballots do not verify"
    for man, d, out in keep:
        assert group.all_nonzero(out[3]) and group.all_nonzero(out[4]), f"{man} ballots do not verify"

    times = {name: [] for name in arms}
    for rep in range(a.reps):
        for name, fn in arms.items():
            group.sync()
            t0 = time.perf_counter()
            fn()
            group.sync()
            dt = time.perf_counter() - t0
            times[name].append(dt)
            print(f"rep {rep} {name:14s} {dt * 1e3:9.3f} ms per call  {nb / dt:12.1f} ballots/s", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_ballot2", "ballots": nb, "reps": a.reps, "fb_window": a.fb_window,
        "shapes": {"v1": "4x(5+1) limit 1", "v2_L1": "4x(5,1,1)", "v2_L3": "4x(5,3,3)"},
        "chunk_ballots": {"v2_L1": B2.chunk_ballots(keep[0][0]), "v2_L3": B2.chunk_ballots(keep[1][0])},
        "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
        "ballots_per_s": {k: round(nb / v, 1) for k, v in med.items()},
        "time_over_yardstick": {k: round(med[k] / med["v1_" + k.split("_")[-1]], 4) for k in med if k[:2] == "v2"},
        "k_pow": mm,
    }
    print(json.dumps(out), flush=True)
    if a.ab_tree:
        for _, d, o in keep:
            for x in d + o:
                x.free()
        group.close()   # the flagship runs get the device to themselves
        print(json.dumps(flagship_ab(a)), flush=True)


if __name__ == "__main__":
    main()
