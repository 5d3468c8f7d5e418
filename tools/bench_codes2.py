#!/usr/bin/env python3
"""What do seeded nonces, ballot hashes and the opening cost beside verification, for ballots
without placeholders?

One process, one context, 10,000 device-resident ballots of 4 x (5, 1, 1) and of 4 x (5, 3, 3),
encrypted from nonces derived on the device.  Four arms per shape on the same buffers, interleaved
over the repetitions, each timed by a host clock around calls that end in a stream synchronise:

  nonces   eg_derive_ballot_nonces_v2_dev   the SN + CN nonce rows of every ballot
  hashes   eg_ballot_hashes_dev, spc = nsel selection, contest and ballot hashes of every ballot
  open     eg_open_ballots_v2_dev           R per selection, g^R, K^R and the match, in chunks
  verify   eg_verify_ballots_v2_dev         proofs + tally: unchanged code, the yardstick

The two hashing arms run --inner calls per timing (the figure reported is per call).  Before
timing, the opening must return the votes with every flag set and the first ballots' nonces and
hashes are checked against the host mirrors.  Prints one line per timing and one JSON summary line.

--ab-tree PATH, a built checkout of the parent commit, also alternates bench.py between this tree
and that one, --ab-rounds runs each.

    python tools/bench_codes2.py [--ballots 10000] [--reps 5] [--inner 10] [--fb-window 12]
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
    return {"tool": "bench_codes2 flagship A/B", "rounds": a.ab_rounds, "steps": a.ab_steps, "warmup": a.ab_warmup,
            "ballots_per_s": runs, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ballots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--fb-window", type=int, default=12)
    ap.add_argument("--ab-tree", default=None, help="a built checkout of the parent commit: also run the flagship A/B")
    ap.add_argument("--ab-only", action="store_true", help="skip the arms: the flagship A/B alone")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--ab-steps", type=int, default=3)
    ap.add_argument("--ab-warmup", type=int, default=1)
    a = ap.parse_args()
    if a.ab_only:
        if not a.ab_tree:
            sys.exit("--ab-only needs --ab-tree")
        print(json.dumps(flagship_ab(a)), flush=True)
        return

    from electionguard import ballot2 as B2
    from electionguard import codes as C
    from electionguard import codes2 as C2
    from electionguard.ballot import ElectionKey
    from electionguard.core import native, productionGroup
    from electionguard.core.marshal import u32p
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, nb = 0xBEEF, a.ballots
    rng = np.random.default_rng(16)
    lib, h = group._lib, group.handle
    Kb, qb = native.buf(key.K_be), native.buf(qbar.to_bytes(32, "big"))
    r = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    arms, keep = {}, []

    for tag, L in (("L1", 1), ("L3", 3)):
        man = B2.Manifest2([(5, L, L)] * 4)
        NS, nc = man.NS, man.n_contests
        votes, bn, ids = B2.random_votes2(rng, man, nb), r(nb, 32), r(nb, 32)
        hashes = C.ManifestHashes(r(NS, 32), r(nc, 32), r(32))
        d_bn, d_ids, d_votes = group.to_device(bn), group.to_device(ids), group.to_device(votes)
        d_desc = group.to_device(np.concatenate([hashes.dsel.reshape(-1), hashes.dcon.reshape(-1), hashes.manifest_hash]))
        d_sn, d_cn = group.device_empty((nb, man.SN, 32)), group.device_empty((nb, man.CN, 32))
        d_cts, d_sp, d_cp = (group.device_empty(s) for s in ((nb, NS, 2, 512), (nb, man.SP, 2, 32), (nb, man.CP, 2, 32)))
        d_B, d_ov, d_ok = group.device_empty((nb, 32)), group.device_empty((nb, NS)), group.device_empty((nb, NS))
        d_oks, d_okc, d_tal = group.device_empty((nb, NS)), group.device_empty((nb, nc)), group.device_empty((NS, 2, 512))
        shape, spc = man._shape_args(), u32p(man.nsel)

        def nonces(shape=shape, d_bn=d_bn, d_sn=d_sn, d_cn=d_cn):
            native.check(lib, "eg_derive_ballot_nonces_v2_dev",
                         lib.eg_derive_ballot_nonces_v2_dev(h, nb, *shape, d_bn.ptr, d_sn.ptr, d_cn.ptr))

        def hash_ballots(nc=nc, NS=NS, spc=spc, d=d_desc, d_ids=d_ids, d_cts=d_cts, d_B=d_B):
            native.check(lib, "eg_ballot_hashes_dev",
                         lib.eg_ballot_hashes_dev(h, nb, nc, spc, d.ptr, d.ptr + NS * 32, d.ptr + (NS + nc) * 32,
                                                  d_ids.ptr, d_cts.ptr, d_B.ptr, None, None))

        def open_ballots(shape=shape, d_bn=d_bn, d_cts=d_cts, d_ov=d_ov, d_ok=d_ok):
            native.check(lib, "eg_open_ballots_v2_dev",
                         lib.eg_open_ballots_v2_dev(h, Kb, nb, *shape, d_bn.ptr, d_cts.ptr, d_ov.ptr, d_ok.ptr))

        def verify(shape=shape, d_cts=d_cts, d_sp=d_sp, d_cp=d_cp, d_oks=d_oks, d_okc=d_okc, d_tal=d_tal):
            native.check(lib, "eg_verify_ballots_v2_dev",
                         lib.eg_verify_ballots_v2_dev(h, Kb, qb, nb, *shape, d_cts.ptr, d_sp.ptr, d_cp.ptr, None,
                                                      d_oks.ptr, d_okc.ptr, d_tal.ptr))

        # the ballots, from nonces derived on the device; then every arm once untimed and checked
        nonces()
        native.check(lib, "eg_encrypt_ballots_v2_dev",
                     lib.eg_encrypt_ballots_v2_dev(h, Kb, qb, nb, *shape, d_votes.ptr, d_sn.ptr, d_cn.ptr, d_cts.ptr,
                                                   d_sp.ptr, d_cp.ptr))
        hash_ballots()
        open_ballots()
        verify()
        group.sync()
        assert group.all_nonzero(d_oks) and group.all_nonzero(d_okc), f"{man}: the bench's own ballots do not verify"
        assert group.all_nonzero(d_ok) and np.array_equal(d_ov.download(), votes), f"{man}: the opening lost votes"
        k = min(nb, 3)
        sn_h, cn_h = C2.derive_nonces2_host(group.q, man, bn[:k], fmt=group.hash_format)
        assert np.array_equal(d_sn[0:k].download(), sn_h) and np.array_equal(d_cn[0:k].download(), cn_h)
        B_h = C2.ballot_hashes2_host(group.q, man, hashes, ids[:k], d_cts[0:k].download(), fmt=group.hash_format)[0]
        assert np.array_equal(d_B[0:k].download(), B_h)
        keep.append((man, spc, [d_bn, d_ids, d_votes, d_desc, d_sn, d_cn, d_cts, d_sp, d_cp, d_B, d_ov, d_ok, d_oks,
                                d_okc, d_tal]))
        arms.update({tag + "_nonces": (nonces, a.inner), tag + "_hashes": (hash_ballots, a.inner),
                     tag + "_open": (open_ballots, 1), tag + "_verify": (verify, 1)})

    times = {name: [] for name in arms}
    for rep in range(a.reps):
        for name, (fn, inner) in arms.items():
            group.sync()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            group.sync()
            dt = (time.perf_counter() - t0) / inner
            times[name].append(dt)
            print(f"rep {rep} {name:10s} {dt * 1e3:9.3f} ms per call  {nb / dt:12.0f} ballots/s", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_codes2", "ballots": nb, "reps": a.reps, "inner": a.inner, "fb_window": a.fb_window,
        "shapes": {"L1": "4x(5,1,1)", "L3": "4x(5,3,3)"},
        "chunk_ballots": {"L1": B2.chunk_ballots(keep[0][0]), "L3": B2.chunk_ballots(keep[1][0])},
        "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
        "ballots_per_s": {k: round(nb / v, 1) for k, v in med.items()},
        "ratio_to_verify": {k: round(med[k] / med[k[:2] + "_verify"], 5) for k in med if not k.endswith("verify")},
    }
    print(json.dumps(out), flush=True)
    if a.ab_tree:
        for _, _, bufs in keep:
            for x in bufs:
                x.free()
        group.close()   # the flagship runs get the device to themselves
        print(json.dumps(flagship_ab(a)), flush=True)


if __name__ == "__main__":
    main()
