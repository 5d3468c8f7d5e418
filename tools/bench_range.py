#!/usr/bin/env python3
"""What does a 0..L range proof cost beside the selection proofs of the fused verifier?

One process, one context, device-resident items.  Arms interleaved over the repetitions, each timed
by a host clock around calls that end in a stream synchronise:

  verify L   eg_range_verify_dev at L = 1, 3, 7            --items proofs (default 40,000)
  prove L    eg_range_prove_dev  at L = 1, 3, 7            the same items
  ballots    eg_verify_ballots_dev, 10,000 ballots of 4 x (5+1): unchanged code, the yardstick
             (240,000 selection proofs and 40,000 contest proofs per call)

Before timing every proof is verified once, and the k_pow multiplies per item are read from the
context's profile (eg_ctx_profile_end) at L = 1, 2, 3, 7, 15.  Prints one line per timing and one
JSON summary line: medians, min-max spreads, time per item, the yardstick's time per selection.

    python tools/bench_range.py [--items 40000] [--ballots 10000] [--reps 5] [--fb-window 12]
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

LIMITS = (1, 3, 7)
MM_LIMITS = (1, 2, 3, 7, 15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=40000)
    ap.add_argument("--ballots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fb-window", type=int, default=12)
    a = ap.parse_args()

    from electionguard import range_proof as RP
    from electionguard.ballot import (ElectionKey, Manifest, Verifier, batch_encryption_device, random_scalars,
                                      random_votes)
    from electionguard.core import productionGroup
    from electionguard.core.group import FixedBase
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, n, nb, man = 0xBEEF, a.items, a.ballots, Manifest(4, 5, 1)
    rng = np.random.default_rng(11)

    def items(L, count):
        """count device-resident items at limit L: cts, values, R, nonces"""
        values = (np.arange(count) % (L + 1)).astype(np.uint8)
        R = random_scalars(rng, (count,), group.q)
        m32 = np.zeros((count, 32), np.uint8)
        m32[:, 31] = values
        kt = FixedBase(group, K, a.fb_window)
        beta = group.multP_batch(kt.pow_batch(R), group.gPowP_batch(m32))
        kt.close()
        cts = np.ascontiguousarray(np.stack([group.gPowP_batch(R), beta], axis=1))
        return (group.to_device(cts), group.to_device(values), group.to_device(R),
                group.to_device(random_scalars(rng, (count, 2 * L + 3), group.q)))

    # multiplies per item from the profile, on a small batch of every limit
    mm = {}
    for L in MM_LIMITS:
        k = 2048
        d_cts, d_val, d_R, d_non = items(L, k)
        d_pr = RP.prove(group, key, qbar, L, d_cts, d_val, d_R, d_non)   # warm: tables, op programs
        group.sync()
        group.profile_begin()
        RP.prove(group, key, qbar, L, d_cts, d_val, d_R, d_non)
        pp = group.profile_end()
        group.profile_begin()
        d_ok = RP.verify(group, key, qbar, L, d_cts, d_pr)
        pv = group.profile_end()
        assert group.all_nonzero(d_ok), f"the bench's own proofs do not verify at L = {L}"
        mm[L] = {"verify_mm_per_item": round(pv.mont_ops / k, 1), "verify_sqr_per_item": round(pv.squarings / k, 1),
                 "verify_launches": pv.launches, "prove_mm_per_item": round(pp.mont_ops / k, 1),
                 "prove_launches": pp.launches}
        print(f"L {L:2d} multiplies per item: verify {mm[L]['verify_mm_per_item']:8.1f} "
              f"({mm[L]['verify_sqr_per_item']:.1f} squarings, {pv.launches} k_pow launches)  "
              f"prove {mm[L]['prove_mm_per_item']:8.1f} ({pp.launches} launches)", flush=True)
        for d in (d_cts, d_val, d_R, d_non, d_pr, d_ok):
            d.free()

    arms = {}
    keep = []
    for L in LIMITS:
        d_cts, d_val, d_R, d_non = items(L, n)
        d_pr = RP.prove(group, key, qbar, L, d_cts, d_val, d_R, d_non)
        d_ok = RP.verify(group, key, qbar, L, d_cts, d_pr)
        assert group.all_nonzero(d_ok), f"the bench's own proofs do not verify at L = {L}"
        keep.append((d_cts, d_val, d_R, d_non, d_pr, d_ok))
        lib, h = group._lib, group.handle
        from electionguard.core import native
        Kb, qb = native.buf(key.K_be), native.buf(qbar.to_bytes(32, "big"))

        def verify(L=L, b=keep[-1]):
            native.check(lib, "eg_range_verify_dev", lib.eg_range_verify_dev(h, Kb, qb, n, L, b[0].ptr, b[4].ptr, b[5].ptr))

        def prove(L=L, b=keep[-1]):
            native.check(lib, "eg_range_prove_dev",
                         lib.eg_range_prove_dev(h, Kb, qb, n, L, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr))

        arms[f"verify_L{L}"] = (verify, n)
        arms[f"prove_L{L}"] = (prove, n)

    # the yardstick: the fused verifier on ballots made by the device encryptor
    nsel, nc = man.nsel, man.n_contests
    d_votes = group.to_device(random_votes(rng, man, nb))
    d_sn = group.to_device(random_scalars(rng, (nb, nsel, 4), group.q))
    d_cn = group.to_device(random_scalars(rng, (nb, nc), group.q))
    d_bc, d_rp, d_cp = group.device_empty((nb, nsel, 2, 512)), group.device_empty((nb, nsel, 4, 32)), \
        group.device_empty((nb, nc, 2, 32))
    batch_encryption_device(group, key, qbar, man, nb, d_votes.ptr, d_sn.ptr, d_cn.ptr, d_bc.ptr, d_rp.ptr, d_cp.ptr)
    d_oks, d_okc = group.device_empty((nb, nsel)), group.device_empty((nb, nc))
    V = Verifier(group, key, qbar, man)

    def ballots():
        V.verify_device(d_bc.ptr, d_rp.ptr, d_cp.ptr, nb, d_oks.ptr, d_okc.ptr, None)

    ballots()
    group.sync()
    assert group.all_nonzero(d_oks) and group.all_nonzero(d_okc), "the yardstick's ballots do not verify"
    arms["ballots"] = (ballots, nb * nsel)

    times = {name: [] for name in arms}
    for rep in range(a.reps):
        for name, (fn, count) in arms.items():
            group.sync()
            t0 = time.perf_counter()
            fn()
            group.sync()
            dt = time.perf_counter() - t0
            times[name].append(dt)
            print(f"rep {rep} {name:10s} {dt * 1e3:9.3f} ms per call  {dt / count * 1e6:9.4f} us per "
                  f"{'selection' if name == 'ballots' else 'item'}", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    per = lambda name, t: round(t / arms[name][1] * 1e6, 5)
    out = {
        "tool": "bench_range", "items": n, "ballots": nb, "shape": "4x(5+1)", "reps": a.reps, "fb_window": a.fb_window,
        "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
        "us_per_item": {k: per(k, v) for k, v in med.items()},
        "us_per_item_min_max": {k: [per(k, min(v)), per(k, max(v))] for k, v in times.items()},
        "verify_L1_over_yardstick_per_selection": round(per("verify_L1", med["verify_L1"]) /
                                                        per("ballots", med["ballots"]), 4),
        "k_pow_multiplies": {str(L): v for L, v in mm.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
