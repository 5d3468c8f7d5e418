#!/usr/bin/env python3
"""What do ballot hashes and nonce derivation cost beside verification?

One process, one context, device-resident buffers, bench.py's configs[1] shape (10,000 ballots of
4 x (5+1)).  Three arms on the same buffers, interleaved over the repetitions, each timed by a
host clock around calls that end in a stream synchronise:

  hashes   eg_ballot_hashes_dev          selection, contest and ballot hashes of every ballot
  nonces   eg_derive_ballot_nonces_dev   the 4 nsel + nc nonces of every ballot
  verify   eg_verify_ballots_dev         proofs + tally: unchanged code, the yardstick

The two hashing arms run --inner calls per timing (one call is a few milliseconds at most; the
figure reported is per call).  Before timing, the device results of the first ballots are checked
against the host mirrors.  Prints one line per timing and one JSON summary line (medians, min-max
spreads, the two ratios to the verify median).

    python tools/bench_codes.py [--ballots 10000] [--reps 7] [--inner 20] [--fb-window 12]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--fb-window", type=int, default=12)
    a = ap.parse_args()

    from electionguard import codes as C
    from electionguard.ballot import ElectionKey, Manifest, Verifier, batch_encryption_device, random_votes
    from electionguard.core import native, productionGroup
    from electionguard.core.marshal import u32p
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    lib = group._lib
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, nb, man = 0xBEEF, a.ballots, Manifest(4, 5, 1)
    nsel, nc = man.nsel, man.n_contests
    rng = np.random.default_rng(9)
    r = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    hashes = C.ManifestHashes(r(nsel, 32), r(nc, 32), r(32))
    bn, ids = r(nb, 32), r(nb, 32)
    # device-resident ballots, encrypted from nonces derived on the device
    d_bn, d_ids = group.to_device(bn), group.to_device(ids)
    d_sn, d_cn = group.device_empty((nb, nsel, 4, 32)), group.device_empty((nb, nc, 32))
    d_desc = group.to_device(np.concatenate([hashes.dsel.reshape(-1), hashes.dcon.reshape(-1), hashes.manifest_hash]))
    d_cts, d_rp, d_cp = group.device_empty((nb, nsel, 2, 512)), group.device_empty((nb, nsel, 4, 32)), \
        group.device_empty((nb, nc, 2, 32))
    d_B = group.device_empty((nb, 32))
    d_oks, d_okc, d_tal = group.device_buffer(nb * nsel), group.device_buffer(nb * nc), \
        group.device_buffer(man.n_real * 2 * 512)
    spc = u32p(man.spc_list)
    V = Verifier(group, key, qbar, man)

    def nonces():
        native.check(lib, "eg_derive_ballot_nonces_dev",
                     lib.eg_derive_ballot_nonces_dev(group.handle, nb, nc, spc, d_bn.ptr, d_sn.ptr, d_cn.ptr))

    def hash_ballots():
        native.check(lib, "eg_ballot_hashes_dev",
                     lib.eg_ballot_hashes_dev(group.handle, nb, nc, spc, d_desc.ptr, d_desc.ptr + nsel * 32,
                                              d_desc.ptr + (nsel + nc) * 32, d_ids.ptr, d_cts.ptr, d_B.ptr, None,
                                              None))

    def verify():
        V.verify_device(d_cts.ptr, d_rp.ptr, d_cp.ptr, nb, d_oks.ptr, d_okc.ptr, d_tal.ptr)

    nonces()
    d_votes = group.to_device(random_votes(rng, man, nb))
    batch_encryption_device(group, key, qbar, man, nb, d_votes.ptr, d_sn.ptr, d_cn.ptr, d_cts.ptr, d_rp.ptr, d_cp.ptr)
    # warm-up of every arm (tables, workspaces, op programs) and a check of what is timed
    hash_ballots()
    verify()
    group.sync()
    assert group.all_nonzero(d_oks) and group.all_nonzero(d_okc), "the bench's own ballots do not verify"
    k = min(nb, 3)
    sn_h, cn_h = C.derive_nonces_host(group.q, man, bn[:k], fmt=group.hash_format)
    assert np.array_equal(d_sn[0:k].download(), sn_h) and np.array_equal(d_cn[0:k].download(), cn_h)
    B_h = C.ballot_hashes_host(group.q, man, hashes, ids[:k], d_cts[0:k].download(), fmt=group.hash_format)[0]
    assert np.array_equal(d_B[0:k].download(), B_h)

    arms = {"hashes": (hash_ballots, a.inner), "nonces": (nonces, a.inner), "verify": (verify, 1)}
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
            print(f"rep {rep} {name:7s} {dt * 1e3:9.3f} ms per call  {nb / dt:12.0f} ballots/s", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_codes", "ballots": nb, "shape": "4x(5+1)", "reps": a.reps, "inner": a.inner,
        "fb_window": a.fb_window,
        "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
        "ratio_to_verify": {k: round(med[k] / med["verify"], 5) for k in ("hashes", "nonces")},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
