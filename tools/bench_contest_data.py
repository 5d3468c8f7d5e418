#!/usr/bin/env python3
"""What does sealing and opening contest data cost beside encrypting the ballots?

One process, one context, device-resident buffers, bench.py's configs[1] shape (10,000 ballots of
4 x (5+1), so 40,000 contest-data items).  Arms on the same buffers, interleaved over the
repetitions, each timed by a host clock around calls that end in a stream synchronise:

  nonces   eg_derive_contest_data_nonces_dev   r of every (ballot, contest)
  seal     eg_seal_contest_data_dev            c0 = g^r, kappa = K^r, the stream and the MAC
  open     eg_open_contest_data_dev            the MAC check and the stream, kappa given
  encrypt  eg_encrypt_ballots_dev              ciphertexts and proofs: unchanged code, the yardstick

Before timing, the first items of the seal are checked against the host mirror and every item is
opened again.  Prints one line per timing and one JSON summary line (medians, min-max spreads,
the ratios to the encrypt median).

    python tools/bench_contest_data.py [--ballots 10000] [--nbytes 64] [--reps 7] [--fb-window 12]
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
    ap.add_argument("--nbytes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5, help="calls per timing of the three contest-data arms")
    ap.add_argument("--fb-window", type=int, default=12)
    a = ap.parse_args()

    from electionguard import codes as C
    from electionguard import contest_data as CD
    from electionguard.ballot import ElectionKey, Manifest, batch_encryption_device, random_votes
    from electionguard.core import native, productionGroup
    from electionguard.core.group import FixedBase
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    lib, h = group._lib, group.handle
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, nb, man, nbytes = 0xBEEF, a.ballots, Manifest(4, 5, 1), a.nbytes
    nsel, nc = man.nsel, man.n_contests
    n = nb * nc
    rng = np.random.default_rng(9)
    r = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    bn, ids, data = r(nb, 32), r(nb, 32), r(n, nbytes)
    d_bn, d_ids, d_data = group.to_device(bn), group.to_device(ids), group.to_device(data)
    d_r, d_c0, d_kappa = group.device_empty((n, 32)), group.device_empty((n, 512)), group.device_empty((n, 512))
    d_c1, d_c2 = group.device_empty((n, nbytes)), group.device_empty((n, 32))
    d_out, d_ok = group.device_empty((n, nbytes)), group.device_buffer(n)
    # the yardstick's buffers
    d_sn, d_cn = C.derive_nonces(group, man, d_bn)
    d_votes = group.to_device(random_votes(rng, man, nb))
    d_cts, d_rp, d_cp = group.device_empty((nb, nsel, 2, 512)), group.device_empty((nb, nsel, 4, 32)), \
        group.device_empty((nb, nc, 2, 32))
    Kb = native.buf(key.K_be)

    def nonces():
        native.check(lib, "eg_derive_contest_data_nonces_dev",
                     lib.eg_derive_contest_data_nonces_dev(h, nb, nc, d_bn.ptr, d_r.ptr))

    def seal():
        native.check(lib, "eg_seal_contest_data_dev",
                     lib.eg_seal_contest_data_dev(h, Kb, nb, nc, nbytes, d_ids.ptr, d_r.ptr, d_data.ptr, d_c0.ptr,
                                                  d_c1.ptr, d_c2.ptr))

    def open_():
        native.check(lib, "eg_open_contest_data_dev",
                     lib.eg_open_contest_data_dev(h, nb, nc, nbytes, d_ids.ptr, d_c0.ptr, d_kappa.ptr, d_c1.ptr,
                                                  d_c2.ptr, d_out.ptr, d_ok.ptr))

    def encrypt():
        batch_encryption_device(group, key, qbar, man, nb, d_votes.ptr, d_sn.ptr, d_cn.ptr, d_cts.ptr, d_rp.ptr,
                                d_cp.ptr)

    # warm-up of every arm (tables, workspaces, op programs) and a check of what is timed
    nonces()
    seal()
    ktab = FixedBase(group, key.K, key.window_bits)
    ktab.pow_batch_dev(d_r.ptr, d_kappa.ptr, n)
    open_()
    encrypt()
    group.sync()
    ktab.close()
    assert group.all_nonzero(d_ok), "the bench's own items do not open"
    assert np.array_equal(d_out.download(), data)
    k = min(nb, 2) * nc
    r_h = CD.derive_nonces_host(group.q, nc, bn[:k // nc], fmt=group.hash_format).reshape(-1, 32)
    assert np.array_equal(d_r[0:k].download(), r_h)
    c1_h, c2_h = CD.seal_host(nc, ids[:k // nc], d_c0[0:k].download(), d_kappa[0:k].download(), data[:k])
    assert np.array_equal(d_c1[0:k].download(), c1_h) and np.array_equal(d_c2[0:k].download(), c2_h)

    arms = {"nonces": (nonces, a.inner), "seal": (seal, a.inner), "open": (open_, a.inner), "encrypt": (encrypt, 1)}
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
        "tool": "bench_contest_data", "ballots": nb, "items": n, "nbytes": nbytes, "shape": "4x(5+1)",
        "reps": a.reps, "inner": a.inner, "fb_window": a.fb_window,
        "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
        "ratio_to_encrypt": {k: round(med[k] / med["encrypt"], 5) for k in ("nonces", "seal", "open")},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
