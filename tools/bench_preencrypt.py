#!/usr/bin/env python3
"""What does pre-encrypting, recording and checking a ballot cost beside encrypting one?

One process, one context, device-resident ballots of 4 x (5+1) (V = 144 component ciphertexts,
S = 24 chosen ones per recorded ballot).  Arms interleaved over the repetitions, each timed by a
host clock around calls that end in a stream synchronise:

  pre        eg_preencrypt_ballots_dev, hashes / order / codes only (ciphertexts in workspace)
  pre_cts    the same with the vec_cts output
  record     eg_preencrypt_record_dev
  verify     eg_preencrypt_verify_dev
  encrypt    eg_encrypt_ballots_dev on the same number of ballots: unchanged code, the yardstick

Before timing every recorded ballot passes the pre-encryption check, and one profiled call of
`pre` gives the k_pow share of its time (the rest is hashing, export and sorting).  Prints one
line per timing and one JSON summary line: medians, min-max spreads, time per ballot and the
ratio of each arm to the yardstick.

    python tools/bench_preencrypt.py [--ballots 4000] [--reps 5] [--fb-window 12]
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
    ap.add_argument("--ballots", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fb-window", type=int, default=12)
    a = ap.parse_args()

    from electionguard import preencrypt as PE
    from electionguard.ballot import ElectionKey, Manifest, batch_encryption_device, random_scalars, random_votes
    from electionguard.codes import ManifestHashes
    from electionguard.core import native, productionGroup
    from electionguard.keyceremony import key_ceremony

    group = productionGroup(0)
    _, K = key_ceremony(group, 3, 3, seed=1)
    key = ElectionKey(group, K, window_bits=a.fb_window)
    qbar, nb, man = 0xBEEF, a.ballots, Manifest(4, 5, 1)
    sh = PE.pre_shape(man)
    nsel, nc = sh.nsel, sh.nc
    rng = np.random.default_rng(14)
    hashes = ManifestHashes(rng.integers(0, 256, (nsel, 32), dtype=np.uint8),
                            rng.integers(0, 256, (nc, 32), dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8))
    d_ids = group.to_device(rng.integers(0, 256, (nb, 32), dtype=np.uint8))
    d_bn = group.to_device(random_scalars(rng, (nb,), group.q))
    d_votes = group.to_device(random_votes(rng, man, nb))

    pre = PE.preencrypt_ballots(group, key, man, hashes, d_ids, d_bn, 2, with_cts=True)
    rec = PE.record_ballots(group, key, qbar, man, hashes, d_bn, d_votes, pre.sorted, 2)
    okc, okb = PE.verify_recorded(group, man, hashes, d_ids, rec.sel_vecs, rec.sel_rank, rec.sel_codes, pre.sorted,
                                  rec.ballots.cts, pre.conf, 2)
    assert group.all_nonzero(rec.ok) and group.all_nonzero(okc) and group.all_nonzero(okb), \
        "the bench's own ballots do not pass the pre-encryption check"

    lib, h = group._lib, group.handle
    Kb, qb = native.buf(key.K_be), native.buf(qbar.to_bytes(32, "big"))
    spc = np.ascontiguousarray(man.spc_list, dtype=np.uint32)
    lim = np.ascontiguousarray(man.limits, dtype=np.uint32)
    u32p = lambda x: x.ctypes.data_as(native.c_vp)
    desc = group.to_device(np.concatenate([np.ascontiguousarray(hashes.dcon).reshape(-1), hashes.manifest_hash]))
    d_dcon, d_mh = desc.ptr, desc.ptr + nc * 32

    def run_pre(vec):
        native.check(lib, "eg_preencrypt_ballots_dev",
                     lib.eg_preencrypt_ballots_dev(h, Kb, nb, nc, u32p(spc), 2, d_dcon, d_mh, d_ids.ptr, d_bn.ptr,
                                                   pre.sorted.ptr, pre.perm.ptr, pre.codes.ptr, pre.unique.ptr,
                                                   pre.conf.ptr, pre.chash.ptr, vec))

    def record():
        native.check(lib, "eg_preencrypt_record_dev",
                     lib.eg_preencrypt_record_dev(h, Kb, nb, nc, u32p(spc), u32p(lim), 2, d_dcon, d_bn.ptr, d_votes.ptr,
                                                  pre.sorted.ptr, rec.sel_vecs.ptr, rec.sel_rank.ptr,
                                                  rec.sel_codes.ptr, rec.sel_nonces.ptr, rec.contest_nonces.ptr,
                                                  rec.ok.ptr))

    def verify():
        native.check(lib, "eg_preencrypt_verify_dev",
                     lib.eg_preencrypt_verify_dev(h, nb, nc, u32p(spc), u32p(lim), 2, d_dcon, d_mh, d_ids.ptr,
                                                  rec.sel_vecs.ptr, rec.sel_rank.ptr, rec.sel_codes.ptr, pre.sorted.ptr,
                                                  rec.ballots.cts.ptr, pre.conf.ptr, okc.ptr, okb.ptr))

    eb = rec.ballots

    def encrypt():
        batch_encryption_device(group, key, qbar, man, nb, d_votes.ptr, rec.sel_nonces.ptr, rec.contest_nonces.ptr,
                                eb.cts.ptr, eb.rproof.ptr, eb.cproof.ptr)

    arms = {"pre": lambda: run_pre(None), "pre_cts": lambda: run_pre(pre.vec_cts.ptr), "record": record,
            "verify": verify, "encrypt": encrypt}

    # the k_pow share of one pre-encryption call
    group.sync()
    group.profile_begin()
    t0 = time.perf_counter()
    arms["pre"]()
    group.sync()
    wall = time.perf_counter() - t0
    prof = group.profile_end()
    share = {"k_pow_ms": round(prof.ms, 3), "call_ms": round(wall * 1e3, 3), "k_pow_share": round(prof.ms / (wall * 1e3), 4),
             "mm_per_ballot": round(prof.mont_ops / nb, 1), "launches": prof.launches}
    print(f"pre: k_pow {prof.ms:.3f} ms of {wall * 1e3:.3f} ms ({prof.mont_ops / nb:.0f} multiplies per ballot, "
          f"{prof.launches} launches); the rest is hashing, export and sorting", flush=True)

    times = {name: [] for name in arms}
    for rep in range(a.reps):
        for name, fn in arms.items():
            group.sync()
            t0 = time.perf_counter()
            fn()
            group.sync()
            dt = time.perf_counter() - t0
            times[name].append(dt)
            print(f"rep {rep} {name:8s} {dt * 1e3:9.3f} ms per call  {dt / nb * 1e6:9.3f} us per ballot", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "bench_preencrypt", "ballots": nb, "shape": "4x(5+1)", "V": sh.V, "S": sh.S, "reps": a.reps,
        "fb_window": a.fb_window, "chunk_cts": PE.CHUNK_CTS,
        "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
        "us_per_ballot": {k: round(v / nb * 1e6, 4) for k, v in med.items()},
        "ratio_to_encrypt": {k: round(v / med["encrypt"], 4) for k, v in med.items()},
        "pre_profile": share,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
