#!/usr/bin/env python3
"""abea probe: gb_abea_align on a seeded set of 20 000 reads (seq_len log-uniform in 500..10 000, 1.6 events per
k-mer), against f5c's CPU align() on the first reads of the same set.

  --live   on the build host (needs the reference tree and g++): times the live align() on one thread over the
           first --live-reads reads and stores the times beside the set's seed in profiles/abea_probe_live.json.
           The GPU machine has no reference tree, so this part is run beforehand.
  default  on the GPU: one warm-up call, then --reps calls; medians with minimum and maximum of the kernel's
           fill and walk times, the whole synchronous call, cells per second, workspace bytes; with the live
           file present, the ratio to the reference's one-thread rate times 16. Writes --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from genomicsbench_palisade_amd import gen  # noqa: E402

SEED, N_READS, LO, HI = 20261020, 20000, 500, 10000
LIVE_JSON = os.path.join(ROOT, "profiles", "abea_probe_live.json")


def make_set(n):
    """The first n reads of the probe set: the generator draws read after read, so a prefix is a prefix."""
    rng = np.random.default_rng(SEED)
    model = gen.abea_model(rng)
    lens = np.exp(rng.uniform(np.log(LO), np.log(HI), N_READS)).astype(np.int64)[:n]
    rs = [gen.abea_read(rng, model, int(l), 1.6, 0.7, 0.01) for l in lens]
    return gen.AbeaReads(model, np.concatenate([b for b, _ in rs]), np.concatenate([e for _, e in rs]),
                         [len(b) for b, _ in rs], [len(e) for _, e in rs], np.ones(n, np.float32), np.zeros(n, np.float32))


def bands(reads):
    return int((reads.n_events.astype(np.int64) + reads.seq_len - gen.ABEA_K + 1 + 2).sum())


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_abea_golden as mk
    reads = make_set(args.live_reads)
    live = mk.LiveAbea(args.reference)
    try:
        per_rep = []
        for _ in range(args.reps):
            t = time.perf_counter()
            for r in range(reads.n):
                b, e = reads.read(r)
                live.align(reads.model, b, e, 1.0, 0.0)
            per_rep.append(time.perf_counter() - t)
    finally:
        live.close()
    out = {"seed": SEED, "set": f"{N_READS} reads, seq_len log-uniform {LO}..{HI}, 1.6 events per k-mer",
           "live_reads": reads.n, "live_bands": bands(reads), "live_bases": int(reads.seq_len.sum()),
           "threads": 1, "seconds": spread(per_rep),
           "note": "align() of benchmarks/abea/src/align.c, g++ -O2 -ffp-contract=off, called read after read "
                   "through ctypes on the build host's CPU; includes the shim's copy of the events and the model"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import abea
    t = time.perf_counter()
    reads = make_set(args.reads)
    gen_s = time.perf_counter() - t
    nb = bands(reads)
    fill, walk, call, cells = [], [], [], 0
    for rep in range(args.reps + 1):  # the first call is the warm-up: buffers, code object, clocks
        t = time.perf_counter()
        pairs, off, st = abea.align(reads)
        dt = time.perf_counter() - t
        f, w, cells = abea.timing()
        if rep:
            fill.append(f), walk.append(w), call.append(dt * 1e3)
    chunks, waves, ws_bytes = abea.plan()
    kern = [a + b for a, b in zip(fill, walk)]
    out = {"seed": SEED, "reads": reads.n, "bands": nb, "cells": int(cells), "bases": int(reads.seq_len.sum()),
           "events": int(reads.n_events.sum()), "pairs": int(len(pairs)), "qc_passed": int((st["n_pairs"] > 0).sum()),
           "generate_s": gen_s, "reps": args.reps, "warmup_calls": 1,
           "fill_ms": spread(fill), "walk_ms": spread(walk), "kernel_ms": spread(kern), "call_ms": spread(call),
           "cells_per_s_kernel": cells / (np.median(kern) * 1e-3), "chunks": chunks, "waves": waves,
           "workspace_bytes": ws_bytes,
           "note": "fill and walk split the kernel's event-timed milliseconds by the waves' own cycle counts; the "
                   "call includes the copies in and out and the host's packing of the pairs"}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        per_band = lv["seconds"]["median"] / lv["live_bands"]
        ref16 = per_band * nb / 16
        out["reference"] = {"one_thread_s_per_band": per_band, "set_seconds_on_16_threads": ref16,
                            "how": "one-thread time of the first %d reads, per band, times this set's bands, "
                                   "divided by 16" % lv["live_reads"],
                            "speedup_kernel": ref16 / (np.median(kern) * 1e-3),
                            "speedup_call": ref16 / (np.median(call) * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--live-reads", type=int, default=300)
    ap.add_argument("--reads", type=int, default=N_READS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abea_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
