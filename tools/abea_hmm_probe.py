#!/usr/bin/env python3
"""abea HMM probe: gb_abea_hmm_score on a seeded set of about 2 M items shaped like real site groups (16..40
k-mers, 1.2..2.5 events per k-mer, each read scored as it is and methylated), against f5c's CPU
profile_hmm_score on the first items of the same set.

The set is generated in pieces of --piece-reads reads of one shape each (two items per read); the generator
draws piece after piece, so a prefix of the pieces is a prefix of the set.

  --live   on the build host (needs the reference tree and g++): times the live profile_hmm_score on one thread
           over the first --live-pieces pieces and stores the times beside the set's seed in
           profiles/abea_hmm_probe_live.json. The GPU machine has no reference tree, so this part is run
           beforehand.
  default  on the GPU: one warm-up call, then --reps calls; medians with minimum and maximum of the kernels'
           time and of the whole synchronous call, cells per second; with the live file present, the ratio to the
           reference's one-thread rate times 16, which is a projection and not a run on 16 threads. Writes --out.
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

SEED, PIECES, PIECE_READS = 20261021, 500, 2000
LIVE_JSON = os.path.join(ROOT, "profiles", "abea_hmm_probe_live.json")
SET = "reads of 16..40 k-mers with 1.2..2.5 events per k-mer, two items each (as it is and methylated), flags 3"


def make_set(pieces, piece_reads):
    rng = np.random.default_rng(SEED)
    model = gen.abea_cpg_model(rng)
    parts = []
    for _ in range(pieces):
        nk = int(rng.integers(16, 41))
        rows = int(nk * rng.uniform(1.2, 2.5))
        parts.append(gen.abea_hmm_items(rng, [(piece_reads, nk, rows)], model=model))
    return gen.AbeaHmmItems.concat(parts)


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_abea_hmm_golden as mk
    x = make_set(args.live_pieces, args.piece_reads)
    live = mk.LiveHmm(args.reference)
    try:
        per_rep = []
        for _ in range(3):
            t = time.perf_counter()
            live.scores(x)
            per_rep.append(time.perf_counter() - t)
    finally:
        live.close()
    out = {"seed": SEED, "set": SET, "live_items": x.n, "live_cells": x.cells(), "threads": 1, "seconds": spread(per_rep),
           "note": "profile_hmm_score of benchmarks/abea/src/hmm.c, g++ -O2 -ffp-contract=off, called item after item "
                   "through ctypes on the build host's CPU; includes the shim's copy of the read's events"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import abea
    t = time.perf_counter()
    x = make_set(args.pieces, args.piece_reads)
    gen_s = time.perf_counter() - t
    cells = x.cells()
    kern, call, scores = [], [], None
    for rep in range(args.reps + 1):  # the first call is the warm-up: buffers, code object, clocks
        t = time.perf_counter()
        scores = abea.hmm_score(x)
        dt = time.perf_counter() - t
        ms, c = abea.hmm_timing()
        assert c == cells
        if rep:
            kern.append(ms), call.append(dt * 1e3)
    out = {"seed": SEED, "set": SET, "items": x.n, "reads": len(x.reads), "cells": cells, "events": len(x.events),
           "finite_scores": int(np.isfinite(scores).sum()), "generate_s": gen_s, "reps": args.reps, "warmup_calls": 1,
           "kernel_ms": spread(kern), "call_ms": spread(call), "cells_per_s_kernel": cells / (np.median(kern) * 1e-3),
           "note": "kernel_ms is the event-timed span of the launches (one per size class); the call includes the "
                   "checks, the sort by size class and rows, and the copies in and out"}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        per_cell = lv["seconds"]["median"] / lv["live_cells"]
        ref16 = per_cell * cells / 16
        out["reference"] = {"one_thread_s_per_cell": per_cell, "projected_set_seconds_on_16_threads": ref16,
                            "how": "a projection: one-thread time of the first %d items, per cell, times this set's "
                                   "cells, divided by 16" % lv["live_items"],
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
    ap.add_argument("--live-pieces", type=int, default=1)
    ap.add_argument("--pieces", type=int, default=PIECES)
    ap.add_argument("--piece-reads", type=int, default=PIECE_READS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abea_hmm_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
