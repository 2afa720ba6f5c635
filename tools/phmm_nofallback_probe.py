#!/usr/bin/env python3
"""PairHMM step time on a job that does not fall back to f64: what the fallback predictor's gate costs
when there is nothing to predict. The job has the 'large' set's batch shapes (64 batches, reads x
haplotypes), but every haplotype of a batch is the same 473 columns with 0.5 % substitutions and every
read an exact window of the first one, so every f32 result passes MIN_ACCEPTED.
    python tools/phmm_nofallback_probe.py [--root TREE] [--steps 20] [--warmup 5]
--root: the tree whose package is timed (default: this one; an A/B run points it at another build)."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=64)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from genomicsbench_palisade_amd import gen, phmm, set_device
    from genomicsbench_palisade_amd._tc import TestcaseArray
    set_device(0)
    phmm.init_pairhmm()
    rng = np.random.default_rng(1)
    bases = np.frombuffer(b"ACGT", np.uint8)
    batches = []
    for _ in range(args.batches):
        R = max(1, int(1193 * rng.random() ** 2))
        H = max(1, int(128 * rng.random() ** 1.5))
        while R * H > 50000:
            R = max(1, R // 2)
        src = bases[rng.integers(0, 4, 473)]
        haps = []
        for _ in range(H):
            h = src.copy()
            sub = rng.random(473) < 0.005
            h[sub] = bases[rng.integers(0, 4, int(sub.sum()))]
            haps.append(h.tobytes())
        reads = []
        for _ in range(R):
            n = int(rng.integers(100, 251))
            at = int(rng.integers(0, 473 - n + 1))
            reads.append((haps[0][at:at + n], rng.integers(6, 41, n).astype(np.uint8).tobytes(),
                          rng.integers(40, 46, n).astype(np.uint8).tobytes(),
                          rng.integers(40, 46, n).astype(np.uint8).tobytes(), bytes([10]) * n))
        batches.append(gen.PhmmBatch(reads, haps))
    ta = TestcaseArray.from_batches(batches)
    job = phmm.DeviceBatch(ta)
    job.run()
    used = job.results()[3]
    for _ in range(args.warmup):
        job.run()
    job.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        job.run()
        job.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = {"testcases": ta.n, "cells": ta.cells(), "fallback_testcases": int(used.sum()),
           "step_ms_min": min(ms), "step_ms_median": float(np.median(ms)), "kernels_ms": job.timing(),
           "exit_stats": job.exit_stats()}
    if hasattr(job, "predict_stats"):
        out["predict_stats"] = job.predict_stats()._asdict()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
