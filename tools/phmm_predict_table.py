#!/usr/bin/env python3
"""Recall / false-positive table of the PairHMM fallback predictor (tests/phmm_predict_ref.py) against the
oracle's f32 results, on testcases sampled evenly over the 'large' job's batches (CPU only).
    python tools/phmm_predict_table.py [--sample 20000] [--batches 64]
Per form and margin: the share of the fallback cells the predictor catches, and the cells of wrongly
predicted testcases (f32 result >= MIN_ACCEPTED) over all cells."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import phmm_predict_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402
from genomicsbench_palisade_amd._tc import TestcaseArray  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    ta = TestcaseArray.from_batches(gen.phmm_dataset("large", args.batches, seed=1))
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(ta.n, min(args.sample, ta.n), replace=False))
    sub = ta.subset(idx)
    a = sub.np_arr
    t0 = time.time()
    out, rf, rd = np.zeros(sub.n), np.zeros(sub.n, np.float32), np.zeros(sub.n)
    oracle_lib.oracle().phmm_oracle_batch(ctypes.addressof(sub.arr), sub.n, out.ctypes.data, rf.ctypes.data,
                                          rd.ctypes.data, None, args.threads)
    print(f"oracle: {sub.n} of {ta.n} testcases, {time.time() - t0:.1f} s", flush=True)
    cells = a["rslen"][:sub.n].astype(np.int64) * a["haplen"][:sub.n]
    fb = rf < np.float32(1e-28)
    print(f"fallback: {fb.mean():.3f} of testcases, {cells[fb].sum() / cells.sum():.3f} of cells")
    cost3, costx, thr = np.zeros(sub.n, np.int64), np.zeros(sub.n, np.int64), np.zeros(sub.n, np.int64)
    t0 = time.time()
    for k in range(sub.n):
        R, C = int(a["rslen"][k]), int(a["haplen"][k])
        rs = ctypes.string_at(int(a["rs"][k]), R)
        q = ctypes.string_at(int(a["q"][k]), R)
        hap = ctypes.string_at(int(a["hap"][k]), C)
        cost3[k] = ref.best_cost(rs, q, hap)
        qq = np.frombuffer(q, np.uint8).astype(np.int64) & 127
        costx[k] = ref.best_cost(rs, q, hap, weights=10 * qq + 48)
        thr[k] = ref.THRESH - ref.lc(C)
    print(f"predictor (numpy): {time.time() - t0:.1f} s", flush=True)
    print("| form | margin | fallback cells caught | false-positive cells / all cells | false-positive testcases |")
    print("|---|---|---|---|---|")
    for name, cost in (("3 classes", cost3), ("exact 10 q + 48", costx)):
        for margin in (-300, -200, -150, -100, -50, 0, 50, 100, 200, 300, 500):
            p = cost > thr + margin
            print(f"| {name} | {margin / 100:.1f} | {cells[p & fb].sum() / cells[fb].sum():.3f} | "
                  f"{cells[p & ~fb].sum() / cells.sum():.5f} | {int((p & ~fb).sum())} |")


if __name__ == "__main__":
    main()
