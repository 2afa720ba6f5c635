#!/usr/bin/env python3
"""CPU replay of phmm_predict's inner loop: how much of it the decision `best > thr` needs.

The kernel sweeps, per testcase, every 64-diagonal chunk of -63 .. C - R + 63 over all of the read's rows,
kPredChunks = 4 chunks (a group) sharing the read's ballots. Every term of a diagonal's cost is
non-negative, so a chunk whose every diagonal is above `thr` after some rows can be left, and a group that
ends with a diagonal at or below `thr` decides "not predicted". This script counts inner-loop units (32
rows x 64 diagonals of one chunk, as the kernel's unrolled body takes them) for several forms of leaving
early, with the integer costs of tests/phmm_predict_ref.py, on a sample of the bench job
(gen.phmm_dataset('large', 64, seed=1)). numpy only.

    python tools/phmm_predict_early_estimate.py [--per-batch 48] [--batches 64]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import phmm_predict_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402

CHUNKS = 4  # kPredChunks


def diagonal_partials(rs, q, hap):
    """costs[k, j]: the mismatch cost of diagonal j - 63 over rows 0 .. min(R, 64 (k + 1)) - 1; and the two
    overhangs per diagonal."""
    R, C = len(rs), len(hap)
    rc = ref.CODE[np.frombuffer(rs, np.uint8)]
    hc = ref.CODE[np.frombuffer(hap, np.uint8)]
    qq = np.frombuffer(q, np.uint8) & 127
    w = np.where(qq < ref.Q_CLASS[0], ref.W_CLASS[0], np.where(qq < ref.Q_CLASS[1], ref.W_CLASS[1], ref.W_CLASS[2]))
    d = np.arange(-ref.DIAG_PAD, C - R + ref.DIAG_PAD + 1)
    width = C + 2 * ref.DIAG_PAD
    P = np.zeros((R, width), np.int32)
    mis = (rc[:, None] != hc[None, :]) & (rc[:, None] != 4) & (hc[None, :] != 4)
    P[:, ref.DIAG_PAD:ref.DIAG_PAD + C] = mis * w.astype(np.int32)[:, None]
    s = P.itemsize
    D = np.lib.stride_tricks.as_strided(P, (R, len(d)), ((width + 1) * s, s))
    cum = np.cumsum(D, axis=0, dtype=np.int64)
    ends = [min(R, r64 + 64) - 1 for r64 in range(0, R, 64)]
    n_lo = np.minimum(R, np.maximum(0, -d))
    n_hi = np.minimum(R - n_lo, np.maximum(0, R + d - C))
    return cum[ends], ref.overhang(n_lo), ref.overhang(n_hi)


def replay(rs, q, hap, form):
    """(units, predicted) of one testcase. form: 'today', 'group' (a group's chunks leave together),
    'chunk' (per-chunk alive mask), 'chunk+lo' (the left overhang in the bound), 'chunk+lo+hi' (both)."""
    R, C = len(rs), len(hap)
    thr = ref.THRESH - ref.lc(C) + ref.MARGIN
    part, oh_lo, oh_hi = diagonal_partials(rs, q, hap)
    nd = part.shape[1]
    nchunk = (nd + 63) // 64
    niter = part.shape[0]
    halves = [2 if r64 + 32 < R else 1 for r64 in range(0, R, 64)]
    final = part[-1] + oh_lo + oh_hi
    known = np.zeros(nd, np.int64)
    if form in ("chunk+lo", "chunk+lo+hi"):
        known = known + oh_lo
    if form == "chunk+lo+hi":
        known = known + oh_hi
    units = 0
    decided = False
    for g in range(0, nchunk, CHUNKS):
        chunks = list(range(g, min(g + CHUNKS, nchunk)))
        alive = set(chunks)
        for it in range(niter):
            if not alive:
                break
            units += halves[it] * len(alive)
            if form == "today" or it == niter - 1:
                continue
            low = {c for c in alive if (part[it, 64 * c:64 * c + 64] + known[64 * c:64 * c + 64] <= thr).any()}
            alive = low if form != "group" else (alive if low else set())
        if form != "today" and any((final[64 * c:64 * c + 64] <= thr).any() for c in alive):
            decided = True
            break
    pred = bool(final.min() > thr)
    assert form == "today" or pred == (not decided)
    return units, pred


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--per-batch", type=int, default=48, help="testcases drawn from each batch")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    cases = []
    for b in gen.phmm_dataset("large", a.batches, seed=1):
        n = b.num_testcases
        for k in rng.choice(n, min(n, a.per_batch), replace=False):
            r, h = b.reads[int(k) // len(b.haps)], b.haps[int(k) % len(b.haps)]
            cases.append((r[0], r[1], h))
    forms = ("today", "group", "chunk", "chunk+lo", "chunk+lo+hi")
    total = dict.fromkeys(forms, 0)
    npred = 0
    for rs, q, hap in cases:
        assert ref.predicted(rs, q, hap) == replay(rs, q, hap, "today")[1]
        for f in forms:
            u, p = replay(rs, q, hap, f)
            total[f] += u
        npred += p
    print(f"{len(cases)} testcases of gen.phmm_dataset('large', {a.batches}, seed=1), {npred} predicted")
    print("form           inner-loop units   relative")
    for f in forms:
        print(f"{f:14s} {total[f]:16d}   {total[f] / total['today']:.3f}")


if __name__ == "__main__":
    main()
