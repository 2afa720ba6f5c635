"""gb_bsw_global rate probe: pairs/s and band cells/s of the banded global alignment with CIGAR on a
gen.bsw_pairs set (h0 ignored, w = global_band(len2, len1, w_cap=100)), the fill / walk kernel split,
the scores-only rate, and bwa's own ksw_global2 (oracle/_ref/libref_bwa.so, when built) called per
pair from 16 threads on a sample of the same pairs, checked bit for bit against the GPU results.

    python tools/bsw_global_probe.py [--pairs 1000000] [--steps 20] [--cpu-sample 100000] [--out file.json]

Times: `call` is a host clock around the synchronous gb_bsw_global call (uploads, kernels, copies
back, CIGAR packing); `fill` / `walk` are hip-event times of the two kernels summed over the call's
chunks. Warm-up runs until 150 ms have passed (at least two calls). Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from genomicsbench_palisade_amd import bsw, gen, set_device  # noqa: E402


def band_cells(ql, tl, w):
    """DP cells ksw_global2 evaluates: sum over rows of min(i+w+1, qlen) - max(i-w, 0)."""
    total = np.zeros(len(ql), np.int64)
    ql, tl, w = ql.astype(np.int64), tl.astype(np.int64), w.astype(np.int64)
    for i in range(int(tl.max())):
        total += np.where(i < tl, np.minimum(i + w + 1, ql) - np.maximum(i - w, 0), 0)
    return total


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed(pairs, w, params, steps, want_cigar):
    t0 = time.perf_counter()
    n = 0
    while n < 2 or time.perf_counter() - t0 < 0.15:  # warm-up
        out = bsw.global_align(pairs, w, params, want_cigar=want_cigar)
        n += 1
    call, fill, walk = [], [], []
    for _ in range(steps):
        t = time.perf_counter()
        out = bsw.global_align(pairs, w, params, want_cigar=want_cigar)
        call.append((time.perf_counter() - t) * 1e3)
        f, k = bsw.global_timing()
        fill.append(f)
        walk.append(k)
    return out, call, fill, walk


def cpu_reference(pairs, w, params, sample, threads=16):
    import make_bsw_global_golden as mk
    ref = mk.ref_lib()
    if ref is None:
        return None
    idx = np.arange(min(sample, pairs.n))
    pen = (params.o_del, params.e_del, params.o_ins, params.e_ins)
    mat = np.ascontiguousarray(params.mat_array())
    seqs = [(np.ascontiguousarray(pairs.qry[pairs.qoff[p]:pairs.qoff[p] + pairs.qlen[p]]),
             np.ascontiguousarray(pairs.tgt[pairs.toff[p]:pairs.toff[p] + pairs.tlen[p]])) for p in idx.tolist()]

    def work(lo, hi):
        return [mk.ksw_global2_one(ref, seqs[p][0], seqs[p][1], w[p], pen, mat) for p in range(lo, hi)]
    cuts = np.linspace(0, len(idx), threads + 1).astype(int)
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: work(cuts[k], cuts[k + 1]), range(threads)))
    dt = time.perf_counter() - t
    res = [r for part in parts for r in part]
    nm = [mk.nm_from_cigar(o, *seqs[p]) for p, (_, o) in enumerate(res)]
    return dt, res, nm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cpu-sample", type=int, default=100_000)
    ap.add_argument("--out")
    a = ap.parse_args()
    set_device(0)
    params = bsw.default_params()
    pairs = gen.bsw_pairs(a.pairs, seed=11)
    w = bsw.global_band(pairs.qlen, pairs.tlen, 100, params)
    cells = int(band_cells(pairs.qlen, pairs.tlen, w).sum())
    out, call, fill, walk = timed(pairs, w, params, a.steps, True)
    _, call0, fill0, _ = timed(pairs, w, params, a.steps, False)
    score, ncig, nm, off, cig = out
    med = statistics.median(call)
    r = {"pairs": pairs.n, "band_cells": cells, "cigar_ops": int(len(cig)), "steps": a.steps,
         "call_ms": spread(call), "fill_ms": spread(fill), "walk_ms": spread(walk),
         "pairs_per_s": pairs.n / med * 1e3, "band_cells_per_s": cells / med * 1e3,
         "kernel_pairs_per_s": pairs.n / (statistics.median(fill) + statistics.median(walk)) * 1e3,
         "kernel_band_cells_per_s": cells / (statistics.median(fill) + statistics.median(walk)) * 1e3,
         "scores_only_call_ms": spread(call0), "scores_only_fill_ms": spread(fill0),
         "scores_only_pairs_per_s": pairs.n / statistics.median(call0) * 1e3}
    cpu = cpu_reference(pairs, w, params, a.cpu_sample)
    if cpu is None:
        r["cpu_ksw_global2"] = "not measured (oracle/_ref not built)"
    else:
        dt, res, cnm = cpu
        bad = sum(1 for p, (s, o) in enumerate(res)
                  if s != score[p] or cnm[p] != nm[p] or len(o) != ncig[p] or (o != cig[off[p]:off[p] + ncig[p]]).any())
        r["cpu_ksw_global2"] = {"pairs": len(res), "threads": 16, "seconds": dt, "pairs_per_s": len(res) / dt,
                                "pairs_differing_from_gpu": bad}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if cpu is not None and r["cpu_ksw_global2"]["pairs_differing_from_gpu"]:
        sys.exit("GPU results differ from ksw_global2")


if __name__ == "__main__":
    main()
