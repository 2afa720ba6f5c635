#!/usr/bin/env python3
"""poa probe: gb_poa_consensus on a seeded benchmark-like set: windows of 20..105 reads of a 500..857-base template
at ~12 % error (substitutions, insertions and deletions in equal parts), the benchmark's parameters (convex);
against the live SISD spoa on the first windows of the same set.

The set is generated window after window from one seed, so a prefix of the count is a prefix of the set.

  --live   on the build host (needs the reference tree and g++): times the reference's spoa (SISD engine, g++ -O2,
           compiled as tests/golden/make_poa_golden.py compiles it) on one thread over the first --live-windows
           windows, align + add_alignment + generate_consensus, and stores the time and the cells beside the seed in
           profiles/poa_probe_live.json. The GPU machine has no reference tree, so this part is run beforehand.
  default  on the GPU: one warm-up call, then --reps calls; medians with minimum and maximum of the fill kernels'
           time, the walk kernels', the host's graph updates and of the whole synchronous call, cells per second in
           the kernels and over the call, the chunk count; with the live file present, the ratio to the reference's
           one-thread rate times 16, which is a projection and not a run on 16 threads. Writes --out. The stored
           run had GB_POA_WS=68719476736 (64 GiB), so that a round of 256 windows is one chunk; under the default
           4 GiB the rounds are cut into chunks that run one after the other.
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

SEED, WINDOWS = 20261021, 256
LIVE_JSON = os.path.join(ROOT, "profiles", "poa_probe_live.json")
SET = "windows of 20..105 reads of a 500..857-base template at 12 % error, m=2 n=-4 g=-6 e=-2 q=-25 c=-1 (convex)"
BENCH = (2, -4, -6, -2, -25, -1)


def make_set(n):
    rng = np.random.default_rng(SEED)
    return gen.poa_windows(rng, n, reads=(20, 105), length=(500, 857), err=0.12)


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_poa_golden as mk
    windows = make_set(args.live_windows)
    live = mk.LivePoa(args.reference or mk.REF_TREE)
    try:
        per_rep, cells = [], 0
        for _ in range(3):
            t = time.perf_counter()
            cells = sum(live.window(BENCH, reads)[3] for reads in windows)
            per_rep.append(time.perf_counter() - t)
    finally:
        live.close()
    out = {"seed": SEED, "set": SET, "live_windows": args.live_windows, "live_reads": sum(map(len, windows)),
           "live_cells": cells, "threads": 1, "seconds": spread(per_rep),
           "note": "spoa of tools/racon/vendor/spoa (SISD engine, no -msse4.1, no -mavx2), g++ -O2, called read after "
                   "read through ctypes on the build host's CPU: align, add_alignment, and generate_consensus per window"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import poa
    t = time.perf_counter()
    windows = make_set(args.windows)
    gen_s = time.perf_counter() - t
    p = poa.params(*BENCH)
    win_off, seq_off, data, _ = poa.pack_windows(windows)
    fill, walk, host, call, cells, done = [], [], [], [], None, 0
    for rep in range(args.reps + 1):  # the first call is the warm-up: buffers, code object, clocks
        t = time.perf_counter()
        st, cons, off, used, nodes, done = poa.consensus_raw(p, win_off, seq_off, data)
        dt = time.perf_counter() - t
        assert st == 0, st
        f, w, h, c = poa.timing()
        assert cells in (None, c)
        cells = c
        if rep:
            fill.append(f), walk.append(w), host.append(h), call.append(dt * 1e3)
    chunks, ws_bytes = poa.plan()
    kern = np.median(fill) + np.median(walk)
    out = {"seed": SEED, "set": SET, "windows": args.windows, "reads": int(len(seq_off) - 1), "bases": int(len(data)),
           "alignments": int(done), "cells": int(cells), "largest_graph_nodes": int(nodes.max()),
           "consensus_bytes": int(used), "chunks": chunks, "largest_chunk_workspace_bytes": ws_bytes,
           "workspace_budget": os.environ.get("GB_POA_WS", "default (4 GiB)"), "generate_s": gen_s, "reps": args.reps,
           "warmup_calls": 1, "fill_ms": spread(fill), "walk_ms": spread(walk), "host_ms": spread(host),
           "call_ms": spread(call), "host_share_of_call": float(np.median(host) / np.median(call)),
           "gcells_per_s_kernels": cells / (kern * 1e-3) / 1e9, "gcells_per_s_call": cells / (np.median(call) * 1e-3) / 1e9,
           "note": "cells are nodes x bases summed over the alignments; fill_ms and walk_ms are event-timed spans summed "
                   "over rounds and chunks (a round's fill is one launch per size class over all windows, so it lasts "
                   "as long as its largest window); host_ms is the graph updates, topological sorts, re-flattened "
                   "views and the consensus on GB_POA_THREADS threads; the call also holds the copies in and out. "
                   "Not measured: hardware counters, the size classes apart."}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        per_cell = lv["seconds"]["median"] / lv["live_cells"]
        ref16 = per_cell * cells / 16
        out["reference"] = {"live_windows": lv["live_windows"], "live_cells": lv["live_cells"],
                            "one_thread_s_per_cell": per_cell, "one_thread_gcells_per_s": 1e-9 / per_cell,
                            "projected_16_thread_gcells_per_s": 16e-9 / per_cell,
                            "projected_set_seconds_on_16_threads": ref16,
                            "how": "a projection: one-thread time of the first %d windows on the build host, per cell, "
                                   "times this set's cells, divided by 16" % lv["live_windows"],
                            "speedup_kernels": ref16 / (kern * 1e-3), "speedup_call": ref16 / (np.median(call) * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--reference", default=None, help="the reference tree (default: the recorder's)")
    ap.add_argument("--live-windows", type=int, default=2)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poa_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
