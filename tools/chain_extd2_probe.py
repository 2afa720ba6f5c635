#!/usr/bin/env python3
"""chain extd2 probe: gb_chain_extd2 on a seeded map-ont-like mix of what mm_align1 asks of ksw_extd2_sse: gap fills
of 200..2000 bases (half with KSW_EZ_APPROX_MAX, the first pass, half exact) and extensions of 500..5000 bases
(left and right), queries at 10..15 % divergence (substitutions, short indels, a few long ones), w = 751,
zdrop = 400, map-ont scoring; against the live ksw_extd2_sse on the first items of the same set.

The set is generated item after item from one seed, so a prefix of the counts is a prefix of the set.

  --live   on the build host (needs the reference tree and gcc): times the live ksw_extd2_sse (gcc -O2 -msse4.1) on
           one thread over the first --live-fills fills and --live-exts extensions and stores the times beside the
           seed in profiles/chain_extd2_probe_live.json. The GPU machine has no reference tree, so this part is
           run beforehand.
  default  on the GPU: one warm-up call, then --reps calls; medians with minimum and maximum of the fill kernels'
           time, the walk and pack kernels' and of the whole synchronous call, in-band cells per second; the live
           subset is run on the device too, which gives its cells; with the live file present, the ratio to the
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

SEED, FILLS, EXTS = 20261020, 2000, 200
LIVE_JSON = os.path.join(ROOT, "profiles", "chain_extd2_probe_live.json")
SET = ("map-ont scoring, w = 751, zdrop = 400: gap fills of 200..2000 bases (flags APPROX_MAX and 0 alternating) and "
       "extensions of 500..5000 bases (EXTZ_ONLY, and EXTZ_ONLY|RIGHT|REV_CIGAR), queries at 10..15 % divergence")


def make_part(seed, n, lo, hi, flags):
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(n):
        tlen = int(rng.integers(lo, hi + 1))
        div = float(rng.uniform(0.10, 0.15))
        qlen = max(1, int(tlen * rng.uniform(0.97, 1.03)))
        parts.append(gen.extd2_items(rng, [(qlen, tlen)], w=751, zdrop=400, end_bonus=-1, flag=flags[k % len(flags)],
                                     sub=0.6 * div, indel=0.2 * div, long_indel=0.002))
    return parts


def make_set(fills, exts):
    return gen.Extd2Items.concat(make_part(SEED, fills, 200, 2000, (0x08, 0)) + make_part(SEED + 1, exts, 500, 5000, (0x40, 0xc2)))


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_chain_extd2_golden as mk
    x = make_set(args.live_fills, args.live_exts)
    live = mk.LiveExtd2(args.reference or mk.REF_TREE)
    try:
        per_rep = []
        for _ in range(3):
            t = time.perf_counter()
            for i in range(x.n):
                live.align_item(x, i)
            per_rep.append(time.perf_counter() - t)
    finally:
        live.close()
    out = {"seed": SEED, "set": SET, "live_fills": args.live_fills, "live_exts": args.live_exts, "live_items": x.n,
           "live_bases": int((x.items["qlen"] + x.items["tlen"]).sum()), "threads": 1, "seconds": spread(per_rep),
           "note": "ksw_extd2_sse of tools/minimap2/ksw2_extd2_sse.c, gcc -O2 -msse4.1, libc allocator, called item after "
                   "item through ctypes on the build host's CPU; includes the copy of the CIGAR into a numpy array"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import chain
    t = time.perf_counter()
    x = make_set(args.fills, args.exts)
    gen_s = time.perf_counter() - t
    fill, walk, call, cells, words = [], [], [], None, 0
    for rep in range(args.reps + 1):  # the first call is the warm-up: buffers, code object, clocks
        t = time.perf_counter()
        res, cig, off = chain.extd2(x)
        dt = time.perf_counter() - t
        f, w, c = chain.extd2_timing()
        assert cells in (None, c)
        cells, words = c, len(cig)
        if rep:
            fill.append(f), walk.append(w), call.append(dt * 1e3)
    chunks, ws_bytes = chain.extd2_plan()
    out = {"seed": SEED, "set": SET, "items": x.n, "fills": args.fills, "exts": args.exts,
           "bases": int((x.items["qlen"] + x.items["tlen"]).sum()), "cells": cells, "cigar_words": words,
           "zdropped": int(res["zdropped"].sum()), "chunks": chunks, "largest_chunk_workspace_bytes": ws_bytes,
           "generate_s": gen_s, "reps": args.reps, "warmup_calls": 1,
           "fill_ms": spread(fill), "walk_ms": spread(walk), "call_ms": spread(call),
           "gcells_per_s_fill": cells / (np.median(fill) * 1e-3) / 1e9,
           "gcells_per_s_fill_and_walk": cells / ((np.median(fill) + np.median(walk)) * 1e-3) / 1e9,
           "gcells_per_s_call": cells / (np.median(call) * 1e-3) / 1e9,
           "note": "cells are the in-band cells of the rows the sweeps reach; fill_ms (one launch per size class) and "
                   "walk_ms (the walk and the pack) are event-timed spans summed over the chunks; the call includes "
                   "the checks, the sort by size class, the copies in and out, one host scan of the lengths per chunk "
                   "and the host's copy of the packed words into the caller's buffer. Not measured: hardware "
                   "counters, the size classes apart."}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        sub = make_set(lv["live_fills"], lv["live_exts"])
        chain.extd2(sub)
        sub_cells = chain.extd2_timing()[2]
        per_cell = lv["seconds"]["median"] / sub_cells
        ref16 = per_cell * cells / 16
        out["reference"] = {"live_items": lv["live_items"], "live_cells": sub_cells, "one_thread_s_per_cell": per_cell,
                            "one_thread_gcells_per_s": 1e-9 / per_cell,
                            "projected_16_thread_gcells_per_s": 16e-9 / per_cell,
                            "projected_set_seconds_on_16_threads": ref16,
                            "how": "a projection: one-thread time of the first %d items, per cell the device counts "
                                   "for them, times this set's cells, divided by 16" % lv["live_items"],
                            "speedup_fill": ref16 / (np.median(fill) * 1e-3),
                            "speedup_kernels": ref16 / ((np.median(fill) + np.median(walk)) * 1e-3),
                            "speedup_call": ref16 / (np.median(call) * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--reference", default=None, help="the reference tree (default: the recorder's)")
    ap.add_argument("--live-fills", type=int, default=150)
    ap.add_argument("--live-exts", type=int, default=15)
    ap.add_argument("--fills", type=int, default=FILLS)
    ap.add_argument("--exts", type=int, default=EXTS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_extd2_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
