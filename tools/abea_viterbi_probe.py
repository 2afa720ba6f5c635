#!/usr/bin/env python3
"""abea Viterbi probe: gb_abea_hmm_align on a seeded set of 100 000 items shaped like the windows that eventalign's
align_read_to_ref cuts (95..105 k-mers, 1.2..2.5 events per k-mer, both strands), against f5c's CPU
profile_hmm_align on the first items of the same set, and beside gb_abea_hmm_score (the forward kernel) on items
of the same k-mer and row counts in the same process.

The set is generated in pieces of --piece-reads reads of one shape each (one item per read); the generator draws
piece after piece, so a prefix of the pieces is a prefix of the set.

  --live   on the build host (needs the reference tree and g++): times the live profile_hmm_align on one thread
           over the first --live-pieces pieces and stores the times beside the set's seed in
           profiles/abea_viterbi_probe_live.json. The GPU machine has no reference tree, so this part is run
           beforehand.
  default  on the GPU: one warm-up call, then --reps calls; medians with minimum and maximum of the fill kernels'
           time, the walk kernel's and of the whole synchronous call, cells per second; the same for the forward
           kernel on --forward-pieces pieces of the same shapes; with the live file present, the ratio to the
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

SEED, PIECES, PIECE_READS = 20261022, 200, 500
LIVE_JSON = os.path.join(ROOT, "profiles", "abea_viterbi_probe_live.json")
SET = "windows of 95..105 k-mers with 1.2..2.5 events per k-mer, one item per read, a random strand each"


def shapes(pieces):
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(pieces):
        nk = int(rng.integers(95, 106))
        out.append((nk, int(nk * rng.uniform(1.2, 2.5))))
    return out


def make_set(pieces, piece_reads):
    rng = np.random.default_rng(SEED + 1)
    model = gen.abea_model(rng)
    return gen.AbeaAlignItems.concat([gen.abea_align_items(rng, [(piece_reads, nk, rows)], model=model)
                                      for nk, rows in shapes(pieces)])


def make_forward_set(pieces, piece_reads):
    """Items for the forward kernel with the same k-mer and row counts, piece for piece."""
    rng = np.random.default_rng(SEED + 2)
    model = gen.abea_cpg_model(rng)
    return gen.AbeaHmmItems.concat([gen.abea_hmm_items(rng, [(piece_reads, nk, rows)], model=model, meth="none", flags=0)
                                    for nk, rows in shapes(pieces)])


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_abea_viterbi_golden as mk
    x = make_set(args.live_pieces, args.piece_reads)
    live = mk.LiveViterbi(args.reference or mk.REF_TREE)
    try:
        per_rep = []
        for _ in range(3):
            t = time.perf_counter()
            live.align(x)
            per_rep.append(time.perf_counter() - t)
    finally:
        live.close()
    out = {"seed": SEED, "set": SET, "live_items": x.n, "live_cells": x.cells(), "threads": 1, "seconds": spread(per_rep),
           "note": "profile_hmm_align of benchmarks/abea/src/eventalign.c, g++ -O2 -ffp-contract=off, called item after "
                   "item through ctypes on the build host's CPU; includes the shim's copy of the read's events and of "
                   "the records"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import abea
    t = time.perf_counter()
    x = make_set(args.pieces, args.piece_reads)
    gen_s = time.perf_counter() - t
    cells = x.cells()
    fill, walk, call, rec = [], [], [], None
    for rep in range(args.reps + 1):  # the first call is the warm-up: buffers, code object, clocks
        t = time.perf_counter()
        rec, off = abea.hmm_align(x)
        dt = time.perf_counter() - t
        f, w, c = abea.hmm_align_timing()
        assert c == cells
        if rep:
            fill.append(f), walk.append(w), call.append(dt * 1e3)
    chunks, ws_bytes = abea.hmm_align_plan()
    fx = make_forward_set(args.forward_pieces, args.piece_reads)
    fwd = []
    for rep in range(args.reps + 1):
        abea.hmm_score(fx)
        ms, c = abea.hmm_timing()
        assert c == fx.cells()
        if rep:
            fwd.append(ms)
    out = {"seed": SEED, "set": SET, "items": x.n, "reads": len(x.reads), "cells": cells, "events": len(x.events),
           "records": len(rec), "skip_records": int((rec["state"] == b"K").sum()),
           "bad_event_records": int((rec["state"] == b"B").sum()), "chunks": chunks, "largest_chunk_workspace_bytes": ws_bytes,
           "generate_s": gen_s, "reps": args.reps, "warmup_calls": 1,
           "fill_ms": spread(fill), "walk_ms": spread(walk), "call_ms": spread(call),
           "cells_per_s_fill": cells / (np.median(fill) * 1e-3),
           "cells_per_s_fill_and_walk": cells / ((np.median(fill) + np.median(walk)) * 1e-3),
           "code_bytes_per_s_fill": 2 * cells / (np.median(fill) * 1e-3),
           "forward_kernel": {"items": fx.n, "cells": fx.cells(), "kernel_ms": spread(fwd),
                              "cells_per_s_kernel": fx.cells() / (np.median(fwd) * 1e-3),
                              "what": "gb_abea_hmm_score on items of the same k-mer and row counts (flags 0), same process"},
           "note": "fill_ms (one launch per size class) and walk_ms (the walk and the pack) are event-timed spans "
                   "summed over the chunks; the call includes the checks, the sort by size class and rows, the "
                   "copies in and out, one host scan of the lengths per chunk and the host's copy of the packed "
                   "records into the caller's buffer"}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        per_cell = lv["seconds"]["median"] / lv["live_cells"]
        ref16 = per_cell * cells / 16
        out["reference"] = {"one_thread_s_per_cell": per_cell, "projected_set_seconds_on_16_threads": ref16,
                            "how": "a projection: one-thread time of the first %d items, per cell, times this set's "
                                   "cells, divided by 16" % lv["live_items"],
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
    ap.add_argument("--live-pieces", type=int, default=6)
    ap.add_argument("--pieces", type=int, default=PIECES)
    ap.add_argument("--forward-pieces", type=int, default=40)
    ap.add_argument("--piece-reads", type=int, default=PIECE_READS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abea_viterbi_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
