#!/usr/bin/env python3
"""kmer probe: gb_kmer_count and gb_kmer_index at k = 17 on one seeded read set shaped like the benchmark's input
(an E. coli-sized genome at 50x: reads of 1 000..20 000 bases, 5 % error), against the live Flye counter on slices of
the same set.

The reads are generated one after the other from one seed, so a prefix of the reads is a prefix of the set.

  --live   on the build host (needs the reference tree and g++): KmerCounter::count(true) of the reference, compiled
           as tests/golden/make_kmer_golden.py compiles it, on one thread over two prefixes of the set (--live-bases).
           count(true) at k = 17 clears an 8 GiB table and walks all 4^17 codes for its histogram whatever the input,
           so two sizes separate that fixed part from the time per occurrence. Stored in profiles/kmer_probe_live.json.
           The GPU machine has no reference tree, so this part is run beforehand.
  default  on the GPU: one warm-up call, then --reps counts and index builds; medians with minimum and maximum of
           every stage's event-timed span from gb_kmer_timing and of the whole synchronous calls, occurrences per
           second in the kernels and over the call, the sort's passes and the bytes a pass moves by construction
           (not measured by counters). With the live file present, the reference's time for this set on 16 threads
           as a projection: the fixed part once plus the per-occurrence part divided by 16. Writes --out.
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

SEED, K, GENOME, COVERAGE = 20261021, 17, 4_641_652, 50
INDEX = (2, 0.4, 10, 100.0)
LIVE_JSON = os.path.join(ROOT, "profiles", "kmer_probe_live.json")
SET = "random genome of 4 641 652 bases with 20 planted 500-base repeats, 50x, reads of 1 000..20 000 bases, 5 % error"


def make_set(coverage):
    return gen.kmer_reads(SEED, GENOME, coverage, (1000, 20000), 0.05, 20)


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def run_live(args):
    import make_kmer_golden as mk
    reads = make_set(max(args.live_bases) / GENOME + 0.01)
    live = mk.LiveFlye(args.reference or mk.REF_TREE)
    runs = []
    try:
        for want in args.live_bases:
            part, total = [], 0
            for r in reads:
                if total >= want:
                    break
                part.append(r)
                total += len(r)
            occ = sum(max(0, len(r) - K) for r in part)
            t = time.perf_counter()
            num, _ = live.run(K, part, np.zeros(0, np.uint64), True)
            runs.append({"reads": len(part), "bases": total, "occurrences": occ, "distinct": int(num),
                         "count_seconds": live.count_seconds, "process_seconds": time.perf_counter() - t})
            print(json.dumps(runs[-1]), flush=True)
    finally:
        live.close()
    a, b = runs[0], runs[-1]
    slope = (b["count_seconds"] - a["count_seconds"]) / (b["occurrences"] - a["occurrences"])
    out = {"seed": SEED, "set": SET, "k": K, "threads": 1, "runs": runs, "seconds_per_occurrence": slope,
           "fixed_seconds": a["count_seconds"] - slope * a["occurrences"],
           "note": "KmerCounter::count(true) of tools/Flye/src/sequence/vertex_index.cpp, g++ -O2, one thread, on the "
                   "build host's CPU; count_seconds is the call itself (table cleared, reads walked, all 4^17 codes "
                   "visited for the histogram); the fixed part and the per-occurrence part are the line through the "
                   "two runs"}
    with open(LIVE_JSON, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def run_gpu(args):
    from genomicsbench_palisade_amd import kmer
    t = time.perf_counter()
    reads = make_set(args.coverage)
    data, off = kmer.pack_reads(reads)
    del reads
    gen_s = time.perf_counter() - t
    stages = ("pack", "extract", "sort", "reduce", "lookup", "select", "fill")
    ms = {s: [] for s in stages}
    count_call, index_call = [], []
    stats = idx_shape = plan_count = plan_index = None
    for rep in range(args.reps + 1):  # the first round is the warm-up: code object, clocks, first allocations
        t = time.perf_counter()
        h = kmer.count(K, (data, off))
        dt_count = time.perf_counter() - t
        plan_count = kmer.plan()
        t = time.perf_counter()
        x = h.index(*INDEX)
        dt_index = time.perf_counter() - t
        plan_index = kmer.plan()
        tm = kmer.timing()
        stats = h.stats()
        idx_shape = {"codes": len(x.codes), "entries": len(x.pos), "repetitive_codes": len(x.rep_codes),
                     "repetitive_frequency": x.repetitive_frequency}
        h.close()
        del x
        if rep:
            for s in stages:
                ms[s].append(tm[s])
            count_call.append(dt_count * 1e3), index_call.append(dt_index * 1e3)
    occ = stats["n_occurrences"]
    med = {s: float(np.median(ms[s])) for s in stages}
    count_kern = med["pack"] + med["extract"] + med["sort"] + med["reduce"]
    index_kern = med["lookup"] + med["select"] + med["fill"]
    tile, passes, _ = plan_count
    tiles = -(-occ // tile)
    out = {"seed": SEED, "set": SET, "k": K, "coverage": args.coverage, "reads": int(len(off) - 1),
           "bases": int(len(data)), "stats": stats, "index_params": INDEX, "index": idx_shape, "generate_s": gen_s,
           "reps": args.reps, "warmup_rounds": 1, "stage_ms": {s: spread(ms[s]) for s in stages},
           "count_call_ms": spread(count_call), "index_call_ms": spread(index_call),
           "count_kernels_ms": count_kern, "index_kernels_ms": index_kern,
           "count_goccurrences_per_s_kernels": occ / (count_kern * 1e-3) / 1e9,
           "count_goccurrences_per_s_call": occ / (np.median(count_call) * 1e-3) / 1e9,
           "index_goccurrences_per_s_kernels": occ / (index_kern * 1e-3) / 1e9,
           "index_goccurrences_per_s_call": occ / (np.median(index_call) * 1e-3) / 1e9,
           "sort": {"tile_keys": tile, "tiles": int(tiles), "passes": passes, "key_bytes": 8,
                    "bytes_per_pass_by_construction": int(3 * 8 * occ + 3 * 4 * 256 * tiles),
                    "how": "keys read by the histogram, read and written by the scatter, and the 256 x tiles table "
                           "written, scanned and read; computed from the sizes, not measured by counters",
                    "gbytes_per_s_by_construction": passes * (3 * 8 * occ + 12 * 256 * tiles) / (med["sort"] * 1e-3) / 1e9},
           "workspace_bytes": {"count": plan_count[2], "index": plan_index[2]},
           "workspace_budget": os.environ.get("GB_KMER_WS", "default (32 GiB)"),
           "note": "stage times are event-timed spans on the call's stream; the calls also hold the host's validation "
                   "of every byte, the copies in, the allocation and release of the workspace and, for the index, the "
                   "copy of the sorted entries to the host and the host pass over the runs. Not measured: hardware "
                   "counters, achieved occupancy, other k, other coverages, the 32-bit key form for k <= 16 (not "
                   "built)."}
    if os.path.exists(LIVE_JSON):
        lv = json.load(open(LIVE_JSON))
        one = lv["fixed_seconds"] + lv["seconds_per_occurrence"] * occ
        p16 = lv["fixed_seconds"] + lv["seconds_per_occurrence"] * occ / 16
        out["reference"] = {"runs": lv["runs"], "seconds_per_occurrence": lv["seconds_per_occurrence"],
                            "fixed_seconds": lv["fixed_seconds"], "extrapolated_one_thread_seconds": one,
                            "projected_16_thread_seconds": p16,
                            "how": "a projection, not a run: the line through two measured one-thread runs on prefixes "
                                   "of this set, the per-occurrence part divided by 16 and the fixed part (table clear "
                                   "and the walk over 4^17 codes, both serial in the reference) kept whole",
                            "speedup_count_kernels": p16 / (count_kern * 1e-3),
                            "speedup_count_call": p16 / (np.median(count_call) * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--reference", default=None, help="the reference tree (default: the recorder's)")
    ap.add_argument("--live-bases", type=int, nargs=2, default=[4_000_000, 24_000_000])
    ap.add_argument("--coverage", type=float, default=COVERAGE)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_probe.json"))
    args = ap.parse_args()
    (run_live if args.live else run_gpu)(args)


if __name__ == "__main__":
    main()
