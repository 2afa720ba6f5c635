"""Times gb_dbg_assemble on a seeded set of regions and writes profiles/dbg_probe.json.

    python tools/dbg_probe.py --live [reference root]   # build host: the live reference (tests/golden/dbg_live_shim.cpp,
                                                        # one thread) on a prefix of the set -> profiles/dbg_probe_live.json
    python tools/dbg_probe.py [--out FILE]              # GPU: one warm-up call, then the median of 3 calls

The set: gen.dbg_regions(41, 256, repeat_every=7), 256 overlapping regions of 4 500 reference bases and about 300
reads of 150 bases each; every 7th region start has a planted repeat that keeps the k loop going. The x16 figure is
the one-thread time divided by 16: a projection, not a run on 16 threads.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genomicsbench_palisade_amd import dbg, gen  # noqa: E402

SEED, REGIONS, REPEAT_EVERY, LIVE_REGIONS = 41, 256, 7, 64
LIVE = os.path.join(ROOT, "profiles", "dbg_probe_live.json")


def the_set(n=REGIONS):
    regions, reads = dbg.pack(*gen.dbg_regions(SEED, REGIONS, repeat_every=REPEAT_EVERY))
    return (regions.take(np.arange(n)) if n < REGIONS else regions), reads


def live(ref_root):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_dbg_golden
    regions, reads = the_set(LIVE_REGIONS)
    shim = make_dbg_golden.LiveDbg(ref_root) if ref_root else make_dbg_golden.LiveDbg()
    try:
        secs = sorted(shim.seconds(dbg.DEFAULTS, regions, reads) for _ in range(3))
    finally:
        shim.close()
    os.environ["GB_DBG_HOST"] = "1"
    a = dbg.assemble(regions, reads)
    graphs = int(a.summary()["n_graphs"].sum())
    out = {"regions": LIVE_REGIONS, "graphs": graphs, "positions": dbg.timing()["positions"], "threads": 1,
           "compiler": "g++ -O2", "seconds": secs[1], "seconds_min_max": [secs[0], secs[2]],
           "ms_per_region": 1e3 * secs[1] / LIVE_REGIONS}
    with open(LIVE, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def device(out_path):
    from genomicsbench_palisade_amd import set_device
    set_device(0)
    regions, reads = the_set()
    dbg.assemble(regions, reads).close()  # warm-up: allocations, code load
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        a = dbg.assemble(regions, reads)
        call_ms = 1e3 * (time.perf_counter() - t0)
        sm = a.summary()
        a.close()
        t = dbg.timing()
        t["kernels"] = t["build"] + t["rank"] + t["edges"] + t["cycle"]
        t["call"] = call_ms
        runs.append(t)
    runs.sort(key=lambda t: t["call"])
    med, p = runs[1], dbg.plan()
    out = {"set": {"seed": SEED, "regions": len(regions), "reads": len(reads), "ref_bases": int(regions.ref_off[-1]),
                   "read_bases": int(reads.read_off[-1]), "graphs": int(sm["n_graphs"].sum()),
                   "cyclic_at_the_end": int(sm["cyclic"].sum()), "redone": int(sm["redone"].sum()),
                   "nodes_of_final_graphs": int(sm["n_nodes"].sum())},
           "median_of_3_by_call": med, "call_ms_min_max": [runs[0]["call"], runs[2]["call"]], "plan": p,
           "kernel_ms_per_region": med["kernels"] / len(regions), "call_ms_per_region": med["call"] / len(regions),
           "positions_per_s_in_kernels": med["positions"] / (1e-3 * med["kernels"]),
           "not_measured": ["hardware counters", "occupancy", "other region sizes and coverages", "keep = 1",
                            "the host path's rate", "the reference on 16 threads"]}
    if os.path.exists(LIVE):
        lv = json.load(open(LIVE))
        out["reference_one_thread"] = lv
        out["reference_x16_projection_ms_per_region"] = lv["ms_per_region"] / 16
        out["vs_reference_x16_projection"] = {"kernels": lv["ms_per_region"] / 16 / out["kernel_ms_per_region"],
                                              "call": lv["ms_per_region"] / 16 / out["call_ms_per_region"]}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", nargs="?", const="", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbg_probe.json"))
    args = ap.parse_args()
    live(args.live) if args.live is not None else device(args.out)
