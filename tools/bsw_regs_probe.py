#!/usr/bin/env python3
"""Probe for gb_bsw_finish_regs: call time of both stages on 1 and on 16 host threads.

The call runs on the host, so the probe needs no GPU and its input is made without one: 100 000 reads of
100 to 250 bases with the hand-made region sets of the fixture's generator (make_constructed: cut true
alignments, redundant pairs, ALT mixes, random sets of up to 44 regions) over the fixture's reference.
That is a far heavier mix than short reads give (about 4 regions and 1.8 merge alignments per read). One
warm-up call, then the median and the range of 10 calls per setting.

  python tools/bsw_regs_probe.py [--reads 100000] [--reps 10] [--out profiles/bsw_regs_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsw_regs_probe.json"))
    a = ap.parse_args()
    import make_bsw_regs_golden as rg
    from genomicsbench_palisade_amd import bsw
    fx = np.load(os.path.join(ROOT, "tests", "golden", "bsw_mkchain_golden.npz"))
    codes, contig_end, is_alt = fx["ref_codes"], fx["contig_end"], fx["contig_is_alt"]
    made = rg.make_constructed(codes, contig_end, is_alt, a.reads, seed=1)
    reads = [x for x, _ in made]
    lens = np.array([len(x) for x in reads], np.int32)
    idq = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])[:-1]
    qbuf = np.concatenate(reads).astype(np.uint8)
    reg_off = np.concatenate([[0], np.cumsum([len(g) for _, g in made], dtype=np.int64)]).astype(np.int64)
    flat = [g for _, gs in made for g in gs]
    regs = np.zeros(len(flat), bsw.ALNREG_DTYPE)
    for f in rg.IN_FIELDS:
        regs[f] = [g[f] for g in flat]
    ref = bsw.Ref.from_codes(codes)
    res = {"reads": a.reads, "regions": int(len(regs)), "reps": a.reps, "settings": []}
    for threads in (1, 16):
        os.environ["GB_BSW_REGS_THREADS"] = str(threads)
        for stage in (0, 1):
            bsw.finish_regs(ref, qbuf, idq, lens, reg_off, regs, stage=stage, contig_is_alt=is_alt)
            ms = []
            for _ in range(a.reps):
                t = time.perf_counter()
                out, n_out = bsw.finish_regs(ref, qbuf, idq, lens, reg_off, regs, stage=stage, contig_is_alt=is_alt)
                ms.append((time.perf_counter() - t) * 1e3)
            tm = bsw.finish_regs_timing()
            row = {"threads": threads, "stage": stage, "call_ms_median": float(np.median(ms)), "call_ms_min": min(ms),
                   "call_ms_max": max(ms), "regions_left": int(n_out.sum()), "alignments": tm[4],
                   "most_alignments_of_one_read": tm[3], "host_reads": tm[5]}
            res["settings"].append(row)
            print(row)
    res["cpus"] = os.cpu_count()
    res["note"] = ("call time includes the wrapper's copy of the region array; the call runs on the host, the three "
                   "device times of finish_regs_timing are 0; the library runs at most as many threads as the machine "
                   "has logical CPUs (cpus)")
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)
    ref.close()


if __name__ == "__main__":
    main()
