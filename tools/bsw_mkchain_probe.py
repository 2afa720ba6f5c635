"""gb_bsw_seeds2chains probe: SMEMs and their coordinates in, chains out, device path against host path.

    python tools/bsw_mkchain_probe.py [--reads 100000] [--ref-bases 268435456] [--steps 10] [--out file.json]

A random reference of --ref-bases bases gets planted repeats: tandem arrays (a unit of 20 to 60 bases, 10 to
30 copies, a substitution now and then) and a dispersed family (copies of a 300-base unit, 2 % diverged).
Reads of 151 bases with 1 % substitutions, both strands: 60 % from anywhere, 20 % from the tandem arrays,
20 % from the family. The seeds are the library's own: gb_fmi_index_build, gb_fmi_search and
gb_fmi_sa_entries (GB_FMI_SA_COMPRESSED) on the same device. Default options, stage 1. Reported, as medians
over --steps calls after two warm-up calls:
  device_call_ms              a host clock around gb_bsw_seeds2chains (C ABI, arrays prebuilt)
  build / filter / emit_ms    the kernel groups of gb_bsw_seeds2chains_timing, and host_reads
  host_1_thread_ms, host_16_threads_ms   the same call with GB_BSW_MKCHAIN_HOST=1 and
                              GB_BSW_MKCHAIN_THREADS=1 / 16; its output is checked against the device's
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genomicsbench_palisade_amd import bsw, check, fmi, set_device  # noqa: E402

QLEN = 151


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def build(n, L, seed=23):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, L, dtype=np.uint8)
    n_tandem, n_family = max(4, L >> 16), max(4, L >> 17)
    tandem = []
    for _ in range(n_tandem):
        unit = rng.integers(0, 4, int(rng.integers(20, 61)), dtype=np.uint8)
        seg = np.tile(unit, int(rng.integers(10, 31)))
        mut = rng.random(len(seg)) < 0.004
        seg[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
        at = int(rng.integers(1000, L - 4000))
        ref[at:at + len(seg)] = seg
        tandem.append((at, len(seg)))
    unit = rng.integers(0, 4, 300, dtype=np.uint8)
    family = rng.integers(1000, L - 4000, n_family)
    for at in family:
        seg = unit.copy()
        mut = rng.random(300) < 0.02
        seg[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
        ref[at:at + 300] = seg
    kind = rng.random(n)
    start = rng.integers(0, L - QLEN, n)
    t = np.array(tandem)[rng.integers(0, n_tandem, n)]
    start = np.where(kind < 0.2, t[:, 0] + (rng.random(n) * np.maximum(t[:, 1] - QLEN, 1)).astype(np.int64) - 20, start)
    start = np.where((kind >= 0.2) & (kind < 0.4), family[rng.integers(0, n_family, n)] + rng.integers(-60, 210, n), start)
    start = np.clip(start, 0, L - QLEN)
    reads = ref[start[:, None] + np.arange(QLEN)[None, :]]
    mut = rng.random(reads.shape) < 0.01
    reads[mut] = (reads[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
    rev = rng.random(n) < 0.5
    reads[rev] = 3 - reads[rev][:, ::-1]
    return ref, np.ascontiguousarray(reads, np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--ref-bases", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    set_device(0)
    n, L = a.reads, a.ref_bases
    ref, reads = build(n, L)
    lens = np.full(n, QLEN, np.int32)
    t = time.perf_counter()
    idx = fmi.Index.build(ref)
    t_build = time.perf_counter() - t
    del ref
    rd = fmi.Reads(idx, reads, lens)
    rd.search(19)
    rd.sync()
    smems = rd.results()[0]
    rd.close()
    coords, counts = idx.sa_entries(smems, max_occ=500, mode=fmi.SA_COMPRESSED)
    idx.close()
    mems = bsw.mems_from_smems(smems, counts)
    coords = np.ascontiguousarray(coords, np.int64)
    nc = len(coords)
    opt = bsw.chain_opt()
    rco, cso = np.zeros(n + 1, np.int64), np.zeros(nc + 1, np.int64)
    seeds, info = np.zeros(max(nc, 1), bsw.SEED_DTYPE), np.zeros(max(nc, 1), bsw.CHAIN_INFO_DTYPE)
    cu, su = ctypes.c_int64(), ctypes.c_int64()
    fn = bsw._decl_mkchain().gb_bsw_seeds2chains

    def call():
        t0 = time.perf_counter()
        check(fn(ctypes.byref(opt), 1, L, None, None, 0, n, lens.ctypes.data, mems.ctypes.data, len(mems),
                 coords.ctypes.data, nc, rco.ctypes.data, cso.ctypes.data, seeds.ctypes.data, info.ctypes.data, nc, nc,
                 ctypes.byref(cu), ctypes.byref(su)), "gb_bsw_seeds2chains")
        return (time.perf_counter() - t0) * 1e3

    def snapshot():
        return [x[:k].tobytes() for x, k in ((rco, n + 1), (cso, cu.value + 1), (seeds, su.value), (info, cu.value))]

    os.environ.pop("GB_BSW_MKCHAIN_HOST", None)
    call(), call()
    ms, kern = [], []
    for _ in range(a.steps):
        ms.append(call())
        kern.append(bsw.seeds2chains_timing())
    dev = snapshot()
    per_read = np.bincount(mems["read"], weights=mems["n_coord"], minlength=n)
    chains_per_read = np.diff(rco)
    r = {"reads": n, "ref_bases": L, "smems": len(mems), "coords": nc, "chains": cu.value, "seeds": su.value,
         "max_coords_per_read": int(per_read.max()), "max_chains_per_read": int(chains_per_read.max()),
         "reads_with_more_than_9_chains": int((chains_per_read > 9).sum()), "steps": a.steps,
         "index_build_s": t_build, "device_call_ms": spread(ms), "build_ms": spread([k[0] for k in kern]),
         "filter_ms": spread([k[1] for k in kern]), "emit_ms": spread([k[2] for k in kern]),
         "host_reads": kern[-1][3]}
    os.environ["GB_BSW_MKCHAIN_HOST"] = "1"
    same = True
    for th in (1, 16):
        os.environ["GB_BSW_MKCHAIN_THREADS"] = str(th)
        call()
        hs = [call() for _ in range(max(3, a.steps // 2))]
        same &= snapshot() == dev
        r["host_%d_thread%s_ms" % (th, "s" if th > 1 else "")] = spread(hs)
    r["host_equals_device"] = same
    r["device_over_host_16"] = statistics.median(ms) / r["host_16_threads_ms"]["median"]
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("host and device results differ")


if __name__ == "__main__":
    main()
