"""gb_bsw_mate_rescue probe: where the time of a mate-rescue call goes.

    python tools/bsw_matesw_probe.py [--pairs 100000] [--ref-bases 67108864] [--unplaced 0.1] [--steps 10] [--out file.json]

A random reference of --ref-bases bases, one contig. Pairs of 151-base reads in FR orientation around an insert
of 400 +- 40 bases, both strands, 1 % substitutions. Every read that is placed carries one hand-made stage-0
region at its true place; a share --unplaced of the pairs has one mate without a region, which the call has to
rescue from its anchor. A twentieth of the placed pairs carry a second, far-away region on one read (a second
anchor, hence a second round). pes is gb_bsw_pestat's over these regions. Reported, as medians over --steps
calls after two warm-up calls:
  call_ms                          a host clock around gb_bsw_mate_rescue (C ABI, arrays prebuilt)
  fetch / dp / region / host_ms    gb_bsw_mate_rescue_timing: the window and fetch kernels, the local DP fed from the
                                   resident windows, the region kernel, and the host bookkeeping between the rounds
  rounds, requests, rescued        and dp_gcups = the DP's cells (window * 151 per request that ran) / dp_ms
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genomicsbench_palisade_amd import bsw, set_device  # noqa: E402

QLEN = 151


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def rc(x):
    return (3 - x)[:, ::-1]


def build(n, L, unplaced, seed=29):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, L, dtype=np.uint8)
    ins = np.clip(rng.normal(400, 40, n).astype(np.int64), QLEN + 10, 800)
    p = rng.integers(1000, L - 2000, n)
    ar = np.arange(QLEN)[None, :]
    left, right = ref[p[:, None] + ar], ref[(p + ins - QLEN)[:, None] + ar]
    for x in (left, right):
        mut = rng.random(x.shape) < 0.01
        x[mut] = (x[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
    flip = rng.random(n) < 0.5  # the fragment from the other strand: read 1 is the right end
    r1 = np.where(flip[:, None], rc(right), left)
    r2 = np.where(flip[:, None], left, rc(right))
    # rb in the doubled space: a forward read at its start, a reversed one mirrored from its end
    f1 = np.where(flip, 2 * L - (p + ins), p)
    f2 = np.where(flip, p, 2 * L - (p + ins))
    reads = np.empty((2 * n, QLEN), np.uint8)
    reads[0::2], reads[1::2] = r1, r2
    rb = np.empty(2 * n, np.int64)
    rb[0::2], rb[1::2] = f1, f2
    lost = rng.random(n) < unplaced
    side = rng.integers(0, 2, n)
    n_reg = np.ones(2 * n, np.int64)
    n_reg[2 * np.flatnonzero(lost) + side[lost]] = 0
    extra = np.flatnonzero(~lost & (rng.random(n) < 0.05))
    n_reg[2 * extra] = 2
    reg_off = np.concatenate([[0], np.cumsum(n_reg)]).astype(np.int64)
    regs = np.zeros(int(reg_off[-1]), bsw.ALNREG_DTYPE)
    first = reg_off[:-1][n_reg > 0]
    regs["rb"][first] = rb[n_reg > 0]
    second = reg_off[2 * extra] + 1
    regs["rb"][second] = rng.integers(1000, L - 2000, len(extra))
    regs["re"] = regs["rb"] + QLEN
    regs["qe"], regs["score"], regs["truesc"], regs["seedcov"], regs["seedlen0"], regs["n_comp"] = QLEN, 140, 140, 75, 19, 1
    regs["score"][second] = 135
    return ref, reads, reg_off, regs, int(lost.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--ref-bases", type=int, default=1 << 26)
    ap.add_argument("--unplaced", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    set_device(0)
    n, L = a.pairs, a.ref_bases
    codes, reads, reg_off, regs, n_lost = build(n, L, a.unplaced)
    ref = bsw.Ref.from_codes(codes)
    del codes
    lens = np.full(2 * n, QLEN, np.int32)
    idq = np.arange(2 * n, dtype=np.int64) * QLEN
    qbuf = reads.ravel()
    t0 = time.perf_counter()
    pes = bsw.pestat(L, reg_off, regs)
    pestat_ms = (time.perf_counter() - t0) * 1e3
    ms, tim, res = [], [], None
    for k in range(a.steps + 2):
        t0 = time.perf_counter()
        res = bsw.mate_rescue(ref, pes, qbuf, idq, lens, reg_off, regs)
        if k >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
            tim.append(bsw.mate_rescue_timing())
    ref.close()
    gained = int((res["n_out"] > np.diff(reg_off)).sum())
    fr = pes[1]
    cells = float(res["n_sw"].sum()) * (int(fr["high"]) - int(fr["low"]) + QLEN) * QLEN
    dp = statistics.median(t[1] for t in tim)
    r = {"pairs": n, "ref_bases": L, "read_len": QLEN, "unplaced_mates": n_lost, "steps": a.steps,
         "pes": [[int(p["low"]), int(p["high"]), int(p["failed"])] for p in pes], "pestat_ms": pestat_ms,
         "call_ms": spread(ms), "fetch_ms": spread([t[0] for t in tim]), "dp_ms": spread([t[1] for t in tim]),
         "region_ms": spread([t[2] for t in tim]), "host_ms": spread([t[3] for t in tim]), "rounds": tim[-1][4],
         "requests": tim[-1][5], "alignments": int(res["n_sw"].sum()), "reads_with_a_region_gained": gained,
         "dp_gcups": cells / (dp * 1e6) if dp > 0 else None,
         "host_share_of_call": statistics.median(t[3] for t in tim) / statistics.median(ms)}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
