"""Rate of gb_bsw_local (csrc/bsw_local.hip) on a seeded mate-rescue-shaped set, and of bwa's live
ksw_align2 on the same set.

    python tools/bsw_local_probe.py [--pairs 100000] [--reps 5] [--seed 31]      # the GPU leg
    python tools/bsw_local_probe.py --cpu [--cpu-pairs 4000]                     # live ksw_align2, one thread

The set: query U[101,151] bases, target U[300,1200] bases holding one copy of the query with 4 %
substitutions and, in 30 % of pairs, one indel of 1-6 bases; 0.2 % N; xtra = local_xtra(len2), that
is mem_matesw's XSUBO | XSTART | XBYTE | 19 (tools/bwa/bwamem_pair.c:150). Cells = sum of len1 * L
over the pairs, L = len2 rounded up to the reference's 16 (XBYTE) or 8 columns: the first pass only,
although every pair with a hit runs the start pass too. GCUPS = cells / kernel time. With
oracle/_ref built, the first --check pairs are compared with live ksw_align2 as well.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from genomicsbench_palisade_amd import bsw, gen  # noqa: E402


def rescue_pairs(n, seed=31):
    rng = np.random.default_rng(seed)
    ql = rng.integers(101, 152, n).astype(np.int32)
    tl = rng.integers(300, 1201, n).astype(np.int32)
    qoff, _, _ = gen._ragged_local(ql)
    toff, tpid, k = gen._ragged_local(tl)
    qry = rng.integers(0, 4, int(ql.sum())).astype(np.uint8)
    tgt = rng.integers(0, 4, len(k)).astype(np.uint8)
    pos = (rng.random(n) * (tl - ql + 1)).astype(np.int64)
    brk = (rng.random(n) * ql).astype(np.int64)
    dlt = rng.integers(1, 7, n) * np.where(rng.random(n) < 0.5, -1, 1)
    dlt[rng.random(n) >= 0.3] = 0
    rel = k - pos[tpid]
    src = rel + np.where(rel >= brk[tpid], dlt[tpid], 0)
    ok = (rel >= 0) & (rel < ql[tpid]) & (src >= 0) & (src < ql[tpid])
    tgt[ok] = qry[qoff[tpid[ok]] + src[ok]]
    m = ok & (rng.random(len(tgt)) < 0.04)
    tgt[m] = rng.integers(0, 4, int(m.sum())).astype(np.uint8)
    tgt[rng.random(len(tgt)) < 0.002] = 4
    qry[rng.random(len(qry)) < 0.002] = 4
    return gen.BswPairs(tgt, toff, tl, qry, qoff, ql, np.zeros(n, np.int32))


def cells(pairs, xtra):
    p = np.where((xtra & bsw.KSW_XBYTE) != 0, 16, 8).astype(np.int64)
    L = (pairs.qlen.astype(np.int64) + p - 1) // p * p
    return int((pairs.tlen.astype(np.int64) * L).sum())


def live(pairs, xtra, n):
    """(int32 [n, 7], seconds) of live ksw_align2 on the first n pairs, one thread; None without oracle/_ref."""
    import make_bsw_local_golden as mk
    lib = mk.ref_lib()
    if lib is None:
        return None
    P = bsw.default_params()
    mat = P.mat_array()
    q, t = pairs.qry.copy(), pairs.tgt.copy()  # the reference reverses in place, and back
    qb, tb = q.ctypes.data, t.ctypes.data
    args = [(int(pairs.qlen[k]), qb + int(pairs.qoff[k]), int(pairs.tlen[k]), tb + int(pairs.toff[k]), int(xtra[k]))
            for k in range(n)]
    out = np.zeros((n, 7), np.int32)
    t0 = time.perf_counter()
    for k, (a, b, c, d, x) in enumerate(args):
        r = lib.ksw_align2(a, b, c, d, 5, mat.ctypes.data, P.o_del, P.e_del, P.o_ins, P.e_ins, x, None)
        out[k] = (r.score, r.te, r.qe, r.score2, r.te2, r.tb, r.qb)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--check", type=int, default=2000, help="pairs compared with live ksw_align2 (GPU leg)")
    ap.add_argument("--cpu", action="store_true", help="time live ksw_align2 instead (no GPU needed)")
    ap.add_argument("--cpu-pairs", type=int, default=4000)
    a = ap.parse_args()
    pairs = rescue_pairs(a.pairs, a.seed)
    xtra = bsw.local_xtra(pairs.qlen)
    tot = cells(pairs, xtra)
    print(f"set: {pairs.n} pairs, {tot / 1e9:.3f} G cells, mean target {pairs.tlen.mean():.0f}, mean query {pairs.qlen.mean():.0f}")
    if a.cpu:
        n = min(a.cpu_pairs, pairs.n)
        got = live(pairs, xtra, n)
        if got is None:
            sys.exit("oracle/_ref/libref_bwa.so not built")
        c = cells(pairs.slice(0, n), xtra[:n])
        print(f"live ksw_align2, one thread: {n} pairs in {got[1] * 1e3:.1f} ms = {c / got[1] / 1e9:.3f} GCUPS; "
              f"times 16 = {16 * c / got[1] / 1e9:.2f} GCUPS")
        return
    from genomicsbench_palisade_amd import set_device
    set_device(0)
    best, res = None, None
    for _ in range(max(1, a.reps) + 1):  # the first call allocates and is not counted
        t0 = time.perf_counter()
        res = bsw.local_align(pairs, xtra)
        wall = time.perf_counter() - t0
        ms = bsw.local_timing()
        if _ and (best is None or ms < best[0]):
            best = (ms, wall)
    ms, wall = best
    print(f"gb_bsw_local: kernel {ms:.3f} ms = {tot / ms / 1e6:.2f} GCUPS (best of {a.reps}); whole call {wall * 1e3:.1f} ms "
          f"= {tot / wall / 1e9:.2f} GCUPS incl. copies")
    rows = np.stack(res, axis=1)
    print(f"hits: score >= 19 on {int((rows[:, 0] >= 19).sum())}, start found on {int((rows[:, 5] >= 0).sum())}, "
          f"score2 >= 0 on {int((rows[:, 3] >= 0).sum())}")
    n = min(a.check, pairs.n)
    got = live(pairs, xtra, n) if n else None
    if got is not None:
        bad = int((got[0] != rows[:n]).any(axis=1).sum())
        print(f"against live ksw_align2 on the first {n} pairs: {bad} differ")
        if bad:
            sys.exit(1)


if __name__ == "__main__":
    main()
