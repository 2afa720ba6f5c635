"""gb_bsw_chain2aln probe: chains of seeds in, alignment regions out, against today's route.

    python tools/bsw_chain2aln_probe.py [--reads 100000] [--ref-bases 268435456] [--steps 10] [--out file.json]

Reads of 151 bases are planted into a random reference of --ref-bases bases, every second one on the
reverse strand, each with two mismatches that cut it into three seeds (one chain); 30 % of the reads get
a second chain, the first two seeds moved to another place. Default parameters. Reported, as medians
over --steps calls after two warm-up calls:
  device_call_ms     a host clock around gb_bsw_chain2aln (C ABI, CSR arrays and query buffer prebuilt)
  gather / ext[4] / finish / filter_ms   the kernel groups of gb_bsw_chain2aln_timing
  second_try_share   the share of extensions that took a second try
  host_route         today's route for the same seeds: the windows gathered from the pac with vectorised
                     numpy, reversed for the left side, into fixed-stride buffers (gather_ms), and the
                     four gb_bsw_get_scores16 calls (scores16_ms): left at w, left at 2 w, right at w,
                     right at 2 w. A C caller would not pay numpy's gather, so the comparison that counts
                     is device_call_ms against scores16_ms. Its results are checked against the raw records.
  cpu_restatement    the fixture generator's restatement of mem_chain2aln (reference ksw_extend2 and
                     bns_get_seq through ctypes, when oracle/_ref is built) on one thread over the first
                     --cpu-sample reads, checked bit for bit against the device's regions.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from genomicsbench_palisade_amd import bsw, check, gen, set_device  # noqa: E402

QLEN = 151


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def ragged(lens):
    lens = lens.astype(np.int64)
    off = np.zeros(len(lens), np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    pid = np.repeat(np.arange(len(lens)), lens)
    return off, pid, np.arange(int(lens.sum())) - off[pid]


def doubled_bases(pac, L, x):
    """The base at doubled-space positions x (bns_get_seq's view)."""
    f = np.where(x >= L, 2 * L - 1 - x, x)
    b = (pac[f >> 2] >> ((~f & 3) << 1)) & 3
    return np.where(x >= L, 3 - b, b).astype(np.uint8)


def max_gap(p, qlen):
    """cal_max_gap (bwamem.c:621-628), vectorised in float64."""
    a = int(p.mat[0])
    l_del = np.trunc((qlen * a - p.o_del) / p.e_del + 1.).astype(np.int64)
    l_ins = np.trunc((qlen * a - p.o_ins) / p.e_ins + 1.).astype(np.int64)
    return np.minimum(np.maximum(np.maximum(l_del, l_ins), 1), p.w << 1)


def build(n, L, seed=17):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, L, dtype=np.uint8)
    pac = bsw.pack_pac(codes)
    del codes
    rev = (np.arange(n) & 1).astype(bool)
    pos = rng.integers(400, L - 400 - QLEN, n) + np.where(rev, L, 0)
    q = doubled_bases(pac, L, (pos[:, None] + np.arange(QLEN)[None, :]).reshape(-1)).reshape(n, QLEN)
    m1, m2 = rng.integers(30, 60, n), rng.integers(90, 120, n)
    for m in (m1, m2):
        q[np.arange(n), m] = (q[np.arange(n), m] + 1 + rng.integers(0, 3, n)) % 4
    two = rng.random(n) < 0.3
    other = rng.integers(400, L - 400 - QLEN, n) + np.where(rng.random(n) < 0.5, L, 0)
    # seeds of the first chain: [0, m1), [m1 + 1, m2), [m2 + 1, QLEN); of the second: the first two, moved
    qb = np.stack([np.zeros(n, np.int64), m1 + 1, m2 + 1, np.zeros(n, np.int64), m1 + 1], axis=1)
    ln = np.stack([m1, m2 - m1 - 1, QLEN - m2 - 1, m1, m2 - m1 - 1], axis=1)
    rb = np.stack([pos + qb[:, 0], pos + qb[:, 1], pos + qb[:, 2], other + qb[:, 3], other + qb[:, 4]], axis=1)
    use = np.ones((n, 5), bool)
    use[~two, 3:] = False
    seeds = np.zeros(int(use.sum()), bsw.SEED_DTYPE)
    seeds["rbeg"], seeds["qbeg"], seeds["len"], seeds["score"] = rb[use], qb[use], ln[use], ln[use]
    n_chain = 1 + two.astype(np.int64)
    rco = np.concatenate([[0], np.cumsum(n_chain)]).astype(np.int64)
    per_chain = np.zeros(int(rco[-1]), np.int64)
    per_chain[rco[:-1]] = 3
    per_chain[rco[:-1][two] + 1] = 2
    cso = np.concatenate([[0], np.cumsum(per_chain)]).astype(np.int64)
    idq = np.arange(n, dtype=np.int64) * QLEN
    return pac, np.ascontiguousarray(q.reshape(-1)), idq, np.full(n, QLEN, np.int32), rco, cso, seeds


def windows(p, L, lq, cso, seeds):
    """rmax of every chain (one contig), vectorised: bwamem.c:642-657."""
    chain = np.repeat(np.arange(len(cso) - 1), np.diff(cso))
    right = lq - seeds["qbeg"] - seeds["len"]
    b = seeds["rbeg"] - (seeds["qbeg"] + max_gap(p, seeds["qbeg"].astype(np.int64)))
    e = seeds["rbeg"] + seeds["len"] + right + max_gap(p, right.astype(np.int64))
    r0 = np.maximum(np.minimum.reduceat(b, cso[:-1]), 0)
    r1 = np.minimum(np.maximum.reduceat(e, cso[:-1]), 2 * L)
    first = seeds["rbeg"][cso[:-1]]
    cross = (r0 < L) & (L < r1)
    r1 = np.where(cross & (first < L), L, r1)
    r0 = np.where(cross & (first >= L), L, r0)
    return chain, r0, r1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--ref-bases", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cpu-sample", type=int, default=5000)
    ap.add_argument("--out")
    a = ap.parse_args()
    set_device(0)
    params = bsw.default_params()
    L, n = a.ref_bases, a.reads
    pac, qbuf, idq, lq, rco, cso, seeds = build(n, L)
    ns = len(seeds)
    ref = bsw.Ref.from_pac(pac, L)
    regs, raw = np.zeros(ns, bsw.REGION_DTYPE), np.zeros(ns, bsw.C2A_RAW_DTYPE)
    reg_off, n_reg, used = np.zeros(n, np.int64), np.zeros(n, np.int32), ctypes.c_int64()
    fn = bsw._decl_chain2aln().gb_bsw_chain2aln

    def device():
        t = time.perf_counter()
        check(fn(ctypes.byref(params), 5, 5, ref.h, None, 0, qbuf.ctypes.data, len(qbuf), n, idq.ctypes.data,
                 lq.ctypes.data, rco.ctypes.data, cso.ctypes.data, seeds.ctypes.data, regs.ctypes.data, ns,
                 reg_off.ctypes.data, n_reg.ctypes.data, ctypes.byref(used), raw.ctypes.data), "gb_bsw_chain2aln")
        return (time.perf_counter() - t) * 1e3

    device(), device()  # the first call uploads the reference
    call, kern = [], []
    for _ in range(a.steps):
        call.append(device())
        kern.append(bsw.chain2aln_timing())
    tries = raw["tries"]
    r = {"reads": n, "chains": int(rco[-1]), "seeds": ns, "regions": used.value, "ref_bases": L, "steps": a.steps,
         "device_call_ms": spread(call), "gather_ms": spread([k[0] for k in kern]),
         "ext_ms": [spread([k[1][i] for k in kern]) for i in range(4)], "finish_ms": spread([k[2] for k in kern]),
         "filter_ms": spread([k[3] for k in kern]),
         "kernel_sum_ms": statistics.median([k[0] + sum(k[1]) + k[2] + k[3] for k in kern]),
         "extensions": int((tries > 0).sum()), "second_try_share": float((tries == 2).sum() / max((tries > 0).sum(), 1))}

    # today's route
    chain, r0, r1 = windows(params, L, QLEN, cso, seeds)
    thr = (params.w >> 1) + (params.w >> 2)
    a1 = int(params.mat[0])
    g_ms, s_ms, same = [], [], True
    for _ in range(max(2, a.steps // 2) + 1):
        tg = ts = 0.0
        out = np.zeros((ns, 2, 6), np.int32)
        tr = np.zeros((ns, 2), np.int32)
        for side in (0, 1):
            t = time.perf_counter()
            if side == 0:
                idx = np.nonzero(seeds["qbeg"] > 0)[0]
                tl = (seeds["rbeg"] - r0[chain])[idx]
                ql = seeds["qbeg"][idx].astype(np.int64)
                h0 = (seeds["len"][idx] * a1).astype(np.int32)
            else:
                idx = np.nonzero(seeds["qbeg"] + seeds["len"] != QLEN)[0]
                tl = (r1[chain] - seeds["rbeg"] - seeds["len"])[idx]
                ql = (QLEN - seeds["qbeg"] - seeds["len"])[idx].astype(np.int64)
                h0 = np.where(seeds["qbeg"][idx] > 0, out[idx, 0, 0], seeds["len"][idx] * a1).astype(np.int32)
            ts_, qs_ = int(tl.max()) + 1, 256  # the fixed strides
            _, pid, k = ragged(tl)
            sd = seeds[idx[pid]]
            x = sd["rbeg"] - 1 - k if side == 0 else sd["rbeg"] + sd["len"] + k
            tgt = np.zeros(len(idx) * ts_, np.uint8)
            tgt[pid * ts_ + k] = doubled_bases(pac, L, x)
            _, qpid, qk = ragged(ql)
            sq = seeds[idx[qpid]]
            read = np.searchsorted(rco, chain[idx], side="right") - 1
            qx = idq[read[qpid]] + (sq["qbeg"] - 1 - qk if side == 0 else sq["qbeg"] + sq["len"] + qk)
            qry = np.zeros(len(idx) * qs_, np.uint8)
            qry[qpid * qs_ + qk] = qbuf[qx]
            pairs = gen.BswPairs(tgt, np.arange(len(idx), dtype=np.int64) * ts_, tl.astype(np.int32), qry,
                                 np.arange(len(idx), dtype=np.int64) * qs_, ql.astype(np.int32), h0)
            tg += time.perf_counter() - t
            t = time.perf_counter()
            p = bsw.default_params(end_bonus=5)
            sp = bsw.get_scores16(pairs, p)
            o6 = np.stack([sp[f] for f in bsw.OUT_FIELDS], axis=1)
            prev = np.full(len(idx), -1, np.int32) if side == 0 else h0
            again = np.nonzero(~((o6[:, 0] == prev) | (o6[:, 5] < thr)))[0]
            tr[idx, side] = 1
            if len(again):
                p2 = bsw.default_params(end_bonus=5, w=params.w << 1)
                sp2 = bsw.get_scores16(pairs.subset(again), p2)
                o6[again] = np.stack([sp2[f] for f in bsw.OUT_FIELDS], axis=1)
                tr[idx[again], side] = 2
            out[idx, side] = o6
            ts += time.perf_counter() - t
        g_ms.append(tg * 1e3)
        s_ms.append(ts * 1e3)
        same &= bool((out == raw["out6"]).all() and (tr == raw["tries"]).all())
    g_ms, s_ms = g_ms[1:], s_ms[1:]
    r["host_route"] = {"gather_ms": spread(g_ms), "scores16_ms": spread(s_ms), "same_as_raw_records": same}
    r["device_over_scores16"] = statistics.median(call) / statistics.median(s_ms)

    import make_bsw_chain2aln_golden as mk
    live = mk.ref_lib()
    if live is None:
        r["cpu_restatement"] = "not measured (oracle/_ref not built)"
        bad = 0
    else:
        m = min(a.cpu_sample, n)
        o = mk.Opt()
        mk.WITNESS_ZDROP = False  # the fixture's second DP per extension is not part of the route
        reads = [(qbuf[idq[k]:idq[k] + QLEN],
                  [[tuple(int(v) for v in (s["rbeg"], s["qbeg"], s["len"], s["score"])) for s in seeds[cso[c]:cso[c + 1]]]
                   for c in range(rco[k], rco[k + 1])]) for k in range(m)]
        t = time.perf_counter()
        res, cb, sb = [], 0, 0
        for q, chains in reads:
            av, rc = mk.chain2aln_read(live, pac, L, None, o, q, chains, cb, sb)
            res.append(av)
            cb, sb = cb + len(chains), sb + len(rc)
        dt = time.perf_counter() - t
        bad = 0
        for k, av in enumerate(res):
            got = regs[reg_off[k]:reg_off[k] + n_reg[k]]
            exp = [[x[f] for f in mk.REG_FIELDS] for x in av]
            bad += [[int(g[f]) for f in mk.REG_FIELDS] for g in got] != exp
        r["cpu_restatement"] = {"reads": m, "threads": 1, "seconds": dt, "reads_per_s_per_thread": m / dt,
                                "note": "the seeds the reference skips are extended too",
                                "reads_differing_from_device": bad}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same or bad:
        sys.exit("device results differ")


if __name__ == "__main__":
    main()
