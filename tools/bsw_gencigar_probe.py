"""gb_bsw_gen_cigar probe: coordinates in, score / CIGAR / NM / MD out, against today's route.

    python tools/bsw_gencigar_probe.py [--pairs 100000] [--ref-bases 268435456] [--steps 10] [--out file.json]

The pairs are gen.bsw_pairs' (the global probe's shapes); every target is planted into a random
reference of --ref-bases bases (64 MiB packed at the default, so the pac does not sit in L2), one pair
per stride, and every second pair is addressed as a reverse-strand region with its query
reverse-complemented. w_ = 100 for every pair. Reported, as medians over --steps calls:
  device_call_ms     a host clock around gb_bsw_gen_cigar (C ABI, pair records and query buffer prebuilt)
  fetch / fill / walk / md_ms   the four kernel times of gb_bsw_gen_cigar_timing
  host_route         today's route for the same pairs: the targets gathered from the pac and the
                     reverse-strand pairs' queries reversed with vectorised numpy (fetch_ms), then the
                     band rule and gb_bsw_global (global_ms). Its MD step is timed apart on a sample
                     with the test suite's plain Python writer (md_sample) and is NOT part of
                     route_ms, which is therefore a lower bound of today's route.
  cpu_bwa_gen_cigar2 the reference's bwa_gen_cigar2 (oracle/_ref/libref_bwa.so, when built) called per
                     pair on one thread on a sample, checked bit for bit against the device results.
The device results are also checked against the host route (score, CIGAR, NM). Prints one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genomicsbench_palisade_amd import bsw, check, gen, set_device  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def ragged(lens):
    """(offsets, pair index, position within pair) of a ragged concatenation."""
    lens = lens.astype(np.int64)
    off = np.zeros(len(lens), np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    pid = np.repeat(np.arange(len(lens)), lens)
    return off, pid, np.arange(int(lens.sum())) - off[pid]


def build(n, ref_bases, seed=11):
    rng = np.random.default_rng(seed)
    pairs = gen.bsw_pairs(n, seed=seed)
    codes = rng.integers(0, 4, ref_bases, dtype=np.uint8)
    stride = ref_bases // n
    assert stride >= int(pairs.tlen.max()), "the reference is too short for one pair per stride"
    pos = np.arange(n, dtype=np.int64) * stride + rng.integers(0, stride - int(pairs.tlen.max()) + 1, n)
    toff, pid, k = ragged(pairs.tlen)
    codes[pos[pid] + k] = np.minimum(pairs.tgt, 3)  # the pac holds no N
    pac = bsw.pack_pac(codes)
    del codes
    rev = (np.arange(n) & 1).astype(bool)
    L = ref_bases
    end = pos + pairs.tlen
    # a reverse-strand region covers the same forward bases; its query is the reverse complement
    rb, re = np.where(rev, 2 * L - end, pos), np.where(rev, 2 * L - pos, end)
    qoff, qpid, qk = ragged(pairs.qlen)
    src = qoff[qpid] + np.where(rev[qpid], pairs.qlen[qpid] - 1 - qk, qk)
    q = pairs.qry[src]
    qbuf = np.where(rev[qpid] & (q < 4), 3 - q, q).astype(np.uint8)
    return pairs, pac, L, rb, re, rev, qoff, qbuf


def host_fetch(pac, L, rb, re, rev, qoff, qlen, qbuf):
    """What a caller does today before gb_bsw_global: the target bytes of every region, as bwa_gen_cigar2
    hands them to the DP (reverse-strand regions: the complement in forward order), and the queries with
    those of the reverse-strand pairs reversed."""
    tl = (re - rb).astype(np.int32)
    toff, pid, k = ragged(tl)
    base = np.where(rev, 2 * L - re, rb)[pid] + k
    tgt = ((pac[base >> 2] >> ((~base & 3) << 1)) & 3).astype(np.uint8)
    tgt[rev[pid]] ^= 3
    _, qpid, qk = ragged(qlen)
    qry = qbuf[qoff[qpid] + np.where(rev[qpid], qlen[qpid] - 1 - qk, qk)]
    return gen.BswPairs(tgt, toff, tl, qry, qoff, qlen, np.zeros(len(tl), np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--ref-bases", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--md-sample", type=int, default=2000)
    ap.add_argument("--cpu-sample", type=int, default=20_000)
    ap.add_argument("--out")
    a = ap.parse_args()
    set_device(0)
    params = bsw.default_params()
    pairs, pac, L, rb, re, rev, qoff, qbuf = build(a.pairs, a.ref_bases)
    n = pairs.n
    ref = bsw.Ref.from_pac(pac, L)
    cp = np.zeros(n, bsw.CPAIR_DTYPE)
    cp["rb"], cp["re"], cp["idq"], cp["len2"], cp["w"] = rb, re, qoff, pairs.qlen, 100
    ccap, mcap = int((re - rb).sum() + pairs.qlen.sum()), bsw.md_cap(rb, re)
    cigar, md = np.zeros(ccap, np.uint32), np.zeros(mcap, np.uint8)
    cu, mu = ctypes.c_int64(), ctypes.c_int64()
    fn = bsw._decl_gencigar().gb_bsw_gen_cigar

    def device():
        t = time.perf_counter()
        check(fn(ctypes.byref(params), ref.h, cp.ctypes.data, n, qbuf.ctypes.data, len(qbuf), cigar.ctypes.data, ccap,
                 ctypes.byref(cu), md.ctypes.data, mcap, ctypes.byref(mu)), "gb_bsw_gen_cigar")
        return (time.perf_counter() - t) * 1e3

    device(), device()  # the first call uploads the reference
    call, kern = [], []
    for _ in range(a.steps):
        call.append(device())
        kern.append(bsw.gen_cigar_timing())
    r = {"pairs": n, "ref_bases": L, "reverse_pairs": int(rev.sum()), "steps": a.steps, "cigar_ops": cu.value,
         "md_bytes": mu.value, "device_call_ms": spread(call)}
    for k, name in enumerate(("fetch_ms", "fill_ms", "walk_ms", "md_ms")):
        r[name] = spread([x[k] for x in kern])

    f_ms, g_ms = [], []
    for _ in range(max(2, a.steps // 2) + 1):
        t = time.perf_counter()
        hp = host_fetch(pac, L, rb, re, rev, qoff, pairs.qlen, qbuf)
        t1 = time.perf_counter()
        band = bsw.global_band(hp.qlen, hp.tlen, 100, params)
        score, ncig, nm, off, cig = bsw.global_align(hp, band, params)
        g_ms.append((time.perf_counter() - t1) * 1e3)
        f_ms.append((t1 - t) * 1e3)
    f_ms, g_ms = f_ms[1:], g_ms[1:]  # the first round warms up
    same = bool((score == cp["score"]).all() and (ncig == cp["n_cigar"]).all() and (nm == cp["nm"]).all() and
                (cig == cigar[:cu.value]).all())
    from test_bsw_gencigar import md_np
    m = min(a.md_sample, n)
    t = time.perf_counter()
    md_ok = True
    for p in range(m):
        s, _ = md_np(cig[off[p]:off[p] + ncig[p]], hp.qry[hp.qoff[p]:hp.qoff[p] + hp.qlen[p]],
                     hp.tgt[hp.toff[p]:hp.toff[p] + hp.tlen[p]], bool(rev[p]))
        md_ok &= s.encode() == md[cp["md_off"][p]:cp["md_off"][p] + cp["md_len"][p]].tobytes()
    md_s = time.perf_counter() - t
    r["host_route"] = {"fetch_ms": spread(f_ms), "global_ms": spread(g_ms),
                       "route_ms": statistics.median(f_ms) + statistics.median(g_ms),
                       "md_sample": {"pairs": m, "seconds": md_s, "python_writer_ms_per_100k_pairs": md_s / m * 1e8},
                       "same_score_cigar_nm_as_device": same, "sample_md_same_as_device": bool(md_ok)}
    r["device_over_host_route"] = statistics.median(call) / r["host_route"]["route_ms"]

    import make_bsw_gencigar_golden as mk
    live = mk.ref_lib()
    if live is None:
        r["cpu_bwa_gen_cigar2"] = "not measured (oracle/_ref not built)"
    else:
        m = min(a.cpu_sample, n)
        pen, mat = (params.o_del, params.e_del, params.o_ins, params.e_ins), np.ascontiguousarray(params.mat_array())
        qs = [qbuf[qoff[p]:qoff[p] + pairs.qlen[p]] for p in range(m)]
        t = time.perf_counter()
        res = [mk.gen_cigar2_one(live, pac, L, qs[p], rb[p], re[p], 100, pen, mat) for p in range(m)]
        dt = time.perf_counter() - t
        bad = sum(1 for p, (s, o, x, d) in enumerate(res)
                  if s != cp["score"][p] or x != cp["nm"][p] or
                  o.tobytes() != cigar[cp["cigar_off"][p]:cp["cigar_off"][p] + cp["n_cigar"][p]].tobytes() or
                  d != md[cp["md_off"][p]:cp["md_off"][p] + cp["md_len"][p]].tobytes())
        r["cpu_bwa_gen_cigar2"] = {"pairs": m, "threads": 1, "seconds": dt, "pairs_per_s_per_thread": m / dt,
                                   "pairs_differing_from_device": bad}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not (same and md_ok) or (live is not None and r["cpu_bwa_gen_cigar2"]["pairs_differing_from_device"]):
        sys.exit("device results differ")


if __name__ == "__main__":
    main()
