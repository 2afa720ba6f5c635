"""Constructed chain calls for the backtrack's size classes, and the witnesses that prove what a call
set reaches (tests/test_chain_bt_trees.py, tests/golden/make_chain_bt_trees_golden.py).

strided_call builds calls whose parent links all have one chosen length D, with exactly D * segs
chains: the knob that puts a call on either side of kParentWindow / kMaxIter (5000), kLdsCtr (8192
ends), kLdsW (2048 kept chains), kRsMin (64), kRingSmall (1024) and chain_rows' 64-anchor ring.
tree_witnesses measures, from the DP outputs and the oracle's chains, what a set reaches, so that
the tests assert the class they mean to enter instead of entering it by accident of a generator.

SETS describes every set by generator arguments only (JSON-able; the fixture stores the same
description, not the anchors): each special call lies between two ordinary gen.chain_call calls, so
its CSR offsets are never 0."""
from __future__ import annotations

import numpy as np

from genomicsbench_palisade_amd import gen
from test_chain import _cloud_call, _concat_calls, _long_window_call

ORDINARY_N = 600
PARAMS = (5000, 5000, 500, 1)
# (min_cnt, min_sc). A per = 3 strided chain has 3 anchors and scores 45: (3,45) is the acceptance
# rule at equality on both sides, (3,46) leaves no ends, (4,40) keeps the ends but no chain.
THRESHOLDS = [(3, 40), (3, 45), (3, 46), (4, 40), (1, 0)]


def strided_call(D, per=3, segs=1, extras=0, xstep=1, twins=False, params=PARAMS, span=15):
    """One call of D * segs chains of `per` anchors whose parent links all have length D (2 D with
    twins). Main anchors i = 0 .. D*per*segs - 1 at x = 1000 + i*xstep, y = x + (i % D)*1000 +
    (i // (D*per)) * 2**23: diagonals lie 1000 apart (more than bw), so the only admissible
    predecessor of an anchor is the one D positions back, at dr = dq = D*xstep; segments lie 2**23
    apart in y (more than max_dist). With twins every anchor appears twice at the same x, the copy's
    y larger by D*1000 + 600000 (pairs of chains whose first anchors tie in x). `extras` lone anchors
    follow at x = last + 1 + k, y = 2**29 - 7k (no predecessor, no successor). If D*xstep exceeds
    max_dist_x, or D exceeds max_iter (5000), no chain forms at all."""
    i = np.arange(D * per * segs, dtype=np.int64)
    x = 1000 + i * xstep
    y = x + (i % D) * 1000 + (i // (D * per)) * 2 ** 23
    if twins:
        x = np.repeat(x, 2)
        y = np.repeat(y, 2)
        y[1::2] += D * 1000 + 600000
    if extras:
        k = np.arange(extras, dtype=np.int64)
        x = np.concatenate([x, x[-1] + 1 + k])
        y = np.concatenate([y, 2 ** 29 - 7 * k])
    assert y.max() < 2 ** 31
    yy = (np.uint64(span) << np.uint64(32)) | y.astype(np.uint64)
    return gen.ChainCalls(np.array([0, len(x)]), x.astype(np.uint64), yy, np.array([span], np.float32),
                          np.array([params], np.int32))


def ordinary_call(rng, n=ORDINARY_N):
    """One gen.chain_call call with avg_qspan as the testbed computes it ((float)sum_qspan / n)."""
    x, y, _ = gen.chain_call(rng, n)
    aq = np.float32(int(((y >> np.uint64(32)) & np.uint64(0xff)).sum())) / np.float32(len(x))
    return gen.ChainCalls(np.array([0, len(x)]), x, y, np.array([aq], np.float32), np.array([PARAMS], np.int32))


def _strided(**kw):
    return {"kind": "strided", "args": kw}


# name -> {"pad_seed": rng seed of the ordinary calls, "calls": [...]}. A "long_window" / "cloud"
# entry draws its calls in order from one rng (as tests/test_chain.py does with the same seeds).
SETS = {
    # chain_rows' 64-anchor ring edge, k_first's chunk edge, k_reorder's ranking vs its sort
    "rank": {"pad_seed": 101, "calls": [_strided(D=D, per=40) for D in (63, 64, 65)]},
    # kLdsW; bitonic padding at a power of two
    "ldsw": {"pad_seed": 102, "calls": [_strided(D=D) for D in (2047, 2048, 2049)]},
    # kParentWindow / kMaxIter from inside, on the edge and from outside
    "window": {"pad_seed": 103, "calls": [_strided(D=D) for D in (4999, 5000, 5001)]},
    # kLdsCtr: 8191 / 8192 / 8193 ends at (1,0)
    "ldsctr": {"pad_seed": 104, "calls": [_strided(D=4095, segs=2, extras=1), _strided(D=4096, segs=2, extras=0),
                                          _strided(D=4096, segs=2, extras=1)]},
    # dr == max_dist_x kept, + 1 dropped; kRingSmall (i - st = 1024 / 1025); params other than 5000/5000
    "xstep": {"pad_seed": 105, "calls": [_strided(D=1024, xstep=4, params=[4096, 4096, 500, 1]),
                                         _strided(D=1025, xstep=4, params=[4096, 4096, 500, 1]),
                                         _strided(D=1025, xstep=4, params=[4100, 4100, 500, 1]),
                                         _strided(D=1026, xstep=4, params=[4100, 4100, 500, 1])]},
    # ksort's tie order on the global-memory path
    "twins": {"pad_seed": 106, "calls": [_strided(D=D, twins=True) for D in (2500, 2501)]},
    # irregular trees with far parents
    "long_window": {"pad_seed": 107, "calls": [{"kind": "long_window", "seed": 5,
                                                 "args": [[9000, 0.05], [7000, 0.3], [3000, 0.8]]}]},
    # duplicate peaks, branches, ties
    "cloud": {"pad_seed": 108, "calls": [{"kind": "cloud", "seed": 91,
                                           "args": [[14000, 24, 2000, [0, 1], 40], [8000, 3, 100, [0, 3], 2],
                                                    [6000, 40, 4000, [0, 1], 200]]}]},
}
STRIDED_SETS = [k for k, s in SETS.items() if s["calls"][0]["kind"] == "strided"]
IRREGULAR_SETS = [k for k in SETS if k not in STRIDED_SETS]


def special_calls(spec):
    """The special calls of one set description, each a one-call ChainCalls."""
    out = []
    for e in spec["calls"]:
        if e["kind"] == "strided":
            kw = dict(e["args"])
            if "params" in kw:
                kw["params"] = tuple(kw["params"])
            out.append(strided_call(**kw))
        elif e["kind"] == "long_window":
            rng = np.random.default_rng(e["seed"])
            out.extend(_long_window_call(rng, n, frac) for n, frac in e["args"])
        elif e["kind"] == "cloud":
            rng = np.random.default_rng(e["seed"])
            out.extend(_cloud_call(rng, n, d, spread, tuple(step), noise) for n, d, spread, step, noise in e["args"])
        else:
            raise ValueError(e["kind"])
    return out


def build_set(spec):
    """-> (calls, special): ordinary, special 0, ordinary, special 1, ..., ordinary; `special` lists
    the call indices of the special calls (1, 3, ...)."""
    rng = np.random.default_rng(spec["pad_seed"])
    parts = [ordinary_call(rng)]
    for s in special_calls(spec):
        parts += [s, ordinary_call(rng)]
    return _concat_calls(parts), list(range(1, len(parts), 2))


def pack_dp(offsets, scores, parents, targets, peaks):
    """The DP outputs in the form the fixture stores (far smaller once compressed; exact both ways):
    parents and targets as distances from their own index (0: none -- a parent lies before its
    anchor and a target mark after it, so a true distance is never 0), peaks as peak - score."""
    i = np.arange(len(scores), dtype=np.int64) - np.repeat(offsets[:-1], np.diff(offsets))
    p, t = np.asarray(parents, np.int64), np.asarray(targets, np.int64)
    assert (p < i).all() and ((t == 0) | (t > i)).all()
    return (np.asarray(scores, np.int32), np.where(p >= 0, i - p, 0).astype(np.int32),
            np.where(t != 0, t - i, 0).astype(np.int32), (np.asarray(peaks, np.int64) - scores).astype(np.int32))


def unpack_dp(offsets, scores, dparent, dtarget, dpeak):
    i = np.arange(len(scores), dtype=np.int64) - np.repeat(offsets[:-1], np.diff(offsets))
    return [np.asarray(scores, np.int32), np.where(dparent != 0, i - dparent, -1).astype(np.int32),
            np.where(dtarget != 0, i + dtarget, 0).astype(np.int32), (scores.astype(np.int64) + dpeak).astype(np.int32)]


def chains_at_min_sc(calls, p, us, anchors, min_sc):
    """Per call: the kept chains whose score equals min_sc and whose first anchor has a parent -- chains
    that stopped on a node claimed earlier and passed `f[start] - f[stop] >= min_sc` at equality."""
    out = []
    for c in range(calls.ncalls):
        o0, o1 = int(calls.offsets[c]), int(calls.offsets[c + 1])
        where = {}
        for i, k in enumerate(zip(calls.x[o0:o1].tolist(), calls.y[o0:o1].tolist())):
            where.setdefault(k, []).append(i)
        lens = (us[c] & np.uint64(0xffffffff)).astype(np.int64)
        first = np.cumsum(lens) - lens
        n = 0
        for k in np.flatnonzero((us[c] >> np.uint64(32)).astype(np.int64) == min_sc):
            a = first[k]
            n += all(p[o0 + i] >= 0 for i in where[(int(anchors[c][0][a]), int(anchors[c][1][a]))])
        out.append(n)
    return out


def tree_witnesses(calls, f, p, v, us, anchors, min_sc):
    """What a set reaches, per call, from the DP outputs f / p / v and the backtrack oracle's chains
    (us, anchors) at min_sc: a list of dicts with
      ends       anchors with no child and v >= min_sc,
      kept       kept chains,
      dup_peaks  ends that share their peak with another end,
      tied_x     kept chains whose first anchor's x another kept chain's first anchor has too,
      max_dist   max(i - p[i]) over anchors with a parent (0 if none),
      branches   nodes with more than one child."""
    out = []
    for c in range(calls.ncalls):
        o0, o1 = int(calls.offsets[c]), int(calls.offsets[c + 1])
        fc, pc, vc = (np.asarray(a[o0:o1], np.int64) for a in (f, p, v))
        n = o1 - o0
        has = pc >= 0
        nchild = np.bincount(pc[has], minlength=n)
        ends = np.flatnonzero((nchild == 0) & (vc >= min_sc))
        # every end to the peak of its parent path (testbed chain.c:150-158)
        j = ends.copy()
        while True:
            mv = (j >= 0) & (fc[np.maximum(j, 0)] < vc[np.maximum(j, 0)])
            if not mv.any():
                break
            j[mv] = pc[j[mv]]
        j = np.where(j < 0, ends, j)
        _, inv, cnt = np.unique(j, return_inverse=True, return_counts=True)
        dup = int((cnt[inv] > 1).sum()) if len(j) else 0
        lens = (us[c] & np.uint64(0xffffffff)).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
        fx = anchors[c][0][first]
        _, inv, cnt = np.unique(fx, return_inverse=True, return_counts=True)
        tied = int((cnt[inv] > 1).sum()) if len(fx) else 0
        idx = np.flatnonzero(has)
        out.append({"ends": len(ends), "kept": len(us[c]), "dup_peaks": dup, "tied_x": tied,
                    "max_dist": int((idx - pc[idx]).max()) if len(idx) else 0,
                    "branches": int((nchild > 1).sum())})
    return out
