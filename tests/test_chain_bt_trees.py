"""Chain backtrack (csrc/chain_bt.hip) and chain_dp on far-parent trees and at every size class.

The generator-shaped calls of test_chain_bt.py / test_edges.py never put a parent more than 42
anchors behind its child and enter the classes above kRsMin (64) / kLdsW (2048) / kLdsCtr (8192) by
accident. The sets of tests/chain_shapes.py put calls on each boundary and one step past it
(kParentWindow / kMaxIter 5000, kLdsCtr 8192 ends, kLdsW 2048 and kRsMin 64 kept chains, kRingSmall
1024, chain_rows' 64-anchor ring), tie first-x keys on the global-memory reorder, test the acceptance
rule at equality, and add the irregular far-parent / duplicate-peak trees of test_chain.py.

CPU: the witnesses (what each set reaches, asserted so that an edit of a generator cannot hollow
the GPU tests out), the C oracle against the live reference and against its record in
tests/golden/chain_bt_trees_golden.npz. GPU: backtrack and DP bit-exact against the oracle and the
record, per set, plus every strided call shuffled into one batch."""
import functools
import json
import os

import numpy as np
import pytest

import chain_shapes as cs
import oracle_lib
from conftest import GOLDEN
from test_chain import assert_same
from test_chain_bt import gpu_chains, same_chains

SET_NAMES = list(cs.SETS)


@functools.lru_cache(maxsize=None)
def built(name):
    """-> (calls, special call indices, oracle DP outputs, {threshold pair: (us, anchors)}); computed
    once per session and never modified."""
    calls, special = cs.build_set(cs.SETS[name])
    dp = oracle_lib.chain_oracle(calls, 8)
    for a in dp[:4]:
        a.setflags(write=False)
    bt = {}
    for mc, ms in cs.THRESHOLDS:
        _, us, an = oracle_lib.chain_bt_oracle(calls, dp[0], dp[1], dp[3], mc, ms, 8)
        bt[(mc, ms)] = (us, an)
    return calls, special, dp, bt


def witnesses(name, thr):
    calls, special, dp, bt = built(name)
    w = cs.tree_witnesses(calls, dp[0], dp[1], dp[3], *bt[thr], thr[1])
    return [w[c] for c in special]


def wit(ends, kept, max_dist, tied_x=0):
    return {"ends": ends, "kept": kept, "dup_peaks": 0, "tied_x": tied_x, "max_dist": max_dist, "branches": 0}


# ---- CPU ---------------------------------------------------------------------------------------------

def test_strided_call_shape():
    """The construction itself: anchor counts, sorted x, and the one admissible predecessor D back."""
    c = cs.strided_call(7, per=3, segs=2, extras=2, xstep=4, twins=True)
    assert c.nanchors == 2 * 7 * 3 * 2 + 2 and (np.diff(c.x.astype(np.int64)) >= 0).all()
    assert (c.x[0:-2:2] == c.x[1:-2:2]).all() and c.avg_qspan[0] == 15.0
    f, p, _, v, _ = oracle_lib.chain_oracle(c)
    i = np.arange(c.nanchors)
    main = i < 2 * 7 * 3 * 2
    first = (i // 2) % (7 * 3) < 7  # the first anchor of each chain
    assert (p[main & ~first] == i[main & ~first] - 14).all() and (p[~main | first] == -1).all()
    assert f.max() == 45 and (f[~main] == 15).all()


@pytest.mark.parametrize("name,D", [("rank", (63, 64, 65)), ("ldsw", (2047, 2048, 2049))])
def test_witness_kept_chain_classes(name, D):
    """k_reorder's three paths: 63 / 64 kept chains rank on 64 lanes, 65 .. 2048 sort in LDS (2047 padded
    to 2048, 2048 unpadded), 2049 replays ksort in global memory; parent links of 63 / 64 / 65 sit on
    chain_rows' 64-anchor ring edge and k_first's chunk edge."""
    assert witnesses(name, (3, 40)) == [wit(d, d, d) for d in D]
    assert witnesses(name, (1, 0)) == [wit(d, d, d) for d in D]
    if name == "ldsw":
        thresholds_at_equality(name, D, D)


def thresholds_at_equality(name, chains, dist, tied=False):
    """A per = 3 chain has 3 anchors and scores 45: kept at (3,45), no ends at (3,46), ends but no chain at
    (4,40)."""
    assert witnesses(name, (3, 45)) == [wit(n, n, d, tied_x=n if tied else 0) for n, d in zip(chains, dist)]
    assert witnesses(name, (3, 46)) == [wit(0, 0, d) for d in dist]
    assert witnesses(name, (4, 40)) == [wit(n, 0, d) for n, d in zip(chains, dist)]


def test_witness_parent_window():
    """kParentWindow / kMaxIter: parents 4999 and 5000 back are found; 5001 back is outside the DP's window,
    so that call has no chain at all (15 003 single-anchor chains at (1,0))."""
    assert witnesses("window", (3, 40)) == [wit(4999, 4999, 4999), wit(5000, 5000, 5000), wit(0, 0, 0)]
    assert witnesses("window", (1, 0)) == [wit(4999, 4999, 4999), wit(5000, 5000, 5000), wit(15003, 15003, 0)]
    thresholds_at_equality("window", (4999, 5000, 0), (4999, 5000, 0))


def test_witness_lds_counters():
    """kLdsCtr: 8191 / 8192 ends keep k_place's counters in LDS, 8193 takes the global atomics."""
    assert witnesses("ldsctr", (1, 0)) == [wit(8191, 8191, 4095), wit(8192, 8192, 4096), wit(8193, 8193, 4096)]
    assert witnesses("ldsctr", (3, 40)) == [wit(8190, 8190, 4095), wit(8192, 8192, 4096), wit(8192, 8192, 4096)]
    thresholds_at_equality("ldsctr", (8190, 8192, 8192), (4095, 4096, 4096))


def test_witness_max_dist_and_small_ring():
    """dr == max_dist_x is kept and max_dist_x + 1 is dropped, under 4096 and 4100 (not the 5000 every other
    big test uses); the windows hold i - st = 1024 / 1025 anchors, either side of kRingSmall."""
    assert witnesses("xstep", (3, 40)) == [wit(1024, 1024, 1024), wit(0, 0, 0), wit(1025, 1025, 1025), wit(0, 0, 0)]
    assert witnesses("xstep", (1, 0)) == [wit(1024, 1024, 1024), wit(3075, 3075, 0), wit(1025, 1025, 1025),
                                          wit(3078, 3078, 0)]
    thresholds_at_equality("xstep", (1024, 0, 1025, 0), (1024, 0, 1025, 0))
    calls, special, _, _ = built("xstep")
    win = []
    for c in special:  # the widest window, as the reference's loop walks st
        x = calls.x[calls.offsets[c]:calls.offsets[c + 1]].astype(np.int64)
        st = np.searchsorted(x, x - int(calls.params4[c][0]), side="left")
        win.append(int((np.arange(len(x)) - st).max()))
    assert win == [1024, 1024, 1025, 1025]


def test_witness_tied_keys_global_reorder():
    """twins: 5000 kept chains (> kLdsW, the global-memory replay of ksort) in 2500 pairs of equal first x;
    parents 2 * 2500 back; with 2 * 2501 no chain forms and (1,0) keeps 15 006 singles in 7 503 tied pairs."""
    assert witnesses("twins", (3, 40)) == [wit(5000, 5000, 5000, tied_x=5000), wit(0, 0, 0)]
    assert witnesses("twins", (1, 0)) == [wit(5000, 5000, 5000, tied_x=5000), wit(15006, 15006, 0, tied_x=15006)]
    thresholds_at_equality("twins", (5000, 0), (5000, 0), tied=True)


def test_witness_irregular_trees():
    """Floors, not equalities (the generators are random): far parents on the long-window calls; duplicate
    peaks, branch nodes and tied keys on the clouds; more than 64 kept chains (the sort, not the ranking)
    on both."""
    lw, cl = witnesses("long_window", (3, 40)), witnesses("cloud", (3, 40))
    assert max(w["max_dist"] for w in lw) >= 4900
    assert max(w["kept"] for w in lw) > 64 and max(w["kept"] for w in cl) > 64
    assert max(w["dup_peaks"] for w in cl) >= 1000
    assert max(w["branches"] for w in cl) >= 3000
    assert max(w["max_dist"] for w in cl) >= 1000
    assert max(w["tied_x"] for w in witnesses("cloud", (1, 0))) >= 1000
    assert max(w["kept"] for w in witnesses("long_window", (1, 0))) > 2048  # tied keys past kLdsW too
    assert max(w["tied_x"] for w in witnesses("long_window", (1, 0))) > 0


def test_witness_score_rule_at_equality():
    """The strided chains end at a root, where only `len >= min_cnt` and the ends' `v >= min_sc` decide (both at
    equality under (3,45)). The other branch, `f[start] - f[stop] >= min_sc` for a chain that stopped on a
    claimed node, is met at equality on the clouds."""
    calls, special, dp, bt = built("cloud")
    for thr in [(3, 40), (3, 45)]:
        n = cs.chains_at_min_sc(calls, dp[1], *bt[thr], thr[1])
        assert sum(n[c] for c in special) >= 1, thr


def test_no_call_at_offset_zero_and_sizes():
    for name in SET_NAMES:
        calls, special, _, _ = built(name)
        n = np.diff(calls.offsets)
        assert special[0] == 1 and special[-1] == calls.ncalls - 2 and n.max() <= 25000
        assert all(500 <= n[c] <= 700 for c in range(calls.ncalls) if c not in special)


@pytest.mark.parametrize("name", SET_NAMES)
def test_oracle_vs_reference_live(name):
    dp_lib, bt_lib = oracle_lib.ref_chain(), oracle_lib.ref_chain_bt()
    if dp_lib is None or bt_lib is None:
        pytest.skip("oracle/_ref not built (needs the reference tree)")
    calls, _, dp, bt = built(name)
    assert_same(dp[:4], oracle_lib.ref_chain_run(dp_lib, calls, 8))
    for mc, ms in cs.THRESHOLDS:
        rus, ran = oracle_lib.ref_chain_bt_run(bt_lib, calls, mc, ms)
        same_chains(calls, *bt[(mc, ms)], rus, ran)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """The live reference's record for one set -> (calls, recorded mask per call, DP outputs over the
    recorded calls, {threshold pair: (us, anchors)}), rebuilt from the generator arguments it stores."""
    z = np.load(os.path.join(GOLDEN, "chain_bt_trees_golden.npz"))
    calls, special = cs.build_set(json.loads(str(z["spec"]))[name])
    keep = np.ones(calls.ncalls, bool)
    for s, k in json.loads(str(z["dropped"])):
        if s == name:
            keep[special[k]] = False
    n = np.where(keep, np.diff(calls.offsets), 0)
    dp = cs.unpack_dp(np.concatenate([[0], np.cumsum(n)]), *[z["%s_%s" % (name, k)] for k in
                                                             ("scores", "dparent", "dtarget", "dpeak")])
    bt = {}
    for k, (mc, ms) in enumerate(z["thresholds"].tolist()):
        nch, nan = z["%s_nch%d" % (name, k)], z["%s_nan%d" % (name, k)]
        cu, ca = np.concatenate([[0], np.cumsum(nch)]), np.concatenate([[0], np.cumsum(nan)])
        u, ai = z["%s_u%d" % (name, k)], np.cumsum(z["%s_dai%d" % (name, k)], dtype=np.int64)
        us, an = [], []
        for c in range(calls.ncalls):
            idx = int(calls.offsets[c]) + ai[ca[c]:ca[c + 1]]
            us.append(u[cu[c]:cu[c + 1]])
            an.append((calls.x[idx], calls.y[idx]))
        bt[(mc, ms)] = (us, an)
    return calls, keep, dp, bt


def same_recorded_chains(calls, keep, got_us, got_an, exp_us, exp_an):
    """same_chains on the recorded calls (an unrecorded call's slot in the record is empty)."""
    us = [u if keep[c] else exp_us[c] for c, u in enumerate(got_us)]
    an = [a if keep[c] else exp_an[c] for c, a in enumerate(got_an)]
    same_chains(calls, us, an, exp_us, exp_an)


@pytest.mark.parametrize("name", SET_NAMES)
def test_oracle_vs_fixture(name):
    calls, _, dp, bt = built(name)
    rcalls, keep, rdp, rbt = recorded(name)
    assert cs.SETS[name] == json.loads(json.dumps(cs.SETS[name]))  # the description survives JSON
    for a, b in ((calls.offsets, rcalls.offsets), (calls.x, rcalls.x), (calls.y, rcalls.y)):
        assert np.array_equal(a, b), "the record was made for other generator arguments"
    amask = np.repeat(keep, np.diff(calls.offsets))
    assert_same([a[amask] for a in dp[:4]], rdp)
    assert sorted(rbt) == sorted(cs.THRESHOLDS)
    for thr in cs.THRESHOLDS:
        same_recorded_chains(calls, keep, *bt[thr], *rbt[thr])
    # every case on a boundary or one step past it is in the record
    droppable = {("ldsw", 0), ("window", 0), ("cloud", 1)}
    _, special, _, _ = built(name)
    assert all(keep[c] or (name, special.index(c)) in droppable for c in range(calls.ncalls))


# ---- GPU ---------------------------------------------------------------------------------------------

def check_backtrack(b, calls, expected):
    """backtrack at every threshold pair on the same buffers; expected: [{pair: (us, anchors)}, keep or None]."""
    for mc, ms in cs.THRESHOLDS:
        b.backtrack(mc, ms)
        gus, gan = gpu_chains(b, calls)  # also checks tc and ta against the sums
        for bt, keep in expected:
            if keep is None:
                same_chains(calls, gus, gan, *bt[(mc, ms)])
            else:
                same_recorded_chains(calls, keep, gus, gan, *bt[(mc, ms)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_backtrack(name):
    """run(), then backtrack at each threshold pair on the same buffers: chains and anchors bit-exact
    against the oracle and against the live reference's record."""
    from genomicsbench_palisade_amd import chain, set_device
    set_device(0)
    calls, _, dp, bt = built(name)
    _, keep, _, rbt = recorded(name)
    b = chain.ChainBatch(calls)
    b.run()
    got = b.results()
    assert_same(got, dp)
    assert got[4] == dp[4]
    check_backtrack(b, calls, [(bt, None), (rbt, keep)])
    b.close()


@pytest.mark.gpu
def test_gpu_backtrack_all_strided_shuffled():
    """Every strided call in one batch, in shuffled order: the per-call scratch slices and the eoff / kidx /
    aoff scans run across calls of every class in one launch."""
    from genomicsbench_palisade_amd import chain, set_device
    from test_chain import _concat_calls
    set_device(0)
    src = [(name, c) for name in cs.STRIDED_SETS for c in built(name)[1]]
    order = np.random.default_rng(7).permutation(len(src))
    parts, bt = [], {thr: ([], []) for thr in cs.THRESHOLDS}
    for k in order:
        name, c = src[k]
        calls, _, _, sbt = built(name)
        parts.append(calls.slice(c, c + 1))
        for thr in cs.THRESHOLDS:
            bt[thr][0].append(sbt[thr][0][c])
            bt[thr][1].append(sbt[thr][1][c])
    calls = _concat_calls(parts)
    b = chain.ChainBatch(calls)
    b.run()
    check_backtrack(b, calls, [(bt, None)])
    b.close()


# rows, GB_CHAIN_SPLIT, GB_CHAIN_SPLIT_FAULT, GB_CHAIN_VLANES
DP_CONFIGS = [("1", "", 0, None), ("0", "", 0, None), ("1", "0", 0, None), ("1", "64,0", 0, None),
              ("1", "128,8", 37, None), ("1", "-1,128,0,5000", 0, None), ("1", "", 0, "0")]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,split,fault,vlanes", DP_CONFIGS)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_dp(name, rows, split, fault, vlanes, monkeypatch):
    """chain_dp on the same sets: scores, parents, targets, peaks and visited counts against the oracle on
    chain_rows and on chain_kernel, whole and as speculative segments (a segment cannot see a parent that
    lies up to 5000 anchors before its warm-up, so these calls live on verification and fix-up), with
    injected wrong guesses, the uncapped window, and wave verification."""
    from genomicsbench_palisade_amd import chain, set_device
    set_device(0)
    calls, _, dp, _ = built(name)
    monkeypatch.setenv("GB_CHAIN_ROWS", rows)
    monkeypatch.setenv("GB_CHAIN_SPLIT", split)
    monkeypatch.setenv("GB_CHAIN_SPLIT_FAULT", str(fault))
    if split:
        monkeypatch.setenv("GB_CHAIN_TARGET", "0")  # equal segments of GB_CHAIN_SPLIT's length, as test_gpu_split_exact
    if vlanes is not None:
        monkeypatch.setenv("GB_CHAIN_VLANES", vlanes)
    b = chain.ChainBatch(calls)
    b.run()
    got = b.results()
    assert_same(got, dp)
    assert got[4] == dp[4]
    b.close()
