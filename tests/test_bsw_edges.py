"""The extension kernels of csrc/bsw.hip (pair-per-lane bsw_lane_kernel<NCH, SYM>, wave-per-pair
extend<K>) at their layout edges and under odd scoring, bit for bit against bwa v1 ksw_extend2
(tests/golden/bsw_edges_golden.npz, written by tests/golden/make_bsw_edges_golden.py from the sets of
tests/bsw_edges.py).

CPU: the restatement (oracle/bsw_oracle.c) equals the fixture (and ksw_extend2 live when built), the
inputs discriminate (a broken rule changes a stated share of the outputs, so no GPU test below can go
vacuous through a later edit of the lists), the sets cover what they claim, and the routing rule of
bsw_batch_plan is restated once. GPU: every parameter set on both kernels, the long and limit sets,
proof that GB_BSW_TAIL=0 really runs the lane kernels, getScores16's two paths, and a shuffled batch."""
import os
import re
import time

import numpy as np
import pytest

import bsw_edges
import oracle_lib
from genomicsbench_palisade_amd import bsw
from test_bsw import assert_same

NCHS = (4, 8, 12, 16, 20)


@pytest.fixture(scope="module")
def fx():
    return bsw_edges.Fixture()


def lane_nch(P, qlen, h0):
    """bsw_batch_plan's routing rule: NCH of the pair-per-lane kernel that takes the pair, or 0 when it
    goes to the wave-per-pair kernel. Lane-eligible iff o_del, o_ins >= 0, h0 >= 0,
    h0 + qlen * max(mat, 0) < 30000 (the 16-bit {H, E} packing) and (qlen + 8) // 8 <= 20 chunks of 8
    columns; the variant is that chunk count rounded up to a multiple of 4."""
    mx = max(int(P.mat_array().max()), 0)
    nch = (int(qlen) + 8) // 8
    if P.o_del < 0 or P.o_ins < 0 or h0 < 0 or int(h0) + int(qlen) * mx >= 30000 or nch > 20:
        return 0
    return 4 * ((nch + 3) // 4)


def lane_nchs(P, p):
    return np.array([lane_nch(P, q, h) for q, h in zip(p.qlen.tolist(), p.h0.tolist())])


# ---------------------------------------------------------------- CPU

def test_fixture_inputs_are_the_edge_sets(fx):
    """The fixture's inputs are what bsw_edges builds today (an edit of the lists needs a new fixture)."""
    sets = bsw_edges.input_sets()
    assert set(sets) == set(fx.sets)
    for s, p in sets.items():
        for k in bsw_edges.INPUT_KEYS:
            assert np.array_equal(getattr(p, k), getattr(fx.sets[s], k)), f"{s}.{k}"
    for k, P in fx.params.items():
        Q = bsw_edges.params(k)
        assert (P.as_array() == Q.as_array()).all() and (P.mat_array() == Q.mat_array()).all(), k
    assert os.path.getsize(bsw_edges.FIXTURE) <= 601912  # the largest fixture before this one


def test_oracle_vs_fixture(fx):
    assert len(bsw_edges.CASES) == 15 + 2 + 3
    for s, k in bsw_edges.CASES:
        got, cells, tot = oracle_lib.bsw_oracle(fx.sets[s], fx.params[k], nthreads=8)
        assert_same(got, fx.out[s, k], f"{s} / {k}")
        assert (cells == fx.cells[s, k]).all() and tot == fx.cells[s, k].sum()


def test_reference_live_vs_fixture(fx):
    lib = oracle_lib.ref_bsw()
    if lib is None:
        pytest.skip("oracle/_ref not built (no reference tree here)")
    for s, k in bsw_edges.CASES:
        assert_same(oracle_lib.ref_bsw_run(lib, fx.sets[s], fx.params[k]), fx.out[s, k], f"{s} / {k}")


def test_inputs_discriminate(fx):
    """Fraction of main-set pairs whose six outputs change when a rule is broken in the oracle's
    arguments; measured when the fixture was written / required here:
      asym_mat transposed                    0.513 / 0.10
      ext_mat transposed                     0.386 / 0.10
      e_only with e_ins := e_del             0.296 / 0.10
      o_only with o_ins := o_del             0.186 / 0.05
      zdrop5_asym with ins and del swapped   0.152 / 0.05
      w0 vs w1                               0.127 / 0.03
      w1 vs w2                               0.059 / 0.03
      bigext vs bigext_bonus                 outputs 0.014, cell counts 0.862 / > 0 in either
    (end_bonus enters through the band adjustment only, so it shows mostly in the cell counts)."""
    p = fx.sets["main"]
    for what, base, kw, need in bsw_edges.BROKEN_RULES:
        broken = oracle_lib.bsw_oracle(p, bsw_edges.params(base, **kw), nthreads=8)[0]
        frac = bsw_edges.changed_fraction(broken, fx.out["main", base])
        print(f"{what}: {frac:.3f}")
        assert frac >= need, f"{what}: only {frac:.3f} of the pairs change"
    fo = bsw_edges.changed_fraction(fx.out["main", "bigext"], fx.out["main", "bigext_bonus"])
    fc = float((fx.cells["main", "bigext"] != fx.cells["main", "bigext_bonus"]).mean())
    print(f"bigext vs bigext_bonus: outputs {fo:.3f}, cells {fc:.3f}")
    assert fo > 0 or fc > 0


def test_main_set_coverage(fx):
    p = fx.sets["main"]
    assert p.n == len(bsw_edges.MAIN_QLENS) * len(bsw_edges.MAIN_TLENS) * len(bsw_edges.MAIN_H0S)
    assert (p.tlen < p.qlen).mean() >= 0.30
    assert (p.tlen == 0).sum() >= 25
    have = set(zip(p.qlen.tolist(), p.h0.tolist()))
    assert have == {(q, h) for q in bsw_edges.MAIN_QLENS for h in bsw_edges.MAIN_H0S}
    # every lane variant and the wave kernel's every K get pairs under the default parameters
    nch = lane_nchs(fx.params["default"], p)
    assert set(nch.tolist()) == {0, *NCHS}
    assert {(q + 64) >> 6 for q in bsw_edges.MAIN_QLENS} == {1, 2, 3, 4}
    assert p.tgt.max() == 4 and p.qry.max() == 4  # code 4 present, nothing above it


def test_routing_rule_on_the_limit_set(fx):
    """d = 0 is the last lane-eligible h0 (for the query lengths a lane kernel holds), d = 1 the first
    that must go to the wave kernel, and the reference's top score at d = 0 fits the 16-bit packing."""
    for mx in bsw_edges.LIMIT_MATCH:
        k = bsw_edges.LIMIT_PARAMS[mx]
        p, P = fx.sets[f"limit{mx}"], fx.params[k]
        assert int(P.mat_array().max()) == mx
        d = bsw_edges.limit_d(p, mx)
        assert sorted(set(d.tolist())) == sorted(bsw_edges.LIMIT_D)
        nch = lane_nchs(P, p)
        short = p.qlen < 160
        assert short.any() and (~short).any()
        assert (nch[short & (d <= 0)] > 0).all() and (nch[d >= 1] == 0).all() and (nch[~short] == 0).all()
        assert set(nch[short & (d == 0)].tolist()) == {4, 16, 20}
        top = fx.out[f"limit{mx}", k][:, 0]
        assert (top[d <= 0] < 2 ** 15).all() and (top >= p.h0).all()
        assert (p.h0 >= 0).all()


# ---------------------------------------------------------------- GPU

def _gpu(p, P):
    from genomicsbench_palisade_amd import set_device
    set_device(0)
    t0 = time.perf_counter()
    b = bsw.BswBatch(p, P)
    b.run()
    out, cells, tot = b.results()
    b.close()
    print(f"BswBatch of {p.n} pairs: {time.perf_counter() - t0:.3f} s")
    return out, cells, tot


def _check(fx, s, k, got, cells, tot, what):
    assert_same(got, fx.out[s, k], what)
    exp = fx.cells[s, k]
    assert (cells == exp).all(), f"{what}: cell counts differ on {(cells != exp).sum()} pairs"
    assert tot == exp.sum()


def _route(monkeypatch, tail):
    """tail "0": eligible pairs on the pair-per-lane kernels; None: the default routing (a batch this
    small runs on the wave-per-pair kernel)."""
    if tail is None:
        monkeypatch.delenv("GB_BSW_TAIL", raising=False)
    else:
        monkeypatch.setenv("GB_BSW_TAIL", tail)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["0", None])
@pytest.mark.parametrize("name", bsw_edges.MAIN_PARAMS)
def test_gpu_main_set(fx, monkeypatch, name, tail):
    _route(monkeypatch, tail)
    got, cells, tot = _gpu(fx.sets["main"], fx.params[name])
    _check(fx, "main", name, got, cells, tot, f"main / {name} (tail {tail})")


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["0", None])
@pytest.mark.parametrize("s,name", [c for c in bsw_edges.CASES if c[0] != "main"])
def test_gpu_long_and_limit_sets(fx, monkeypatch, s, name, tail):
    _route(monkeypatch, tail)
    got, cells, tot = _gpu(fx.sets[s], fx.params[name])
    _check(fx, s, name, got, cells, tot, f"{s} / {name} (tail {tail})")


PROF_LINE = re.compile(r"\[bsw prof\] NCH=(\d+) pairs (\d+):.*\(cells (\d+) /")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "asym_mat", "e_only"])
def test_gpu_tail0_runs_the_lane_kernels(fx, monkeypatch, capfd, name):
    """Under GB_BSW_TAIL=0 every lane-eligible pair of the main set runs on its lane variant: the
    kernels' own counters (GB_BSW_PROF=1) report, per NCH, the pair count the routing rule gives and
    the cells the oracle counts for those pairs. SYM follows the gap costs alone (o_del == o_ins and
    e_del == e_ins): default and asym_mat count the SYM = true instantiations (asym_mat under the
    asymmetric score table), e_only the SYM = false ones."""
    monkeypatch.setenv("GB_BSW_TAIL", "0")
    monkeypatch.setenv("GB_BSW_PROF", "1")
    p, P = fx.sets["main"], fx.params[name]
    capfd.readouterr()
    got, cells, tot = _gpu(p, P)
    err = capfd.readouterr().err
    _check(fx, "main", name, got, cells, tot, f"main / {name} (prof)")
    seen = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in PROF_LINE.finditer(err)}
    nch = lane_nchs(P, p)
    exp = {n: (int((nch == n).sum()), int(fx.cells["main", name][nch == n].sum())) for n in NCHS}
    assert all(v[0] > 0 and v[1] > 0 for v in exp.values())
    assert seen == exp, err


@pytest.mark.gpu
@pytest.mark.parametrize("limit", ["0", "100000000"])
def test_gpu_get_scores16_paths(fx, monkeypatch, limit):
    """getScores16's batch launch (GB_BSW_SMALL=0) and its small-call path (every pair on the
    wave-per-pair kernel, sequences repacked on the host) on the main set."""
    from genomicsbench_palisade_amd import set_device
    set_device(0)
    monkeypatch.setenv("GB_BSW_SMALL", limit)
    p = fx.sets["main"]
    for name in ("e_only", "asym_mat", "w0"):
        t0 = time.perf_counter()
        sp = bsw.get_scores16(p, fx.params[name])
        print(f"get_scores16 {name}: {time.perf_counter() - t0:.3f} s")
        assert_same(np.stack([sp[f] for f in bsw.OUT_FIELDS], axis=1), fx.out["main", name],
                    f"get_scores16 {name} (limit {limit})")


@pytest.mark.gpu
def test_gpu_shuffled_main_set_in_mixed_waves(fx, monkeypatch):
    """The main set in a fixed random order, grouped by variant and 64-column query step only (no h0
    step), on the lane kernels under zdrop5_asym: the lanes of one wave hold very different qlen, tlen
    and h0, and every result lands at its pair's own index."""
    monkeypatch.setenv("GB_BSW_H0STEP", "0")
    monkeypatch.setenv("GB_BSW_QSHIFT", "6")
    monkeypatch.setenv("GB_BSW_TAIL", "0")
    perm = np.random.default_rng(5).permutation(fx.sets["main"].n)
    p = fx.sets["main"].subset(perm)
    got, cells, tot = _gpu(p, fx.params["zdrop5_asym"])
    assert_same(got, fx.out["main", "zdrop5_asym"][perm], "shuffled main / zdrop5_asym")
    exp = fx.cells["main", "zdrop5_asym"][perm]
    assert (cells == exp).all() and tot == exp.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["0", None])
def test_gpu_empty_targets_only(fx, monkeypatch, tail):
    """A batch whose every target is empty has a target buffer of no bytes at all (each pair's offset
    is the buffer's end): score h0, no cells, and no kernel has a target byte to read."""
    _route(monkeypatch, tail)
    idx = np.nonzero(fx.sets["main"].tlen == 0)[0]
    p = fx.sets["main"].subset(idx)
    assert p.n >= 25 and len(p.tgt) == 0
    got, cells, tot = _gpu(p, fx.params["default"])
    exp = fx.out["main", "default"][idx]
    assert (exp == np.stack([p.h0, 0 * p.h0, 0 * p.h0, 0 * p.h0, 0 * p.h0 - 1, 0 * p.h0], axis=1)).all()
    assert_same(got, exp, f"empty targets (tail {tail})")
    assert (cells == 0).all() and tot == 0
