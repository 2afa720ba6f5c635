"""The rolled sweep of the PairHMM stacks (csrc/phmm.hip phmm_rolled: lanes move on to the next 64
rows in groups of 16 instead of waiting for lane 63; GB_PHMM_ROLL=0 selects the fill-per-stripe
sweep) against the oracle, bit for bit, in both passes: every period class and both sides of the
path choice, every kind of row on the lanes where groups and turns meet, the early exit's decisions
and statistics, and rolled, unrolled and long-haplotype stacks in one launch."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
from conftest import GOLDEN, assert_phmm_exact, bits
from genomicsbench_palisade_amd import gen
from genomicsbench_palisade_amd._tc import TestcaseArray

pytestmark = pytest.mark.gpu

GROUP = 16  # kRollGroup
BASES = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def phmm():
    from genomicsbench_palisade_amd import phmm, set_device
    set_device(0)
    phmm.init_pairhmm()
    return phmm


def oracle_run(ta):
    o = oracle_lib.oracle()
    out, rf, rd = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
    o.phmm_oracle_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data, None, 16)
    return out, rf, rd


def assert_raw_exact(got, expect):
    for k, name in enumerate(("log10", "raw f32", "raw f64")):
        bad = np.nonzero(bits(got[k]) != bits(expect[k]))[0]
        assert len(bad) == 0, f"{name} mismatch at {bad[:10]}: {got[k][bad[:5]]} vs {expect[k][bad[:5]]}"


def random_hap(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def make_read(rng, n, hap):
    """A read of n rows with benchmark-range qualities: a mutated piece of the haplotype where it fits
    (so some testcases pass the f32 test), random bases where it does not."""
    if n <= len(hap):
        at = int(rng.integers(0, len(hap) - n + 1))
        b = np.frombuffer(hap, np.uint8)[at:at + n].copy()
        sub = rng.random(n) < 0.1
        b[sub] = BASES[rng.integers(0, 4, int(sub.sum()))]
    else:
        b = BASES[rng.integers(0, 4, n)]
    return (b.tobytes(), rng.integers(6, 41, n).astype(np.uint8).tobytes(),
            rng.integers(40, 46, n).astype(np.uint8).tobytes(), rng.integers(40, 46, n).astype(np.uint8).tobytes(),
            bytes([10]) * n)


def both_exact(phmm, monkeypatch, ta, exp=None):
    """The job with the early exit off (every raw f32) and on (what computelikelihoodsboth exposes)."""
    exp = oracle_run(ta) if exp is None else exp
    monkeypatch.setenv("GB_PHMM_EXIT", "0")
    assert_raw_exact(phmm.compute_likelihoods_both(ta), exp)
    monkeypatch.delenv("GB_PHMM_EXIT")
    assert_phmm_exact(phmm.compute_likelihoods_both(ta), exp)
    return exp


# ------------------------------------------------------------------------- 1. A/B over both passes


def test_ab_both_passes(phmm, monkeypatch):
    """Rolled against fill-per-stripe with the exit off: finals, raw f32 and raw f64 identical to each
    other and to the reference, and the f64 pass forced over every testcase identical too."""
    rng = np.random.default_rng(61)
    ta = TestcaseArray.from_batches([gen.phmm_batch(rng, 50, 20) for _ in range(4)])
    exp = oracle_run(ta)
    assert (exp[1] < 1e-28).any() and (exp[1] >= 1e-28).any()
    o = oracle_lib.oracle()
    exp64 = np.array([o.phmm_oracle_prob_f64(ctypes.addressof(ta.arr[k])) for k in range(ta.n)])
    monkeypatch.setenv("GB_PHMM_EXIT", "0")
    outs = {}
    for roll in ("0", "1"):
        monkeypatch.setenv("GB_PHMM_ROLL", roll)
        outs[roll] = phmm.compute_likelihoods_both(ta)[:3] + (phmm.compute_f64(ta),)
        assert_raw_exact(outs[roll], exp)
        assert (bits(outs[roll][3]) == bits(exp64)).all()
    for a, b in zip(outs["0"], outs["1"]):
        assert (bits(a) == bits(b)).all()


# --------------------------------------------------------- 2. period classes and the path boundary


def fit_stack(lens):
    """The longest prefix of the read lengths that batch_fill puts into one 2048-row stack."""
    out, rows = [], 0
    for n in lens:
        if len(out) == 64 or rows + n + 2 > 2048:
            break
        out.append(int(n))
        rows += n + 2
    return out


@pytest.mark.parametrize("C", list(range(60, 73)) + [473])
def test_period_classes(phmm, monkeypatch, C):
    """One haplotype length per case: every P mod 4 class, C = 63 / 64 on the two sides of the path
    choice and the LDS-limit shape. Up to 12 reads of 100-250 rows in one tall stack (at least 17
    turns), and between them four reads cut from the haplotype, whose f32 results do not underflow
    (the long reads' do at C <= 72)."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "2048")
    rng = np.random.default_rng(1000 + C)
    hap = random_hap(rng, C)
    lens = list(rng.integers(100, 251, 12))
    for k in (1, 4, 7, 10):
        lens.insert(k, int(rng.integers(30, 60)))
    lens = fit_stack(lens)
    assert len(lens) >= 10 and sum(n + 2 for n in lens) > 17 * 64
    ta = TestcaseArray([make_read(rng, n, hap) for n in lens], [hap])
    exp = both_exact(phmm, monkeypatch, ta)
    assert (exp[1] >= 1e-28).any() and (exp[1] < 1e-28).any()


# --------------------------------------------------------------------- 3. row kinds on every lane

ROW_LENS = (1, 2, 3) + tuple(range(13, 19)) + tuple(range(29, 35)) + tuple(range(61, 67))


def stack_rows_of(lens):
    """(kind, stacked row) of every row of reads stacked as batch_fill stacks them, one stack."""
    out, at = [], 0
    for n in lens:
        out += [("va", at), ("v0", at + 1), ("first", at + 2), ("last", at + n + 1)]
        at += n + 2
    return out, at


def test_row_kinds_on_every_lane(phmm, monkeypatch):
    """Tall stacks over C = 100 whose read lengths cycle through 1-3, 13-18, 29-34 and 61-66 rows (in
    five orders), so that va, v0, first and last rows each land on lanes 0, G - 1, G, 2G - 1, 2G, 3G - 1
    and 63, reads of one row included (the last row directly under v0); a stack
    whose last turn is a single row and one whose rows are an exact multiple of 64."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "2048")
    rng = np.random.default_rng(67)
    batches, on_lane = [], {}
    for order in range(5):
        lens = fit_stack(list(np.roll(ROW_LENS, 5 * order)) * 4)
        if order >= 2:
            lens = [int(n) for n in np.random.default_rng(order).permutation(lens)]
        rows, total = stack_rows_of(lens)
        assert total > 1900
        for kind, g in rows:
            on_lane.setdefault(kind, set()).add(g % 64)
        hap = random_hap(rng, 100)
        batches.append(gen.PhmmBatch([make_read(rng, n, hap) for n in lens], [hap]))
    for kind in ("va", "v0", "first", "last"):
        need = {0, GROUP - 1, GROUP, 2 * GROUP - 1, 2 * GROUP, 3 * GROUP - 1, 63}
        assert need <= on_lane[kind], (kind, sorted(need - on_lane[kind]))
    for lens in ((62, 62, 62, 62, 60, 1), (62,) * 5):  # 5 turns + 1 row; exactly 5 turns
        total = sum(n + 2 for n in lens)
        assert total % 64 == (1 if len(lens) == 6 else 0)
        hap = random_hap(rng, 100)
        batches.append(gen.PhmmBatch([make_read(rng, n, hap) for n in lens], [hap]))
    both_exact(phmm, monkeypatch, TestcaseArray.from_batches(batches))


# ------------------------------------------------------------------------------------ 4. early exit


@pytest.fixture(scope="module")
def exit_cases():
    spec = importlib.util.spec_from_file_location("make_phmm_exit_golden",
                                                  os.path.join(GOLDEN, "make_phmm_exit_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load()


def expect_of(cs):
    return (np.array([c["final"] for c in cs]), np.array([c["raw_f"] for c in cs], np.float32),
            np.array([c["raw_d"] for c in cs]))


def exit_run(phmm, monkeypatch, ta, roll):
    monkeypatch.setenv("GB_PHMM_ROLL", roll)
    db = phmm.DeviceBatch(ta)
    try:
        db.run()
        return db.results()[:4], db.exit_stats()
    finally:
        db.close()


def assert_same_exit(phmm, monkeypatch, ta, exp):
    """Fill-per-stripe and rolled: the same exit statistics, the same testcases dropped, exact finals."""
    (r0, s0), (r1, s1) = (exit_run(phmm, monkeypatch, ta, roll) for roll in ("0", "1"))
    print("exit_stats fill-per-stripe", s0, "rolled", s1)
    assert s0 == s1
    assert ((r0[1] == 0) == (r1[1] == 0)).all()
    assert_phmm_exact(r0, exp)
    assert_phmm_exact(r1, exp)
    return s1


@pytest.fixture(scope="module")
def seed43_job():
    rng = np.random.default_rng(43)
    ta = TestcaseArray.from_batches([gen.phmm_batch(rng, 64, 32) for _ in range(4)])
    return ta, oracle_run(ta)


@pytest.mark.parametrize("stack_rows", ["", "2048"])
def test_exit_same_decisions(phmm, monkeypatch, seed43_job, stack_rows):
    """The job of test_early_exit_drops_and_stays_exact at its own stack height and in 2048-row stacks."""
    if stack_rows:
        monkeypatch.setenv("GB_PHMM_STACK_ROWS", stack_rows)
    ta, exp = seed43_job
    dropped, skipped = assert_same_exit(phmm, monkeypatch, ta, exp)
    assert dropped > 0 and skipped > 0


def test_exit_controls_and_traps(phmm, monkeypatch, exit_cases):
    """The fixture's controls (every one dropped) and traps (none dropped), together and traps alone."""
    pairs = lambda cs: TestcaseArray.from_pairs([(c["read"], c["hap"]) for c in cs])
    ctl = [c for c in exit_cases if c["kind"] == "control"]
    traps = [c for c in exit_cases if c["kind"] == "trap"]
    dropped, _ = assert_same_exit(phmm, monkeypatch, pairs(exit_cases), expect_of(exit_cases))
    assert dropped == len(ctl)
    assert assert_same_exit(phmm, monkeypatch, pairs(traps), expect_of(traps)) == (0, 0)


# ---------------------------------------------------------------------------------- 5. mixed stacks


def test_mixed_stacks(phmm, monkeypatch):
    """C = 40 (fill per stripe), C = 300 (rolled) and C = 9 401 (records in global memory) in one batch."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "2048")
    rng = np.random.default_rng(71)
    haps = [random_hap(rng, C) for C in (40, 300, 9401)]
    reads = [make_read(rng, int(rng.integers(100, 251)), haps[1]) for _ in range(6)]
    both_exact(phmm, monkeypatch, TestcaseArray(reads, haps))
