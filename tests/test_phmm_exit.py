"""The f32 pass's early exit (csrc/phmm.hip phmm_stack, "Early exit") against testcases whose
probability mass falls far below MIN_ACCEPTED and then GROWS back above it (traps: rows whose
outflow of a state exceeds 1, which the reference accepts and answers from its f32 result), and
against controls of the same shape whose mass stays down (the exit must still drop them).
Fixture: tests/golden/phmm_exit_golden.npz, the reference GKL kernels' outputs
(tests/golden/make_phmm_exit_golden.py). CPU: the oracle and the live reference against the
fixture, and the fixture's trap / control conditions re-derived. GPU: the HIP path bit-exact on the
fixture alone, stacked at shifting stripe offsets, with the exit off, through the GKL entry point,
and the exit's own statistics."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
from conftest import GOLDEN, ROOT, assert_phmm_exact, bits
from genomicsbench_palisade_amd._tc import TestcaseArray

MIN_ACCEPTED = np.float32(1e-28)
FILLER_LENS = (1, 17, 30, 45, 61)


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_phmm_exit_golden",
                                                  os.path.join(GOLDEN, "make_phmm_exit_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def maker():
    return _load_generator()


@pytest.fixture(scope="module")
def cases(maker):
    cs = maker.load()
    kinds = [c["kind"] for c in cs]
    assert kinds.count("trap") == 7 + 32 and kinds.count("control") == 2 + 16
    assert [c["name"] for c in cs if c["named"]] == ["A", "B1", "B2", "C", "D1", "D2", "control1", "control2", "A_473"]
    return cs


def expect_of(cs):
    return (np.array([c["final"] for c in cs]), np.array([c["raw_f"] for c in cs], np.float32),
            np.array([c["raw_d"] for c in cs]))


def pairs_of(cs):
    return TestcaseArray.from_pairs([(c["read"], c["hap"]) for c in cs])


def oracle_run(ta):
    o = oracle_lib.oracle()
    out, rf, rd, ud = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n), np.zeros(ta.n, np.int32)
    o.phmm_oracle_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data,
                        ud.ctypes.data, 8)
    return out, rf, rd, ud


def assert_raw_exact(got, expect):
    for k, name in enumerate(("log10", "raw f32", "raw f64")):
        bad = np.nonzero(bits(got[k]) != bits(expect[k]))[0]
        assert len(bad) == 0, f"{name} mismatch at {bad[:10]}: {got[k][bad[:5]]} vs {expect[k][bad[:5]]}"


# ------------------------------------------------------------------------------------------ CPU


def test_oracle_equals_fixture(cases):
    """oracle/phmm_oracle.c on the fixture: finals, raw f32, raw f64 and the fallback choice are the
    reference's, bit for bit. Traps answer from f32, controls fall back."""
    exp = expect_of(cases)
    out, rf, rd, ud = oracle_run(pairs_of(cases))
    assert_raw_exact((out, rf, rd), exp)
    assert (ud.astype(bool) == (exp[1] < MIN_ACCEPTED)).all()
    trap = np.array([c["kind"] == "trap" for c in cases])
    assert not ud[trap].any() and ud[~trap].all()
    assert (exp[2][trap] == 0).all() and (exp[2][~trap] > 0).all()


def test_reference_live_equals_fixture(cases):
    """The reference GKL kernels (AVX2 and AVX-512 engines) reproduce the committed fixture."""
    ref = oracle_lib.ref_phmm()
    if ref is None:
        pytest.skip("oracle/_ref not built (no reference tree here)")
    ta, exp = pairs_of(cases), expect_of(cases)
    for eng in (256, 512):
        got = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
        ref.ref_phmm_batch(ctypes.addressof(ta.arr), ta.n, got[0].ctypes.data, got[1].ctypes.data,
                           got[2].ctypes.data, eng, 4)
        for k in range(3):
            assert (bits(got[k]) == bits(exp[k])).all(), (eng, k)


def test_named_cases_hold_their_conditions(cases, maker):
    """The named cases, re-derived with the generator's float64 replay of the crossing mass: every one
    stays below 2.5e-31 (100 x under the exit's threshold) and above 1e-35 for at least 72
    consecutive rows; every trap's reference result then does not fall back, every control's does.
    The f32 results are the ones the cases were built to reproduce."""
    table = {"A": 4.58e-19, "B1": 2.42e-21, "B2": 3.35e-21, "C": 2.62e-26, "D1": 1.46e-21, "D2": 2.91e-26,
             "control1": 6.17e-33, "control2": 2.51e-33}
    assert (maker.WINDOW_BELOW, maker.WINDOW_ROWS, maker.WINDOW_ABOVE) == (2.5e-31, 72, 1e-35)
    for c in cases:
        if not c["named"]:
            continue
        first, rows, low = maker.window(maker.replay(c["read"], c["hap"]))
        assert rows >= 72 and low >= 1e-35, (c["name"], first, rows, low)
        assert (c["raw_f"] < MIN_ACCEPTED) == (c["kind"] == "control"), c["name"]
        if c["name"] in table:
            assert abs(float(c["raw_f"]) / table[c["name"]] - 1) < 5e-3, (c["name"], c["raw_f"])


def test_random_family_floor(cases):
    """A random trap's reference f32 result is at least 1e-24, well clear of MIN_ACCEPTED; haplotypes
    are longer than the reads and 300 or 473 columns."""
    for c in cases:
        assert len(c["hap"]) in (300, 473)
        if not c["named"]:
            assert len(c["read"][0]) < len(c["hap"])
            if c["kind"] == "trap":
                assert c["raw_f"] >= 1e-24, c["name"]


# ------------------------------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def phmm():
    from genomicsbench_palisade_amd import phmm, set_device
    set_device(0)
    phmm.init_pairhmm()
    return phmm


@pytest.mark.gpu
def test_fixture_exact(phmm, cases):
    """The whole fixture in one call: finals, raw f32 of the testcases that pass MIN_ACCEPTED, raw f64
    and the fallback choice are the reference's. An exit that drops a trap answers from f64 instead."""
    got = phmm.compute_likelihoods_both(pairs_of(cases))
    bad = assert_phmm_exact(got, expect_of(cases))
    assert bad["f32_dropped"] > 0, bad  # the controls: the exit is at work in this very call


def stacked_job(cases):
    """All traps and controls of the haplotype most of them share, each behind a filler read of 1, 17,
    30, 45 or 61 rows, as one reads x [haplotype] job: (reads, hap, positions of the cases)."""
    by_hap = {}
    for c in cases:
        by_hap.setdefault(c["hap"], []).append(c)
    hap, group = max(by_hap.items(), key=lambda kv: len(kv[1]))
    assert {c["kind"] for c in group} == {"trap", "control"} and len(group) >= 8
    rng = np.random.default_rng(7)
    letter = hap[:1]
    reads, where = [], []
    for k, c in enumerate(group):
        n = FILLER_LENS[k % len(FILLER_LENS)]
        reads.append((letter * n, bytes(rng.integers(20, 41, n).astype(np.uint8)), bytes([45]) * n, bytes([45]) * n,
                      bytes([10]) * n))
        where.append(len(reads))
        reads.append(c["read"])
    return reads, hap, np.array(where), group


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_stacked_exact(phmm, cases, monkeypatch, order):
    """The traps and controls of one haplotype stacked into tall stacks behind filler reads, so that
    they start at different places in a 64-row stripe, in both orders: bit-exact against the oracle,
    whose outputs for the fixture's testcases are the stored reference outputs."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "2048")  # a job this small would get one stack per read
    reads, hap, where, group = stacked_job(cases)
    if order == "reversed":
        reads, where = reads[::-1], len(reads) - 1 - where
    ta = TestcaseArray(reads, [hap])
    exp = oracle_run(ta)
    stored = expect_of(group)
    for k in range(3):
        assert (bits(exp[k][where]) == bits(stored[k])).all()
    # first stacked row of every read (batch_fill: up to 64 testcases and 2048 rows of R + 2 a stack)
    starts, at, count = [], 0, 0
    for r in reads:
        if count == 64 or (count and at + len(r[0]) + 2 > 2048):
            at = count = 0
        starts.append(at)
        at, count = at + len(r[0]) + 2, count + 1
    offsets = {starts[k] % 64 for k in where}
    assert len(offsets) >= 8 and any(starts[k] >= 64 for k in where), offsets  # all over the stripe
    got = phmm.compute_likelihoods_both(ta)
    bad = assert_phmm_exact(got, exp)
    assert bad["f32_dropped"] > 0, bad


@pytest.mark.gpu
def test_exit_drops_no_trap(phmm, cases):
    traps = [c for c in cases if c["kind"] == "trap"]
    db = phmm.DeviceBatch(pairs_of(traps))
    try:
        db.run()
        res = db.results()
        assert db.exit_stats() == (0, 0)
        assert_phmm_exact(res[:4], expect_of(traps))
    finally:
        db.close()


@pytest.mark.gpu
def test_exit_drops_every_control(phmm, cases):
    """Controls carry only benchmark-range qualities (i, d in 40..45, c = 10, or the named control2's
    constant ones): the exit drops every one of them and skips their remaining cells."""
    ctl = [c for c in cases if c["kind"] == "control"]
    db = phmm.DeviceBatch(pairs_of(ctl))
    try:
        db.run()
        res = db.results()
        dropped, skipped = db.exit_stats()
        assert dropped == len(ctl)
        # a control alone in its stack is dropped at its second stripe boundary at the latest
        assert skipped >= sum((len(c["read"][0]) - 126) * len(c["hap"]) for c in ctl) > 0
        assert (res[1] == 0).all()
        assert_phmm_exact(res[:4], expect_of(ctl))
    finally:
        db.close()


@pytest.mark.gpu
def test_exit_off_raw_f32(phmm, cases, monkeypatch):
    """GB_PHMM_EXIT=0: every raw f32 of the fixture is the reference's, and so is
    gb_phmm_compute_f32's (computelikelihoodsfloat's path), for traps and controls alike."""
    ta, exp = pairs_of(cases), expect_of(cases)
    assert (bits(phmm.compute_f32(ta)) == bits(exp[1])).all()
    monkeypatch.setenv("GB_PHMM_EXIT", "0")
    assert_raw_exact(phmm.compute_likelihoods_both(ta), exp)


@pytest.mark.gpu
def test_gkl_entry_traps(phmm, cases):
    """The traps through libgkl_pairhmm_c.so's computelikelihoodsboth, called by its mangled name as a
    binary linked against GKL would: bit-exact finals."""
    so = ctypes.CDLL(os.path.join(ROOT, "genomicsbench_palisade_amd", "lib", "libgkl_pairhmm_c.so"))
    so._Z11initPairHMMv()
    so._Z22computelikelihoodsbothP8testcasePdi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    traps = [c for c in cases if c["kind"] == "trap"]
    ta = pairs_of(traps)
    out = np.zeros(ta.n)
    so._Z22computelikelihoodsbothP8testcasePdi(ctypes.addressof(ta.arr), out.ctypes.data, ta.n)
    assert (bits(out) == bits(expect_of(traps)[0])).all()
