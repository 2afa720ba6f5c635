"""The PairHMM fallback predictor (csrc/phmm.hip phmm_predict / phmm_verify and the redo launch): testcases
predicted to fall below MIN_ACCEPTED skip the f32 pass; the f64 result and the read's certificate confirm
the prediction, or the f32 result is computed after all. CPU: the certificate's bound against the oracle and
the near-threshold fixture. GPU: the device's decisions against the numpy restatement
(tests/phmm_predict_ref.py), outputs against the oracle under GB_PHMM_PREDICT unset / 0 / all and both
sweeps, the redo path, the early-exit fixture, compaction at the stack's edges, and the gate."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
import phmm_predict_ref as ref
from conftest import GOLDEN, assert_phmm_exact, bits
from genomicsbench_palisade_amd import gen
from genomicsbench_palisade_amd._tc import TestcaseArray

MIN_ACCEPTED = np.float32(1e-28)
BASES = np.frombuffer(b"ACGT", np.uint8)


def _golden_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def oracle_run(ta):
    o = oracle_lib.oracle()
    out, rf, rd = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
    o.phmm_oracle_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data, None, 16)
    return out, rf, rd


def quals(n, q=40):
    return (bytes([q]) * n, bytes([45]) * n, bytes([45]) * n, bytes([10]) * n)


@pytest.fixture(scope="module")
def exit_cases():
    return _golden_module("make_phmm_exit_golden").load()


@pytest.fixture(scope="module")
def near_pairs():
    return _golden_module("make_phmm_near_golden").load()


@pytest.fixture(scope="module")
def seed43_job():
    """The job of test_phmm_roll.py's exit tests: 4 batches of 64 reads x 32 haplotypes, with the oracle's
    outputs and the numpy restatement's decisions."""
    rng = np.random.default_rng(43)
    ta = TestcaseArray.from_batches([gen.phmm_batch(rng, 64, 32) for _ in range(4)])
    return ta, oracle_run(ta), ref.predict_array(ta)


# ------------------------------------------------------------------------------------------ CPU


def test_log_estimate():
    """lc(C) is 100 log10(C) to within 4 units: the mantissa is linear between powers of two (at most
    0.0861 in log2, 2.6 units), cut to 8 bits (0.12) and the product floored (1)."""
    for C in list(range(1, 2000)) + [9400, 65535]:
        assert abs(ref.lc(C) - 100 * np.log10(C)) <= 4, C


def test_certificate_bounds_f32_by_f64(exit_cases):
    """About 2 000 testcases (gen.phmm_batch jobs, reads with R + C up to 723, the early-exit fixture): for
    every certified one the oracle's f32 result is at most K * f64 result * 2^-900 + 4e-35."""
    from genomicsbench_palisade_amd import phmm
    rng = np.random.default_rng(11)
    parts = [TestcaseArray.from_batch(gen.phmm_batch(rng, 40, 24)),
             TestcaseArray.from_batch(gen.phmm_batch(rng, 30, 20, read_len=(240, 250))),
             TestcaseArray.from_batch(gen.phmm_batch(rng, 20, 16, q_range=(1, 60))),
             TestcaseArray.from_pairs([(c["read"], c["hap"]) for c in exit_cases])]
    long_hap = BASES[rng.integers(0, 4, 473)].tobytes()  # the longest of the benchmark's shapes: 250 + 473
    parts.append(TestcaseArray.from_pairs([((long_hap[at:at + 250],) + quals(250, q), long_hap)
                                           for at, q in ((0, 40), (100, 20), (223, 6))]))
    assert 1900 <= sum(p.n for p in parts) <= 2200
    assert max(int((p.np_arr["rslen"][:p.n] + p.np_arr["haplen"][:p.n]).max()) for p in parts) >= 723
    o = oracle_lib.oracle()
    ncert = 0
    for ta in parts:
        K, cert = phmm.certificate(ta)
        assert (np.isfinite(K) | ~cert).all() and (K[cert] <= 2).all() and (K[np.isfinite(K)] >= 1).all()
        idx = np.nonzero(np.isfinite(K))[0]
        rf = np.array([o.phmm_oracle_prob_f32(ctypes.addressof(ta.arr[k])) for k in idx], np.float64)
        rd = np.array([o.phmm_oracle_prob_f64(ctypes.addressof(ta.arr[k])) for k in idx])
        bound = K[idx] * np.ldexp(rd, -900) + 4e-35
        assert (rf <= bound).all(), (rf[rf > bound][:5], bound[rf > bound][:5])
        ncert += int(cert.sum())
    assert ncert >= 1800


def test_uncertified_reads():
    """An insertion or deletion quality of 0..3 or a base quality of 0 in any row: never certified."""
    rng = np.random.default_rng(12)
    b = gen.phmm_batch(rng, 1, 1)
    read, hap = b.reads[0], b.haps[0]
    from genomicsbench_palisade_amd import phmm
    pairs = [(read, hap)]
    for field, vals in ((2, range(4)), (3, range(4)), (1, (0,))):
        for v in vals:
            for row in (0, len(read[0]) // 2, len(read[0]) - 1):
                x = bytearray(read[field])
                x[row] = v
                pairs.append((read[:field] + (bytes(x),) + read[field + 1:], hap))
    K, cert = phmm.certificate(TestcaseArray.from_pairs(pairs))
    assert cert[0] and np.isfinite(K[0])
    assert not cert[1:].any() and np.isinf(K[1:]).all()


def test_near_threshold_fixture(near_pairs):
    """The fixture's f32 results lie in (0.5e-28, 2e-28), at least 8 on each side of MIN_ACCEPTED; the
    search that found them (tests/golden/make_phmm_near_golden.py) took about a minute and a half, recorded."""
    z = np.load(os.path.join(GOLDEN, "phmm_near_golden.npz"))
    assert float(z["search_seconds"]) > 0 and int(z["search_evals"]) > 0
    rf = oracle_run(TestcaseArray.from_pairs(near_pairs))[1]
    assert ((rf > 0.5e-28) & (rf < 2e-28)).all()
    assert (rf < MIN_ACCEPTED).sum() >= 8 and (rf >= MIN_ACCEPTED).sum() >= 8


# ------------------------------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def phmm():
    from genomicsbench_palisade_amd import phmm, set_device
    set_device(0)
    phmm.init_pairhmm()
    return phmm


def run_batch(phmm, ta, stacks=None):
    """One run of a device batch: (results, raw f32, raw f64, used), exit_stats, predict_stats, predicted.
    stacks: the number of stacks the batch must have been packed into."""
    db = phmm.DeviceBatch(ta)
    try:
        assert stacks is None or db.stacks() == stacks, (db.stacks(), stacks)
        db.run()
        return db.results()[:4], db.exit_stats(), db.predict_stats(), db.predicted().astype(bool)
    finally:
        db.close()


@pytest.mark.gpu
def test_decisions_pinned(phmm, monkeypatch, seed43_job):
    """The seed-43 job: the gate opens and the predicted set is the numpy restatement's exactly (every
    read of the job is certified); outputs exact with the predictor on, off and on every certified
    testcase, in both sweeps; the early exit's statistics do not fall."""
    ta, exp, want = seed43_job
    assert phmm.certificate(ta)[1].all() and 0 < want.sum() < ta.n
    for roll in ("0", "1"):
        monkeypatch.setenv("GB_PHMM_ROLL", roll)
        monkeypatch.delenv("GB_PHMM_PREDICT", raising=False)
        got, ex_on, st, pred = run_batch(phmm, ta)
        assert_phmm_exact(got, exp)
        assert st.sampled > 0 and st.predicted == int(want.sum()) > 0
        assert (pred == want).all(), np.nonzero(pred != want)[0][:10]
        assert st.confirmed + st.redone == st.predicted and st.confirmed > 0
        # a confirmed testcase skipped the f32 pass (raw f32 0); a redone one holds the reference's f32
        # (every false positive, and a fallback whose f64 result lies within the certificate's K of 1e-28)
        redone = pred & ((exp[1] >= MIN_ACCEPTED) | (got[1] != 0))
        assert st.redone == int(redone.sum()) >= int((pred & (exp[1] >= MIN_ACCEPTED)).sum())
        assert (got[1][pred & ~redone] == 0).all()
        assert (bits(got[1][redone]) == bits(exp[1][redone])).all()
        assert (np.ldexp(exp[2][redone & (exp[1] < MIN_ACCEPTED)], -900) * 1.01 >= 1e-28).all()
        monkeypatch.setenv("GB_PHMM_PREDICT", "0")
        got, ex_off, st0, pred0 = run_batch(phmm, ta)
        assert_phmm_exact(got, exp)
        assert st0 == (0, 0, 0, 0) and not pred0.any()
        assert ex_on[0] >= ex_off[0] > 0
        monkeypatch.setenv("GB_PHMM_PREDICT", "all")
        got, _, st2, pred2 = run_batch(phmm, ta)
        assert_phmm_exact(got, exp)
        assert pred2.all() and st2.predicted == ta.n


@pytest.mark.gpu
def test_redo_path(phmm, monkeypatch, seed43_job, near_pairs):
    """GB_PHMM_PREDICT=all: every passing testcase goes f64 -> verify fails -> f32 redo, and comes out as
    if never predicted (answered from f32, raw f64 0, raw f32 the reference's bits); next to the
    threshold the fallback choice is the reference's on both sides."""
    monkeypatch.setenv("GB_PHMM_PREDICT", "all")
    ta, exp, _ = seed43_job
    passing = exp[1] >= MIN_ACCEPTED
    got, ex, st, pred = run_batch(phmm, ta)
    assert_phmm_exact(got, exp)
    assert (got[3][passing] == 0).all() and (got[2][passing] == 0).all()
    assert (bits(got[1][passing]) == bits(exp[1][passing])).all()
    assert st.redone == int((passing & phmm.certificate(ta)[1]).sum()) and st.confirmed == ta.n - st.redone
    assert ex[0] == st.confirmed  # redone testcases are not counted
    near = TestcaseArray.from_pairs(near_pairs)
    nexp = oracle_run(near)
    got, _, st, pred = run_batch(phmm, near)
    assert pred.all()
    assert_phmm_exact(got, nexp)
    assert (got[3].astype(bool) == (nexp[1] < MIN_ACCEPTED)).all()
    assert st.redone >= int((nexp[1] >= MIN_ACCEPTED).sum()) >= 8 and st.confirmed <= int((nexp[1] < MIN_ACCEPTED).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [None, "all"])
def test_exit_fixture(phmm, monkeypatch, exit_cases, mode):
    """The early exit's traps and controls: outputs exact, no trap answered from f64, no uncertified read
    predicted."""
    if mode:
        monkeypatch.setenv("GB_PHMM_PREDICT", mode)
    ta = TestcaseArray.from_pairs([(c["read"], c["hap"]) for c in exit_cases])
    exp = (np.array([c["final"] for c in exit_cases]), np.array([c["raw_f"] for c in exit_cases], np.float32),
           np.array([c["raw_d"] for c in exit_cases]))
    trap = np.array([c["kind"] == "trap" for c in exit_cases])
    cert = phmm.certificate(ta)[1]
    got, _, st, pred = run_batch(phmm, ta)
    assert_phmm_exact(got, exp)
    assert not got[3][trap].any() and (got[2][trap] == 0).all()
    assert not (pred & ~cert).any()
    if mode == "all":
        assert (pred == cert).all()


def edge_job(rng, C, kinds):
    """One haplotype of C columns and a read per entry of `kinds`: 'p' 80 random rows (predicted: no
    diagonal is cheap), 's' a 30-row piece of the haplotype (a survivor), or a survivor's row count."""
    hap = BASES[rng.integers(0, 4, C)].tobytes()
    reads = []
    for k in kinds:
        if k == "p":
            reads.append((BASES[rng.integers(0, 4, 80)].tobytes(),) + quals(80))
        else:
            n = min(30 if k == "s" else int(k), C)
            at = int(rng.integers(0, C - n + 1))
            reads.append((hap[at:at + n],) + quals(n))
    return TestcaseArray(reads, [hap])


PATTERNS = {"first": ["p"] * 16 + ["s"] * 48, "last": ["s"] * 48 + ["p"] * 16, "alternating": ["p", "s"] * 32,
            "all": ["p"] * 64, "all but one": ["p"] * 40 + ["s"] + ["p"] * 23,
            "one turn": ["p"] * 20 + [30] + ["p"] * 20 + [30] + ["p"] * 22,
            "two turns": ["p"] * 20 + [62] + ["p"] * 20 + [62] + ["p"] * 22}


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 67, 72, 473])
def test_stack_edges(phmm, monkeypatch, C):
    """One stack of 64 testcases over one haplotype, the predicted ones first, last, alternating, all and
    all but one, and survivors of exactly one and two turns (64 and 128 stacked rows): the compacted
    f32 pass is exact and the decisions are the restatement's."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "8192")
    monkeypatch.setenv("GB_PHMM_TAIL", "0")  # one stack: no tail split into 512-row pieces
    monkeypatch.setenv("GB_PHMM_PREDICT", "open")  # the gate samples two testcases of a stack: too few here
    rng = np.random.default_rng(100 + C)
    for name, kinds in PATTERNS.items():
        ta = edge_job(rng, C, kinds)
        want = ref.predict_array(ta)
        assert (want == np.array([k == "p" for k in kinds])).all(), name
        got, ex, st, pred = run_batch(phmm, ta, stacks=1)
        assert_phmm_exact(got, oracle_run(ta))
        assert (pred == want).all(), name
        assert st.confirmed == int(want.sum()) and st.redone == 0, (name, st)
        assert (got[1][~want] >= MIN_ACCEPTED).all(), name  # the survivors were computed in f32


@pytest.mark.gpu
def test_redo_shares_a_stack(phmm, monkeypatch):
    """A false positive: a read that is two pieces of the haplotype with 40 columns deleted between them has
    no cheap ungapped diagonal, yet passes the f32 test. It is redone inside a stack whose other
    testcases are confirmed predictions and survivors."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "8192")
    monkeypatch.setenv("GB_PHMM_TAIL", "0")  # one stack: no tail split into 512-row pieces
    monkeypatch.setenv("GB_PHMM_PREDICT", "open")  # the gate samples two testcases of a stack: too few here
    rng = np.random.default_rng(5)
    C = 300
    hap = BASES[rng.integers(0, 4, C)].tobytes()
    gapped = (hap[20:70] + hap[110:160],) + quals(100)
    reads = []
    for k in range(24):
        reads.append(gapped if k % 8 == 3 else
                     ((BASES[rng.integers(0, 4, 80)].tobytes(),) + quals(80)) if k % 2 else
                     ((hap[k:k + 60],) + quals(60)))
    ta = TestcaseArray(reads, [hap])
    exp = oracle_run(ta)
    is_gapped = np.array([k % 8 == 3 for k in range(24)])
    assert (exp[1][is_gapped] >= MIN_ACCEPTED).all()
    want = ref.predict_array(ta)
    assert want[is_gapped].all()
    got, ex, st, pred = run_batch(phmm, ta, stacks=1)
    assert_phmm_exact(got, exp)
    assert (pred == want).all()
    assert st.redone == int(is_gapped.sum()) and st.confirmed == int(want.sum()) - st.redone > 0
    assert (bits(got[1][is_gapped]) == bits(exp[1][is_gapped])).all() and (got[2][is_gapped] == 0).all()
    assert ex[0] >= st.confirmed


@pytest.mark.gpu
def test_other_base_codes(phmm, monkeypatch):
    """N on either side matches everything and any byte besides A, C, T, G, N is an A (ConvertChar), in the
    kernel as in the restatement: reads and a haplotype with N, lower-case and IUPAC bytes, decisions
    pinned on both sides of the threshold."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "8192")
    monkeypatch.setenv("GB_PHMM_TAIL", "0")
    monkeypatch.setenv("GB_PHMM_PREDICT", "open")
    rng = np.random.default_rng(31)
    h = bytearray(BASES[rng.integers(0, 4, 200)].tobytes())
    for at in range(5, 200, 9):
        h[at] = b"NnRYa"[at % 5]
    hap = bytes(h)
    reads = []
    for k in range(16):
        n = 90
        b = bytearray(hap[k:k + n]) if k % 2 else bytearray(BASES[rng.integers(0, 4, n)].tobytes())
        for at in range(k % 7, n, 7):  # a seventh of the rows: N, or a byte that reads as A
            b[at] = b"NNacgtKM"[(at + k) % 8]
        reads.append((bytes(b),) + quals(n))
    ta = TestcaseArray(reads, [hap])
    want = ref.predict_array(ta)
    assert want.any() and not want.all()
    got, _, st, pred = run_batch(phmm, ta, stacks=1)
    assert_phmm_exact(got, oracle_run(ta))
    assert (pred == want).all(), np.nonzero(pred != want)[0]
    assert st.confirmed + st.redone == int(want.sum())


@pytest.mark.gpu
def test_long_haplotype(phmm):
    """A haplotype of 9 401 columns (records in global memory): never predicted, exact."""
    rng = np.random.default_rng(9)
    hap = BASES[rng.integers(0, 4, 9401)].tobytes()
    reads = [(hap[500:600],) + quals(100), (BASES[rng.integers(0, 4, 100)].tobytes(),) + quals(100)]
    ta = TestcaseArray(reads, [hap])
    got, _, st, pred = run_batch(phmm, ta)
    assert_phmm_exact(got, oracle_run(ta))
    assert not pred.any() and st.predicted == 0


@pytest.mark.gpu
def test_gate_stays_closed(phmm):
    """Reads identical to their haplotype window: nothing falls back, the sample taken when the batch is
    packed predicts nothing, and the run launches no predictor."""
    rng = np.random.default_rng(21)
    haps = [BASES[rng.integers(0, 4, int(rng.integers(250, 474)))].tobytes() for _ in range(16)]
    pairs = []
    for h in haps:
        for _ in range(32):
            n = int(rng.integers(100, 251))
            at = int(rng.integers(0, len(h) - n + 1))
            pairs.append(((h[at:at + n],) + quals(n, 30), h))
    ta = TestcaseArray.from_pairs(pairs)
    exp = oracle_run(ta)
    assert (exp[1] >= MIN_ACCEPTED).all()
    got, ex, st, pred = run_batch(phmm, ta)
    assert_phmm_exact(got, exp)
    assert st.sampled > 0 and st.predicted == 0 and not pred.any() and ex == (0, 0)
