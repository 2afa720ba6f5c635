"""The PairHMM fallback predictor's early leave and the f64 pass's own verify and redo (csrc/phmm.hip
phmm_predict, verify_unit). phmm_predict leaves a 64-diagonal chunk once none of its diagonals can end at or
below the threshold and a testcase once a group of chunks decided it; the f64 pass's waves confirm their
predicted testcases themselves and sweep the unconfirmed ones in f32 at once. Decisions against the numpy
restatement (tests/phmm_predict_ref.py), outputs against the oracle bit for bit, at the row, chunk and
group edges of the predictor and at the stack, part and grid edges of the redo. One stack holds a
haplotype's testcases (GB_PHMM_STACK_ROWS=8192, GB_PHMM_TAIL=0), no gate (GB_PHMM_PREDICT=open / all), and
every read is certified (q = 10 / 20 / 40, i = d = 45, c = 10). The jobs are built and their expectations
asserted on the reference alone (module fixtures) before any device is touched."""
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
ROWS = (1, 32, 33, 63, 64, 65, 127, 128, 129, 250)  # one to four 64-row iterations, and their edges
# chunks per testcase: a group of one chunk, a full group, a full group and one, two full groups and one.
# A batch takes two of them: with one chunk the read overhangs the haplotype by 63 rows or more, which alone
# costs more than thr, so those testcases are all predicted.
CHUNKS = ((1, 2), (4, 5), (8, 9))
Q_OF_CLASS = (10, 20, 40)    # a base quality of each class (weights 140, 250, 390)


def oracle_run(ta):
    o = oracle_lib.oracle()
    out, rf, rd = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
    o.phmm_oracle_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data, None, 16)
    return out, rf, rd


def thr_of(C):
    return ref.THRESH - ref.lc(C) + ref.MARGIN


def nchunks(R, C):
    return (C - R + 126) // 64 + 1


def rand_bases(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def read_on(rng, hap, R, d, mism=()):
    """A read of R rows on diagonal d of the haplotype (row r against column r + d; rows outside the
    haplotype are random), matching but for `mism`: (row, quality class) pairs that mismatch."""
    C = len(hap)
    b = bytearray(rand_bases(rng, R))
    q = bytearray([40]) * R
    for r in range(R):
        if 0 <= r + d < C:
            b[r] = hap[r + d]
    for r, cls in mism:
        assert 0 <= r + d < C, (r, d, C)
        if hap[r + d] not in b"ACGT":  # an N column matches everything
            continue
        b[r] = b"ACGT"[(b"ACGT".index(hap[r + d]) + 1) % 4]
        q[r] = Q_OF_CLASS[cls]
    return (bytes(b), bytes(q), bytes([45]) * R, bytes([45]) * R, bytes([10]) * R)


def cost_on(read, hap, d):
    """The restatement's cost of one diagonal."""
    R, C = len(read[0]), len(hap)
    rc, hc = ref.CODE[np.frombuffer(read[0], np.uint8)], ref.CODE[np.frombuffer(hap, np.uint8)]
    qq = np.frombuffer(read[1], np.uint8) & 127
    w = np.where(qq < 14, 140, np.where(qq < 28, 250, 390))
    cost = 0
    for r in range(R):
        if 0 <= r + d < C and rc[r] != hc[r + d] and rc[r] != 4 and hc[r + d] != 4:
            cost += int(w[r])
    n_lo = min(R, max(0, -d))
    n_hi = min(R - n_lo, max(0, R + d - C))
    return cost + int(ref.overhang(np.int64(n_lo))) + int(ref.overhang(np.int64(n_hi)))


class Job:
    """Testcases with the oracle's outputs and the restatement's decisions, computed once. Consecutive
    pairs over the same haplotype object share its buffer, so the pack puts them into one stack, in order."""

    def __init__(self, pairs, notes=None):
        groups = []
        for read, hap in pairs:
            if not groups or groups[-1][1] is not hap:
                groups.append(([], hap))
            groups[-1][0].append(read)
        self.ta = TestcaseArray.from_batches([gen.PhmmBatch(reads, [hap]) for reads, hap in groups])
        assert self.ta.n == len(pairs)
        self.exp = oracle_run(self.ta)
        self.want = ref.predict_array(self.ta)
        self.notes = notes or [None] * len(pairs)
        self.cells = np.array([len(r[0]) * len(h) for r, h in pairs], np.int64)


def edge_pairs(nch, seed):
    """For every R of ROWS that a haplotype of nch chunks exists for: the true diagonal in chunk 0 with a
    left overhang, in the last chunk of the first group, in the first chunk of the second group and in the
    last chunk with a right overhang; each matching (a cheap diagonal: not predicted; in a later group
    than the first, that group decides) and with 20 q = 40 mismatches (7800 > thr: predicted)."""
    rng = np.random.default_rng(seed)
    pairs, notes = [], []
    for R in ROWS:
        # (with 4 and 5 chunks the last chunk holds a diagonal with at most 3 rows of overhang only at its
        # widest)
        C = R - 126 + 64 * (nch - 1) + int(rng.integers(60 if nch in (4, 5) else 0, 64))
        if C < 1:
            continue
        assert nchunks(R, C) == nch
        hap = rand_bases(rng, C)
        dhi = C - R + 63
        places = {"left": max(-63, min(-min(3, R - 1), dhi)), "right": min(dhi, max(-63, C - R + min(3, R - 1)))}
        if C - R + 3 >= 192 - 63:
            places["group 0 last"] = max(192 - 63, min(C - R, 255 - 63))
        if C - R + 3 >= 256 - 63:
            places["group 1 first"] = 256 - 63
        for name, d in places.items():
            assert -63 <= d <= C - R + 63
            inside = [r for r in range(R) if 0 <= r + d < C]
            pairs.append((read_on(rng, hap, R, d), hap))
            notes.append((R, C, name, d, False))
            if len(inside) >= 20:
                # spread over the read, so that every 64-row iteration has some
                rows = [inside[(k * len(inside)) // 20] for k in range(20)]
                pairs.append((read_on(rng, hap, R, d, [(r, 2) for r in rows]), hap))
                notes.append((R, C, name, d, True))
    return pairs, notes


@pytest.fixture(scope="module", params=CHUNKS)
def edge_job(request):
    pairs, notes = [], []
    for nch in request.param:
        p, n = edge_pairs(nch, 1000 + nch)
        pairs += p
        notes += n
    job = Job(pairs, notes)
    # on the reference alone: both decisions occur, a matching read that fits its haplotype is not predicted,
    # and from 63 rows on (where no other diagonal of a random haplotype is cheap) the mismatching ones are
    assert job.want.any() and not job.want.all(), request.param
    places = set()
    for (R, C, name, d, mis), w, (read, hap) in zip(notes, job.want, pairs):
        if not mis and C >= R:
            assert not w and cost_on(read, hap, d) <= 650, (R, C, name)
        elif mis and R >= 63:
            assert w, (R, C, name)
        places.add(name)
    nch = max(request.param)
    assert places >= {"left", "right"} and (nch < 4 or "group 0 last" in places) and (nch < 5 or "group 1 first" in places)
    assert {nchunks(n[0], n[1]) for n in notes} == set(request.param)
    return job


def abc_for(target, most):
    """a, b, c with 140 a + 250 b + 390 c = target and a + b + c <= most, each class present."""
    for c in range(1, target // 390 + 1):
        for b in range(1, (target - 390 * c) // 250 + 1):
            rest = target - 390 * c - 250 * b
            if rest > 0 and rest % 140 == 0 and rest // 140 + b + c <= most:
                return rest // 140, b, c
    raise AssertionError(target)


@pytest.fixture(scope="module")
def threshold_job():
    """Late crossing: reads of 129 and 250 rows that match their diagonal on all but their last k rows (q = 40),
    k on both sides of thr (at C = 473: 15 -> 5850, 16 -> 6240): the chunk stays alive to the end and the last
    rows decide. The strict compare: mixed quality classes whose cost is exactly thr (not predicted) and
    thr + 10 (predicted), reached only in the rows after the last 64-row check, or already in the first 64
    rows. N rows and N columns, which match everything, and reads of a single quality class."""
    rng = np.random.default_rng(77)
    pairs, notes = [], []
    C = 473
    hap = rand_bases(rng, C)
    thr = thr_of(C)
    assert 15 * 390 <= thr < 16 * 390
    for R in (129, 250):
        for k in (15, 16):
            pairs.append((read_on(rng, hap, R, 100, [(r, 2) for r in range(R - k, R)]), hap))
            notes.append(("late", 390 * k, thr))
    # a haplotype length whose threshold is a multiple of 10, as every cost is
    C2 = next(c for c in range(473, 300, -1) if thr_of(c) % 10 == 0)
    hap2 = rand_bases(rng, C2)
    thr2 = thr_of(C2)
    R = 250
    for target in (thr2, thr2 + 10):
        a, b, c = abc_for(target, 58)
        classes = [0] * a + [1] * b + [2] * c
        for rows in (range(R - len(classes), R), range(len(classes))):  # rows 192.. : after the last check
            assert min(rows) >= 192 or max(rows) < 64
            pairs.append((read_on(rng, hap2, R, 57, list(zip(rows, classes))), hap2))
            notes.append(("strict", target, thr2))
    # N: a seventh of the read's rows and a ninth of the columns; a single class per read
    h3 = bytearray(rand_bases(rng, 300))
    for at in range(4, 300, 9):
        h3[at] = ord("N")
    hap3 = bytes(h3)
    for k in range(6):
        cls = k % 3
        n = 150
        rd = read_on(rng, hap3, n, 20 + k, [(r, cls) for r in range(0, n, 3 + 12 * (k // 3))])
        b = bytearray(rd[0])
        for at in range(k, n, 7):
            b[at] = ord("N")
        pairs.append(((bytes(b), bytes([Q_OF_CLASS[cls]]) * n) + rd[2:], hap3))
        notes.append(("n", None, thr_of(300)))
    job = Job(pairs, notes)
    for (kind, cost, t), w, (read, hap) in zip(notes, job.want, pairs):
        if kind in ("late", "strict"):
            d = 100 if kind == "late" else 57
            assert cost_on(read, hap, d) == cost == ref.best_cost(read[0], read[1], hap) and abs(cost - t) <= 390
            assert w == (cost > t)
    strict = [n[1] - n[2] for n in notes if n[0] == "strict"]
    assert strict == [0, 0, 10, 10]
    nw = job.want[[n[0] == "n" for n in notes]]
    assert nw.any() and not nw.all() and job.want.any() and not job.want.all()
    return job


# ------------------------------------------------------------------------------------------ CPU


def test_edge_jobs_on_the_reference(edge_job):
    """Every parametrised batch holds predicted and unpredicted testcases at each feasible placement
    (asserted where the job is built)."""
    assert 0 < edge_job.want.sum() < edge_job.ta.n


def test_threshold_job_on_the_reference(threshold_job):
    """The late-crossing and strict cases lie within one mismatch of thr, on both sides."""
    assert 0 < threshold_job.want.sum() < threshold_job.ta.n


# ------------------------------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def phmm():
    from genomicsbench_palisade_amd import phmm, set_device
    set_device(0)
    phmm.init_pairhmm()
    return phmm


@pytest.fixture
def one_stack_env(monkeypatch):
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "8192")
    monkeypatch.setenv("GB_PHMM_TAIL", "0")
    monkeypatch.setenv("GB_PHMM_PREDICT", "open")
    return monkeypatch


def run_batch(phmm, ta, stacks=None):
    """(results, raw f32, raw f64, used), exit_stats, predict_stats, predicted, stats of one run."""
    db = phmm.DeviceBatch(ta)
    try:
        assert stacks is None or db.stacks() == stacks, (db.stacks(), stacks)
        db.run()
        return db.results()[:4], db.exit_stats(), db.predict_stats(), db.predicted().astype(bool), db.stats()
    finally:
        db.close()


def check_decisions(phmm, job):
    assert phmm.certificate(job.ta)[1].all()
    got, ex, st, pred, _ = run_batch(phmm, job.ta)
    assert_phmm_exact(got, job.exp)
    bad = np.nonzero(pred != job.want)[0]
    assert not len(bad), [(int(k), job.notes[k]) for k in bad[:10]]
    assert st.predicted == int(job.want.sum()) and st.confirmed + st.redone == st.predicted


@pytest.mark.gpu
def test_row_and_chunk_edges(phmm, one_stack_env, edge_job):
    """R of one to four 64-row iterations against one to nine chunks, the true diagonal at the group and
    overhang edges: the decisions are the restatement's and the outputs exact, in both sweeps."""
    for roll in ("0", "1"):
        one_stack_env.setenv("GB_PHMM_ROLL", roll)
        check_decisions(phmm, edge_job)


@pytest.mark.gpu
def test_threshold_edges(phmm, one_stack_env, threshold_job):
    """Late crossings, costs of exactly thr and thr + 10, N rows and columns, single-class reads."""
    check_decisions(phmm, threshold_job)


@pytest.mark.gpu
def test_sample_mode(phmm, monkeypatch):
    """The gate's sample uses the same kernel: on test_phmm_predict.py's seed-43 job shape the gate opens, as
    the restatement's share of predicted testcases (far above one in eight) says, and the run then predicts
    the restatement's set; the same sample in both sweeps."""
    rng = np.random.default_rng(43)
    ta = TestcaseArray.from_batches([gen.phmm_batch(rng, 64, 32) for _ in range(4)])
    want = ref.predict_array(ta)
    assert want.mean() > 0.25
    exp = oracle_run(ta)
    seen = []
    for roll in ("0", "1"):
        monkeypatch.setenv("GB_PHMM_ROLL", roll)
        db = phmm.DeviceBatch(ta)
        try:
            ns = db.stacks()
            db.run()
            st, pred, got = db.predict_stats(), db.predicted().astype(bool), db.results()[:4]
        finally:
            db.close()
        # at most two testcases a stack, of one stack in 16 beyond 1024 stacks
        assert 0 < st.sampled <= 2 * ns and (ns <= 1024 or st.sampled <= ns // 4), (ns, st)
        assert (pred == want).all() and st.predicted == int(want.sum())
        assert_phmm_exact(got, exp)
        seen.append(st.sampled)
    assert seen[0] == seen[1]


def redo_job(rng, C, kinds):
    """One haplotype of C columns and a read per entry of `kinds`: 'p' 80 random rows (falls back, confirmed)
    or 's' a 30-row piece of the haplotype (passes in f32: under GB_PHMM_PREDICT=all it is sent back)."""
    hap = rand_bases(rng, C)
    pairs = []
    for k in kinds:
        if k == "p":
            pairs.append((read_on(rng, hap, 80, -200), hap))  # no row inside the haplotype: all random
        else:
            n = min(30, C)
            pairs.append((read_on(rng, hap, n, int(rng.integers(0, C - n + 1))), hap))
    return Job(pairs, list(kinds))


def check_redo(phmm, job, stacks=None):
    """Under GB_PHMM_PREDICT=all: outputs exact; the confirmed set is the certificate's on the oracle's f64
    results; a redone testcase that passes reads raw f64 0, used_double 0 and leaves the fallback count; the
    exit statistics count the confirmed testcases with all their cells."""
    K, cert = phmm.certificate(job.ta)
    assert cert.all()
    _, rf, rd = job.exp
    # (the oracle computes f64 only below MIN_ACCEPTED; a passing testcase cannot be confirmed: that would
    # prove its f32 result below MIN_ACCEPTED)
    passing = rf >= MIN_ACCEPTED
    confirmed = ~passing & (K * np.ldexp(rd, -900) + 4e-35 < float(MIN_ACCEPTED))
    got, ex, st, pred, stats = run_batch(phmm, job.ta, stacks)
    assert_phmm_exact(got, job.exp)
    assert pred.all() and st.predicted == job.ta.n
    assert st.confirmed == int(confirmed.sum()) and st.redone == int((~confirmed).sum()), (st, int(confirmed.sum()))
    assert (got[2][passing] == 0).all() and (got[3][passing] == 0).all()
    assert (bits(got[1][passing]) == bits(job.exp[1][passing])).all()
    assert (got[1][confirmed] == 0).all()
    assert stats[2] == int((~passing).sum()), stats
    assert ex == (int(confirmed.sum()), int(job.cells[confirmed].sum())), ex
    return st


REDO_PATTERNS = {"first": ["s"] + ["p"] * 11, "last": ["p"] * 11 + ["s"], "every": ["s"] * 12, "none": ["p"] * 12,
                 "between": ["p"] * 5 + ["s"] + ["p"] * 6}


@pytest.fixture(scope="module", params=[60, 64, 67, 473])
def redo_jobs(request):
    """Stripes only (C < 64), the rolled sweep at its smallest width and just above, the bench's width."""
    C = request.param
    rng = np.random.default_rng(300 + C)
    jobs = {name: redo_job(rng, C, kinds) for name, kinds in REDO_PATTERNS.items()}
    for name, job in jobs.items():  # on the reference: 's' passes, 'p' falls back far below the threshold
        s = np.array([k == "s" for k in job.notes])
        assert (job.exp[1][s] >= MIN_ACCEPTED).all() and (np.ldexp(job.exp[2][~s], -900) * 4 < 1e-28).all(), name
    return jobs


@pytest.mark.gpu
def test_redo_in_one_stack(phmm, one_stack_env, redo_jobs):
    """A stack whose redone entry is first, last, every one, none, or one between confirmed ones."""
    one_stack_env.setenv("GB_PHMM_PREDICT", "all")
    for roll in ("0", "1"):
        one_stack_env.setenv("GB_PHMM_ROLL", roll)
        for name, job in redo_jobs.items():
            st = check_redo(phmm, job, stacks=1)
            assert st.redone == job.notes.count("s"), (name, st)


@pytest.fixture(scope="module")
def parts_jobs():
    rng = np.random.default_rng(41)
    a = ["s", "p", "p", "p", "p", "s", "p", "p", "p", "p", "p", "s", "p", "p", "p", "p"]  # quarters 0, 1, 2; both halves
    b = ["p", "s", "p", "p", "p", "p", "s", "p", "p", "p", "p", "p", "p", "p", "p", "p"]  # the first half only
    return [redo_job(rng, 200, a), redo_job(rng, 200, b)]


@pytest.mark.gpu
@pytest.mark.parametrize("parts", ["1", "2", "4"])
def test_redo_in_parts(phmm, one_stack_env, parts_jobs, parts):
    """The f64 pass takes a stack in 1, 2 and 4 units: a redone testcase in each unit, and a unit without one;
    with and without the plan, in both sweeps."""
    one_stack_env.setenv("GB_PHMM_PREDICT", "all")
    one_stack_env.setenv("GB_PHMM_F64_PARTS", parts)
    for plan in ("0", "1"):
        one_stack_env.setenv("GB_PHMM_F64_PLAN", plan)
        for roll in ("0", "1"):
            one_stack_env.setenv("GB_PHMM_ROLL", roll)
            for job in parts_jobs:
                assert check_redo(phmm, job, stacks=1).redone == job.notes.count("s")


@pytest.mark.gpu
def test_redo_then_next_unit(phmm, one_stack_env):
    """Several stacks through a grid of one wave: f64 unit, redo, f64 unit, redo in sequence. The redo has
    rewritten the records, and the unit after it is exact; stacks without a redone testcase in between."""
    one_stack_env.setenv("GB_PHMM_PREDICT", "all")
    one_stack_env.setenv("GB_PHMM_F64_GRID", "1")
    rng = np.random.default_rng(58)
    pairs = []
    for h in range(8):
        C = int(rng.integers(64, 474))
        hap = rand_bases(rng, C)
        for k in (["p", "s", "p"] * 3 if h % 3 else ["p"] * 6):
            pairs.append((read_on(rng, hap, 80, -200), hap) if k == "p" else
                         (read_on(rng, hap, 30, int(rng.integers(0, C - 29))), hap))
    job = Job(pairs)
    for plan in ("0", "1"):
        one_stack_env.setenv("GB_PHMM_F64_PLAN", plan)
        for roll in ("0", "1"):
            one_stack_env.setenv("GB_PHMM_ROLL", roll)
            st = check_redo(phmm, job, stacks=8)
            assert st.redone == 15 and st.confirmed == job.ta.n - 15


@pytest.mark.gpu
def test_near_threshold_in_the_grid(phmm, one_stack_env):
    """tests/golden/phmm_near_golden.npz (20 testcases within a factor 2 of MIN_ACCEPTED) through verify and
    redo inside the f64 pass: the fallback choice is the reference's on both sides."""
    spec = importlib.util.spec_from_file_location("make_phmm_near_golden", os.path.join(GOLDEN, "make_phmm_near_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    near = mod.load()
    one_stack_env.setenv("GB_PHMM_PREDICT", "all")
    ta = TestcaseArray.from_pairs(near)
    exp = oracle_run(ta)
    passing = exp[1] >= MIN_ACCEPTED
    assert passing.sum() >= 8 and (~passing).sum() >= 8
    got, ex, st, pred, stats = run_batch(phmm, ta)
    assert_phmm_exact(got, exp)
    assert pred.all() and st.confirmed + st.redone == st.predicted == ta.n
    assert st.redone >= int(passing.sum()) and ex[0] == st.confirmed
    assert (got[2][passing] == 0).all() and (got[3][passing] == 0).all() and stats[2] == int((~passing).sum())
