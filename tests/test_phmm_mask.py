"""The emission select of the PairHMM sweeps (csrc/phmm.hip select_dist: dmatch or dmis from the row's
match mask and the column's haplotype code, the code 5 at column 0 and 6 below it serving v0) against
the oracle, bit for bit, in both passes: every class of row (va, v0, read base A C G T, N, a byte
outside ACGTN) against every class of column, every class of row on the lanes where the rolled
sweep's groups and turns meet, the haplotype lengths around kLdsHaplen, and every kind of stack in
one launch. Written for the trial of per-base 0x00 / 0xFF mask rows in LDS (phmm: "Match
masks from LDS"), which any other layout of the codes has to pass as well."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from conftest import assert_phmm_exact, bits
from genomicsbench_palisade_amd import gen
from genomicsbench_palisade_amd._tc import TestcaseArray

pytestmark = pytest.mark.gpu

LDS_HAPLEN = 9400  # csrc/phmm.hip:51 kLdsHaplen: the longest haplotype whose stack keeps its records in LDS
BASES = np.frombuffer(b"ACGT", np.uint8)
SYMBOLS = np.frombuffer(b"ACGTNX", np.uint8)  # X: a byte outside ACGTN (ConvertChar gives it A's code)
MIN_ACCEPTED = np.float32(1e-28)


@pytest.fixture(scope="module")
def phmm():
    from genomicsbench_palisade_amd import phmm, set_device
    set_device(0)
    phmm.init_pairhmm()
    return phmm


def oracle_run(ta):
    """(log10, raw f32, raw f64 where f32 falls back, raw f64 of every testcase) of the oracle, checked
    against the reference's own GKL kernels where they are built."""
    o = oracle_lib.oracle()
    out, rf, rd = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
    o.phmm_oracle_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data, None, 16)
    all64 = np.array([o.phmm_oracle_prob_f64(ctypes.addressof(ta.arr[k])) for k in range(ta.n)])
    ref = oracle_lib.ref_phmm()
    if ref is not None:
        for eng in (256, 512) if ref.ref_phmm_has_avx512() else (256,):
            g = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
            ref.ref_phmm_batch(ctypes.addressof(ta.arr), ta.n, g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data,
                               eng, 16)
            for a, b in zip(g, (out, rf, rd)):
                assert (bits(a) == bits(b)).all(), eng
    return out, rf, rd, all64


def both_sides(exp):
    """The job exercises the f64 pass on purpose: f32 results on both sides of MIN_ACCEPTED."""
    return bool((exp[1] < MIN_ACCEPTED).any() and (exp[1] >= MIN_ACCEPTED).any())


def assert_raw_exact(got, expect):
    for k, name in enumerate(("log10", "raw f32", "raw f64")):
        bad = np.nonzero(bits(got[k]) != bits(expect[k]))[0]
        assert len(bad) == 0, f"{name} mismatch at {bad[:10]}: {got[k][bad[:5]]} vs {expect[k][bad[:5]]}"


def all_exact(phmm, monkeypatch, ta, exp):
    """The early exit off (every raw f32) and on (what computelikelihoodsboth exposes), and the f64 pass
    forced over every testcase."""
    monkeypatch.setenv("GB_PHMM_EXIT", "0")
    assert_raw_exact(phmm.compute_likelihoods_both(ta), exp)
    monkeypatch.delenv("GB_PHMM_EXIT")
    assert_phmm_exact(phmm.compute_likelihoods_both(ta), exp)
    assert (bits(phmm.compute_f64(ta)) == bits(exp[3])).all()


def quals(rng, n):
    """Benchmark-range qualities of a read of n rows."""
    return (rng.integers(6, 41, n).astype(np.uint8).tobytes(), rng.integers(40, 46, n).astype(np.uint8).tobytes(),
            rng.integers(40, 46, n).astype(np.uint8).tobytes(), bytes([10]) * n)


def cut_read(rng, n, hap):
    """n rows cut from the haplotype (wrapping), one base in ten substituted: a passing f32 result."""
    h = np.frombuffer(hap, np.uint8)
    b = h[(int(rng.integers(0, len(h))) + np.arange(n)) % len(h)].copy()
    sub = rng.random(n) < 0.1
    b[sub] = BASES[rng.integers(0, 4, int(sub.sum()))]
    return (b.tobytes(),) + quals(rng, n)


def random_read(rng, n, symbols=BASES):
    return (symbols[rng.integers(0, len(symbols), n)].tobytes(),) + quals(rng, n)


# ------------------------------------------------------------- 1. row classes against column classes


def class_job(C):
    """Haplotypes of C columns over A C G T N and X -- N at column 1 and at column C, every symbol in
    turn, plain bases -- against reads over the same symbols, N their first and their last row, short
    ones cut from the plain haplotype (passing) and long random ones (falling back). 272 to 295 stacked
    rows per haplotype: a rolled sweep from C = 64 on, a fill per stripe below."""
    rng = np.random.default_rng(4100 + C)
    mid = SYMBOLS[rng.integers(0, 6, max(C - 2, 0))].tobytes()
    haps = [(b"N" + mid + b"N")[:C] if C > 1 else b"N", (b"XNTGCA" * (C // 6 + 1))[:C],
            BASES[rng.integers(0, 4, C)].tobytes()]
    reads = [(b"N",) + quals(rng, 1), (b"NACGTXN",) + quals(rng, 7), (b"XTGCAN",) + quals(rng, 6),
             cut_read(rng, 3, haps[2]), cut_read(rng, min(C, 24), haps[2])]
    r = random_read(rng, 110, SYMBOLS)
    reads.append((b"N" + r[0][1:-1] + b"N",) + r[1:])
    reads.append(random_read(rng, 130, SYMBOLS))
    assert sum(len(x[0]) + 2 for x in reads) == 271 + min(C, 24)  # 5 turns
    return TestcaseArray(reads, haps)


@pytest.fixture(scope="module")
def class_jobs():
    jobs = {C: class_job(C) for C in (1, 2, 63, 64, 65, 130)}
    return {C: (ta, oracle_run(ta)) for C, ta in jobs.items()}


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130])
def test_row_classes_against_column_classes(phmm, monkeypatch, class_jobs, C):
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "512")
    ta, exp = class_jobs[C]
    assert both_sides(exp)
    all_exact(phmm, monkeypatch, ta, exp)


# ---------------------------------------------------------------- 2. row classes on the layout's lanes

LANES = (0, 15, 16, 47, 48, 63)  # the first and last lanes of a turn and of the groups that switch inside it
ROW_CLASSES = ("va", "v0") + tuple("NACGTX")


def lane_stack(rng, va_lanes, hap, turn, seen):
    """Reads of one stack (at most 512 rows, so batch_fill keeps it whole) whose first virtual rows fall
    on `va_lanes` in turn, then 62- and 126-row reads up to 8 turns. Real rows on a lane of LANES take the read
    bases N A C G T X in turn (per lane, counted in `turn` across stacks); every other row is cut from
    the haplotype, or random in the 126-row reads, so that results fall on both sides of
    MIN_ACCEPTED. `seen` collects (class, lane)."""
    lens, at = [], 0  # the first read's va is on lane 0
    for nxt in va_lanes:
        n = (nxt - at) % 64 - 2
        lens.append(n if n >= 1 else n + 64)
        at += lens[-1] + 2
    while at + 128 <= 512:
        lens.append(126 if len(lens) % 2 else 62)
        at += lens[-1] + 2
    assert at >= 200 and at <= 512 and len(lens) <= 64
    reads, g = [], 0
    h = np.frombuffer(hap, np.uint8)
    for k, n in enumerate(lens):
        seen.add(("va", g % 64))
        seen.add(("v0", (g + 1) % 64))
        rd = cut_read(rng, n, hap) if n < 100 else random_read(rng, n)
        b = np.frombuffer(rd[0], np.uint8).copy()
        for r in range(n):
            lane = (g + 2 + r) % 64
            if lane in LANES:
                b[r] = SYMBOLS[(4, 0, 1, 2, 3, 5)[turn[lane] % 6]]
                turn[lane] += 1
                seen.add((chr(b[r]), lane))
        reads.append((b.tobytes(),) + rd[1:])
        g += n + 2
    return reads


@pytest.fixture(scope="module")
def lane_job():
    rng = np.random.default_rng(4200)
    seen, turn, parts = set(), {l: 0 for l in LANES}, []
    for va_lanes in ((15, 16, 47, 48, 63, 0), (63, 14, 15, 46, 47, 62), (16, 48, 15, 47, 63, 0),
                     (63, 15, 47, 14, 46, 62)):
        hap = BASES[rng.integers(0, 4, 100)].tobytes()
        parts.append(gen.PhmmBatch(lane_stack(rng, va_lanes, hap, turn, seen), [hap]))
    missing = [(c, l) for c in ROW_CLASSES for l in LANES if (c, l) not in seen]
    assert not missing, missing
    ta = TestcaseArray.from_batches(parts)
    return ta, oracle_run(ta)


@pytest.mark.parametrize("roll", ["1", "0"])
def test_row_classes_on_layout_lanes(phmm, monkeypatch, lane_job, roll):
    """va, v0, an N row, a row of each base and of a byte outside ACGTN on lanes 0, 15, 16, 47, 48 and 63
    of a turn, in stacks of 7 or 8 turns over C = 100, rolled and with a fill per stripe, the exit off and on."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "512")
    monkeypatch.setenv("GB_PHMM_ROLL", roll)
    ta, exp = lane_job
    assert both_sides(exp)
    all_exact(phmm, monkeypatch, ta, exp)


# ----------------------------------------------------------------------------------- 3. the LDS edge


def test_lds_edge(phmm, monkeypatch):
    """Haplotypes of kLdsHaplen - 1, kLdsHaplen (the last in LDS), kLdsHaplen + 1 (the first with its
    records in global memory) and 300 columns in one batch, both passes."""
    rng = np.random.default_rng(4300)
    src = BASES[rng.integers(0, 4, LDS_HAPLEN + 1)]
    pairs = []
    for hl in (LDS_HAPLEN - 1, LDS_HAPLEN, LDS_HAPLEN + 1, 300):
        hap = src[:hl].tobytes()
        for st in (0, hl // 2, hl - 12):
            pairs.append(((src[st:st + 12].tobytes(),) + quals(rng, 12), hap))
        pairs.append((random_read(rng, 150), hap))
        pairs.append((random_read(rng, 70, SYMBOLS), hap))
    ta = TestcaseArray.from_pairs(pairs)
    exp = oracle_run(ta)
    assert both_sides(exp)
    all_exact(phmm, monkeypatch, ta, exp)


# ------------------------------------------------------------------------------- 4. one mixed launch


def test_mixed_launch_twice(phmm, monkeypatch):
    """A rolled stack (C = 300), a single stripe (C = 200), C < 64 and a long haplotype in one
    DeviceBatch, run twice: the two runs identical, and exact."""
    monkeypatch.setenv("GB_PHMM_STACK_ROWS", "512")
    rng = np.random.default_rng(4400)
    haps = {C: BASES[rng.integers(0, 4, C)].tobytes() for C in (300, 200, 40, LDS_HAPLEN + 1)}
    pairs = []
    for k in range(5):  # 62 and 122 stacked rows in turn
        rd = cut_read(rng, 60, haps[300]) if k % 2 else random_read(rng, 120, SYMBOLS)
        pairs.append((rd, haps[300]))
    pairs += [(cut_read(rng, 20, haps[200]), haps[200]), (random_read(rng, 30, SYMBOLS), haps[200])]
    pairs += [(cut_read(rng, 30, haps[40]), haps[40]), (random_read(rng, 100, SYMBOLS), haps[40])]
    pairs += [(cut_read(rng, 40, haps[LDS_HAPLEN + 1]), haps[LDS_HAPLEN + 1]),
              (random_read(rng, 90), haps[LDS_HAPLEN + 1])]
    ta = TestcaseArray.from_pairs(pairs)
    exp = oracle_run(ta)
    assert both_sides(exp)
    db = phmm.DeviceBatch(ta)
    try:
        runs = []
        for _ in range(2):
            db.run()
            runs.append(db.results())
    finally:
        db.close()
    for a, b in zip(*runs):
        assert (bits(a) == bits(b)).all() if a.dtype != np.uint8 else (a == b).all()
    assert_phmm_exact(runs[0][:4], exp)
    monkeypatch.setenv("GB_PHMM_EXIT", "0")
    assert_raw_exact(phmm.compute_likelihoods_both(ta), exp)
    assert (bits(phmm.compute_f64(ta)) == bits(exp[3])).all()
