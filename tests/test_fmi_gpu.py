"""GPU parity for the fmi path: the HIP index builder (csrc/fmi_build.hip) reproduces the
reference index bit for bit, and the HIP SMEM search (csrc/fmi.hip) reproduces the oracle's
(rid, m, n, k, l, s) lists, per-batch counts and phase counts exactly."""
import os

import numpy as np
import pytest

import fmi_util
from conftest import GOLDEN
from genomicsbench_palisade_amd import gen

KCAP = 40  # csrc/fmi.hip kCap: first-pass SMEM slots per read

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmi():
    from genomicsbench_palisade_amd import fmi, set_device
    set_device(0)
    return fmi


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fmi_golden.npz"))


def smem_tuple_array(a):
    return np.stack([a["rid"].astype(np.int64), a["m"].astype(np.int64), a["n"].astype(np.int64),
                     a["k"], a["l"], a["s"]], axis=1)


@pytest.mark.parametrize("size,seed,rep", [(1000, 1, 0.0), (65_536, 2, 0.1), (200_000, 11, 0.08)])
def test_gpu_index_build_bit_exact(fmi, tmp_path, size, seed, rep):
    ref = gen.fmi_reference(size, seed=seed, repeat_frac=rep)
    p_or, p_gpu = str(tmp_path / "o.bwt.2bit.64"), str(tmp_path / "g.bwt.2bit.64")
    oi = fmi_util.OracleIndex(ref, path_out=p_or)
    gi = fmi.Index.build(ref, out_path=p_gpu)
    assert gi.info() == oi.info()
    assert open(p_or, "rb").read() == open(p_gpu, "rb").read()
    oi.close()
    gi.close()


def test_search_golden_vs_bwa(fmi, golden):
    idx = fmi.Index.build(golden["ref"])
    rs = fmi.Reads(idx, golden["codes"], golden["lens"])
    rs.search(19)
    sm, tot, bc, pc = rs.results(batch_size=64)
    per = fmi_util.per_read(sm, len(golden["lens"]))
    exp = [[] for _ in range(len(golden["lens"]))]
    for r, m, n, k, l, s in zip(golden["rid"], golden["m"], golden["n"], golden["k"], golden["l"], golden["s"]):
        exp[int(r)].append((int(m), int(n), int(k), int(l), int(s)))
    assert per == [sorted(x) for x in exp]
    assert tot == len(golden["rid"]) and bc.sum() == tot


@pytest.mark.parametrize("size,nreads,L,seed", [(200_000, 3000, 151, 5), (1_000_000, 4000, 101, 6),
                                                (300_000, 2000, 250, 7)])
def test_search_vs_oracle_exact(fmi, tmp_path, size, nreads, L, seed):
    ref = gen.fmi_reference(size, seed=seed)
    codes, lens = gen.fmi_reads(ref, nreads, read_len=L, seed=seed + 100, sub_rate=0.02, n_rate=0.002)
    lens = lens.copy()
    lens[::97] = np.maximum(1, lens[::97] // 3)  # ragged lengths
    p = str(tmp_path / "r.bwt.2bit.64")
    oi = fmi_util.OracleIndex(ref, path_out=p)
    exp, ebc, epc = oi.run(codes, lens, batch_size=512)
    idx = fmi.Index.load(p)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert tot == len(exp)
    assert (bc == ebc).all() and (pc == epc).all()
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
    _, _, calls = rs.timing()
    assert calls == oi.bwt_calls()  # identical work: the same backwardExt calls


@pytest.mark.parametrize("top", ["0", "4", "5", "6", "7", "8"])
def test_prev_head_sizes_exact(fmi, monkeypatch, top):
    """The `prev` list head kept in LDS (GB_FMI_TOP entries: a ring of the last pushes, a power of two
    masked, 5 / 6 / 7 by an unsigned modulo) on reads in repeats, whose lists grow long and are
    compacted through the head: SMEMs, counts and backwardExt calls equal the oracle's."""
    monkeypatch.setenv("GB_FMI_TOP", top)
    ref = gen.fmi_reference(300_000, seed=41, repeat_frac=0.3)
    codes, lens = gen.fmi_reads(ref, 2500, read_len=151, seed=42, sub_rate=0.03, n_rate=0.002)
    oi = fmi_util.OracleIndex(ref)
    exp, ebc, epc = oi.run(codes, lens, batch_size=512)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert tot == len(exp) and (bc == ebc).all() and (pc == epc).all()
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
    assert rs.timing()[2] == oi.bwt_calls()


@pytest.mark.parametrize("q2,n_rate", [("3", 0.002), ("3", 0.03), ("3", 0.2), ("1", 0.03), ("1", 0.2), ("0", 0.03)])
def test_read_code_staging_exact(fmi, monkeypatch, q2, n_rate):
    """The search's read codes staged at 2 bits per base with each read's N positions in a register
    (pack_q2; a read with more than four N's goes to the heavy pass) -- the first 128 bases in LDS and
    the rest in registers (GB_FMI_Q2=3, default) or whole 11-word LDS rows (1) -- or at 4 bits (0), on reads from no N to mostly N's, a quarter of them in a
    repeat-rich reference, ragged lengths included: SMEMs, counts and backwardExt calls equal the
    oracle's."""
    monkeypatch.setenv("GB_FMI_Q2", q2)
    ref = gen.fmi_reference(300_000, seed=43, repeat_frac=0.25)
    codes, lens = gen.fmi_reads(ref, 2500, read_len=151, seed=44, sub_rate=0.03, n_rate=n_rate)
    lens = lens.copy()
    lens[::89] = np.maximum(1, lens[::89] // 2)
    nper = [(codes[r, :lens[r]] >= 4).sum() for r in range(len(lens))]
    if n_rate == 0.03:
        assert max(nper) > 4 and min(nper) <= 4  # both the register and the qdb form
    elif n_rate == 0.2:
        assert min(nper) > 4  # every read through qdb
    oi = fmi_util.OracleIndex(ref)
    exp, ebc, epc = oi.run(codes, lens, batch_size=512)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert tot == len(exp) and (bc == ebc).all() and (pc == epc).all()
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
    assert rs.timing()[2] == oi.bwt_calls()


def test_search_repeat_runs_identical(fmi):
    ref = gen.fmi_reference(100_000, seed=9)
    codes, lens = gen.fmi_reads(ref, 1500, seed=10)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    a = rs.results()[0]
    rs.search(19)
    rs.search(19)
    b = rs.results()[0]
    assert (a == b).all()


def test_empty_and_degenerate_reads(fmi):
    ref = gen.fmi_reference(50_000, seed=4)
    codes = np.full((6, 40), 4, np.uint8)
    codes[1, :] = 0
    codes[2, :20] = ref[100:120]
    codes[3, :] = ref[1000:1040]
    lens = np.array([40, 40, 20, 0, 1, 40], np.int32)
    oi = fmi_util.OracleIndex(ref)
    exp, _, _ = oi.run(codes, lens, batch_size=4)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    sm, tot, _, _ = rs.results(batch_size=4)
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()


def test_overflow_second_pass(fmi):
    """Short min_seed_len gives far more SMEMs per read than the first-pass slots (40): those reads
    are redone by the second pass and must still match the oracle exactly."""
    ref = gen.fmi_reference(400_000, seed=31, repeat_frac=0.3)
    codes, lens = gen.fmi_reads(ref, 1500, read_len=151, seed=32, sub_rate=0.08)
    oi = fmi_util.OracleIndex(ref)
    exp, ebc, epc = oi.run(codes, lens, batch_size=512, min_seed_len=6)
    per_read = np.bincount(exp["rid"], minlength=len(lens))
    assert per_read.max() > 40, per_read.max()
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(6)
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
    assert (bc == ebc).all() and (pc == epc).all()
    assert rs.timing()[2] == oi.bwt_calls()


@pytest.mark.parametrize("budget,min_seed,rep", [("1", 19, 0.3), ("150", 19, 0.3), ("700", 19, 0.4),
                                                  ("60", 6, 0.3), ("0", 19, 0.3)])
def test_heavy_read_pass_exact(fmi, monkeypatch, budget, min_seed, rep):
    """Reads the lane kernel hands over after GB_FMI_HEAVY backwardExt calls are redone by the
    wave-cooperative smem_heavy (one wave per read, 64 prev-list extensions per backward step): with
    small budgets most reads take that path -- including reads promoted to big slots before the
    hand-over (min_seed_len 6) and reads longer than 64 bases' lists -- and the SMEM lists, per-batch
    and per-phase counts and backwardExt calls stay those of the oracle. Budget 0 = never hand over."""
    monkeypatch.setenv("GB_FMI_HEAVY", budget)
    ref = gen.fmi_reference(400_000, seed=51, repeat_frac=rep)
    codes, lens = gen.fmi_reads(ref, 2500, read_len=151, seed=52, sub_rate=0.03, n_rate=0.002)
    lens = lens.copy()
    lens[::89] = np.maximum(1, lens[::89] // 4)
    oi = fmi_util.OracleIndex(ref)
    exp, ebc, epc = oi.run(codes, lens, batch_size=512, min_seed_len=min_seed)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(min_seed)
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert tot == len(exp)
    assert (bc == ebc).all() and (pc == epc).all()
    assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
    assert rs.timing()[2] == oi.bwt_calls()
    # every read holds at most one big slot, even one promoted by the lane kernel and then handed
    # over (smem_heavy promotes it into the slot it released)
    ctl = rs.ctl()
    per_read = np.bincount(sm["rid"].astype(np.int64), minlength=len(lens))
    assert ctl[1] == int((per_read > KCAP).sum())
    if budget in ("1", "60", "150"):
        assert ctl[4] > 0


@pytest.mark.parametrize("nthreads,min_seed,rl", [(1, 19, 151), (3, 19, 151), (1, 8, 70), (7, 12, 101)])
def test_get_smems_vs_oracle(fmi, nthreads, min_seed, rl):
    """FMI_search::getSMEMs (FMI_search.cpp:1328-1497, no benchmark caller): the right-to-left search
    over fixed-stride reads with N's (double push at an N, in-place prev/curr) and the reference's
    single-thread quota (only the first ceil(numReads / nthreads) reads), bit-exact against the C
    restatement, SMEMs in the reference's emission order, equal backwardExt counts."""
    ref = gen.fmi_reference(300_000, seed=61, repeat_frac=0.2)
    codes, lens = gen.fmi_reads(ref, 700, read_len=rl, seed=62, sub_rate=0.03, n_rate=0.01)
    codes = np.ascontiguousarray(codes[:, :rl])
    oi = fmi_util.OracleIndex(ref)
    c0 = oi.bwt_calls()
    exp = oi.get_smems(codes, len(codes), min_seed, nthreads)
    ecalls = oi.bwt_calls() - c0
    idx = fmi.Index.build(ref)
    got, calls = idx.get_smems(codes, len(codes), min_seed, nthreads)
    assert len(exp) > 0
    assert len(got) == len(exp)
    assert (smem_tuple_array(got) == smem_tuple_array(exp)).all()
    assert calls == ecalls
    assert got["rid"].max() < (len(codes) + nthreads - 1) // nthreads
    idx.close()


def test_cli_dropin(fmi, golden, tmp_path):
    """bin/fmi (CLI of benchmarks/fmi/fmi.cpp: index prefix, FASTQ, batch size, minSeedLen, threads)
    with GB_FMI_PRINT_OUTPUT=1 prints the same SMEMs and per-batch totals as bwa on the golden set."""
    import subprocess
    from conftest import ROOT
    prefix = str(tmp_path / "ref.fa")
    fmi.Index.build(golden["ref"], out_path=prefix + ".bwt.2bit.64").close()
    fq = tmp_path / "reads.fq"
    gen.write_fastq(fq, golden["codes"], golden["lens"])
    exe = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "fmi")
    env = dict(os.environ, GB_FMI_PRINT_OUTPUT="1")
    r = subprocess.run([exe, prefix, str(fq), "64", "19", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    got, rid = [], -1
    batches = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("batch_id: "):
            b, c = ln[len("batch_id: "):].split(", numTotalSmem[batch_id]: ")
            batches[int(b)] = int(c)
        elif ln.startswith("totalSmems = "):
            total = int(ln.split("=")[1])
        elif ln.endswith(":") and ln[:-1].isdigit():
            rid = int(ln[:-1])
        elif ln.startswith("[") and ln.endswith("]"):
            m, n1 = ln[1:-1].split(",")
            got.append((rid, int(m), int(n1) - 1))
    exp = sorted(zip(golden["rid"].tolist(), golden["m"].tolist(), golden["n"].tolist()))
    assert sorted(got) == exp
    assert total == len(exp) and sum(batches.values()) == total
    assert len(batches) == (len(golden["lens"]) + 63) // 64


# ---------------------------------------------------------------- SA lookup (csrc/fmi_sa.hip)

@pytest.fixture(scope="module")
def sa_golden():
    return np.load(os.path.join(GOLDEN, "fmi_sa_golden.npz"))


def golden_smems(z):
    sm = np.zeros(len(z["k"]), fmi_util.SMEM_DTYPE)
    for f in ("rid", "m", "n", "k", "l", "s"):
        sm[f] = z[f]
    return sm


def test_sa_lookup_golden_vs_bwa(fmi, golden, sa_golden, tmp_path):
    """GPU LF walk == bwa v1's SA on the golden rows (mode 0), == the call_one_step restatement
    (mode 1), for the GPU-built index and for the same index loaded from its file."""
    p = str(tmp_path / "g.bwt.2bit.64")
    built = fmi.Index.build(golden["ref"], out_path=p)
    loaded = fmi.Index.load(p)
    oi = fmi_util.OracleIndex(golden["ref"])
    rows = sa_golden["rows"]
    for idx in (built, loaded):
        assert (idx.sa_lookup(rows, fmi.SA_COMPRESSED) == sa_golden["sa"]).all()
        assert (idx.sa_lookup(rows, fmi.SA_PREFETCH) == oi.sa_lookup(rows, 1)).all()
        sm = golden_smems(golden)
        for mo in (500, 2):
            c, n = idx.sa_entries(sm, max_occ=mo, mode=fmi.SA_COMPRESSED)
            assert (n == sa_golden[f"counts{mo}"]).all() and (c == sa_golden[f"coords{mo}"]).all()
    n_, _, sent = built.info()
    every = built.sa_lookup(np.arange(n_), fmi.SA_COMPRESSED)
    assert (every == oi.sa_lookup(np.arange(n_), 0)).all() and (np.sort(every) == np.arange(n_)).all()
    assert built.sa_lookup([sent])[0] == 0
    built.close()
    loaded.close()


@pytest.mark.parametrize("max_occ,mode", [(500, 1), (100, 1), (3, 1), (40, 0)])
def test_sa_reads_vs_oracle(fmi, max_occ, mode):
    """Search then SA coordinates of every SMEM on the device (bwamem.cpp:737 over every read) ==
    the oracle's get_sa_entries(_prefetch) over the oracle's SMEMs, on a repeat-rich reference."""
    ref = gen.fmi_reference(300_000, seed=41, repeat_frac=0.4)
    codes, lens = gen.fmi_reads(ref, 3000, read_len=151, seed=42, sub_rate=0.02)
    oi = fmi_util.OracleIndex(ref)
    sm, _, _ = oi.run(codes, lens, batch_size=512)
    assert max_occ == 500 or sm["s"].max() > max_occ  # sampled intervals (step > 1) are exercised
    exp_c, exp_n = oi.sa_entries(sm, max_occ=max_occ, mode=mode)
    idx = fmi.Index.build(ref)
    rs = fmi.Reads(idx, codes, lens)
    rs.search(19)
    rs.sa_run(max_occ=max_occ, mode=mode)
    c, n, tot = rs.sa_results()
    assert tot == len(exp_c)
    assert (n == exp_n).all()
    assert (c == exp_c).all()
    ms, steps, nc = rs.sa_timing()
    assert nc == tot and ms > 0 and steps > 0
    # again, after a new search of the same reads (buffers reused)
    rs.search(19)
    rs.sa_run(max_occ=max_occ, mode=mode)
    assert (rs.sa_results()[0] == exp_c).all()


def test_sa_edge_cases(fmi):
    from genomicsbench_palisade_amd import GbError
    ref = gen.fmi_reference(30_000, seed=43)
    idx = fmi.Index.build(ref)
    n, _, _ = idx.info()
    assert len(idx.sa_lookup(np.zeros(0, np.int64))) == 0
    c, cnt = idx.sa_entries(np.zeros(0, fmi.SMEM_DTYPE))
    assert len(c) == 0 and len(cnt) == 0
    for bad in ([-1], [n]):
        with pytest.raises(GbError):
            idx.sa_lookup(bad)
    with pytest.raises(GbError):
        idx.sa_entries(np.zeros(1, fmi.SMEM_DTYPE), max_occ=0)
    # a read set whose reads give no SMEM at all
    codes = np.full((3, 50), 4, np.uint8)
    rs = fmi.Reads(idx, codes, np.full(3, 50, np.int32))
    rs.search(19)
    rs.sa_run()
    c, cnt, tot = rs.sa_results()
    assert tot == 0 and len(c) == 0
    rs2 = fmi.Reads(idx, codes, np.full(3, 50, np.int32))
    with pytest.raises(GbError):
        rs2.sa_run()  # not searched yet


def _repeat_heavy_reference():
    """Genome-like text plus long exact repeats (a 3 kb segment in four places, a 1.5 kb poly-A run,
    an 800-base dinucleotide run): tied groups that need many doubling rounds and span chunks."""
    ref = gen.fmi_reference(150_000, seed=21, repeat_frac=0.1)
    seg = ref[5_000:8_000].copy()
    for d in (20_000, 47_000, 90_000, 131_000):
        ref[d:d + len(seg)] = seg
    ref[60_000:61_500] = 0
    ref[110_000:110_800] = np.resize(np.array([1, 2], np.uint8), 800)
    return ref


@pytest.mark.parametrize("wide,chunk", [("1", ""), ("0", "5000"), ("1", "3000"), ("0", "")])
def test_gpu_index_build_chunked_and_wide(fmi, tmp_path, monkeypatch, wide, chunk):
    """The bucketed first sort, whole-group doubling chunks and 64-bit rows (the builder's path above
    2^31 rows), forced on a small repeat-heavy text, reproduce the reference index byte for byte."""
    monkeypatch.setenv("GB_FMI_BUILD_WIDE", wide)
    monkeypatch.setenv("GB_FMI_BUILD_CHUNK", chunk)
    ref = _repeat_heavy_reference()
    p_or, p_gpu = str(tmp_path / "o.bwt.2bit.64"), str(tmp_path / "g.bwt.2bit.64")
    oi = fmi_util.OracleIndex(ref, path_out=p_or)
    gi = fmi.Index.build(ref, out_path=p_gpu)
    assert gi.info() == oi.info()
    assert open(p_or, "rb").read() == open(p_gpu, "rb").read()
    oi.close()
    gi.close()


def test_gpu_index_build_refuses_oversized_chunk_groups(fmi, monkeypatch):
    # 64-suffix chunks cannot hold the ~1500 suffixes that start with eight A's (the poly-A run)
    monkeypatch.setenv("GB_FMI_BUILD_CHUNK", "64")
    from genomicsbench_palisade_amd import GbError
    with pytest.raises(GbError, match="share one 8-base prefix"):
        fmi.Index.build(_repeat_heavy_reference())


def test_recycled_read_set_and_workspace_grow_shrink_grow(fmi):
    """A closed read set goes back to its thread's free list and the next one takes over its stream
    and grow-only buffers; FMI_search's methods keep one workspace per (thread, device). Three sets in
    a row on this thread -- small, large (every buffer grows), small again (every buffer larger than
    needed) -- each searched and located, then each through getSMEMs: SMEMs, per-batch counts and SA
    coordinates equal the oracle's every time."""
    ref = gen.fmi_reference(30_000, seed=43)
    sets = [gen.fmi_reads(ref, 100, read_len=60, seed=71, sub_rate=0.02),
            gen.fmi_reads(ref, 2000, read_len=151, seed=72, sub_rate=0.02, n_rate=0.002)]
    sets.append(sets[0])
    oi = fmi_util.OracleIndex(ref)
    idx = fmi.Index.build(ref)
    for codes, lens in sets:
        exp, ebc, epc = oi.run(codes, lens, batch_size=512)
        exp_c, exp_n = oi.sa_entries(exp, max_occ=500, mode=1)
        rs = fmi.Reads(idx, codes, lens)
        rs.search(19)
        sm, tot, bc, pc = rs.results(batch_size=512)
        assert tot == len(exp) and (bc == ebc).all() and (pc == epc).all()
        assert (smem_tuple_array(sm) == smem_tuple_array(exp)).all()
        rs.sa_run(max_occ=500, mode=1)
        c, n, ctot = rs.sa_results()
        assert ctot == len(exp_c) and (n == exp_n).all() and (c == exp_c).all()
        rs.close()
    for codes, lens in sets:
        c0 = oi.bwt_calls()
        exp = oi.get_smems(codes, len(codes), 19, 1)
        ecalls = oi.bwt_calls() - c0
        got, calls = idx.get_smems(codes, len(codes), 19, 1)
        assert len(exp) > 0 and len(got) == len(exp)
        assert (smem_tuple_array(got) == smem_tuple_array(exp)).all()
        assert calls == ecalls
    idx.close()
    oi.close()
