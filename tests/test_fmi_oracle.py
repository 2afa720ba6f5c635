"""CPU: the bwa-mem2 SMEM restatement (oracle/fmi_oracle.c) is pinned to bwa v1's own SMEM code:
the committed golden vectors (tests/golden/fmi_golden.npz, made by tools/bwa via oracle/_ref) and,
when oracle/_ref is built, a live cross-check on fresh inputs."""
import os
import tempfile

import numpy as np
import pytest

import fmi_util
from conftest import GOLDEN
from genomicsbench_palisade_amd import gen


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fmi_golden.npz"))


def golden_per_read(z):
    per = [[] for _ in range(len(z["lens"]))]
    for r, m, n, k, l, s in zip(z["rid"], z["m"], z["n"], z["k"], z["l"], z["s"]):
        per[int(r)].append((int(m), int(n), int(k), int(l), int(s)))
    return [sorted(x) for x in per]


def test_oracle_matches_bwa_golden(golden):
    oi = fmi_util.OracleIndex(golden["ref"])
    sm, bc, pc = oi.run(golden["codes"], golden["lens"], batch_size=64)
    got = fmi_util.per_read(sm, len(golden["lens"]))
    exp = golden_per_read(golden)
    bad = [r for r in range(len(exp)) if got[r] != exp[r]]
    assert not bad, f"{len(bad)} reads differ, first {bad[:5]}"
    assert bc.sum() == len(sm) == len(golden["rid"])
    assert pc.sum() == len(sm) and pc.min() > 0
    oi.close()


def test_oracle_batch_order_and_counts(golden):
    """fmi.cpp:336-344: rid offset per batch, sort by (rid asc, m asc, n desc)."""
    oi = fmi_util.OracleIndex(golden["ref"])
    sm, bc, _ = oi.run(golden["codes"], golden["lens"], batch_size=100)
    key = sm["rid"].astype(np.int64) * 2**40 + sm["m"].astype(np.int64) * 2**20 - sm["n"].astype(np.int64)
    assert (np.diff(key) >= 0).all()
    edges = np.concatenate([[0], np.cumsum(bc)])
    for b in range(len(bc)):
        rids = sm["rid"][edges[b]:edges[b + 1]]
        assert ((rids >= 100 * b) & (rids < 100 * (b + 1))).all()
    oi.close()


def test_oracle_refuses_more_reseed_tasks_than_its_arrays_hold():
    """The reseeding task arrays hold batch_size * 64 entries (the reference's allocation): random
    128-base reads against a 4 000-base reference at min_seed_len 2 give more phase-2 tasks per
    512-read batch than that, which the oracle refuses with its own code instead of overrunning them;
    the same reads in batches with room for them run."""
    oi = fmi_util.OracleIndex(gen.fmi_reference(4000, seed=3, repeat_frac=0.0))
    codes = np.random.default_rng(1).integers(0, 4, (512, 128), dtype=np.uint8)
    lens = np.full(512, 128, np.int32)
    with pytest.raises(AssertionError, match="more reseeding .* tasks than its task arrays hold"):
        oi.run(codes, lens, batch_size=512, min_seed_len=2)
    sm, bc, pc = oi.run(codes[:64], lens[:64], batch_size=64, min_seed_len=6)
    assert len(sm) == bc.sum() == pc.sum() > 0
    oi.close()


def test_index_file_roundtrip(tmp_path, golden):
    p = str(tmp_path / "g.bwt.2bit.64")
    a = fmi_util.OracleIndex(golden["ref"][:50000], path_out=p)
    b = fmi_util.OracleIndex(load_path=p)
    assert a.info() == b.info()
    n, count, sent = a.info()
    assert n == 2 * 50000 + 1 and count[0] == 1 and count[4] == n
    assert os.path.getsize(p) == 8 + 40 + ((n >> 6) + 1) * 64 + ((n >> 3) + 1) * 5 + 8


def test_oracle_vs_bwa_live():
    lib = fmi_util.ref_bwa()
    if lib is None:
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    ref = gen.fmi_reference(120_000, seed=21, repeat_frac=0.2)
    codes, lens = gen.fmi_reads(ref, 400, read_len=101, seed=22, sub_rate=0.03, n_rate=0.005)
    with tempfile.TemporaryDirectory() as d:
        gen.write_fasta(d + "/ref.fa", ref)
        assert lib.ref_bwa_build((d + "/ref.fa").encode(), (d + "/ref").encode()) == 0
        bwt = lib.ref_bwa_load((d + "/ref.bwt").encode())
        exp = fmi_util.bwa_smems(lib, bwt, codes, lens)
        lib.ref_bwa_free(bwt)
    oi = fmi_util.OracleIndex(ref)
    sm, _, _ = oi.run(codes, lens, batch_size=128)
    assert fmi_util.per_read(sm, len(lens)) == exp


# ---------------------------------------------------------------- SA lookup (row f1 of SURVEY.md 8)

@pytest.fixture(scope="module")
def sa_golden():
    return np.load(os.path.join(GOLDEN, "fmi_sa_golden.npz"))


def golden_smems(z):
    sm = np.zeros(len(z["k"]), fmi_util.SMEM_DTYPE)
    for f in ("rid", "m", "n", "k", "l", "s"):
        sm[f] = z[f]
    return sm


def test_sa_oracle_matches_bwa_golden(golden, sa_golden):
    """get_sa_entry_compressed (FMI_search.cpp:1714) restated == bwa v1 bwt_sa on the same rows."""
    oi = fmi_util.OracleIndex(golden["ref"])
    assert (oi.sa_lookup(sa_golden["rows"], mode=0) == sa_golden["sa"]).all()
    sm = golden_smems(golden)
    for mo in (500, 2):
        c, n = oi.sa_entries(sm, max_occ=mo, mode=0)
        assert (n == sa_golden[f"counts{mo}"]).all()
        assert (c == sa_golden[f"coords{mo}"]).all()
    oi.close()


def test_sa_prefetch_variant_sentinel_rule(golden, sa_golden):
    """call_one_step (FMI_search.cpp:1834-1893) answers 0 where the walk meets the sentinel row after
    >= 1 step; everywhere else it equals get_sa_entry_compressed. Those rows have SA < 64 here."""
    oi = fmi_util.OracleIndex(golden["ref"])
    rows, sa = sa_golden["rows"], sa_golden["sa"]
    p = oi.sa_lookup(rows, mode=1)
    diff = p != sa
    assert diff.any() and (p[diff] == 0).all() and (sa[diff] > 0).all() and (sa[diff] < 64).all()
    n, _, sent = oi.info()
    # the row of SA value v < 64 walks v LF steps to the sentinel row unless it meets a sampled row first
    assert (oi.sa_lookup([sent], mode=1) == 0).all() and (oi.sa_lookup([sent], mode=0) == 0).all()
    oi.close()


def test_sa_all_rows_permutation(tmp_path):
    """Every row of a small index: mode 0 is a permutation of [0, n) and matches the file round trip."""
    ref = gen.fmi_reference(20_000, seed=4, repeat_frac=0.2)
    p = str(tmp_path / "s.bwt.2bit.64")
    a = fmi_util.OracleIndex(ref, path_out=p)
    b = fmi_util.OracleIndex(load_path=p)
    n, _, _ = a.info()
    rows = np.arange(n)
    sa = a.sa_lookup(rows, 0)
    assert (np.sort(sa) == rows).all()
    assert (b.sa_lookup(rows, 0) == sa).all()
    assert a.lf_steps() > 0


def test_sa_oracle_vs_bwa_live(tmp_path):
    lib = fmi_util.ref_bwa()
    if lib is None:
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    ref = gen.fmi_reference(60_000, seed=23, repeat_frac=0.3)
    d = str(tmp_path)
    gen.write_fasta(d + "/ref.fa", ref)
    assert lib.ref_bwa_build((d + "/ref.fa").encode(), (d + "/ref").encode()) == 0
    bwt = lib.ref_bwa_load((d + "/ref.bwt").encode())
    n = 2 * len(ref) + 1
    exp = fmi_util.bwa_sa(lib, bwt, d + "/ref.sa", np.arange(n))
    lib.ref_bwa_free(bwt)
    exp[0] = n - 1  # bwa v1 keeps -1 for the '$' row
    oi = fmi_util.OracleIndex(ref)
    assert (oi.sa_lookup(np.arange(n), 0) == exp).all()


@pytest.mark.parametrize("size,seed", [(120_000, 21), (1_000, 3), (4_099, 4), (65_553, 5)])
def test_bwa_v1_over_cp_occ_tables_matches_oracle(tmp_path, size, seed):
    """bwa v1's own SMEM collection (mem_collect_intv over bwt_smem1/bwt_seed_strategy1) running on a
    bwt_t rebuilt from bwa-mem2 CP_OCC tables equals the oracle per read -- this is what makes it a
    'reference'-kind CPU baseline over the GPU-built index. Sizes put the sentinel row and the table's
    end at different places of the 16-base words the word-level packing writes."""
    lib = fmi_util.ref_bwa()
    if lib is None:
        pytest.skip("oracle/_ref/libref_bwa.so not built")
    ref = gen.fmi_reference(size, seed=seed, repeat_frac=0.2)
    p = str(tmp_path / "o.bwt.2bit.64")
    oi = fmi_util.OracleIndex(ref, path_out=p)
    n, _, sent = oi.info()
    raw = np.fromfile(p, np.uint8)
    sz = (n >> 6) + 1
    cp = raw[48:48 + sz * 64].view(np.int64).reshape(sz, 8)
    bwt = fmi_util.bwa_from_tables(lib, n, sent, cp)
    codes, lens = gen.fmi_reads(ref, 600, seed=seed + 1, read_len=min(151, size // 4), sub_rate=0.02)
    got = fmi_util.bwa_smems(lib, bwt, codes, lens)
    exp, _, _ = oi.run(codes, lens, batch_size=512)
    assert got == fmi_util.per_read(exp, len(lens))
    assert fmi_util.bwa_collect_threaded(lib, bwt, codes, lens, 3) == len(exp)
    lib.ref_bwa_free(bwt)
    oi.close()


def test_packed_layouts_above_2_32():
    """The search's 16-byte `prev` entries and Occ32 count words (csrc/fmi_index.h) hold row values up
    to 2^34 - 1, i.e. indexes of > 2^32 BWT rows (a human genome's 6.2 G rows): host round trip
    through the same inline functions the kernels use (gb_fmi_debug_pack, no device work)."""
    import ctypes
    from genomicsbench_palisade_amd import lib
    L = lib()
    L.gb_fmi_debug_pack.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4
    rng = np.random.default_rng(5)
    top = (1 << 34) - 1
    rows = np.array([0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 12345, 6_200_000_001, top - 1, top],
                    np.int64)
    n = 400
    ent = np.zeros((n, 5), np.int64)
    ent[:, :3] = rng.choice(rows, size=(n, 3))
    ent[: len(rows), 0] = rows
    ent[: len(rows), 1] = rows[::-1]
    ent[: len(rows), 2] = rows
    ent[:, 3] = rng.integers(0, 1 << 13, n)
    ent[:, 4] = rng.integers(0, 1 << 13, n)
    cnt = rng.choice(rows, size=(n, 3)).astype(np.int64)
    eo, co = np.zeros_like(ent), np.zeros_like(cnt)
    assert L.gb_fmi_debug_pack(n, ent.ctypes.data, eo.ctypes.data, cnt.ctypes.data, co.ctypes.data) == 0
    assert (eo == ent).all() and (co == cnt).all()
