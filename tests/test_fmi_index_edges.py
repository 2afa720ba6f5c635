"""The fmi path at the index's own edges: the builder (csrc/fmi_build.hip), the Occ32 search layout
(csrc/fmi_index.h, compress_occ and the kernels of csrc/fmi.hip, csrc/fmi_wave.h, csrc/fmi_tasks.hip)
and the SA walk (csrc/fmi_sa.hip) on references chosen for where they put the sentinel row, the end
of the last block and the last sampled row, on texts shorter than the 21-mer sort key and texts the
key cannot resolve, and with reads whose intervals start and end at the sentinel row.

tests/fmi_index_shapes.py makes the inputs and an independent brute-force index. The CPU tests pin
the oracle's build to that index and assert, through the oracle's edge counters, that the inputs
reach every edge they are meant for; the GPU tests are exact against the oracle."""
import ctypes

import numpy as np
import pytest

import fmi_index_shapes as shapes
import fmi_util
from fmi_index_shapes import CATALOGUE, NAMES, PLANTED, SENTINEL_NAMES, STAGGERED, WIDE_NAMES

FIELDS = ("rid", "m", "n", "k", "l", "s")
SENTINEL_EDGES = ("sp_eq_z", "sp_eq_z1", "ep_eq_z", "ep_eq_z1", "t_at_edge")
BLOCK_EDGES = ("sp_y0", "sp_y32", "sp_y63", "ep_y0", "ep_y32", "ep_y63", "ep_eq_n", "same_block", "diff_block",
               "sp_zblock_above", "ep_zblock_below")
WALK_EDGES = ("sa_start_z", "sa_reach_z", "sa_step_from_z1", "sa_t_step", "sa_end_row0", "sa_end_last")
DEGENERATE_SEEDS = (1, 3, 19)
TINY = ("random_1", "random_2", "random_3")
gpu = pytest.mark.gpu


# ------------------------------------------------------------------ the oracle side, shared
class Entry:
    """One catalogue reference: its oracle index, the oracle's index file and that file's tables, and
    the oracle's answers computed so far (each once, then shared unchanged)."""

    def __init__(self, name, path):
        self.name, self.path = name, path
        self.ref = CATALOGUE[name]
        self.oi = fmi_util.OracleIndex(self.ref, path_out=path)
        self.n, self.count, self.z = self.oi.info()
        _, self.count_file, self.cp, self.sa64, sentinel = fmi_util.read_index_file(path)
        assert sentinel == self.z
        self.bytes = open(path, "rb").read()
        self.memo = {}

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def sentinel_reads(self):
        return self.once("sentinel_reads", lambda: shapes.sentinel_reads(self.ref, self.oi))

    def degenerate_reads(self):
        return self.once("degenerate_reads", lambda: shapes.degenerate_reads(self.ref))

    def search(self, kind, min_seed):
        """(SMEMs, per-batch counts, per-phase counts, backwardExt calls, edge counters) of the oracle's
        run over this entry's `kind` reads."""
        def make():
            codes, lens = getattr(self, kind)()
            self.oi.edges()
            c0 = self.oi.bwt_calls()
            sm, bc, pc = self.oi.run(codes, lens, batch_size=512, min_seed_len=min_seed)
            return sm, bc, pc, self.oi.bwt_calls() - c0, self.oi.edges()
        return self.once((kind, min_seed), make)

    def sa_all(self, mode):
        """(the oracle's SA lookup of every row, its edge counters)."""
        def make():
            self.oi.edges()
            return self.oi.sa_lookup(np.arange(self.n), mode), self.oi.edges()
        return self.once(("sa_all", mode), make)


@pytest.fixture(scope="module")
def entries(tmp_path_factory):
    d = tmp_path_factory.mktemp("fmi_index_edges")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Entry(name, str(d / f"{name}.oracle.bwt.2bit.64"))
        return made[name]
    yield get
    for e in made.values():
        e.oi.close()


# ------------------------------------------------------------------ CPU: the inputs and the oracle
@pytest.mark.parametrize("name", NAMES)
def test_oracle_build_equals_brute_force(entries, name):
    """The oracle's index (prefix doubling in C) equals the one derived from Python's sort of the
    suffixes: n, count, sentinel row, every CP_OCC line, the sampled SA, and the SA value its LF walk
    gives every row; the call_one_step variant differs only where the walk meets the sentinel row after
    at least one step, where it answers 0."""
    e = entries(name)
    b = shapes.Brute(e.ref)
    assert e.oi.info() == b.info()
    assert e.count_file.tolist() == [c - 1 for c in b.count]
    assert e.cp.shape == b.cp.shape and (e.cp == b.cp).all()
    assert (e.sa64 == b.sa_sampled).all()
    assert len(e.bytes) == 8 + 40 + ((e.n >> 6) + 1) * 64 + ((e.n >> 3) + 1) * 5 + 8
    sa0, sa1 = e.sa_all(0)[0], e.sa_all(1)[0]
    assert (sa0 == b.sa_lookup(0)).all() and (np.sort(sa0) == np.arange(e.n)).all()
    assert (sa1 == b.sa_lookup(1)).all()
    assert ((sa1 == sa0) | (sa1 == 0)).all()


def test_catalogue_shapes():
    """What the catalogue is for: n & 63 in {63, 1, 3} (the last block nearly full and nearly empty),
    references below, at and above the 21-mer key, G % 4 == 0 (the last row is a sampled row), and the
    homopolymers' sentinel rows at row 1 and at the last row."""
    n_of = {name: 2 * len(ref) + 1 for name, ref in CATALOGUE.items()}
    assert {n_of[f"random_{G}"] & 63 for G in (31, 32, 33)} == {63, 1, 3}
    assert set(shapes.RANDOM_G) >= {1, 2, 3, 10, 20, 21, 22}  # 2 G below, and G around, the 21 bases of the key
    assert any(((n - 1) & 7) == 0 for n in n_of.values()) and any(((n - 1) & 7) != 0 for n in n_of.values())
    for G in shapes.HOMO_G:
        for b in "AC":
            assert shapes.Brute(CATALOGUE[f"homo_{b}_{G}"]).sentinel == 1
        for b in "GT":
            assert shapes.Brute(CATALOGUE[f"homo_{b}_{G}"]).sentinel == 2 * G
    acgt = CATALOGUE["acgt_x100"]
    assert (shapes.revcomp(acgt) == acgt).all() and shapes.Brute(acgt).sentinel == 200
    x = CATALOGUE["x_revcomp_x"]
    assert (shapes.revcomp(x) == x).all()


def test_planted_seed_classes(entries):
    """The seed table puts the sentinel row where its names say (a change to the generator would move
    them silently otherwise)."""
    for name, (seed, cls) in PLANTED.items():
        e = entries(name)
        assert (e.ref == shapes.planted(shapes.PLANTED_G, seed)).all()
        assert shapes.planted_class_holds(cls, e.n, e.z), (name, e.n, e.z)
        # the sentinel's suffix has neighbours on both sides
        assert 0 < e.z - 1 and e.z + 1 < e.n


@pytest.mark.parametrize("name", SENTINEL_NAMES)
def test_sentinel_reads_reach_the_sentinel(entries, name):
    """sentinel_reads makes backwardExt calls whose interval starts or ends at the sentinel row and at
    the row after it, T extensions among them. A condition on the inputs: if it fails, change them."""
    e = entries(name)
    codes, _ = e.sentinel_reads()
    assert len(codes) == 4680
    sm, _, _, _, edges = e.search("sentinel_reads", 19)
    assert len(sm) > 0
    for k in SENTINEL_EDGES:
        assert edges[k] > 0, (k, edges)


def test_edge_counters_are_per_handle_and_cleared_by_reading(entries):
    """edges() reads and clears; the handles that run_threaded shares out (the timed CPU baselines of
    bench.py run on such handles) give the same SMEMs and count nothing, on themselves or on the
    handle they were shared from."""
    e = entries("planted_z64_0")
    codes, lens = e.sentinel_reads()
    sm = e.search("sentinel_reads", 19)[0]
    e.oi.edges()
    assert not any(e.oi.edges().values())
    tot, _, parts = e.oi.run_threaded(codes, lens, 3, collect=True)
    got = np.concatenate(parts)
    assert tot == len(sm) and all((got[f] == sm[f]).all() for f in FIELDS)
    assert not any(e.oi.edges().values())
    e.oi.run(codes[:64], lens[:64], batch_size=512, min_seed_len=19)
    first = e.oi.edges()
    assert first["same_block"] + first["diff_block"] > 0 and not any(e.oi.edges().values())


def test_staggered_references_put_the_sentinel_at_an_interval_end(entries):
    """backwardExt's sentinel offset is k <= z && k + s > z. Where the interval is the sentinel row
    alone every extension is empty, and where the row is strictly inside both comparisons are far from
    equality: on the planted references, whose three copies all leave the text at base 40, no call has
    sp == z (or ep == z + 1) with two or more rows, so `<` for `<=` would change nothing there. The
    staggered references are what makes those calls."""
    for name, (seed, low) in STAGGERED.items():
        e = entries(name)
        assert (e.ref == shapes.staggered(shapes.PLANTED_G, seed, low)).all()
        edges = e.search("sentinel_reads", 19)[4]
        assert edges["sp_eq_z_wide" if low else "ep_eq_z1_wide"] > 0, edges


def test_catalogue_reaches_block_and_walk_edges(entries):
    """Over the whole catalogue, the searches the GPU tests run (degenerate reads at three seed
    lengths, sentinel reads on the planted references) make backwardExt calls at rows 0, 32 and 63 of
    a block on either end of the interval, with the interval ending at the last row, inside one block
    and across two, and on either side of the sentinel within its block; the all-rows SA lookups start
    at the sentinel, reach it, step from the row after it, step over T, and end at the first and the
    last sampled row. Conditions on the inputs."""
    tot = dict.fromkeys(fmi_util.EDGE_NAMES, 0)
    most = 0
    for name in NAMES:
        e = entries(name)
        runs = [e.search("degenerate_reads", ms) for ms in DEGENERATE_SEEDS]
        if name in SENTINEL_NAMES:
            runs.append(e.search("sentinel_reads", 19))
        for sm, _, _, _, edges in runs:
            most = max(most, int(np.bincount(sm["rid"]).max()) if len(sm) else 0)
            for k, v in edges.items():
                tot[k] += v
        for mode in (0, 1):
            for k, v in e.sa_all(mode)[1].items():
                tot[k] += v
    for k in BLOCK_EDGES + WALK_EDGES + SENTINEL_EDGES:
        assert tot[k] > 0, (k, tot)
    assert 40 < most < 2048  # reads promoted to a big slot, none above its capacity


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def fmi():
    from genomicsbench_palisade_amd import fmi, set_device
    set_device(0)
    return fmi


class Bed:
    """The device side of one entry: the index built on the device (written next to the oracle's file)
    and the oracle's file loaded."""

    def __init__(self, fmi, e):
        self.e = e
        self.built_path = e.path.replace(".oracle.", ".built.")
        self.built = fmi.Index.build(e.ref, out_path=self.built_path)
        self.loaded = fmi.Index.load(e.path)

    def close(self):
        self.built.close()
        self.loaded.close()


@pytest.fixture(scope="module")
def beds(fmi, entries):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Bed(fmi, entries(name))
        return made[name]
    yield get
    for b in made.values():
        b.close()


def assert_index_equals_oracle(idx, path, e):
    assert open(path, "rb").read() == e.bytes
    assert idx.info() == (e.n, e.count, e.z)
    assert (idx.cp_occ() == e.cp).all()
    assert (idx.sampled_sa() == e.sa64).all()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_build_bit_exact(beds, name):
    """Index.build writes the oracle's file byte for byte and keeps the same tables on the device."""
    b = beds(name)
    assert_index_equals_oracle(b.built, b.built_path, b.e)


@gpu
@pytest.mark.parametrize("name", WIDE_NAMES)
def test_build_wide_rows_bit_exact(fmi, entries, monkeypatch, tmp_path, name):
    """The same with 64-bit suffix-array rows (the builder's path above 2^31 rows)."""
    monkeypatch.setenv("GB_FMI_BUILD_WIDE", "1")
    e = entries(name)
    p = str(tmp_path / "w.bwt.2bit.64")
    idx = fmi.Index.build(e.ref, out_path=p)
    assert_index_equals_oracle(idx, p, e)
    idx.close()


def build_chunked(fmi, e, monkeypatch, tmp_path, chunk):
    if chunk is None:
        monkeypatch.delenv("GB_FMI_BUILD_CHUNK", raising=False)
    else:
        monkeypatch.setenv("GB_FMI_BUILD_CHUNK", str(chunk))
    p = str(tmp_path / f"c{chunk}.bwt.2bit.64")
    idx = fmi.Index.build(e.ref, out_path=p)
    assert_index_equals_oracle(idx, p, e)
    idx.close()


@gpu
def test_build_chunk_exactly_one_prefix_bin(fmi, entries, monkeypatch, tmp_path):
    """A chunk of exactly the largest 8-base prefix bin (the A run's suffixes that start with eight
    A's) holds it; one row less is refused, and the next build on the same process is exact again."""
    from genomicsbench_palisade_amd import GbError
    e = entries("homo_A_300")
    big = shapes.largest_prefix_bin(e.ref)
    assert 64 < big < 2 * 300  # above the floor of the chunk setting, and more than one chunk in the text
    build_chunked(fmi, e, monkeypatch, tmp_path, big)
    monkeypatch.setenv("GB_FMI_BUILD_CHUNK", str(big - 1))
    with pytest.raises(GbError, match="share one 8-base prefix"):
        fmi.Index.build(e.ref)
    build_chunked(fmi, e, monkeypatch, tmp_path, None)


@gpu
@pytest.mark.parametrize("chunk", [65, 64])
def test_build_chunk_ends_inside_tied_pairs(fmi, entries, monkeypatch, tmp_path, chunk):
    """x + revcomp(x) is its own reverse complement, so the text is the reference twice and every
    suffix ties with its copy until the doubling distance reaches G: an odd or even chunk length puts
    chunk ends inside pairs, which are cut back to the pair's first row."""
    e = entries("x_revcomp_x")
    assert shapes.largest_prefix_bin(e.ref) <= 64
    build_chunked(fmi, e, monkeypatch, tmp_path, chunk)


@gpu
@pytest.mark.parametrize("name", ["at_x150", "cgg_500"])
def test_build_chunk_of_largest_bin_on_tandems(fmi, entries, monkeypatch, tmp_path, name):
    """Short-period tandem texts with the chunk at their largest prefix bin."""
    e = entries(name)
    big = shapes.largest_prefix_bin(e.ref)
    assert big >= 64
    build_chunked(fmi, e, monkeypatch, tmp_path, big)


def sa_debug_calls():
    from genomicsbench_palisade_amd import check, lib
    L = lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_fmi_sa_raw.argtypes = [vp, vp, i64, vp]
    L.gb_fmi_sa_one_step.argtypes = [vp, i64, vp, vp, vp]
    return L, check


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_sa_walk_every_row(fmi, beds, name):
    """Every row's SA value in both modes, every raw sample, one call_one_step from every row, and
    hand-made intervals (every row, the sentinel row alone and with its neighbours, the rows after it,
    and widths around max_occ and 2 max_occ that end at the last row), on the built index and on the
    oracle's file loaded."""
    b = beds(name)
    e = b.e
    L, check = sa_debug_calls()
    rows = np.arange(e.n)
    smems = shapes.edge_smems(e.n, e.z)
    exp = {(mo, mode): e.once(("edge_smems", mo, mode), lambda: e.oi.sa_entries(smems[mo], max_occ=mo, mode=mode))
           for mo in smems for mode in (0, 1)}
    steps = e.once("one_step", lambda: [fmi_util.call_one_step(e.count, e.cp, e.sa64, int(r), int(r) % 3)
                                        for r in rows])
    for idx in (b.built, b.loaded):
        for mode in (fmi.SA_COMPRESSED, fmi.SA_PREFETCH):
            assert (idx.sa_lookup(rows, mode) == e.sa_all(mode)[0]).all(), mode
        pos = np.arange(len(e.sa64), dtype=np.int64)
        raw = np.zeros(len(pos), np.int64)
        check(L.gb_fmi_sa_raw(idx.h, pos.ctypes.data, len(pos), raw.ctypes.data), "gb_fmi_sa_raw")
        assert (raw == e.sa64).all()
        for r in rows.tolist():
            entry, off, done = ctypes.c_int64(), ctypes.c_int64(r % 3), ctypes.c_int32()
            check(L.gb_fmi_sa_one_step(idx.h, r, ctypes.byref(entry), ctypes.byref(off), ctypes.byref(done)),
                  "gb_fmi_sa_one_step")
            assert (done.value, entry.value, off.value) == steps[r], r
        for (mo, mode), (ec, en) in exp.items():
            c, cnt = idx.sa_entries(smems[mo], max_occ=mo, mode=mode)
            assert (cnt == en).all() and len(c) == len(ec) and (c == ec).all(), (mo, mode)


def assert_search_exact(rs, exp):
    sm_e, bc_e, pc_e, calls_e, _ = exp
    sm, tot, bc, pc = rs.results(batch_size=512)
    assert tot == len(sm_e)
    assert (bc == bc_e).all() and (pc == pc_e).all()
    for f in FIELDS:
        assert (sm[f] == sm_e[f]).all(), f
    assert rs.timing()[2] == calls_e


def assert_sa_runs_exact(rs, e, key):
    sm_e = e.memo[key][0]
    for mo, mode in ((500, 1), (3, 0)):
        ec, en = e.once(key + ("sa", mo, mode), lambda: e.oi.sa_entries(sm_e, max_occ=mo, mode=mode))
        rs.sa_run(max_occ=mo, mode=mode)
        c, cnt, tot = rs.sa_results()
        assert tot == len(ec) and (cnt == en).all() and (c == ec).all(), (mo, mode)


@gpu
@pytest.mark.parametrize("heavy", ["", "1"])
@pytest.mark.parametrize("name", SENTINEL_NAMES)
def test_search_at_the_sentinel(fmi, beds, monkeypatch, name, heavy):
    """Reads whose intervals start and end at the sentinel row and the row after it, by the lane
    kernel and (GB_FMI_HEAVY=1: every read handed over after one backwardExt call) by smem_heavy, then
    the SA coordinates of their SMEMs."""
    if heavy:
        monkeypatch.setenv("GB_FMI_HEAVY", heavy)
    b = beds(name)
    e = b.e
    codes, lens = e.sentinel_reads()
    exp = e.search("sentinel_reads", 19)
    rs = fmi.Reads(b.built, codes, lens)
    rs.search(19)
    assert_search_exact(rs, exp)
    if heavy:
        assert rs.ctl()[4] > 0
    assert_sa_runs_exact(rs, e, ("sentinel_reads", 19))
    rs.close()


@gpu
@pytest.mark.parametrize("nthreads", [1, 3])
@pytest.mark.parametrize("name", SENTINEL_NAMES)
def test_get_smems_at_the_sentinel(beds, name, nthreads):
    """FMI_search::getSMEMs (the task kernels of csrc/fmi_tasks.hip) over the same reads."""
    b = beds(name)
    e = b.e
    codes, _ = e.sentinel_reads()

    def make():
        c0 = e.oi.bwt_calls()
        sm = e.oi.get_smems(codes, len(codes), 19, nthreads)
        return sm, e.oi.bwt_calls() - c0
    sm_e, calls_e = e.once(("get_smems", nthreads), make)
    got, calls = b.built.get_smems(codes, len(codes), 19, nthreads)
    assert len(sm_e) > 0 and len(got) == len(sm_e)
    for f in FIELDS:
        assert (got[f] == sm_e[f]).all(), f
    assert calls == calls_e


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_search_on_degenerate_indexes(fmi, beds, name):
    """Windows of the text, the text tiled past its end, reads with an N, short and random reads, at
    min_seed_len 1, 3 and 19, on indexes of one block, homopolymers, tandems and self-complementary
    texts; the built and the loaded index for the three smallest."""
    b = beds(name)
    e = b.e
    codes, lens = e.degenerate_reads()
    for idx in (b.built, b.loaded) if name in TINY else (b.built,):
        rs = fmi.Reads(idx, codes, lens)
        for min_seed in DEGENERATE_SEEDS:
            exp = e.search("degenerate_reads", min_seed)
            rs.search(min_seed)
            assert_search_exact(rs, exp)
            assert rs.ctl()[2] == 0
            if len(exp[0]):
                assert_sa_runs_exact(rs, e, ("degenerate_reads", min_seed))
        rs.close()
