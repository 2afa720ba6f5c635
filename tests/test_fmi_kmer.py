"""gb_kmer_count / gb_kmer_index (include/gb_fmi_kmer.h) against tests/golden/kmer_golden.npz, which holds what the
live reference (Flye's KmerCounter and VertexIndex) gave for every set, and against the restatement tests/kmer_ref.py.
Without a GPU the host path (GB_KMER_HOST=1) and the restatement are checked; the device tests repeat the fixture
bit for bit and add a second set, a shuffled read order, two runs and LDS poisoning."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import kmer_ref
import kmer_sets
from conftest import GOLDEN, ROOT
from genomicsbench_palisade_amd import GbError, gen, kmer, lib


@pytest.fixture(scope="module")
def fx():
    z, sets = kmer_sets.load(os.path.join(GOLDEN, "kmer_golden.npz"))
    return {"z": z, "sets": sets, "by_name": {s.name: s for s in sets}}


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_KMER_HOST", "1")
    monkeypatch.delenv("GB_KMER_WS", raising=False)
    return monkeypatch


@pytest.fixture
def device(monkeypatch):
    from genomicsbench_palisade_amd import set_device
    monkeypatch.delenv("GB_KMER_HOST", raising=False)
    monkeypatch.delenv("GB_KMER_WS", raising=False)
    set_device(0)
    return monkeypatch


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and (a == b).all(), what


def check_index(got, codes, off, pos, rep, rep_freq, what):
    same(got.codes, codes, f"{what}: codes")
    same(got.off, off, f"{what}: offsets")
    same(got.pos, pos, f"{what}: positions")
    same(got.rep_codes, rep, f"{what}: repetitive codes")
    assert got.repetitive_frequency == rep_freq, what


def check_set(s, what=""):
    """Counts, statistics, histogram, getFreq and every index of one stored set, bit for bit."""
    h = kmer.count(s.k, (s.data, s.seq_off))
    codes, counts = h.export()
    same(codes, s.expect("codes"), f"{what}{s.name}: codes")
    same(counts, s.expect("counts"), f"{what}{s.name}: counts")
    assert h.stats() == s.stats, (s.name, h.stats(), s.stats)
    same(h.hist(32), s.hist, f"{what}{s.name}: histogram")
    if len(codes):
        fwd = np.concatenate([kmer_ref.codes_of(r, s.k)[0] for r in s.reads])
        near = np.concatenate([codes[::11] + np.uint64(1), np.array([0, (1 << (2 * s.k)) - 1], np.uint64)])
        absent = np.setdiff1d(near, codes)
        q = np.concatenate([codes[::7], fwd[::5], absent])
        same(h.freq(q), kmer_ref.freq(codes, counts, q), f"{what}{s.name}: freq")
    for i, p in enumerate(s.params):
        got = h.index(*p)
        n_codes, n_entries, n_rep, rep_freq = s.scalars(i)
        check_index(got, s.expect(f"idx{i}_codes"), s.expect(f"idx{i}_off"), s.expect(f"idx{i}_pos"),
                    s.expect(f"idx{i}_rep"), rep_freq, f"{what}{s.name} {p}")
        assert (len(got.codes), len(got.pos), len(got.rep_codes)) == (n_codes, n_entries, n_rep)
    h.close()


def test_fixture_has_every_label(fx):
    z = fx["z"]
    names, counts = [str(n) for n in z["label_names"]], z["label_counts"]
    assert names == list(kmer_sets.LABELS)
    assert (counts > 0).all(), [n for n, c in zip(names, counts) if c <= 0]
    assert {s.k for s in fx["sets"]} >= set(kmer_sets.KS)
    assert os.path.getsize(os.path.join(GOLDEN, "kmer_golden.npz")) <= 400 * 1024


def test_restatement_equals_every_stored_value(fx):
    for s in fx["sets"]:
        r = s.restated()
        st = kmer_ref.stats(r["codes"], r["counts"])
        assert st == s.stats, s.name
        same(kmer_ref.hist(r["counts"], 32), s.hist, s.name)
        for name in r:
            if not name.endswith("rep_freq"):
                same(r[name], s.expect(name), f"{s.name}/{name}")
        for i in range(len(s.params)):
            assert r[f"idx{i}_rep_freq"] == s.scalars(i)[3]


def test_de_bruijn_analytically(fx, host):
    """B(4, 6): every 6-mer once, so 2 016 canonical codes twice and the 64 palindromes once."""
    s = fx["by_name"]["de_bruijn"]
    h = kmer.count(6, (s.data, s.seq_off))
    codes, counts = h.export()
    assert len(codes) == 2080 and (counts == 2).sum() == 2016 and (counts == 1).sum() == 64
    fwd, rc = kmer_ref.codes_of(s.reads[0], 6)
    same(np.sort(codes[counts == 1]), np.sort(fwd[fwd == rc]), "palindromes")
    assert h.stats() == {"n_distinct": 2080, "n_occurrences": 4096, "n_over15": 0, "max_count": 2}


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_equals_fixture(fx, host, threads):
    host.setenv("GB_KMER_THREADS", threads)
    for s in fx["sets"]:
        check_set(s, "host ")


def test_the_walk_ends_one_kmer_before_the_read(host):
    """The reference's IterKmers: a read of L bases has L - k k-mers, so the last one is not counted."""
    h = kmer.count(3, [b"ACGTTGCA", b"ACG", b"", b"GGGA"])
    codes, counts = h.export()
    # live Flye on these four reads (count(true) and count(false)): {1: 1, 6: 2, 16: 1, 21: 1, 36: 1}
    assert dict(zip(codes.tolist(), counts.tolist())) == {1: 1, 6: 2, 16: 1, 21: 1, 36: 1}
    assert h.freq([6, 27, 40, 63]).tolist() == [2, 0, 0, 0]  # 27 = CGT, the non-canonical form of ACG


def test_palindrome_stays_forward(host):
    h = kmer.count(4, [b"ATATCC"])
    got = h.index(1, 0.4, 0, 100.0)
    code = 0b00110011  # ATAT
    assert code in got.codes.tolist()
    pos = got.pos[got.off[got.codes.tolist().index(code)]]
    assert kmer.locate(h.seq_off, [pos])[1][0] == 0


def test_locate():
    off = np.array([5, 9, 9, 12], np.int64)
    read, strand, offset = kmer.locate(off, [0, 3, 4, 7, 8, 10, 11, 13])
    assert read.tolist() == [0, 0, 0, 0, 2, 2, 2, 2]
    assert strand.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert offset.tolist() == [0, 3, 0, 3, 0, 2, 0, 2]


def _count_raw(k, data, off, n_seqs=None, n_bytes=None):
    L = kmer._decl()
    out = ctypes.c_void_p(0xDEAD)
    st = L.gb_kmer_count(k, data.ctypes.data, len(data) if n_bytes is None else n_bytes, off.ctypes.data,
                         len(off) - 1 if n_seqs is None else n_seqs, ctypes.byref(out))
    return st, out.value, lib().gb_last_error().decode()


REFUSALS = [
    ("k_0", dict(k=0), ["k = 0"]),
    ("k_32", dict(k=32), ["k = 32"]),
    ("offsets_decrease", dict(off=[0, 8, 6, 12]), ["read 1", "8..6"]),
    ("offsets_leave", dict(off=[0, 4, 8, 13]), ["read 2", "8..13", "12 bytes"]),
    ("bad_byte", dict(data=b"ACGTACNTACGT"), ["read 1", "0x4e", "position 2"]),
    ("budget", dict(env={"GB_KMER_WS": "100"}, device=True), ["need", "bytes", "budget of 100"]),
    ("budget_text", dict(env={"GB_KMER_WS": "lots"}, device=True), ["GB_KMER_WS", "lots"]),
]


@pytest.mark.parametrize("name,change,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_first_and_leave_the_outputs(monkeypatch, name, change, words):
    """GB_ERR_ARG before any device work (the budget cases run without GB_KMER_HOST: the budget is checked before a
    device is looked for), *out untouched, the item named."""
    if change.get("device"):
        monkeypatch.delenv("GB_KMER_HOST", raising=False)
    else:
        monkeypatch.setenv("GB_KMER_HOST", "1")
    for key, v in change.get("env", {}).items():
        monkeypatch.setenv(key, v)
    data = np.frombuffer(change.get("data", b"ACGTACGTACGT"), np.uint8).copy()
    off = np.array(change.get("off", [0, 4, 8, 12]), np.int64)
    st, out, msg = _count_raw(change.get("k", 3), data, off)
    assert st == -1 and out == 0xDEAD, (st, out, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_a_count_that_could_pass_uint32_is_refused(host):
    """More than GB_KMER_MAX_OCC occurrences: the offsets describe 2^31 + 1 k-mers of one read. The refusal comes
    from the offsets alone, before any byte is read: the array is zero pages that are never touched."""
    n = (1 << 31) + 4
    data = np.zeros(n, np.uint8)
    st, out, msg = _count_raw(3, data, np.array([0, n], np.int64))
    assert st == -1 and out == 0xDEAD and "could pass uint32" in msg, msg


def test_index_refusals(host):
    h = kmer.count(3, [b"ACGTTGCAGG"])
    for args, word in (((0, 0.4, 0, 2.0), "min_freq"), ((1, 0.0, 0, 2.0), "select_rate"),
                       ((1, 1.0, 0, 2.0), "select_rate"), ((1, 0.4, 0, -1.0), "repeat_rate")):
        with pytest.raises(GbError, match=word):
            h.index(*args)
    L = kmer._decl()
    codes, counts, used = np.full(2, 77, np.uint64), np.full(2, 77, np.uint32), ctypes.c_int64(-1)
    st = L.gb_kmer_counts_export(h._h, codes.ctypes.data, counts.ctypes.data, 2, ctypes.addressof(used))
    assert st == -1 and used.value == h.stats()["n_distinct"] > 2 and (codes == 77).all() and (counts == 77).all()


def test_empty_inputs_touch_no_device(monkeypatch):
    """No read, and no read longer than k: empty results, without GB_KMER_HOST and without a device."""
    monkeypatch.delenv("GB_KMER_HOST", raising=False)
    for reads in ([], [b"", b"ACG", b"AC"]):
        h = kmer.count(3, reads)
        assert h.stats() == {"n_distinct": 0, "n_occurrences": 0, "n_over15": 0, "max_count": 0}
        codes, counts = h.export()
        assert len(codes) == 0 and h.hist(4).tolist() == [0, 0, 0, 0] and h.freq([5]).tolist() == [0]
        got = h.index()
        assert len(got.codes) == 0 and got.off.tolist() == [0] and len(got.pos) == 0 and len(got.rep_codes) == 0


def test_exports_appear_in_libgb():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "genomicsbench_palisade_amd", "lib", "libgb.so")],
                         capture_output=True, text=True, check=True).stdout
    for f in ("gb_kmer_count", "gb_kmer_free", "gb_kmer_counts_stats", "gb_kmer_counts_export", "gb_kmer_counts_freq",
              "gb_kmer_counts_hist", "gb_kmer_index", "gb_kmer_idx_free", "gb_kmer_idx_stats", "gb_kmer_idx_export",
              "gb_kmer_timing", "gb_kmer_plan"):
        assert f" T {f}\n" in out, f


def _fasta(path, reads, fastq=False):
    with (gzip.open(path, "wt") if path.endswith(".gz") else open(path, "w")) as f:
        for i, r in enumerate(reads):
            s = bytes(r).decode()
            if fastq:
                f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
            else:
                f.write(f">r{i} generated\n")
                for j in range(0, len(s), 60):
                    f.write(s[j:j + 60] + "\n")


def _driver_lines(reads, k, min_len):
    kept = [r for r in reads if len(r) > min_len]
    codes, counts = kmer_ref.count(k, kept)
    st = kmer_ref.stats(codes, counts)
    lines = [f"Hash size: {st['n_over15']}", f"Total k-mers {st['n_distinct']}"]
    h = np.bincount(counts.astype(np.int64)) if len(counts) else np.zeros(1, np.int64)
    return lines + [f"{f}\t{n}" for f, n in enumerate(h.tolist()) if n and f]


def test_bin_kmer_cnt_prints_the_reference_lines(tmp_path):
    """FASTA, a gz copy and FASTQ give the restatement's lines, and the length filter is strict: a read of exactly
    max(min-read, min-ovlp) bases is left out."""
    exe = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "kmer-cnt")
    assert os.path.exists(exe), f"{exe} not built (make)"
    reads = gen.kmer_reads(5, 3000, 6, (40, 160), 0.02, 2)
    reads += [reads[0][:50].copy(), reads[1][:51].copy()]
    env = dict(os.environ, GB_KMER_HOST="1")
    want = _driver_lines(reads, 11, 50)
    assert len([r for r in reads if len(r) == 50]) >= 1
    for name, fastq in (("a.fasta", False), ("a.fasta.gz", False), ("a.fastq", True)):
        path = str(tmp_path / name)
        _fasta(path, reads, fastq)
        out = subprocess.run([exe, "--reads", path, "--kmer", "11", "--min-read", "50", "--min-ovlp", "20"], env=env,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.splitlines() == want, name
    # two files, and the overlap as the larger bound
    _fasta(str(tmp_path / "b.fasta"), reads[:7])
    out = subprocess.run([exe, "--reads", f"{tmp_path / 'a.fasta'},{tmp_path / 'b.fasta'}", "--kmer", "11",
                          "--min-read", "10", "--min-ovlp", "60"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == _driver_lines(reads + reads[:7], 11, 60), out.stderr


def test_generator_is_seeded():
    a = gen.kmer_reads(3, 2000, 4, (50, 100), 0.05, 1)
    b = gen.kmer_reads(3, 2000, 4, (50, 100), 0.05, 1)
    assert len(a) == len(b) > 10 and all((x == y).all() for x, y in zip(a, b))
    assert all(50 <= len(r) <= 100 and np.isin(r, np.frombuffer(b"ACGT", np.uint8)).all() for r in a)
    assert abs(sum(len(r) for r in a) - 4 * 2000) <= 100


# ------------------------------------------------------------------------------------------------------- device

@pytest.mark.gpu
def test_device_equals_fixture(fx, device):
    for s in fx["sets"]:
        check_set(s, "device ")


@pytest.fixture(scope="module")
def second_set():
    """About 2 M occurrences at k = 17 with the host path's results."""
    reads = gen.kmer_reads(11, 40000, 50, (500, 3000), 0.03, 3)
    data, off = kmer.pack_reads(reads)
    os.environ["GB_KMER_HOST"] = "1"
    try:
        h = kmer.count(17, (data, off))
        out = {"data": data, "off": off, "counts": h.export(), "stats": h.stats(), "hist": h.hist(64),
               "index": [h.index(*p) for p in ((1, 0.4, 0, 100.0), (2, 0.4, 3, 2.0))]}
        h.close()
    finally:
        del os.environ["GB_KMER_HOST"]
    return out


@pytest.mark.gpu
def test_device_equals_host_on_a_second_set(second_set, device):
    s = second_set
    assert 1_500_000 <= s["stats"]["n_occurrences"] <= 2_500_000
    h = kmer.count(17, (s["data"], s["off"]))
    codes, counts = h.export()
    same(codes, s["counts"][0], "codes")
    same(counts, s["counts"][1], "counts")
    assert h.stats() == s["stats"]
    same(h.hist(64), s["hist"], "histogram")
    for p, e in zip(((1, 0.4, 0, 100.0), (2, 0.4, 3, 2.0)), s["index"]):
        check_index(h.index(*p), e.codes, e.off, e.pos, e.rep_codes, e.repetitive_frequency, f"second set {p}")
    t = kmer.timing()
    assert t["occurrences"] == s["stats"]["n_occurrences"]
    assert all(t[x] > 0 for x in ("pack", "extract", "sort", "reduce", "lookup", "select", "fill")), t
    assert kmer.plan()[:2] == (kmer_sets.TILE, 5)


@pytest.mark.gpu
def test_device_under_another_read_order(fx, device):
    """Counts are unchanged and positions follow the new offsets: the shuffled set equals the restatement."""
    s = fx["by_name"]["index_k11"]
    order = np.random.default_rng(7).permutation(len(s.reads))
    reads = [s.reads[i] for i in order]
    h = kmer.count(s.k, reads)
    codes, counts = h.export()
    same(codes, s.expect("codes"), "codes")
    same(counts, s.expect("counts"), "counts")
    for p in s.params[:2]:
        e = kmer_ref.index(s.k, reads, codes, counts, *p)
        check_index(h.index(*p), *e, f"shuffled {p}")


@pytest.mark.gpu
def test_device_tile_edge_totals(fx, device):
    tile = kmer.plan()[0]
    assert tile == kmer_sets.TILE
    totals = [tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1]
    for t in totals:
        s = fx["by_name"][f"total_{t}"]
        assert s.stats["n_occurrences"] == t
        check_set(s, "tile edge ")


@pytest.mark.gpu
def test_device_two_runs_give_identical_bytes(fx, device):
    s = fx["by_name"]["index_k13"]
    runs = []
    for _ in range(2):
        h = kmer.count(s.k, (s.data, s.seq_off))
        x = h.index(*s.params[0])
        runs.append([a.tobytes() for a in (*h.export(), h.hist(32), x.codes, x.off, x.pos, x.rep_codes)])
        h.close()
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_device_after_lds_poison(fx, device):
    """The sort's histograms and ranks, the scans' wave totals and the radix select go through LDS: the fixture once
    after every CU's LDS has been filled with each pattern of tests/cpp/lds_poison.hip."""
    path = os.path.join(ROOT, "tests", "_build", "liblds_poison.so")
    assert os.path.exists(path), f"{path} not built (make)"
    L = ctypes.CDLL(path)
    L.lds_poison.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    sets = [fx["by_name"][n] for n in ("edges_k8", "index_k4", "index_k13", "total_8193")]
    for mode, value in [(0, 0), (1, 0), (2, 2), (2, 37), (2, 300), (3, 1000), (4, 0)]:
        assert L.lds_poison(0, mode, value, 1) == 0
        for s in sets:
            check_set(s, f"pattern {(mode, value)} ")
