"""gb_dbg_assemble (include/gb_fmi_dbg.h) against tests/golden/dbg_golden.npz, which holds what the live reference
(benchmarks/dbg/debruijn.cpp behind tests/golden/dbg_live_shim.cpp) built for every fixture region, and against the
restatement tests/dbg_ref.py. Without a GPU the host path (GB_DBG_HOST=1) and the restatement are checked; the device
tests repeat the fixture bit for bit and add a second set, a permuted order, chunks, weakened fingerprints, two runs,
LDS poisoning and keep = 0."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dbg_ref
import dbg_sets
from conftest import GOLDEN, ROOT
from genomicsbench_palisade_amd import dbg, gen, lib

NPZ = os.path.join(GOLDEN, "dbg_golden.npz")
SUMMARY_FIELDS = ("k", "n_graphs", "cyclic", "n_nodes", "n_edges", "n_ref_and_read", "node_weight_sum",
                  "edge_weight_sum")
REF40 = b"ACGTTGCAAGGCTTACCGATAGGCTCAATGCCGTAAGCTT"
ENV = ("GB_DBG_HOST", "GB_DBG_WS", "GB_DBG_FP_BITS", "GB_DBG_THREADS")


@pytest.fixture(scope="module")
def fx():
    z, sets = dbg_sets.load(NPZ)
    return {"z": z, "sets": sets, "by_name": {s.name: s for s in sets}}


@pytest.fixture
def host(monkeypatch):
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    monkeypatch.setenv("GB_DBG_HOST", "1")
    return monkeypatch


@pytest.fixture
def device(monkeypatch):
    from genomicsbench_palisade_amd import set_device
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    set_device(0)
    return monkeypatch


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), what


def check_set(s, what="", redone=0):
    """Summary and export of one stored set, bit for bit; returns the summaries."""
    a = dbg.assemble(s.regions, s.reads, s.params, keep=True)
    sm = a.summary()
    assert len(sm) == len(s)
    for i in range(len(s)):
        want = s.summary(i)
        got = {f: int(sm[f][i]) for f in SUMMARY_FIELDS}
        assert got == want, (what, s.name, i, s.labels[i], got, want)
        if redone is not None:
            assert sm["redone"][i] == redone, (what, s.name, i)
        g, e = a.graph(i), s.graph(i)
        for f in dbg_sets.FIELDS:
            same(g[f], e[f], f"{what}{s.name}/{i} {s.labels[i]}: {f}")
    a.close()
    return sm


def results(regions, reads, params=dbg.DEFAULTS, keep=True):
    """(summary without the redone flag, [graph bytes]) of one call"""
    a = dbg.assemble(regions, reads, params, keep=keep)
    sm = a.summary()
    graphs = [[a.graph(i)[f].tobytes() for f in dbg_sets.FIELDS] for i in range(len(regions))] if keep else None
    a.close()
    return sm, graphs


def table_slots(s):
    """The header's sizing rule over a stored set: the smallest power of two, at least 16, that is at least twice a
    region's walk positions at k0 plus its texts plus one, of the region where that is largest."""
    R, P, k0 = s.regions, s.reads, s.params[0]
    most = 0
    for i in range(len(s)):
        own = range(int(R.read_first[i]), int(R.read_last[i]))
        lens = [int(R.ref_off[i + 1] - R.ref_off[i])] + [int(P.read_off[j + 1] - P.read_off[j]) for j in own
                                                        if not P.flag[j] & 512]
        most = max(most, sum(max(0, n - k0 - 1) for n in lens) + 1 + len(own) + 1)
    cap = 16
    while cap < 2 * most:
        cap *= 2
    return cap


def same_summaries(a, b, what):
    for f in SUMMARY_FIELDS:
        same(a[f], b[f], f"{what}: {f}")


# ---------------------------------------------------------------------------------------------------------- CPU

def test_fixture_has_every_label(fx):
    assert [str(n) for n in fx["z"]["label_names"]] == list(dbg_sets.LABELS)
    seen = {x for s in fx["sets"] for x in s.labels}
    assert seen == set(dbg_sets.LABELS), set(dbg_sets.LABELS) ^ seen
    assert os.path.getsize(NPZ) <= 400 * 1024


def test_fixture_cases_are_what_their_labels_say(fx):
    m = fx["by_name"]["main"]
    at = {x: i for i, x in enumerate(m.labels)}
    tried = {x: m.tried_of(i) for x, i in at.items()}
    assert tried["repeat_cyclic_at_15_resolved_at_20"] == [(15, 1), (20, 0)]
    assert sorted({len(t) for t in tried.values()}) == [1, 2, 4, 9]
    assert tried["repeat_resolved_only_at_55"] == [(k, int(k < 55)) for k in range(15, 60, 5)]
    assert tried["tandem_repeat_cyclic_at_55"] == [(k, 1) for k in range(15, 60, 5)]
    assert tried["cycle_through_read_edge_39"] == [(15, 0)] and tried["cycle_through_read_edge_40"][0] == (15, 1)
    assert len(m.graph(at["reference_shorter_than_k_plus_2"])["src"]) == 0
    assert m.regions.read_first[at["empty_read_range"]] == m.regions.read_last[at["empty_read_range"]]
    g = m.graph(at["read_only_branch"])
    assert ((g["colours"] == 2) & (g["position"] == -1)).sum() == 15 and (g["colours"] == 3).sum() > 0
    g = m.graph(at["read_of_k_plus_1"])
    assert (g["colours"] == 1).all()
    g = m.graph(at["read_of_k_plus_2"])
    assert (g["colours"] == 3).sum() == 2 and (g["colours"] == 2).sum() == 2
    g = m.graph(at["window_min_qual_20"])
    assert (g["colours"] == 3).sum() == 25 and (g["edge_weight"] == 1 + 20).sum() == 16
    assert (m.graph(at["window_min_qual_19"])["colours"] == 3).sum() == 3 + 7  # 16 of the 24 windows hold the base
    assert (m.graph(at["lower_case_reference"])["colours"] == 2).sum() == 35
    g = m.graph(at["realistic_region"])
    assert len(g["src"]) > 4096 and m.regions.read_last[at["realistic_region"]] - m.regions.read_first[at["realistic_region"]] >= 50


def test_restatement_equals_every_stored_value(fx):
    for s in fx["sets"]:
        for i in range(len(s)):
            tried, nodes = dbg_ref.assemble(*s.texts(i), s.params)
            assert tried == s.tried_of(i), (s.name, i)
            g, e = dbg_ref.arrays(nodes), s.graph(i)
            for f in dbg_sets.FIELDS:
                same(g[f], e[f], f"{s.name}/{i}: {f}")


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_equals_fixture(fx, host, threads):
    host.setenv("GB_DBG_THREADS", threads)
    for s in fx["sets"]:
        check_set(s, "host ")
    t = dbg.timing()
    assert t["build"] == 0 and t["positions"] > t["valid_positions"] > 0
    assert dbg.plan() == {"max_table_slots": 0, "workspace_bytes": 0, "chunks": 0, "rounds": 0}


def test_five_successors_analytically(host):
    """k = 3 over AAAC.AAAG.AAAT.AAAN.AAAa.AAAC..: AAA is visited 11 times, keeps its first four successors and
    drops the edge to AAa, whose node exists all the same."""
    a = dbg.assemble([(dbg_sets.FIVE, 100, 0, 0)], [], (3, 5, 2, 20, 40), keep=True)
    g = a.graph(0)
    text = dbg_sets.FIVE
    kmer = [text[o:o + 3] for o in g["off"]]
    assert len(kmer) == 17 and (g["src"] == -1).all() and (g["position"] == 100 + g["off"]).all()
    aaa = kmer.index(b"AAA")
    assert g["weight"][aaa] == 11 and g["n_edges"][aaa] == 4
    assert [kmer[t] for t in g["edge_to"][aaa]] == [b"AAC", b"AAG", b"AAT", b"AAN"]
    assert g["edge_weight"][aaa].tolist() == [2, 1, 1, 1]
    assert b"AAa" in kmer and not (g["edge_to"] == kmer.index(b"AAa")).any()
    sm = a.summary()[0]
    assert (sm["k"], sm["n_graphs"], sm["cyclic"], sm["n_nodes"], sm["n_edges"]) == (3, 1, 1, 17, 20)


def _raw(change):
    L = dbg._decl()
    ref = np.frombuffer(change.get("ref", b"ACGTACGTACGTACGTACGTACGTA"), np.uint8).copy()
    seq = np.frombuffer(change.get("seq", b"ACGTACGTACGTACGTACGTTTTT"), np.uint8).copy()
    qual = np.full(len(seq), 30, np.uint8)
    ref_off = np.array(change.get("ref_off", [0, 10, len(ref)]), np.int64)
    read_off = np.array(change.get("read_off", [0, 4, len(seq)]), np.int64)
    first = np.array(change.get("first", [0, 1]), np.int64)
    last = np.array(change.get("last", [1, 2]), np.int64)
    start, flag = np.zeros(2, np.int32), np.zeros(2, np.uint32)
    params = (ctypes.c_int32 * 5)(*change.get("params", dbg.DEFAULTS))
    out = ctypes.c_void_p(0xDEAD)
    st = L.gb_dbg_assemble(ref.ctypes.data, len(ref), ref_off.ctypes.data, start.ctypes.data, first.ctypes.data,
                           last.ctypes.data, 2, seq.ctypes.data, qual.ctypes.data, len(seq), read_off.ctypes.data,
                           flag.ctypes.data, 2, params, change.get("keep", 0), ctypes.byref(out))
    return st, out.value, lib().gb_last_error().decode()


REFUSALS = [
    ("nul_in_reference", dict(ref=b"ACGTACGTACGTACGT\0CGTACGTA"), ["region 1", "NUL", "position 6"]),
    ("nul_in_read", dict(seq=b"ACGTACGTAC\0TACGTACGTTTTT"), ["read 1", "NUL", "position 6"]),
    ("ref_offsets_decrease", dict(ref_off=[0, 12, 10]), ["region 1", "12..10"]),
    ("ref_offsets_leave", dict(ref_off=[0, 10, 26]), ["region 1", "10..26", "25 bytes"]),
    ("read_offsets_decrease", dict(read_off=[0, 9, 4]), ["read 1", "9..4"]),
    ("read_offsets_leave", dict(read_off=[0, 4, 25]), ["read 1", "4..25", "24 bytes"]),
    ("range_outside_pool", dict(last=[1, 3]), ["region 1", "1..3", "pool of 2"]),
    ("range_reversed", dict(first=[1, 1], last=[0, 2]), ["region 0", "1..0"]),
    ("k0_0", dict(params=(0, 5, 50, 20, 40)), ["k0 = 0"]),
    ("k_step_0", dict(params=(15, 0, 50, 20, 40)), ["k_step = 0"]),
    ("largest_k", dict(params=(15, 5, 60, 20, 40)), ["k = 65", "GB_DBG_MAX_K"]),
    ("k0_above_max_k", dict(params=(65, 5, 50, 20, 40)), ["k = 65", "GB_DBG_MAX_K"]),
    ("keep_2", dict(keep=2), ["keep = 2"]),
    ("budget", dict(env={"GB_DBG_WS": "100"}, device=True), ["region 0", "bytes", "budget of 100"]),
    ("budget_text", dict(env={"GB_DBG_WS": "lots"}, device=True), ["GB_DBG_WS", "lots"]),
    ("fp_bits", dict(env={"GB_DBG_FP_BITS": "65"}, device=True), ["GB_DBG_FP_BITS", "65"]),
]


@pytest.mark.parametrize("name,change,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_first_and_leave_the_outputs(monkeypatch, name, change, words):
    """GB_ERR_ARG before any device work (the environment cases run without GB_DBG_HOST: they are checked before a
    device is looked for), *out untouched, the item named."""
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    if not change.get("device"):
        monkeypatch.setenv("GB_DBG_HOST", "1")
    for key, v in change.get("env", {}).items():
        monkeypatch.setenv(key, v)
    st, out, msg = _raw(change)
    assert st == -1 and out == 0xDEAD, (st, out, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_largest_k_of_64_is_taken(host):
    a = dbg.assemble([(b"ACGT" * 30, 0, 0, 0)], [], (14, 10, 60, 20, 40))
    sm = a.summary()[0]
    assert (sm["k"], sm["n_graphs"], sm["cyclic"]) == (64, 6, 1)


def test_a_region_whose_visits_pass_32_bits_is_refused(host):
    """The refusal comes from the offsets alone, before any byte is read: the array is zero pages never touched."""
    n = dbg.MAX_EDGES + 20
    L = dbg._decl()
    ref = np.zeros(n, np.uint8)
    ref_off, z64, z32 = np.array([0, n], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int32)
    out = ctypes.c_void_p(0xDEAD)
    st = L.gb_dbg_assemble(ref.ctypes.data, n, ref_off.ctypes.data, z32.ctypes.data, z64.ctypes.data, z64.ctypes.data,
                           1, None, None, 0, z64.ctypes.data, None, 0, None, 0, ctypes.byref(out))
    msg = lib().gb_last_error().decode()
    assert st == -1 and out.value == 0xDEAD and "cannot be indexed in 32 bits" in msg and "region 0" in msg, msg


def test_export_refusals(host):
    a = dbg.assemble([(REF40, 0, 0, 0)], [], keep=True)
    L = dbg._decl()
    n, src = ctypes.c_int64(-1), np.full(4, 77, np.int32)
    st = L.gb_dbg_export(a._h, 0, 4, src.ctypes.data, *([None] * 7), ctypes.addressof(n))
    assert st == -1 and n.value == a.summary()["n_nodes"][0] > 4 and (src == 77).all()
    assert L.gb_dbg_export(a._h, 1, 4, *([None] * 8), ctypes.addressof(n)) == -1
    b = dbg.assemble([(REF40, 0, 0, 0)], [], keep=False)
    st = L.gb_dbg_export(b._h, 0, 100, src.ctypes.data, *([None] * 7), ctypes.addressof(n))
    assert st == -1 and "keep = 0" in lib().gb_last_error().decode() and (src == 77).all()
    assert L.gb_dbg_summary(a._h, None, 0) == -1


def _without_a_pool():
    """One region through the C call with no read pool at all: every read array null."""
    L = dbg._decl()
    ref = np.frombuffer(REF40, np.uint8).copy()
    ref_off, z64 = np.array([0, len(ref)], np.int64), np.zeros(1, np.int64)
    start = np.array([2147483640], np.int32)
    h = ctypes.c_void_p(None)
    st = L.gb_dbg_assemble(ref.ctypes.data, len(ref), ref_off.ctypes.data, start.ctypes.data, z64.ctypes.data,
                           z64.ctypes.data, 1, None, None, 0, None, None, 0, None, 1, ctypes.byref(h))
    assert st == 0, lib().gb_last_error().decode()
    sm, n = np.zeros(1, dbg.SUMMARY), ctypes.c_int64(-1)
    pos = np.zeros(25, np.int32)
    assert L.gb_dbg_summary(h, sm.ctypes.data, 1) == 0
    assert L.gb_dbg_export(h, 0, 25, None, None, None, pos.ctypes.data, *([None] * 4), ctypes.addressof(n)) == 0
    L.gb_dbg_free(h)
    assert (sm["k"][0], sm["n_nodes"][0], sm["n_edges"][0], sm["cyclic"][0], n.value) == (15, 25, 24, 0, 25)
    # positions are ref_start + offset in 64 bits, then cut to int32, on either path
    assert pos.tolist() == [int(np.int64(2147483640 + i).astype(np.int32)) for i in range(25)]


def test_host_without_a_read_pool(host):
    _without_a_pool()


@pytest.mark.gpu
def test_device_without_a_read_pool(device):
    _without_a_pool()


def test_empty_inputs_touch_no_device(monkeypatch):
    """No region: an empty summary, without GB_DBG_HOST and without a device."""
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    a = dbg.assemble(dbg.Regions(np.zeros(0, np.uint8), [0], [], [], []), dbg.Reads([], [], [0], []), keep=True)
    assert len(a.summary()) == 0
    a = dbg.assemble([], [(b"ACGT", [30] * 4, 0)])
    assert len(a.summary()) == 0


def test_exports_appear_in_libgb():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "genomicsbench_palisade_amd", "lib", "libgb.so")],
                         capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "gb_fmi_dbg.h")).read()
    names = ("gb_dbg_assemble", "gb_dbg_free", "gb_dbg_summary", "gb_dbg_export", "gb_dbg_timing", "gb_dbg_plan")
    assert set(re.findall(r"\b(gb_dbg_\w+)\(", header)) == set(names)
    for f in names:
        assert f" T {f}\n" in out, f


def test_windows_equal_the_reference(fx):
    z = fx["z"]
    pos, end, longest, spans = dbg_sets.window_reads()
    for n, (beg, stop, region) in enumerate(spans):
        got = dbg.windows(pos, end, longest, beg, stop, region)
        want = z["win_expect"][z["win_off"][n]:z["win_off"][n + 1]]
        assert len(got) == len(want) > 0
        shift = max(100, min(1000, region // 2))
        for i, (a0, r0, r1, first, last) in enumerate(got):
            assert a0 == beg + i * shift and r0 == max(0, a0 - region) and r1 == min(a0 + region, stop) + region
            assert (first, last) == tuple(want[i]), (n, i)
    # reads that end at or before the window start are passed over, and a window past the last read is empty
    got = dbg.windows(pos, end, longest, *spans[0])
    assert any(f > np.searchsorted(pos, max(1, a0 - longest)) for a0, _, _, f, _ in got)
    assert got[-1][3] == got[-1][4] == len(pos)
    assert [tuple(x) for x in z["win_empty"]] == [w[3:] for w in dbg.windows([], [], 0, 0, 3000)] == [(0, 0)] * 4
    # the reference exits when the first read that reaches the window lies past the window's end
    with pytest.raises(ValueError, match="read start pointer"):
        dbg.windows([10, 20, 5000], [5, 6, 50], 100, 100, 1600)


def test_generator_is_seeded():
    a, b = gen.dbg_regions(3, 4, n_reads=40), gen.dbg_regions(3, 4, n_reads=40)
    assert len(a[0]) == len(b[0]) == 4 and len(a[1]) == len(b[1]) > 100
    assert all((x[0] == y[0]).all() and x[1:] == y[1:] for x, y in zip(a[0], b[0]))
    assert all((x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2] == y[2] for x, y in zip(a[1], b[1]))
    for ref, start, first, last in a[0]:
        assert len(ref) == 4500 and 20 <= last - first <= 65
    assert a[0][1][2] < a[0][0][3], "neighbouring regions share reads"
    assert any(r[2] & 512 for r in gen.dbg_regions(3, 8)[1])


# ------------------------------------------------------------------------------------------------------- device

@pytest.fixture(scope="module")
def second_set():
    """About 40 regions of 1 500 reference bases and 50 reads, with the host path's results."""
    regions, reads = dbg.pack(*gen.dbg_regions(23, 40, region=500, n_reads=50, read_len=100, repeat_every=13))
    saved = {e: os.environ.pop(e, None) for e in ENV}  # the caller's settings shape no expected value
    os.environ["GB_DBG_HOST"] = "1"
    try:
        sm, graphs = results(regions, reads)
    finally:
        del os.environ["GB_DBG_HOST"]
        os.environ.update({e: v for e, v in saved.items() if v is not None})
    return {"regions": regions, "reads": reads, "summary": sm, "graphs": graphs}


@pytest.mark.gpu
def test_device_equals_fixture(fx, device):
    for s in fx["sets"]:
        check_set(s, "device ")
    t, p = dbg.timing(), dbg.plan()
    assert all(t[x] > 0 for x in ("pack", "build", "rank", "edges", "cycle")) and t["redo"] == 0, t
    main = fx["by_name"]["main"]
    assert p["chunks"] == 1 and p["rounds"] == 9 and p["max_table_slots"] == table_slots(main) == 32768 and p["workspace_bytes"] > 0, p
    assert t["positions"] > t["valid_positions"] > 0 and len(main) == 20


@pytest.mark.gpu
def test_device_equals_host_on_a_second_set(second_set, device):
    s = second_set
    assert len(s["regions"]) == 40 and s["summary"]["n_graphs"].max() >= 3 and s["summary"]["n_graphs"].min() == 1
    sm, graphs = results(s["regions"], s["reads"])
    same_summaries(sm, s["summary"], "second set")
    assert not sm["redone"].any() and graphs == s["graphs"]


@pytest.mark.gpu
def test_device_under_another_region_order(second_set, device):
    s = second_set
    order = np.random.default_rng(7).permutation(len(s["regions"]))
    sm, graphs = results(s["regions"].take(order), s["reads"])
    same_summaries(sm, s["summary"][order], "permuted")
    assert graphs == [s["graphs"][i] for i in order]


@pytest.mark.gpu
def test_device_in_chunks(second_set, device):
    s = second_set
    results(s["regions"], s["reads"], keep=False)
    whole = dbg.plan()
    assert whole["chunks"] == 1
    device.setenv("GB_DBG_WS", str(whole["workspace_bytes"] // 3))
    sm, graphs = results(s["regions"], s["reads"])
    assert dbg.plan()["chunks"] >= 3
    same_summaries(sm, s["summary"], "chunks")
    assert graphs == s["graphs"]


@pytest.mark.gpu
def test_device_with_weakened_fingerprints(fx, device):
    """8 bits of fingerprint: colliding regions are marked and built again on the host, and nothing changes. With
    the full fingerprint no fixture region is marked, and on the host restatement no two of the fixture's k-mers
    share one."""
    for s in fx["sets"]:
        assert not check_set(s, "full ", redone=0)["redone"].any()
    device.setenv("GB_DBG_FP_BITS", "8")
    redone = np.concatenate([check_set(s, "8 bits ", redone=None)["redone"] for s in fx["sets"]])
    assert redone.sum() >= 1 and dbg.timing()["redo"] > 0


def test_no_fixture_kmers_collide_under_the_full_fingerprint(fx):
    """The polynomial and the finalizer of csrc/fmi_dbg_internal.h, restated: over every k a fixture region is built
    at, distinct k-mers of a region have distinct fingerprints."""
    m64 = (1 << 64) - 1

    def mix(x):
        x ^= x >> 33
        x = x * 0xFF51AFD7ED558CCD & m64
        x ^= x >> 33
        x = x * 0xC4CEB9FE1A85EC53 & m64
        return x ^ x >> 33

    def fp(kmer):
        p = 0
        for c in kmer:
            p = (p * 0x9E3779B97F4A7C15 + c) & m64
        return mix(p) or 1

    for s in fx["sets"]:
        for i in range(len(s)):
            ref, _, reads = s.texts(i)
            for k, _ in s.tried_of(i):
                kmers = {t[o:o + k] for t in [ref] + [r[1] for r in reads] for o in range(len(t) - k + 1)}
                assert len({fp(x) for x in kmers}) == len(kmers), (s.name, i, k)


@pytest.mark.gpu
def test_device_two_runs_give_identical_bytes(fx, device):
    s = fx["by_name"]["main"]
    runs = []
    for _ in range(2):
        sm, graphs = results(s.regions, s.reads, s.params)
        runs.append((sm.tobytes(), graphs))
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_device_after_lds_poison(fx, device):
    """The scan's wave totals and the peeling's progress flag and count go through LDS: the fixture once after every
    CU's LDS has been filled with each pattern of tests/cpp/lds_poison.hip."""
    path = os.path.join(ROOT, "tests", "_build", "liblds_poison.so")
    assert os.path.exists(path), f"{path} not built (make)"
    L = ctypes.CDLL(path)
    L.lds_poison.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    for mode, value in [(0, 0), (1, 0), (2, 2), (2, 37), (2, 300), (3, 1000), (4, 0)]:
        assert L.lds_poison(0, mode, value, 1) == 0
        for s in fx["sets"]:
            check_set(s, f"pattern {(mode, value)} ")


@pytest.mark.gpu
def test_device_keep_0_equals_keep_1(second_set, device):
    s = second_set
    sm, _ = results(s["regions"], s["reads"], keep=False)
    same_summaries(sm, s["summary"], "keep = 0")
    assert not sm["redone"].any()
