"""gb_chain_extd2 (minimap2's ksw_extd2_sse for a batch of items) against tests/golden/chain_extd2_golden.npz, recorded
from the reference's CPU ksw_extd2_sse by tests/golden/make_chain_extd2_golden.py.

Without a GPU: the host path (GB_CHAIN_EXTD2_HOST=1) on the whole fixture in every byte with one thread and with
several, the numpy restatement on the fixture's small items, the refusals, the CIGAR invariants, and a live
cross-check of fresh items where the reference tree and a compiler are present. On the GPU: the whole fixture bit
for bit, shuffled, each size class alone, in many chunks under a small workspace budget, the device against the
host path on a second seeded set with wide rows and a row state too large for the LDS, and the timing and plan
calls.
"""
import collections
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import chain_extd2_ref as ref
from genomicsbench_palisade_amd import chain, gen

SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 128, 129, 257)
BANDS = (-1, 0, 1, 7, 15, 16, 17, 33, 100)
GROUPS = ("shape", "zdrop", "flags", "params", "ambi", "repeat", "longgap", "wide", "empty")
LDS_MAX = 64 * 1024


def size_class(items):
    """The kernel's size class of EXTD2_ITEM_DTYPE records: 0, 1, 2 by the blocks of a row of backtrack codes
    (n_col_ <= 16, <= 64, above), 3 when the row state passes the LDS."""
    q, t, w = (items[f].astype(np.int64) for f in ("qlen", "tlen", "w"))
    w = np.where(w < 0, np.maximum(q, t), w)
    ncol = (np.minimum(np.minimum(q, t), w + 1) + 15) // 16 + 1
    t16, q16 = (t + 15) // 16 * 16, (q + 15) // 16 * 16
    return np.where(12 * t16 + q16 + 16 > LDS_MAX, 3, np.where(ncol <= 16, 0, np.where(ncol <= 64, 1, 2)))


def code_bytes(items):
    q, t, w = (items[f].astype(np.int64) for f in ("qlen", "tlen", "w"))
    w = np.where(w < 0, np.maximum(q, t), w)
    return (q + t - 1) * ((np.minimum(np.minimum(q, t), w + 1) + 15) // 16 + 1) * 16


class Fixture:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "chain_extd2_golden.npz"))
        self.z = z
        self.group = np.array([str(g) for g in z["group"]])
        self.res = z["res"].astype(np.int32)
        self.cigar = z["cigar"]
        self.off = np.concatenate([[0], np.cumsum(z["cigar_len"], dtype=np.int64)])
        self.n = len(z["items"])
        self.sets = []  # (item indices, Extd2Items) per parameter set
        for pid in range(len(z["params"])):
            idx = np.flatnonzero(z["param_id"] == pid)
            self.sets.append((idx, gen.Extd2Items(z["params"][pid:pid + 1], z["seqs"], z["items"][idx])))

    def words(self, i):
        return self.cigar[self.off[i]:self.off[i + 1]]

    def check(self, run, select=None):
        """run(Extd2Items) -> (res, cigar, cigar_off), compared in every byte; select(Extd2Items) -> indices to run
        (all)."""
        for idx, x in self.sets:
            sel = np.arange(x.n) if select is None else np.asarray(select(x), np.int64)
            if not len(sel):
                continue
            res, cig, off = run(x.subset(sel))
            want = [self.words(idx[s]) for s in sel]
            assert (np.diff(off) == [len(w) for w in want]).all() and off[0] == 0 and off[-1] == len(cig)
            got = res.view(np.int32).reshape(-1, 12)
            bad = np.flatnonzero((got != self.res[idx[sel]]).any(1))
            assert not len(bad), (len(bad), x.items[sel[bad[0]]], got[bad[0]], self.res[idx[sel[bad[0]]]])
            bad = np.flatnonzero(cig != np.concatenate(want))
            assert not len(bad), (len(bad), x.items[sel[np.searchsorted(off, bad[0], "right") - 1]])


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_CHAIN_EXTD2_HOST", "1")
    monkeypatch.delenv("GB_CHAIN_THREADS", raising=False)
    monkeypatch.delenv("GB_CHAIN_EXTD2_WS", raising=False)
    return monkeypatch


def test_fixture_covers_its_labels_groups_and_shapes(fx):
    z = fx.z
    counts = dict(zip([str(x) for x in z["label_names"]], z["label_counts"]))
    minima = dict(zip([str(x) for x in z["label_names"]], z["label_minima"]))
    assert set(counts) == set(ref.LABELS) == set(ref.MINIMA)
    for k, v in ref.MINIMA.items():
        assert v >= 1 and minima[k] == v and counts[k] >= v, (k, counts[k], v)
    for g in GROUPS:
        assert (fx.group == g).any(), g
    it = z["items"]
    grid = it[fx.group == "shape"]
    assert {(n, n, w, f) for n in SIZES for w in BANDS for f in gen.EXTD2_USES} <= {
        tuple(int(v) for v in r) for r in zip(grid["qlen"], grid["tlen"], grid["w"], grid["flag"])}
    assert (grid["qlen"] < grid["tlen"]).any() and (grid["qlen"] > grid["tlen"]).any()
    zd = it[fx.group == "zdrop"]
    assert set(zd["zdrop"].tolist()) == {-1, 8, 30, 400} and set(zd["end_bonus"].tolist()) == {-1, 10}
    assert {0x18, 0x02, 0x80} <= set(it["flag"][fx.group == "flags"].tolist()) and not (it["flag"] & ~chain.EXTD2_FLAGS).any()
    assert [str(s) for s in z["param_names"]] == ["map-ont", "asm5", "asm20", "sr", "swapped", "early", "ambi0"]
    assert all((z["param_id"] == p).any() for p in range(7))
    cls = size_class(it[(it["qlen"] > 0) & (it["tlen"] > 0)])
    assert (cls == 0).sum() > 500 and (cls == 1).sum() >= 3 and (cls == 2).sum() >= 1  # class 3: see the second set
    wide = it[fx.group == "wide"]
    assert ((wide["w"] == 751) & (wide["qlen"] >= 1000)).sum() >= 3 and ((wide["w"] < 0) & (wide["qlen"] >= 2000)).any()
    assert (wide["tlen"] - wide["qlen"] > wide["w"])[wide["w"] >= 0].any()
    assert ((it["qlen"] == 0) & (it["tlen"] > 0)).any() and ((it["tlen"] == 0) & (it["qlen"] > 0)).any()
    assert (z["seqs"] == 4).any() and z["seqs"].max() == 4
    assert os.path.getsize(os.path.join(GOLDEN, "chain_extd2_golden.npz")) <= 400 * 1024


@pytest.mark.parametrize("threads", [1, 5])
def test_host_path_equals_fixture(fx, host, threads):
    host.setenv("GB_CHAIN_THREADS", str(threads))
    fx.check(chain.extd2)


def test_restatement_equals_fixture_on_small_items(fx):
    """The numpy restatement is checked against the live reference on every item by the recorder; here on every
    seventh item of at most 70 rows."""
    n = 0
    for idx, x in fx.sets:
        small = np.flatnonzero(x.items["qlen"] + x.items["tlen"] <= 70)
        for i in small[::7]:
            rec, cig = ref.align_item(x, int(i))
            assert list(rec) == fx.res[idx[i]].tolist() and cig.tolist() == fx.words(idx[i]).tolist(), x.items[i]
            n += 1
    assert n >= 60


def _spans(words):
    op, ln = words & 15, (words >> 4).astype(np.int64)
    return int(ln[op != 2].sum()), int(ln[op != 1].sum())  # query bases, target bases


def test_cigar_invariants(fx, host):
    """A CIGAR spans the matrix from its first cell to the cell the walk starts from: in the fixture and out of the
    host path, whose cigar_off is monotone."""
    walked = 0
    for idx, x in fx.sets:
        res, cig, off = chain.extd2(x)
        early = ref.Par(x.params).early  # the `-min_sc > 2 * (q + e)` return: reset records, no walk
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(cig) <= chain.extd2_need(x.items)
        for j, i in enumerate(idx):
            it, w = x.items[j], fx.words(i)
            end = ref.walk_end(fx.res[i], int(it["qlen"]), int(it["tlen"]), int(it["flag"]))
            assert fx.res[i][10] == len(w) == off[j + 1] - off[j] and fx.res[i][11] == 0
            if not it["qlen"] or not it["tlen"] or end is None or early:
                assert not len(w)
                continue
            assert len(w) and ((w & 15) <= 2).all() and (w >> 4 >= 1).all() and ((w[1:] & 15) != (w[:-1] & 15)).all()
            assert _spans(w) == (end[1] + 1, end[0] + 1), it
            walked += 1
    assert walked > 1300


def _small(seed=3):
    return gen.extd2_items(np.random.default_rng(seed), [(20, 24)] * 4, w=10, flag=0)


REFUSALS = ["flag_score_only", "flag_generic_sc", "flag_splice", "flag_high", "qlen_negative", "tlen_negative", "qlen_over",
            "tlen_over", "q_off_negative", "q_off_outside", "t_off_outside", "query_code_5", "target_code_255", "budget",
            "budget_text"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_come_before_any_device_work_and_leave_the_outputs_untouched(case, monkeypatch):
    """No GB_CHAIN_EXTD2_HOST here: every refusal comes before the device is touched, so none is needed."""
    from genomicsbench_palisade_amd import lib
    monkeypatch.delenv("GB_CHAIN_EXTD2_HOST", raising=False)
    monkeypatch.delenv("GB_CHAIN_EXTD2_WS", raising=False)
    x = _small()
    seqs, items = x.seqs.copy(), x.items.copy()
    named = "item 3"
    if case == "flag_score_only":
        items["flag"][3] = 0x01
    elif case == "flag_generic_sc":
        items["flag"][3] = 0x40 | 0x04
    elif case == "flag_splice":
        items["flag"][3] = 0x100
    elif case == "flag_high":
        items["flag"][3] = -2147483648
    elif case == "qlen_negative":
        items["qlen"][3] = -1
    elif case == "tlen_negative":
        items["tlen"][3] = -5
    elif case == "qlen_over":
        items["qlen"][3] = chain.EXTD2_MAX_LEN + 1
    elif case == "tlen_over":
        items["tlen"][3] = chain.EXTD2_MAX_LEN + 1
    elif case == "q_off_negative":
        items["q_off"][3] = -1
    elif case == "q_off_outside":
        items["q_off"][3] = len(seqs) - items["qlen"][3] + 1
    elif case == "t_off_outside":
        items["t_off"][3] = len(seqs)
    elif case == "query_code_5":
        seqs[items["q_off"][3] + 7] = 5
    elif case == "target_code_255":
        seqs[items["t_off"][3] + 23] = 255
    elif case == "budget":  # 43 rows of 2 blocks of codes, and twice 44 words
        monkeypatch.setenv("GB_CHAIN_EXTD2_WS", str(43 * 2 * 16 + 2 * 44 * 4 - 1))
        named = "item 0"
    elif case == "budget_text":
        monkeypatch.setenv("GB_CHAIN_EXTD2_WS", "1g")
        named = "GB_CHAIN_EXTD2_WS"
    cap = chain.extd2_need(x.items)
    res = np.full(12 * x.n, -7, np.int32).view(chain.EXTD2_RESULT_DTYPE)
    cigar = np.full(cap, 777, np.uint32)
    off = np.full(x.n + 1, -5, np.int64)
    st, r, c, o, used = chain.extd2_raw(x.params, seqs, items, cap, res, cigar, off)
    assert st == -1 and r is res and c is cigar and o is off and used == -1
    assert (res.view(np.int32) == -7).all() and (cigar == 777).all() and (off == -5).all()
    assert named in lib().gb_last_error().decode()


def test_cigar_cap_one_short_is_refused_with_the_need(host):
    from genomicsbench_palisade_amd import lib
    x = _small()
    need = chain.extd2_need(x.items)
    assert need == 4 * 44
    res = np.full(12 * x.n, -7, np.int32).view(chain.EXTD2_RESULT_DTYPE)
    cigar = np.full(need, 777, np.uint32)
    off = np.full(x.n + 1, -5, np.int64)
    st, _, _, _, used = chain.extd2_raw(x.params, x.seqs, x.items, need - 1, res, cigar, off)
    assert st == -1 and used == need and (res.view(np.int32) == -7).all() and (cigar == 777).all() and (off == -5).all()
    assert str(need) in lib().gb_last_error().decode()
    st, res, _, off, used = chain.extd2_raw(x.params, x.seqs, x.items, need)
    assert st == 0 and off[0] == 0 and off[-1] == used <= need and (res["n_cigar"] == np.diff(off)).all()


def test_no_items_and_only_early_items_succeed_without_a_device(monkeypatch):
    monkeypatch.delenv("GB_CHAIN_EXTD2_HOST", raising=False)
    x = _small()
    st, res, cig, off, used = chain.extd2_raw(x.params, x.seqs, x.items[:0])
    assert st == 0 and len(res) == 0 and (off == [0]).all() and used == 0
    # the `-min_sc > 2 * (q + e)` return and the empty sides leave the reset record
    reset = [0, 0, -1, -1, chain.EXTD2_NEG_INF, -1, chain.EXTD2_NEG_INF, -1, chain.EXTD2_NEG_INF, 0, 0, 0]
    st, res, cig, off, used = chain.extd2_raw(gen.extd2_params(1, 19, 1, 4, 2, 24, 1), x.seqs, x.items)
    assert st == 0 and used == 0 and (off == 0).all() and (res.view(np.int32).reshape(-1, 12) == reset).all()
    items = x.items.copy()
    items["qlen"][::2], items["tlen"][1::2] = 0, 0
    st, res, cig, off, used = chain.extd2_raw(x.params, x.seqs, items)
    assert st == 0 and used == 0 and (off == 0).all() and (res.view(np.int32).reshape(-1, 12) == reset).all()


def test_the_length_limit_itself_is_accepted(host):
    """32 768 bases against 40 in a band of 4: the band leaves the matrix after a few dozen rows."""
    rng = np.random.default_rng(8)
    x = gen.extd2_items(rng, [(40, chain.EXTD2_MAX_LEN), (chain.EXTD2_MAX_LEN, 40)], w=4, zdrop=400, flag=0x40)
    res, cig, off = chain.extd2(x)
    for i in range(2):
        rec, words = ref.align_item(x, i)
        assert res[i].tolist() == tuple(rec) and cig[off[i]:off[i + 1]].tolist() == words.tolist() and rec[1] == 1


def _second_set(seed, n_items, wide=True):
    """Items over all size classes: most are gap fills and extensions of up to 300 bases; with `wide`, rows of
    w = 751, one item without a band (more than 64 blocks per row) and one whose row state passes the LDS."""
    rng = np.random.default_rng(seed)
    shapes = [(int(q), int(np.clip(q + rng.integers(-30, 31), 1, None))) for q in rng.integers(1, 300, n_items)]
    parts = [gen.extd2_items(rng, shapes, sub=0.08, indel=0.05, long_indel=0.004, n_rate=0.004)]
    if wide:
        parts.append(gen.extd2_items(rng, [(900, 1000), (1500, 1400), (2500, 2450)], w=751, zdrop=400, long_indel=0.003))
        parts.append(gen.extd2_items(rng, [(1300, 1250)], w=-1, flag=(0, 0x02)))
        parts.append(gen.extd2_items(rng, [(5600, 5500)], w=100, zdrop=400, flag=0x40, sub=0.03, indel=0.01))
    return gen.Extd2Items.concat(parts)


def test_host_path_equals_the_live_reference_on_fresh_items(host):
    sys.path.insert(0, GOLDEN)
    import make_chain_extd2_golden as mk
    if not os.path.exists(os.path.join(mk.REF_TREE, "tools", "minimap2", "ksw2_extd2_sse.c")) or not shutil.which("gcc"):
        pytest.skip("no reference tree or no compiler here")
    live = mk.LiveExtd2(mk.REF_TREE)
    try:
        x = _second_set(99, 300)
        res, cig, off = chain.extd2(x)
        for i in range(x.n):
            assert mk.equal((res[i].tolist(), cig[off[i]:off[i + 1]]), live.align_item(x, i)), x.items[i]
    finally:
        live.close()


# ---- on the device ----


@pytest.fixture
def device(monkeypatch):
    monkeypatch.delenv("GB_CHAIN_EXTD2_HOST", raising=False)
    monkeypatch.delenv("GB_CHAIN_EXTD2_WS", raising=False)
    return monkeypatch


@pytest.mark.gpu
def test_device_equals_fixture_bit_for_bit(fx, device):
    fx.check(chain.extd2)


@pytest.mark.gpu
def test_device_equals_fixture_with_its_items_shuffled(fx, device):
    rng = np.random.default_rng(12)
    fx.check(chain.extd2, select=lambda x: rng.permutation(x.n))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", range(4))
def test_device_equals_fixture_on_each_size_class_alone(fx, device, cls):
    if cls == 3:  # no fixture item's state passes the LDS: one that does, against the host path
        x = gen.extd2_items(np.random.default_rng(31), [(5400, 5600), (300, 6000)], w=(60, 100), zdrop=400, flag=(0, 0x40))
        assert (size_class(x.items) == 3).all()
        d = chain.extd2(x)
        device.setenv("GB_CHAIN_EXTD2_HOST", "1")
        h = chain.extd2(x)
        assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(d, h)) and (h[0]["n_cigar"] > 20).all()
        return
    ran = []
    live = lambda x: (x.items["qlen"] > 0) & (x.items["tlen"] > 0)  # noqa: E731
    fx.check(lambda x: (ran.append(x.n), chain.extd2(x))[1], select=lambda x: np.flatnonzero(live(x) & (size_class(x.items) == cls)))
    assert sum(ran) >= (500, 3, 1)[cls]
    if cls == 0:  # a launch of 1, 2, 3 and 5 workgroups
        for n in (1, 2, 3, 5):
            fx.check(chain.extd2, select=lambda x: np.arange(min(n, x.n)))


@pytest.mark.gpu
def test_device_equals_fixture_in_many_chunks(fx, device):
    """A workspace budget just above the largest item's need: the fixture runs in many chunks, to the same bytes."""
    idx, x = fx.sets[0]
    big = int(np.argmax(code_bytes(x.items)))
    assert (x.items["qlen"][big], x.items["tlen"][big], x.items["w"][big]) == (2000, 2040, -1)
    chain.extd2(x.subset([big]))
    chunks, need = chain.extd2_plan()
    assert chunks == 1 and need == 4039 * 126 * 16 + 2 * 4040 * 4
    device.setenv("GB_CHAIN_EXTD2_WS", str(need))
    seen = []
    fx.check(lambda x: (chain.extd2(x), seen.append(chain.extd2_plan()))[0])
    assert seen[0][0] >= 3 and all(b <= need for _, b in seen)
    device.setenv("GB_CHAIN_EXTD2_WS", str(need - 1))
    st = chain.extd2_raw(x.params, x.seqs, x.items)[0]
    assert st == -1


@pytest.mark.gpu
def test_device_equals_host_path_on_a_second_set(device):
    x = _second_set(4242, 1500)
    cls = size_class(x.items)
    assert x.n == 1505 and all((cls == c).any() for c in range(4))
    d = chain.extd2(x)
    fill, walk, cells = chain.extd2_timing()
    assert fill > 0 and walk > 0 and cells > 0 and chain.extd2_plan()[0] == 1
    device.setenv("GB_CHAIN_EXTD2_HOST", "1")
    h = chain.extd2(x)
    assert (d[2] == h[2]).all() and len(h[1]) > 5000
    bad = np.flatnonzero((d[0].view(np.int32).reshape(-1, 12) != h[0].view(np.int32).reshape(-1, 12)).any(1))
    assert not len(bad), (len(bad), x.items[bad[0]], d[0][bad[0]], h[0][bad[0]])
    assert (d[1] == h[1]).all()


@pytest.mark.gpu
def test_timing_counts_the_cells_the_reference_sweeps(device):
    """The in-band cells of the rows reached, z-dropped and band-exited items included, against the restatement."""
    x = gen.extd2_items(np.random.default_rng(77), [(60, 64), (120, 100), (33, 200), (150, 150)] * 6, w=(5, 17, 100, -1),
                        zdrop=(8, 30, 400), sub=0.2, indel=0.08, tail=0.3)
    count = collections.defaultdict(int, cells=0)
    want = [ref.align_item(x, i, labels=count) for i in range(x.n)]
    res, cig, off = chain.extd2(x)
    for i, (rec, words) in enumerate(want):
        assert res[i].tolist() == tuple(rec) and cig[off[i]:off[i + 1]].tolist() == words.tolist()
    fill, walk, cells = chain.extd2_timing()
    assert count["zdropped_by_score"] >= 3 and count["band_exit"] >= 3 and cells == count["cells"] and fill > 0 and walk > 0
    assert chain.extd2_plan() == (1, int((code_bytes(x.items) + 8 * (x.items["qlen"] + x.items["tlen"])).sum()))
