"""gb_abea_hmm_align (Viterbi event alignment with traceback) against tests/golden/abea_viterbi_golden.npz, recorded
from f5c's CPU profile_hmm_align by tests/golden/make_abea_viterbi_golden.py.

Without a GPU: the host path (GB_ABEA_HOST=1) on the whole fixture in every field and bit with one thread and
with several, the numpy restatement on the fixture's small items, the refusals, the path invariants, the order
of a read's items, and a live cross-check of fresh items where the reference tree and a compiler are present. On
the GPU: the whole fixture bit for bit, shuffled, each size class alone, in many chunks under a small workspace
budget, the device against the host path on a second seeded set, and the timing call.
"""
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN, bits

import abea_viterbi_ref as ref
from genomicsbench_palisade_amd import abea, gen

QUANTUM = 0.125
KMERS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 256)
ROWS = (2, 3, 10, 63, 64, 65)
LONG_KMERS = (1, 17, 64, 129, 256)
LONG_ROWS = (300, 2000)
GROUPS = ("shape", "typical", "outlier", "nonacgt", "epb_one", "scaled", "grid")
CLASS_BOUNDS = ((1, 16), (17, 64), (65, 128), (129, 256))  # k-mers per size class of the kernel


def expected_records(items, path_len, kmer, state, l_fm_bits):
    """The fixture's records as abea.HMM_PATH_DTYPE: a record's row rises by one at every record but a 'K'."""
    rec = np.zeros(len(kmer), abea.HMM_PATH_DTYPE)
    rec["kmer_idx"], rec["state"], rec["l_fm"] = kmer, state.view("S1"), l_fm_bits.view(np.float32)
    off = np.concatenate([[0], np.cumsum(path_len, dtype=np.int64)])
    for i, it in enumerate(items):
        s = state[off[i]:off[i + 1]]
        row = np.cumsum(s != ord("K")) - int(s[0] != ord("K"))  # 0 at the first record
        rec["event_idx"][off[i]:off[i + 1]] = int(it["event_start"]) + (-1 if it["rc"] else 1) * row
    return rec, off


class Fixture:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "abea_viterbi_golden.npz"))
        self.z = z
        self.group = np.array([str(g) for g in z["group"]])
        self.want, self.off = expected_records(z["items"], z["path_len"], z["path_kmer"], z["path_state"], z["path_l_fm_bits"])
        models = np.stack([z["model_mean_q"].astype(np.float32) / np.float32(64),
                           z["model_stdv_q"].astype(np.float32) / np.float32(128), z["model_log_stdv"]], -1)
        events = z["events_q"].astype(np.float32) * np.float32(QUANTUM)
        self.sets = []  # (item indices, AbeaAlignItems) per model
        for mid in range(len(models)):
            idx = np.flatnonzero(z["model_id"] == mid)
            self.sets.append((idx, gen.AbeaAlignItems(models[mid], z["seqs"], events, z["reads"], z["items"][idx])))
        self.n = len(z["items"])

    def records(self, i):
        return self.want[self.off[i]:self.off[i + 1]]

    def check(self, run, select=None):
        """run(AbeaAlignItems) -> (records, path_off), compared in every byte; select(AbeaAlignItems) -> indices to
        run (all)."""
        for idx, x in self.sets:
            sel = np.arange(x.n) if select is None else np.asarray(select(x), np.int64)
            if not len(sel):
                continue
            rec, off = run(x.subset(sel))
            want = [self.records(idx[s]) for s in sel]
            assert (np.diff(off) == [len(w) for w in want]).all() and off[0] == 0 and off[-1] == len(rec)
            want = np.concatenate(want)
            bad = np.flatnonzero(rec.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))
            assert not len(bad), (len(bad), rec[bad[0] // 16], want[bad[0] // 16], np.searchsorted(off, bad[0] // 16, "right") - 1)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_ABEA_HOST", "1")
    monkeypatch.delenv("GB_ABEA_THREADS", raising=False)
    return monkeypatch


def test_fixture_covers_its_labels_groups_and_shapes(fx):
    z = fx.z
    counts = dict(zip([str(x) for x in z["label_names"]], z["label_counts"]))
    minima = dict(zip([str(x) for x in z["label_names"]], z["label_minima"]))
    assert set(counts) == set(ref.LABELS)
    for k, v in ref.MINIMA.items():
        assert v >= 1 and minima[k] == v and counts[k] >= v, (k, counts[k], v)
    assert set(ref.LABELS) - set(ref.MINIMA) == {"tie_cells", "tie_path_cells"}  # stored, no minimum
    for g in GROUPS:
        assert (fx.group == g).any(), g
    it = z["items"][fx.group == "shape"]
    shapes = {(int(a) - 5, int(b), int(c)) for a, b, c in
              zip(it["seq_len"], np.abs(it["event_stop"] - it["event_start"]) + 1, it["rc"])}
    assert shapes == ({(k, r, rc) for k in KMERS for r in ROWS for rc in (0, 1)}
                      | {(k, r, rc) for k in LONG_KMERS for r in LONG_ROWS for rc in (0, 1)})
    assert (z["items"]["flags"] == 0).all()
    typical = fx.sets[0][1].subset(np.flatnonzero(fx.group[fx.sets[0][0]] == "typical"))
    ratio = typical.n_rows / typical.n_kmers
    assert (typical.n_kmers >= 90).all() and (typical.n_kmers <= 100).all() and (ratio >= 1.15).all() and (ratio <= 2.5).all()
    # -infinity or NaN would compare equal to many wrong kernels
    assert np.isfinite(fx.want["l_fm"]).all()
    rd = fx.sets[0][1].reads
    assert (rd["events_per_base"] == 1.0).sum() >= 4 and (rd["var"] > 1.5).any() and (rd["var"] < 0.75).any()
    assert os.path.getsize(os.path.join(GOLDEN, "abea_viterbi_golden.npz")) <= 400 * 1024


@pytest.mark.parametrize("threads", [1, 5])
def test_host_path_equals_fixture(fx, host, threads):
    host.setenv("GB_ABEA_THREADS", str(threads))
    fx.check(abea.hmm_align)


def test_restatement_equals_fixture_on_small_items(fx):
    """The numpy restatement is checked against the live reference on every item by the recorder; here on the
    items of at most 1500 cells."""
    n = 0
    for idx, x in fx.sets:
        for i in np.flatnonzero(x.n_kmers * x.n_rows <= 1500):
            e, k, s, v = ref.align_item(x, int(i))
            w = fx.records(idx[i])
            assert (len(e) == len(w) and (e == w["event_idx"]).all() and (k == w["kmer_idx"]).all() and (s == w["state"]).all()
                    and (bits(v) == bits(w["l_fm"])).all()), (fx.group[idx[i]], x.items[i])
            n += 1
    assert n >= 60


def test_path_invariants(fx):
    """The first record is (event_start, 0, 'M'), the last (event_stop, last k-mer, 'M'), and there are rows + the
    number of 'K' records: in the fixture and out of the host path."""
    for idx, x in fx.sets:
        for j, i in enumerate(idx):
            w, it = fx.records(i), x.items[j]
            assert (w["event_idx"][0], w["kmer_idx"][0], w["state"][0]) == (it["event_start"], 0, b"M")
            assert (w["event_idx"][-1], w["kmer_idx"][-1], w["state"][-1]) == (it["event_stop"], x.n_kmers[j] - 1, b"M")
            assert len(w) == x.n_rows[j] + (w["state"] == b"K").sum() <= x.n_rows[j] + x.n_kmers[j] - 1
            assert (np.diff(w["kmer_idx"]) >= 0).all() and (np.diff(w["kmer_idx"]) <= 1).all() and (w["pad"] == 0).all()


def _small(seed=3):
    """Two reads of 8 k-mers and 12 rows, and a second item on each read: the same window again."""
    x = gen.abea_align_items(np.random.default_rng(seed), [(2, 8, 12)], quantum=QUANTUM)
    return gen.AbeaAlignItems(x.model, x.seqs, x.events, x.reads, np.repeat(x.items, 2))


REFUSALS = ["seq_len_5", "kmers_over", "rows_over", "rows_one", "event_stop_outside", "event_start_negative",
            "rc0_descending", "rc1_ascending", "rc_2", "flags_1", "flags_3", "read_index", "read_negative", "seq_off",
            "seq_off_negative", "event_off", "epb_nan", "epb_below_one", "p_mm_next", "var_zero", "var_inf", "log_var_nan",
            "scale_inf", "shift_nan", "event_nan", "event_inf", "model_mean_inf", "model_log_stdv_nan", "stdv_zero",
            "stdv_nan", "no_path", "budget", "budget_text"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_come_before_any_device_work_and_leave_the_outputs_untouched(case, monkeypatch):
    """No GB_ABEA_HOST here: every refusal comes before the device is touched, so none is needed."""
    from genomicsbench_palisade_amd import lib
    monkeypatch.delenv("GB_ABEA_HOST", raising=False)
    x = _small()
    model, seqs, events, reads, items = x.model.copy(), x.seqs, x.events.copy(), x.reads.copy(), x.items.copy()
    assert x.n == 4 and (items["read"] == [0, 0, 1, 1]).all()
    named = "item 3"
    if case == "seq_len_5":
        items["seq_len"][3] = 5
    elif case == "kmers_over":
        items["seq_len"][3] = abea.HMM_MAX_KMERS + 6
    elif case == "rows_over":
        events = np.full(abea.HMM_MAX_EVENTS + 8, 80.0, np.float32)
        reads["event_off"], reads["n_events"] = 0, len(events)
        items["rc"], items["event_start"], items["event_stop"] = 0, 0, 3
        items["event_stop"][3] = abea.HMM_MAX_EVENTS
    elif case == "rows_one":
        items["event_stop"][3] = items["event_start"][3]
    elif case == "event_stop_outside":
        items["rc"][3], items["event_start"][3], items["event_stop"][3] = 0, 2, reads["n_events"][1]
    elif case == "event_start_negative":
        items["rc"][3], items["event_start"][3], items["event_stop"][3] = 0, -1, 4
    elif case == "rc0_descending":
        items["rc"][3], items["event_start"][3], items["event_stop"][3] = 0, 9, 3
    elif case == "rc1_ascending":
        items["rc"][3], items["event_start"][3], items["event_stop"][3] = 1, 3, 9
    elif case == "rc_2":
        items["rc"][3] = 2
    elif case == "flags_1":
        items["flags"][3] = 1
    elif case == "flags_3":
        items["flags"][3] = 3
    elif case == "read_index":
        items["read"][3] = len(reads)
    elif case == "read_negative":
        items["read"][3] = -1
    elif case == "seq_off":
        items["seq_off"][3] = len(seqs) - items["seq_len"][3] + 1
    elif case == "seq_off_negative":
        items["seq_off"][3] = -1
    elif case == "event_off":
        reads["event_off"][1], named = len(events) - reads["n_events"][1] + 1, "read 1"
    elif case == "epb_nan":
        reads["events_per_base"][1], named = np.nan, "read 1"
    elif case == "epb_below_one":
        reads["events_per_base"][1], named = 0.99, "read 1"
    elif case == "p_mm_next":
        reads["events_per_base"][1], named = 1e6, "read 1"
    elif case == "var_zero":
        reads["var"][1], named = 0.0, "read 1"
    elif case == "var_inf":
        reads["var"][1], named = np.inf, "read 1"
    elif case == "log_var_nan":
        reads["log_var"][1], named = np.nan, "read 1"
    elif case == "scale_inf":
        reads["scale"][1], named = np.inf, "read 1"
    elif case == "shift_nan":
        reads["shift"][1], named = np.nan, "read 1"
    elif case == "event_nan":
        events[reads["event_off"][1] + 3], named = np.nan, "read 1"
    elif case == "event_inf":
        events[reads["event_off"][1] + 3], named = -np.inf, "read 1"
    elif case == "model_mean_inf":
        model[3077, 0], named = np.inf, "model entry 3077"
    elif case == "model_log_stdv_nan":
        model[3077, 2], named = np.nan, "model entry 3077"
    elif case == "stdv_zero":
        model[3077, 1], named = 0.0, "model entry 3077"
    elif case == "stdv_nan":
        model[3077, 1], named = np.nan, "model entry 3077"
    elif case == "no_path":  # one k-mer, two rows, lp_mm_self == -infinity: the last cell's six terms are -infinity
        reads["events_per_base"][1] = 1.0
        items["seq_len"][3] = 6
        items["event_stop"][3] = items["event_start"][3] + (-1 if items["rc"][3] else 1)
    elif case == "budget":  # an item of 8 k-mers and 12 rows needs 12 x 8 codes of 2 B and twice 19 records of 16 B
        monkeypatch.setenv("GB_ABEA_VITERBI_WS", str(12 * 8 * 2 + 2 * 19 * 16 - 1))
        named = "item 0"
    elif case == "budget_text":
        monkeypatch.setenv("GB_ABEA_VITERBI_WS", "1g")
        named = "GB_ABEA_VITERBI_WS"
    path = np.zeros(abea.hmm_align_need(x.items), abea.HMM_PATH_DTYPE)
    path["kmer_idx"] = 777
    off = np.full(len(items) + 1, -5, np.int64)
    st, p, o, used = abea.hmm_align_raw(model, seqs, events, reads, items, len(path), path, off)
    assert st == -1 and p is path and o is off and (path["kmer_idx"] == 777).all() and (off == -5).all() and used == -1
    assert named in lib().gb_last_error().decode()


def test_path_cap_one_short_is_refused_with_the_need(host):
    from genomicsbench_palisade_amd import lib
    x = _small()
    need = abea.hmm_align_need(x.items)
    assert need == 4 * (12 + 8 - 1)
    path = np.zeros(need, abea.HMM_PATH_DTYPE)
    path["kmer_idx"] = 777
    off = np.full(x.n + 1, -5, np.int64)
    st, _, _, used = abea.hmm_align_raw(x.model, x.seqs, x.events, x.reads, x.items, need - 1, path, off)
    assert st == -1 and used == need and (path["kmer_idx"] == 777).all() and (off == -5).all()
    assert str(need) in lib().gb_last_error().decode()
    st, _, off, used = abea.hmm_align_raw(x.model, x.seqs, x.events, x.reads, x.items, need, path)
    assert st == 0 and off[0] == 0 and off[-1] == used <= need


def test_no_items_succeed_without_a_device(monkeypatch):
    monkeypatch.delenv("GB_ABEA_HOST", raising=False)
    x = _small()
    st, path, off, used = abea.hmm_align_raw(x.model, x.seqs, x.events, x.reads, x.items[:0])
    assert st == 0 and len(path) == 0 and (off == [0]).all() and used == 0


def test_the_limits_themselves_are_accepted(host):
    """256 k-mers over two rows with events_per_base == 1.0 (lp_mm_self is then -infinity) is legal: 254 'K'."""
    x = gen.abea_align_items(np.random.default_rng(8), [(1, abea.HMM_MAX_KMERS, 2)], quantum=QUANTUM, epb=1.0)
    rec, off = abea.hmm_align(x)
    e, k, s, v = ref.align_item(x, 0)
    assert len(rec) == 2 + 254 and (rec["state"] == b"K").sum() == 254 and np.isfinite(rec["l_fm"]).all()
    assert (rec["event_idx"] == e).all() and (rec["kmer_idx"] == k).all() and (rec["state"] == s).all()
    assert (bits(rec["l_fm"]) == bits(v)).all()


def test_items_of_one_read_in_any_order_give_the_same_records(host):
    """Several windows of the same reads, in item order and shuffled."""
    rng = np.random.default_rng(21)
    x = gen.abea_align_items(rng, [(3, 30, 70), (2, 5, 9)], quantum=QUANTUM)
    items = []
    for it in x.items:  # three windows per read: the whole one, its first half and its second half
        step = -1 if it["rc"] else 1
        rows = abs(int(it["event_stop"]) - int(it["event_start"])) + 1
        a, b = it.copy(), it.copy()
        a["event_stop"] = it["event_start"] + step * (rows // 2 - 1)
        b["event_start"] = it["event_start"] + step * (rows // 2)
        items += [it, a, b]
    x = gen.AbeaAlignItems(x.model, x.seqs, x.events, x.reads, np.array(items))
    rec, off = abea.hmm_align(x)
    perm = rng.permutation(x.n)
    rec2, off2 = abea.hmm_align(x.subset(perm))
    for j, i in enumerate(perm):
        assert rec2[off2[j]:off2[j + 1]].tobytes() == rec[off[i]:off[i + 1]].tobytes()


def _mixed_set(seed, n_items):
    """Items over all size classes: most small, k-mers 1..256, rows 2..600 (0.5 to 3 per k-mer)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(CLASS_BOUNDS).T
    cls = rng.choice(4, n_items, p=[0.6, 0.25, 0.1, 0.05])
    nk = rng.integers(lo[cls], hi[cls] + 1)
    rows = np.clip((nk * rng.uniform(0.5, 3.0, n_items)).astype(int), 2, 600)
    return gen.abea_align_items(rng, [(1, int(k), int(r)) for k, r in zip(nk, rows)], non_acgt=0.002)


def test_host_path_equals_the_live_reference_on_fresh_items(host):
    sys.path.insert(0, GOLDEN)
    import make_abea_viterbi_golden as mk
    if not os.path.isdir(os.path.join(mk.REF_TREE, "benchmarks", "abea", "src")) or not shutil.which("g++"):
        pytest.skip("no reference tree or no compiler here")
    live = mk.LiveViterbi(mk.REF_TREE)
    try:
        x = _mixed_set(99, 60)
        rec, off = abea.hmm_align(x)
        for i, want in enumerate(live.align(x)):
            r = rec[off[i]:off[i + 1]]
            assert mk.equal((r["event_idx"], r["kmer_idx"], r["state"], r["l_fm"]), want), x.items[i]
    finally:
        live.close()


# ---- on the device ----


@pytest.fixture
def device(monkeypatch):
    monkeypatch.delenv("GB_ABEA_HOST", raising=False)
    monkeypatch.delenv("GB_ABEA_VITERBI_WS", raising=False)
    return monkeypatch


@pytest.mark.gpu
def test_device_equals_fixture_bit_for_bit(fx, device):
    fx.check(abea.hmm_align)
    fill, walk, cells = abea.hmm_align_timing()
    _, x = fx.sets[-1]  # the last call was the last set
    assert fill > 0 and walk > 0 and cells == x.cells()
    assert abea.hmm_align_plan()[0] == 1


@pytest.mark.gpu
def test_device_equals_fixture_with_its_items_shuffled(fx, device):
    rng = np.random.default_rng(12)
    fx.check(abea.hmm_align, select=lambda x: rng.permutation(x.n))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", range(4))
def test_device_equals_fixture_on_each_size_class_alone(fx, device, cls):
    lo, hi = CLASS_BOUNDS[cls]
    ran = []
    fx.check(lambda x: (ran.append(x.n), abea.hmm_align(x))[1],
             select=lambda x: np.flatnonzero((x.n_kmers >= lo) & (x.n_kmers <= hi)))
    # the shape grid alone gives a class 12 items per k-mer count of KMERS inside it, and each class has two
    assert sum(ran) >= 12 * sum(1 for k in KMERS if lo <= k <= hi) >= 24
    if cls == 0:  # a packed class that does not fill its last wave: 1, 2, 3 and 5 items
        small = lambda x: np.flatnonzero(x.n_kmers <= 16)  # noqa: E731
        for n in (1, 2, 3, 5):
            fx.check(abea.hmm_align, select=lambda x: small(x)[:n])


@pytest.mark.gpu
def test_device_equals_fixture_in_many_chunks(fx, device):
    """A workspace budget just above the largest item's need: the fixture runs in many chunks, to the same bytes."""
    idx, x = fx.sets[0]
    big = int(np.argmax(x.n_kmers * x.n_rows))
    assert (x.n_kmers[big], x.n_rows[big]) == (256, 2000)
    abea.hmm_align(x.subset([big]))
    chunks, need = abea.hmm_align_plan()
    assert chunks == 1 and need >= 2 * 256 * 2000
    device.setenv("GB_ABEA_VITERBI_WS", str(need + 1))
    seen = []
    fx.check(lambda x: (abea.hmm_align(x), seen.append(abea.hmm_align_plan()))[0])
    assert seen[0][0] > 4 and all(b <= need + 1 for _, b in seen)
    device.setenv("GB_ABEA_VITERBI_WS", str(need - 1))
    st, _, _, _ = abea.hmm_align_raw(x.model, x.seqs, x.events, x.reads, x.items)
    assert st == -1


@pytest.mark.gpu
def test_device_equals_host_path_on_a_second_set(device):
    x = _mixed_set(4242, 2000)
    assert x.n == 2000 and x.n_kmers.max() > 200 and x.n_rows.max() > 500 and x.n_rows.min() == 2
    d, doff = abea.hmm_align(x)
    fill, walk, cells = abea.hmm_align_timing()
    assert fill > 0 and walk > 0 and cells == x.cells()
    device.setenv("GB_ABEA_HOST", "1")
    h, hoff = abea.hmm_align(x)
    assert np.isfinite(h["l_fm"]).all() and (doff == hoff).all()
    bad = np.flatnonzero(d.view(np.uint8).reshape(-1, 16) != h.view(np.uint8).reshape(-1, 16))
    assert not len(bad), (len(bad), d[bad[0] // 16], h[bad[0] // 16])
