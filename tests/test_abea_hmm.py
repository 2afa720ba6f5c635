"""gb_abea_hmm_score (methylation profile-HMM scores) against tests/golden/abea_hmm_golden.npz, recorded from f5c's
CPU profile_hmm_score by tests/golden/make_abea_hmm_golden.py.

Without a GPU: the host path (GB_ABEA_HOST=1) on the whole fixture bit for bit with one thread and with several,
the log-sum table, the refusals, the numpy restatement on the fixture's small items, the identity of the two
flank tables, and a live cross-check of fresh items where the reference tree and a compiler are present. On the
GPU: the whole fixture bit for bit, shuffled and with each size class alone, the device against the host path on
a second seeded set, and the timing call.
"""
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN, bits

import abea_hmm_ref as ref
from genomicsbench_palisade_amd import abea, gen

QUANTUM = 0.125
KMERS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 216, 256)
ROWS = (1, 2, 3, 10, 63, 64, 65, 300, 2000)
GROUPS = ("shape", "typical", "meth", "nonacgmt", "epb_one", "outlier", "grid", "scaled")
CLASS_BOUNDS = ((1, 16), (17, 64), (65, 128), (129, 256))  # k-mers per size class of the kernel


class Fixture:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "abea_hmm_golden.npz"))
        self.z = z
        self.group = np.array([str(g) for g in z["group"]])
        self.want = z["score_bits"]
        models = np.stack([z["model_mean_q"].astype(np.float32) / np.float32(64),
                           z["model_stdv_q"].astype(np.float32) / np.float32(128), z["model_log_stdv"]], -1)
        events = z["events_q"].astype(np.float32) * np.float32(QUANTUM)
        self.sets = []  # (item indices, AbeaHmmItems) per model
        for mid in range(len(models)):
            idx = np.flatnonzero(z["model_id"] == mid)
            self.sets.append((idx, gen.AbeaHmmItems(models[mid], z["seqs"], events, z["reads"], z["items"][idx])))
        self.n = len(self.want)

    def check(self, run, select=None):
        """run(AbeaHmmItems) -> scores, compared bit for bit; select(AbeaHmmItems) -> indices to run (all)."""
        for idx, x in self.sets:
            sel = np.arange(x.n) if select is None else np.asarray(select(x), np.int64)
            if not len(sel):
                continue
            got = bits(run(x.subset(sel)))
            bad = np.flatnonzero(got != self.want[idx[sel]])
            assert not len(bad), (len(bad), self.group[idx[sel[bad]]][:5], x.items[sel[bad]][:5],
                                  got[bad][:5].view(np.float32), self.want[idx[sel[bad]]][:5].view(np.float32))


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
    for k in ref.LABELS:
        assert minima[k] >= 1 and counts[k] >= minima[k], (k, counts[k], minima[k])
    for g in GROUPS:
        assert (fx.group == g).any(), g
    it = z["items"][fx.group == "shape"]
    shapes = {(int(a) - 5, int(b), int(c), int(d)) for a, b, c, d in
              zip(it["seq_len"], np.abs(it["event_stop"] - it["event_start"]) + 1, it["rc"], it["flags"])}
    assert shapes == {(k, r, rc, f) for k in KMERS for r in ROWS for rc in (0, 1) for f in range(4)}
    # -infinity or NaN would compare equal to many wrong kernels
    assert np.isfinite(fx.want.view(np.float32)).all()
    idx, x = fx.sets[0]
    assert ((x.reads["events_per_base"] == 1.0).sum() >= 4 and (x.reads["var"] > 1.5).any() and (x.reads["var"] < 0.75).any())


def test_logsum_table_equals_fixture_and_restatement(fx):
    t = abea.hmm_logsum_table()
    assert (bits(t) == fx.z["table_bits"]).all()
    assert (bits(ref.logsum_table()) == fx.z["table_bits"]).all()


@pytest.mark.parametrize("threads", [1, 5])
def test_host_path_equals_fixture(fx, host, threads):
    host.setenv("GB_ABEA_THREADS", str(threads))
    fx.check(abea.hmm_score)


def test_restatement_equals_fixture_on_small_items(fx):
    """The numpy restatement is checked against the live reference on every item by the recorder; here on the
    items of at most 1500 cells, every twelfth of them, plus every grid item of that size."""
    n = 0
    for mid, (idx, x) in enumerate(fx.sets):
        small = np.flatnonzero(x.n_kmers * x.n_rows <= 1500)
        pick = small if mid == 1 else small[::12]  # model 1 is the grid's
        for i in pick:
            assert bits(np.array([ref.score_item(x, int(i))]))[0] == fx.want[idx[i]], (fx.group[idx[i]], x.items[i])
            n += 1
    assert n >= 40


@pytest.mark.parametrize("n", [1, 2, 3, 64, 2000])
def test_post_flank_is_pre_flank_reversed(n):
    """One table indexed by distance serves both (the library keeps only that one)."""
    pre, post = ref.pre_flank(n), ref.post_flank(n)
    assert len(pre) == n + 1 and len(post) == n
    assert (bits(post) == bits(pre[:n][::-1])).all()


def _small(seed=3):
    return gen.abea_hmm_items(np.random.default_rng(seed), [(2, 8, 12)], quantum=QUANTUM)


REFUSALS = ["seq_len_5", "kmers_over", "rows_over", "event_stop_outside", "event_start_negative", "rc0_descending",
            "rc1_ascending", "rc_2", "flags_4", "read_index", "read_negative", "seq_off", "seq_off_negative", "event_off",
            "epb_nan", "epb_below_one", "p_mm_next", "var_zero", "var_inf", "log_var_nan", "scale_inf", "shift_nan",
            "event_nan", "event_inf", "model_mean_inf", "model_log_stdv_nan", "stdv_zero", "stdv_nan"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_come_before_any_device_work_and_leave_scores_untouched(case):
    """No GB_ABEA_HOST here: every refusal comes before the device is touched, so none is needed."""
    from genomicsbench_palisade_amd import lib
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
    elif case == "flags_4":
        items["flags"][3] = 4
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
        model[9077, 0], named = np.inf, "model entry 9077"
    elif case == "model_log_stdv_nan":
        model[9077, 2], named = np.nan, "model entry 9077"
    elif case == "stdv_zero":
        model[9077, 1], named = 0.0, "model entry 9077"
    elif case == "stdv_nan":
        model[9077, 1], named = np.nan, "model entry 9077"
    scores = np.full(len(items), 777.0, np.float32)
    st, out = abea.hmm_score_raw(model, seqs, events, reads, items, scores)
    assert st == -1 and out is scores and (scores == 777.0).all()
    assert named in lib().gb_last_error().decode()


def test_no_items_succeed_without_a_device():
    x = _small()
    st, out = abea.hmm_score_raw(x.model, x.seqs, x.events, x.reads, x.items[:0])
    assert st == 0 and len(out) == 0


def test_the_limits_themselves_are_accepted(host):
    """256 k-mers and events_per_base == 1.0 (lp_mm_self is then -infinity) are legal."""
    x = gen.abea_hmm_items(np.random.default_rng(8), [(1, abea.HMM_MAX_KMERS, 5)], quantum=QUANTUM, epb=1.0)
    s = abea.hmm_score(x)
    assert np.isfinite(s).all()
    assert bits(s)[0] == bits(np.array([ref.score_item(x, 0)]))[0]


def _mixed_set(seed, n_reads):
    """Reads over all size classes, two items each: most small, rows 0.5 to 3 per k-mer."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(CLASS_BOUNDS).T
    cls = rng.choice(4, n_reads, p=[0.6, 0.25, 0.1, 0.05])
    nk = rng.integers(lo[cls], hi[cls] + 1)
    rows = np.clip((nk * rng.uniform(0.5, 3.0, n_reads)).astype(int), 1, 500)
    return gen.abea_hmm_items(rng, [(1, int(k), int(r)) for k, r in zip(nk, rows)], flags=[0, 1, 2, 3], non_acgmt=0.002)


def test_host_path_equals_the_live_reference_on_fresh_items(host):
    sys.path.insert(0, GOLDEN)
    import make_abea_hmm_golden as mk
    if not os.path.isdir(os.path.join(mk.REF_TREE, "benchmarks", "abea", "src")) or not shutil.which("g++"):
        pytest.skip("no reference tree or no compiler here")
    live = mk.LiveHmm(mk.REF_TREE)
    try:
        x = _mixed_set(99, 60)
        assert (bits(abea.hmm_score(x)) == bits(live.scores(x))).all()
    finally:
        live.close()


# ---- on the device ----


@pytest.fixture
def device(monkeypatch):
    monkeypatch.delenv("GB_ABEA_HOST", raising=False)
    return monkeypatch


@pytest.mark.gpu
def test_device_equals_fixture_bit_for_bit(fx, device):
    fx.check(abea.hmm_score)
    ms, cells = abea.hmm_timing()
    _, x = fx.sets[-1]  # the last call was the last set
    assert ms > 0 and cells == x.cells()


@pytest.mark.gpu
def test_device_equals_fixture_with_its_items_shuffled(fx, device):
    rng = np.random.default_rng(12)
    fx.check(abea.hmm_score, select=lambda x: rng.permutation(x.n))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", range(4))
def test_device_equals_fixture_on_each_size_class_alone(fx, device, cls):
    lo, hi = CLASS_BOUNDS[cls]
    ran = []
    fx.check(lambda x: (ran.append(x.n), abea.hmm_score(x))[1],
             select=lambda x: np.flatnonzero((x.n_kmers >= lo) & (x.n_kmers <= hi)))
    # the shape grid alone gives a class 72 items per k-mer count of KMERS inside it, and each class has two
    assert sum(ran) >= 72 * sum(1 for k in KMERS if lo <= k <= hi) >= 144
    if cls == 0:  # a packed class that does not fill its last wave: 1, 2, 3 and 5 items
        idx, x = fx.sets[0]
        small = np.flatnonzero(x.n_kmers <= 16)
        for n in (1, 2, 3, 5):
            assert (bits(abea.hmm_score(x.subset(small[:n]))) == fx.want[idx[small[:n]]]).all()


@pytest.mark.gpu
def test_device_equals_host_path_on_a_second_set(device):
    x = _mixed_set(4242, 1000)
    assert x.n == 2000
    d = abea.hmm_score(x)
    ms, cells = abea.hmm_timing()
    assert ms > 0 and cells == x.cells()
    device.setenv("GB_ABEA_HOST", "1")
    h = abea.hmm_score(x)
    assert np.isfinite(h).mean() > 0.99
    bad = np.flatnonzero(bits(d) != bits(h))
    assert not len(bad), (len(bad), x.items[bad][:5], d[bad][:5], h[bad][:5])
