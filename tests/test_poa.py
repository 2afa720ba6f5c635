"""gb_poa_align / gb_poa_consensus against tests/golden/poa_golden.npz (tests/golden/make_poa_golden.py): spoa's
own six expected consensus strings of its sample.fastq, and the live SISD reference's pairs, views, consensus,
node counts and rank orders on generated windows. Without a GPU the host path (GB_POA_HOST=1) and the restatement
(tests/poa_ref.py) are held to the fixture; on the GPU the device is, bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import poa_ref
from conftest import GOLDEN, ROOT
from genomicsbench_palisade_amd import gen, lib, poa

LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
GROUPS = ("bench", "spoa-linear", "spoa-affine", "spoa-convex", "racon-linear", "weights")
ERR_ARG = -1


class Fixture:
    def __init__(self):
        z = self.z = np.load(os.path.join(GOLDEN, "poa_golden.npz"))
        self.param_names = [str(x) for x in z["param_names"]]
        self.params = [tuple(int(v) for v in row) for row in z["params"]]
        ro, rb, qb = z["read_off"], z["read_bytes"], z["qual_bytes"]
        self.windows, qpos = [], 0
        for w in range(len(z["win_group"])):
            a, b = z["win_read_off"][w], z["win_read_off"][w + 1]
            reads = [rb[ro[k]:ro[k + 1]].tobytes() for k in range(a, b)]
            quals = None
            if z["win_weighted"][w]:
                quals = []
                for r in reads:
                    quals.append(qb[qpos:qpos + len(r)].tobytes())
                    qpos += len(r)
            self.windows.append(dict(group=str(z["win_group"][w]), ps=int(z["win_params"][w]), reads=reads, quals=quals,
                                     cons=z["win_cons"][z["win_cons_off"][w]:z["win_cons_off"][w + 1]].tobytes(),
                                     nodes=int(z["win_nodes"][w]), done=int(z["win_done"][w]), cells=int(z["win_cells"][w]),
                                     rank_sum=int(z["win_rank_sum"][w])))
        self.items = []
        no, eo, so, po = z["item_node_off"], z["item_edge_off"], z["item_seq_off"], z["item_pair_off"]
        for k in range(len(z["item_win"])):
            n0, n1, e0, e1 = no[k], no[k + 1], eo[k], eo[k + 1]
            view = poa.View(z["node_base"][n0:n1], z["node_id"][n0:n1], z["node_out"][n0:n1], z["in_end"][n0:n1],
                            z["pred_rank"][e0:e1])
            self.items.append(dict(win=int(z["item_win"][k]), round=int(z["item_round"][k]), view=view,
                                   seq=z["item_seq"][so[k]:so[k + 1]].tobytes(), pairs=z["item_pairs"][po[k]:po[k + 1]],
                                   score=int(z["item_score"][k]), ps=self.windows[int(z["item_win"][k])]["ps"]))
        sro = z["sample_read_off"]
        self.sample_reads = [z["sample_reads"][sro[k]:sro[k + 1]].tobytes() for k in range(len(sro) - 1)]
        self.sample_quals = [z["sample_quals"][sro[k]:sro[k + 1]].tobytes() for k in range(len(sro) - 1)]
        seo = z["sample_expected_off"]
        self.sample = [(str(z["sample_tests"][k]), int(z["sample_params"][k]), bool(z["sample_weighted"][k]),
                        z["sample_expected"][seo[k]:seo[k + 1]].tobytes()) for k in range(len(seo) - 1)]

    def p(self, ps):
        return poa.params(*self.params[ps])

    def by_params(self, idx=None):
        """{parameter set: [item indices]} of the items idx (all by default), in order."""
        out = {}
        for k in (range(len(self.items)) if idx is None else idx):
            out.setdefault(self.items[k]["ps"], []).append(k)
        return out

    def cells(self, k):
        return self.items[k]["view"].n * len(self.items[k]["seq"])


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_POA_HOST", "1")
    return monkeypatch


@pytest.fixture
def device(monkeypatch):
    from genomicsbench_palisade_amd import set_device
    monkeypatch.delenv("GB_POA_HOST", raising=False)
    monkeypatch.delenv("GB_POA_WS", raising=False)
    set_device(0)
    return monkeypatch


def check_items(fx, idx, what=""):
    """gb_poa_align of the items idx (one call per parameter set, in the order given) equals the fixture."""
    for ps, ks in fx.by_params(idx).items():
        scores, pairs, off = poa.align(fx.p(ps), [fx.items[k]["view"] for k in ks], [fx.items[k]["seq"] for k in ks])
        assert off[0] == 0 and off[-1] == len(pairs)
        for i, k in enumerate(ks):
            it = fx.items[k]
            assert scores[i] == it["score"], f"{what} item {k}: score {scores[i]} vs {it['score']}"
            assert off[i + 1] - off[i] == len(it["pairs"]), f"{what} item {k}: {off[i + 1] - off[i]} pairs vs {len(it['pairs'])}"
            assert (pairs[off[i]:off[i + 1]] == it["pairs"]).all(), f"{what} item {k}: pairs differ"


def check_windows(fx, what=""):
    """gb_poa_consensus of the fixture's windows (one call per parameter set and weighting) equals the fixture."""
    calls = {}
    for w, win in enumerate(fx.windows):
        calls.setdefault((win["ps"], win["quals"] is not None), []).append(w)
    for (ps, weighted), ws in calls.items():
        cons, nodes, done = poa.consensus(fx.p(ps), [fx.windows[w]["reads"] for w in ws],
                                          [fx.windows[w]["quals"] for w in ws] if weighted else None)
        for i, w in enumerate(ws):
            assert cons[i] == fx.windows[w]["cons"], f"{what} window {w}: consensus differs"
            assert nodes[i] == fx.windows[w]["nodes"], f"{what} window {w}: {nodes[i]} nodes vs {fx.windows[w]['nodes']}"
        assert done == sum(fx.windows[w]["done"] for w in ws)
        assert poa.timing()[3] == sum(fx.windows[w]["cells"] for w in ws)


def check_sample(fx):
    for name, ps, weighted, expected in fx.sample:
        cons, nodes, done = poa.consensus(fx.p(ps), [fx.sample_reads], [fx.sample_quals] if weighted else None)
        assert cons[0] == expected, name
        assert done == len(fx.sample_reads) - 1


# ---- without a GPU ----

def test_fixture_labels_groups_and_shapes(fx):
    counts = dict(zip([str(x) for x in fx.z["label_names"]], [int(x) for x in fx.z["label_counts"]]))
    assert set(counts) == set(poa_ref.LABELS)
    for k, v in poa_ref.MINIMA.items():
        assert counts[k] >= v, (k, counts[k])
    assert sum(v >= 1 for v in poa_ref.MINIMA.values()) == len(poa_ref.LABELS) - 1  # all but up_q_open (poa_ref.py)
    assert {w["group"] for w in fx.windows} == set(GROUPS)
    subs = {ps: poa.subtype(fx.p(ps)) for ps in range(len(fx.params))}
    assert sorted(set(subs.values())) == [poa.LINEAR, poa.AFFINE, poa.CONVEX]
    assert subs[fx.param_names.index("bench")] == poa.CONVEX
    for sub in (poa.LINEAR, poa.AFFINE, poa.CONVEX):
        lens = {len(it["seq"]) for it in fx.items if subs[it["ps"]] == sub}
        assert set(LENGTHS) <= lens, (sub, sorted(set(LENGTHS) - lens))
        assert any(850 <= n <= 870 for n in lens), sub
    n_reads = {len(w["reads"]) for w in fx.windows}
    assert {1, 2, 3, 8} <= n_reads and any(28 <= n <= 32 for n in n_reads) and max(n_reads) >= 100
    assert any(b"" in w["reads"] for w in fx.windows)
    assert any(set(b"".join(w["reads"])) - set(b"ACGT") for w in fx.windows)
    assert any(len(it["seq"]) * 4 < it["view"].n for it in fx.items) and any(len(it["seq"]) > 2 * it["view"].n for it in fx.items)
    assert any((1 - it["view"].out.astype(int)).sum() >= 2 for it in fx.items)  # more than one sink
    assert max(int(np.diff(np.concatenate([[0], it["view"].in_end])).max()) for it in fx.items) >= 4
    assert os.path.getsize(os.path.join(GOLDEN, "poa_golden.npz")) <= 400 * 1024


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_align_equals_fixture(fx, host, threads):
    host.setenv("GB_POA_THREADS", threads)
    check_items(fx, None, "host")
    assert poa.plan() == (0, 0)


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_consensus_equals_fixture(fx, host, threads):
    host.setenv("GB_POA_THREADS", threads)
    check_windows(fx, "host")


def test_host_gives_the_six_spoa_strings(fx, host):
    check_sample(fx)


def test_restatement_equals_fixture_on_a_thinned_subset(fx):
    """Every alignment item of at most 12 000 cells whose index is a multiple of 3 (pairs and score), and every
    fourth window of at most 60 000 cells (consensus, node count, alignments, cells, rank order)."""
    ran = 0
    for k, it in enumerate(fx.items):
        if k % 3 == 0 and fx.cells(k) <= 12_000:
            v = poa_ref.View(it["view"].base, it["view"].id, it["view"].out, it["view"].in_end, it["view"].pred)
            pairs, score = poa_ref.align(fx.params[it["ps"]], v, it["seq"])
            assert pairs == [(int(a), int(b)) for a, b in it["pairs"]] and score == it["score"], k
            ran += 1
    assert ran >= 40
    ran = 0
    for w, win in enumerate(fx.windows):
        if w % 4 == 0 and win["cells"] <= 60_000:
            wt = None if win["quals"] is None else [[b - 33 for b in q] for q in win["quals"]]
            got = poa_ref.window(fx.params[win["ps"]], win["reads"], wt)
            assert got == (win["cons"], win["nodes"], win["done"], win["cells"], win["rank_sum"]), w
            ran += 1
    assert ran >= 10


def test_alignment_invariants(fx, host):
    """Sequence positions are 0 .. len - 1, each exactly once and ascending; the node ids' ranks never go down."""
    for ps, ks in fx.by_params().items():
        _, pairs, off = poa.align(fx.p(ps), [fx.items[k]["view"] for k in ks], [fx.items[k]["seq"] for k in ks])
        for i, k in enumerate(ks):
            it, pr = fx.items[k], pairs[off[i]:off[i + 1]]
            pos = pr[:, 1][pr[:, 1] >= 0]
            assert (pos == np.arange(len(it["seq"]))).all(), k
            rank_of = np.full(int(it["view"].id.max()) + 1, -1)
            rank_of[it["view"].id] = np.arange(it["view"].n)
            ranks = rank_of[pr[:, 0][pr[:, 0] >= 0]]
            assert (ranks >= 0).all() and (np.diff(ranks) > 0).all(), k
            assert not ((pr[:, 0] == -1) & (pr[:, 1] == -1)).any()


def small_batch(fx):
    ks = [k for k in fx.by_params()[fx.param_names.index("bench")] if 200 <= fx.cells(k) <= 5000][:3]
    assert len(ks) == 3 and all(len(fx.items[k]["view"].pred) >= 3 for k in ks)
    return poa.Batch([fx.items[k]["view"] for k in ks], [fx.items[k]["seq"] for k in ks])


def _item(b, **kw):
    items = b.items.copy()
    for f, v in kw.items():
        items[1][f] = v
    return dict(items=items)


def _unsorted(b):
    r = int(np.nonzero(np.diff(np.concatenate([[0], b.in_end[b.items[1]["node_off"]:][:b.items[1]["n_nodes"]]])) > 0)[0][-1])
    e = int(b.items[1]["edge_off"]) + (int(b.in_end[b.items[1]["node_off"] + r - 1]) if r else 0)
    b.pred[e] = r
    return {}


def _range_outside(b):
    b.in_end[b.items[1]["node_off"] + 2] = b.items[1]["n_edges"] + 1
    return {}


# (name, parameters or None for the benchmark's, change to the batch, environment, words of the message)
REFUSALS = [
    ("type kSW", dict(type=poa.SW), None, {}, ["kSW"]),
    ("type kOV", dict(type=poa.OV), None, {}, ["kOV"]),
    ("type 7", dict(type=7), None, {}, ["invalid alignment type"]),
    ("positive g", dict(g=1), None, {}, ["gap opening penalty must be non-positive!"]),
    ("positive q", dict(q=3), None, {}, ["gap opening penalty must be non-positive!"]),
    ("positive e", dict(e=1), None, {}, ["gap extension penalty must be non-positive!"]),
    ("positive c", dict(c=2), None, {}, ["gap extension penalty must be non-positive!"]),
    ("negative length", None, lambda b: _item(b, seq_len=-1), {}, ["item 1", "-1 bases"]),
    ("negative node count", None, lambda b: _item(b, n_nodes=-2), {}, ["item 1", "-2 nodes"]),
    ("length over the limit", None, lambda b: _item(b, seq_len=poa.MAX_LEN + 1), {}, ["item 1", str(poa.MAX_LEN + 1)]),
    ("nodes over the limit", None, lambda b: _item(b, n_nodes=poa.MAX_NODES + 1), {}, ["item 1", str(poa.MAX_NODES + 1)]),
    ("sequence outside", None, lambda b: _item(b, seq_off=len(b.seqs) - 1), {}, ["item 1", "sequence outside"]),
    ("view outside", None, lambda b: _item(b, node_off=len(b.base) - 1), {}, ["item 1", "view outside"]),
    ("edges outside", None, lambda b: _item(b, edge_off=len(b.pred) - 1), {}, ["item 1", "in-edges outside"]),
    ("not topologically sorted", None, _unsorted, {}, ["item 1", "not topologically sorted"]),
    ("in-edge range outside", None, _range_outside, {}, ["item 1", "in-edge range"]),
    ("no node but in-edges", None, lambda b: _item(b, n_nodes=0), {}, ["item 1", "no node but"]),
    ("budget too small", None, None, {"GB_POA_WS": "4096"}, ["item ", "more than the budget of 4096"]),
    ("budget text", None, None, {"GB_POA_WS": "12k"}, ["GB_POA_WS is '12k'"]),
]


@pytest.mark.parametrize("name,pkw,change,env,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_first_and_leave_the_outputs(fx, monkeypatch, name, pkw, change, env, words):
    """GB_ERR_ARG before any device work (the budget cases run without GB_POA_HOST: the budget is checked before
    the first HIP call), outputs as they were, the item named."""
    b = small_batch(fx)
    if env:
        monkeypatch.delenv("GB_POA_HOST", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    else:
        monkeypatch.setenv("GB_POA_HOST", "1")
    p = poa.params(*poa.BENCH)
    for f, v in (pkw or {}).items():
        p[0][f] = v
    kw = change(b) if change else {}
    st, scores, pairs, off, used = poa.align_raw(p, b, **kw)
    msg = lib().gb_last_error().decode()
    assert st == ERR_ARG, (st, msg)
    for w in words:
        assert w in msg, msg
    assert (scores == -7).all() and (pairs == -9).all() and (off == -1).all() and used == -1


def test_consensus_refusals(fx, host):
    win_off, seq_off, data, _ = poa.pack_windows([w["reads"] for w in fx.windows[:4]])
    p = poa.params(*poa.BENCH)

    def untouched(r):
        st, cons, off, used, nodes, done = r
        assert st == ERR_ARG and (cons == 0x21).all() and (off == -1).all() and (nodes == -7).all() and done == -1
        return used, lib().gb_last_error().decode()

    bad = win_off.copy()
    bad[2] = len(seq_off)
    used, msg = untouched(poa.consensus_raw(p, bad, seq_off, data))
    assert used == -1 and "window 1" in msg
    bad = seq_off.copy()
    bad[3] = bad[2] - 1
    used, msg = untouched(poa.consensus_raw(p, win_off, bad, data))
    assert used == -1 and "sequence 2" in msg
    q = p.copy()
    q[0]["type"] = poa.SW
    used, msg = untouched(poa.consensus_raw(q, win_off, seq_off, data))
    assert "kSW" in msg
    need = len(data)
    used, msg = untouched(poa.consensus_raw(p, win_off, seq_off, data, cons_cap=need - 1))
    assert used == need and str(need) in msg
    st, cons, off, used, nodes, done = poa.consensus_raw(p, win_off, seq_off, data, cons_cap=need)
    assert st == 0 and [cons[off[w]:off[w + 1]].tobytes() for w in range(4)] == [w["cons"] for w in fx.windows[:4]]


def test_cap_one_short_is_refused_with_the_need(fx, host):
    b = small_batch(fx)
    p, need = poa.params(*poa.BENCH), b.need()
    st, scores, pairs, off, used = poa.align_raw(p, b, pair_cap=need - 1)
    assert st == ERR_ARG and used == need and str(need) in lib().gb_last_error().decode()
    assert (scores == -7).all() and (pairs == -9).all() and (off == -1).all()
    st, scores, pairs, off, used = poa.align_raw(p, b, pair_cap=need)
    assert st == 0 and 0 < used <= need and off[-1] == used


def test_zero_items_zero_windows_and_empty_windows(fx, host):
    p = poa.params(*poa.BENCH)
    st, scores, pairs, off, used = poa.align_raw(p, poa.Batch([], []))
    assert st == 0 and used == 0 and off[0] == 0
    cons, nodes, done = poa.consensus(p, [])
    assert cons == [] and done == 0
    cons, nodes, done = poa.consensus(p, [[b""], [], [b"", b""], [b"ACGT"]])
    assert cons == [b"", b"", b"", b"ACGT"] and list(nodes) == [0, 0, 0, 4] and done == 0
    # an item with no node or no base owns no pair and scores 0
    v = fx.items[0]["view"]
    scores, pairs, off = poa.align(p, [poa.View([], [], [], [], []), v], [b"ACGT", b""])
    assert list(scores) == [0, 0] and len(pairs) == 0 and list(off) == [0, 0, 0]


def test_the_length_limit_itself(host):
    p = poa.params(*poa.BENCH)
    one = poa.View([65], [0], [0], [0], [])
    seq = np.full(poa.MAX_LEN, 65, np.uint8)
    scores, pairs, off = poa.align(p, [one], [seq])
    assert len(pairs) == poa.MAX_LEN and (pairs[:, 1] == np.arange(poa.MAX_LEN)).all()
    assert (pairs[:, 0] >= 0).sum() == 1 and scores[0] == 2 - 25 - (poa.MAX_LEN - 2)
    st = poa.align_raw(p, poa.Batch([one], [np.full(poa.MAX_LEN + 1, 65, np.uint8)]))[0]
    assert st == ERR_ARG and str(poa.MAX_LEN + 1) in lib().gb_last_error().decode()


def test_bin_poa_prints_the_consensus(tmp_path):
    exe = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "poa")
    assert os.path.exists(exe), f"{exe} not built (make)"
    rng = np.random.default_rng(5)
    windows = gen.poa_windows(rng, 6, reads=(1, 9), length=(20, 120), long_indel=0.004)
    path = str(tmp_path / "in.fasta")
    gen.write_poa_file(path, windows)
    env = dict(os.environ, GB_POA_HOST="1")
    for args, pr in (([], poa.BENCH), (["-m", "5", "-x", "4", "-o", "2,6", "-e", "6,2", "-n", "3"], (5, -4, -8, -6, -8, -2))):
        out = subprocess.run([exe, "-s", path, "-t", "2"] + args, env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        os.environ["GB_POA_HOST"] = "1"
        try:
            cons, _, _ = poa.consensus(poa.params(*pr), windows)
        finally:
            del os.environ["GB_POA_HOST"]
        assert out.stdout == "".join(">Consensus_sequence\n%s\n" % c.decode() for c in cons)
    for flag in ("-o", "-e"):
        out = subprocess.run([exe, "-s", path, flag, "4"], env=env, capture_output=True, text=True)
        assert out.returncode != 0 and "two values" in out.stderr


def test_live_cross_check_of_fresh_windows(host):
    """Fresh seeded windows through the reference's spoa, compiled as the recorder compiles it."""
    sys.path.insert(0, GOLDEN)
    import make_poa_golden as mk
    if not os.path.isdir(mk.spoa_dir()) or not shutil.which("g++"):
        pytest.skip("no reference tree or no compiler")
    live = mk.LivePoa()
    try:
        rng = np.random.default_rng(77)
        for name in ("bench", "spoa-linear", "spoa-affine", "spoa-convex"):
            windows = gen.poa_windows(rng, 6, reads=(2, 10), length=(20, 160), err=0.15, long_indel=0.005, clip=0.3)
            cons, nodes, done = poa.consensus(poa.params(*mk.PARAM_SETS[name]), windows)
            for w, reads in enumerate(windows):
                views, seqs, want = [], [], []
                exp = live.window(mk.PARAM_SETS[name], reads,
                                  on_alignment=lambda k, v, r, pr: (views.append(poa.View(*v)), seqs.append(r), want.append(pr.copy())))
                assert (cons[w], nodes[w]) == (exp[0], exp[1]), (name, w)
                _, pairs, off = poa.align(poa.params(*mk.PARAM_SETS[name]), views, seqs)
                for i in range(len(views)):
                    assert (pairs[off[i]:off[i + 1]] == want[i]).all(), (name, w, i)
    finally:
        live.close()


# ---- on the GPU ----

def class_of(it):
    return poa.size_class(len(it["seq"]))


@pytest.mark.gpu
def test_device_align_equals_fixture(fx, device):
    check_items(fx, None, "device")
    chunks, ws = poa.plan()
    assert chunks == 1 and ws > 0


@pytest.mark.gpu
def test_device_align_shuffled(fx, device):
    order = np.random.default_rng(3).permutation(len(fx.items))
    check_items(fx, [int(k) for k in order], "shuffled")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [poa.CLASS_WAVE, poa.CLASS_GROUP], ids=["wave", "group"])
def test_device_each_size_class_alone(fx, device, cls):
    """The items of one class only, per parameter set, and launches of 1, 2, 3 and 5 of them."""
    ks = [k for k in range(len(fx.items)) if class_of(fx.items[k]) == cls]
    assert len(ks) >= 9
    assert {len(fx.items[k]["seq"]) for k in ks} >= ({255, 256} if cls == poa.CLASS_WAVE else {257})
    check_items(fx, ks, "class")
    for ps, mine in fx.by_params(ks).items():
        for n in (1, 2, 3, 5):
            if len(mine) >= n:
                check_items(fx, mine[-n:], f"launch of {n}")


@pytest.mark.gpu
def test_device_long_class_equals_host(device):
    """Sequences above GROUP_MAX_LEN bases (more than four columns a thread): the device equals the host path, which
    the fixture holds to the reference, on chains with skip edges at every subtype and on whole windows."""
    rng = np.random.default_rng(11)
    views, seqs = [], []
    for n, L in ((900, 1025), (1200, 1100), (40, 1500), (1300, 2049), (1024, 1024 + 256 * 3 + 1)):
        t = np.frombuffer(gen.poa_template(rng, n), np.uint8)
        in_end, pred = [], []
        for r in range(n):
            pred += [r - 1] if r else []
            pred += [r - 3] if r >= 3 and r % 7 == 0 else []
            in_end.append(len(pred))
        views.append(poa.View(t, rng.permutation(n), [1] * (n - 1) + [0], in_end, pred))
        seq = gen.poa_read(rng, gen.poa_template(rng, 30) + t.tobytes() * (L // n + 2), 0.05, 0.05, 0.05, 0.002)[:L]
        assert len(seq) == L and poa.size_class(L) == poa.CLASS_LONG
        seqs.append(seq)
    windows = [gen.poa_window(rng, 4, L, err=0.1)[0] for L in (1100, 1300)]
    for pr in (poa.BENCH, (5, -4, -8, -8, -8, -8), (5, -4, -8, -6, -8, -6)):
        p = poa.params(*pr)
        got = poa.align(p, views, seqs)
        got_w = poa.consensus(p, windows)
        device.setenv("GB_POA_HOST", "1")
        exp = poa.align(p, views, seqs)
        exp_w = poa.consensus(p, windows)
        device.delenv("GB_POA_HOST")
        assert all((a == b).all() for a, b in zip(got, exp)), pr
        assert got_w[0] == exp_w[0] and (got_w[1] == exp_w[1]).all() and got_w[2] == exp_w[2], pr


@pytest.mark.gpu
def test_device_in_many_chunks(fx, device):
    """A budget just above the largest item's need cuts the call into many chunks; one byte less refuses it."""
    ps = fx.param_names.index("bench")
    ks = [k for k in fx.by_params()[ps] if fx.cells(k) <= 60_000]
    sub = poa.subtype(fx.p(ps))
    need = [poa.item_bytes(sub, fx.items[k]["view"].n, len(fx.items[k]["seq"])) for k in ks]
    big = max(need)
    device.setenv("GB_POA_WS", str(big))
    check_items(fx, ks, "chunks")
    chunks, ws = poa.plan()
    assert chunks >= 5 and ws <= big
    # the greedy cut, restated
    exp, cur = 1, 0
    for b in need:
        if cur and cur + b > big:
            exp, cur = exp + 1, 0
        cur += b
    assert chunks == exp
    device.setenv("GB_POA_WS", str(big - 1))
    b = poa.Batch([fx.items[k]["view"] for k in ks], [fx.items[k]["seq"] for k in ks])
    st, scores, pairs, off, used = poa.align_raw(fx.p(ps), b)
    msg = lib().gb_last_error().decode()
    assert st == ERR_ARG and f"item {int(np.argmax(need))} needs {big} bytes" in msg, msg
    assert (scores == -7).all() and (pairs == -9).all() and (off == -1).all() and used == -1


@pytest.mark.gpu
def test_device_consensus_equals_fixture_and_spoa(fx, device):
    check_windows(fx, "device")
    check_sample(fx)


@pytest.fixture(scope="module")
def second_set():
    rng = np.random.default_rng(2026)
    windows = gen.poa_windows(rng, 300, reads=(2, 12), length=(20, 300), err=0.12, long_indel=0.002, clip=0.2)
    windows += [gen.poa_window(rng, 30, 850, err=0.12)[0] for _ in range(3)]
    os.environ["GB_POA_HOST"] = "1"
    try:
        exp = poa.consensus(poa.params(*poa.BENCH), windows)
        cells = poa.timing()[3]
    finally:
        del os.environ["GB_POA_HOST"]
    return windows, exp, cells


@pytest.mark.gpu
def test_device_equals_host_on_a_second_set(second_set, device):
    windows, (cons, nodes, done), cells = second_set
    got = poa.consensus(poa.params(*poa.BENCH), windows)
    assert got[0] == cons and (got[1] == nodes).all() and got[2] == done
    fill_ms, walk_ms, host_ms, got_cells = poa.timing()
    assert got_cells == cells and fill_ms > 0 and walk_ms > 0 and host_ms > 0


@pytest.mark.gpu
def test_device_timing_cells_and_plan_bytes(fx, device):
    ps = fx.param_names.index("spoa-affine")
    ks = fx.by_params()[ps]
    check_items(fx, ks, "plan")
    sub = poa.subtype(fx.p(ps))
    assert sub == poa.AFFINE
    assert poa.timing()[3] == sum(fx.cells(k) for k in ks)
    assert poa.plan() == (1, sum(poa.item_bytes(sub, fx.items[k]["view"].n, len(fx.items[k]["seq"])) for k in ks))
    n, L = fx.items[ks[0]]["view"].n, len(fx.items[ks[0]]["seq"])
    assert poa.item_bytes(sub, n, L) == (3 * (n + 1) * (L + 1) + 3) // 4 * 16 + 8 * (n + L)
    win = [w for w in fx.windows if w["ps"] == ps and w["quals"] is None][:5]
    poa.consensus(fx.p(ps), [w["reads"] for w in win])
    assert poa.timing()[3] == sum(w["cells"] for w in win)


@pytest.mark.gpu
def test_device_after_lds_poison(fx, device):
    """The workgroup-class kernel passes its waves' scan totals through LDS: one run of the alignment items after
    every CU's LDS has been filled with each pattern of tests/cpp/lds_poison.hip."""
    import ctypes
    path = os.path.join(ROOT, "tests", "_build", "liblds_poison.so")
    assert os.path.exists(path), f"{path} not built (make)"
    L = ctypes.CDLL(path)
    L.lds_poison.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    ks = [k for k in range(len(fx.items)) if class_of(fx.items[k]) == poa.CLASS_GROUP or k % 4 == 0]
    for mode, value in [(0, 0), (1, 0), (2, 2), (2, 37), (2, 300), (3, 1000), (4, 0)]:
        assert L.lds_poison(0, mode, value, 1) == 0
        check_items(fx, ks, f"pattern {(mode, value)}")
