"""gb_poa_align / gb_poa_consensus against tests/golden/poa_edges_golden.npz (tests/poa_edges.py,
tests/golden/make_poa_edges_golden.py): the live SISD reference's pairs on sequences at every change of the fill
kernel's column split and size class, with gaps whose origin lies several waves to the left, on sixteen parameter
sets at the boundaries of spoa's subtype rule, and at GB_POA_MAX_LEN. Without a GPU the host path (GB_POA_HOST=1)
and the restatement (tests/poa_ref.py) are held to the fixture; on the GPU the device is, bit for bit."""
import os
import shutil
import sys

import numpy as np
import pytest

import poa_edges as pe
import poa_ref
from conftest import GOLDEN
from genomicsbench_palisade_amd import gen, poa

PATH = os.path.join(GOLDEN, "poa_edges_golden.npz")
GROUP_LENGTHS = {511, 512, 513, 767, 768, 769, 1023, 1024}
LONG_LENGTHS = {1025, 1279, 1280, 1281}


@pytest.fixture(scope="module")
def fx():
    return pe.Fixture(PATH)


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


def align_limit(fx):
    """(score, pairs) of the length-limit item."""
    scores, pairs, off = poa.align(fx.p("bench"), [fx.limit["view"]], [fx.limit["seq"]])
    assert list(off) == [0, len(pairs)]
    return int(scores[0]), pairs


def check_limit(fx, pairs):
    assert len(pairs) == fx.limit["n_pairs"] and pe.checksum(pairs) == fx.limit["pair_sum"]
    assert (pairs[:, 1][pairs[:, 1] >= 0] == np.arange(poa.MAX_LEN)).all()
    assert pe.longest_inserted_run(pairs) >= poa.MAX_LEN - pe.CAP_SLACK


# ---- without a GPU ----

def test_fixture_labels_sets_and_cap(fx):
    assert os.path.getsize(PATH) <= pe.MAX_BYTES
    assert tuple(fx.param_names) == pe.PARAM_NAMES
    for name, (p, sub) in pe.PARAM_SETS.items():
        assert fx.params[name] == p and fx.param_sub[name] == sub == poa.subtype(poa.params(*p)), name
        assert poa_ref.subtype(p)[0] == sub, name
    assert sorted(pe.PARAM_SETS[k][1] for k in pe.ODD_SETS) == [poa.LINEAR] * 5 + [poa.AFFINE] * 5 + [poa.CONVEX] * 6
    # the labels, as stored and counted again
    pe.check_labels(fx.label_counts)
    assert pe.count_labels(fx.items) == fx.label_counts
    assert all(it["n_pairs"] > 0 and (it["pairs"] is None or len(it["pairs"]) == it["n_pairs"]) for it in fx.items)
    split = [it for it in fx.items if it["group"] == "split"]
    assert len(split) == len(pe.SPLIT_SETS) * len(pe.SPLIT_LENGTHS) * len(pe.KINDS)
    assert {(it["ps"], len(it["seq"]), it["kind"]) for it in split} == \
        {(ps, L, kind) for ps in pe.SPLIT_SETS for L in pe.SPLIT_LENGTHS for kind in pe.KINDS}
    assert sorted((len(it["seq"]), it["ps"]) for it in fx.items if it["group"] == "square") == sorted(pe.SQUARE)
    for it in fx.items:
        if it["group"] == "square":  # the graph is as long as the sequence
            assert it["view"].n >= len(it["seq"])
    # the stored items are the recipes' own
    for it, (ps, L, kind, _, seq) in zip(split, pe.split_items()):
        assert (it["ps"], it["kind"], it["seq"]) == (ps, kind, seq)
        assert it["view"].n * L <= int(fx.z["ref_cells"][0])
    windows = pe.odd_windows()
    assert [(w["ps"], w["reads"]) for w in fx.windows] == [(ps, reads) for ps in pe.ODD_SETS for reads in windows]
    for ps in pe.ODD_SETS:
        assert sum(it["ps"] == ps for it in fx.items) == sum(len(w) - 1 for w in windows)
    # the cap: the insertion is one gap, so its origin lies up to L - 64 columns to the left of the cells it wins
    for it in split:
        if it["kind"] == "disjoint" and pe.PARAM_SETS[it["ps"]][1] != poa.LINEAR:
            L = len(it["seq"])
            assert it["pairs"] is not None and pe.longest_inserted_run(it["pairs"]) >= L - pe.CAP_SLACK, (it["ps"], L)


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_align_equals_fixture(fx, host, threads):
    host.setenv("GB_POA_THREADS", threads)
    pe.check_items(fx, None, "host")
    assert poa.plan() == (0, 0)


@pytest.mark.parametrize("threads", ["1", "5"])
def test_host_consensus_equals_fixture(fx, host, threads):
    host.setenv("GB_POA_THREADS", threads)
    pe.check_windows(fx, "host")


def test_host_length_limit_item(fx, host):
    check_limit(fx, align_limit(fx)[1])


def test_restatement_equals_fixture_on_a_thinned_subset(fx):
    """Every odd-scoring item of at most 12 000 cells whose index is a multiple of 3, the six split items of 511
    bases (pairs and score), and every fourth odd-scoring window (consensus, node count, alignments, cells)."""
    ran = 0
    for k, it in enumerate(fx.items):
        if (it["group"] == "odd" and k % 3 == 0 and fx.cells(k) <= 12_000) or (it["group"] == "split" and len(it["seq"]) == 511):
            v = poa_ref.View(it["view"].base, it["view"].id, it["view"].out, it["view"].in_end, it["view"].pred)
            pairs, score = poa_ref.align(fx.params[it["ps"]], v, it["seq"])
            assert pairs == [(int(a), int(b)) for a, b in it["pairs"]] and score == it["score"], k
            ran += 1
    assert ran >= 40
    ran = 0
    for w, win in enumerate(fx.windows):
        if w % 4 == 0:
            got = poa_ref.window(fx.params[win["ps"]], win["reads"])
            assert got[:4] == (win["cons"], win["nodes"], win["done"], win["cells"]), w
            ran += 1
    assert ran >= 12


def test_live_cross_check_of_fresh_windows(host):
    """One fresh seeded window per odd parameter set through the reference's spoa, compiled as the recorder
    compiles it."""
    sys.path.insert(0, GOLDEN)
    import make_poa_golden as mk
    if not os.path.isdir(mk.spoa_dir()) or not shutil.which("g++"):
        pytest.skip("no reference tree or no compiler")
    live = mk.LivePoa()
    try:
        rng = np.random.default_rng(78)
        for name in pe.ODD_SETS:
            pr = pe.PARAM_SETS[name][0]
            reads = gen.poa_windows(rng, 1, reads=(3, 8), length=(20, 160), err=0.15, long_indel=0.01, clip=0.3)[0]
            cons, nodes, done = poa.consensus(poa.params(*pr), [reads])
            views, seqs, want = [], [], []
            exp = live.window(pr, reads,
                              on_alignment=lambda k, v, r, p: (views.append(poa.View(*v)), seqs.append(r), want.append(p.copy())))
            assert (cons[0], nodes[0], done) == (exp[0], exp[1], exp[2]), name
            _, pairs, off = poa.align(poa.params(*pr), views, seqs)
            for i in range(len(views)):
                assert (pairs[off[i]:off[i + 1]] == want[i]).all(), (name, i)
    finally:
        live.close()


# ---- on the GPU ----

@pytest.mark.gpu
def test_device_split_and_square_equal_fixture(fx, device):
    pe.check_items(fx, fx.group("split", "square"), "device")
    chunks, ws = poa.plan()
    assert chunks == 1 and ws > 0


@pytest.mark.gpu
def test_device_split_and_square_shuffled(fx, device):
    ks = fx.group("split", "square")
    order = np.random.default_rng(4).permutation(len(ks))
    pe.check_items(fx, [ks[int(k)] for k in order], "shuffled")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [poa.CLASS_WAVE, poa.CLASS_GROUP, poa.CLASS_LONG], ids=["wave", "group", "long"])
def test_device_each_size_class_alone(fx, device, cls):
    """The items of one class only, per parameter set: no launch of another class runs beside them. The long class
    (more than four columns a thread, read back from memory) is held to the reference here."""
    ks = [k for k, it in enumerate(fx.items) if poa.size_class(len(it["seq"])) == cls]
    lens = {len(fx.items[k]["seq"]) for k in ks}
    if cls == poa.CLASS_WAVE:
        assert len(ks) >= 100 and all(fx.items[k]["group"] == "odd" for k in ks)
    elif cls == poa.CLASS_GROUP:
        assert lens >= GROUP_LENGTHS and any(fx.items[k]["group"] == "odd" for k in ks)
    else:
        assert lens == LONG_LENGTHS
        assert {fx.param_sub[fx.items[k]["ps"]] for k in ks if len(fx.items[k]["seq"]) == 1281} == {0, 1, 2}
    pe.check_items(fx, ks, "class")


@pytest.mark.gpu
def test_device_odd_scoring_equals_fixture(fx, device):
    ks = fx.group("odd")
    assert {fx.items[k]["ps"] for k in ks} == set(pe.ODD_SETS)
    pe.check_items(fx, ks, "device")


@pytest.mark.gpu
def test_device_odd_scoring_consensus(fx, device):
    pe.check_windows(fx, "device")


@pytest.mark.gpu
def test_device_length_limit(fx, device):
    """GB_POA_MAX_LEN bases, 256 columns a thread: the one-node case of test_poa.py's host test with its analytic
    score, and the length-limit item, by the checksum of the reference's pairs and the host path's score."""
    p = poa.params(*poa.BENCH)
    one = poa.View([65], [0], [0], [0], [])
    scores, pairs, off = poa.align(p, [one], [np.full(poa.MAX_LEN, 65, np.uint8)])
    assert len(pairs) == poa.MAX_LEN and (pairs[:, 1] == np.arange(poa.MAX_LEN)).all()
    assert (pairs[:, 0] >= 0).sum() == 1 and scores[0] == 2 - 25 - (poa.MAX_LEN - 2)
    score, pairs = align_limit(fx)
    assert poa.plan()[0] == 1
    check_limit(fx, pairs)
    device.setenv("GB_POA_HOST", "1")
    host_score, host_pairs = align_limit(fx)
    assert score == host_score and (pairs == host_pairs).all()
