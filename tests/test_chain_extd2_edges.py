"""gb_chain_extd2 against tests/golden/chain_extd2_edges_golden.npz (tests/chain_extd2_edges.py,
tests/golden/make_chain_extd2_edges_golden.py): the reference's ksw_extd2_sse on items at every edge of the fill
kernel's layout. Rows of 240 | 241 cells (4 or 16 bytes a lane), 1008 | 1009 | 1010 (class 1 | 2, then the first
row swept in two pieces) and 2033 | 2034 (three pieces); states of exactly 65536 bytes (the largest LDS launch)
and 65552 (the workspace); two and three pieces with the state in the workspace; the 8, 16 and 32 KiB launch
buckets; all of them under the flags that change the sweep or the walk, with a z-drop, a band exit and wildcards
in multi-piece rows.

Without a GPU the host path (GB_CHAIN_EXTD2_HOST=1) is held to the fixture. On the GPU the device is, bit for bit:
whole, shuffled, class by class, with every launch group in one call and in many chunks; the walk's and the
pack's indexing is held to the host path at item counts around their block and grid edges; and the timing call's
cell count is held to the restated rows.
"""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import chain_extd2_edges as ee
import chain_extd2_ref as ref
from conftest import GOLDEN
from genomicsbench_palisade_amd import chain, gen

PATH = os.path.join(GOLDEN, "chain_extd2_edges_golden.npz")


@pytest.fixture(scope="module")
def fx():
    return ee.Fixture(PATH)


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_CHAIN_EXTD2_HOST", "1")
    monkeypatch.delenv("GB_CHAIN_THREADS", raising=False)
    monkeypatch.delenv("GB_CHAIN_EXTD2_WS", raising=False)
    return monkeypatch


@pytest.fixture
def device(monkeypatch):
    monkeypatch.delenv("GB_CHAIN_EXTD2_HOST", raising=False)
    monkeypatch.delenv("GB_CHAIN_EXTD2_WS", raising=False)
    return monkeypatch


def same_bytes(a, b):
    return all(p.dtype == q.dtype and p.shape == q.shape and (p.view(np.uint8) == q.view(np.uint8)).all() for p, q in zip(a, b))


# ---- without a GPU ----

def test_fixture_has_every_label_and_its_items_are_the_recipes_own(fx):
    assert fx.size <= ee.MAX_BYTES
    assert tuple(fx.label_counts) == ee.LABELS
    ee.check_labels(fx.label_counts)
    assert ee.count_labels(fx.x, fx.res, fx.rows_swept) == fx.label_counts
    x = ee.build_items()
    assert same_bytes((x.params, x.seqs, x.items), (fx.x.params, fx.x.seqs, fx.x.items))
    assert (fx.res[:, 10] == np.diff(fx.off)).all() and (fx.res[:, 11] == 0).all()
    it = fx.x.items
    # the items of a pair share its bases
    assert len(set(zip(it["q_off"].tolist(), it["t_off"].tolist()))) == len(ee._pairs()) < fx.n
    assert len(fx.x.seqs) == sum(q + t for q, t, _, _ in ee._pairs())
    # the restated arithmetic at the edges it names
    assert [ee.worst_span(m) for m in (240, 241, 1008, 1009, 1010, 2033, 2034)] == [256, 256, 1024, 1024, 1040, 2048, 2064]
    assert ee.state_bytes(240, 5440) == 65536 and ee.state_bytes(241, 5440) == 65552
    assert (fx.cls == 2).sum() and ((fx.cls == 2) & (fx.pieces >= 2)).sum() >= 2 and ((fx.cls == 3) & (fx.pieces >= 2)).sum() >= 2
    assert fx.pieces.max() == 3 and ((fx.cls == 3) & (fx.pieces == 3)).any() and ((fx.cls == 2) & (fx.pieces == 3)).any()
    # a row of the kernel's lanes: class 0 never passes 64 lanes of 4 bytes
    assert (fx.pieces[fx.cls == 0] == 1).all() and (fx.pieces[fx.cls == 1] == 1).all()


def test_at_most_a_quarter_of_the_unstopped_items_end_without_a_cigar(fx):
    none, of = ee.cigarless(fx.x, fx.res)
    assert of >= 100 and 4 * none <= of, (none, of)


def test_a_class_2_item_cannot_fall_into_the_8k_bucket():
    """Class 2 needs more than 1008 cells a row, so both lengths above 1008 and a state of at least 13 328 bytes:
    of the 13 launch groups the kernel numbers, the one of class 2 and up to 8 KiB stays empty."""
    assert ee.n_col(1008, 1008, -1) == 64 and ee.n_col(1009, 1009, -1) == 65
    assert ee.state_bytes(1009, 1009) == 13328 > 8192
    assert ee.launch_group(1009, 1009, -1) == 7 and ee.launch_group(30, 30, -1) == 12


@pytest.mark.parametrize("threads", [1, 5])
def test_host_path_equals_fixture(fx, host, threads):
    host.setenv("GB_CHAIN_THREADS", str(threads))
    fx.check(chain.extd2)


def test_restatement_equals_fixture_on_bucket_edge_items(fx):
    """Two of the items on which the recorder held the restatement to the live reference: one that leaves the band,
    one swept to its last row."""
    it = fx.x.items
    rows = it["qlen"] + it["tlen"] - 1
    pick = [np.flatnonzero((rows <= ee.RESTATED_ROWS) & (it["tlen"] == 672) & (it["w"] == w))[0] for w in (50, -1)]
    assert fx.res[pick[0]][1] == 1 and fx.res[pick[1]][1] == 0
    for i in pick:
        rec, cig = ref.align_item(fx.x, int(i))
        assert list(rec) == fx.res[i].tolist() and cig.tolist() == fx.words(i).tolist(), it[i]


def test_host_path_equals_the_live_reference_on_fresh_edge_items(host):
    """The edge shapes over fresh bases, one flag set each, through the reference compiled as the recorder does."""
    sys.path.insert(0, GOLDEN)
    import make_chain_extd2_golden as mk
    if not os.path.exists(os.path.join(mk.REF_TREE, "tools", "minimap2", "ksw2_extd2_sse.c")) or not shutil.which("gcc"):
        pytest.skip("no reference tree or no compiler here")
    rng = np.random.default_rng(515)
    parts = [gen.extd2_items(rng, [(q, t)], w=w, zdrop=400, flag=ee.VARIANT_FLAGS, sub=0.1, indel=0.05, long_indel=0.004)
             for q, t, w in ((600, 640, 239), (241, 700, -1), (1300, 1340, 1008), (1010, 1500, -1), (2034, 2100, -1))]
    x = gen.Extd2Items.concat(parts)
    live = mk.LiveExtd2(mk.REF_TREE)
    try:
        res, cig, off = chain.extd2(x)
        for i in range(x.n):
            assert mk.equal((res[i].tolist(), cig[off[i]:off[i + 1]]), live.align_item(x, i)), x.items[i]
    finally:
        live.close()


# ---- on the device ----

@pytest.mark.gpu
def test_device_equals_fixture_bit_for_bit(fx, device):
    fx.check(chain.extd2)
    assert chain.extd2_plan()[0] == 1


@pytest.mark.gpu
def test_device_equals_fixture_with_its_items_shuffled(fx, device):
    fx.check(chain.extd2, np.random.default_rng(12).permutation(fx.n))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", range(4))
def test_device_equals_fixture_on_each_size_class_alone(fx, device, cls):
    """No launch of another class runs beside them. Class 3 is the sweep in two and three pieces over a state in the
    workspace."""
    sel = np.flatnonzero(fx.cls == cls)
    assert len(sel) >= 12
    if cls >= 2:
        assert (fx.pieces[sel] >= 2).sum() >= 2 and (fx.pieces[sel] == 3).any()
    fx.check(chain.extd2, sel)


@pytest.mark.gpu
def test_device_runs_every_launch_group_in_one_call(fx, device):
    """An item of every launch group the arithmetic can reach (12 of the kernel's 13: see
    test_a_class_2_item_cannot_fall_into_the_8k_bucket), so all four streams and the join, the two items of most
    and of fewest rows of each group."""
    assert sorted(set(fx.group.tolist())) == [g for g in range(13) if g != 10]
    rows = fx.x.items["qlen"] + fx.x.items["tlen"]
    sel = []
    for g in sorted(set(fx.group.tolist())):
        of = np.flatnonzero(fx.group == g)
        of = of[np.argsort(rows[of], kind="stable")]
        sel += sorted({int(of[0]), int(of[-1])})
    assert len(set(fx.group[sel].tolist())) == 12
    fx.check(chain.extd2, sel)
    assert chain.extd2_plan()[0] == 1


@pytest.mark.gpu
def test_device_equals_fixture_in_many_chunks(fx, device):
    """A workspace budget of exactly the largest item's need."""
    it = fx.x.items
    codes = np.array([(int(q) + int(t) - 1) * ee.n_col(int(q), int(t), int(w)) * 16 for q, t, w in zip(it["qlen"], it["tlen"], it["w"])])
    big = int(np.argmax(codes + np.where(fx.cls == 3, [ee.state_bytes(int(q), int(t)) for q, t in zip(it["qlen"], it["tlen"])], 0)))
    assert (it["qlen"][big], it["tlen"][big], it["w"][big]) == (2100, 5300, -1)
    fx.check(chain.extd2, [big])
    chunks, need = chain.extd2_plan()
    assert chunks == 1 and need == 7399 * 133 * 16 + ee.state_bytes(2100, 5300) + 2 * 7400 * 4
    device.setenv("GB_CHAIN_EXTD2_WS", str(need))
    fx.check(chain.extd2)
    chunks, most = chain.extd2_plan()
    assert chunks >= 3 and most <= need


def _compute_units():
    """The device's compute units, by the attribute that the pack's launch reads, from the HIP runtime that the
    library has loaded. torch.cuda.get_device_properties(0).multi_processor_count is the same number, but torch
    brings a HIP runtime of its own, which finds no device in a process where the library's already holds it."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    for path in paths:
        n = ctypes.c_int(0)
        if ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0:  # hipDeviceAttributeMultiprocessorCount
            return n.value
    raise AssertionError(f"no HIP runtime among {paths} tells the compute units of device 0")


def _batch(seed, n):
    rng = np.random.default_rng(seed)
    return gen.extd2_items(rng, [(int(q), int(t)) for q, t in rng.integers(8, 41, (n, 2))])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, "32 * CUs + 70"])
def test_device_equals_host_path_at_batch_edges(device, n):
    """The walk's block of 64 items, the pack's four waves a block and, in the large call, its grid stride (the
    grid stops at 8 * CUs blocks of four items): small items, which the fixtures pin to the reference, at item
    counts around those edges. The kernels see the items that reach the sweep, so the large call holds
    32 * CUs + 70 of those and, as every third item of the call, one with an empty side between them: items that
    return early lie between live ones and take their cigar_off from the next."""
    large = isinstance(n, str)
    if large:
        cus = _compute_units()
        assert 16 <= cus <= 4096
        live = 32 * cus + 70
        n = live + live // 2
    x = _batch(1000 + n, n)
    if large:
        x.items["qlen"][2::6] = 0
        x.items["tlen"][5::6] = 0
        assert ((x.items["qlen"] > 0) & (x.items["tlen"] > 0)).sum() == live
    d = chain.extd2(x)
    if large:
        assert chain.extd2_plan()[0] == 1  # one chunk: the pack's grid strides over all of them
    device.setenv("GB_CHAIN_EXTD2_HOST", "1")
    h = chain.extd2(x)
    assert len(h[0]) == n and len(h[2]) == n + 1 and h[2][-1] == len(h[1]) >= n // 2
    bad = np.flatnonzero((d[0].view(np.int32).reshape(-1, 12) != h[0].view(np.int32).reshape(-1, 12)).any(1))
    assert not len(bad), (len(bad), bad[:8], x.items[bad[0]], d[0][bad[0]], h[0][bad[0]])
    assert same_bytes(d, h)


@pytest.mark.gpu
def test_timing_counts_the_cells_of_the_rows_reached(fx, device):
    """The in-band cells of the restated rows, up to the row the fixture stores for an item that stopped early."""
    want = ee.cells_reached(fx.x, fx.res, fx.rows_swept)
    fx.check(chain.extd2)
    assert chain.extd2_timing()[2] == int(want.sum())
    stopped = np.flatnonzero(fx.res[:, 1] == 1)
    assert len(stopped) >= 20
    fx.check(chain.extd2, stopped)
    assert chain.extd2_timing()[2] == int(want[stopped].sum())
