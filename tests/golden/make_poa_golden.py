"""Records tests/golden/poa_golden.npz: windows and alignment items for gb_poa_consensus and gb_poa_align with what
the reference's spoa returns for them.

Two pins.
1. spoa's own expected results: the reads and qualities of test/data/sample.fastq (one window of 55 reads) and the
   six consensus strings that test/spoa_test.cpp expects for kNW (Global*Consensus*), read out of that file here.
2. The live reference: tools/racon/vendor/spoa/src/{alignment_engine,graph,sisd_alignment_engine,
   simd_alignment_engine}.cpp of the reference tree, compiled unmodified, without -msse4.1 and without -mavx2 (so
   createAlignmentEngine returns the SISD engine), together with poa_live_shim.cpp, into a temporary directory
   outside the repository, and called through ctypes. graph.cpp prints two lines per add_alignment to stdout; the
   recorder sends its own stdout to the null device while the library runs.
The live build must reproduce the six strings of pin 1.

tests/poa_ref.py restates the contract and must equal the live path: its graph (driven by the live pairs) in every
view, consensus, node count and rank order on every window, and its alignment on every stored item and on every
other alignment of at most REF_CELLS cells. It counts the labels (poa_ref.MINIMA), asserted here and again by
tests/test_poa.py on the stored counts.

Stored: per window its group, parameter set, reads, qualities (if weighted), consensus, node count, alignments
done, cells and the checksum of rank_to_node_id; per alignment item (all of the small windows, a few rounds of the
large ones) its window and round, graph view, pairs and score. The reference does not return the score and its
walk's path need not be priced at it (the convex extend-up loop may follow an O chain where the optimum came
through F), so an item's score is the restatement's final H value, of the run whose pairs equal the live ones.

Usage: python tests/golden/make_poa_golden.py [reference root]
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import poa_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402
from make_abea_golden import REF_TREE  # noqa: E402

OUT = os.path.join(HERE, "poa_golden.npz")
MAX_BYTES = 400 * 1024
REF_CELLS = 120_000  # the restatement's alignment runs on items of at most this many cells
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 860)
BENCH = (2, -4, -6, -2, -25, -1)
PARAM_SETS = {"bench": BENCH, "spoa-linear": (5, -4, -8, -8, -8, -8), "spoa-affine": (5, -4, -8, -6, -8, -6),
              "spoa-convex": (5, -4, -8, -6, -10, -2), "racon-linear": (3, -5, -4, -4, -4, -4)}
SPOA_TESTS = (("GlobalConsensus", "spoa-linear", False), ("GlobalAffineConsensus", "spoa-affine", False),
              ("GlobalConvexConsensus", "spoa-convex", False), ("GlobalConsensusWithQualities", "spoa-linear", True),
              ("GlobalAffineConsensusWithQualities", "spoa-affine", True),
              ("GlobalConvexConsensusWithQualities", "spoa-convex", True))
SPOA_SRCS = ("alignment_engine.cpp", "graph.cpp", "sisd_alignment_engine.cpp", "simd_alignment_engine.cpp")


def spoa_dir(ref_root=REF_TREE):
    return os.path.join(ref_root, "tools", "racon", "vendor", "spoa")


class quiet_stdout:
    """The process's stdout at the null device for a while (the reference's graph.cpp prints from add_alignment)."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, 1)
        os.close(null)

    def __exit__(self, *a):
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)


class LivePoa:
    """The reference's spoa (SISD engine) and poa_live_shim.cpp compiled in a temporary directory."""

    def __init__(self, ref_root=REF_TREE):
        d = spoa_dir(ref_root)
        srcs = [os.path.join(d, "src", s) for s in SPOA_SRCS]
        for s in srcs:
            if not os.path.exists(s):
                raise FileNotFoundError(s)
        self.dir = tempfile.mkdtemp(prefix="gb_poa_live_")
        so = os.path.join(self.dir, "libpoa_live.so")
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-fPIC", "-shared", "-w", "-I", os.path.join(d, "include"),
                               "-I", os.path.join(d, "src")] + srcs + [os.path.join(HERE, "poa_live_shim.cpp"), "-o", so])
        L = self.lib = ctypes.CDLL(so)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.poa_live_engine.restype = vp
        L.poa_live_engine.argtypes = [ci] * 7 + [vp, ci]
        L.poa_live_engine_free.argtypes = [vp]
        L.poa_live_graph.restype = vp
        L.poa_live_graph_free.argtypes = [vp]
        L.poa_live_align.argtypes = [vp, vp, vp, ci, vp, ci]
        L.poa_live_add.argtypes = [vp, vp, ci, vp, ci, vp]
        L.poa_live_add_quality.argtypes = [vp, vp, ci, vp, ci, vp]
        L.poa_live_consensus.argtypes = [vp, vp, ci]
        L.poa_live_nodes.argtypes = [vp]
        L.poa_live_edges.argtypes = [vp]
        L.poa_live_view.argtypes = [vp] * 6

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def engine(self, p, type=1):
        err = ctypes.create_string_buffer(256)
        e = self.lib.poa_live_engine(type, *[int(x) for x in p], err, 256)
        if not e:
            raise ValueError(err.value.decode())
        return e

    def view(self, g):
        n, ne = self.lib.poa_live_nodes(g), self.lib.poa_live_edges(g)
        base, ids, out = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        in_end, pred = np.zeros(n, np.int32), np.zeros(ne, np.int32)
        self.lib.poa_live_view(g, base.ctypes.data, ids.ctypes.data, out.ctypes.data, in_end.ctypes.data, pred.ctypes.data)
        return base, ids, out, in_end, pred

    def window(self, p, reads, quals=None, weights=None, on_alignment=None):
        """(consensus, node count, alignments done, cells, rank_to_node_id) of one window. quals goes through
        add_alignment's quality form, weights through its vector form. on_alignment(round, view arrays, read,
        pairs) is called for every alignment done, before the read is added."""
        L = self.lib
        with quiet_stdout():
            e, g = self.engine(p), L.poa_live_graph()
            done = cells = 0
            for k, r in enumerate(reads):
                r = bytes(r)
                n = L.poa_live_nodes(g)
                pairs = np.zeros(2 * (n + len(r)), np.int32)
                got = L.poa_live_align(e, g, r, len(r), pairs.ctypes.data, n + len(r))
                assert got >= 0
                pairs = pairs[:2 * got]
                if n and len(r):
                    done, cells = done + 1, cells + n * len(r)
                    if on_alignment:
                        on_alignment(k, self.view(g), r, pairs.reshape(-1, 2))
                if quals is not None:
                    L.poa_live_add_quality(g, pairs.ctypes.data, got, r, len(r), bytes(quals[k]))
                elif weights is not None:
                    w = np.ascontiguousarray(weights[k], np.uint32)
                    L.poa_live_add(g, pairs.ctypes.data, got, r, len(r), w.ctypes.data if len(w) else None)
                else:
                    L.poa_live_add(g, pairs.ctypes.data, got, r, len(r), None)
            n = L.poa_live_nodes(g)
            buf = ctypes.create_string_buffer(max(n, 1))
            m = L.poa_live_consensus(g, buf, n) if n else 0
            assert m >= 0
            order = self.view(g)[1] if n else np.zeros(0, np.int32)
            L.poa_live_graph_free(g)
            L.poa_live_engine_free(e)
        return buf.raw[:m], n, done, cells, order


def read_sample(ref_root=REF_TREE):
    """(reads, quals, {test name: expected consensus}) of spoa's own test."""
    d = os.path.join(spoa_dir(ref_root), "test")
    lines = open(os.path.join(d, "data", "sample.fastq"), "rb").read().split(b"\n")
    reads, quals = [], []
    k = 0
    while k + 3 < len(lines) and lines[k].startswith(b"@"):
        reads.append(lines[k + 1]), quals.append(lines[k + 3])
        k += 4
    src = open(os.path.join(d, "spoa_test.cpp")).read()
    expected = {}
    for name, _, _ in SPOA_TESTS:
        body = src[src.index("TEST_F(SpoaAlignmentTest, %s)" % name):]
        body = body[body.index("valid_result ="):body.index(";", body.index("valid_result ="))]
        expected[name] = "".join(re.findall(r'"([A-Z]*)"', body)).encode()
    return reads, quals, expected


def exact_read(rng, template, sub=0.08):
    """A read of the template's own length: substitutions only."""
    t = np.frombuffer(template, np.uint8).copy()
    al = np.frombuffer(b"ACGT", np.uint8)
    hit = rng.random(len(t)) < sub
    t[hit] = al[rng.integers(0, 4, int(hit.sum()))]
    return t.tobytes()


def make_windows():
    """[(group, parameter set, reads, quals or None, rounds to store or None for all)]"""
    rng = np.random.default_rng(20261021)
    W = []
    # every listed length at every subtype: three reads, the second and third of exactly that length
    for group in ("bench", "spoa-linear", "spoa-affine", "spoa-convex"):
        for L in LENGTHS:
            t = gen.poa_template(rng, L)
            reads = [gen.poa_read(rng, t, 0.04, 0.04, 0.04) or t, exact_read(rng, t), exact_read(rng, t)]
            W.append((group, group, reads, None, None if L < 300 else (1,)))
    # the benchmark's parameters over shapes
    for n_reads, L in ((1, 40), (2, 50), (3, 45), (8, 70), (8, 33)):
        W.append(("bench", "bench", gen.poa_window(rng, n_reads, L, err=0.15)[0], None, None))
    W.append(("bench", "bench", gen.poa_window(rng, 30, 90, err=0.15)[0], None, (1, 15, 29)))
    W.append(("bench", "bench", gen.poa_window(rng, 110, 24, err=0.3)[0], None, (109,)))  # in-degree
    # long indels (the second gap piece wins from 21 bases), also on the graph side
    for k in range(6):
        W.append(("bench", "bench", gen.poa_window(rng, 6, 150, err=0.06, long_indel=0.008)[0], None, None))
    t = gen.poa_template(rng, 160)
    W.append(("bench", "bench", [t, t[:60] + t[95:], t[:60] + gen.poa_template(rng, 30) + t[60:], t, t[:20] + t[50:]], None, None))
    W.append(("spoa-convex", "spoa-convex", gen.poa_window(rng, 6, 150, err=0.06, long_indel=0.008)[0], None, None))
    # the heaviest node is no sink: most reads end early, and the one that goes on meets a heavier side branch
    t, junk = gen.poa_template(rng, 100), gen.poa_template(rng, 12)
    W.append(("bench", "bench", [t[:80]] * 6 + [t] + [junk + t[80:]] * 2, None, None))
    W.append(("spoa-affine", "spoa-affine", [t[:80]] * 6 + [t] + [junk + t[80:]] * 2, None, None))
    # reads much shorter and much longer than the graph
    t = gen.poa_template(rng, 120)
    W.append(("bench", "bench", [t, t[40:52], t[:5], gen.poa_read(rng, t + gen.poa_template(rng, 150)), t[100:]], None, None))
    # reads that begin before or end after the graph: new sources and sinks, more than one sink
    t = gen.poa_template(rng, 100)
    W.append(("bench", "bench", [t[20:80], t[:70], t[30:], gen.poa_template(rng, 12) + t[20:80] + gen.poa_template(rng, 9),
                                 t[25:75] + gen.poa_template(rng, 14), t], None, None))
    for group in ("bench", "spoa-affine", "racon-linear"):
        W.append((group, group, gen.poa_window(rng, 8, 80, err=0.12, clip=0.7)[0], None, None))
    # ties: homopolymer and short-period templates
    for group in ("bench", "spoa-linear", "spoa-affine", "racon-linear"):
        for kind in ("homopolymer", "period"):
            W.append((group, group, gen.poa_window(rng, 6, 60, err=0.2, kind=kind)[0], None, None))
    # bytes outside ACGT, an empty read inside a window
    W.append(("bench", "bench", gen.poa_window(rng, 6, 50, err=0.15, alphabet=b"ACGTNacgtn")[0], None, None))
    r = gen.poa_window(rng, 5, 40, err=0.15)[0]
    W.append(("bench", "bench", [r[0], b"", r[1], r[2], b"", r[3]], None, None))
    W.append(("bench", "bench", [b"", r[0], r[4]], None, None))
    # a racon-like linear set
    for n_reads, L in ((4, 60), (8, 100), (12, 40)):
        W.append(("racon-linear", "racon-linear", gen.poa_window(rng, n_reads, L, err=0.15)[0], None, None))
    # weights
    for ps in ("bench", "spoa-linear", "spoa-affine", "spoa-convex"):
        reads, quals = gen.poa_window(rng, 8, 60, err=0.2, quals=True)
        W.append(("weights", ps, reads, quals, None))
    reads, quals = gen.poa_window(rng, 10, 30, err=0.3, kind="period", quals=True)
    W.append(("weights", "bench", reads, [bytes([33 + (x % 3) for x in q]) for q in quals], None))
    # the size of the benchmark's own windows, thinned to one stored round
    W.append(("bench", "bench", gen.poa_window(rng, 30, 857, err=0.12)[0], None, (29,)))
    return W


def cat(parts, dt):
    return np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts]).astype(dt) if parts else np.zeros(0, dt)


def offs(parts):
    return np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)


def record(ref_root=REF_TREE):
    live = LivePoa(ref_root)
    try:
        names = list(PARAM_SETS)
        reads, quals, expected = read_sample(ref_root)
        assert len(reads) == 55 and min(map(len, reads)) == 149 and max(map(len, reads)) == 515
        for name, ps, use_q in SPOA_TESTS:
            got = live.window(PARAM_SETS[ps], reads, quals if use_q else None)[0]
            assert got == expected[name], (name, got, expected[name])
        counts = ref.new_counts()
        win, items = [], []
        for wi, (group, ps, wreads, wquals, rounds) in enumerate(make_windows()):
            p = PARAM_SETS[ps]
            weights = None if wquals is None else [(np.frombuffer(q, np.uint8).astype(np.int64) - 33).astype(np.uint32)
                                                  for q in wquals]
            G = ref.Graph()
            state = {"next": 0}

            def catch_up(upto, pending):  # the restatement's graph takes the reads before round `upto`
                while state["next"] < upto:
                    k = state["next"]
                    G.add_alignment(pending.pop(k, []), wreads[k], None if weights is None else weights[k], counts)
                    state["next"] += 1

            pending = {}

            def on_alignment(k, view, r, pairs):
                catch_up(k, pending)
                v = G.view()
                for a, b in zip((v.base, v.id, v.out, v.in_end, v.pred), view):
                    assert list(a) == [int(x) for x in b], ("view", wi, k)
                stored = rounds is None or k in rounds
                if stored or v.n * len(r) <= REF_CELLS:
                    rp, score = ref.align(p, v, r, counts)
                    assert rp == [(int(a), int(b)) for a, b in pairs], ("pairs", wi, k)
                pending[k] = [(int(a), int(b)) for a, b in pairs]
                if stored:
                    items.append((wi, k, view, np.frombuffer(r, np.uint8), pairs.copy(), score))

            # the quality form and the vector form of add_alignment are the same arithmetic; use the first
            cons, n_nodes, done, cells, order = live.window(p, wreads, quals=wquals, on_alignment=on_alignment)
            catch_up(len(wreads), pending)
            assert G.consensus(counts) == cons and len(G.base) == n_nodes, ("consensus", wi)
            assert list(G.rank_to_node) == [int(x) for x in order], ("rank order", wi)
            win.append((group, names.index(ps), wreads, wquals, cons, n_nodes, done, cells, ref.rank_checksum(order)))
        for k, v in ref.MINIMA.items():
            assert counts[k] >= v, (k, counts[k], counts)
        all_reads = [r for w in win for r in w[2]]
        all_quals = [q for w in win if w[3] is not None for q in w[3]]
        data = dict(
            param_names=np.array(names), params=np.array([PARAM_SETS[k] for k in names], np.int8),
            sample_reads=cat([np.frombuffer(r, np.uint8) for r in reads], np.uint8), sample_read_off=offs(reads),
            sample_quals=cat([np.frombuffer(q, np.uint8) for q in quals], np.uint8),
            sample_tests=np.array([t[0] for t in SPOA_TESTS]), sample_params=np.array([names.index(t[1]) for t in SPOA_TESTS], np.int32),
            sample_weighted=np.array([t[2] for t in SPOA_TESTS], np.uint8),
            sample_expected=cat([np.frombuffer(expected[t[0]], np.uint8) for t in SPOA_TESTS], np.uint8),
            sample_expected_off=offs([expected[t[0]] for t in SPOA_TESTS]),
            win_group=np.array([w[0] for w in win]), win_params=np.array([w[1] for w in win], np.int32),
            win_weighted=np.array([w[3] is not None for w in win], np.uint8),
            win_read_off=offs([w[2] for w in win]), read_off=offs(all_reads),
            read_bytes=cat([np.frombuffer(r, np.uint8) for r in all_reads], np.uint8),
            qual_bytes=cat([np.frombuffer(q, np.uint8) for q in all_quals], np.uint8),
            win_cons=cat([np.frombuffer(w[4], np.uint8) for w in win], np.uint8), win_cons_off=offs([w[4] for w in win]),
            win_nodes=np.array([w[5] for w in win], np.int32), win_done=np.array([w[6] for w in win], np.int64),
            win_cells=np.array([w[7] for w in win], np.int64), win_rank_sum=np.array([w[8] for w in win], np.int64),
            item_win=np.array([it[0] for it in items], np.int32), item_round=np.array([it[1] for it in items], np.int32),
            item_node_off=offs([it[2][0] for it in items]), item_edge_off=offs([it[2][4] for it in items]),
            node_base=cat([it[2][0] for it in items], np.uint8), node_id=cat([it[2][1] for it in items], np.int32),
            node_out=cat([it[2][2] for it in items], np.uint8), in_end=cat([it[2][3] for it in items], np.int32),
            pred_rank=cat([it[2][4] for it in items], np.int32),
            item_seq_off=offs([it[3] for it in items]), item_seq=cat([it[3] for it in items], np.uint8),
            item_pair_off=offs([it[4] for it in items]), item_pairs=cat([it[4] for it in items], np.int32).reshape(-1, 2),
            item_score=np.array([it[5] for it in items], np.int32),
            label_names=np.array(list(ref.LABELS)), label_counts=np.array([counts[k] for k in ref.LABELS], np.int64),
            ref_cells=np.array([REF_CELLS], np.int64))
        return data
    finally:
        live.close()


def main():
    data = record(sys.argv[1] if len(sys.argv) > 1 else REF_TREE)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes, {len(data['win_group'])} windows, {len(data['item_win'])} alignment items")
    print(dict(zip(data["label_names"].tolist(), data["label_counts"].tolist())))
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
