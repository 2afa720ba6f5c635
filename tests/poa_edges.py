"""The items of tests/golden/poa_edges_golden.npz: how they are made, which labels they must show, how they are
stored and loaded. Shared by tests/golden/make_poa_edges_golden.py and tests/test_poa_edges.py.

Four groups, each aimed at a place where poa_fill_kernel<NT, REG> differs from the reference's left-to-right row:
- split: a graph of about 50 nodes and a sequence of exactly L bases with an insertion of L - 48 bases in its
  middle, at every L around a change of the columns a thread owns (cpt = ceil(L / 256)) and of the size class. The
  gap that wins the cells right of the insertion opens hundreds of columns, so several waves, to their left: its
  value reaches them only through the waves' totals in LDS.
- square: round 2 of a three-read window whose reads are as long as the graph, at 513, 1024 and 1025 bases.
- odd: sixteen parameter sets at the boundaries of spoa's subtype rule, with free extension, free gaps, m <= 0,
  n >= m, all-zero and the int8 extremes, each on the same three small windows.
- limit: a split item of GB_POA_MAX_LEN bases, regenerated from its seed and stored as a checksum of its pairs."""
import os

import numpy as np

from genomicsbench_palisade_amd import gen, poa

SEED = 20261022
MAX_BYTES = 400 * 1024
SUBTYPE_NAMES = ("linear", "affine", "convex")
SPLIT_SETS = ("bench", "spoa-affine", "spoa-linear")
SPLIT_LENGTHS = (511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281)
KINDS = ("disjoint", "random")
SQUARE = ((513, "spoa-affine"), (1024, "bench"), (1025, "spoa-linear"))
TEMPLATE, CUT = 48, 24
CAP_SLACK = 64  # a disjoint item's longest inserted run is at least L - CAP_SLACK under the affine and convex sets

# name -> ((m, n, g, e, q, c), the subtype spoa's rule gives it)
PARAM_SETS = {
    "bench": ((2, -4, -6, -2, -25, -1), poa.CONVEX),
    "spoa-affine": ((5, -4, -8, -6, -8, -6), poa.AFFINE),
    "spoa-linear": ((5, -4, -8, -8, -8, -8), poa.LINEAR),
    "odd-g-eq-e": ((5, -4, -8, -8, -10, -2), poa.LINEAR),
    "odd-g-gt-e": ((5, -4, -4, -8, -10, -2), poa.LINEAR),
    "odd-free-gaps": ((5, -4, 0, 0, 0, 0), poa.LINEAR),
    "odd-all-zero": ((0, 0, 0, 0, 0, 0), poa.LINEAR),
    "odd-int8-linear": ((127, -128, -128, -128, -128, -128), poa.LINEAR),
    "odd-g-eq-q": ((5, -4, -8, -6, -8, -2), poa.AFFINE),
    "odd-e-eq-c": ((5, -4, -8, -6, -10, -6), poa.AFFINE),
    "odd-e-gt-c": ((5, -4, -8, -2, -10, -6), poa.AFFINE),
    "odd-free-extension": ((5, -4, -8, 0, -8, 0), poa.AFFINE),
    "odd-int8-affine": ((127, -128, -128, -127, -128, -1), poa.AFFINE),
    "odd-tightest-convex": ((5, -4, -8, -6, -9, -5), poa.CONVEX),
    "odd-c-zero": ((5, -4, -4, -2, -20, 0), poa.CONVEX),
    "odd-m-zero": ((0, -4, -8, -6, -10, -2), poa.CONVEX),
    "odd-n-gt-m": ((1, 3, -8, -6, -10, -2), poa.CONVEX),
    "odd-m-negative": ((-2, -5, -8, -6, -10, -2), poa.CONVEX),
    "odd-int8-convex": ((127, -128, -127, -1, -128, 0), poa.CONVEX),
}
PARAM_NAMES = tuple(PARAM_SETS)
ODD_SETS = tuple(k for k in PARAM_NAMES if k.startswith("odd-"))
assert len(ODD_SETS) == 16


def cpt(L):
    """Columns per thread of the workgroup kernels (NT = 256)."""
    return -(-L // 256)


# each label names a case that must be there; the recorder asserts every count against MINIMA, the test the stored ones
LABELS = tuple(f"split/{SUBTYPE_NAMES[PARAM_SETS[ps][1]]}/{L}/{kind}" for ps in SPLIT_SETS for L in SPLIT_LENGTHS
               for kind in KINDS) + \
    ("cpt2_reg", "cpt3_reg", "cpt4_reg", "cpt5_long", "cpt6_long", "square", "items_without_pairs") + \
    tuple(f"{ps}/{SUBTYPE_NAMES[PARAM_SETS[ps][1]]}" for ps in ODD_SETS)
MINIMA = {k: 1 for k in LABELS}
MINIMA["square"] = 3
MINIMA["items_without_pairs"] = 0  # and the maximum: no stored item has zero pairs


def split_reads(kind, L, *key):
    """(the three reads of the graph, the sequence of exactly L bases) of one split item, drawn from SEED and key."""
    rng = np.random.default_rng([SEED, *key])
    al_t, al_i = (b"AC", b"GT") if kind == "disjoint" else (b"ACGT", b"ACGT")
    t = gen.poa_template(rng, TEMPLATE, alphabet=al_t)
    reads = [t, gen.poa_read(rng, t, 0.06, 0.06, 0.06), gen.poa_read(rng, t, 0.06, 0.06, 0.06)]
    seq = t[:CUT] + gen.poa_template(rng, L - TEMPLATE, alphabet=al_i) + t[CUT:]
    assert len(seq) == L
    return reads, seq


def split_items():
    """[(parameter set, L, kind, graph reads, sequence)]. The cap is a condition on the inputs: a graph read's
    inserted G or T can pair with a base of the insertion and cut its run in two. The key's last word names the
    draw; the one before it left spoa-affine / 513 / disjoint with a run of L - 75."""
    out = []
    for si, ps in enumerate(SPLIT_SETS):
        for L in SPLIT_LENGTHS:
            for ki, kind in enumerate(KINDS):
                out.append((ps, L, kind) + split_reads(kind, L, 1, si, L, ki, 0))
    return out


def square_windows():
    """[(parameter set, L, three reads)]: round 2 aligns a read of exactly L bases to the graph of the first two."""
    out = []
    for k, (L, ps) in enumerate(SQUARE):
        rng = np.random.default_rng([SEED, 2, k])
        t = gen.poa_template(rng, L)
        reads = [gen.poa_read(rng, t, 0.04, 0.04, 0.04) for _ in range(3)]
        reads[2] = (reads[2] + gen.poa_template(rng, L))[:L]
        out.append((ps, L, reads))
    return out


def odd_windows():
    """The three windows every odd parameter set runs."""
    rng = np.random.default_rng([SEED, 3])
    w0 = gen.poa_windows(rng, 1, reads=(3, 8), length=(20, 120), err=0.15, long_indel=0.01, clip=0.3)[0]
    w1 = gen.poa_window(rng, 6, 60, err=0.2, kind="homopolymer")[0]
    t = gen.poa_template(rng, 60)
    w2 = [t, t[:30] + gen.poa_template(rng, 300) + t[30:], t, t[:10] + t[40:]]
    assert poa.size_class(len(w2[1])) == poa.CLASS_GROUP
    return [w0, w1, w2]


def limit_reads():
    return split_reads("disjoint", poa.MAX_LEN, 4)


def checksum(a):
    """Sum of (index + 1) * (value + 2) over the flattened array, modulo 2^61 - 1."""
    a = np.asarray(a, np.int64).reshape(-1)
    m = (1 << 61) - 1
    return int((np.arange(1, len(a) + 1, dtype=object) * (a.astype(object) + 2)).sum() % m) if len(a) else 0


def longest_inserted_run(pairs):
    """The longest run of consecutive pairs (-1, position)."""
    best = cur = 0
    for node in np.asarray(pairs)[:, 0]:
        cur = cur + 1 if node == -1 else 0
        best = max(best, cur)
    return best


def count_labels(items):
    """{label: count} of items given as dicts with group, ps (name), kind, seq and n_pairs."""
    c = {k: 0 for k in LABELS}
    for it in items:
        L, sub = len(it["seq"]), SUBTYPE_NAMES[PARAM_SETS[it["ps"]][1]]
        c["items_without_pairs"] += it["n_pairs"] == 0
        if it["group"] == "split":
            c[f"split/{sub}/{L}/{it['kind']}"] += 1
        if it["group"] == "square":
            c["square"] += 1
        if it["group"] == "odd":
            c[f"{it['ps']}/{sub}"] += 1
        if it["group"] in ("split", "square"):
            cls, k = poa.size_class(L), cpt(L)
            if cls == poa.CLASS_GROUP and 2 <= k <= 4:
                c[f"cpt{k}_reg"] += 1
            if cls == poa.CLASS_LONG and 5 <= k <= 6:
                c[f"cpt{k}_long"] += 1
    return c


def check_labels(counts):
    assert set(counts) == set(LABELS), sorted(set(counts) ^ set(LABELS))
    for k, v in MINIMA.items():
        assert counts[k] >= v, (k, counts[k])
    assert counts["items_without_pairs"] == 0


class Fixture:
    """poa_edges_golden.npz. items: dicts with group ("split", "square", "odd"), ps (name), kind, win, round, view,
    seq, score, n_pairs and pairs, or pairs None and pair_sum where the pairs are stored as a checksum. windows: the
    odd sets' (ps, reads, cons, nodes, done, cells). limit: the length-limit item (view, seq, n_pairs, pair_sum)."""

    def __init__(self, path):
        z = self.z = np.load(path)
        self.size = os.path.getsize(path)
        self.param_names = [str(x) for x in z["param_names"]]
        self.params = {n: tuple(int(v) for v in row) for n, row in zip(self.param_names, z["params"])}
        self.param_sub = {n: int(s) for n, s in zip(self.param_names, z["param_sub"])}
        no, eo, so, po = z["item_node_off"], z["item_edge_off"], z["item_seq_off"], z["item_pair_off"]

        def view(n0, n1, e0, e1):
            return poa.View(z["node_base"][n0:n1], z["node_id"][n0:n1], z["node_out"][n0:n1], z["in_end"][n0:n1],
                            z["pred_rank"][e0:e1])

        self.items = []
        for k in range(len(z["item_group"])):
            whole = bool(z["item_whole"][k])
            pairs = np.stack([z["pair_node"][po[k]:po[k + 1]], z["pair_pos"][po[k]:po[k + 1]]], 1) if whole else None
            self.items.append(dict(group=str(z["item_group"][k]), ps=self.param_names[int(z["item_params"][k])],
                                   kind=str(z["item_kind"][k]), win=int(z["item_win"][k]), round=int(z["item_round"][k]),
                                   view=view(no[k], no[k + 1], eo[k], eo[k + 1]), seq=z["item_seq"][so[k]:so[k + 1]].tobytes(),
                                   score=int(z["item_score"][k]), n_pairs=int(z["item_pairs"][k]), pairs=pairs,
                                   pair_sum=int(z["item_pair_sum"][k])))
        ro, rb = z["odd_read_off"], z["odd_read_bytes"]
        wo = z["odd_win_read_off"]
        reads = [[rb[ro[k]:ro[k + 1]].tobytes() for k in range(wo[w], wo[w + 1])] for w in range(len(wo) - 1)]
        co = z["win_cons_off"]
        self.windows = [dict(ps=self.param_names[int(z["win_params"][w])], reads=reads[int(z["win_reads"][w])],
                             cons=z["win_cons"][co[w]:co[w + 1]].tobytes(), nodes=int(z["win_nodes"][w]),
                             done=int(z["win_done"][w]), cells=int(z["win_cells"][w])) for w in range(len(co) - 1)]
        reads, seq = limit_reads()
        assert checksum(np.frombuffer(seq, np.uint8)) == int(z["limit_seq_sum"]), "the length-limit sequence differs"
        n, e = len(z["limit_node_base"]), len(z["limit_pred_rank"])
        self.limit = dict(view=poa.View(z["limit_node_base"], z["limit_node_id"], z["limit_node_out"], z["limit_in_end"],
                                        z["limit_pred_rank"]), seq=seq, n_pairs=int(z["limit_pairs"]),
                          pair_sum=int(z["limit_pair_sum"]))
        assert n > 0 and e > 0
        self.label_counts = dict(zip([str(x) for x in z["label_names"]], [int(x) for x in z["label_counts"]]))

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

    def group(self, *names):
        return [k for k, it in enumerate(self.items) if it["group"] in names]


def check_items(fx, idx, what=""):
    """gb_poa_align of the items idx (one call per parameter set, in the order given) equals the fixture: score, pair
    count and pairs, or their checksum where the fixture stores that."""
    for ps, ks in fx.by_params(idx).items():
        scores, pairs, off = poa.align(fx.p(ps), [fx.items[k]["view"] for k in ks], [fx.items[k]["seq"] for k in ks])
        assert off[0] == 0 and off[-1] == len(pairs)
        for i, k in enumerate(ks):
            it, got = fx.items[k], pairs[off[i]:off[i + 1]]
            name = f"{what} item {k} ({it['group']} {ps} {len(it['seq'])} {it['kind']})"
            assert scores[i] == it["score"], f"{name}: score {scores[i]} vs {it['score']}"
            assert len(got) == it["n_pairs"], f"{name}: {len(got)} pairs vs {it['n_pairs']}"
            if it["pairs"] is not None:
                assert (got == it["pairs"]).all(), f"{name}: pairs differ"
            else:
                assert checksum(got) == it["pair_sum"], f"{name}: pairs differ (checksum)"


def check_windows(fx, what=""):
    """gb_poa_consensus of the odd windows (one call per parameter set) equals the fixture."""
    calls = {}
    for w, win in enumerate(fx.windows):
        calls.setdefault(win["ps"], []).append(w)
    for ps, ws in calls.items():
        cons, nodes, done = poa.consensus(fx.p(ps), [fx.windows[w]["reads"] for w in ws])
        for i, w in enumerate(ws):
            assert cons[i] == fx.windows[w]["cons"], f"{what} {ps} window {w}: consensus differs"
            assert nodes[i] == fx.windows[w]["nodes"], f"{what} {ps} window {w}: {nodes[i]} nodes vs {fx.windows[w]['nodes']}"
        assert done == sum(fx.windows[w]["done"] for w in ws)
        assert poa.timing()[3] == sum(fx.windows[w]["cells"] for w in ws)
