"""The items of tests/golden/chain_extd2_edges_golden.npz: how they are made, which labels they must show, how they
are stored and loaded. Shared by tests/golden/make_chain_extd2_edges_golden.py and tests/test_chain_extd2_edges.py.

The kernel's layout arithmetic is restated here (row_bounds, n_col, eff_w, state_bytes, size_class, launch_group)
and every label is counted from it, never from a shape's name: a shape that misses its edge leaves its label at 0.

    m           = min(qlen, tlen, w + 1), w < 0 read as max(qlen, tlen): the cells of a full row
    n_col       = (m + 15) / 16 + 1: class 0 up to 16 (m <= 240), class 1 up to 64 (m <= 1008), class 2 above
    span        = en - st + 1 of the aligned range; at most 16 * ((m + 14) / 16 + 1), reached when st0 % 16 == 15,
                  which needs a band that slides or |tlen - qlen| >= 15
    pieces      = ceil(span / (64 * B)), B = 4 bytes a lane in class 0 and 16 above: one piece up to 1024 bytes
                  (m <= 1009), two up to 2048 (m <= 2033), then three
    state_bytes = 12 * T16 + Q16 + 16 (the reference's block and the 32-bit H[]); above 65536 it is class 3
    launch      = class x LDS bucket (up to 8, 16, 32, 64 KiB), and class 3
"""
import io
import os
import zipfile

import numpy as np

from genomicsbench_palisade_amd import gen

SEED = 20261021
MAX_BYTES = 400 * 1024
MAX_LEN = 32768
LDS_MAX = 64 * 1024
NEAR_LDS = 60 * 1024  # "near the limit": a state in the last 4 KiB below it
BUCKET_STATES = (8192, 8208, 16384, 16400, 32768, 32784)  # the launch buckets' edges and 16 bytes above
RESTATED_ROWS = 800   # the recorder runs the numpy restatement of the sweep on bucket-edge items up to this
RIGHT, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR = 0x02, 0x08, 0x10, 0x40, 0x80
# the multi-piece and class-3 shapes run under each of these over the same bases
VARIANT_FLAGS = (0, RIGHT, APPROX_MAX, APPROX_MAX | APPROX_DROP, EXTZ_ONLY | REV_CIGAR, EXTZ_ONLY | RIGHT | REV_CIGAR)
ZDROP, END_BONUS = 400, 10
WIDE_MUT = dict(long_indel=0.003)  # the wide group's rates of make_chain_extd2_golden.py (sub 0.06, indel 0.04)

LABELS = ("span_256_all_lanes_B4", "class_0_m240", "class_1_m241",
          "span_1024_one_piece", "class_2_one_piece_m1009", "span_1040_two_pieces",
          "span_2048_two_pieces", "span_2064_three_pieces",
          "state_65536_in_lds", "state_65552_in_workspace", "class_1_near_lds_limit", "class_2_near_lds_limit",
          "class_3_two_pieces", "class_3_three_pieces", "bucket_edge_8k", "bucket_edge_16k", "bucket_edge_32k",
          "zdropped_in_multi_piece_row", "band_exit_in_class_2", "wildcard_in_multi_piece_row",
          "cigar_over_64_words", "cigar_over_64_words_rev") + \
    tuple(f"multi_piece_flag_{f:#04x}" for f in VARIANT_FLAGS) + tuple(f"class_3_flag_{f:#04x}" for f in VARIANT_FLAGS)


# ---- the kernel's arithmetic, restated ----

def r16(v):
    return (v + 15) // 16 * 16


def eff_w(qlen, tlen, w):
    return min(max(qlen, tlen) if w < 0 else w, 4 * MAX_LEN)


def full_row(qlen, tlen, w):
    """m: the cells of a row that the band does not cut short."""
    return min(qlen, tlen, eff_w(qlen, tlen, w) + 1)


def n_col(qlen, tlen, w):
    return (full_row(qlen, tlen, w) + 15) // 16 + 1


def state_bytes(qlen, tlen):
    return 12 * r16(tlen) + r16(qlen) + 16


def size_class(qlen, tlen, w):
    if state_bytes(qlen, tlen) > LDS_MAX:
        return 3
    nc = n_col(qlen, tlen, w)
    return 0 if nc <= 16 else 1 if nc <= 64 else 2


def lds_bucket(qlen, tlen):
    sb = state_bytes(qlen, tlen)
    return 0 if sb <= 8192 else 1 if sb <= 16384 else 2 if sb <= 32768 else 3


def launch_group(qlen, tlen, w):
    c = size_class(qlen, tlen, w)
    return 0 if c == 3 else 1 + (3 - lds_bucket(qlen, tlen)) * 3 + (2 - c)


def worst_span(m):
    return 16 * ((m + 14) // 16 + 1)


class Rows:
    """The rows of one shape up to the band's exit: st0, en0, st, en per row, the aligned span, the pieces of the
    sweep and the in-band cells."""
    _cache = {}

    def __init__(self, qlen, tlen, w):
        w = eff_w(qlen, tlen, w)
        r = np.arange(qlen + tlen - 1, dtype=np.int64)
        st0 = np.maximum(np.maximum(0, r - qlen + 1), (r - w + 1) >> 1)
        en0 = np.minimum(np.minimum(tlen - 1, r), (r + w) >> 1)
        out = st0 > en0
        self.exits = bool(out.any())
        self.n = int(np.argmax(out)) if self.exits else len(r)  # rows swept when nothing else stops the sweep
        self.st0, self.en0 = st0[:self.n], en0[:self.n]
        self.st, self.en = self.st0 // 16 * 16, (self.en0 + 16) // 16 * 16 - 1
        self.span = self.en - self.st + 1
        self.cls = size_class(qlen, tlen, w)
        self.lane_bytes = 4 if self.cls == 0 else 16
        self.pieces = (self.span - 1) // (64 * self.lane_bytes) + 1
        self.cells = np.cumsum(self.en0 - self.st0 + 1)  # through row k
        self.m = full_row(qlen, tlen, w)
        self.state = state_bytes(qlen, tlen)

    @classmethod
    def of(cls, qlen, tlen, w):
        key = (int(qlen), int(tlen), int(w))
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]


def rows_of(it):
    return Rows.of(it["qlen"], it["tlen"], it["w"])


def item_class(items):
    return np.array([size_class(int(q), int(t), int(w)) for q, t, w in zip(items["qlen"], items["tlen"], items["w"])])


def item_group(items):
    return np.array([launch_group(int(q), int(t), int(w)) for q, t, w in zip(items["qlen"], items["tlen"], items["w"])])


def item_pieces(items):
    """The most pieces any row of each item is swept in."""
    return np.array([int(rows_of(it).pieces.max()) for it in items])


# ---- the items ----

def _pairs():
    """[(qlen, tlen, [(w, zdrop, flag)], mutation rates)]: a pair of sequences and the items that run over it."""
    uses = gen.EXTD2_USES

    def each(ws, flags, zdrop=ZDROP):
        return [(w, zdrop, f) for w in ws for f in flags]

    out = []
    # class 0 | 1: 240 | 241 cells a row, by the band and by either length
    out.append((600, 640, each((239, 240), uses), WIDE_MUT))
    for q, t in ((240, 700), (241, 700), (700, 240), (700, 241)):
        out.append((q, t, each((-1,), uses), WIDE_MUT))
    # class 1 | 2 and one | two pieces: 1008 | 1009 | 1010 cells a row
    out.append((1300, 1340, each((1007, 1008, 1009), VARIANT_FLAGS), WIDE_MUT))
    for q, t in ((1008, 1500), (1009, 1500), (1010, 1500), (1500, 1010)):
        out.append((q, t, each((-1,), VARIANT_FLAGS), WIDE_MUT))
    # two | three pieces: 2033 | 2034 cells a row
    for q, t in ((2033, 2100), (2034, 2100), (2100, 2034)):
        out.append((q, t, each((-1,), VARIANT_FLAGS), WIDE_MUT))
    # the LDS limit: 65536 bytes of state is the largest LDS launch, 65552 goes to the workspace
    out.append((240, 5440, each((100,), uses) + each((-1,), (0,)), WIDE_MUT))
    out.append((241, 5440, each((100,), VARIANT_FLAGS) + each((-1,), (0, EXTZ_ONLY | RIGHT | REV_CIGAR)), WIDE_MUT))
    out.append((500, 5200, each((400,), uses), WIDE_MUT))
    out.append((1100, 5360, each((-1,), VARIANT_FLAGS), WIDE_MUT))
    out.append((1100, 5376, each((-1,), VARIANT_FLAGS), WIDE_MUT))
    out.append((2100, 5300, each((-1,), VARIANT_FLAGS), WIDE_MUT))
    # the launch buckets: states of exactly 8, 16 and 32 KiB and 16 bytes above
    for q, t in ((112, 672), (113, 672), (48, 1360), (49, 1360), (112, 2720), (113, 2720)):
        out.append((q, t, each((50,), uses) + each((-1,), (0,)), WIDE_MUT))
    # a z-drop and a band exit in multi-piece rows, wildcards in a wide pair
    out.append((1300, 1340, each((-1,), (0, EXTZ_ONLY, APPROX_MAX | APPROX_DROP), zdrop=100), dict(tail=0.5, **WIDE_MUT)))
    out.append((1200, 2400, each((1100,), (0, EXTZ_ONLY)), WIDE_MUT))
    out.append((1300, 1340, each((-1,), (0, RIGHT)), dict(n_rate=0.01, **WIDE_MUT)))
    return out


def build_items():
    """The edge items as a gen.Extd2Items over map-ont: the bases once per pair, the items of a pair sharing q_off
    and t_off."""
    seqs, items, pos = [], [], 0
    for k, (qlen, tlen, variants, mut) in enumerate(_pairs()):
        one = gen.extd2_items(np.random.default_rng([SEED, k]), [(qlen, tlen)], w=0, zdrop=0, end_bonus=0, flag=0, **mut)
        seqs.append(one.seqs)
        for w, zdrop, flag in variants:
            items.append((pos, pos + qlen, qlen, tlen, w, zdrop, END_BONUS, flag))
        pos += qlen + tlen
    return gen.Extd2Items(gen.extd2_params(*gen.EXTD2_PRESETS["map-ont"]), np.concatenate(seqs),
                          np.array(items, gen.EXTD2_ITEM_DTYPE))


def rows_reached(x, res, rows_swept):
    """Per item the rows whose cells the sweep counts: all of them, up to the band's exit, or up to the row in
    which the z-drop fired (rows_swept, which only the recorder's restatement knows)."""
    return np.array([int(rows_swept[i]) if res[i][1] else rows_of(x.items[i]).n for i in range(x.n)])


def cells_reached(x, res, rows_swept):
    n = rows_reached(x, res, rows_swept)
    return np.array([int(rows_of(x.items[i]).cells[n[i] - 1]) for i in range(x.n)], np.int64)


def count_labels(x, res, rows_swept):
    """{label: count} of the items x with their 12-word records and the rows each swept."""
    c = dict.fromkeys(LABELS, 0)
    at = dict.fromkeys(BUCKET_STATES, 0)
    for i, it in enumerate(x.items):
        R = rows_of(it)
        q, t, flag = int(it["qlen"]), int(it["tlen"]), int(it["flag"])
        n = int(rows_swept[i]) if res[i][1] else R.n
        span, pieces = R.span[:n], R.pieces[:n]
        zdropped, n_cigar = bool(res[i][1]), int(res[i][10])
        by_band = zdropped and R.exits and n == R.n
        multi = pieces.max() >= 2
        c["span_256_all_lanes_B4"] += R.cls == 0 and span.max() == 256 == worst_span(R.m)
        c["class_0_m240"] += R.cls == 0 and R.m == 240
        c["class_1_m241"] += R.cls == 1 and R.m == 241
        c["span_1024_one_piece"] += R.cls in (1, 2) and span.max() == 1024 and pieces.max() == 1
        c["class_2_one_piece_m1009"] += R.cls == 2 and R.m == 1009 and pieces.max() == 1
        c["span_1040_two_pieces"] += R.cls == 2 and span.max() == 1040 and pieces.max() == 2
        c["span_2048_two_pieces"] += R.cls == 2 and span.max() == 2048 and pieces.max() == 2
        c["span_2064_three_pieces"] += R.cls == 2 and span.max() == 2064 and pieces.max() == 3
        c["state_65536_in_lds"] += R.state == 65536 and R.cls < 3
        c["state_65552_in_workspace"] += R.state == 65552 and R.cls == 3
        c["class_1_near_lds_limit"] += R.cls == 1 and NEAR_LDS < R.state <= LDS_MAX
        c["class_2_near_lds_limit"] += R.cls == 2 and NEAR_LDS < R.state <= LDS_MAX and multi
        c["class_3_two_pieces"] += R.cls == 3 and pieces.max() == 2
        c["class_3_three_pieces"] += R.cls == 3 and pieces.max() == 3
        if R.state in at:
            at[R.state] += 1
        c["zdropped_in_multi_piece_row"] += zdropped and not by_band and pieces[-1] >= 2
        c["band_exit_in_class_2"] += by_band and R.cls == 2 and multi and t - q > eff_w(q, t, int(it["w"]))
        wild = (x.seqs[it["q_off"]:it["q_off"] + q] == 4).any() or (x.seqs[it["t_off"]:it["t_off"] + t] == 4).any()
        c["wildcard_in_multi_piece_row"] += bool(wild) and multi
        c["cigar_over_64_words"] += n_cigar > 64 and not flag & REV_CIGAR
        c["cigar_over_64_words_rev"] += n_cigar > 64 and bool(flag & REV_CIGAR)
        if flag in VARIANT_FLAGS and not zdropped:
            c[f"multi_piece_flag_{flag:#04x}"] += R.cls == 2 and multi
            c[f"class_3_flag_{flag:#04x}"] += R.cls == 3 and multi
    for name, lo in (("bucket_edge_8k", 8192), ("bucket_edge_16k", 16384), ("bucket_edge_32k", 32768)):
        c[name] = min(at[lo], at[lo + 16])  # both sides of the edge
    return {k: int(v) for k, v in c.items()}


def check_labels(counts):
    assert tuple(counts) == LABELS, sorted(set(counts) ^ set(LABELS))
    short = [k for k, v in counts.items() if v <= 0]
    assert not short, f"labels at zero: {short}"


def cigarless(x, res):
    """(items that end without a CIGAR, items counted) among those that neither z-drop nor leave the band: both
    set zdropped."""
    res = np.asarray(res).reshape(x.n, 12)
    keep = res[:, 1] == 0
    return int((res[keep][:, 10] == 0).sum()), int(keep.sum())


# ---- the file ----

def save(path, **arrays):
    """An npz whose bytes depend on the arrays alone (np.savez stamps every member with the time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


class Fixture:
    """chain_extd2_edges_golden.npz: x (the gen.Extd2Items), res (n x 12), the CIGAR words, rows_swept and the
    stored label counts."""

    def __init__(self, path):
        z = self.z = np.load(path)
        self.size = os.path.getsize(path)
        self.x = gen.Extd2Items(z["params"], z["seqs"], z["items"])
        self.n = self.x.n
        self.res = z["res"].astype(np.int32)
        self.cigar = z["cigar"]
        self.off = np.concatenate([[0], np.cumsum(z["cigar_len"], dtype=np.int64)])
        self.rows_swept = z["rows_swept"]
        self.label_counts = dict(zip([str(k) for k in z["label_names"]], [int(v) for v in z["label_counts"]]))
        self.cls, self.group, self.pieces = item_class(self.x.items), item_group(self.x.items), item_pieces(self.x.items)

    def words(self, i):
        return self.cigar[self.off[i]:self.off[i + 1]]

    def check(self, run, sel=None):
        """run(Extd2Items) -> (res, cigar, cigar_off) of the items sel (all), compared in every byte."""
        sel = np.arange(self.n) if sel is None else np.asarray(sel, np.int64)
        assert len(sel)
        x = self.x.subset(sel)
        res, cig, off = run(x)
        want = [self.words(s) for s in sel]
        assert (np.diff(off) == [len(w) for w in want]).all() and off[0] == 0 and off[-1] == len(cig)
        got = res.view(np.int32).reshape(-1, 12)
        bad = np.flatnonzero((got != self.res[sel]).any(1))
        assert not len(bad), (len(bad), x.items[bad[0]], got[bad[0]], self.res[sel[bad[0]]])
        bad = np.flatnonzero(cig != np.concatenate(want))
        assert not len(bad), (len(bad), x.items[np.searchsorted(off, bad[0], "right") - 1])
