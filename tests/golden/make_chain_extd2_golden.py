"""Records tests/golden/chain_extd2_golden.npz: items for gb_chain_extd2 with the records and CIGARs that
minimap2's ksw_extd2_sse returns for them.

The live reference is tools/minimap2/ksw2_extd2_sse.c of the reference tree, compiled unmodified into a temporary
directory outside the repository with `gcc -O2 -msse4.1`, without HAVE_KALLOC and without KSW_CPU_DISPATCH (so the
symbol is ksw_extd2_sse and the allocator is libc's), and called through ctypes with m = 5 and the matrix of
ksw_gen_simple_mat (align.c:9-22), restated in live_mat below.

tests/chain_extd2_ref.py restates the contract in numpy and must equal the live path on every item in every
field and word. It counts the labels, each with a minimum (chain_extd2_ref.MINIMA) asserted here and again by
tests/test_chain_extd2.py on the stored counts. padding_sensitive compares the restatement with its keep_pad
switch; right_differs compares the live CIGAR with that of the same item with KSW_EZ_RIGHT toggled.

The fixture stores the parameter sets, per item its set, the bases as codes, the item records, the result records
and the CIGAR words.

Usage: python tests/golden/make_chain_extd2_golden.py [reference root]
"""
import ctypes
import os
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

import chain_extd2_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402
from make_abea_golden import REF_TREE  # noqa: E402

MAX_BYTES = 400 * 1024
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 128, 129, 257)
UNEQUAL = ((1, 17), (17, 1), (2, 33), (33, 2), (15, 64), (64, 15), (16, 129), (129, 16), (31, 48), (48, 31), (65, 128),
           (128, 65), (49, 257), (257, 49), (32, 33), (33, 32))
BANDS = (-1, 0, 1, 7, 15, 16, 17, 33, 100)
# (a, b, sc_ambi, q, e, q2, e2); `swapped` has the larger sum first, `early` takes the -min_sc > 2 * (q + e) return
PARAM_SETS = {"map-ont": gen.EXTD2_PRESETS["map-ont"], "asm5": gen.EXTD2_PRESETS["asm5"], "asm20": gen.EXTD2_PRESETS["asm20"],
              "sr": gen.EXTD2_PRESETS["sr"], "swapped": (2, 4, 1, 24, 1, 4, 2), "early": (1, 19, 1, 4, 2, 24, 1),
              "ambi0": (2, 4, 0, 4, 2, 24, 1)}


class Extz(ctypes.Structure):
    _fields_ = [("max_zd", ctypes.c_uint32), ("max_q", ctypes.c_int), ("max_t", ctypes.c_int), ("mqe", ctypes.c_int),
                ("mqe_t", ctypes.c_int), ("mte", ctypes.c_int), ("mte_q", ctypes.c_int), ("score", ctypes.c_int),
                ("m_cigar", ctypes.c_int), ("n_cigar", ctypes.c_int), ("reach_end", ctypes.c_int),
                ("cigar", ctypes.POINTER(ctypes.c_uint32))]


def live_mat(a, b, sc_ambi):
    """ksw_gen_simple_mat(5, mat, a, b, sc_ambi)."""
    a, b, sc_ambi = int(ref.i8(-a if a < 0 else a)), int(ref.i8(-b if b > 0 else b)), int(ref.i8(-sc_ambi if sc_ambi > 0 else sc_ambi))
    mat = np.full((5, 5), b, np.int8)
    mat[np.arange(4), np.arange(4)] = a
    mat[:, 4] = sc_ambi
    mat[4, :] = sc_ambi
    return np.ascontiguousarray(mat.reshape(-1))


class LiveExtd2:
    """ksw2_extd2_sse.c compiled in a temporary directory."""

    def __init__(self, ref_root=REF_TREE):
        src = os.path.join(ref_root, "tools", "minimap2", "ksw2_extd2_sse.c")
        if not os.path.exists(src):
            raise FileNotFoundError(src)
        self.dir = tempfile.mkdtemp(prefix="gb_chain_extd2_")
        so = os.path.join(self.dir, "libksw_extd2_live.so")
        subprocess.check_call(["gcc", "-O2", "-msse4.1", "-fPIC", "-shared", "-w", src, "-o", so])
        self.lib = ctypes.CDLL(so)
        vp, ci, c8 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int8
        self.lib.ksw_extd2_sse.argtypes = [vp, ci, vp, ci, vp, c8, vp, c8, c8, c8, c8, ci, ci, ci, ci, ctypes.POINTER(Extz)]
        self.lib.ksw_extd2_sse.restype = None
        self.libc = ctypes.CDLL(None)
        self.libc.free.argtypes = [vp]

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def align(self, params, query, target, w, zdrop, end_bonus, flag):
        """(tuple of ref.FIELDS, uint32 CIGAR words) of one call."""
        p = np.asarray(params).reshape(-1)[0]
        mat = live_mat(int(p["a"]), int(p["b"]), int(p["sc_ambi"]))
        query, target = np.ascontiguousarray(query, np.uint8), np.ascontiguousarray(target, np.uint8)
        ez = Extz()
        ctypes.memset(ctypes.byref(ez), 0, ctypes.sizeof(ez))
        self.lib.ksw_extd2_sse(None, len(query), query.ctypes.data, len(target), target.ctypes.data, 5, mat.ctypes.data,
                               int(p["q"]), int(p["e"]), int(p["q2"]), int(p["e2"]), w, zdrop, end_bonus, flag,
                               ctypes.byref(ez))
        cig = np.array(ez.cigar[:ez.n_cigar], np.uint32) if ez.n_cigar else np.zeros(0, np.uint32)
        if ez.cigar:
            self.libc.free(ez.cigar)
        rec = (ez.max_zd & 0x7fffffff, ez.max_zd >> 31, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score,
               ez.reach_end, ez.n_cigar, 0)
        return rec, cig

    def align_item(self, x, i, flag=None):
        q, t, it = x.item(i)
        return self.align(x.params, q, t, int(it["w"]), int(it["zdrop"]), int(it["end_bonus"]),
                          int(it["flag"]) if flag is None else flag)


def equal(a, b):
    return tuple(int(v) for v in a[0]) == tuple(int(v) for v in b[0]) and len(a[1]) == len(b[1]) and (a[1] == b[1]).all()


def build_items(rng):
    """[(group, parameter set name, gen.Extd2Items)]."""
    parts = []

    def add(group, pset, shapes, **kw):
        parts.append((group, pset, gen.extd2_items(rng, shapes, params=gen.extd2_params(*PARAM_SETS[pset]), **kw)))

    # every size at which a path changes, crossed with the bands and mm_align1's four uses
    shapes = [(n, n) for n in SIZES] + list(UNEQUAL)
    for w in BANDS:
        for flag in gen.EXTD2_USES:
            add("shape", "map-ont", shapes, w=w, flag=flag, zdrop=400)
    diverged = dict(sub=0.25, indel=0.10, tail=0.4)
    for zdrop in (-1, 8, 30, 400):
        for bonus in (-1, 10):
            for flag in gen.EXTD2_USES:
                add("zdrop", "map-ont", [(90, 100), (130, 129), (200, 260), (300, 280)], w=(33, 100, 751), zdrop=zdrop,
                    end_bonus=bonus, flag=flag, **diverged)
    for flag in (ref.APPROX_MAX | ref.APPROX_DROP, ref.RIGHT, ref.REV_CIGAR, ref.APPROX_MAX | ref.APPROX_DROP | ref.EXTZ_ONLY):
        for zdrop in (8, 400):
            add("flags", "map-ont", [(33, 33), (64, 70), (129, 120), (257, 257)], w=(17, 100), zdrop=zdrop, flag=flag)
            add("flags", "map-ont", [(33, 33), (64, 70), (129, 120), (257, 257)], w=(17, 100), zdrop=zdrop, flag=flag, **diverged)
    for pset in ("asm5", "asm20", "sr", "swapped", "early"):
        for flag in gen.EXTD2_USES:
            add("params", pset, [(17, 17), (48, 64), (129, 129), (257, 200)] * 2, w=(-1, 17, 100), flag=flag,
                long_indel=0.01)
    for pset in ("map-ont", "ambi0"):
        for flag in gen.EXTD2_USES:
            add("ambi", pset, [(17, 17), (48, 64), (129, 129), (257, 200)], w=(-1, 17, 100), flag=flag, n_rate=0.05)
    for period in (1, 2, 3, 5):
        for flag in (0, ref.RIGHT, ref.EXTZ_ONLY | ref.RIGHT | ref.REV_CIGAR, ref.EXTZ_ONLY):
            add("repeat", "map-ont", [(60, 64), (120, 129), (250, 257)], w=(33, 100), zdrop=400, flag=flag, repeat=period)
    add("longgap", "map-ont", [(257, 300), (400, 330), (520, 600), (600, 520)] * 4, w=(100, 751), long_indel=0.012)
    add("longgap", "swapped", [(257, 300), (400, 330), (520, 600), (600, 520)] * 2, w=(100, 751), long_indel=0.012)
    # wide rows: w = 751 extensions and fills, one item without a band (more than 64 blocks per row), one whose band
    # leaves the matrix
    for (shape, flag) in (((1000, 1100), ref.EXTZ_ONLY), ((2000, 1800), 0), ((2900, 3000), ref.EXTZ_ONLY | ref.RIGHT | ref.REV_CIGAR)):
        add("wide", "map-ont", [shape], w=751, zdrop=400, flag=flag, long_indel=0.003)
    add("wide", "map-ont", [(2000, 2040)], w=-1, zdrop=400, flag=0, long_indel=0.003)
    add("wide", "map-ont", [(1200, 2200)], w=751, zdrop=400, flag=ref.EXTZ_ONLY)
    add("empty", "map-ont", [(0, 5), (5, 0), (0, 0)], w=10)
    return parts


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveExtd2(ref_root)
    rng = np.random.default_rng(20261020)
    parts = build_items(rng)
    labels = dict.fromkeys(ref.LABELS, 0)
    names = list(PARAM_SETS)
    recs, cigs, lens = [], [], []
    for group, pset, x in parts:
        P = ref.Par(x.params)
        for i in range(x.n):
            want = live.align_item(x, i)
            got = ref.align_item(x, i, labels=labels)
            assert equal(got, want), (group, pset, i, x.items[i], got[0], want[0])
            it = x.items[i]
            if it["qlen"] and it["tlen"] and not P.early:
                labels["padding_sensitive"] += not equal(ref.align_item(x, i, keep_pad=True), want)
                other = live.align_item(x, i, flag=int(it["flag"]) ^ ref.RIGHT)
                labels["right_differs"] += not (len(other[1]) == len(want[1]) and (other[1] == want[1]).all())
            recs.append(want[0]), cigs.append(want[1]), lens.append(len(want[1]))
        print(f"{group:8s} {pset:8s} {x.n:3d} items", flush=True)
    live.close()
    for k in ref.LABELS:
        print(f"label {k:22s} {labels[k]:9d} (min {ref.MINIMA.get(k, 0)})")
    short = [k for k, v in ref.MINIMA.items() if labels[k] < v]
    assert not short, f"labels below their minimum: {short}"
    allx = gen.Extd2Items.concat([x for _, _, x in parts])
    out = os.path.join(HERE, "chain_extd2_golden.npz")
    np.savez_compressed(
        out, param_names=np.array(names), params=np.concatenate([gen.extd2_params(*PARAM_SETS[k]) for k in names]),
        param_id=np.concatenate([[names.index(p)] * x.n for _, p, x in parts]).astype(np.int8),
        group=np.concatenate([[g] * x.n for g, _, x in parts]), seqs=allx.seqs, items=allx.items,
        res=np.array(recs, np.int32), cigar=np.concatenate(cigs).astype(np.uint32), cigar_len=np.array(lens, np.int32),
        label_names=np.array(list(labels)), label_counts=np.array(list(labels.values()), np.int64),
        label_minima=np.array([ref.MINIMA.get(k, 0) for k in labels], np.int64))
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {allx.n} items, {sum(lens)} CIGAR words")
    assert os.path.getsize(out) <= MAX_BYTES, "thin the long items first"


if __name__ == "__main__":
    main()
