#!/usr/bin/env python3
"""Generates tests/golden/bsw_mkchain_golden.npz: chains from seeds, recorded from bwa v1's own mem_chain
and mem_chain_flt (tools/bwa/bwamem.c:251-385) run live.

Build container only: needs /root/reference and oracle/_ref/libref_bwa.so (make ref). In a temporary
directory outside the repository, removed at the end, the reference's bwa sources are compiled where they
lie, with bwamem.c added, into a shared object; a synthetic FASTA is indexed with its bwa_idx_build and
mem_chain / mem_chain_flt are called through ctypes for every read, once with the default options and
once per option group. Nothing compiled from the reference and none of its text goes into the repository:
only the recorded inputs and outputs do.

mem_collect_intv is static, so the seeds come from its restatement over bwt_smem1 that
oracle/_ref/libref_bwa.so exports (ref_bwa_collect), plus bwt_sa, on the same index. That these are the
seeds mem_chain saw is shown by the self-check: py_mem_chain / py_chain_flt below restate the contract
(B-tree with t = 5, ks_introsort, the filter) in Python and must reproduce the live chains before and
after the filter, read by read. A failure of that assertion is a finding about the restatement.

The helpers (LiveBwa, make_reference, make_reads, py_*) are also used by tests/test_bsw_mkchain.py for
its live fuzz.
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
REF_TREE = "/root/reference"
BWA_DIR = os.path.join(REF_TREE, "tools", "bwa")
BWA_FILES = ("bwtindex.c bntseq.c bwt.c utils.c kstring.c QSufSort.c bwt_gen.c is.c rope.c rle.c bwa.c ksw.c "
             "bwamem.c bwamem_pair.c bwamem_extra.c kthread.c malloc_wrap.c").split()
OUT = os.path.join(HERE, "bsw_mkchain_golden.npz")
MAX_LEN = 250

DEFAULTS = dict(w=100, max_chain_gap=10000, max_occ=500, min_seed_len=19, min_chain_weight=0,
                max_chain_extend=1 << 30, mask_level=0.5, drop_ratio=0.5)
GROUPS = {"default": {}, "w": dict(w=4), "max_chain_gap": dict(max_chain_gap=50), "max_occ": dict(max_occ=8),
          "min_chain_weight": dict(min_chain_weight=40), "max_chain_extend": dict(max_chain_extend=2),
          "mask_level": dict(mask_level=0.9), "drop_ratio": dict(drop_ratio=0.9)}
INFO_FIELDS = ("pos", "rid", "is_alt", "w", "kept", "l_rep", "frac_rep")
LABELS = ("pos_tie", "gt9", "gt81", "weight_tie3", "kept1", "kept2", "dropped", "skipped", "contained",
          "strand", "alt_ovlp")


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---- the contract restated in Python -------------------------------------------------------------

T = 5  # kb_init(chn, 512) with sizeof(mem_chain_t) == 40


class _Node:
    __slots__ = ("keys", "ptr")

    def __init__(self, internal):
        self.keys = []  # chains (dicts), ordered by pos
        self.ptr = [] if internal else None


def _getp_aux(x, pos):
    """__kb_getp_aux: (i, r)."""
    n = len(x.keys)
    if n == 0:
        return -1, 0
    b, e = 0, n
    while b < e:
        mid = (b + e) >> 1
        if x.keys[mid]["pos"] < pos:
            b = mid + 1
        else:
            e = mid
    if b == n:
        return n - 1, 1
    r = (x.keys[b]["pos"] < pos) - (pos < x.keys[b]["pos"])
    return (b - 1, r) if r < 0 else (b, r)


class _Tree:
    def __init__(self):
        self.root = _Node(False)
        self.n_keys = 0

    def lower(self, pos):
        x, lower = self.root, None
        while x is not None:
            i, r = _getp_aux(x, pos)
            if i >= 0 and r == 0:
                return x.keys[i]
            if i >= 0:
                lower = x.keys[i]
            if x.ptr is None:
                return lower
            x = x.ptr[i + 1]
        return lower

    @staticmethod
    def _split(x, i, y):
        z = _Node(y.ptr is not None)
        z.keys = y.keys[T:]
        if y.ptr is not None:
            z.ptr = y.ptr[T:]
            y.ptr = y.ptr[:T]
        mid = y.keys[T - 1]
        y.keys = y.keys[:T - 1]
        x.ptr.insert(i + 1, z)
        x.keys.insert(i, mid)

    def put(self, c):
        self.n_keys += 1
        r = self.root
        if len(r.keys) == 2 * T - 1:
            s = _Node(True)
            s.ptr = [r]
            self.root = s
            self._split(s, 0, r)
            r = s
        x = r
        while True:
            if x.ptr is None:
                i, _ = _getp_aux(x, c["pos"])
                x.keys.insert(i + 1, c)
                return
            i = _getp_aux(x, c["pos"])[0] + 1
            if len(x.ptr[i].keys) == 2 * T - 1:
                self._split(x, i, x.ptr[i])
                if c["pos"] > x.keys[i]["pos"]:
                    i += 1
            x = x.ptr[i]

    def traverse(self):
        out = []

        def walk(x):
            for i in range(len(x.keys) + 1):
                if x.ptr is not None:
                    walk(x.ptr[i])
                if i < len(x.keys):
                    out.append(x.keys[i])
        walk(self.root)
        return out


def _pos2rid(contig_end, pos_f):
    return int(np.searchsorted(contig_end, pos_f, side="right"))


def _intv2rid(l_pac, contig_end, rb, re):
    if rb < l_pac and re > l_pac:
        return -2
    dep = lambda p: 2 * l_pac - 1 - p if p >= l_pac else p
    a = _pos2rid(contig_end, dep(rb))
    b = _pos2rid(contig_end, dep(re - 1)) if rb < re else a
    return a if a == b else -1


def expected_coords(s, max_occ):
    step = s // max_occ if s > max_occ else 1
    return min(max_occ, (s + step - 1) // step)


def py_mem_chain(o, l_pac, contig_end, is_alt, l_query, mems, flags=None):
    """mems: list of (m, n, s, [coords]) in any order. Returns (chains in traversal order, l_rep); a
    chain is a dict pos, rid, is_alt, seeds [(rbeg, qbeg, len)]. flags (a set) collects labels."""
    flags = flags if flags is not None else set()
    if l_query < o["min_seed_len"]:
        return [], 0
    mems = sorted(mems, key=lambda x: (x[0] << 32) | (x[1] + 1))
    b = e = l_rep = 0
    for m, n, s, _ in mems:
        if s <= o["max_occ"]:
            continue
        sb, se = m, n + 1
        if sb > e:
            l_rep += e - b
            b, e = sb, se
        else:
            e = max(e, se)
    l_rep += e - b
    tree = _Tree()
    for m, n, s, cs in mems:
        slen = n + 1 - m
        for rbeg in cs:
            rid = _intv2rid(l_pac, contig_end, rbeg, rbeg + slen)
            if rid < 0:
                flags.add("skipped")
                continue
            to_add = True
            if tree.n_keys:
                c = tree.lower(rbeg)
                if c is not None:
                    first, last = c["seeds"][0], c["seeds"][-1]
                    qend, rend = last[1] + last[2], last[0] + last[2]
                    if rid != c["rid"]:
                        pass
                    elif m >= first[1] and m + slen <= qend and rbeg >= first[0] and rbeg + slen <= rend:
                        to_add = False
                        flags.add("contained")
                    elif (last[0] < l_pac or first[0] < l_pac) and rbeg >= l_pac:
                        flags.add("strand")
                    else:
                        x, y = m - last[1], rbeg - last[0]
                        if (y >= 0 and x - y <= o["w"] and y - x <= o["w"] and x - last[2] < o["max_chain_gap"]
                                and y - last[2] < o["max_chain_gap"]):
                            c["seeds"].append((rbeg, m, slen))
                            to_add = False
            if to_add:
                tree.put({"pos": rbeg, "rid": rid, "is_alt": int(bool(is_alt[rid])), "seeds": [(rbeg, m, slen)]})
    return tree.traverse(), l_rep


def py_chain_weight(c):
    w = end = 0
    for rbeg, qbeg, ln in c["seeds"]:
        if qbeg >= end:
            w += ln
        elif qbeg + ln > end:
            w += qbeg + ln - end
        end = max(end, qbeg + ln)
    tmp, w, end = w, 0, 0
    for rbeg, qbeg, ln in c["seeds"]:
        if rbeg >= end:
            w += ln
        elif rbeg + ln > end:
            w += rbeg + ln - end
        end = max(end, rbeg + ln)
    w = min(w, tmp)
    return w if w < 1 << 30 else (1 << 30) - 1


def py_introsort(a, lt):
    """ks_introsort (ksort.h:176-226) in place."""
    n = len(a)
    if n < 1:
        return
    if n == 2:
        if lt(a[1], a[0]):
            a[0], a[1] = a[1], a[0]
        return

    def insertsort(lo, hi):
        for i in range(lo + 1, hi):
            j = i
            while j > lo and lt(a[j], a[j - 1]):
                a[j], a[j - 1] = a[j - 1], a[j]
                j -= 1

    def combsort(lo, m):
        gap = m
        while True:
            if gap > 2:
                gap = int(gap / 1.2473309501039786540366528676643)
                if gap in (9, 10):
                    gap = 11
            do_swap = False
            for i in range(lo, lo + m - gap):
                j = i + gap
                if lt(a[j], a[i]):
                    a[i], a[j] = a[j], a[i]
                    do_swap = True
            if not (do_swap or gap > 2):
                break
        if gap != 1:
            insertsort(lo, lo + m)

    d = 2
    while (1 << d) < n:
        d += 1
    stack = []
    s, t = 0, n - 1
    d <<= 1
    while True:
        if s < t:
            d -= 1
            if d == 0:
                combsort(s, t - s + 1)
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            rp = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], rp):
                    i += 1
                j -= 1
                while i <= j and lt(rp, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                insertsort(0, n)
                return
            s, t, d = stack.pop()


def py_chain_flt(o, chains, flags=None):
    """mem_chain_flt on the output of py_mem_chain; returns the chains left, each with w and kept."""
    flags = flags if flags is not None else set()
    f32 = np.float32
    if not chains:
        return []
    a = []
    for c in chains:
        c = dict(c)
        c["first"], c["kept"] = -1, 0
        c["w"] = py_chain_weight(c) & ((1 << 29) - 1)
        if c["w"] >= o["min_chain_weight"]:
            a.append(c)
    py_introsort(a, lambda x, y: x["w"] > y["w"])
    if not a:
        return []
    ws = [c["w"] for c in a]
    if len(a) >= 3 and len(set(ws)) < len(ws):
        flags.add("weight_tie3")
    beg = lambda c: c["seeds"][0][1]
    end = lambda c: c["seeds"][-1][1] + c["seeds"][-1][2]
    a[0]["kept"] = 3
    kept = [0]
    for i in range(1, len(a)):
        large = False
        broke = False
        for j in kept:
            b_max, e_min = max(beg(a[j]), beg(a[i])), min(end(a[j]), end(a[i]))
            if e_min > b_max and a[j]["is_alt"] != a[i]["is_alt"]:
                flags.add("alt_ovlp")
            if e_min > b_max and (not a[j]["is_alt"] or a[i]["is_alt"]):
                min_l = min(end(a[i]) - beg(a[i]), end(a[j]) - beg(a[j]))
                if f32(e_min - b_max) >= f32(min_l) * f32(o["mask_level"]) and min_l < o["max_chain_gap"]:
                    large = True
                    if a[j]["first"] < 0:
                        a[j]["first"] = i
                    if (f32(a[i]["w"]) < f32(a[j]["w"]) * f32(o["drop_ratio"])
                            and a[j]["w"] - a[i]["w"] >= o["min_seed_len"] << 1):
                        broke = True
                        flags.add("dropped")
                        break
        if not broke:
            kept.append(i)
            a[i]["kept"] = 2 if large else 3
    for i in kept:
        if a[i]["first"] >= 0:
            a[a[i]["first"]]["kept"] = 1
    i = k = 0
    while i < len(a):
        if a[i]["kept"] not in (0, 3):
            k += 1
            if k >= o["max_chain_extend"]:
                break
        i += 1
    for c in a[i:]:
        if c["kept"] < 3:
            c["kept"] = 0
    out = [c for c in a if c["kept"]]
    for c in out:
        if c["kept"] in (1, 2):
            flags.add("kept%d" % c["kept"])
    return out


# ---- the live reference ----------------------------------------------------------------------------

class _MemOpt(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_int) for k in "a b o_del e_del o_ins e_ins pen_unpaired pen_clip5 pen_clip3 w zdrop".split()]
                + [("max_mem_intv", ctypes.c_uint64)]
                + [(k, ctypes.c_int) for k in "T flag min_seed_len min_chain_weight max_chain_extend".split()]
                + [("split_factor", ctypes.c_float)]
                + [(k, ctypes.c_int) for k in "split_width max_occ max_chain_gap n_threads chunk_size".split()]
                + [(k, ctypes.c_float) for k in "mask_level drop_ratio XA_drop_ratio mask_level_redun mapQ_coef_len".split()]
                + [(k, ctypes.c_int) for k in "mapQ_coef_fac max_ins max_matesw max_XA_hits max_XA_hits_alt".split()]
                + [("mat", ctypes.c_int8 * 25)])


class _MemSeed(ctypes.Structure):
    _fields_ = [("rbeg", ctypes.c_int64), ("qbeg", ctypes.c_int32), ("len", ctypes.c_int32), ("score", ctypes.c_int)]


class _MemChain(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("m", ctypes.c_int), ("first", ctypes.c_int), ("rid", ctypes.c_int),
                ("w", ctypes.c_uint32, 29), ("kept", ctypes.c_uint32, 2), ("is_alt", ctypes.c_uint32, 1),
                ("frac_rep", ctypes.c_float), ("pos", ctypes.c_int64), ("seeds", ctypes.POINTER(_MemSeed))]


class _MemChainV(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("m", ctypes.c_size_t), ("a", ctypes.POINTER(_MemChain))]


class _BwaIdx(ctypes.Structure):
    _fields_ = [("bwt", ctypes.c_void_p), ("bns", ctypes.c_void_p), ("pac", ctypes.c_void_p)]


assert ctypes.sizeof(_MemSeed) == 24 and ctypes.sizeof(_MemChain) == 40


def available():
    return os.path.isdir(BWA_DIR) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_bwa.so"))


class LiveBwa:
    """bwa v1 with bwamem.c, compiled in a temporary directory, over one indexed reference.
    contigs: list of (name, uint8 codes 0..3, is_alt)."""

    def __init__(self, contigs):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import fmi_util
        self.dir = tempfile.mkdtemp(prefix="gb_mkchain_")
        objs = []
        for f in BWA_FILES:
            o = os.path.join(self.dir, f[:-2] + ".o")
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-w", "-DHAVE_PTHREAD", "-I" + BWA_DIR, "-c",
                                   os.path.join(BWA_DIR, f), "-o", o])
            objs.append(o)
        so = os.path.join(self.dir, "libbwa_live.so")
        subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-lz", "-lm", "-lpthread"])
        self.lib = L = ctypes.CDLL(so)
        fa, self.prefix = os.path.join(self.dir, "ref.fa"), os.path.join(self.dir, "ref")
        with open(fa, "w") as fh:
            for name, codes, _ in contigs:
                fh.write(">%s\n%s\n" % (name, "".join("ACGT"[c] for c in codes)))
        with open(self.prefix + ".alt", "w") as fh:
            for name, _, alt in contigs:
                if alt:
                    fh.write(name + "\n")
        ctypes.c_int.in_dll(L, "bwa_verbose").value = 1
        L.bwa_idx_build.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        assert L.bwa_idx_build(fa.encode(), self.prefix.encode(), 0, 10000000) == 0
        L.bwa_idx_load.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.bwa_idx_load.restype = ctypes.POINTER(_BwaIdx)
        self.idx = L.bwa_idx_load(self.prefix.encode(), 7).contents
        L.mem_opt_init.restype = ctypes.POINTER(_MemOpt)
        L.mem_chain.argtypes = [ctypes.POINTER(_MemOpt), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_void_p]
        L.mem_chain.restype = _MemChainV
        L.mem_chain_flt.argtypes = [ctypes.POINTER(_MemOpt), ctypes.c_int, ctypes.POINTER(_MemChain)]
        self.libc = ctypes.CDLL(None)
        self.libc.free.argtypes = [ctypes.c_void_p]
        self.codes = np.concatenate([c for _, c, _ in contigs]).astype(np.uint8)
        self.l_pac = len(self.codes)
        assert ctypes.cast(self.idx.bns, ctypes.POINTER(ctypes.c_int64))[0] == self.l_pac
        self.contig_end = np.cumsum([len(c) for _, c, _ in contigs]).astype(np.int64)
        self.is_alt = np.array([int(bool(a)) for _, _, a in contigs], np.uint8)
        # the seeds: mem_collect_intv's restatement and bwt_sa from the oracle's build of the same sources
        self.fmi_util = fmi_util
        self.rlib = fmi_util.ref_bwa()
        self.rbwt = self.rlib.ref_bwa_load((self.prefix + ".bwt").encode())

    def close(self):
        self.rlib.ref_bwa_free(self.rbwt)
        shutil.rmtree(self.dir, ignore_errors=True)

    def _opt(self, o):
        p = self.lib.mem_opt_init()
        for k, v in o.items():
            setattr(p.contents, k, v)
        return p

    def chains(self, read, o):
        """(stage 0, stage 1) for one read (uint8 codes 0..4): lists of chain dicts with pos, rid, is_alt,
        w, kept, frac_rep and seeds [(rbeg, qbeg, len, score)]."""
        p = self._opt(o)
        q = np.ascontiguousarray(read, np.uint8)
        v = self.lib.mem_chain(p, self.idx.bwt, self.idx.bns, len(q), q.ctypes.data, None)

        def grab(k, flt):
            out = []
            for i in range(k):
                c = v.a[i]
                out.append({"pos": c.pos, "rid": c.rid, "is_alt": c.is_alt, "w": c.w if flt else 0,
                            "kept": c.kept if flt else 0, "frac_rep": c.frac_rep,
                            "seeds": [(c.seeds[j].rbeg, c.seeds[j].qbeg, c.seeds[j].len, c.seeds[j].score)
                                      for j in range(c.n)]})
            return out
        s0 = grab(v.n, False)
        k = self.lib.mem_chain_flt(p, v.n, v.a) if v.n else 0
        s1 = grab(k, True)
        for i in range(k):
            self.libc.free(v.a[i].seeds)
        self.libc.free(v.a)
        self.libc.free(p)
        return s0, s1

    def seeds(self, read, o):
        """[(m, n, s, [coords])] for one read: the SMEMs of mem_collect_intv and, per SMEM, the coordinates
        mem_chain's loop takes."""
        per = self.fmi_util.bwa_smems(self.rlib, self.rbwt, np.asarray(read, np.uint8)[None, :], [len(read)],
                                      o["min_seed_len"])[0]
        out = []
        for m, n, k, l, s in per:
            step = s // o["max_occ"] if s > o["max_occ"] else 1
            rows = [k + j * step for j in range(expected_coords(s, o["max_occ"]))]
            cs = self.fmi_util.bwa_sa(self.rlib, self.rbwt, self.prefix + ".sa", rows)
            out.append((m, n, s, [int(x) for x in cs]))
        return out


# ---- inputs ------------------------------------------------------------------------------------------

def _mutate(rng, seq, n_sub):
    seq = seq.copy()
    for p in rng.choice(len(seq), size=min(n_sub, len(seq)), replace=False):
        seq[p] = (seq[p] + rng.integers(1, 4)) % 4
    return seq


def make_reference(seed=7):
    """Three contigs, the middle one ALT. Returns (contigs, sites): sites maps a kind to the list of
    (global start, length) regions reads are drawn around."""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    sites = {"tandem": [], "family": [], "mega": [], "alt_src": [], "unique": []}
    unit60, unit40 = rnd(60), rnd(40)
    sites["unit60"], sites["unit40"] = unit60, unit40
    # chr1: unique sequence, three tandem repeats of a 37-base unit, 60 family copies
    parts, pos = [], 0

    def add(x, kind=None):
        nonlocal pos
        if kind:
            sites[kind].append((pos, len(x)))
        parts.append(x)
        pos += len(x)
    add(rnd(3000), "unique")
    for copies in (12, 9, 15):
        u = rnd(37)
        add(np.concatenate([_mutate(rng, u, int(rng.random() < 0.3)) for _ in range(copies)]), "tandem")
        add(rnd(700), "unique")
    # a family copy lies between two A's (the reads' flanks meet the unit with a C, so that no copy extends
    # a segment of the unit and hides it from the SMEM search)
    def family(count):
        for _ in range(count):
            add(np.zeros(1, np.uint8))
            add(_mutate(rng, unit60, int(rng.integers(0, 2))), "family")
            add(np.zeros(1, np.uint8))
            add(rnd(int(rng.integers(60, 140))))
    family(60)
    alt_lo = pos
    add(rnd(2500), "alt_src")
    add(rnd(1000), "unique")
    chr1 = np.concatenate(parts)
    # chrA (ALT): a diverged copy of chr1's alt_src segment and of its first tandem repeat
    t0 = sites["tandem"][0]
    alt = np.concatenate([_mutate(rng, chr1[alt_lo:alt_lo + 2500], 40), rnd(200),
                          _mutate(rng, chr1[t0[0] - 100:t0[0] + t0[1] + 100], 6), rnd(300)])
    # chr2: 45 more family copies, 1050 exact copies of a 40-base unit, unique sequence
    parts2, base = [], len(chr1) + len(alt)
    pos = base
    parts = parts2
    add(rnd(1500), "unique")
    family(45)
    for _ in range(1050):
        add(unit40, "mega")
        add(np.concatenate([[0], rnd(int(rng.integers(6, 12))), [0]]).astype(np.uint8))
    add(rnd(2500), "unique")
    chr2 = np.concatenate(parts2)
    return [("chr1", chr1, 0), ("chrA", alt, 1), ("chr2", chr2, 0)], sites


def _rc(x):
    x = np.asarray(x, np.uint8)
    return np.where(x < 4, 3 - x, 4)[::-1].astype(np.uint8)


def make_reads(contigs, sites, n_scale=1.0, seed=11):
    """A list of uint8 code arrays (0..4), 30..250 bases, both strands."""
    rng = np.random.default_rng(seed)
    ref = np.concatenate([c for _, c, _ in contigs])
    ends = np.cumsum([len(c) for _, c, _ in contigs])
    L = len(ref)
    reads = []

    def length():
        return int(rng.choice([30, 50, 80, 101, 120, 151, 200, 250]))

    def finish(x, subs=None, n_ok=True):
        x = _mutate(rng, np.asarray(x, np.uint8), int(rng.integers(0, 5)) if subs is None else subs)
        if n_ok and rng.random() < 0.05 and len(x) > 40:
            x[int(rng.integers(0, len(x)))] = 4
        if rng.random() < 0.15 and len(x) > 60:  # a short deletion
            p, d = int(rng.integers(20, len(x) - 20)), int(rng.integers(1, 6))
            x = np.concatenate([x[:p], x[p + d:]])
        reads.append(_rc(x) if rng.random() < 0.5 else x)

    def around(kind, count, lens=None):
        for _ in range(int(count * n_scale)):
            s, ln = sites[kind][int(rng.integers(len(sites[kind])))]
            rl = length() if lens is None else int(rng.choice(lens))
            lo = int(rng.integers(max(0, s - rl + 25), max(1, min(L - rl, s + ln - 25))))
            finish(ref[lo:lo + rl])

    around("unique", 670)
    around("tandem", 800, [80, 120, 151, 200])
    around("alt_src", 200)
    # the family: the consensus unit with the read's own substitutions between flanks of one copy
    # (random flanks: the segments between the substitutions are then SMEMs of their own, found in most copies)
    for k in range(int(50 * n_scale)):
        s, ln = sites["family"][int(rng.integers(len(sites["family"])))]
        fl = int(rng.integers(5, 60))
        def rf(at):
            f = rng.integers(0, 4, fl).astype(np.uint8)
            f[at] = 1
            return f
        unit = sites["unit60"].copy()
        for p in ((30,), (20, 40), (25,), (33,))[k % 4]:
            unit[p + int(rng.integers(-3, 4))] ^= 1
        x = np.concatenate([rf(-1) if k % 5 else ref[s - fl:s], unit, rf(0) if k % 5 else ref[s + ln:s + ln + fl]])
        finish(x, subs=0, n_ok=False)
    around("family", 50, [80, 120, 151])
    # the 1050 exact copies: s > max_occ and step > 1
    for k in range(int(8 * n_scale)):
        s, ln = sites["mega"][int(rng.integers(1, len(sites["mega"]) - 1))]
        fl = int(rng.integers(1, 30))
        lf, rf = rng.integers(0, 4, fl).astype(np.uint8), rng.integers(0, 4, fl).astype(np.uint8)
        lf[-1] = rf[0] = 1
        if k % 4 == 0:
            lf, rf = ref[s - fl:s], ref[s + ln:s + ln + fl]
        finish(np.concatenate([lf, sites["unit40"], rf]), subs=0, n_ok=False)
    # across a contig boundary and across l_pac (forward end + its reverse complement)
    for _ in range(int(90 * n_scale)):
        e = int(ends[int(rng.integers(0, 2))])
        rl, off = length(), 0
        off = int(rng.integers(10, max(11, rl - 10)))
        finish(ref[e - off:e - off + rl])
    for _ in range(int(40 * n_scale)):
        k, k2 = int(rng.integers(25, 100)), int(rng.integers(25, 100))
        finish(np.concatenate([ref[L - k:], _rc(ref)[:k2]]))
    # chimeras within the last contig: a forward piece, then the reverse complement of another piece
    lo3, hi3 = int(ends[1]), int(ends[2])
    for _ in range(int(60 * n_scale)):
        a, b = (int(rng.integers(hi3 - 2400, hi3 - 100)) for _ in range(2))
        finish(np.concatenate([ref[a:a + 60], _rc(ref[b:b + 60])]), subs=int(rng.integers(0, 2)))
    # shorter than min_seed_len, and no SMEM at all
    for _ in range(int(10 * n_scale)):
        s = int(rng.integers(0, L - 20))
        reads.append(ref[s:s + int(rng.integers(5, 19))].copy())
    for _ in range(int(20 * n_scale)):
        reads.append(rng.integers(0, 4, length()).astype(np.uint8))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def pack_inputs(seed_lists):
    """MEM-record fields and coordinates for a list of per-read seed lists [(m, n, s, [coords])]."""
    read, m, n, nc, s, coords = [], [], [], [], [], []
    for r, per in enumerate(seed_lists):
        for mm, nn, ss, cs in per:
            read.append(r), m.append(mm), n.append(nn), nc.append(len(cs)), s.append(ss)
            coords.extend(cs)
    a = lambda x, t: np.array(x, t)
    return dict(read=a(read, np.int32), m=a(m, np.int32), n=a(n, np.int32), n_coord=a(nc, np.int32), s=a(s, np.int64),
                coords=a(coords, np.int64))


def pack_chains(per_read):
    """CSR arrays for a list (per read) of lists of chain dicts."""
    rco = np.zeros(len(per_read) + 1, np.int64)
    rco[1:] = np.cumsum([len(x) for x in per_read])
    flat = [c for x in per_read for c in x]
    cso = np.zeros(len(flat) + 1, np.int64)
    cso[1:] = np.cumsum([len(c["seeds"]) for c in flat])
    sd = np.array([s[:4] for c in flat for s in c["seeds"]], np.int64).reshape(-1, 4)
    # score == len for every seed (asserted by check_read), so it is not stored
    # nor is pos, the rbeg of a chain's first seed (asserted here), nor the offsets: counts pack better
    assert all(c["pos"] == c["seeds"][0][0] for c in flat)
    out = dict(n_chains=np.diff(rco).astype(np.int32), n_seeds=np.diff(cso).astype(np.int32), rbeg=sd[:, 0].copy(),
               qbeg=sd[:, 1].astype(np.int16), len=sd[:, 2].astype(np.int16))
    for f in ("rid", "is_alt", "l_rep", "frac_rep"):
        out[f] = np.array([c[f] for c in flat], np.float32 if f == "frac_rep" else np.int64 if f == "pos" else np.int32)
    return out


def pack_stage1(per0, per1):
    """Stage 1 as references into stage 0: mem_chain_flt moves whole chains and changes none, so a chain
    it leaves is a stage-0 chain of the same read (asserted) with w and kept. src is that chain's index
    in the group's stage-0 numbering."""
    rco = np.zeros(len(per1) + 1, np.int64)
    rco[1:] = np.cumsum([len(x) for x in per1])
    src, w, kept, base = [], [], [], 0
    same = ("pos", "rid", "is_alt", "frac_rep", "l_rep", "seeds")
    for c0, c1 in zip(per0, per1):
        used = set()
        for c in c1:
            k = next(i for i, d in enumerate(c0) if i not in used and all(d[f] == c[f] for f in same))
            used.add(k)
            src.append(base + k), w.append(c["w"]), kept.append(c["kept"])
        base += len(c0)
    return dict(n_chains=np.diff(rco).astype(np.int32), src=np.array(src, np.int32), w=np.array(w, np.int32), kept=np.array(kept, np.int32))


def expected(fx, g, stage):
    """The live chains of group g at `stage` as the arrays gb_bsw_seeds2chains returns: (read_chain_off,
    chain_seed_off, seeds dict rbeg / qbeg / len, info dict)."""
    p = "%s_s0_" % g
    csum = lambda x: np.concatenate([[0], np.cumsum(x, dtype=np.int64)])
    rco, cso = csum(fx[p + "n_chains"]), csum(fx[p + "n_seeds"])
    seeds = {"rbeg": fx[p + "rbeg"], "qbeg": fx[p + "qbeg"].astype(np.int32), "len": fx[p + "len"].astype(np.int32)}
    info = {f: fx[p + f] for f in ("rid", "is_alt", "l_rep", "frac_rep")}
    info["pos"] = seeds["rbeg"][cso[:-1]]
    nc = len(cso) - 1
    info["w"], info["kept"] = np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    if stage == 0:
        return rco, cso, seeds, info
    q = "%s_s1_" % g
    src = fx[q + "src"].astype(np.int64)
    n = cso[src + 1] - cso[src]
    cso1 = np.zeros(len(src) + 1, np.int64)
    cso1[1:] = np.cumsum(n)
    idx = np.repeat(cso[src] - cso1[:-1], n) + np.arange(int(cso1[-1]))
    seeds1 = {f: v[idx] for f, v in seeds.items()}
    info1 = {f: v[src] for f, v in info.items()}
    info1["w"], info1["kept"] = fx[q + "w"], fx[q + "kept"]
    return csum(fx[q + "n_chains"]), cso1, seeds1, info1


def check_read(live, read, o, seeds, flags=None):
    """The self-check for one read: the restatement on `seeds` against the live chains. Returns the live
    (stage 0, stage 1) with l_rep filled in."""
    s0, s1 = live.chains(read, o)
    mine0, l_rep = py_mem_chain(o, live.l_pac, live.contig_end, live.is_alt, len(read), seeds, flags)
    mine1 = py_chain_flt(o, mine0, flags)
    strip = lambda cs, flt: [(c["pos"], c["rid"], c["is_alt"], c["w"] if flt else 0, c["kept"] if flt else 0,
                             [tuple(s[:3]) for s in c["seeds"]]) for c in cs]
    assert strip(s0, False) == [(c["pos"], c["rid"], c["is_alt"], 0, 0, c["seeds"]) for c in mine0], "stage 0 differs"
    assert strip(s1, True) == strip(mine1, True), "stage 1 differs"
    fr = np.float32(l_rep) / np.float32(len(read)) if len(read) else np.float32(0)
    for c in s0 + s1:
        assert np.float32(c["frac_rep"]) == fr and all(s[3] == s[2] for s in c["seeds"])
        c["l_rep"] = l_rep
    if flags is not None:
        pos = [c["pos"] for c in s0]
        if len(set(pos)) < len(pos):
            flags.add("pos_tie")
        if len(s0) > 9:
            flags.add("gt9")
        if len(s0) > 81:
            flags.add("gt81")
    return s0, s1


def main():
    if not available():
        print("skipped: needs %s and oracle/_ref/libref_bwa.so (make ref)" % REF_TREE)
        return 0
    contigs, sites = make_reference()
    reads = make_reads(contigs, sites)
    live = LiveBwa(contigs)
    try:
        n = len(reads)
        print("reference %d bases, %d reads" % (live.l_pac, n))
        fx = dict(ref_codes=live.codes, contig_end=live.contig_end, contig_is_alt=live.is_alt,
                  lens=np.array([len(r) for r in reads], np.int32))
        codes = np.full((n, MAX_LEN), 4, np.uint8)
        for r, x in enumerate(reads):
            codes[r, :len(x)] = x
        fx["reads"] = codes
        labels = np.zeros((n, len(LABELS)), np.uint8)
        o = opts()
        seeds = [live.seeds(x, o) for x in reads]
        rng = np.random.default_rng(5)
        weight = np.array([sum(len(c) for *_, c in s) for s in seeds])
        for g, kw in GROUPS.items():
            o = opts(**kw)
            if g == "default":
                sel = np.arange(n)
            else:  # a few hundred reads: mostly light ones, a few of the heavy
                light, heavy = np.flatnonzero(weight <= 60), np.flatnonzero((weight > 60) & (weight <= 400))
                mega = np.flatnonzero(weight > 400)
                sel = np.sort(np.concatenate([rng.choice(light, 262, replace=False), rng.choice(heavy, 36, replace=False),
                                              rng.choice(mega, 2, replace=False)]))
            gs = [live.seeds(reads[r], o) for r in sel] if "max_occ" in kw else [seeds[r] for r in sel]
            per0, per1 = [], []
            for k, r in enumerate(sel):
                flags = set()
                try:
                    s0, s1 = check_read(live, reads[r], o, gs[k], flags)
                except AssertionError as e:
                    raise AssertionError("group %s read %d: %s" % (g, r, e))
                per0.append(s0), per1.append(s1)
                if g == "default":
                    for f in flags:
                        labels[r, LABELS.index(f)] = 1
            fx[g + "_reads"] = sel.astype(np.int32)
            for k, v in pack_inputs(gs).items():
                if g == "default" or "max_occ" in kw:
                    fx["%s_in_%s" % (g, k)] = v
            for st, pc in ((0, pack_chains(per0)), (1, pack_stage1(per0, per1))):
                for k, v in pc.items():
                    fx["%s_s%d_%s" % (g, st, k)] = v
            print("group %-16s %4d reads, %6d chains, %6d after the filter" % (g, len(sel), sum(map(len, per0)),
                                                                               sum(map(len, per1))))
        fx["labels"] = labels
        fx["label_names"] = np.array(LABELS)
        fx["group_names"] = np.array(list(GROUPS))
        fx["group_opts"] = np.array([[float(opts(**kw)[k]) for k in DEFAULTS] for kw in GROUPS.values()], np.float64)
        fx["opt_names"] = np.array(list(DEFAULTS))
        for k, name in enumerate(LABELS):
            print("label %-12s %5d reads" % (name, int(labels[:, k].sum())))
        np.savez_compressed(OUT, **fx)
        print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    finally:
        live.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
