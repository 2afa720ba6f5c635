#!/usr/bin/env python3
"""Writes tests/golden/bsw_matesw_golden.npz: inputs and expected outputs of gb_bsw_pestat and
gb_bsw_mate_rescue, recorded from the live reference.

The reference is bwa (tools/bwa of the reference tree) compiled by LiveBwa of make_bsw_mkchain_golden.py in a
temporary directory outside the tree; mem_pestat, mem_matesw, mem_align1_core and ksw_align2 are called
through ctypes. The reference sequence is make_reference()'s and is not stored again (the mkchain fixture
holds it). Only recorded inputs and outputs are written.

Two sources of pairs:
  aligned      read pairs drawn from the reference around a mean insert, mostly FR; one mate is mutated until
               it has no seed, replaced by a chimera, or taken from elsewhere. Stage-0 regions come from live
               mem_align1_core. Their pes is live mem_pestat's.
  constructed  hand-made region lists around real sequence, under a hand-set pes with all four orientations
               open: anchors near contig ends and near 0 / 2 l_pac, mates at the edges of [low, high], mate
               lists built around what the rescue will find (a first pass with an empty list tells).
The restatement in Python (py_pestat, py_rescue) must equal the live result in every field; it counts the
labels, each of which has a minimum that is asserted here and again by the test on the stored counts.

Run from the repository root after `make ref`: python3 tests/golden/make_bsw_matesw_golden.py
(GB_MATESW_SCALE=0.2 GB_MATESW_DRAFT=1 makes a small draft and prints the labels that fall short instead of
asserting them.)"""
import ctypes
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_bsw_mkchain_golden as mk  # noqa: E402
import make_bsw_regs_golden as rg  # noqa: E402

OUT = os.path.join(HERE, "bsw_matesw_golden.npz")
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, min_seed_len=19, max_chain_gap=10000, pen_unpaired=17,
                max_matesw=50, max_ins=10000, mask_level=0.5, mask_level_redun=0.95)
OPEN = [(100, 400, 0)] * 4  # (low, high, failed) per orientation: the constructed pairs' pes
# group -> (option overrides, source of pairs, pes: "live" or a list of four (low, high, failed))
GROUPS = {"default": ({}, "aligned", "live"),
          "open": ({}, "constructed", OPEN),
          "ab": (dict(a=2, b=8), "constructed", OPEN),
          "o_ins0": (dict(o_ins=0), "constructed", OPEN),
          "max_matesw": (dict(max_matesw=2), "constructed", OPEN),
          "pen_unpaired": (dict(pen_unpaired=0), "constructed", OPEN),
          "mask_level_redun": (dict(mask_level_redun=0.5), "constructed", OPEN),
          "min_seed_len": (dict(min_seed_len=10), "constructed", OPEN),
          "fr_only": ({}, "constructed", [(0, 0, 1), (100, 400, 0), (0, 0, 1), (0, 0, 1)]),
          "wide": ({}, "wide", [(0, 0, 1), (1, 16383 - 255 - 2, 0), (0, 0, 1), (0, 0, 1)])}
FIELDS = tuple(f for f in rg.FIELDS if f not in ("mapq", "hash"))
LABELS = ("resc_FF", "resc_FR", "resc_RF", "resc_RR", "ran_FF", "ran_FR", "ran_RF", "ran_RR", "clamp_0", "clamp_2l",
          "clip_fwd", "clip_mir", "rid_mismatch", "short_window", "empty_window", "noreg_score", "noreg_qb", "ins_head",
          "ins_middle", "ins_tail", "ins_equal", "ins_empty", "dedup_rescued_removed", "dedup_existing_removed",
          "dedup_after_nothing", "later_skipped", "max_matesw_reached", "pen_excluded", "mate_N", "dp16",
          "ps_cnt_fail", "ps_ratio_fail", "ps_low_clamp", "ps_widen", "ex_noreg", "ex_sub", "ex_rid", "ex_is")
LABEL_MIN = 5
MATE_LENS = (1, 63, 64, 65, 128, 129, 192, 193, 255)
DIRS = ("FF", "FR", "RF", "RR")
XSUBO, XSTART, XBYTE = 0x40000, 0x80000, 0x10000


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---- the contract restated in Python -------------------------------------------------------------

def infer_dir(l_pac, b1, b2):
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def cal_sub(o, a):
    ml = np.float32(o["mask_level"])
    for x in a[1:]:
        b_max, e_min = max(x["qb"], a[0]["qb"]), min(x["qe"], a[0]["qe"])
        if e_min > b_max:
            min_l = min(x["qe"] - x["qb"], a[0]["qe"] - a[0]["qb"])
            if np.float32(e_min - b_max) >= np.float32(min_l) * ml:
                return x["score"]
    return o["min_seed_len"] * o["a"]


def py_pestat(o, l_pac, lists, flags):
    """mem_pestat over lists (one region list per read). Returns four dicts low, high, failed, avg, std; flags
    receives (label, count) increments as a list."""
    isize = [[], [], [], []]
    for p in range(len(lists) // 2):
        r0, r1 = lists[2 * p], lists[2 * p + 1]
        if not r0 or not r1:
            flags.append("ex_noreg")
            continue
        if cal_sub(o, r0) > 0.8 * r0[0]["score"] or cal_sub(o, r1) > 0.8 * r1[0]["score"]:
            flags.append("ex_sub")
            continue
        if r0[0]["rid"] != r1[0]["rid"]:
            flags.append("ex_rid")
            continue
        d, dist = infer_dir(l_pac, r0[0]["rb"], r1[0]["rb"])
        if dist and dist <= o["max_ins"]:
            isize[d].append(dist)
        else:
            flags.append("ex_is")
    pes = []
    for d in range(4):
        q = sorted(isize[d])
        r = dict(low=0, high=0, failed=0, avg=0.0, std=0.0)
        pes.append(r)
        if len(q) < 10:
            r["failed"] = 1
            flags.append("ps_cnt_fail")
            continue
        n = len(q)
        p25, p75 = q[int(.25 * n + .499)], q[int(.75 * n + .499)]
        r["low"] = int(p25 - 2.0 * (p75 - p25) + .499)
        r["low"] = max(r["low"], 1)
        r["high"] = int(p75 + 2.0 * (p75 - p25) + .499)
        inside = [v for v in q if r["low"] <= v <= r["high"]]
        avg = 0.0
        for v in inside:
            avg += float(v)
        avg /= len(inside)
        var = 0.0
        for v in inside:
            var += (float(v) - avg) * (float(v) - avg)
        std = math.sqrt(var / len(inside))
        r["avg"], r["std"] = avg, std
        r["low"] = int(p25 - 3.0 * (p75 - p25) + .499)
        r["high"] = int(p75 + 3.0 * (p75 - p25) + .499)
        wid = False
        if r["low"] > avg - 4.0 * std:
            r["low"], wid = int(avg - 4.0 * std + .499), True
        if r["high"] < avg + 4.0 * std:
            r["high"], wid = int(avg + 4.0 * std + .499), True
        if wid:
            flags.append("ps_widen")
        if r["low"] < 1:
            r["low"] = 1
            flags.append("ps_low_clamp")
    mx = max(len(x) for x in isize)
    for d in range(4):
        if not pes[d]["failed"] and len(isize[d]) < mx * 0.05:
            pes[d]["failed"] = 1
            flags.append("ps_ratio_fail")
    return pes


class Ctx:
    """What the restatement needs of the reference: its bases, the contigs, and ksw_align2 (live)."""

    def __init__(self, codes, contig_end, ksw):
        self.codes, self.l_pac, self.contig_end, self.ksw = codes, len(codes), [int(x) for x in contig_end], ksw

    def fetch(self, rb, re):
        l = self.l_pac
        if rb < l:
            return self.codes[rb:re].copy()
        return (3 - self.codes[2 * l - re:2 * l - rb])[::-1].copy()

    def clip(self, mid):
        """The contig, or its mirror, that holds mid: (rid, far_beg, far_end)."""
        l = self.l_pac
        pos_f = 2 * l - 1 - mid if mid >= l else mid
        rid = next(k for k, e in enumerate(self.contig_end) if e > pos_f)
        fb, fe = (self.contig_end[rid - 1] if rid else 0), self.contig_end[rid]
        if mid >= l:
            fb, fe = 2 * l - fe, 2 * l - fb
        return rid, fb, fe, mid >= l


def dedup_nopatch(o, l_pac, regs, flags):
    """mem_sort_dedup_patch with a null bns: the restatement of the regs generator with mem_patch_reg off."""
    saved = rg.py_patch_pre
    rg.py_patch_pre = lambda *a: None
    try:
        oo = dict(o, w=100)
        out, _ = rg.py_dedup(oo, l_pac, np.zeros(64, np.uint8), regs, None, flags)
    finally:
        rg.py_patch_pre = saved
    return out


def py_matesw(o, cx, pes, a, ms, ma, flags):
    """One mem_matesw call: anchor a, mate ms, the mate's list ma (changed in place). Returns n."""
    l_pac, l_ms = cx.l_pac, len(ms)
    skip = [1 if p["failed"] else 0 for p in pes]
    for m in ma:
        r, dist = infer_dir(l_pac, a["rb"], m["rb"])
        if pes[r]["low"] <= dist <= pes[r]["high"]:
            skip[r] = 1
    if sum(skip) == 4:
        return 0, True
    n = 0
    for r in range(4):
        if skip[r]:
            continue
        is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
        near = pes[r]["low"] if is_larger else -pes[r]["high"]
        far = pes[r]["high"] if is_larger else -pes[r]["low"]
        rb, re = a["rb"] + near - (l_ms if is_rev else 0), a["rb"] + far + (0 if is_rev else l_ms)
        if rb < 0:
            rb = 0
            flags.add("clamp_0")
        if re > 2 * l_pac:
            re = 2 * l_pac
            flags.add("clamp_2l")
        run = False
        if rb < re:
            rid, fb, fe, mir = cx.clip((rb + re) >> 1)
            if fb > rb or fe < re:
                flags.add("clip_mir" if mir else "clip_fwd")
            rb, re = max(rb, fb), min(re, fe)
            if a["rid"] != rid:
                flags.add("rid_mismatch")
            elif re - rb < o["min_seed_len"]:
                flags.add("short_window")
            else:
                run = True
        else:
            flags.add("empty_window")
        if run:
            seq = mk._rc(ms) if is_rev else np.asarray(ms, np.uint8)
            xtra = XSUBO | XSTART | (XBYTE if l_ms * o["a"] < 250 else 0) | (o["min_seed_len"] * o["a"])
            if not xtra & XBYTE:
                flags.add("dp16")
            if (np.asarray(ms) > 3).any():
                flags.add("mate_N")
            flags.add("ran_" + DIRS[r])
            flags.add("win_%d" % (re - rb))
            flags.add("mlen_%d" % l_ms)
            k = cx.ksw(seq, cx.fetch(rb, re), xtra, o)
            if k["score"] >= o["min_seed_len"] and k["qb"] >= 0:
                b = rg.new_reg(rid=a["rid"], is_alt=a["is_alt"], score=k["score"], csub=k["score2"], secondary=-1)
                if is_rev:
                    b["qb"], b["qe"] = l_ms - (k["qe"] + 1), l_ms - k["qb"]
                    b["rb"], b["re"] = 2 * l_pac - (rb + k["te"] + 1), 2 * l_pac - (rb + k["tb"])
                else:
                    b["qb"], b["qe"] = k["qb"], k["qe"] + 1
                    b["rb"], b["re"] = rb + k["tb"], rb + k["te"] + 1
                b["seedcov"] = min(b["re"] - b["rb"], b["qe"] - b["qb"]) >> 1
                pos = next((i for i, m in enumerate(ma) if m["score"] < b["score"]), len(ma))
                if not ma:
                    flags.add("ins_empty")
                elif pos == 0:
                    flags.add("ins_head")
                elif pos == len(ma):
                    flags.add("ins_equal" if ma[-1]["score"] == b["score"] else "ins_tail")
                else:
                    flags.add("ins_equal" if ma[pos - 1]["score"] == b["score"] else "ins_middle")
                b["_new"] = True
                ma.insert(pos, b)
                flags.add("resc_" + DIRS[r])
            else:
                b = None
                flags.add("noreg_qb" if k["score"] >= o["min_seed_len"] else "noreg_score")
            n += 1
        if n:
            if not (run and b is not None):
                flags.add("dedup_after_nothing")
            before = [id(x) for x in ma]
            news = {id(x) for x in ma if x.get("_new")}
            kept = dedup_nopatch(o, l_pac, ma, set())
            gone = set(before) - {id(x) for x in kept}
            if gone & news:
                flags.add("dedup_rescued_removed")
            if gone - news:
                flags.add("dedup_existing_removed")
            ma[:] = kept
    return n, False


def py_rescue(o, cx, pes, reads, lists, flags):
    """The rescue loop of mem_sam_pe for one pair: reads[2], lists[2] (lists of region dicts, copied). Returns
    (the two final lists, n, the number of rounds the pair needs)."""
    a = [[dict(x) for x in lists[0]], [dict(x) for x in lists[1]]]
    b = [[dict(x) for x in a[i] if x["score"] >= a[i][0]["score"] - o["pen_unpaired"]] for i in range(2)]
    n, rounds = 0, 0
    for i in range(2):
        if len(b[i]) < len(a[i]):
            flags.add("pen_excluded")
        if len(b[i]) > o["max_matesw"]:
            flags.add("max_matesw_reached")
        ran = False
        for j in range(min(len(b[i]), o["max_matesw"])):
            k, all_skipped = py_matesw(o, cx, pes, b[i][j], reads[1 - i], a[1 - i], flags)
            if all_skipped and ran and not all(p["failed"] for p in pes):
                flags.add("later_skipped")
            if k:
                ran = True
                rounds = max(rounds, j + 1)
            n += k
    for i in range(2):
        for x in a[i]:
            x.pop("_new", None)
    return a, n, rounds


# ---- the live reference ----------------------------------------------------------------------------

class _Kswr(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in "score te qe score2 te2 tb qb".split()]


class _Pes(ctypes.Structure):
    _fields_ = [("low", ctypes.c_int), ("high", ctypes.c_int), ("failed", ctypes.c_int), ("avg", ctypes.c_double),
                ("std", ctypes.c_double)]


assert ctypes.sizeof(_Pes) == 32


class _Quiet:
    """The reference prints from mem_pestat (stderr) and from its seed extension (stdout): not into this log."""

    def __init__(self, fd):
        self.fd = fd

    def __enter__(self):
        (sys.stderr if self.fd == 2 else sys.stdout).flush()
        self.saved, null = os.dup(self.fd), os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, self.fd)
        os.close(null)

    def __exit__(self, *exc):
        if self.fd == 1:
            ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved, self.fd)
        os.close(self.saved)


class LivePair:
    def __init__(self, live):
        self.live, L = live, live.lib
        self.lr = rg.LiveRegs(live)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        popt = ctypes.POINTER(mk._MemOpt)
        L.ksw_align2.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp]
        L.ksw_align2.restype = _Kswr
        L.mem_pestat.argtypes = [popt, ctypes.c_int64, ci, ctypes.POINTER(rg._AlnRegV), ctypes.POINTER(_Pes)]
        L.mem_pestat.restype = None
        L.mem_matesw.argtypes = [popt, vp, vp, ctypes.POINTER(_Pes), ctypes.POINTER(rg._AlnReg), ci, vp,
                                 ctypes.POINTER(rg._AlnRegV)]
        self.libc = live.libc
        self.libc.malloc.restype = ctypes.c_void_p
        self.libc.malloc.argtypes = [ctypes.c_size_t]
        self._opts = {}

    def opt(self, o):
        key = tuple(sorted(o.items()))
        if key not in self._opts:
            p = self.live._opt(o)
            self.live.lib.bwa_fill_scmat(o["a"], o["b"], ctypes.addressof(p.contents) + mk._MemOpt.mat.offset)
            self._opts[key] = p
        return self._opts[key]

    def ksw(self, seq, tgt, xtra, o):
        p = self.opt(o).contents
        q, t = np.ascontiguousarray(seq, np.uint8).copy(), np.ascontiguousarray(tgt, np.uint8).copy()
        r = self.live.lib.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5,
                                     ctypes.addressof(p) + mk._MemOpt.mat.offset, p.o_del, p.e_del, p.o_ins, p.e_ins,
                                     xtra, None)
        return {k: getattr(r, k) for k, _ in _Kswr._fields_}

    def stage0(self, o, read):
        """mem_align1_core: the read's stage-0 regions."""
        L, idx = self.live.lib, self.live.idx
        q = np.ascontiguousarray(read, np.uint8).copy()
        with _Quiet(1):
            v = L.mem_align1_core(self.opt(o), idx.bwt, idx.bns, idx.pac, len(q), q.ctypes.data, None)
        out = rg.LiveRegs._grab(v.a, v.n) if v.n else []
        self.libc.free(v.a)
        for x in out:
            x["mapq"] = 0
        return out

    def _vec(self, regs, room=0):
        n = len(regs)
        mem = self.libc.malloc(max(n + room, 1) * ctypes.sizeof(rg._AlnReg))
        arr = ctypes.cast(mem, ctypes.POINTER(rg._AlnReg))
        ctypes.memset(mem, 0, max(n + room, 1) * ctypes.sizeof(rg._AlnReg))
        for i, x in enumerate(regs):
            for f in rg._LIVE_FIELDS:
                setattr(arr[i], f, x[f])
        return rg._AlnRegV(n, n, arr)

    def pestat(self, o, lists):
        n = len(lists)
        vs = (rg._AlnRegV * max(n, 1))(*[self._vec(x) for x in lists])
        pes = (_Pes * 4)()
        with _Quiet(2):
            self.live.lib.mem_pestat(self.opt(o), self.live.l_pac, n, vs, pes)
        for v in vs[:n]:
            self.libc.free(v.a)
        return [dict(low=p.low, high=p.high, failed=p.failed, avg=p.avg, std=p.std) for p in pes]

    def rescue(self, o, pes, reads, lists):
        """mem_sam_pe's rescue loop over live mem_matesw."""
        L, idx = self.live.lib, self.live.idx
        cp = (_Pes * 4)(*[_Pes(p["low"], p["high"], p["failed"], p["avg"], p["std"]) for p in pes])
        a = [self._vec(lists[0]), self._vec(lists[1])]
        b = [[x for x in lists[i] if x["score"] >= lists[i][0]["score"] - o["pen_unpaired"]] for i in range(2)]
        n = 0
        qs = [np.ascontiguousarray(r, np.uint8).copy() for r in reads]
        for i in range(2):
            for j in range(min(len(b[i]), o["max_matesw"])):
                anchor = self._vec([b[i][j]])
                n += L.mem_matesw(self.opt(o), idx.bns, idx.pac, cp, anchor.a, len(qs[1 - i]), qs[1 - i].ctypes.data,
                                  ctypes.byref(a[1 - i]))
                self.libc.free(anchor.a)
        out = []
        for v in a:
            g = rg.LiveRegs._grab(v.a, v.n)
            for x in g:
                x["mapq"] = 0
            out.append(g)
            self.libc.free(v.a)
        return out, n


# ---- inputs ------------------------------------------------------------------------------------------

def no_seed(rng, seq, k):
    """A substitution every k bases or closer: no exact match of k bases is left."""
    seq = seq.copy()
    p = int(rng.integers(0, k))
    while p < len(seq):
        seq[p] = (seq[p] + rng.integers(1, 4)) % 4
        p += int(rng.integers(max(k - 6, 2), k))
    return seq


def make_aligned(cx, n, seed):
    """Pairs of reads (read1, read2): codes 0..4. Mostly FR around a mean insert of 300."""
    rng = np.random.default_rng(seed)
    l, ce = cx.l_pac, [0] + cx.contig_end
    pairs = []
    while len(pairs) < n:
        c = int(rng.choice([0, 0, 2, 2, 2, 1]))
        lo, hi = ce[c], ce[c + 1]
        ins = int(rng.normal(300, 25))
        l1, l2 = int(rng.choice([50, 101, 151, 250])), int(rng.choice(MATE_LENS[1:] + (101, 151, 151, 30)))
        if ins < max(l1, l2) + 5:
            continue
        p = int(rng.integers(lo, hi - ins))
        frag = cx.codes[p:p + ins]
        u = rng.random()
        d = 1 if u < 0.94 else int(rng.choice([0, 2, 3]))
        # read 1 starts the fragment; read 2 ends it. FR: read 2 reverse-complemented
        r1, r2 = frag[:l1].copy(), frag[ins - l2:].copy()
        if d == 1:
            r2 = mk._rc(r2)
        elif d == 2:
            r1, r2 = mk._rc(frag[ins - l1:]), frag[:l2].copy()
        elif d == 3:
            r1, r2 = mk._rc(frag[ins - l1:]), mk._rc(frag[:l2])
        if rng.random() < 0.5:  # the whole fragment from the other strand
            r1, r2 = (mk._rc(r2), mk._rc(r1)) if d in (0, 3) else (r1, r2)
        kind = rng.choice(["clean", "clean", "noseed", "noseed", "elsewhere", "chimera", "chimera", "n"])
        which = int(rng.integers(0, 2))
        m = [r1, r2][which]
        if kind == "noseed":
            m = no_seed(rng, m, 17)
        elif kind == "elsewhere":
            q = int(rng.integers(0, l - len(m)))
            m = cx.codes[q:q + len(m)].copy()
        elif kind == "chimera" and len(m) >= 100:
            cut = int(rng.integers(35, len(m) - 35))
            q = int(rng.integers(0, l - len(m)))
            other = cx.codes[q:q + len(m)].copy()
            m = np.concatenate([no_seed(rng, m[:cut], 17), other[cut:]]) if rng.random() < 0.5 else \
                np.concatenate([other[:cut], no_seed(rng, m[cut:], 17)])
        elif kind == "n":
            m = no_seed(rng, m, 17)
            m[rng.integers(0, len(m), 3)] = 4
        if which == 0:
            r1 = m
        else:
            r2 = m
        pairs.append((r1.astype(np.uint8), r2.astype(np.uint8)))
    return pairs


def rid_of(cx, rb):
    return cx.clip(rb)[0]


def make_constructed(cx, o, pes, n, seed):
    """Hand-made pairs for the pes given: (reads, lists). The anchor read's regions are made by hand around
    real sequence; the mate is real sequence placed relative to the anchor; the mate's list is made around
    what a first pass with an empty list finds."""
    rng = np.random.default_rng(seed)
    l, ce = cx.l_pac, [0] + cx.contig_end
    edges = sorted(set(ce + [2 * l - x for x in ce]))
    out = []

    def reg(rb, re, qb, qe, score, **kw):
        return rg.new_reg(rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), rid=rid_of(cx, int(rb)), score=int(score),
                          truesc=int(score), seedcov=max(int(qe - qb) >> 1, 1), seedlen0=19, w=100, n_comp=1, **kw)

    open_r = [r for r in range(4) if not pes[r]["failed"]]
    tiny_w, tiny_k = (o["min_seed_len"], 15, 16, 17, 255, 256, 257), 0
    while len(out) < n:
        r = int(rng.choice(open_r))
        is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
        low, high = pes[r]["low"], pes[r]["high"]
        la = int(rng.choice([40, 101, 151]))
        l_ms = int(rng.choice(MATE_LENS + (101, 151, 151, 151, 40)))
        # the anchor's place in the doubled space: anywhere, or near an edge (contig ends, 0, 2 l_pac, l_pac)
        u = rng.random()
        tiny = None
        if u < (0.3 if o["min_seed_len"] < 15 else 0.1) and (0 in open_r or 3 in open_r):
            # a window of a chosen length, cut by the clamp at 2 l_pac (FF) or at 0 (RR)
            r = int(rng.choice([x for x in (0, 3) if x in open_r]))
            is_rev, is_larger, la = False, r == 0, 40
            low, high = pes[r]["low"], pes[r]["high"]
            tiny = int(tiny_w[tiny_k % len(tiny_w)])
            arb = 2 * l - low - tiny if r == 0 else tiny + low - l_ms
            if arb < 0 or arb + la > 2 * l:
                continue
        elif u < 0.45:
            arb = int(rng.integers(0, 2 * l - la))
        else:
            e = int(rng.choice(edges))
            off = int(rng.choice([low, high, high + l_ms, low + l_ms, (low + high) // 2, 30, high + 300]))
            arb = e + int(rng.choice([-1, 1])) * off + int(rng.integers(-20, 21))
        arb = min(max(arb, 0), 2 * l - la)
        if arb < l < arb + la or cx.clip(arb)[0] != cx.clip(arb + la - 1)[0]:
            continue
        anchor = reg(arb, arb + la, 0, la, la * o["a"])
        read_a = cx.fetch(arb, arb + la)
        # where the mate comes from, as a distance (mem_infer_dir's) from the anchor
        v = rng.random()
        if v < 0.35:
            dist = int(rng.integers(low, high + 1))
        elif v < 0.6:
            dist = int(rng.choice([low, high, low + 1, high - 1]))
        elif v < 0.75:
            dist = int(rng.choice([low - int(rng.integers(1, 40)), high + int(rng.integers(1, 40))]))
        else:
            dist = None  # no mate there
        if tiny is not None and tiny >= l_ms:  # somewhere inside the cut window
            dist = (2 * l - tiny + int(rng.integers(0, tiny - l_ms + 1)) - arb) if r == 0 else \
                arb - int(rng.integers(0, tiny - l_ms + 1))
        mate, tb = None, None
        if dist is not None and dist > 0:
            # the mate's first base on the anchor's strand: a mate on the other strand has its rb mirrored, and
            # the distance is taken from its last base there
            p2 = arb + dist if is_larger else arb - dist
            tb = p2 - (l_ms - 1) if is_rev else p2
            if tb >= 0 and tb + l_ms <= 2 * l and not (tb < l < tb + l_ms):
                seq = cx.fetch(tb, tb + l_ms)
                mate = mk._rc(seq) if is_rev else seq
        if mate is None:
            q = int(rng.integers(0, l - l_ms))
            mate = cx.codes[q:q + l_ms].copy() if rng.random() < 0.5 else rng.integers(0, 4, l_ms).astype(np.uint8)
        mut = rng.random()
        if mut < 0.3:
            mate = no_seed(rng, mate, int(rng.choice([8, 12, 17, 30])))
        elif mut < 0.4 and l_ms > 60:  # an insertion or a deletion in the mate
            k, m = int(rng.integers(20, l_ms - 20)), int(rng.integers(1, 8))
            mate = np.concatenate([mate[:k], rng.integers(0, 4, m).astype(np.uint8), mate[k:]])[:l_ms] \
                if rng.random() < 0.5 else np.concatenate([mate[:k], mate[k + m:], mate[:m]])[:l_ms]
        if rng.random() < 0.08:
            mate = mate.copy()
            mate[rng.integers(0, l_ms, int(rng.integers(1, 4)))] = 4
        mate = np.asarray(mate, np.uint8)
        # the anchor read's other regions: close in score or not, at the same place shifted or elsewhere
        la_list = [anchor]
        for _ in range(int(rng.choice([0, 0, 1, 1, 2, 3]))):
            sc = anchor["score"] - int(rng.choice([0, 1, 5, 16, 17, 18, 30]))
            if sc < 1:
                continue
            if rng.random() < 0.5:
                sh = int(rng.integers(-3, 4))
                nb = min(max(arb + sh, 0), 2 * l - la)
            else:
                nb = int(rng.integers(0, 2 * l - la))
            if nb < l < nb + la or cx.clip(nb)[0] != cx.clip(nb + la - 1)[0]:
                continue
            la_list.append(reg(nb, nb + la, 0, la, sc))
        la_list.sort(key=lambda x: -x["score"])
        # first pass: what the rescue finds with an empty mate list
        first, _, _ = py_rescue(o, cx, pes, [read_a, mate], [la_list, []], set())
        found = first[1]
        ma = []
        w = rng.random()
        if found and w < 0.7:
            f = found[0]
            kinds = rng.choice(["above", "below", "equal", "both", "redun_lo", "redun_hi", "two_equal"])
            far = lambda: int(rng.integers(0, l - l_ms))  # noqa: E731

            def elsewhere(score):
                while True:
                    nb = far() + (l if rng.random() < 0.5 else 0)
                    nb = min(nb, 2 * l - l_ms)
                    if not (nb < l < nb + l_ms) and cx.clip(nb)[0] == cx.clip(nb + l_ms - 1)[0]:
                        if not any(pes[d]["low"] <= infer_dir(l, x["rb"], nb)[1] <= pes[d]["high"]
                                   for x in la_list for d in [infer_dir(l, x["rb"], nb)[0]]):
                            return reg(nb, nb + l_ms, 0, l_ms, score)
            if kinds in ("above", "both"):
                ma.append(elsewhere(f["score"] + int(rng.integers(1, 9))))
            if kinds in ("equal", "two_equal"):
                ma.append(elsewhere(f["score"]))
            if kinds == "two_equal":
                ma.append(elsewhere(f["score"]))
            if kinds in ("below", "both") and f["score"] > 3:
                ma.append(elsewhere(f["score"] - int(rng.integers(1, 3))))
            if kinds in ("redun_lo", "redun_hi") and f["qe"] - f["qb"] > 30:
                # almost the region the rescue will find, a few bases shorter at its start: redundant with it, and
                # out of [low, high] only when the mate sits at the edge
                sh = int(rng.integers(1, 4))
                sc = f["score"] + (-sh if kinds == "redun_lo" else sh)
                ma.append(dict(reg(f["rb"] + sh, f["re"], f["qb"] + sh, f["qe"], max(sc, 1)), rid=f["rid"]))
            ma.sort(key=lambda x: -x["score"])
        elif w < 0.85:
            for _ in range(int(rng.integers(1, 4))):
                nb = int(rng.integers(0, 2 * l - l_ms))
                if nb < l < nb + l_ms or cx.clip(nb)[0] != cx.clip(nb + l_ms - 1)[0]:
                    continue
                ma.append(reg(nb, nb + l_ms, 0, l_ms, int(rng.integers(19, max(l_ms * o["a"], 19) + 2))))
            ma.sort(key=lambda x: -x["score"])
        pair = ([read_a, mate], [la_list, ma])
        tiny_k += tiny is not None
        if rng.random() < 0.5:  # the anchor as read 2
            pair = (pair[0][::-1], pair[1][::-1])
        out.append(pair)
    return out


def make_pestat_case(rng, l_pac, contig_end, kind, n):
    """A synthetic set of stage-0 lists for mem_pestat alone: only rb, qb, qe, score and rid matter."""
    lists = []
    mix = rng.dirichlet([1, 6, 1, 1])
    if kind == "fr_only":
        mix = np.array([0.01, 0.97, 0.01, 0.01])
    elif kind == "ratio":  # a few more than MIN_DIR_CNT, below MIN_DIR_RATIO of the largest
        mix = np.array([0.04, 0.88, 0.04, 0.04])
    mu, sd = (60, 40) if kind == "small" else (int(rng.integers(200, 600)), int(rng.integers(10, 60)))
    for _ in range(n):
        def one(rb, score=100, qb=0, qe=100):
            pos_f = rb if rb < l_pac else 2 * l_pac - 1 - rb
            rid = int(np.searchsorted(contig_end, pos_f, side="right"))
            return rg.new_reg(rb=int(rb), re=int(rb) + 100, qb=qb, qe=qe, score=score, rid=rid, seedcov=50)
        d = int(rng.choice(4, p=mix))
        if kind == "tails" and rng.random() < 0.6:
            dist = int(rng.normal(mu, 3))
        elif kind == "tails":
            dist = int(mu + rng.choice([-1, 1]) * rng.integers(8, 14))
        else:
            dist = int(rng.normal(mu, sd))
        u = rng.random()
        if u < 0.03:
            dist = 0
        elif u < 0.06:
            dist = 10001 + int(rng.integers(0, 500))
        b1 = int(rng.integers(12000, l_pac - 12000))
        # choose b2 so that mem_infer_dir gives (d, dist)
        larger = d in (0, 1)
        other = (d in (1, 2))
        p2 = b1 + dist if larger else b1 - dist
        b2 = 2 * l_pac - 1 - p2 if other else p2
        a0, a1 = [one(b1)], [one(b2)]
        v = rng.random()
        if v < 0.05:
            a0 = []
        elif v < 0.10:
            a1.append(one(int(rng.integers(0, l_pac)), score=95, qb=5, qe=100))  # a close second over the same query
        elif v < 0.14:
            a1.append(one(int(rng.integers(0, l_pac)), score=60, qb=50, qe=100))  # half of it: counts at 0.5, score low
        elif v < 0.18:
            a0[0] = one(int(rng.integers(0, contig_end[0] - 200)))
            a1[0] = one(int(contig_end[1] + rng.integers(0, 1000)))
        lists.append(a0), lists.append(a1)
    return lists


# ---- packing -----------------------------------------------------------------------------------------

def pack_lists(lists):
    out = {"n": np.array([len(x) for x in lists], np.int32)}
    flat = [g for x in lists for g in x]
    for f in FIELDS:  # l_pac is small: rb fits 32 bits, and re is stored as the length
        t = np.float32 if f == "frac_rep" else np.int32
        out[f] = np.array([(g["re"] - g["rb"]) if f == "re" else g[f] for g in flat], t)
    return out


def same(x, y):
    return len(x) == len(y) and all(all((np.float32(a[f]) == np.float32(b[f])) if f == "frac_rep" else a[f] == b[f]
                                        for f in FIELDS) for a, b in zip(x, y))


def pes_array(pes):
    return np.array([[p["low"], p["high"], p["failed"]] for p in pes], np.int32), \
        np.array([[p["avg"], p["std"]] for p in pes], np.float64)


def main():
    if not mk.available():
        print("skipped: needs %s and oracle/_ref/libref_bwa.so (make ref)" % mk.REF_TREE)
        return 0
    scale = float(os.environ.get("GB_MATESW_SCALE", "1"))
    contigs, _ = mk.make_reference()
    live = mk.LiveBwa(contigs)
    try:
        lp = LivePair(live)
        cx = Ctx(live.codes, live.contig_end, lp.ksw)
        l_pac = live.l_pac
        fx = {}
        counts = np.zeros((len(GROUPS) + 1, len(LABELS)), np.int32)
        windows, mate_lens, n_pairs_all, n_dp_pairs, n_gain_pairs, max_rounds = set(), set(), 0, 0, 0, 0
        sets = {}
        for gi, (g, (kw, source, gp)) in enumerate(GROUPS.items()):
            o = opts(**kw)
            if source == "aligned":
                reads2 = make_aligned(cx, int(420 * scale), seed=101)
                pairs = [([r1, r2], [lp.stage0(o, r1), lp.stage0(o, r2)]) for r1, r2 in reads2]
            elif source == "wide":
                reads2 = make_aligned(cx, 10, seed=303)
                pairs = [([r1, r2], [lp.stage0(o, r1), lp.stage0(o, r2)]) for r1, r2 in reads2]
            else:
                pes0 = [dict(low=a, high=b, failed=c, avg=0.0, std=0.0) for a, b, c in gp]
                if g == "open":
                    pairs = make_constructed(cx, o, pes0, int(620 * scale), seed=202)
                else:
                    pairs = make_constructed(cx, o, pes0, int(85 * scale), seed=400 + gi)
            all_lists = [x for _, ls in pairs for x in ls]
            pflags = []
            live_pes = lp.pestat(o, all_lists)
            my_pes = py_pestat(o, l_pac, all_lists, pflags)
            assert live_pes == my_pes, "group %s: the restatement's mem_pestat differs: %s vs %s" % (g, live_pes, my_pes)
            for f in pflags:
                counts[gi, LABELS.index(f)] += 1
            pes = live_pes if gp == "live" else [dict(low=a, high=b, failed=c, avg=0.0, std=0.0) for a, b, c in gp]
            outs, n_sws = [], []
            for k, (reads, lists) in enumerate(pairs):
                flags = set()
                mine, n_mine, rounds = py_rescue(o, cx, pes, reads, lists, flags)
                theirs, n_live = lp.rescue(o, pes, reads, lists)
                assert n_mine == n_live, "group %s pair %d: n differs (%d, live %d)" % (g, k, n_mine, n_live)
                for i in range(2):
                    assert same(mine[i], theirs[i]), "group %s pair %d read %d: the restatement differs" % (g, k, i)
                windows |= {int(f[4:]) for f in flags if f.startswith("win_")}
                mate_lens |= {int(f[5:]) for f in flags if f.startswith("mlen_")}
                for f in flags:
                    if not f.startswith(("win_", "mlen_")):
                        counts[gi, LABELS.index(f)] += 1
                n_pairs_all += 1
                n_dp_pairs += n_live > 0
                # a region gained: one in a final list that was not in the list given
                place = lambda x: (x["rb"], x["re"], x["qb"], x["qe"])  # noqa: E731
                n_gain_pairs += any(place(x) not in {place(y) for y in lists[i]} for i in range(2) for x in theirs[i])
                max_rounds = max(max_rounds, rounds)
                outs.extend(theirs), n_sws.append(n_live)
            reads_flat = [r for rs, _ in pairs for r in rs]
            fx[g + "_qbuf"] = np.concatenate(reads_flat).astype(np.uint8)
            fx[g + "_lens"] = np.array([len(r) for r in reads_flat], np.int32)
            for k, v in pack_lists(all_lists).items():
                fx["%s_in_%s" % (g, k)] = v
            for k, v in pack_lists(outs).items():
                fx["%s_out_%s" % (g, k)] = v
            fx[g + "_n_sw"] = np.array(n_sws, np.int32)
            fx[g + "_pes_i"], fx[g + "_pes_d"] = pes_array(pes)
            fx[g + "_pestat_i"], fx[g + "_pestat_d"] = pes_array(live_pes)
            sets[g] = (len(pairs), sum(map(len, all_lists)), sum(map(len, outs)), sum(n_sws))
            print("group %-18s %4d pairs, %5d regions in, %5d out, %5d alignments" % ((g,) + sets[g]))
        # mem_pestat alone, on synthetic lists
        rng = np.random.default_rng(77)
        kinds = ["normal", "normal", "fr_only", "small", "small", "tails", "tails", "tails", "tails", "tails", "ratio",
                 "ratio", "ratio"]
        gi = len(GROUPS)
        for c, kind in enumerate(kinds):
            lists = make_pestat_case(rng, l_pac, live.contig_end, kind, 400 if kind == "ratio" else int(rng.integers(150, 400)))
            o = opts()
            pflags = []
            live_pes = lp.pestat(o, lists)
            assert live_pes == py_pestat(o, l_pac, lists, pflags), "pestat case %d: the restatement differs" % c
            for f in pflags:
                counts[gi, LABELS.index(f)] += 1
            flat = [x for ls in lists for x in ls]
            fx["ps%d_n" % c] = np.array([len(x) for x in lists], np.int8)
            for f in ("rb", "qb", "qe", "score", "rid"):
                fx["ps%d_%s" % (c, f)] = np.array([x[f] for x in flat], np.int32)
            fx["ps%d_pestat_i" % c], fx["ps%d_pestat_d" % c] = pes_array(live_pes)
            print("pestat case %2d %-8s %s" % (c, kind, [(p["low"], p["high"], p["failed"]) for p in live_pes]))
        fx["n_pestat_cases"] = np.int32(len(kinds))
        fx["label_counts"], fx["label_names"], fx["label_min"] = counts, np.array(LABELS), np.int32(LABEL_MIN)
        fx["group_names"] = np.array(list(GROUPS))
        fx["opt_names"] = np.array(list(DEFAULTS))
        fx["group_opts"] = np.array([[float(opts(**kw)[k]) for k in DEFAULTS] for kw, _, _ in GROUPS.values()], np.float64)
        fx["windows"] = np.array(sorted(windows), np.int32)
        fx["mate_lens_ran"] = np.array(sorted(mate_lens), np.int32)  # the mates' lengths of the alignments that ran
        fx["conditions"] = np.array([n_pairs_all, n_dp_pairs, n_gain_pairs, max_rounds], np.int32)
        total = counts.sum(0)
        for k, name in enumerate(LABELS):
            print("label %-24s %5d" % (name, int(total[k])))
        print("pairs %d, with a DP %d, with a region gained %d, most rounds %d" % (n_pairs_all, n_dp_pairs, n_gain_pairs,
                                                                                 max_rounds))
        print("windows:", [w for w in sorted(windows) if w < 20 or w in (255, 256, 257) or w > 15000][:40])
        short = [LABELS[k] for k in range(len(LABELS)) if total[k] < LABEL_MIN]
        if os.environ.get("GB_MATESW_DRAFT") != "1":
            assert not short, "labels below %d: %s" % (LABEL_MIN, short)
            assert 3 * n_dp_pairs >= n_pairs_all and 10 * n_gain_pairs >= n_pairs_all and max_rounds >= 3
            # the windows that ran: min_seed_len, the fetch's 16-base chunks, the DP's 256 rows per register, and one
            # near the bound of GB_BSW_LOCAL_MAX_TLEN
            assert {10, 15, 16, 17, 19, 255, 256, 257} <= windows and max(windows) > 16000, sorted(windows)[:12]
            assert set(MATE_LENS) <= mate_lens, sorted(mate_lens)  # the DP's columns-per-lane steps
        else:
            print("short:", short)
        np.savez_compressed(OUT, **fx)
        print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    finally:
        live.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
