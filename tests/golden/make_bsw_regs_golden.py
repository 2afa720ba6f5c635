#!/usr/bin/env python3
"""Generates tests/golden/bsw_regs_golden.npz: from a read's regions to its primaries, recorded from bwa
v1's own mem_sort_dedup_patch, mem_mark_primary_se, mem_reorder_primary5 and mem_approx_mapq_se
(tools/bwa/bwamem.c:406-558, 993-1041) run live through ctypes.

Build container only: needs /root/reference and oracle/_ref/libref_bwa.so (make ref). The live library is
LiveBwa of make_bsw_mkchain_golden.py (the reference's bwa sources compiled in a temporary directory
outside the repository, removed at the end) over the same synthetic reference, make_reference(): the
reference itself is therefore not stored again, tests take it from bsw_mkchain_golden.npz. Nothing compiled
from the reference and none of its text goes into the repository: only recorded inputs and outputs do.

Two sources of reads:
  aligned      reads drawn from the reference (make_reads). Their regions come from live mem_chain2aln over
               the live, filtered chains, and the expected final state is cross-checked against live
               mem_align1_core (+ mem_mark_primary_se).
  constructed  region sets written by hand (make_constructed): short reads rarely reach mem_patch_reg's
               branches by themselves. A true co-linear alignment is cut into 2 to 4 pieces with gaps or
               overlaps of a few bases; near-copies make redundant pairs; pieces with a shifted diagonal,
               with a garbage middle, on both strands, out of order, on ALT and primary contigs; random
               region sets of 2 to 48 regions for the sort ties.
Every read is also run through a restatement of the contract in Python (py_dedup, py_mark, py_mapq), which
must reproduce the live result in every field and which counts the labels: a label's minimum is asserted
here and again by the test on the stored counts.

The helpers (make_constructed, LiveRegs, py_*) are also used by tests/test_bsw_regs.py.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_bsw_mkchain_golden as mk  # noqa: E402

OUT = os.path.join(HERE, "bsw_regs_golden.npz")
MAX_LEN = 250
INT_MAX = 2 ** 31 - 1

DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100, max_chain_gap=10000, min_seed_len=19,
                mask_level=0.5, mask_level_redun=0.95, mapQ_coef_len=50.0, mapQ_coef_fac=3, T=30, primary5=0)
# group -> (option overrides, id0)
GROUPS = {"default": ({}, 0), "w": (dict(w=4), 0), "max_chain_gap": (dict(max_chain_gap=50), 0),
          "mask_level_redun": (dict(mask_level_redun=0.5), 0), "mask_level": (dict(mask_level=0.9), 0),
          "mapQ_coef_len": (dict(mapQ_coef_len=0.0), 0), "ab": (dict(a=2, b=8), 0), "primary5": (dict(primary5=1), 0),
          "id0": ({}, 10 ** 9 + 7)}
IN_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "sub", "csub", "sub_n",
             "frac_rep")
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov",
          "secondary", "secondary_all", "seedlen0", "n_comp", "is_alt", "frac_rep", "mapq", "hash")
LABELS = ("n0", "n1", "n2", "n3", "n16", "n17", "n40p", "re_tie", "redun_p", "redun_q", "redun_eq", "exit_strand",
          "exit_colinear", "exit_noovlp", "exit_ovlp", "ovlp_strict_refuse", "exit_ratio", "merged", "aln1", "aln2",
          "aln3p", "merge_rev", "identical", "npri_all", "npri_some", "npri_none", "sub_set", "sub_n_both", "alt_sc",
          "sec_intmax", "hash_tie", "p5_swap", "mapq_sub_ge", "mapq_l_lt", "mapq_l_ge", "mapq_coef0_ident", "mapq_sub_n",
          "mapq_clamp", "mapq_frac_rep", "mapq_csub")
LABEL_MIN = 5
S0_ZERO = ("secondary", "secondary_all", "alt_sc", "hash", "mapq")   # what stage 0 leaves as given
S1_FIELDS = ("sub", "alt_sc", "sub_n", "secondary", "secondary_all", "mapq")  # what stage 1 changes, with hash


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def new_reg(**kw):
    d = {f: 0 for f in FIELDS}
    d["frac_rep"] = 0.0
    d.update(kw)
    return d


# ---- the contract restated in Python -------------------------------------------------------------

F32 = np.float32


def hash_64(key):
    m = (1 << 64) - 1
    key &= m
    key = (key + (~(key << 32) & m)) & m
    key ^= key >> 22
    key = (key + (~(key << 13) & m)) & m
    key ^= key >> 8
    key = (key + (key << 3)) & m
    key ^= key >> 15
    key = (key + (~(key << 27) & m)) & m
    key ^= key >> 31
    return key


def py_patch_pre(o, l_pac, a, b, flags):
    """mem_patch_reg up to the alignment: the w to align with, or None."""
    if a["rb"] < l_pac and b["rb"] >= l_pac:
        flags.add("exit_strand")
        return None
    if a["qb"] >= b["qb"] or a["qe"] >= b["qe"] or a["re"] >= b["re"]:
        flags.add("exit_colinear")
        return None
    w = abs((a["re"] - b["rb"]) - (a["qe"] - b["qb"]))
    r = abs((a["re"] - b["rb"]) / (b["re"] - a["rb"]) - (a["qe"] - b["qb"]) / (b["qe"] - a["qb"]))
    strict = w > o["w"] << 1 or r >= float(F32(0.05))
    if a["re"] < b["rb"] or a["qe"] < b["qb"]:
        if strict:
            flags.add("exit_noovlp")
            return None
    else:
        if w > o["w"] << 2 or r >= float(F32(0.05) * F32(2)):
            flags.add("exit_ovlp")
            return None
        if strict:
            flags.add("ovlp_strict_refuse")
    w += a["w"] + b["w"]
    return min(w, o["w"] << 2)


def py_patch_post(a, b, score, flags):
    q_s = int((b["qe"] - a["qb"]) / ((b["qe"] - b["qb"]) + (a["qe"] - a["qb"])) * (b["score"] + a["score"]) + .499)
    r_s = int((b["re"] - a["rb"]) / ((b["re"] - b["rb"]) + (a["re"] - a["rb"])) * (b["score"] + a["score"]) + .499)
    if score / max(q_s, r_s) < float(F32(0.90)):
        flags.add("exit_ratio")
        return 0
    return score


def py_dedup(o, l_pac, is_alt, regs, align, flags):
    """mem_sort_dedup_patch and the is_alt step on a list of region dicts (changed in place); align(rb, re,
    qb, qe, w) is the alignment's score. Returns (the regions left, the number of alignments)."""
    a, n, n_aln = regs, len(regs), 0
    if n > 1:
        if len(set(x["re"] for x in a)) < n:
            flags.add("re_tie")
        mk.py_introsort(a, lambda x, y: x["re"] < y["re"])
        for x in a:
            x["n_comp"] = 1
        mlr = F32(o["mask_level_redun"])
        for i in range(1, n):
            p = a[i]
            if p["rid"] != a[i - 1]["rid"] or p["rb"] >= a[i - 1]["re"] + o["max_chain_gap"]:
                continue
            j = i
            while True:
                j -= 1
                if not (j >= 0 and p["rid"] == a[j]["rid"] and p["rb"] < a[j]["re"] + o["max_chain_gap"]):
                    break
                q = a[j]
                if q["qe"] == q["qb"]:
                    continue
                orr = q["re"] - p["rb"]
                oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
                mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
                mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
                if F32(orr) > mlr * F32(mr) and F32(oq) > mlr * F32(mq):
                    if p["score"] < q["score"]:
                        flags.add("redun_p")
                        p["qe"] = p["qb"]
                        break
                    flags.add("redun_eq" if p["score"] == q["score"] else "redun_q")
                    q["qe"] = q["qb"]
                elif q["rb"] < p["rb"]:
                    w = py_patch_pre(o, l_pac, q, p, flags)
                    if w is None:
                        continue
                    n_aln += 1
                    score = py_patch_post(q, p, align(q["rb"], p["re"], q["qb"], p["qe"], w), flags)
                    if score > 0:
                        flags.add("merged")
                        if p["rb"] >= l_pac:
                            flags.add("merge_rev")
                        p["n_comp"] += q["n_comp"] + 1
                        for f in ("seedcov", "sub", "csub"):
                            p[f] = max(p[f], q[f])
                        p["qb"], p["rb"] = q["qb"], q["rb"]
                        p["truesc"] = p["score"] = score
                        p["w"] = w
                        q["qb"] = q["qe"]
        a = [x for x in a if x["qe"] > x["qb"]]
        mk.py_introsort(a, lambda x, y: x["score"] > y["score"] or (x["score"] == y["score"] and (
            x["rb"] < y["rb"] or (x["rb"] == y["rb"] and x["qb"] < y["qb"]))))
        for i in range(1, len(a)):
            if all(a[i][f] == a[i - 1][f] for f in ("score", "rb", "qb")):
                a[i]["qe"] = a[i]["qb"]
                flags.add("identical")
        a = a[:1] + [x for x in a[1:] if x["qe"] > x["qb"]]
    for x in a:
        if is_alt[x["rid"]]:
            x["is_alt"] = 1
    if n_aln:
        flags.add("aln1" if n_aln == 1 else "aln2" if n_aln == 2 else "aln3p")
    return a, n_aln


def _py_core(o, a, first_pass_hits, flags):
    tmp = max(o["a"] + o["b"], o["o_del"] + o["e_del"], o["o_ins"] + o["e_ins"])
    z = [0]
    ml = F32(o["mask_level"])
    for i in range(1, len(a)):
        for j in z:
            b_max, e_min = max(a[j]["qb"], a[i]["qb"]), min(a[j]["qe"], a[i]["qe"])
            if e_min > b_max:
                min_l = min(a[i]["qe"] - a[i]["qb"], a[j]["qe"] - a[j]["qb"])
                if F32(e_min - b_max) >= F32(min_l) * ml:
                    if a[j]["sub"] == 0:
                        a[j]["sub"] = a[i]["score"]
                        flags.add("sub_set")
                    if a[j]["score"] - a[i]["score"] <= tmp and (a[j]["is_alt"] or not a[i]["is_alt"]):
                        a[j]["sub_n"] += 1
                        if first_pass_hits is not None and id(a[j]) in first_pass_hits:
                            flags.add("sub_n_both")
                        elif first_pass_hits is None:
                            a[j]["_hit"] = True
                    a[i]["secondary"] = j
                    break
        else:
            z.append(i)


def py_mark(o, a, idv, flags):
    """mem_mark_primary_se and mem_reorder_primary5 (o["primary5"]) on a list of region dicts, in place."""
    n = len(a)
    if n == 0:
        return
    for i, x in enumerate(a):
        x["sub"] = x["alt_sc"] = 0
        x["secondary"] = x["secondary_all"] = -1
        x["hash"] = hash_64(idv + i)
        x.pop("_hit", None)
    n_pri = sum(1 for x in a if not x["is_alt"])
    flags.add("npri_all" if n_pri == n else "npri_none" if n_pri == 0 else "npri_some")
    mk.py_introsort(a, lambda x, y: x["score"] > y["score"] or (x["score"] == y["score"] and (
        x["is_alt"] < y["is_alt"] or (x["is_alt"] == y["is_alt"] and x["hash"] < y["hash"]))))
    _py_core(o, a, None, flags)
    for i, p in enumerate(a):
        p["secondary_all"] = i
        if not p["is_alt"] and p["secondary"] >= 0 and a[p["secondary"]]["is_alt"]:
            p["alt_sc"] = a[p["secondary"]]["score"]
            flags.add("alt_sc")
    if n_pri < n:
        if n_pri > 0:
            mk.py_introsort(a, lambda x, y: x["is_alt"] < y["is_alt"] or (x["is_alt"] == y["is_alt"] and (
                x["score"] > y["score"] or (x["score"] == y["score"] and x["hash"] < y["hash"]))))
        z = [0] * n
        for i, x in enumerate(a):
            z[x["secondary_all"]] = i
        for x in a:
            if x["secondary"] >= 0:
                x["secondary_all"] = z[x["secondary"]]
                if x["is_alt"]:
                    x["secondary"] = INT_MAX
                    flags.add("sec_intmax")
            else:
                x["secondary_all"] = -1
        if n_pri > 0:
            hits = set(id(x) for x in a if x.get("_hit"))
            for x in a[:n_pri]:
                x["sub"], x["secondary"] = 0, -1
            _py_core(o, a[:n_pri], hits, flags)
    else:
        for x in a:
            x["secondary_all"] = x["secondary"]
    for x in a:
        x.pop("_hit", None)
    if not o["primary5"]:
        return
    ok = lambda p: p["secondary"] < 0 and not p["is_alt"] and p["score"] >= o["T"]
    if sum(1 for p in a if ok(p)) <= 1:
        return
    left_st, left_k = INT_MAX, -1
    for k, p in enumerate(a):
        if ok(p) and p["qb"] < left_st:
            left_st, left_k = p["qb"], k
    if left_k == 0:
        return
    flags.add("p5_swap")
    a[0], a[left_k] = a[left_k], a[0]
    for p in a[1:]:
        for f in ("secondary", "secondary_all"):
            if p[f] == 0:
                p[f] = left_k
            elif p[f] == left_k:
                p[f] = 0


def py_mapq(o, a, flags):
    """mem_approx_mapq_se."""
    from math import log
    sub = a["sub"] if a["sub"] else o["min_seed_len"] * o["a"]
    if a["csub"] > sub:
        sub = a["csub"]
        flags.add("mapq_csub")
    if sub >= a["score"]:
        flags.add("mapq_sub_ge")
        return 0
    l = max(a["qe"] - a["qb"], a["re"] - a["rb"])
    identity = 1. - (l * o["a"] - a["score"]) / (o["a"] + o["b"]) / l
    if F32(o["mapQ_coef_len"]) > 0:
        if F32(l) < F32(o["mapQ_coef_len"]):
            tmp = 1.
            flags.add("mapq_l_lt")
        else:
            tmp = o["mapQ_coef_fac"] / log(l)
            flags.add("mapq_l_ge")
        tmp *= identity * identity
        mapq = int(6.02 * (a["score"] - sub) / o["a"] * tmp * tmp + .499)
    else:
        mapq = int(30.0 * (1. - sub / a["score"]) * log(a["seedcov"]) + .499)
        if identity < 0.95:
            mapq = int(mapq * identity * identity + .499)
            flags.add("mapq_coef0_ident")
    if a["sub_n"] > 0:
        mapq -= int(4.343 * log(a["sub_n"] + 1) + .499)
        flags.add("mapq_sub_n")
    if mapq > 60:
        mapq = 60
        flags.add("mapq_clamp")
    mapq = max(mapq, 0)
    fr = float(F32(a["frac_rep"]))
    if fr > 0:
        flags.add("mapq_frac_rep")
    return int(mapq * (1. - fr) + .499)


def py_finish(o, l_pac, is_alt, regs, align, idv, flags):
    """(stage 0, stage 1, alignments) for one read's regions (dicts; not changed)."""
    s0, n_aln = py_dedup(o, l_pac, is_alt, [dict(x) for x in regs], align, flags)
    s0 = [dict(x, mapq=0) for x in s0]
    s1 = [dict(x) for x in s0]
    py_mark(o, s1, idv, flags)
    for x in s1:
        x["mapq"] = py_mapq(o, x, flags) if x["secondary"] < 0 else 0
    return s0, s1, n_aln


# ---- the live reference ----------------------------------------------------------------------------

class _AlnReg(ctypes.Structure):
    _fields_ = ([("rb", ctypes.c_int64), ("re", ctypes.c_int64)]
                + [(k, ctypes.c_int) for k in "qb qe rid score truesc sub alt_sc csub sub_n w seedcov secondary "
                                              "secondary_all seedlen0".split()]
                + [("n_comp", ctypes.c_int, 30), ("is_alt", ctypes.c_int, 2), ("frac_rep", ctypes.c_float),
                   ("hash", ctypes.c_uint64)])


class _AlnRegV(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("m", ctypes.c_size_t), ("a", ctypes.POINTER(_AlnReg))]


assert ctypes.sizeof(_AlnReg) == 88
_LIVE_FIELDS = tuple(f for f in FIELDS if f != "mapq")


class LiveRegs:
    """The reference's own functions over a LiveBwa index."""

    def __init__(self, live):
        self.live, L = live, live.lib
        vp, ci = ctypes.c_void_p, ctypes.c_int
        popt = ctypes.POINTER(mk._MemOpt)
        L.mem_sort_dedup_patch.argtypes = [popt, vp, vp, vp, ci, ctypes.POINTER(_AlnReg)]
        L.mem_mark_primary_se.argtypes = [popt, ci, ctypes.POINTER(_AlnReg), ctypes.c_int64]
        L.mem_reorder_primary5.argtypes = [ci, ctypes.POINTER(_AlnRegV)]
        L.mem_approx_mapq_se.argtypes = [popt, ctypes.POINTER(_AlnReg)]
        L.mem_chain2aln.argtypes = [popt, vp, vp, ci, vp, ctypes.POINTER(mk._MemChain), ctypes.POINTER(_AlnRegV)]
        L.mem_chain2aln.restype = None
        L.mem_align1_core.argtypes = [popt, vp, vp, vp, ci, vp, vp]
        L.mem_align1_core.restype = _AlnRegV
        L.bwa_gen_cigar2.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.c_int64, vp, ci, vp, ctypes.c_int64, ctypes.c_int64,
                                     vp, vp, vp]
        L.bwa_gen_cigar2.restype = vp
        L.bwa_fill_scmat.argtypes = [ci, ci, vp]
        self.bns_is_alt = live.is_alt

    def opt(self, o):
        kw = {k: v for k, v in o.items() if k != "primary5"}
        p = self.live._opt(kw)
        p.contents.flag = 0x800 if o["primary5"] else 0  # MEM_F_PRIMARY5
        self.live.lib.bwa_fill_scmat(o["a"], o["b"], ctypes.addressof(p.contents) + mk._MemOpt.mat.offset)
        return p

    def align(self, p, query):
        """The alignment callback of py_dedup on the live bwa_gen_cigar2."""
        o, L, idx = p.contents, self.live.lib, self.live.idx

        def f(rb, re, qb, qe, w):
            q = np.ascontiguousarray(query[qb:qe], np.uint8).copy()
            sc = ctypes.c_int(0)
            L.bwa_gen_cigar2(ctypes.addressof(o) + mk._MemOpt.mat.offset, o.o_del, o.e_del, o.o_ins, o.e_ins, w,
                             self.live.l_pac, idx.pac, len(q), q.ctypes.data, rb, re, ctypes.byref(sc), None, None)
            return sc.value
        return f

    @staticmethod
    def _grab(arr, n):
        return [{f: (float(getattr(arr[i], f)) if f == "frac_rep" else int(getattr(arr[i], f))) for f in _LIVE_FIELDS}
                for i in range(n)]

    def _stage1(self, p, arr, n, idv, primary5):
        L = self.live.lib
        L.mem_mark_primary_se(p, n, arr, idv)
        if primary5:
            v = _AlnRegV(n, n, arr)
            L.mem_reorder_primary5(p.contents.T, ctypes.byref(v))
        out = self._grab(arr, n)
        for i, x in enumerate(out):
            x["mapq"] = L.mem_approx_mapq_se(p, ctypes.byref(arr[i])) if x["secondary"] < 0 else 0
        return out

    def finish(self, o, query, regs, idv):
        """(stage 0, stage 1) of one read's regions from the live functions."""
        L, idx, p = self.live.lib, self.live.idx, self.opt(o)
        n = len(regs)
        arr = (_AlnReg * max(n, 1))()
        for i, x in enumerate(regs):
            for f in _LIVE_FIELDS:
                setattr(arr[i], f, x[f])
        q = np.ascontiguousarray(query, np.uint8).copy()
        n = L.mem_sort_dedup_patch(p, idx.bns, idx.pac, q.ctypes.data, n, arr)
        for i in range(n):
            if self.bns_is_alt[arr[i].rid]:
                arr[i].is_alt = 1
        s0 = [dict(x, mapq=0) for x in self._grab(arr, n)]
        s1 = self._stage1(p, arr, n, idv, o["primary5"])
        self.live.libc.free(p)
        return s0, s1

    def chain2aln(self, o, read):
        """The regions live mem_chain2aln pushes for one read over the live, filtered chains."""
        L, idx, p = self.live.lib, self.live.idx, self.opt(o)
        q = np.ascontiguousarray(read, np.uint8).copy()
        v = L.mem_chain(p, idx.bwt, idx.bns, len(q), q.ctypes.data, None)
        k = L.mem_chain_flt(p, v.n, v.a) if v.n else 0
        regs = _AlnRegV(0, 0, None)
        for i in range(k):
            L.mem_chain2aln(p, idx.bns, idx.pac, len(q), q.ctypes.data, ctypes.byref(v.a[i]), ctypes.byref(regs))
            self.live.libc.free(v.a[i].seeds)
        out = self._grab(regs.a, regs.n)
        self.live.libc.free(v.a)
        self.live.libc.free(regs.a)
        self.live.libc.free(p)
        return out

    def align1(self, o, read, idv):
        """Stage 1 from live mem_align1_core and mem_mark_primary_se."""
        L, idx, p = self.live.lib, self.live.idx, self.opt(o)
        q = np.ascontiguousarray(read, np.uint8).copy()
        v = L.mem_align1_core(p, idx.bwt, idx.bns, idx.pac, len(q), q.ctypes.data, None)
        out = self._stage1(p, v.a, v.n, idv, o["primary5"]) if v.n else []
        self.live.libc.free(v.a)
        self.live.libc.free(p)
        return out


# ---- constructed region sets -------------------------------------------------------------------------

KINDS = ("cut", "cut", "cut", "redundant", "strand", "noncolinear", "diag", "garbage", "alt", "random", "random",
         "chimera", "single", "identical", "ties")


def make_constructed(codes, contig_end, is_alt, n, seed, kinds=KINDS):
    """n reads with hand-made region sets over the reference `codes` (uint8, 0..3): a list of (read codes,
    list of region dicts). Needs nothing but the reference, so that tests can make fresh ones anywhere."""
    rng = np.random.default_rng(seed)
    codes = np.asarray(codes, np.uint8)
    l_pac = len(codes)
    cstart = np.concatenate([[0], contig_end[:-1]]).astype(np.int64)
    ri = lambda lo, hi: int(rng.integers(lo, hi))

    def rid_of(rb):
        return int(np.searchsorted(contig_end, rb if rb < l_pac else 2 * l_pac - 1 - rb, side="right"))

    def reg(rb, re, qb, qe, score, **kw):
        d = new_reg(rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), rid=rid_of(int(rb)), score=max(1, int(score)),
                    w=ri(0, 12), seedcov=max(1, (int(qe) - int(qb)) // 2 + ri(0, 5)), seedlen0=ri(19, 40))
        d["truesc"] = d["score"]
        if rng.random() < 0.12:
            d["csub"] = ri(1, max(2, d["score"] + 10))
        if rng.random() < 0.08:
            d["sub_n"] = ri(1, 4)
        if rng.random() < 0.08:
            d["sub"] = ri(1, max(2, d["score"]))
        d.update(kw)
        return d

    def true_read(lr=None, contig=None, n_sub=None, indel=None):
        """A read copied from the reference: (forward read, blocks [(q0, q1, r0)], substituted positions)."""
        lr = lr or ri(100, MAX_LEN + 1)
        c = ri(0, len(contig_end)) if contig is None else contig
        d = 0 if indel is None else indel
        s = ri(int(cstart[c]) + 10, int(contig_end[c]) - lr - abs(d) - 10)
        subs = sorted(rng.choice(lr, size=ri(0, 5) if n_sub is None else n_sub, replace=False).tolist())
        if d > 0:  # deletion from the read
            x = ri(30, lr - 30)
            fq = np.concatenate([codes[s:s + x], codes[s + x + d:s + lr + d]])
            blocks = [(0, x, s), (x, lr, s + x + d)]
        elif d < 0:  # insertion into the read
            x = ri(30, lr - 30 + d)
            fq = np.concatenate([codes[s:s + x], rng.integers(0, 4, -d).astype(np.uint8), codes[s + x:s + lr + d]])
            blocks = [(0, x, s), (x - d, lr, s + x)]
        else:
            fq, blocks = codes[s:s + lr].copy(), [(0, lr, s)]
        fq = fq.copy()
        for p in subs:
            fq[p] = (fq[p] + ri(1, 4)) % 4
        return fq, blocks, subs

    def rpos(blocks, q):
        for q0, q1, r0 in blocks:
            if q < q1:
                return r0 + max(q, q0) - q0
        q0, q1, r0 = blocks[-1]
        return r0 + q1 - q0

    def piece(blocks, subs, a, b, extra=0):
        rb, re = rpos(blocks, a), rpos(blocks, b - 1) + 1
        pen = 5 * sum(1 for p in subs if a <= p < b) + (7 if (re - rb) != (b - a) else 0)
        return [rb, re, a, b, (b - a) - pen + extra]

    def orient(fq, pieces, rev):
        """Regions in the read's orientation from forward pieces [rb, re, qb, qe, score]."""
        lr = len(fq)
        if not rev:
            return fq, [reg(*p) for p in pieces]
        return mk._rc(fq), [reg(2 * l_pac - p[1], 2 * l_pac - p[0], lr - p[3], lr - p[2], p[4]) for p in pieces]

    out = []
    for it in range(n):
        kind = kinds[ri(0, len(kinds))]
        rev = rng.random() < 0.4
        if kind == "cut":
            indel = int(rng.choice([0, 0, ri(1, 6), -ri(1, 6), ri(6, 30)]))
            fq, blocks, subs = true_read(indel=indel)
            lr, k = len(fq), ri(2, 5)
            cuts = sorted(rng.choice(np.arange(30, lr - 30, 30), size=min(k - 1, max(1, (lr - 60) // 30)), replace=False).tolist())
            edges = [0] + cuts + [lr]
            pcs = []
            for t in range(len(edges) - 1):
                a = edges[t] + (ri(-6, 7) if t else 0)
                b = edges[t + 1] + (ri(-6, 7) if t + 1 < len(edges) - 1 else 0)
                pcs.append(piece(blocks, subs, a, b))
            read, regs = orient(fq, pcs, rev)
        elif kind == "redundant":
            fq, blocks, subs = true_read()
            lr = len(fq)
            a, b = ri(0, 20), lr - ri(0, 20)
            pcs = [piece(blocks, subs, a, b)]
            for _ in range(ri(1, 4)):
                pcs.append(piece(blocks, subs, a + ri(0, 4), b - ri(0, 4), extra=int(rng.choice([-3, -1, 0, 0, 2]))))
            if rng.random() < 0.5:
                pcs.append(piece(blocks, subs, a, a + (b - a) // 2))
            read, regs = orient(fq, pcs, rev)
        elif kind == "strand":
            c = len(contig_end) - 1
            lr = ri(100, 200)
            s = l_pac - ri(lr + 20, lr + 400)
            fq = codes[s:s + lr].copy()
            x = lr // 2
            regs = [reg(s, s + x, 0, x, x), reg(l_pac + ri(5, 300), 0, x, lr, lr - x - ri(0, 10))]
            regs[1]["re"] = regs[1]["rb"] + lr - x
            read = fq
        elif kind == "noncolinear":
            fq, blocks, subs = true_read(n_sub=1)
            lr = len(fq)
            x = lr // 2
            p0, p1 = piece(blocks, subs, 0, x), piece(blocks, subs, x, lr)
            sh = ri(20, 60)  # the right half of the query lies left on the reference
            p1[0], p1[1] = p0[0] - sh - (lr - x), p0[0] - sh
            read, regs = orient(fq, [p0, p1], rev)
        elif kind == "diag":
            fq, blocks, subs = true_read(n_sub=ri(0, 3))
            lr = len(fq)
            x = ri(40, lr - 40)
            gq, gr = ri(-12, 25), ri(-30, 45)
            p0 = piece(blocks, subs, 0, x)
            p1 = piece(blocks, subs, x + gq, lr)
            p1[0] += gr - gq
            p1[1] += gr - gq
            read, regs = orient(fq, [p0, p1], rev)
        elif kind == "garbage":
            fq, blocks, subs = true_read(lr=ri(160, MAX_LEN + 1), n_sub=0)
            lr = len(fq)
            g0, g1 = lr // 2 - ri(10, 25), lr // 2 + ri(10, 25)
            fq[g0:g1] = rng.integers(0, 4, g1 - g0)
            read, regs = orient(fq, [piece(blocks, subs, 0, g0), piece(blocks, subs, g1, lr)], rev)
        elif kind == "alt" and is_alt.any():
            ca = int(np.flatnonzero(is_alt)[0])
            mode = ri(0, 4)
            lr = ri(80, 200)
            off = ri(10, 2200)
            pa = int(cstart[ca]) + off                       # on the ALT contig: a diverged copy of a primary segment
            # the primary copy's start is not known here; any primary locus does for the bookkeeping
            cp = int(rng.choice(np.flatnonzero(is_alt == 0)))
            pp = ri(int(cstart[cp]) + 10, int(contig_end[cp]) - lr - 10)
            fq = codes[pa:pa + lr].copy()
            sc = lambda: lr - 5 * ri(0, 6)
            regs = []
            if mode != 0:
                regs.append(reg(pp, pp + lr, 0, lr, sc()))
            regs.append(reg(pa, pa + lr, 0, lr, sc()))
            if mode >= 2:
                regs.append(reg(pp + 500, pp + 500 + lr - 10, 5, lr - 5, sc() - 10))
            if mode == 3:
                regs.append(reg(pa + 300, pa + 300 + lr // 2, 0, lr // 2, lr // 2 - ri(0, 4)))
            read = fq
        elif kind in ("random", "ties"):
            lr = ri(100, MAX_LEN + 1)
            c = ri(0, len(contig_end))
            base = ri(int(cstart[c]) + 50, int(contig_end[c]) - lr - 400)
            fq = codes[base:base + lr].copy()
            nr = int(rng.choice([2, 3, 3, 4, 5, 6, 8, 12, 16, 17, 17, 24, 40, 44])) if kind == "random" else ri(2, 8)
            scores = [ri(20, 40), ri(40, 80), ri(80, 120)]
            pcs = []
            for _ in range(nr):
                if pcs and rng.random() < (0.5 if kind == "ties" else 0.25):
                    p = list(pcs[ri(0, len(pcs))])
                    m = ri(0, 4)
                    if m == 0:
                        p[2] = max(0, p[2] - ri(1, 5)); p[0] -= ri(1, 5)
                    elif m == 1:
                        p[4] = int(rng.choice(scores))
                    elif m == 2:
                        p[0] += ri(0, 3); p[2] += ri(0, 3)
                    if not (p[0] < p[1] and p[2] < p[3]):
                        p = list(pcs[0])
                    pcs.append(p)
                    continue
                qb = ri(0, lr - 25)
                ql = ri(20, lr - qb + 1)
                far = ri(0, 3 if nr < 24 else 6) * 150 if kind == "random" else 0
                rb = base + qb + ri(-4, 5) + far
                pcs.append([rb, rb + ql + ri(-3, 4), qb, qb + ql, int(rng.choice(scores)) if rng.random() < 0.7 else ri(19, ql + 1)])
            read, regs = orient(fq, pcs, rev)
        elif kind == "chimera":
            f1, b1, s1 = true_read(lr=ri(60, 120))
            f2, b2, s2 = true_read(lr=ri(60, 120))
            fq = np.concatenate([f1, f2])
            l1 = len(f1)
            lo = ri(0, 4)
            regs = [reg(b1[0][2], b1[0][2] + l1 - lo, 0, l1 - lo, l1 - lo - 5 * len(s1) - ri(0, 30)),
                    reg(b2[0][2], b2[0][2] + len(f2), l1, len(fq), len(f2) - 5 * len(s2))]
            if rng.random() < 0.5:
                regs.append(reg(b1[0][2] + 4, b1[0][2] + 4 + l1 // 2, 0, l1 // 2, l1 // 2 - ri(0, 5)))
            for g in regs:
                g["score"] = g["truesc"] = max(g["score"], 31)
            read = fq
        elif kind == "identical":
            fq, blocks, subs = true_read()
            lr = len(fq)
            s, sc = blocks[0][2], ri(40, 60)
            regs = [reg(s, s + 50, 0, 50, sc), reg(s, s + lr - 10, 0, lr - 10, sc),
                    reg(s + 60, s + 80, 60, 80, 20, rid=(rid_of(s) + 1) % len(contig_end))]
            read = fq
        else:  # single: no region, or one
            fq, blocks, subs = true_read(lr=ri(30, MAX_LEN + 1), n_sub=ri(0, 8))
            lr = len(fq)
            pcs = [] if rng.random() < 0.3 else [piece(blocks, subs, 0, lr if rng.random() < 0.6 else ri(25, lr + 1))]
            read, regs = orient(fq, pcs, rev)
            for g in regs:
                if rng.random() < 0.4:
                    g["frac_rep"] = float(F32(ri(1, 60) / 100.))
        # keep every region inside the call's domain
        ok = []
        for g in regs:
            g["qb"], g["qe"] = max(0, g["qb"]), min(len(read), g["qe"])
            if g["qb"] < g["qe"] and 0 <= g["rb"] < g["re"] <= 2 * l_pac and not (g["rb"] < l_pac < g["re"]):
                if kind != "identical":  # that kind sets a rid of its own
                    g["rid"] = rid_of(g["rb"])
                ok.append(g)
        if rng.random() < 0.15 and ok:
            fr = float(F32(ri(1, 50) / 100.))
            for g in ok:
                g["frac_rep"] = fr
        order = rng.permutation(len(ok))
        out.append((np.asarray(read, np.uint8), [ok[i] for i in order]))
    return out


def pack_regs(per_read, fields):
    """Flat arrays for a list (per read) of lists of region dicts."""
    out = {"n": np.array([len(x) for x in per_read], np.int32)}
    flat = [g for x in per_read for g in x]
    for f in fields:
        t = np.float32 if f == "frac_rep" else np.int64 if f in ("rb", "re") else np.int32
        out[f] = np.array([g[f] for g in flat], t)
    return out


def hash_64_np(key):
    """hash_64 on a uint64 array."""
    k = np.asarray(key, np.uint64).copy()
    u = lambda v: np.uint64(v)
    with np.errstate(over="ignore"):
        k += ~(k << u(32))
        k ^= k >> u(22)
        k += ~(k << u(13))
        k ^= k >> u(8)
        k += k << u(3)
        k ^= k >> u(15)
        k += ~(k << u(27))
        k ^= k >> u(31)
    return k


def expected(fx, g, stage):
    """The live result of group g at `stage`: (n_out per read, dict field -> flat array over the regions
    left, in read order)."""
    p = "%s_s0_" % g
    n0 = fx[p + "n"]
    s0 = {f: fx[p + f] for f in FIELDS if f not in S0_ZERO}
    for f in S0_ZERO:
        s0[f] = np.zeros(len(s0["rb"]), np.uint64 if f == "hash" else np.int32)
    if stage == 0:
        return n0, s0
    q = "%s_s1_" % g
    off0 = np.concatenate([[0], np.cumsum(n0, dtype=np.int64)])[:-1]
    read = np.repeat(np.arange(len(n0)), n0)
    src = off0[read] + fx[q + "hash_i"]
    s1 = {f: v[src] for f, v in s0.items()}
    for f in S1_FIELDS:
        s1[f] = fx[q + f]
    id0 = int(fx["group_id0"][list(fx["group_names"]).index(g)])
    s1["hash"] = hash_64_np((np.uint64(id0) + read.astype(np.uint64) + fx[q + "hash_i"].astype(np.uint64)))
    return fx[q + "n"], s1


def same(x, y):
    return len(x) == len(y) and all(all((F32(a[f]) == F32(b[f])) if f == "frac_rep" else a[f] == b[f] for f in FIELDS)
                                    for a, b in zip(x, y))


def main():
    if not mk.available():
        print("skipped: needs %s and oracle/_ref/libref_bwa.so (make ref)" % mk.REF_TREE)
        return 0
    contigs, sites = mk.make_reference()
    live = mk.LiveBwa(contigs)
    try:
        lr = LiveRegs(live)
        mkfx = np.load(os.path.join(HERE, "bsw_mkchain_golden.npz"))
        assert (mkfx["ref_codes"] == live.codes).all() and (mkfx["contig_end"] == live.contig_end).all()
        o0 = opts()
        aligned = [r for r in mk.make_reads(contigs, sites, n_scale=0.3, seed=23) if len(r) >= 19]
        reads, regs_in = [], []
        for x in aligned:
            g = lr.chain2aln(o0, x)
            for d in g:
                d["mapq"] = 0
            reads.append(x), regs_in.append(g)
        n_al = len(reads)
        for x, g in make_constructed(live.codes, live.contig_end, live.is_alt, 1400, seed=31):
            reads.append(x), regs_in.append(g)
        n = len(reads)
        print("reference %d bases, %d aligned and %d constructed reads, %d regions" % (
            live.l_pac, n_al, n - n_al, sum(map(len, regs_in))))
        fx = dict(lens=np.array([len(r) for r in reads], np.int32), n_aligned=np.int32(n_al))
        codes = np.full((n, MAX_LEN), 4, np.uint8)
        for r, x in enumerate(reads):
            codes[r, :len(x)] = x
        fx["reads"] = codes
        for k, v in pack_regs(regs_in, IN_FIELDS).items():
            fx["in_" + k] = v
        counts = np.zeros((len(GROUPS) + 1, len(LABELS)), np.int32)
        rng = np.random.default_rng(41)
        order_default = {}
        for gi, (g, (kw, id0)) in enumerate(GROUPS.items()):
            o = opts(**kw)
            if g == "default":
                sel = np.arange(n)
            else:
                sel = np.sort(np.concatenate([rng.choice(n_al, 50, replace=False), n_al + rng.choice(n - n_al, 200, replace=False)]))
            per0, per1, n_alns = [], [], []
            for k, r in enumerate(sel):
                flags = set()
                p = lr.opt(o)
                s0, s1 = lr.finish(o, reads[r], regs_in[r], id0 + k)
                m0, m1, n_aln = py_finish(o, live.l_pac, live.is_alt, regs_in[r], lr.align(p, reads[r]), id0 + k, flags)
                live.libc.free(p)
                assert same(s0, m0), "group %s read %d: the restatement's stage 0 differs" % (g, r)
                assert same(s1, m1), "group %s read %d: the restatement's stage 1 differs" % (g, r)
                if g == "default" and r < n_al:  # the same from the reads alone
                    assert same(s1, lr.align1(o, reads[r], id0 + k)), "read %d: mem_align1_core differs" % r
                nr = len(regs_in[r])
                flags.add("n40p" if nr >= 40 else "n%d" % nr if nr in (0, 1, 2, 3, 16, 17) else "")
                key = [(x["rb"], x["re"], x["qb"]) for x in s1]
                if g == "default":
                    order_default[int(r)] = key
                elif g == "id0" and key != order_default[int(r)] and sorted(key) == sorted(order_default[int(r)]):
                    flags.add("hash_tie")
                for f in flags - {""}:
                    counts[gi, LABELS.index(f)] += 1
                # the hash is stored as the i of hash_64(id + i): the region's place in the stage-0 order
                place = {hash_64(id0 + k + i): i for i in range(len(s1))}
                for x in s1:
                    x["hash_i"] = place[x["hash"]]
                    assert all(x[f] == s0[x["hash_i"]][f] for f in FIELDS if f not in S1_FIELDS and f not in S0_ZERO)
                per0.append(s0), per1.append(s1), n_alns.append(n_aln)
            fx[g + "_reads"] = sel.astype(np.int32)
            fx[g + "_n_aln"] = np.array(n_alns, np.int8)
            for st, per in ((0, per0), (1, per1)):
                # stage 0 leaves secondary, secondary_all, alt_sc, hash and mapq as given: 0 in this fixture.
                # stage 1 moves whole records and changes S1_FIELDS only (asserted), so it is stored as the
                # record's place in stage 0, which is also the i of its hash, plus those fields.
                fields = [f for f in FIELDS if f not in S0_ZERO] if st == 0 else list(S1_FIELDS) + ["hash_i"]
                for k, v in pack_regs(per, fields).items():
                    fx["%s_s%d_%s" % (g, st, k)] = v
            print("group %-16s %4d reads, %5d regions in, %5d left, %4d alignments, at most %d per read" % (
                g, len(sel), sum(len(regs_in[r]) for r in sel), sum(map(len, per1)), sum(n_alns), max(n_alns)))
        # end to end: the aligned reads come first and the default group's id is the read's index, so the
        # default group's first n_aligned reads are what live mem_align1_core and mem_mark_primary_se give
        # for a call of those reads alone (asserted above, read by read)
        fx["label_counts"] = counts
        fx["label_names"] = np.array(LABELS)
        fx["label_min"] = np.int32(LABEL_MIN)
        fx["group_names"] = np.array(list(GROUPS))
        fx["opt_names"] = np.array(list(DEFAULTS))
        fx["group_opts"] = np.array([[float(opts(**kw)[k]) for k in DEFAULTS] for kw, _ in GROUPS.values()], np.float64)
        fx["group_id0"] = np.array([i for _, i in GROUPS.values()], np.int64)
        total = counts.sum(0)
        for k, name in enumerate(LABELS):
            print("label %-20s %5d" % (name, int(total[k])))
        short = [LABELS[k] for k in range(len(LABELS)) if total[k] < LABEL_MIN]
        assert not short, "labels below %d: %s" % (LABEL_MIN, short)
        np.savez_compressed(OUT, **fx)
        print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    finally:
        live.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
