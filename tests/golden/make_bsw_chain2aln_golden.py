"""Regenerate tests/golden/bsw_chain2aln_golden.npz: inputs and expected outputs of bwa's mem_chain2aln
(tools/bwa/bwamem.c:632-824) for what tests/test_bsw_chain2aln.py runs through gb_bsw_chain2aln.
Seeds are fixed: a rerun reproduces the file.

    python tests/golden/make_bsw_chain2aln_golden.py

bwamem.c is not part of oracle/_ref/libref_bwa.so, so mem_chain2aln's CONTROL FLOW (cal_max_gap, the
window and its clamps, bns_fetch_seq's clip to the contig, the order of the seeds, the band retry, the
local / to-end choice, seedcov, the containment test and the overlapping-seed check) is RESTATED here in
Python (chain2aln_read), line by line. Every FETCH and every DP is the reference's own: bns_get_seq and
ksw_extend2 of libref_bwa.so through ctypes. mem_chain2aln extends only the seeds it keeps; the
restatement also extends the seeds it skips (an extension does not depend on the region list), so that
the raw records cover every seed.

References: l4096 and l4099, random bases (l_pac % 4 is 0 and 3), the ones of the gen_cigar fixture.
Groups (`sets`; each under one reference, one parameter set, one contig_end):
  ends        a seed at the read's start, at its end, and covering it: the three no-extension branches
  clip        windows clamped at 0, at 2 l_pac and at l_pac from either side, reverse-strand chains, a left
              and a right target of length 0
  contig2, contig3   two and three contigs; windows clipped by a contig end on each strand
  band4, band8       w = 4 / 8 with planted indels: one crossable at w that drives max_off past 3w/4, and a
              second one behind it that only 2w crosses (second try, other score); the first alone (second
              try, same score); none (one try, max_off below 3w/4); a right flank of mismatches (one try,
              score == prev). On the left prev is -1, which no score is, so only the right side can stop
              by score == prev.
  clipend0, clipend5, clipasym   mismatches 1-4 bases from the read's ends, pen_clip (0, 0), (5, 5), (5, 0)
  zdrop       zdrop = 10 and flanks with four mismatches in a row followed by matches
  contain     later seeds skipped; seeds contained but kept by the overlapping-seed check; seeds kept by
              the seedlen0 rule; a later chain's seeds skipped by an earlier chain's region; reads whose
              every later seed is skipped
  general     benchmark defaults, 5 % substitutions, indels, N; one or two chains of up to four seeds.
              CIGARs for its regions: mem_reg2aln's loop (bwamem.c:1154-1163) around live bwa_gen_cigar2
              with w = the region's w and truesc
  asym        o_del 4, e_del 2, o_ins 7, e_ins 1
  match2      match 2, mismatch -4
Per seed and side the fixture also records why it is there: `stop` (0 no extension, 1 one try ended by
max_off < 3w/4, 2 one try ended by score == prev, 3 two tries with another score, 4 two tries with the same
score), `end` (0 none, 1 local, 2 to-end), `zd` (1: the outputs change when zdrop is switched off, so the
extension ended by z-drop), and per seed `fate` (0 kept without being contained, 1 skipped, 2 contained but
kept by the overlapping-seed check), `by_seedlen0` (kept, and :676 passed over a containing region),
`by_earlier` (skipped because of a region of an earlier chain)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_bsw_gencigar_golden as gc  # noqa: E402  (reference library, pac packing, bwa_gen_cigar2)

OUT = os.path.join(HERE, "bsw_chain2aln_golden.npz")
REG_FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "seedlen0", "chain", "seed")
IN_KEYS = ("ref", "pen", "mat", "pw", "zdrop", "clip", "contig_end", "qry", "qoff", "qlen", "rco", "cso", "seeds")
OUT_KEYS = ("regs", "n_reg", "raw_out6", "raw_tries", "raw_skipped", "stop", "end", "zd", "fate", "by_seedlen0",
            "by_earlier")
CIGAR_KEYS = ("cg_score", "cg_n_cigar", "cg_nm", "cg_cigar", "cg_md_len", "cg_md", "cg_tries", "cg_w_final")
WITNESS_ZDROP = True  # run every extension a second time without z-drop to see whether it ended by it
SETS = ("ends", "clip", "contig2", "contig3", "band4", "band8", "clipend0", "clipend5", "clipasym", "zdrop", "contain",
        "general", "asym", "match2")


def ref_lib():
    """gc.ref_lib() with ksw_extend2 declared as well, or None when oracle/_ref is not built."""
    ref = gc.ref_lib()
    if ref is None:
        return None
    ci, vp = ctypes.c_int, ctypes.c_void_p
    ip = ctypes.POINTER(ci)
    ref[0].ksw_extend2.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ip, ip, ip, ip, ip]
    ref[0].ksw_extend2.restype = ci
    return ref


class Opt:
    """The fields of mem_opt_t that mem_chain2aln reads."""

    def __init__(self, pen=(6, 1, 6, 1), mat=None, w=100, zdrop=100, clip=(5, 5)):
        self.o_del, self.e_del, self.o_ins, self.e_ins = (int(x) for x in pen)
        self.mat = gc.scmat() if mat is None else np.ascontiguousarray(mat, np.int8)
        self.a, self.w, self.zdrop = int(self.mat[0]), int(w), int(zdrop)
        self.pen_clip5, self.pen_clip3 = int(clip[0]), int(clip[1])


def cal_max_gap(o, qlen):
    """bwamem.c:621-628; Python's int / int is the double division of the reference, int() its truncation."""
    l_del = int((qlen * o.a - o.o_del) / o.e_del + 1.)
    l_ins = int((qlen * o.a - o.o_ins) / o.e_ins + 1.)
    l = max(l_del, l_ins, 1)
    return min(l, o.w << 1)


def extend(ref, o, q, t, w, end_bonus, h0, zdrop=None):
    """One live ksw_extend2: [score, qle, tle, gtle, gscore, max_off]."""
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    v = [ctypes.c_int(0) for _ in range(5)]
    sc = ref[0].ksw_extend2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, o.mat.ctypes.data, o.o_del, o.e_del,
                            o.o_ins, o.e_ins, int(w), int(end_bonus), o.zdrop if zdrop is None else zdrop, int(h0),
                            *[ctypes.byref(x) for x in v])
    return [sc] + [x.value for x in v]


def window(o, l_pac, contig_end, l_query, seeds):
    """rmax of bwamem.c:642-657 and bns_fetch_seq's clip (bntseq.c:433-444)."""
    r0, r1 = l_pac << 1, 0
    for rbeg, qbeg, ln, _ in seeds:
        b = rbeg - (qbeg + cal_max_gap(o, qbeg))
        e = rbeg + ln + ((l_query - qbeg - ln) + cal_max_gap(o, l_query - qbeg - ln))
        r0, r1 = min(r0, b), max(r1, e)
    r0, r1 = max(r0, 0), min(r1, l_pac << 1)
    if r0 < l_pac < r1:
        if seeds[0][0] < l_pac:
            r1 = l_pac
        else:
            r0 = l_pac
    mid = seeds[0][0]
    assert r0 <= mid < r1
    is_rev = mid >= l_pac
    pos_f = (l_pac << 1) - 1 - mid if is_rev else mid
    ends = [l_pac] if contig_end is None else [int(x) for x in contig_end]
    rid = next(k for k, e in enumerate(ends) if pos_f < e)
    far_beg, far_end = (ends[rid - 1] if rid else 0), ends[rid]
    if is_rev:
        far_beg, far_end = (l_pac << 1) - far_end, (l_pac << 1) - far_beg
    return max(r0, far_beg), min(r1, far_end)


def extend_seed(ref, o, query, rseq, rmax0, seed):
    """Both sides of one seed (bwamem.c:715-809): the region fields, the raw record and the statistics."""
    rbeg, qbeg, ln, _ = seed
    l_query = len(query)
    a = {"w": o.w, "score": -1, "truesc": -1}
    aw = [o.w, o.w]
    raw, tries, stop, end, zd = np.zeros((2, 6), np.int32), [0, 0], [0, 0], [0, 0], [0, 0]

    def side(k, qs, ts, pen_clip, h0, prev0):
        res, scores = None, []
        for i in range(2):  # MAX_BAND_TRY
            prev = prev0 if i == 0 else scores[-1]
            aw[k] = o.w << i
            res = extend(ref, o, qs, ts, aw[k], pen_clip, h0)
            if WITNESS_ZDROP and res != extend(ref, o, qs, ts, aw[k], pen_clip, h0, zdrop=0):
                zd[k] = 1
            scores.append(res[0])
            tries[k] = i + 1
            if res[0] == prev or res[5] < (aw[k] >> 1) + (aw[k] >> 2):
                break
        if len(scores) == 1:
            stop[k] = 2 if scores[0] == prev0 else 1
        else:
            stop[k] = 4 if scores[1] == scores[0] else 3
        raw[k] = res
        return res

    if qbeg:
        tmp = rbeg - rmax0
        sc, qle, tle, gtle, gscore, _ = side(0, query[:qbeg][::-1], rseq[:tmp][::-1], o.pen_clip5, ln * o.a, -1)
        a["score"] = sc
        if gscore <= 0 or gscore <= sc - o.pen_clip5:
            a["qb"], a["rb"], a["truesc"], end[0] = qbeg - qle, rbeg - tle, sc, 1
        else:
            a["qb"], a["rb"], a["truesc"], end[0] = 0, rbeg - gtle, gscore, 2
    else:
        a["score"] = a["truesc"] = ln * o.a
        a["qb"], a["rb"] = 0, rbeg
    if qbeg + ln != l_query:
        sc0, qe, re = a["score"], qbeg + ln, rbeg + ln - rmax0
        assert re >= 0
        sc, qle, tle, gtle, gscore, _ = side(1, query[qe:], rseq[re:], o.pen_clip3, sc0, sc0)
        a["score"] = sc
        if gscore <= 0 or gscore <= sc - o.pen_clip3:
            a["qe"], a["re"], end[1] = qe + qle, rmax0 + re + tle, 1
            a["truesc"] += sc - sc0
        else:
            a["qe"], a["re"], end[1] = l_query, rmax0 + re + gtle, 2
            a["truesc"] += gscore - sc0
    else:
        a["qe"], a["re"] = l_query, rbeg + ln
    a["w"] = max(aw)
    a["seedlen0"] = ln
    return a, raw, tries, stop, end, zd


def chain2aln_read(ref, pac, l_pac, contig_end, o, query, chains, chain_base=0, seed_base=0):
    """mem_chain2aln for every chain of one read into one region list (av), restated. Returns (regions as
    dicts with chain / seed = index in the call, per-seed records in seed order)."""
    av, recs = [], []
    l_query = len(query)
    for ci, seeds in enumerate(chains):
        n = len(seeds)
        assert n > 0
        rmax0, rmax1 = window(o, l_pac, contig_end, l_query, seeds)
        rseq = gc.get_seq_one(ref, pac, l_pac, rmax0, rmax1)
        assert len(rseq) == rmax1 - rmax0
        srt = sorted((s[3] << 32) | i for i, s in enumerate(seeds))
        rec = [None] * n
        for k in range(n - 1, -1, -1):
            idx = srt[k] & 0xFFFFFFFF
            s = seeds[idx]
            rbeg, qbeg, ln, _ = s
            ext = extend_seed(ref, o, query, rseq, rmax0, s)
            r = {"raw": ext[1], "tries": ext[2], "stop": ext[3], "end": ext[4], "zd": ext[5], "skipped": 0, "fate": 0,
                 "by_seedlen0": 0, "by_earlier": 0}
            rec[idx] = r
            passed = False
            hit = None
            for p in av:  # bwamem.c:671-687
                if rbeg < p["rb"] or rbeg + ln > p["re"] or qbeg < p["qb"] or qbeg + ln > p["qe"]:
                    continue
                if ln - p["seedlen0"] > .1 * l_query:
                    passed = True
                    continue
                qd, rd = qbeg - p["qb"], rbeg - p["rb"]
                w = min(cal_max_gap(o, min(qd, rd)), p["w"])
                if qd - rd < w and rd - qd < w:
                    hit = p
                    break
                qd, rd = p["qe"] - (qbeg + ln), p["re"] - (rbeg + ln)
                w = min(cal_max_gap(o, min(qd, rd)), p["w"])
                if qd - rd < w and rd - qd < w:
                    hit = p
                    break
            if hit is not None:  # bwamem.c:692-703
                i = k + 1
                while i < n:
                    if srt[i] != 0:
                        tr, tq, tl, _ = seeds[srt[i] & 0xFFFFFFFF]
                        if not tl < ln * .95:
                            if qbeg <= tq and qbeg + ln - tq >= ln >> 2 and tq - qbeg != tr - rbeg:
                                break
                            if tq <= qbeg and tq + tl - qbeg >= ln >> 2 and qbeg - tq != rbeg - tr:
                                break
                    i += 1
                if i == n:
                    srt[k] = 0
                    r["skipped"], r["fate"] = 1, 1
                    r["by_earlier"] = int(hit["chain"] != chain_base + ci)
                    continue
                r["fate"] = 2
            elif passed:
                r["by_seedlen0"] = 1
            a = ext[0]
            a["seedcov"] = sum(t[2] for t in seeds
                               if t[1] >= a["qb"] and t[1] + t[2] <= a["qe"] and t[0] >= a["rb"] and t[0] + t[2] <= a["re"])
            a["chain"], a["seed"] = chain_base + ci, seed_base + idx
            av.append(a)
        recs += rec
        seed_base += n
    return av, recs


def reads_of(g):
    """[(query, [chain, ...])] of a group dict, a chain being a list of (rbeg, qbeg, len, score)."""
    out = []
    for r in range(len(g["qlen"])):
        q = g["qry"][g["qoff"][r]:g["qoff"][r] + g["qlen"][r]]
        chains = [[tuple(int(x) for x in g["seeds"][k]) for k in range(g["cso"][c], g["cso"][c + 1])]
                  for c in range(g["rco"][r], g["rco"][r + 1])]
        out.append((q, chains))
    return out


def opt_of(g):
    return Opt(g["pen"], g["mat"], g["pw"], g["zdrop"], g["clip"])


def run_group(ref, refs, g):
    """Reference outputs of a group: dict of OUT_KEYS."""
    pac, l_pac = refs[refs["names"][int(g["ref"])]]
    ce = g["contig_end"] if len(g["contig_end"]) else None
    o = opt_of(g)
    regs, n_reg, recs = [], [], []
    cb = sb = 0
    for q, chains in reads_of(g):
        av, rc = chain2aln_read(ref, pac, l_pac, ce, o, q, chains, cb, sb)
        regs += [[a[f] for f in REG_FIELDS] for a in av]
        n_reg.append(len(av))
        recs += rc
        cb, sb = cb + len(chains), sb + len(rc)
    n = len(recs)
    return {"regs": np.array(regs, np.int64).reshape(-1, len(REG_FIELDS)), "n_reg": np.array(n_reg, np.int32),
            "raw_out6": np.array([r["raw"] for r in recs], np.int32).reshape(n, 2, 6),
            "raw_tries": np.array([r["tries"] for r in recs], np.int32).reshape(n, 2),
            "raw_skipped": np.array([r["skipped"] for r in recs], np.int32),
            "stop": np.array([r["stop"] for r in recs], np.int8).reshape(n, 2),
            "end": np.array([r["end"] for r in recs], np.int8).reshape(n, 2),
            "zd": np.array([r["zd"] for r in recs], np.int8).reshape(n, 2),
            "fate": np.array([r["fate"] for r in recs], np.int8),
            "by_seedlen0": np.array([r["by_seedlen0"] for r in recs], np.int8),
            "by_earlier": np.array([r["by_earlier"] for r in recs], np.int8)}


def region_queries(g, regs):
    """Per region: the read's bases [qb, qe), which is what mem_reg2aln aligns."""
    read_of = np.repeat(np.arange(len(g["n_reg"])), g["n_reg"])
    return [g["qry"][g["qoff"][r] + regs[k, 2]:g["qoff"][r] + regs[k, 3]] for k, r in enumerate(read_of)]


def run_cigars(ref, refs, g, regs):
    """mem_reg2aln's loop over live bwa_gen_cigar2 (gc.run_retry) for every region: dict of CIGAR_KEYS."""
    qs = region_queries(g, regs)
    pg = gc.pack(int(g["ref"]), [(q, int(regs[k, 0]), int(regs[k, 1]), int(regs[k, 6])) for k, q in enumerate(qs)],
                 pen=tuple(int(x) for x in g["pen"]), mat=g["mat"], pw=int(g["pw"]))
    pg["truesc"] = regs[:, 5].astype(np.int32)
    out = gc.run_retry(ref, refs, pg)
    return {"cg_" + k: v for k, v in out.items()}


# ---- inputs -------------------------------------------------------------------------------------------

def doubled(codes):
    """bwa's doubled coordinate space: position x >= L is the complement of forward base 2 L - 1 - x."""
    return np.concatenate([codes, 3 - codes[::-1]]).astype(np.uint8)


def build_read(rng, D, pos, plan, prefix=0, suffix=0):
    """A read planted at D[pos ...]: plan is a list of ('M', n) copy, ('X', n) n mismatches, ('N', n) n
    bases of code 4, ('I', n) n bases the reference lacks, ('D', n) n reference bases the read lacks;
    prefix / suffix random bases hang over. Returns (query, [(rbeg, qbeg, len)] of the M runs)."""
    q, runs, r = list(rng.integers(0, 4, prefix)), [], pos
    for op, n in plan:
        if op == "M":
            runs.append((r, len(q), n))
            q += D[r:r + n].tolist()
            r += n
        elif op == "X":
            q += [(int(D[r + i]) + 1 + int(rng.integers(0, 3))) % 4 for i in range(n)]
            r += n
        elif op == "N":
            q += [4] * n
            r += n
        elif op == "I":
            q += rng.integers(0, 4, n).tolist()
        else:
            r += n
    q += list(rng.integers(0, 4, suffix))
    return np.array(q, np.uint8), runs


def seed_of(run, a=1, score=None):
    return (int(run[0]), int(run[1]), int(run[2]), int(run[2] * a if score is None else score))


def pack(ref_idx, reads, o=None, contig_end=None):
    """Group dict from [(query, [chain, ...])]."""
    o = o or Opt()
    ql = np.array([len(q) for q, _ in reads], np.int32)
    qoff = np.zeros(len(reads), np.int64)
    qoff[1:] = np.cumsum(ql)[:-1]
    rco = np.zeros(len(reads) + 1, np.int64)
    rco[1:] = np.cumsum([len(c) for _, c in reads])
    flat = [c for _, cs in reads for c in cs]
    cso = np.zeros(len(flat) + 1, np.int64)
    cso[1:] = np.cumsum([len(c) for c in flat])
    seeds = np.array([s for c in flat for s in c], np.int64).reshape(-1, 4)
    return {"ref": np.int32(ref_idx), "pen": np.array([o.o_del, o.e_del, o.o_ins, o.e_ins], np.int32), "mat": o.mat,
            "pw": np.int32(o.w), "zdrop": np.int32(o.zdrop), "clip": np.array([o.pen_clip5, o.pen_clip3], np.int32),
            "contig_end": np.array([] if contig_end is None else contig_end, np.int64),
            "qry": np.concatenate([q for q, _ in reads]), "qoff": qoff, "qlen": ql, "rco": rco, "cso": cso, "seeds": seeds}


def strand_pos(rng, L, k, span, margin=40):
    """A start in the doubled space for read k of a group: even k forward, odd k reverse."""
    p = int(rng.integers(margin, L - span - margin))
    return p + (L if k & 1 else 0)


def g_ends(rng, D, L):
    reads = []
    for k in range(33):
        kind = k % 3
        plan = [("M", 25), ("X", 1), ("M", 30), ("I", 2), ("M", 28)] if kind < 2 else [("M", int(rng.integers(40, 120)))]
        q, runs = build_read(rng, D, strand_pos(rng, L, k // 3, 130), plan)
        reads.append((q, [[seed_of(runs[0] if kind == 0 else runs[-1])]]))
    return reads


def g_clip(rng, D, L):
    reads = []
    two = [("M", 22), ("X", 1), ("M", 40)]
    for k in range(4):
        q, runs = build_read(rng, D, 2 + k, two)  # the window would start below 0
        reads.append((q, [[seed_of(runs[1])]]))
        q, runs = build_read(rng, D, 2 * L - 63 - 2 - k, two)  # ... end beyond 2 l_pac
        reads.append((q, [[seed_of(runs[0])]]))
        q, runs = build_read(rng, D, L - 63 - 2 - k, two)  # forward chain whose window would cross l_pac
        reads.append((q, [[seed_of(runs[0])]]))
        q, runs = build_read(rng, D, L + 2 + k, two)  # reverse chain whose window would cross l_pac
        reads.append((q, [[seed_of(runs[1])]]))
        for at in (0, L):  # a left target of length 0: the seed starts where the strand does
            q, runs = build_read(rng, D, at, [("M", 40), ("X", 1), ("M", 12)], prefix=3 + k)
            reads.append((q, [[seed_of(runs[0])]]))
        for at in (L, 2 * L):  # a right target of length 0
            q, runs = build_read(rng, D, at - 53, [("M", 12), ("X", 1), ("M", 40)], suffix=3 + k)
            reads.append((q, [[seed_of(runs[1])]]))
    for k in range(8):  # reverse-strand chains of several seeds
        q, runs = build_read(rng, D, L + int(rng.integers(100, L - 300)),
                             [("M", 30), ("X", 1), ("M", 25), ("D", 2), ("M", 35), ("I", 1), ("M", 20)])
        reads.append((q, [[seed_of(r) for r in runs]]))
    return reads


def g_contig(rng, D, L, ends):
    reads = []
    two = [("M", 22), ("X", 1), ("M", 40)]
    for e in ends[:-1]:
        for k in range(3):
            # forward: a read ending just before the contig end, one starting just behind it; reverse: the mirrors
            for pos, run in ((e - 63 - 1 - k, 0), (e + 1 + k, 1), (2 * L - e - 63 - 1 - k, 0), (2 * L - e + 1 + k, 1)):
                q, runs = build_read(rng, D, pos, two)
                reads.append((q, [[seed_of(runs[run])]]))
    return reads


def g_band(rng, D, L, w):
    thr = (w >> 1) + (w >> 2)
    reads = []
    for k in range(36):
        kind, left, ins = k % 3, (k // 3) % 2 == 0, (k // 6) % 2 == 0
        d1 = int(rng.integers(thr, w + 1))
        d2 = int(rng.integers(w + 1 - d1, 2 * w + 1 - d1)) if d1 < w else int(rng.integers(1, w + 1))
        op = "I" if ins else "D"
        gaps = [[], [(op, d1)], [(op, d1), (op, d2)]][kind]
        flank = [("M", 20)]
        for g in gaps:
            flank += [g, ("M", 20)]
        seed = [("M", 20)]
        plain = [("X", 1), ("M", 28)]
        # the flank as the extension meets it: outwards from the seed
        plan = flank[::-1] + seed + plain if left else plain[::-1] + seed + flank
        q, runs = build_read(rng, D, strand_pos(rng, L, k, 200), plan)
        s = runs[len(gaps) + 1] if left else runs[1]
        reads.append((q, [[seed_of(s)]]))
    for k in range(12):  # a right flank that gains nothing: one try, score == prev
        q, runs = build_read(rng, D, strand_pos(rng, L, k, 120), [("M", 30), ("X", 1), ("M", 20), ("X", 25)])
        reads.append((q, [[seed_of(runs[1])]]))
    return reads


def g_clipend(rng, D, L):
    reads = []
    for k in range(24):
        kl, kr = 1 + k % 4, 1 + (k // 4) % 4
        plan = ([("M", kl), ("X", 1)] if k % 3 else []) + [("M", 24), ("X", 1), ("M", 25), ("X", 1), ("M", 24)] + \
               ([("X", 1), ("M", kr)] if k % 5 else [])
        q, runs = build_read(rng, D, strand_pos(rng, L, k, 130), plan)
        reads.append((q, [[seed_of(next(r for r in runs if r[2] == 25))]]))
    return reads


def g_zdrop(rng, D, L):
    reads = []
    for k in range(12):
        plan = [("M", 30), ("X", 4), ("M", 25), ("X", 4), ("M", 30)]
        q, runs = build_read(rng, D, strand_pos(rng, L, k, 130), plan)
        reads.append((q, [[seed_of(runs[1])]]))
    return reads


def g_contain(rng, D, L):
    reads = []
    for k in range(8):
        pos = strand_pos(rng, L, k, 130)
        q, _ = build_read(rng, D, pos, [("M", 100)])

        def sd(qb, ln, diag=0, score=None):
            return (pos + qb + diag, qb, ln, ln if score is None else score)
        # every later seed skipped: one region from five seeds
        reads.append((q, [[sd(10, 30), sd(20, 50), sd(35, 40), sd(0, 25), sd(60, 40, score=39)]]))
        # T on another diagonal is contained in A's region but overlaps A; S is contained and overlaps T
        reads.append((q, [[sd(0, 60), sd(30, 40, diag=3, score=45), sd(35, 35)]]))
        # a short seed with a high score first; the long one is contained but 50 bases longer
        reads.append((q, [[sd(40, 20, score=90), sd(10, 70)]]))
        # a second chain on the first one's diagonal
        reads.append((q, [[sd(5, 40), sd(50, 45)], [sd(20, 30), sd(60, 25)]]))
    return reads


def g_general(rng, D, L, n, a=1):
    reads = []
    for k in range(n):
        plan, total = [], 0
        want = int(rng.integers(40, 152))
        while total < want:
            m = int(rng.integers(8, 45))
            plan.append(("M", m))
            r = rng.random()
            if r < .5:
                plan.append(("X", 1))
            elif r < .65:
                plan.append(("I", int(rng.integers(1, 4))))
            elif r < .8:
                plan.append(("D", int(rng.integers(1, 4))))
            elif r < .9:
                plan.append(("N", 1))
            else:
                plan.append(("X", 2))
            total += m + 2
        pos = strand_pos(rng, L, k, 200)
        q, runs = build_read(rng, D, pos, plan[:-1])
        q = q[:151]
        runs = [(r, qb, min(ln, len(q) - qb)) for r, qb, ln in runs if qb < len(q)]
        good = [r for r in runs if r[2] >= 12][:4] or [max(runs, key=lambda r: r[2])]
        chains = [[seed_of(r, a) for r in good]]
        if k % 3 == 0:  # a second chain: the same read placed somewhere else, seeds as they come
            other = strand_pos(rng, L, k + 1, 200) - pos
            chains.append([(r[0] + other, r[1], r[2], r[2] * a) for r in good[:2]])
        reads.append((q, chains))
    return reads


def build(ref=None):
    """All inputs: (refs, {group name: dict of IN_KEYS})."""
    codes = gc.build_refs()
    refs = {"names": ["l4096", "l4099"]}
    for n in refs["names"]:
        refs[n] = (gc.pack_pac(codes[n]), len(codes[n]))
    D = [doubled(codes[n]) for n in refs["names"]]
    Ls = [len(codes[n]) for n in refs["names"]]
    rng = np.random.default_rng(632)
    g = {}
    g["ends"] = pack(0, g_ends(rng, D[0], Ls[0]))
    g["clip"] = pack(1, g_clip(rng, D[1], Ls[1]))
    g["contig2"] = pack(0, g_contig(rng, D[0], Ls[0], [2000, 4096]), contig_end=[2000, 4096])
    g["contig3"] = pack(1, g_contig(rng, D[1], Ls[1], [1000, 2500, 4099]), contig_end=[1000, 2500, 4099])
    g["band4"] = pack(0, g_band(rng, D[0], Ls[0], 4), Opt(w=4))
    g["band8"] = pack(1, g_band(rng, D[1], Ls[1], 8), Opt(w=8))
    g["clipend0"] = pack(0, g_clipend(rng, D[0], Ls[0]), Opt(clip=(0, 0)))
    g["clipend5"] = pack(1, g_clipend(rng, D[1], Ls[1]), Opt(clip=(5, 5)))
    g["clipasym"] = pack(0, g_clipend(rng, D[0], Ls[0]), Opt(clip=(5, 0)))
    g["zdrop"] = pack(1, g_zdrop(rng, D[1], Ls[1]), Opt(zdrop=10))
    g["contain"] = pack(0, g_contain(rng, D[0], Ls[0]))
    g["general"] = pack(1, g_general(rng, D[1], Ls[1], 36))
    g["asym"] = pack(0, g_general(rng, D[0], Ls[0], 20), Opt(pen=(4, 2, 7, 1)))
    g["match2"] = pack(1, g_general(rng, D[1], Ls[1], 20, a=2), Opt(mat=gc.scmat(2, 4)))
    return refs, g


def load(z):
    """(refs, {group name: dict of IN_KEYS + OUT_KEYS (+ CIGAR_KEYS for general)}) of the loaded fixture."""
    refs = {"names": [str(n) for n in z["refs"]]}
    for n in refs["names"]:
        refs[n] = (z[f"ref_{n}__pac"], int(z[f"ref_{n}__l_pac"]))
    names = [str(n) for n in z["sets"]]
    groups = {n: {} for n in names}
    for k in IN_KEYS + OUT_KEYS:
        cuts = np.concatenate([[0], np.cumsum(z[k + "__n"])])
        for i, n in enumerate(names):
            groups[n][k] = z[k][cuts[i]:cuts[i + 1]]
    for g in groups.values():
        for k in ("ref", "pw", "zdrop"):
            g[k] = g[k][0]
    groups["general"].update({k: z[f"general__{k}"] for k in CIGAR_KEYS})
    return refs, groups


def counts(g, out):
    """What test_fixture_is_consistent asserts, as a dict."""
    st, en = out["stop"], out["end"]
    c = {f"stop{v}_{'lr'[s]}": int((st[:, s] == v).sum()) for v in (1, 2, 3, 4) for s in (0, 1)}
    c.update({f"end{v}_{'lr'[s]}": int((en[:, s] == v).sum()) for v in (1, 2) for s in (0, 1)})
    sd, ql = g["seeds"], np.repeat(np.repeat(g["qlen"], np.diff(g["rco"])), np.diff(g["cso"]))
    at0, at1 = sd[:, 1] == 0, sd[:, 1] + sd[:, 2] == ql
    c.update({"start_only": int((at0 & ~at1).sum()), "end_only": int((~at0 & at1).sum()), "both": int((at0 & at1).sum()),
              "zd": int(out["zd"].sum()), "skipped": int((out["fate"] == 1).sum()), "overlap_kept": int((out["fate"] == 2).sum()),
              "seedlen0_kept": int(out["by_seedlen0"].sum()), "by_earlier": int(out["by_earlier"].sum()),
              "code4": int((g["qry"] == 4).sum())})
    return c


def main():
    ref = ref_lib()
    if ref is None:
        sys.exit("oracle/_ref/libref_bwa.so is missing: run `make ref` first")
    refs, groups = build()
    data = {"refs": np.array(refs["names"]), "sets": np.array(SETS)}
    for n in refs["names"]:
        data[f"ref_{n}__pac"], data[f"ref_{n}__l_pac"] = refs[n][0], np.int64(refs[n][1])
    vals = {}
    for name in SETS:
        g = groups[name]
        out = run_group(ref, refs, g)
        vals[name] = {**g, **out}
        if name == "general":
            cg = run_cigars(ref, refs, {**g, **out}, out["regs"])
            for k in CIGAR_KEYS:
                data[f"general__{k}"] = cg[k]
        print(name, len(g["qlen"]), "reads", len(g["seeds"]), "seeds", len(out["regs"]), "regions",
              {k: v for k, v in counts(g, out).items() if v})
    # one array per key, the groups' arrays one after the other along the first axis (`<key>__n` their lengths):
    # a zip member per group and key would cost more than the data
    for k in IN_KEYS + OUT_KEYS:
        arrs = [np.atleast_1d(vals[name][k]) for name in SETS]
        data[k], data[k + "__n"] = np.concatenate(arrs), np.array([len(a) for a in arrs], np.int64)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
