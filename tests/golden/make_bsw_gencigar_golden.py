"""Regenerate tests/golden/bsw_gencigar_golden.npz: inputs and the outputs of bwa's bwa_gen_cigar2 and
bns_get_seq (oracle/_ref/libref_bwa.so, built from the reference tree by `make ref`) for what
tests/test_bsw_gencigar.py runs through gb_ref_fetch, gb_bsw_gen_cigar and gb_bsw_gen_cigar_retry.
Seeds are fixed: a rerun reproduces the file.

    python tests/golden/make_bsw_gencigar_golden.py

References (`refs` lists them; ref_<name>__pac holds bwa's 2-bit packing, ref_<name>__l_pac the length):
  l1, l5, l4096, l4099   random bases; l_pac % 4 is 1, 1, 0 and 3
  md                     the hand-made targets of the `md` group, one after the other
Fetch regions (fetch__ref, beg, end -> len, bytes): on l4096 and l4099 every combination of beg & 3 and
(end - beg) & 15, forward and reverse; regions touching 0, l_pac and 2 l_pac; end < beg; clamped at both
ends; bridging; whole strands of l1 and l5.
Pair groups (`sets`; each under one reference and one parameter set):
  strands           one locus as a forward and as a reverse region (the query reverse-complemented), the
                    query a copy with 5 % substitutions and 3 % indel events of 1-5 bases, 2 % N;
                    w in {0, 3, 100}
  shortcut          len2 == re - rb with w == 0 (bwa.c:141-149: no DP) and its neighbours: w == 1, and
                    the region one base longer or shorter
  md                a mismatch at position 0, adjacent mismatches, a deletion followed directly by a
                    mismatch, a leading and a trailing D run, a leading I, match runs of 9, 10, 99 and
                    100, all-mismatch, 1 x 1, 255 x 2047; each on both strands
  tiny              every region of l1, both strands, match and mismatch, w 0 and 1
  rejects           on l5: rb == re, rb > re, bridging l_pac, rb < 0, re > 2 l_pac, among good pairs
  skewed_asym       o_del 4, e_del 2, o_ins 7, e_ins 1
  skewed_zero_open  gap open 0, extension 2
  skewed_match2     match 2, mismatch -4
  retry             an insertion and a deletion of the same length k apart from each other, so that the
                    band |len1 - len2| + 3 of a small w is too narrow: mem_reg2aln's loop
                    (tools/bwa/bwamem.c:1154-1163) composed here from live bwa_gen_cigar2 calls;
                    truesc is the score at w = 4 params.w. Tries 1, 2 and 3 all occur.
A rejected pair has n_cigar 0, nm -1, no MD, and score -1: the reference leaves *score alone there, and
-1 is what it was given.
"""
import ctypes
import ctypes.util
import os
import re as regex
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_bwa.so")
OUT = os.path.join(HERE, "bsw_gencigar_golden.npz")
MAX_QLEN, MAX_TLEN = 255, 2047
PAIR_KEYS = ("ref", "qry", "qoff", "qlen", "rb", "re", "w", "pen", "mat", "pw")
OUT_KEYS = ("score", "n_cigar", "nm", "cigar", "md_len", "md")
RETRY_KEYS = ("truesc", "tries", "w_final")


def ref_lib():
    """(libref_bwa.so with bwa_gen_cigar2, bns_get_seq and ksw_global2 declared, libc free), or None
    when oracle/_ref is not built."""
    if not os.path.exists(REF_SO):
        return None
    lib = ctypes.CDLL(REF_SO)
    ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    ip = ctypes.POINTER(ci)
    lib.bwa_gen_cigar2.argtypes = [vp, ci, ci, ci, ci, ci, i64, vp, ci, vp, i64, i64, ip, ip, ip]
    lib.bwa_gen_cigar2.restype = vp
    lib.bns_get_seq.argtypes = [i64, vp, i64, i64, ctypes.POINTER(i64)]
    lib.bns_get_seq.restype = vp
    lib.ksw_global2.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ip, ctypes.POINTER(vp)]
    lib.ksw_global2.restype = ci
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.free.argtypes = [vp]
    libc.free.restype = None
    return lib, libc.free


def pack_pac(codes):
    """_set_pac (tools/bwa/bntseq.c:42): base l in byte l >> 2 at shift (~l & 3) << 1. One spare byte
    behind, as bwa allocates it (l_pac / 4 + 1)."""
    c = np.asarray(codes, np.uint8)
    c4 = np.zeros((len(c) // 4 + 1) * 4, np.uint8)
    c4[:len(c)] = c
    c4 = c4.reshape(-1, 4)
    return (c4[:, 0] << 6 | c4[:, 1] << 4 | c4[:, 2] << 2 | c4[:, 3]).astype(np.uint8)


def get_seq_one(ref, pac, l_pac, beg, end):
    """bns_get_seq: the bytes (uint8 array, empty for length 0)."""
    lib, free = ref
    n = ctypes.c_int64(-1)
    p = lib.bns_get_seq(int(l_pac), pac.ctypes.data, int(beg), int(end), ctypes.byref(n))
    out = np.zeros(0, np.uint8)
    if p:
        if n.value > 0:
            out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value,)).copy()
        free(p)
    return out


def gen_cigar2_one(ref, pac, l_pac, q, rb, re, w, pen, mat, want_cigar=True):
    """(score, ops uint32[], NM, MD bytes) of one bwa_gen_cigar2 call. The reference reverses the query in
    place and back, so it gets a copy; score goes in as -1."""
    lib, free = ref
    q = np.array(q, np.uint8)
    score, n, nm = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(-1)
    p = lib.bwa_gen_cigar2(mat.ctypes.data, int(pen[0]), int(pen[1]), int(pen[2]), int(pen[3]), int(w), int(l_pac),
                           pac.ctypes.data, len(q), q.ctypes.data, int(rb), int(re), ctypes.byref(score),
                           ctypes.byref(n) if want_cigar else None, ctypes.byref(nm) if want_cigar else None)
    ops, md = np.zeros(0, np.uint32), b""
    if p:
        if want_cigar:
            # the operations, then the NUL-terminated MD (bwa.c:171,196)
            ops = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n.value,)).copy()
            md = ctypes.string_at(p + 4 * n.value)
        free(p)
    return score.value, ops, nm.value, md


def ksw_global2_score(ref, q, t, w, pen, mat):
    lib, _ = ref
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    return lib.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, mat.ctypes.data, int(pen[0]), int(pen[1]),
                           int(pen[2]), int(pen[3]), int(w), None, None)


def queries_of(g):
    return [g["qry"][g["qoff"][p]:g["qoff"][p] + g["qlen"][p]] for p in range(len(g["w"]))]


def run_group(ref, refs, g, want_cigar=True):
    """Reference outputs of a pair group: dict of OUT_KEYS."""
    name = refs["names"][int(g["ref"])]
    pac, l_pac = refs[name]
    n = len(g["w"])
    out = {"score": np.zeros(n, np.int32), "n_cigar": np.zeros(n, np.int32), "nm": np.zeros(n, np.int32),
           "md_len": np.zeros(n, np.int32)}
    ops, mds = [], []
    for p, q in enumerate(queries_of(g)):
        s, o, nm, md = gen_cigar2_one(ref, pac, l_pac, q, g["rb"][p], g["re"][p], g["w"][p], g["pen"], g["mat"], want_cigar)
        out["score"][p], out["n_cigar"][p], out["nm"][p], out["md_len"][p] = s, len(o), nm, len(md)
        ops.append(o)
        mds.append(md)
    out["cigar"] = np.concatenate(ops) if ops else np.zeros(0, np.uint32)
    out["md"] = np.frombuffer(b"".join(mds), np.uint8).copy()
    return out


def run_retry(ref, refs, g):
    """mem_reg2aln's loop (bwamem.c:1154-1163) around live bwa_gen_cigar2 calls: OUT_KEYS + tries, w_final.
    A pair the reference rejects leaves the loop's score undefined there; it counts as final after one try."""
    name = refs["names"][int(g["ref"])]
    pac, l_pac = refs[name]
    n = len(g["w"])
    out = {k: np.zeros(n, np.int32) for k in ("score", "n_cigar", "nm", "md_len", "tries", "w_final")}
    ops, mds = [], []
    cap, a = int(g["pw"]) << 2, int(g["mat"][0])
    for p, q in enumerate(queries_of(g)):
        w2, last_sc, i = int(g["w"][p]), -(1 << 30), 0
        while True:
            w2 = min(w2, cap)
            s, o, nm, md = gen_cigar2_one(ref, pac, l_pac, q, g["rb"][p], g["re"][p], w2, g["pen"], g["mat"])
            used = w2
            i += 1
            if len(o) == 0 and nm == -1:
                break
            if s == last_sc or w2 == cap:
                break
            last_sc = s
            w2 <<= 1
            if not (i < 3 and s < int(g["truesc"][p]) - a):
                break
        out["score"][p], out["n_cigar"][p], out["nm"][p], out["md_len"][p] = s, len(o), nm, len(md)
        out["tries"][p], out["w_final"][p] = i, used
        ops.append(o)
        mds.append(md)
    out["cigar"] = np.concatenate(ops) if ops else np.zeros(0, np.uint32)
    out["md"] = np.frombuffer(b"".join(mds), np.uint8).copy()
    return out


def scmat(a=1, b=4, ambig=-1):
    m = np.full((5, 5), ambig, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(-1)


def revcomp(q):
    q = np.asarray(q, np.uint8)[::-1]
    return np.where(q < 4, 3 - q, q).astype(np.uint8)


def mutate(rng, t, sub=0.05, indel=0.03, n_rate=0.0):
    """A query from target bases t: substitutions and indel events of 1-5 bases; 1 to MAX_QLEN long."""
    out, k = [], 0
    while k < len(t):
        r = rng.random()
        if r < indel / 2:
            k += int(rng.integers(1, 6))
            continue
        if r < indel:
            out.extend(rng.integers(0, 4, int(rng.integers(1, 6))).tolist())
        out.append(int(rng.integers(0, 4)) if rng.random() < sub else int(t[k]))
        k += 1
    if not out:
        out.append(int(rng.integers(0, 4)))
    q = np.array(out[:MAX_QLEN], np.uint8)
    q[rng.random(len(q)) < n_rate] = 4
    return q


def pack(ref_idx, pairs, pen=(6, 1, 6, 1), mat=None, pw=100):
    """Group dict from [(query, rb, re, w)]."""
    ql = np.array([len(q) for q, _, _, _ in pairs], np.int32)
    qoff = np.zeros(len(pairs), np.int64)
    qoff[1:] = np.cumsum(ql)[:-1]
    return {"ref": np.int32(ref_idx), "qry": np.concatenate([np.asarray(q, np.uint8) for q, _, _, _ in pairs]),
            "qoff": qoff, "qlen": ql, "rb": np.array([b for _, b, _, _ in pairs], np.int64),
            "re": np.array([e for _, _, e, _ in pairs], np.int64), "w": np.array([w for _, _, _, w in pairs], np.int32),
            "pen": np.array(pen, np.int32), "mat": scmat() if mat is None else mat, "pw": np.int32(pw)}


def both_strands(l_pac, q, s, e, w):
    """The forward region [s, e) with q, and the same locus as a reverse region with q reverse-complemented."""
    return [(q, s, e, w), (revcomp(q), 2 * l_pac - e, 2 * l_pac - s, w)]


def build_refs():
    rng = np.random.default_rng(200)
    codes = {f"l{n}": rng.integers(0, 4, n).astype(np.uint8) for n in (1, 5, 4096, 4099)}
    return codes


def strands(rng, codes, n_loci, ws=(0, 3, 100)):
    L = len(codes)
    pairs = []
    spans = [(0, 40), (L - 37, L), (0, 1), (L - 1, L)]
    while len(spans) < n_loci:
        ln = int(rng.integers(2, 260))
        s = int(rng.integers(0, L - ln))
        spans.append((s, s + ln))
    for s, e in spans:
        q = mutate(rng, codes[s:e], n_rate=0.02)
        for w in ws:
            pairs += both_strands(L, q, s, e, w)
    return pairs


def shortcut(rng, codes, n_loci):
    L = len(codes)
    pairs = []
    for k in range(n_loci):
        ln = int(rng.integers(8, 250))
        s = int(rng.integers(1, L - ln - 1))
        q = mutate(rng, codes[s:s + ln + 12])[:ln]  # equal length, yet with indels inside
        if len(q) < ln:
            q = np.concatenate([q, codes[s + len(q):s + ln]])
        cases = [(q, s, s + ln, 0), (q, s, s + ln, 1), (q, s, s + ln + 1, 0), (q, s + 1, s + ln, 0)]
        for c in cases:
            pairs.append(both_strands(L, *c)[k & 1])
    return pairs


def md_cases(rng):
    """[(label, query, target, w)]; the targets become the `md` reference."""
    T = lambda n: rng.integers(0, 4, n).astype(np.uint8)  # noqa: E731
    other = lambda b: np.uint8((int(b) + 1 + int(rng.integers(0, 3))) & 3)  # noqa: E731
    cases = []
    t = T(30)
    q = t.copy()
    q[0] = other(t[0])
    cases.append(("mm_at_0", q, t, 0))
    cases.append(("mm_at_0_dp", q, t, 5))
    t = T(40)
    q = t.copy()
    q[10], q[11], q[39] = other(t[10]), other(t[11]), other(t[39])
    cases.append(("adjacent_mm", q, t, 0))
    cases.append(("adjacent_mm_dp", q, t, 5))
    t = np.concatenate([T(40), np.array([0, 0, 0], np.uint8), T(40)])
    t[39], t[43] = 1, 1
    q = np.concatenate([t[:40], t[43:]])
    q[40] = 2  # the base right behind the deletion
    cases.append(("del_then_mm", q, t, 10))
    t = T(80)
    cases.append(("lead_trail_D", t[5:-4].copy(), t, 50))
    cases.append(("lead_I", np.concatenate([T(3), t]), t, 50))
    t = T(9 + 1 + 10 + 1 + 99 + 1 + 100)
    q = t.copy()
    for at in (9, 20, 120):
        q[at] = other(t[at])
    cases.append(("digit_counts", q, t, 0))
    cases.append(("digit_counts_dp", q, t, 7))
    t = T(20)
    q = ((t + 1 + rng.integers(0, 3, 20)) & 3).astype(np.uint8)
    cases.append(("all_mm", q, t, 0))
    cases.append(("all_mm_dp", q, t, 3))
    t = T(1)
    cases.append(("one_by_one_match", t.copy(), t, 0))
    cases.append(("one_by_one_mm", np.array([other(t[0])], np.uint8), t, 0))
    cases.append(("one_by_one_dp", np.array([other(t[0])], np.uint8), t, 1))
    t = T(MAX_TLEN)
    cases.append(("255x2047", mutate(rng, t[900:1200])[:255], t, MAX_TLEN))
    return cases


def rejects(l):
    """On a reference of l bases; queries are arbitrary."""
    q = lambda n: (np.arange(n) & 3).astype(np.uint8)  # noqa: E731
    return [(q(5), 0, l, 3), (q(3), 2, 2, 3), (q(3), 4, 1, 3), (q(5), l, 2 * l, 0), (q(4), l - 2, l + 2, 3),
            (q(2), 1, l - 1, 0), (q(4), -1, 3, 3), (q(4), 2 * l - 3, 2 * l + 1, 3), (q(3), l + 1, 2 * l - 1, 1),
            (q(6), 0, l + 1, 3), (q(1), 0, 1, 0), (q(3), -2, -1, 0), (q(1), 2 * l - 1, 2 * l, 0), (q(2), 2 * l, 2 * l + 2, 0)]


def retry_pairs(rng, codes):
    """(pairs, ks): an insertion and a deletion of k bases 40+ bases apart; k == 0 is a plain copy."""
    L = len(codes)
    pairs, ks = [], []
    for k, w0 in [(0, 2), (0, 400), (0, 1000), (2, 2), (4, 2), (4, 1), (7, 2), (7, 3), (12, 2), (30, 2), (30, 5), (9, 100),
                  (5, 4), (16, 3), (3, 0)] * 2:
        ln = int(rng.integers(150, 240))
        s = int(rng.integers(0, L - ln))
        t = codes[s:s + ln]
        a, b = int(rng.integers(20, 50)), int(rng.integers(110, 140))
        q = np.concatenate([t[:a], rng.integers(0, 4, k).astype(np.uint8), t[a:b], t[b + k:]])
        q[rng.random(len(q)) < 0.02] = 0
        pairs.append(both_strands(L, q, s, s + ln, w0)[len(pairs) & 1])
        ks.append(k)
    pairs.append((np.zeros(4, np.uint8), 4000, 4200, 3))  # bridging: rejected inside the loop
    return pairs


def build(ref=None):
    """(refs, fetch, groups): everything but the reference's outputs."""
    codes = build_refs()
    rng = np.random.default_rng(201)
    cases = md_cases(rng)
    codes["md"] = np.concatenate([t for _, _, t, _ in cases])
    names = list(codes)
    refs = {"names": names}
    for n in names:
        refs[n] = (pack_pac(codes[n]), len(codes[n]))
    ridx = {n: i for i, n in enumerate(names)}

    # fetch regions
    fr, fb, fe = [], [], []

    def add(name, b, e):
        fr.append(ridx[name]), fb.append(b), fe.append(e)
    for name in ("l4096", "l4099"):
        L = len(codes[name])
        for b3 in range(4):
            for ln in range(16):
                b = 100 + 4 * ln + b3
                add(name, b, b + 32 + ln)                       # forward
                add(name, 2 * L - (b + 32 + ln), 2 * L - b)     # the same bases on the reverse strand
                add(name, L + b, L + b + ln)                    # short reverse regions (ln == 0: empty)
        for b, e in [(0, 17), (L - 17, L), (L, L + 17), (2 * L - 17, 2 * L), (0, L), (L, 2 * L), (50, 20), (L + 50, L + 20),
                     (-5, 30), (2 * L - 30, 2 * L + 9), (-10, -3), (2 * L + 1, 2 * L + 5), (L - 3, L + 3), (0, 2 * L),
                     (L - 1, L), (L, L + 1), (7, 7), (3000, 5500 if name == "l4096" else 4090)]:
            add(name, b, e)
    for name in ("l1", "l5"):
        L = len(codes[name])
        for b, e in [(0, L), (L, 2 * L), (0, 2 * L), (0, 1), (2 * L - 1, 2 * L), (-1, L), (L, 2 * L + 3), (L, 0)]:
            add(name, b, e)
    fetch = {"ref": np.array(fr, np.int32), "beg": np.array(fb, np.int64), "end": np.array(fe, np.int64)}

    g = {}
    g["strands"] = pack(ridx["l4099"], strands(np.random.default_rng(202), codes["l4099"], 60))
    g["shortcut"] = pack(ridx["l4096"], shortcut(np.random.default_rng(203), codes["l4096"], 70))
    mdp, at = [], 0
    Lm = len(codes["md"])
    for _, q, t, w in cases:
        mdp += both_strands(Lm, q, at, at + len(t), w)
        at += len(t)
    g["md"] = pack(ridx["md"], mdp)
    c1 = codes["l1"]
    tiny = []
    for q in (c1.copy(), ((c1 + 1) & 3).astype(np.uint8), np.array([4], np.uint8)):
        for w in (0, 1):
            tiny += [(q, 0, 1, w), (q, 1, 2, w)]
    g["tiny"] = pack(ridx["l1"], tiny)
    g["rejects"] = pack(ridx["l5"], rejects(5))
    sk = strands(np.random.default_rng(204), codes["l4099"], 16)
    g["skewed_asym"] = pack(ridx["l4099"], sk, pen=(4, 2, 7, 1))
    g["skewed_zero_open"] = pack(ridx["l4099"], sk, pen=(0, 2, 0, 2))
    g["skewed_match2"] = pack(ridx["l4099"], sk, mat=scmat(2, 4, -1))
    g["retry"] = pack(ridx["l4096"], retry_pairs(np.random.default_rng(205), codes["l4096"]))
    return refs, fetch, g, [c[0] for c in cases]


def md_strings(g, out):
    off = np.concatenate([[0], np.cumsum(out["md_len"])])
    return [out["md"][off[p]:off[p + 1]].tobytes().decode() for p in range(len(g["w"]))]


def cigar_strings(out):
    off = np.concatenate([[0], np.cumsum(out["n_cigar"])])
    return ["".join(f"{int(o) >> 4}{'MID'[int(o) & 15]}" for o in out["cigar"][off[p]:off[p + 1]])
            for p in range(len(out["n_cigar"]))]


def main():
    ref = ref_lib()
    if ref is None:
        sys.exit(f"{REF_SO} not built: run `make ref` where the reference tree exists")
    refs, fetch, groups, labels = build()
    out = {"refs": np.array(refs["names"]), "sets": np.array(list(groups)), "md_labels": np.array(labels)}
    for n in refs["names"]:
        out[f"ref_{n}__pac"], out[f"ref_{n}__l_pac"] = refs[n][0], np.int64(refs[n][1])

    seqs = [get_seq_one(ref, *refs[refs["names"][r]], b, e) for r, b, e in zip(fetch["ref"], fetch["beg"], fetch["end"])]
    fetch["len"] = np.array([len(s) for s in seqs], np.int32)
    fetch["bytes"] = np.concatenate(seqs)
    for k, v in fetch.items():
        out[f"fetch__{k}"] = v
    print(f"fetch: {len(seqs)} regions, {len(fetch['bytes'])} bases, {int((fetch['len'] == 0).sum())} empty")

    for name, g in groups.items():
        if name == "retry":
            pac, l_pac = refs[refs["names"][int(g["ref"])]]
            g["truesc"] = np.array([gen_cigar2_one(ref, pac, l_pac, q, g["rb"][p], g["re"][p], int(g["pw"]) << 2, g["pen"],
                                                   g["mat"])[0] for p, q in enumerate(queries_of(g))], np.int32)
            o = run_retry(ref, refs, g)
            assert {1, 2, 3} <= set(o["tries"].tolist()), np.bincount(o["tries"])
            print("retry tries:", np.bincount(o["tries"]).tolist(), "final w:", sorted(set(o["w_final"].tolist())))
        else:
            o = run_group(ref, refs, g)
        assert (g["qlen"] >= 1).all() and (g["qlen"] <= MAX_QLEN).all() and (g["w"] >= 0).all()
        ok = o["n_cigar"] > 0
        assert ((g["re"] - g["rb"])[ok] <= MAX_TLEN).all()
        cs, ms = cigar_strings(o), md_strings(g, o)
        if name == "shortcut":
            pac, l_pac = refs[refs["names"][int(g["ref"])]]
            sc = (g["qlen"] == g["re"] - g["rb"]) & (g["w"] == 0)
            differ = 0
            for p in np.nonzero(sc)[0]:
                assert cs[p] == f"{g['qlen'][p]}M"
                t = get_seq_one(ref, pac, l_pac, g["rb"][p], g["re"][p])
                q = queries_of(g)[p]
                if g["rb"][p] >= l_pac:
                    t, q = t[::-1], q[::-1]
                differ += int(ksw_global2_score(ref, q, t, 3, g["pen"], g["mat"]) != o["score"][p])
            assert differ >= 10, differ
            print(f"shortcut: {int(sc.sum())} pairs on the shortcut, {differ} score differently from ksw_global2")
        if name == "md":
            by = {lab: (cs[2 * k], ms[2 * k], cs[2 * k + 1], ms[2 * k + 1]) for k, lab in enumerate(labels)}
            for lab, v in by.items():
                print(f"  {lab}: {v[0]} {v[1] if len(v[1]) < 50 else v[1][:47] + '...'} | rev {v[2]}")
            assert regex.match(r"0[ACGT]29$", by["mm_at_0"][1]) and regex.match(r"0[ACGT]", by["mm_at_0_dp"][1])
            assert regex.match(r"10[ACGT]0[ACGT]27[ACGT]0$", by["adjacent_mm"][1])
            assert regex.search(r"\^[ACGT]+0[ACGT]", by["del_then_mm"][1]), by["del_then_mm"]
            assert regex.match(r"5D71M4D$", by["lead_trail_D"][0]) and by["lead_trail_D"][1] == "71"
            assert by["lead_I"][0] == "3I80M" and by["lead_I"][1] == "80"
            assert regex.match(r"9[ACGT]10[ACGT]99[ACGT]100$", by["digit_counts"][1])
            assert regex.match(r"(0[ACGT]){20}0$", by["all_mm"][1])
            assert by["one_by_one_match"][:2] == ("1M", "1") and regex.match(r"0[ACGT]0$", by["one_by_one_mm"][1])
        if name == "rejects":
            assert (o["n_cigar"] == 0).sum() >= 7 and (o["score"][o["n_cigar"] == 0] == -1).all() and ok.sum() >= 5
        for key in PAIR_KEYS:
            out[f"{name}__{key}"] = g[key]
        for key in OUT_KEYS:
            out[f"{name}__{key}"] = o[key]
        if name == "retry":
            out["retry__truesc"], out["retry__tries"], out["retry__w_final"] = g["truesc"], o["tries"], o["w_final"]
        print(f"{name}: {len(g['w'])} pairs ({int((~ok).sum())} rejected), {len(o['cigar'])} operations, "
              f"{len(o['md'])} MD bytes, longest MD {int(o['md_len'].max())}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
