"""Regenerate tests/golden/bsw_local_golden.npz: inputs and the outputs of bwa's ksw_align2
(oracle/_ref/libref_bwa.so, built from the reference tree by `make ref`) for the pair sets
tests/test_bsw_local.py runs through gb_bsw_local. Seeds are fixed: a rerun reproduces the file.

    python tests/golden/make_bsw_local_golden.py

Groups (each one set of pairs under one parameter set, xtra per pair; `sets` in the file lists them):
  random            600 pairs, query 1-255 (every multiple of 8 and of 16 with both neighbours, hence
                    every K boundary 64/65, 128/129, 192/193) with 2 % N, target = flank, mutated
                    copy, flank; xtra = XSUBO | XSTART | minsc, with XBYTE on most pairs that allow it
  two_hits          the target holds two mutated copies 0-250 bases apart: score2 is decided both
                    inside and outside te +- w
  pads              qlen % 16 == 1 under XBYTE and qlen % 8 == 1 without, the target holding only the
                    query's last 10-24 bases: after the hit's last row only the reference's padded
                    query columns carry the score, so they alone decide score2 / te2
  ties              homopolymers and dinucleotide repeats: te = first row, qe = smallest column, and
                    the entry-merge rule on long runs of equal row maxima
  no_hit            all-N query or all-N target, with and without XSUBO
  flags             the eight combinations of XSTOP, XSUBO, XSTART (XBYTE on every other pair), the
                    threshold 12-40 shared by XSTOP and XSUBO
  skewed_asym       o_del 4, e_del 2, o_ins 7, e_ins 1
  skewed_zero_open  gap open 0, extension 2: with o_ins == 0 the reference's lazy-F loop ends after its
                    first step, and F no longer crosses more than one stripe boundary of the striped
                    query; 4 of these pairs score below the ordinary DP
  skewed_zero_ins   o_del 3, e_del 1, o_ins 0, e_ins 2: that rule alone
  skewed_zero_del   o_del 0, e_del 2, o_ins 5, e_ins 1: a free deletion-open leaves the DP ordinary
  skewed_mm20       mismatch -20, gaps 1+1
  skewed_match2     match 2, mismatch -4
  edges             1 x 1, query lengths 1-255 against a target of 1, and 255 x 16383 (one pair)
Every pair lies inside gb_bsw_local's accepted domain (include/gb_bsw.h); main() asserts it.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_bwa.so")
OUT = os.path.join(HERE, "bsw_local_golden.npz")
XBYTE, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000  # tools/bwa/ksw.h:6-9
FIELDS = ("score", "te", "qe", "score2", "te2", "tb", "qb")
MAX_QLEN, MAX_TLEN = 255, 16383
# every multiple of 8 (hence of 16) below 256 with both neighbours, and 1, 2, 254, 255
QLEN_COVER = tuple(sorted({1, 2, 254, 255} | {m + d for m in range(8, 256, 8) for d in (-1, 0, 1)}))


class KswR(ctypes.Structure):  # kswr_t (tools/bwa/ksw.h:14-19)
    _fields_ = [(f, ctypes.c_int) for f in FIELDS]


def ref_lib():
    """libref_bwa.so with ksw_align2 declared, or None when oracle/_ref is not built."""
    if not os.path.exists(REF_SO):
        return None
    lib = ctypes.CDLL(REF_SO)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.ksw_align2.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp]
    lib.ksw_align2.restype = KswR
    return lib


def ksw_align2_one(lib, q, t, xtra, pen, mat):
    """The seven fields of one pair. The reference reverses both sequences in place and back, so it
    gets copies."""
    q, t = np.array(q, np.uint8), np.array(t, np.uint8)
    r = lib.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, mat.ctypes.data, int(pen[0]), int(pen[1]),
                       int(pen[2]), int(pen[3]), int(xtra), None)
    return [getattr(r, f) for f in FIELDS]


def run_group(lib, g):
    """Reference outputs of a group dict: int32 [n, 7] in FIELDS order."""
    n = len(g["xtra"])
    out = np.zeros((n, 7), np.int32)
    mat = np.ascontiguousarray(g["mat"], np.int8)
    for p in range(n):
        q = g["qry"][g["qoff"][p]:g["qoff"][p] + g["qlen"][p]]
        t = g["tgt"][g["toff"][p]:g["toff"][p] + g["tlen"][p]]
        out[p] = ksw_align2_one(lib, q, t, g["xtra"][p], g["pen"], mat)
    return out


def byte_ok(qlen, pen, mat):
    """Whether XBYTE is inside the accepted domain for a query of qlen bases."""
    return pen[0] + pen[1] <= 255 and pen[2] + pen[3] <= 255 and qlen * int(mat.max()) - int(mat.min()) < 255


def in_domain(g):
    pen, mat = g["pen"], g["mat"]
    ok = (pen >= 0).all() and pen[0] + pen[1] < 32768 and pen[2] + pen[3] < 32768
    ok = ok and mat.max() >= 1 and mat.min() <= 0 and g["qry"].max() <= 4 and g["tgt"].max() <= 4
    for p in range(len(g["xtra"])):
        x, ql, tl = int(g["xtra"][p]), int(g["qlen"][p]), int(g["tlen"][p])
        ok = ok and 1 <= ql <= MAX_QLEN and 1 <= tl <= MAX_TLEN and (x & ~(XBYTE | XSTOP | XSUBO | XSTART | 0xffff)) == 0
        ok = ok and (not (x & XBYTE) or byte_ok(ql, pen, mat))
        ok = ok and g["qoff"][p] + ql <= len(g["qry"]) and g["toff"][p] + tl <= len(g["tgt"])
    return bool(ok)


def scmat(a=1, b=4, ambig=-1):
    m = np.full((5, 5), ambig, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(-1)


def pack(pairs, pen=(6, 1, 6, 1), mat=None):
    """Group dict from [(query, target, xtra)]."""
    ql = np.array([len(q) for q, _, _ in pairs], np.int32)
    tl = np.array([len(t) for _, t, _ in pairs], np.int32)
    qoff, toff = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int64)
    qoff[1:], toff[1:] = np.cumsum(ql)[:-1], np.cumsum(tl)[:-1]
    return {"qry": np.concatenate([np.asarray(q, np.uint8) for q, _, _ in pairs]),
            "tgt": np.concatenate([np.asarray(t, np.uint8) for _, t, _ in pairs]),
            "qoff": qoff, "toff": toff, "qlen": ql, "tlen": tl,
            "xtra": np.array([x for _, _, x in pairs], np.int32), "pen": np.array(pen, np.int32),
            "mat": scmat() if mat is None else mat}


def rand_seq(rng, n, n_rate=0.02):
    s = rng.integers(0, 4, n).astype(np.uint8)
    s[rng.random(n) < n_rate] = 4
    return s


def mutate(rng, q, sub=0.05, indel=0.03):
    """q with substitutions and indel events of 1-5 bases; never empty."""
    out = []
    k = 0
    while k < len(q):
        r = rng.random()
        if r < indel / 2:
            k += int(rng.integers(1, 6))  # bases missing from the target
            continue
        if r < indel:
            out.extend(rng.integers(0, 4, int(rng.integers(1, 6))).tolist())  # bases only the target has
        out.append(int(rng.integers(0, 4)) if rng.random() < sub else int(q[k]))
        k += 1
    if not out:
        out.append(int(rng.integers(0, 4)))
    return np.array(out, np.uint8)


def flanked(rng, core, lo=0, hi=200):
    return np.concatenate([rand_seq(rng, int(rng.integers(lo, hi + 1))), core, rand_seq(rng, int(rng.integers(lo, hi + 1)))])


def with_byte(rng, x, qlen, pen, mat, prob=0.7):
    return x | (XBYTE if byte_ok(qlen, np.asarray(pen), mat) and rng.random() < prob else 0)


def related(rng, n, qlens=(), qmax=255, pen=(6, 1, 6, 1), mat=None, flank=200):
    mat = scmat() if mat is None else mat
    ql = list(qlens) + rng.integers(1, qmax + 1, max(0, n - len(qlens))).tolist()
    pairs = []
    for L in ql:
        q = rand_seq(rng, int(L))
        t = flanked(rng, mutate(rng, q, sub=float(rng.choice([0.0, 0.03, 0.08])), indel=0.03), 0, flank)
        minsc = int(rng.choice([0, 5, 10, 19, 30]))
        pairs.append((q, t, with_byte(rng, XSUBO | XSTART | minsc, int(L), pen, mat)))
    return pairs


def two_hits(rng, n):
    pairs = []
    for k in range(n):
        L = int(rng.integers(30, 151))
        q = rand_seq(rng, L)
        # distances around w = ceil(score / 1), that is about the query length, on both sides of it
        gap = int(rng.choice([0, 3, 10, 30, 60, 120, 250]))
        c1, c2 = mutate(rng, q, 0.04, 0.02), mutate(rng, q, 0.10, 0.03)
        if k % 3 == 0:  # the second copy is a part of the query only
            c2 = c2[int(rng.integers(0, L // 2)):][:int(rng.integers(20, L))]
        if k % 2:
            c1, c2 = c2, c1
        t = np.concatenate([rand_seq(rng, int(rng.integers(0, 60))), c1, rand_seq(rng, gap), c2,
                            rand_seq(rng, int(rng.integers(0, 60)))])
        pairs.append((q, t, with_byte(rng, XSUBO | XSTART | int(rng.integers(8, 20)), L, (6, 1, 6, 1), scmat(), 0.5)))
    return pairs


def pads(rng):
    pairs = []
    for byte in (True, False):
        p = 16 if byte else 8
        for L in range(p + 1, 250 if byte else 256, p):
            for rep in range(2 if byte else 1):
                q = rng.integers(0, 4, L).astype(np.uint8)
                s = int(rng.integers(10, 25))
                tail = q[max(0, L - s):]
                # the bases after the hit differ from nothing in particular: the pad columns score 0
                t = np.concatenate([rand_seq(rng, int(rng.integers(5, 80)), 0.0), tail,
                                    rand_seq(rng, int(rng.integers(5, 80)), 0.0)])
                pairs.append((q, t, XSUBO | XSTART | (XBYTE if byte else 0) | int(rng.integers(3, 10))))
    return pairs


def ties(rng):
    A = lambda n, b=0: np.full(n, b, np.uint8)  # noqa: E731
    di = lambda n: np.tile(np.array([0, 1], np.uint8), n)[:n]  # noqa: E731
    pairs = []
    for L in (1, 7, 8, 9, 16, 17, 40, 64, 65, 130, 200):
        for T in (1, 5, 40, 300):
            for minsc in (0, 1, 5, 19):
                base = XSUBO | XSTART | minsc
                pairs.append((A(L), A(T), base | (XBYTE if L % 2 else 0)))
                pairs.append((di(L), di(T), base | (0 if L % 2 else XBYTE)))
        pairs.append((di(L), np.concatenate([di(30), A(7, 2), di(45)]), XSUBO | XSTART | 3))
        pairs.append((A(L), np.concatenate([A(20), A(3, 1), A(60)]), XSUBO | XSTART | XBYTE | 2))
    return pairs


def no_hit(rng):
    N = lambda n: np.full(n, 4, np.uint8)  # noqa: E731
    pairs = []
    for L, T in ((1, 1), (5, 30), (17, 100), (64, 64), (130, 250), (255, 40)):
        for x in (XSUBO | XSTART, XSUBO | XSTART | 5, XSTART, 0, XSUBO, XSUBO | XSTART | XBYTE, XSTART | XBYTE):
            if (x & XBYTE) and L > 250:
                x &= ~XBYTE
            pairs.append((N(L), rand_seq(rng, T, 0.0), x))
            pairs.append((rand_seq(rng, L, 0.0), N(T), x))
            pairs.append((N(L), N(T), x))
    return pairs


def flags(rng):
    pairs = []
    for combo in range(8):
        base = (XSTOP if combo & 1 else 0) | (XSUBO if combo & 2 else 0) | (XSTART if combo & 4 else 0)
        for k in range(12):
            L = int(rng.integers(20, 201))
            q = rand_seq(rng, L)
            t = flanked(rng, mutate(rng, q, 0.05, 0.03), 0, 60)
            if k % 4 == 0:  # a second copy: rows past the forward XSTOP's stop that would score higher
                t = np.concatenate([q[L // 2:], rand_seq(rng, 15), t])
            pairs.append((q, t, base | (XBYTE if k % 2 else 0) | int(rng.integers(12, 41))))
    return pairs


def edges(rng):
    one = lambda *c: np.array(c, np.uint8)  # noqa: E731
    pairs = []
    for x in (0, XSTART, XSUBO | XSTART, XSUBO | XSTART | 1, XSUBO | XSTART | XBYTE, XSTOP | XSTART | 1):
        pairs += [(one(0), one(0), x), (one(0), one(1), x), (one(4), one(4), x), (one(2), one(4), x)]
    for L in (2, 8, 9, 16, 17, 64, 65, 255):
        q = rand_seq(rng, L, 0.0)
        for b in (int(q[0]), int(q[-1]), 4):
            pairs.append((q, one(b), XSUBO | XSTART | (XBYTE if L <= 250 else 0)))
            pairs.append((q, one(b), XSTART))
    q = rand_seq(rng, 255)
    big = np.concatenate([rand_seq(rng, 9000), mutate(rng, q), rand_seq(rng, 3000), mutate(rng, q[40:200], 0.1),
                          rand_seq(rng, MAX_TLEN)])[:MAX_TLEN]
    pairs.append((q, big, XSUBO | XSTART | 19))
    return pairs


def build_groups():
    g = {}
    g["random"] = pack(related(np.random.default_rng(201), 600, QLEN_COVER))
    g["two_hits"] = pack(two_hits(np.random.default_rng(202), 120))
    g["pads"] = pack(pads(np.random.default_rng(203)))
    g["ties"] = pack(ties(np.random.default_rng(204)))
    g["no_hit"] = pack(no_hit(np.random.default_rng(205)))
    g["flags"] = pack(flags(np.random.default_rng(206)))
    cover = (1, 8, 9, 16, 17, 64, 65, 120, 128, 129, 192, 193, 255)
    for name, pen, mat in (("skewed_asym", (4, 2, 7, 1), scmat()), ("skewed_zero_open", (0, 2, 0, 2), scmat()),
                           ("skewed_zero_ins", (3, 1, 0, 2), scmat()), ("skewed_zero_del", (0, 2, 5, 1), scmat()),
                           ("skewed_mm20", (1, 1, 1, 1), scmat(1, 20, -1)), ("skewed_match2", (6, 1, 6, 1), scmat(2, 4, -1))):
        g[name] = pack(related(np.random.default_rng(207), 60, cover, pen=pen, mat=mat, flank=80), pen=pen, mat=mat)
    g["edges"] = pack(edges(np.random.default_rng(208)))
    return g


def main():
    lib = ref_lib()
    if lib is None:
        sys.exit(f"{REF_SO} not built: run `make ref` where the reference tree exists")
    groups = build_groups()
    out = {"sets": np.array(list(groups))}
    for name, g in groups.items():
        assert in_domain(g), name
        r = run_group(lib, g)
        for key in ("qry", "tgt", "qoff", "toff", "qlen", "tlen", "xtra", "pen", "mat"):
            out[f"{name}__{key}"] = g[key]
        for k, f in enumerate(FIELDS):
            out[f"{name}__{f}"] = r[:, k].copy()
        print(f"{name}: {len(r)} pairs, longest target {int(g['tlen'].max())}, score2 >= 0 on {int((r[:, 3] >= 0).sum())}, "
              f"start found on {int((r[:, 5] >= 0).sum())}, XBYTE on {int(((g['xtra'] & XBYTE) != 0).sum())}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
