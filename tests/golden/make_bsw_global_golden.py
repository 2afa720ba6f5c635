"""Regenerate tests/golden/bsw_global_golden.npz: inputs and the outputs of bwa's ksw_global2
(oracle/_ref/libref_bwa.so, built from the reference tree by `make ref`) for the pair sets
tests/test_bsw_global.py runs through gb_bsw_global. Seeds are fixed: a rerun reproduces the file.

    python tests/golden/make_bsw_global_golden.py

Groups (each one set of pairs under one parameter set; `sets` in the file lists them):
  random            600 pairs, query 1-255 (every K boundary present) with 5 % N, target = query with
                    5 % substitutions and 3 % indel events of 1-5 bases, w = |len1-len2| + U[0,11]
  band_edges        query 1, 17, 64, 200: w = 0 on equal lengths, w = |len1-len2| exactly in both
                    directions, w >= qlen, and 2047 x 255
  ties              homopolymer and dinucleotide repeats with an indel: only the tie rules decide
  skewed_asym       o_del 4, e_del 2, o_ins 7, e_ins 1
  skewed_zero_open  gap open 0, extension 2
  skewed_mm20       mismatch -20, gaps 1+1 (adjacent I and D runs)
  skewed_default    1 x 1 pairs and other tiny shapes under the default scoring
  unrelated         random query against a random target of another length: long alternating gap runs
NM is counted from the CIGAR the way bwa_gen_cigar2 does (tools/bwa/bwa.c:169-200): mismatching
positions in M runs, the I runs, and the D runs that are neither the first nor the last operation.
"""
import ctypes
import ctypes.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_bwa.so")
OUT = os.path.join(HERE, "bsw_global_golden.npz")
K_BOUNDARIES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255)


def ref_lib():
    """(libref_bwa.so with ksw_global2 declared, libc free) or None when oracle/_ref is not built."""
    if not os.path.exists(REF_SO):
        return None
    lib = ctypes.CDLL(REF_SO)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.ksw_global2.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ctypes.POINTER(ci),
                                ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]
    lib.ksw_global2.restype = ci
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.free.argtypes = [vp]
    libc.free.restype = None
    return lib, libc.free


def ksw_global2_one(ref, q, t, w, pen, mat, want_cigar=True):
    """(score, ops uint32[]) of one pair; q, t contiguous uint8 code arrays, pen = o_del, e_del, o_ins, e_ins."""
    lib, free = ref
    n = ctypes.c_int(0)
    cg = ctypes.POINTER(ctypes.c_uint32)()
    score = lib.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, mat.ctypes.data, int(pen[0]), int(pen[1]),
                            int(pen[2]), int(pen[3]), int(w), ctypes.byref(n) if want_cigar else None,
                            ctypes.byref(cg) if want_cigar else None)
    ops = np.zeros(0, np.uint32)
    if want_cigar:
        ops = np.ctypeslib.as_array(cg, shape=(n.value,)).copy() if n.value else ops
        free(ctypes.cast(cg, ctypes.c_void_p))
    return score, ops


def nm_from_cigar(ops, q, t):
    """bwa.c:169-200."""
    x = y = nm = 0
    for k, o in enumerate(ops.tolist()):
        op, ln = o & 15, o >> 4
        if op == 0:
            nm += int((q[x:x + ln] != t[y:y + ln]).sum())
            x += ln
            y += ln
        elif op == 2:
            if 0 < k < len(ops) - 1:
                nm += ln
            y += ln
        else:
            x += ln
            nm += ln
    return nm


def run_group(ref, g, want_cigar=True):
    """Reference outputs of a group dict: score, n_cigar, nm int32 [n], flattened ops uint32."""
    n = len(g["w"])
    score, ncig, nm, ops = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32), []
    mat = np.ascontiguousarray(g["mat"], np.int8)
    for p in range(n):
        q = np.ascontiguousarray(g["qry"][g["qoff"][p]:g["qoff"][p] + g["qlen"][p]])
        t = np.ascontiguousarray(g["tgt"][g["toff"][p]:g["toff"][p] + g["tlen"][p]])
        score[p], o = ksw_global2_one(ref, q, t, g["w"][p], g["pen"], mat, want_cigar)
        if want_cigar:
            ncig[p] = len(o)
            nm[p] = nm_from_cigar(o, q, t)
            ops.append(o)
    return score, ncig, nm, (np.concatenate(ops) if ops else np.zeros(0, np.uint32))


def scmat(a=1, b=4, ambig=-1):
    m = np.full((5, 5), ambig, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(-1)


def pack(pairs, pen=(6, 1, 6, 1), mat=None):
    """Group dict from [(query, target, w)]."""
    ql = np.array([len(q) for q, _, _ in pairs], np.int32)
    tl = np.array([len(t) for _, t, _ in pairs], np.int32)
    qoff, toff = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int64)
    qoff[1:], toff[1:] = np.cumsum(ql)[:-1], np.cumsum(tl)[:-1]
    return {"qry": np.concatenate([np.asarray(q, np.uint8) for q, _, _ in pairs]),
            "tgt": np.concatenate([np.asarray(t, np.uint8) for _, t, _ in pairs]),
            "qoff": qoff, "toff": toff, "qlen": ql, "tlen": tl,
            "w": np.array([w for _, _, w in pairs], np.int32), "pen": np.array(pen, np.int32),
            "mat": scmat() if mat is None else mat}


def rand_seq(rng, n, n_rate=0.05):
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


def related(rng, n, qlens=(), qmax=255, slack=11):
    ql = list(qlens) + rng.integers(1, qmax + 1, n - len(qlens)).tolist()
    pairs = []
    for L in ql:
        q = rand_seq(rng, int(L))
        t = mutate(rng, q)
        pairs.append((q, t, abs(len(t) - len(q)) + int(rng.integers(0, slack + 1))))
    return pairs


def band_edges(rng):
    pairs = []
    for L in (1, 17, 64, 200):
        q = rand_seq(rng, L)
        t = q.copy()
        t[rng.random(L) < 0.1] = 0
        pairs.append((q, t, 0))  # one column per row
        for d in (1, 3):
            at = int(rng.integers(0, L + 1))
            longer = np.concatenate([q[:at], rng.integers(0, 4, d).astype(np.uint8), q[at:]])
            pairs.append((q, longer, d))  # the end cell on the band edge, target longer
            pairs.append((longer, q, d))  # ... and query longer (both lengths stay <= 255)
        pairs.append((q, mutate(rng, q), L + 5))  # no band: the direction row is qlen wide
        pairs.append((q, rand_seq(rng, L + 2), L + 2))
    q = rand_seq(rng, 255)
    big = np.concatenate([rand_seq(rng, 900), mutate(rng, q), rand_seq(rng, 2047)])[:2047]
    pairs.append((q, big, 2047 - 255))
    pairs.append((q, big, 2047))
    pairs.append((rand_seq(rng, 1), big, 2046))
    return pairs


def ties(rng):
    A = lambda n: np.zeros(n, np.uint8)  # noqa: E731
    pairs = [(A(20), A(17), 3), (A(17), A(20), 3)]  # 3I17M (score 8) and 3D17M
    for L in (5, 30, 64, 65, 130):
        for d in (1, 2, 3):
            for extra in (0, 1, 5):
                di = np.tile(np.array([0, 1], np.uint8), L)[:L]
                pairs.append((A(L + d), A(L), d + extra))
                pairs.append((A(L), A(L + d), d + extra))
                pairs.append((di, np.tile(np.array([0, 1], np.uint8), L)[:L + d], d + extra))
                pairs.append((np.tile(np.array([0, 1], np.uint8), L)[:L + d], di, d + extra))
    n4 = np.full(40, 4, np.uint8)
    pairs += [(n4, n4[:37], 3), (n4[:37], n4, 4), (A(8), A(8), 0), (A(8), A(8), 8)]
    return pairs


def unrelated(rng, n):
    pairs = []
    for _ in range(n):
        L, T = int(rng.integers(1, 256)), int(rng.integers(1, 401))
        if T == L:
            T += 1
        pairs.append((rand_seq(rng, L, 0.02), rand_seq(rng, T, 0.02), abs(T - L) + int(rng.integers(0, 41))))
    return pairs


def build_groups():
    g = {}
    g["random"] = pack(related(np.random.default_rng(101), 600, K_BOUNDARIES))
    g["band_edges"] = pack(band_edges(np.random.default_rng(102)))
    g["ties"] = pack(ties(np.random.default_rng(103)))
    sk = related(np.random.default_rng(104), 90, (1, 2, 64, 65, 128, 129, 192, 193, 255), qmax=160)
    g["skewed_asym"] = pack(sk, pen=(4, 2, 7, 1))
    g["skewed_zero_open"] = pack(sk, pen=(0, 2, 0, 2))
    g["skewed_mm20"] = pack(sk, pen=(1, 1, 1, 1), mat=scmat(1, 20, -1))
    one = lambda *c: np.array(c, np.uint8)  # noqa: E731
    g["skewed_default"] = pack([(one(0), one(1), 0), (one(2), one(2), 0), (one(0), one(1), 3), (one(0, 1), one(1), 1),
                                (one(3), one(0, 3, 3), 2), (one(4), one(4), 0)])
    g["unrelated"] = pack(unrelated(np.random.default_rng(105), 150))
    return g


def main():
    ref = ref_lib()
    if ref is None:
        sys.exit(f"{REF_SO} not built: run `make ref` where the reference tree exists")
    groups = build_groups()
    out = {"sets": np.array(list(groups))}
    counts = {0: 0, 1: 0, 2: 0}
    for name, g in groups.items():
        score, ncig, nm, ops = run_group(ref, g)
        # every CIGAR consumes exactly len2 query and len1 target bases
        off = np.concatenate([[0], np.cumsum(ncig)])
        for p in range(len(ncig)):
            o = ops[off[p]:off[p + 1]]
            ln, op = (o >> 4).astype(np.int64), o & 15
            assert ln[op != 2].sum() == g["qlen"][p] and ln[op != 1].sum() == g["tlen"][p], (name, p)
        for k in counts:
            counts[k] += int(((ops & 15) == k).sum())
        for key in ("qry", "tgt", "qoff", "toff", "qlen", "tlen", "w", "pen", "mat"):
            out[f"{name}__{key}"] = g[key]
        out[f"{name}__score"], out[f"{name}__n_cigar"], out[f"{name}__nm"], out[f"{name}__cigar"] = score, ncig, nm, ops
        print(f"{name}: {len(ncig)} pairs, {len(ops)} operations, longest CIGAR {int(ncig.max())}")
    print(f"runs: {counts[0]} M, {counts[1]} I, {counts[2]} D")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
