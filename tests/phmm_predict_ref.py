"""numpy restatement of the PairHMM fallback predictor (csrc/phmm.hip phmm_predict): which testcases
the f32 pass may skip because their f32 result is expected to fall below MIN_ACCEPTED. Integer
arithmetic only, so the device's decisions are reproduced exactly.

The estimate of a testcase (read of R rows, haplotype of C columns), in units of 0.01 log10:
the cheapest ungapped diagonal d (row r against column r + d, both 0-based) among -63 .. C - R + 63,

    cost(d) = sum over rows inside the haplotype of W[class(q_r)] * mismatch(r, r + d)
              + overhang(rows left of column 0) + overhang(rows right of column C - 1)

with the classes q < 14, q < 28, else -> W = 140, 250, 390, a match costing nothing, an N on either
side matching, and overhang(n) = 450 + 100 * (n - 1) for n > 0 (an insertion opened at i = 45 and
extended at c = 10). The testcase is predicted when

    cost > 6412 - lc(C) + margin      (6412 = -100 * log10(1e-28 * 2^-120), lc(C) ~ 100 * log10(C))
"""
import numpy as np

W_CLASS = (140, 250, 390)
Q_CLASS = (14, 28)
OH_OPEN, OH_EXT = 450, 100
DIAG_PAD = 63
THRESH = 6412
MARGIN = -100         # kPredMargin: the smallest with false-positive cells <= 0.5 % of all cells
NO_DIAGONAL = 1 << 30
MAX_ROWS, MAX_COLS = 2046, 9400  # longer reads / haplotypes are never predicted
CODE = np.full(256, 0, np.uint8)
for _k, _ch in enumerate(b"ACTGN"):
    CODE[_ch] = _k


def lc(C):
    """~ 100 * log10(C): the position of C's top bit and its next 8 bits, times 100 * log10(2) / 256."""
    C = int(C)
    msb = C.bit_length() - 1
    l2 = (msb << 8) | (((C << (31 - msb)) & 0xFFFFFFFF) >> 23 & 0xFF)
    return (l2 * 7706) >> 16


def overhang(n):
    return np.where(n > 0, OH_OPEN + OH_EXT * (n - 1), 0)


def best_cost(rs, q, hap, weights=None):
    """The cheapest diagonal's cost. weights: per-row mismatch cost (default: the three classes)."""
    R, C = len(rs), len(hap)
    rc = CODE[np.frombuffer(rs, np.uint8)]
    hc = CODE[np.frombuffer(hap, np.uint8)]
    if weights is None:
        qq = np.frombuffer(q, np.uint8) & 127
        weights = np.where(qq < Q_CLASS[0], W_CLASS[0], np.where(qq < Q_CLASS[1], W_CLASS[1], W_CLASS[2]))
    d = np.arange(-DIAG_PAD, C - R + DIAG_PAD + 1)
    if len(d) == 0:
        return NO_DIAGONAL
    # P[r, c + DIAG_PAD]: the cost of row r against column c, 0 outside the haplotype; diagonal d of row
    # r is P's flat element r * (width + 1) + d + DIAG_PAD
    width = C + 2 * DIAG_PAD
    P = np.zeros((R, width), np.int32)
    mis = (rc[:, None] != hc[None, :]) & (rc[:, None] != 4) & (hc[None, :] != 4)
    P[:, DIAG_PAD:DIAG_PAD + C] = mis * np.asarray(weights, np.int32)[:, None]
    s = P.itemsize
    cost = np.lib.stride_tricks.as_strided(P, (R, len(d)), ((width + 1) * s, s)).sum(axis=0, dtype=np.int64)
    n_lo = np.minimum(R, np.maximum(0, -d))
    n_hi = np.minimum(R - n_lo, np.maximum(0, R + d - C))
    cost += overhang(n_lo) + overhang(n_hi)
    return int(cost.min())


def predicted(rs, q, hap, margin=MARGIN):
    R, C = len(rs), len(hap)
    if R > MAX_ROWS or C > MAX_COLS:
        return False
    return best_cost(rs, q, hap) > THRESH - lc(C) + margin


def predict_array(ta, margin=MARGIN):
    """Decisions for every testcase of a TestcaseArray (before the certificate and the gate)."""
    import ctypes
    out = np.zeros(ta.n, bool)
    a = ta.np_arr
    for k in range(ta.n):
        R, C = int(a["rslen"][k]), int(a["haplen"][k])
        out[k] = predicted(ctypes.string_at(int(a["rs"][k]), R), ctypes.string_at(int(a["q"][k]), R),
                           ctypes.string_at(int(a["hap"][k]), C), margin)
    return out
