"""profile_hmm_align (benchmarks/abea/src/eventalign.c:703-911) restated in numpy and `math`: the contract of
gb_abea_hmm_align (include/gb_bsw_abea_viterbi.h).

The transitions are abea_hmm_ref.transitions (calculate_transitions is the same text in eventalign.c:171-240 and
hmm.c); every other operation is a float32 numpy operation in the reference's order. Unlike the library, this
file keeps the whole matrix: three values and three `from` codes per cell, filled by anti-diagonals (K reads its
own row's previous block), and the traceback reads l_fm out of it. That the library reproduces these values
without a matrix is therefore checked, not assumed.

align() also counts labels; tests/golden/make_abea_viterbi_golden.py checks this file against the live reference
on every fixture item and stores the counts.
"""
import math

import numpy as np

from abea_hmm_ref import F, NEG, K, transitions

SAME_M, PREV_M, SAME_B, PREV_B, PREV_K, SOFT = range(6)
ST_K, ST_B, ST_M = range(3)  # ProfileStateR9; ps2char is "KBM"[state]
LABELS = ("paths_with_k", "paths_with_b", "cells_all_neg_inf", "stride_up", "stride_down", "rank0_byte",
          "mm_self_neg_inf", "more_kmers_than_rows", "two_rows", "tie_cells", "tie_path_cells")
# tie_cells and tie_path_cells (two finite terms equal to the maximum) are counted and stored without a minimum
# The minima follow from the fixture's shape grid (11 k-mer counts x 6 row counts plus 5 x 2 long ones, on both
# strands: 76 items per strand, 39 shapes with more k-mers than rows, which force a 'K', 11 of two rows) and from
# the groups of four items each that plant an outlier every seventh row (a 'B' costs log 0.001, the emission 40 pA
# off far more), a byte other than ACGT, and events_per_base 1; K of k-mer 0 has six terms of -infinity in every row.
MINIMA = {"paths_with_k": 78, "paths_with_b": 4, "cells_all_neg_inf": 1000, "stride_up": 76, "stride_down": 76,
          "rank0_byte": 4, "mm_self_neg_inf": 4, "more_kmers_than_rows": 78, "two_rows": 22}

_RANK = np.zeros(256, np.int64)
for _i, _ch in enumerate(b"ACGT"):
    _RANK[_ch] = _i
_IS_ACGT = np.zeros(256, bool)
_IS_ACGT[list(b"ACGT")] = True


def kmer_ranks(seq, rc):
    """The k-mers in the order the reference visits them (eventalign.c:244-291, 434-446)."""
    c = _RANK[np.asarray(seq, np.uint8)]
    n = len(c) - K + 1
    r = np.zeros(n, np.int64)
    for i in range(K):
        r = r * 4 + c[i:i + n]
    return r[::-1].copy() if rc else r


def _fold(terms, em):
    """ProfileHMMViterbiOutputR9::update_cell (eventalign.c:621-633): (value, from, all six -infinity, two finite
    terms at the maximum)."""
    mx = terms[0]
    frm = np.zeros(len(mx), np.int64)
    for i in range(1, 6):
        mx = np.where(terms[i] > mx, terms[i], mx)
        frm = np.where(mx == terms[i], i, frm)
    at_max = sum((t == mx).astype(np.int64) for t in terms)
    return (mx + em).astype(F), frm, mx == NEG, (mx != NEG) & (at_max >= 2)


def align(model, seq, events, scale, shift, var, log_var, event_start, event_stop, rc, events_per_base, labels=None):
    """The records of one call: (event_idx int32, kmer_idx int32, state bytes, l_fm float32), in the reference's
    final order; `events` are the read's event means. With `labels` (a dict over LABELS) the labels of this call
    are added to it."""
    model = np.asarray(model, F)
    seq = np.asarray(seq, np.uint8)
    events = np.asarray(events, F)
    scale, shift, var, log_var = F(scale), F(shift), F(var), F(log_var)
    nk = len(seq) - K + 1
    n = abs(int(event_stop) - int(event_start)) + 1
    assert n >= 2  # eventalign.c:725
    stride = -1 if rc else 1
    T = transitions(events_per_base)
    soft0 = F(0.0) + F(math.log(1 - 0.5))  # lp_sm + pre_flank[0]
    ranks = kmer_ranks(seq, rc)
    gm = (scale * model[ranks, 0] + shift).astype(F)
    sd = (model[ranks, 1] * var).astype(F)
    c = (F(-0.918938) - (model[ranks, 2] + log_var).astype(F)).astype(F)
    V = np.full((3, n + 1, nk + 1), NEG, F)  # row 0 and block 0 (the start block) stay -infinity
    frm = np.full((3, n + 1, nk + 1), -1, np.int8)
    tie = np.zeros((3, n + 1, nk + 1), bool)
    all_neg = 0
    for t in range(1, n + nk):
        ki = np.arange(max(0, t - n), min(nk - 1, t - 1) + 1)
        r = t - ki
        neg = np.full(len(ki), NEG, F)
        zero = np.zeros(len(ki), F)
        x = events[int(event_start) + (r - 1) * stride]
        a = ((x - gm[ki]) / sd[ki]).astype(F)
        em = (c[ki] + (F(-0.5) * a * a).astype(F)).astype(F)
        soft = np.where((ki == 0) & (r == 1), soft0, NEG).astype(F)
        upM, upB = V[ST_M, r - 1, ki + 1], V[ST_B, r - 1, ki + 1]
        luM, luB, luK = V[ST_M, r - 1, ki], V[ST_B, r - 1, ki], V[ST_K, r - 1, ki]
        lM, lB, lK = V[ST_M, r, ki], V[ST_B, r, ki], V[ST_K, r, ki]  # this row's previous block: one step ago
        cells = (
            (ST_M, [T["mm_self"] + upM, T["mm_next"] + luM, T["bm_self"] + upB, T["bm_next"] + luB, T["km"] + luK, soft], em),
            (ST_B, [T["mb"] + upM, neg, T["bb"] + upB, neg, neg, neg], zero),
            (ST_K, [neg, T["mk"] + lM, neg, T["bk"] + lB, T["kk"] + lK, neg], zero))
        for st, terms, e in cells:
            v, f, an, tw = _fold([np.asarray(u, F) for u in terms], e)
            V[st, r, ki + 1], frm[st, r, ki + 1], tie[st, r, ki + 1] = v, f, tw
            all_neg += int(an.sum())
    # the traceback (eventalign.c:809-886)
    row, ki, st = n, nk - 1, ST_M
    out = []
    while row > 0:
        out.append((int(event_start) + (row - 1) * stride, ki, st, V[st, row, ki + 1], bool(tie[st, row, ki + 1])))
        move = int(frm[st, row, ki + 1])
        if move == SOFT:
            break
        ki -= int(move in (PREV_M, PREV_B, PREV_K))
        if st != ST_K:
            row -= 1
        st = ST_M if move <= PREV_M else ST_B if move <= PREV_B else ST_K
    out.reverse()
    states = np.array([b"KBM"[s:s + 1] for _, _, s, _, _ in out], "S1")
    if labels is not None:
        labels["paths_with_k"] += int((states == b"K").any())
        labels["paths_with_b"] += int((states == b"B").any())
        labels["cells_all_neg_inf"] += all_neg
        labels["stride_up" if stride == 1 else "stride_down"] += 1
        labels["rank0_byte"] += int((~_IS_ACGT[seq]).any())
        labels["mm_self_neg_inf"] += int(T["mm_self"] == NEG)
        labels["more_kmers_than_rows"] += int(nk > n)
        labels["two_rows"] += int(n == 2)
        labels["tie_cells"] += int(tie.sum())
        labels["tie_path_cells"] += sum(int(o[4]) for o in out)
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32), states,
            np.array([o[3] for o in out], F))


def align_item(x, i, labels=None):
    """align() of item i of a gen.AbeaAlignItems."""
    seq, ev, rd, it = x.item(i)
    assert int(it["flags"]) == 0
    return align(x.model, seq, ev, rd["scale"], rd["shift"], rd["var"], rd["log_var"], int(it["event_start"]),
                 int(it["event_stop"]), int(it["rc"]), float(rd["events_per_base"]), labels)
