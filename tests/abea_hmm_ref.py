"""profile_hmm_score (benchmarks/abea/src/hmm.c:301-727) restated in numpy and `math`: the contract of
gb_abea_hmm_score (include/gb_bsw_abea_hmm.h).

Everything the reference takes from libm goes through math.log / math.exp (libm's, in double) and is rounded to
float32 where the reference stores a float; every other operation is a float32 numpy operation in the
reference's order. The matrix is evaluated by anti-diagonals (K reads its own row's previous block, so a row is
a serial chain), one numpy operation over all k-mers per term; only two rows' worth of values are kept.

score() also counts labels over the cells inside the matrix; tests/golden/make_abea_hmm_golden.py checks this
file against the live reference on every fixture item and stores the counts.
"""
import math

import numpy as np

K = 6
TBL = 16000
PRE_CLIP, POST_CLIP = 1, 2
F = np.float32
NEG = F(-np.inf)
LABELS = ("cut_distance", "cut_neg_inf", "index_0", "index_15000", "mm_self_neg_inf", "m_kmer", "rank0_byte", "one_row",
          "more_kmers_than_rows", "stride_up", "stride_down")

_RANK = np.zeros(256, np.int64)
for _i, _ch in enumerate(b"ACGMT"):
    _RANK[_ch] = _i
_IS_ACGMT = np.zeros(256, bool)
_IS_ACGMT[list(b"ACGMT")] = True


def logsum_table():
    """p7_FLogsumInit (logsum.h:35-48)."""
    return np.array([math.log(1. + math.exp(-i / 1000.0)) for i in range(TBL)], np.float64).astype(F)


_TABLE = logsum_table()


def pre_flank(n):
    """make_pre_flanking (hmm.c:172-205): n + 1 values, sums in double, stored as float."""
    pre = [F(math.log(1 - 0.5)), F(math.log(0.5) + -3.0 + math.log(1 - 0.9))]
    for i in range(2, n + 1):
        pre.append(F(math.log(0.9) + -3.0 + float(pre[i - 1])))
    return np.array(pre[:n + 1], F)


def post_flank(n):
    """make_post_flanking (hmm.c:132-168), written out on its own: n values."""
    post = [F(0)] * n
    post[n - 1] = F(math.log(1 - 0.5))
    if n > 1:
        post[n - 2] = F(math.log(0.5) + -3.0 + math.log(1 - 0.9))
        for i in range(n - 3, -1, -1):
            post[i] = F(math.log(0.9) + -3.0 + float(post[i + 1]))
    return np.array(post, F)


def _flog(p):
    p = float(p)
    return F(math.log(p)) if p > 0 else (NEG if p == 0 else F(np.nan))


def transitions(events_per_base):
    """calculate_transitions (hmm.c:231-298): float probabilities, each stored as (float)log((double)p)."""
    p_stay = F(1 - (1 / events_per_base))
    p_skip, p_bad, p_skip_self = F(0.0025), F(0.001), F(0.3)
    p_mm_next = F(1.0) - p_stay - p_skip - p_bad
    p_bk = (F(1.0) - p_bad) / F(3)
    p_km = F(1.0) - p_skip_self
    return {"mm_self": _flog(p_stay), "mb": _flog(p_bad), "mk": _flog(p_skip), "mm_next": _flog(p_mm_next),
            "bb": _flog(p_bad), "bk": _flog(p_bk), "bm_next": _flog(p_bk), "bm_self": _flog(p_bk),
            "kk": _flog(p_skip_self), "km": _flog(p_km), "p_mm_next": p_mm_next}


def kmer_ranks(seq, rc):
    """The k-mers in the order the reference visits them (hmm.c:21-52, 382-393)."""
    c = _RANK[np.asarray(seq, np.uint8)]
    n = len(c) - K + 1
    r = np.zeros(n, np.int64)
    for i in range(K):
        r = r * 5 + c[i:i + n]
    return r[::-1].copy() if rc else r


def _logsum(a, b, valid, lab):
    """p7_FLogsum (logsum.h:61-71) over arrays; labels are counted where `valid`."""
    with np.errstate(invalid="ignore"):
        mx = np.where(a > b, a, b)
        mn = np.where(a < b, a, b)
        d = mx - mn
        by_inf = mn == NEG
        by_dist = ~by_inf & (d >= F(15.7))
        cut = by_inf | by_dist
        idx = (np.where(cut, F(0), d) * F(1000.)).astype(np.int32)
        out = np.where(cut, mx, mx + _TABLE[idx]).astype(F)
    if lab is not None:
        lab["cut_distance"] += int((by_dist & valid).sum())
        lab["cut_neg_inf"] += int((by_inf & valid).sum())
        lab["index_0"] += int((~cut & valid & (idx == 0)).sum())
        lab["index_15000"] += int((~cut & valid & (idx >= 15000)).sum())
    return out


def _fold(terms, em, valid, lab):
    """update_cell (hmm.c:558-566): six terms, folded from term 0, then the emission."""
    s = terms[0]
    for x in terms[1:]:
        s = _logsum(s, x, valid, lab)
    return (s + em).astype(F)


def score(model, seq, events, scale, shift, var, log_var, event_start, event_stop, rc, events_per_base, flags,
          labels=None):
    """The score of one call as float32; `events` are the read's event means. With `labels` (a dict over LABELS)
    the labels of this call are added to it."""
    model = np.asarray(model, F)
    seq = np.asarray(seq, np.uint8)
    events = np.asarray(events, F)
    scale, shift, var, log_var = F(scale), F(shift), F(var), F(log_var)
    nk = len(seq) - K + 1
    n = abs(int(event_stop) - int(event_start)) + 1
    stride = -1 if rc else 1
    T = transitions(events_per_base)
    pre, post = pre_flank(n), post_flank(n)
    # what lets the library keep one table indexed by distance: post_flank[i] == pre_flank[n - 1 - i], bit for bit
    assert (post.view(np.uint32) == pre[:n][::-1].view(np.uint32)).all()
    ranks = kmer_ranks(seq, rc)
    gm = (scale * model[ranks, 0] + shift).astype(F)
    sd = (model[ranks, 1] * var).astype(F)
    c = (F(-0.918938) - (model[ranks, 2] + log_var).astype(F)).astype(F)
    lab = labels
    if lab is not None:
        lab["mm_self_neg_inf"] += int(T["mm_self"] == NEG)
        lab["m_kmer"] += int((seq == ord("M")).any())  # the k-mers cover the whole string on either strand
        lab["rank0_byte"] += int((~_IS_ACGMT[seq]).any())
        lab["one_row"] += int(n == 1)
        lab["more_kmers_than_rows"] += int(nk > n)
        lab["stride_up" if stride == 1 else "stride_down"] += 1
    ki = np.arange(nk)
    neg = np.full(nk, NEG, F)
    zero = np.zeros(nk, F)
    M, B, Kk = neg.copy(), neg.copy(), neg.copy()  # each k-mer's last computed row
    lM1, lB1, lK1 = neg.copy(), neg.copy(), neg.copy()  # the previous k-mer's, one step earlier
    lp_end = np.array([NEG], F)
    one = np.array([True])
    for t in range(1, n + nk):
        r = t - ki  # k-mer ki is at row t - ki
        valid = (r >= 1) & (r <= n)
        rr = np.clip(r, 1, n)
        x = np.where(valid, events[int(event_start) + (rr - 1) * stride], F(0)).astype(F)
        # the previous k-mer's blocks: this row's (computed one step ago) and the row above (two steps ago)
        lM0, lB0, lK0 = (np.concatenate([[NEG], v[:-1]]).astype(F) for v in (M, B, Kk))
        soft = np.where((ki == 0) & valid & ((r == 1) | bool(flags & PRE_CLIP)), F(0.0) + pre[rr - 1], NEG).astype(F)
        a = ((x - gm) / sd).astype(F)
        em = (c + (F(-0.5) * a * a).astype(F)).astype(F)
        m = _fold([T["mm_self"] + M, T["mm_next"] + lM1, T["bm_self"] + B, T["bm_next"] + lB1, T["km"] + lK1, soft], em,
                  valid, lab)
        b = _fold([T["mb"] + M, neg, T["bb"] + B, neg, neg, neg], zero, valid, lab)
        k = _fold([neg, T["mk"] + lM0, neg, T["bk"] + lB0, T["kk"] + lK0, neg], zero, valid, lab)
        # rows outside 1..n hold -infinity (above) or nothing that a row inside reads (below)
        M, B, Kk = (np.where(r >= 1, v, NEG).astype(F) for v in (m, b, k))
        lM1, lB1, lK1 = lM0, lB0, lK0
        rl = t - (nk - 1)
        if 1 <= rl <= n and ((flags & POST_CLIP) or rl == n):
            for v in (M, B, Kk):
                lp_end = _logsum(lp_end, (F(0.0) + v[nk - 1:] + post[rl - 1]).astype(F), one, lab)
    return F(lp_end[0])


def score_item(x, i, labels=None):
    """score() of item i of a gen.AbeaHmmItems."""
    seq, ev, rd, it = x.item(i)
    return score(x.model, seq, ev, rd["scale"], rd["shift"], rd["var"], rd["log_var"], int(it["event_start"]),
                 int(it["event_stop"]), int(it["rc"]), float(rd["events_per_base"]), int(it["flags"]), labels)
