"""numpy restatement of the abea contract: f5c's CPU align() (benchmarks/abea/src/align.c:169-548) with the
library's definition of the no_end_cell case (include/gb_bsw_abea.h). One band at a time, vectorised over its 100
offsets; f32 and f64 exactly where the reference has them. Beyond align()'s pairs and count it returns what
the reference computes but does not hand back (max_gap, spanned, sum_emission, fills, the end cell) and counts
labels: which situations a read exercised.

Used by tests/golden/make_abea_golden.py to record the fixture (and checked there against the live
reference), and by tests/test_abea.py for freshly generated reads.
"""
import numpy as np

K, BW, HALF = 6, 100, 50
FROM_D, FROM_U, FROM_L = 0, 1, 2
F32, F64 = np.float32, np.float64
NEG = F32(-np.inf)

LABELS = ("tie_u", "tie_l", "alternate", "move_right", "move_down", "clamp_kmer_min", "clamp_event_min",
          "clamp_kmer_max", "clamp_event_max", "trim_cell", "trim_past_events", "qc_emission_only", "qc_gap_only",
          "walk_ends_kmer", "walk_ends_event")
# Not among them, because no input that passes the call's checks reaches them (abea): a filled cell
# whose three scores are all -infinity, a read without an end cell, and a QC failure by `spanned` alone.


def kmer_ranks(bases):
    code = np.zeros(256, np.int64)
    code[ord("C")], code[ord("G")], code[ord("T")] = 1, 2, 3
    c = code[np.asarray(bases, np.uint8)]
    n = len(c) - K + 1
    r = np.zeros(n, np.int64)
    for i in range(K):
        r = r * 4 + c[i:i + n]
    return r


def consts(n_events, n_kmers):
    """align.c:196-205 in double; numpy's log and exp of a double are libm's."""
    import math
    events_per_kmer = float(n_events) / n_kmers
    p_stay = 1 - (1 / (events_per_kmer + 1))
    lp_skip = math.log(1e-10)
    lp_stay = math.log(p_stay)
    lp_step = math.log(1.0 - math.exp(lp_skip) - math.exp(lp_stay))
    lp_trim = math.log(0.01)
    return F64(lp_skip), F64(lp_stay), F64(lp_step), F64(lp_trim)


def emission(x, mean, stdv, log_stdv, scale, shift):
    """log_probability_match_r9 under CACHED_LOG (align.c:99-143): f32 throughout."""
    gp_mean = F32(scale) * mean + F32(shift)
    a = (x - gp_mean) / stdv
    return F32(-0.918938) - log_stdv + (F32(-0.5) * a * a)


def align(model, bases, events, scale=1.0, shift=0.0):
    """Returns a dict: n_pairs, n_raw, pairs (int32 [n_raw, 2] of (ref_pos, read_pos), final order), moves
    (uint8 per walk step, in walk order: the `from` of each visited cell), max_gap, spanned, end_event,
    no_end_cell, fills, end_score (f32), sum_emission (f64), labels (dict of counts)."""
    model = np.asarray(model, F32).reshape(4096, 3)
    events = np.asarray(events, F32)
    ranks = kmer_ranks(bases)
    n_events, n_kmers = len(events), len(ranks)
    assert n_events >= 1 and n_kmers >= 1
    lp_skip, lp_stay, lp_step, lp_trim = consts(n_events, n_kmers)
    n_bands = n_events + n_kmers + 2
    lab = dict.fromkeys(LABELS, 0)
    km_mean, km_stdv, km_ls = model[ranks, 0], model[ranks, 1], model[ranks, 2]
    o = np.arange(BW)
    trace = np.zeros((n_bands, BW), np.uint8)
    kll = np.zeros(n_bands, np.int64)
    # bands padded by one -inf cell on either side: index offset + 1
    Q = np.full(BW + 2, NEG, F32)
    P = np.full(BW + 2, NEG, F32)
    e_b, k_b = HALF - 1, -1 - HALF
    kll[0] = k_b
    Q[HALF + 1] = F32(0.0)
    e_b += 1
    kll[1] = k_b
    P[HALF + 1] = F32(lp_trim)
    trace[1, HALF] = FROM_U
    fills = 0
    best, best_ev = NEG, 0
    r_prev = 0
    with np.errstate(all="ignore"):
        for b in range(2, n_bands):
            ll, ur = P[1], P[BW]
            if ll == NEG and ur == NEG:
                right = b % 2 == 1
                lab["alternate"] += 1
            else:
                right = bool(ll < ur)
            if right:
                k_b += 1
                lab["move_right"] += 1
            else:
                e_b += 1
                lab["move_down"] += 1
            kll[b] = k_b
            r = int(right)
            N = np.full(BW + 2, NEG, F32)
            trim_off = -1 - k_b
            if 0 <= trim_off < BW:
                event_idx = e_b - trim_off
                if 0 <= event_idx < n_events:
                    N[trim_off + 1] = F32(lp_trim * F64(event_idx + 1))
                    trace[b, trim_off] = FROM_U
                    lab["trim_cell"] += 1
                else:
                    lab["trim_past_events"] += int(event_idx >= n_events)
            kmin, emin = -k_b, e_b - (n_events - 1)
            kmax, emax = n_kmers - k_b, e_b + 1
            min_off = max(kmin, emin, 0)
            max_off = min(kmax, emax, BW)
            if max_off > min_off:
                lab["clamp_kmer_min"] += int(kmin > 0 and kmin >= emin)
                lab["clamp_event_min"] += int(emin > 0 and emin > kmin)
                lab["clamp_kmer_max"] += int(kmax < BW and kmax <= emax)
                lab["clamp_event_max"] += int(emax < BW and emax < kmax)
                oo = o[min_off:max_off]
                ev_i, km_i = e_b - oo, k_b + oo
                up = P[oo + r + 1]          # offset_up = offset + (move b was right)
                left = P[oo + r]            # offset_left = offset_up - 1
                diag = Q[oo + r + r_prev]   # offset_diag = offset - 1 + (right moves among b - 1, b)
                em = emission(events[ev_i], km_mean[km_i], km_stdv[km_i], km_ls[km_i], scale, shift)
                score_d = (diag.astype(F64) + lp_step + em.astype(F64)).astype(F32)
                score_u = (up.astype(F64) + lp_stay + em.astype(F64)).astype(F32)
                score_l = (left.astype(F64) + lp_skip).astype(F32)
                m = score_d.copy()
                f = np.zeros(len(oo), np.uint8)
                m = np.where(score_u > m, score_u, m)
                f = np.where(m == score_u, FROM_U, f)
                m2 = np.where(score_l > m, score_l, m)
                f = np.where(m2 == score_l, FROM_L, f)
                finite = m2 > NEG
                lab["tie_u"] += int(np.count_nonzero(finite & (score_u == score_d) & (f == FROM_U)))
                lab["tie_l"] += int(np.count_nonzero(finite & (score_l == m) & (f == FROM_L)))
                N[oo + 1] = m2
                trace[b, oo] = f
                fills += len(oo)
            ev_end, o_end = b - 1 - n_kmers, n_kmers - 1 - k_b
            if 0 <= ev_end < n_events and 0 <= o_end < BW:
                s = F32(F64(N[o_end + 1]) + F64(n_events - ev_end) * lp_trim)
                if s > best:
                    best, best_ev = s, ev_end
            Q, P, r_prev = P, N, r
    out = dict(n_pairs=0, n_raw=0, pairs=np.zeros((0, 2), np.int32), moves=np.zeros(0, np.uint8), max_gap=0, spanned=0,
               end_event=int(best_ev), no_end_cell=0, fills=int(fills), end_score=F32(best), sum_emission=F64(0.0),
               labels=lab)
    if not best > NEG:
        out["no_end_cell"] = 1
        return out
    ev_i, km_i = int(best_ev), n_kmers - 1
    walk, moves = [], []
    gap = max_gap = 0
    s = F64(0.0)
    with np.errstate(all="ignore"):
        while km_i >= 0 and ev_i >= 0:
            walk.append((km_i, ev_i))
            s = s + F64(emission(events[ev_i], km_mean[km_i], km_stdv[km_i], km_ls[km_i], scale, shift))
            b = ev_i + km_i + 2
            off = km_i - kll[b]
            assert 0 <= off < BW, "the walk left its band"
            f = int(trace[b, off])
            moves.append(f)
            if f == FROM_D:
                km_i -= 1
                ev_i -= 1
                gap = 0
            elif f == FROM_U:
                ev_i -= 1
                gap = 0
            else:
                km_i -= 1
                gap += 1
                max_gap = max(gap, max_gap)
    lab["walk_ends_event"] = int(ev_i < 0)
    lab["walk_ends_kmer"] = int(km_i < 0 and ev_i >= 0)
    pairs = np.array(walk[::-1], np.int32).reshape(-1, 2)
    n = len(pairs)
    spanned = bool(pairs[0, 0] == 0 and pairs[-1, 0] == n_kmers - 1)
    avg = s / F64(n)
    why = [bool(avg < -5.0), not spanned, max_gap > 50]
    if sum(why) == 1:
        lab[("qc_emission_only", "qc_span_only", "qc_gap_only")[why.index(True)]] = 1
    assert not lab.pop("qc_span_only", 0), "a walk from a finite cell always ends at k-mer 0"
    out.update(n_raw=n, n_pairs=0 if any(why) else n, pairs=pairs, moves=np.array(moves, np.uint8), max_gap=int(max_gap),
               spanned=int(spanned), sum_emission=F64(s))
    return out


def pairs_from_moves(n_kmers, end_event, moves):
    """The final-order pairs of a walk stored as its end cell and one move per step."""
    moves = np.asarray(moves, np.int64)
    dk = (moves != FROM_U).astype(np.int64)
    de = (moves != FROM_L).astype(np.int64)
    km = (n_kmers - 1) - np.concatenate([[0], np.cumsum(dk[:-1])])
    ev = end_event - np.concatenate([[0], np.cumsum(de[:-1])])
    return np.stack([km, ev], 1)[::-1].astype(np.int32)
