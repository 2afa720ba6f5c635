"""numpy restatement of the contract of gb_chain_extd2: minimap2's ksw_extd2_sse (tools/minimap2/ksw2_extd2_sse.c)
with m = 5 over ksw_gen_simple_mat's matrix, and ksw_backtrack (ksw2.h:119-151).

It keeps what the reference keeps: one block of int8 bytes holding u v x y x2 y2 s (each T16 = 16 * ceil(tlen / 16)
bytes), the target padded to T16 and the reversed query followed by zeros; a row writes its scores in 16-byte
runs from the unaligned st0 (past en0, into whatever lies there) and updates the aligned range [st, en]; sums
wrap at 8 bits; H[0] uses q + e from before the gap pairs swap. `keep_pad=True` is the one departure, a switch
that leaves the score bytes past en0 as they were: the label padding_sensitive counts the items whose outputs that
changes, which is how much of the contract lies outside the band.

align() returns (record, CIGAR words): the record is the tuple FIELDS of ksw_extz_t.
"""
import numpy as np

FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end", "n_cigar", "pad")
NEG_INF = -0x40000000
RIGHT, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR = 0x02, 0x08, 0x10, 0x40, 0x80

LABELS = ("padding_sensitive", "band_exit", "zdropped_by_score", "reach_end", "max_t_tie", "swapped", "early_return",
          "state_3_or_4_in_path", "forced_state", "right_differs")
# what tests/golden/make_chain_extd2_golden.py must reach, each well below what its seeded fixture yields
MINIMA = {"padding_sensitive": 40, "band_exit": 200, "zdropped_by_score": 50, "reach_end": 70, "max_t_tie": 100,
          "swapped": 20, "early_return": 16, "state_3_or_4_in_path": 40, "forced_state": 12, "right_differs": 300}


def i8(v):
    return np.array(int(v)).astype(np.int8)[()]


class Par:
    """The call's constants (ksw2_extd2_sse.c:68-105)."""

    def __init__(self, params):
        p = np.asarray(params).reshape(-1)[0]
        a, b, amb = int(p["a"]), int(p["b"]), int(p["sc_ambi"])
        ma, mb, mn = int(i8(-a if a < 0 else a)), int(i8(-b if b > 0 else b)), int(i8(-amb if amb > 0 else amb))
        q, e, q2, e2 = int(p["q"]), int(p["e"]), int(p["q2"]), int(p["e2"])
        self.qe_pre = q + e
        self.swapped = q2 + e2 < q + e
        if self.swapped:
            q, q2, e, e2 = q2, q, e2, e
        self.q, self.e, self.q2, self.e2 = q, e, q2, e2
        self.mch, self.mis, self.scn = i8(ma), i8(mb), i8(-e2 if mn == 0 else mn)
        self.nqe, self.nqe2, self.qe8, self.qe28 = i8(-q - e), i8(-q2 - e2), i8(q + e), i8(q2 + e2)
        self.q8, self.q28 = i8(q), i8(q2)
        self.early = -min(ma, mb, mn) > 2 * (q + e)
        lt = int((q2 - q) / (e - e2)) - 1 if e != e2 else 0  # C division truncates
        if q2 + e2 + lt * e2 > q + e + lt * e:
            lt += 1
        self.long_thres = lt
        self.ne, self.ne2, self.ldiff = i8(-e), i8(-e2), i8(lt * (e - e2) - (q2 - q) - e2)

    def edge_gap(self, r):
        return self.nqe if r == 0 else self.ne if r < self.long_thres else self.ldiff if r == self.long_thres else self.ne2


def row_bounds(r, qlen, tlen, w):
    st, en = max(0, r - qlen + 1, (r - w + 1) >> 1), min(tlen - 1, r, (r + w) >> 1)
    if st > en:
        return None
    return st, en, st // 16 * 16, (en + 16) // 16 * 16 - 1


def n_col(qlen, tlen, w):
    return (min(qlen, tlen, w + 1) + 15) // 16 + 1


def reset_record():
    return dict(max=0, zdropped=0, max_q=-1, max_t=-1, mqe=NEG_INF, mqe_t=-1, mte=NEG_INF, mte_q=-1, score=NEG_INF,
                reach_end=0, n_cigar=0, pad=0)


def apply_zdrop(ez, H, r, t, zdrop, e, labels):
    if H > ez["max"]:
        ez["max"], ez["max_t"], ez["max_q"] = H, t, r - t
    elif t >= ez["max_t"] and r - t >= ez["max_q"]:
        tl, ql = t - ez["max_t"], (r - t) - ez["max_q"]
        if zdrop >= 0 and ez["max"] - H > zdrop + abs(tl - ql) * e:
            ez["zdropped"] = 1
            if labels is not None:
                labels["zdropped_by_score"] += 1
            return True
    return False


def backtrack(codes, qlen, tlen, w, i0, j0, labels):
    """ksw_backtrack with is_rot = 1, min_intron_len = 0; the words in walk order."""
    out, i, j, state = [], i0, j0, 0
    long_state = forced = False

    def push(op, n):
        if out and out[-1] & 0xf == op:
            out[-1] += n << 4
        else:
            out.append(n << 4 | op)

    while i >= 0 and j >= 0:
        r = i + j
        _, _, st, en = row_bounds(r, qlen, tlen, w)
        force = -1
        if i < st:
            force = 2
        if i > en:
            force = 1
        tmp = int(codes[r][i - st]) if force < 0 else 0
        if state == 0:
            state = tmp & 7
        elif not (tmp >> (state + 2)) & 1:
            state = 0
        if state == 0:
            state = tmp & 7
        if force >= 0:
            state, forced = force, True
        long_state |= state in (3, 4)
        if state == 0:
            push(0, 1)
            i, j = i - 1, j - 1
        elif state in (1, 3):
            push(2, 1)
            i -= 1
        else:
            push(1, 1)
            j -= 1
    if i >= 0:
        push(2, i + 1)
    if j >= 0:
        push(1, j + 1)
    if labels is not None:
        labels["state_3_or_4_in_path"] += long_state
        labels["forced_state"] += forced
    return out


def align(params, query, target, w, zdrop, end_bonus, flag, keep_pad=False, labels=None):
    """ksw_extd2_sse(0, qlen, query, tlen, target, 5, mat, q, e, q2, e2, w, zdrop, end_bonus, flag, &ez) over
    codes 0..4: (tuple of FIELDS, uint32 CIGAR words). `labels` (a dict over LABELS) is counted into."""
    P = params if isinstance(params, Par) else Par(params)
    query, target = np.asarray(query, np.uint8), np.asarray(target, np.uint8)
    qlen, tlen = len(query), len(target)
    ez = reset_record()
    done = lambda cig=(): (tuple(ez[f] for f in FIELDS), np.array(cig, np.uint32))  # noqa: E731
    if qlen <= 0 or tlen <= 0 or P.early:
        if labels is not None and qlen > 0 and tlen > 0:
            labels["early_return"] += 1
        return done()
    if labels is not None:
        labels["swapped"] += P.swapped
    if w < 0:
        w = max(tlen, qlen)
    T16, Q16 = (tlen + 15) // 16 * 16, (qlen + 15) // 16 * 16
    ncol16 = n_col(qlen, tlen, w) * 16
    mem = np.zeros(8 * T16 + Q16 + 16, np.int8)
    u, v, x, y, x2, y2, s = (mem[k * T16:(k + 1) * T16] for k in range(7))
    for arr in (u, v, x, y):
        arr[:] = P.nqe
    x2[:], y2[:] = P.nqe2, P.nqe2
    S, SF, QR = 6 * T16, 7 * T16, 8 * T16
    mem[SF:SF + tlen] = target.view(np.int8)
    mem[QR:QR + qlen] = query[::-1].view(np.int8)
    H = np.full(T16, NEG_INF, np.int64)
    approx, right = bool(flag & APPROX_MAX), bool(flag & RIGHT)
    codes = []
    H0 = last = 0
    last_st = last_en = -1
    for r in range(qlen + tlen - 1):
        b = row_bounds(r, qlen, tlen, w)
        if b is None:
            ez["zdropped"] = 1
            if labels is not None:
                labels["band_exit"] += 1
            break
        st0, en0, st, en = b
        if labels is not None and "cells" in labels:  # the in-band cells of the rows reached (not a label)
            labels["cells"] += en0 - st0 + 1
        x1, x21, v1 = P.nqe, P.nqe2, P.nqe
        if st > 0:
            if last_st <= st - 1 <= last_en:
                x1, x21, v1 = x[st - 1], x2[st - 1], v[st - 1]
        else:
            v1 = P.edge_gap(r)
        if en >= r:
            y[r], y2[r], u[r] = P.nqe, P.nqe2, P.edge_gap(r)
        # the scores, in 16-byte runs from st0; a run reads the block as it is when the run starts
        qo = QR + qlen - 1 - r
        for t in range(st0, en0 + 1, 16):
            hi = min(t + 16, en0 + 1) if keep_pad else t + 16
            sq, sr = mem[SF + t:SF + hi], mem[qo + t:qo + hi]
            sc = np.where(sq == sr, P.mch, P.mis)
            mem[S + t:S + hi] = np.where((sq == 4) | (sr == 4), P.scn, sc)
        # the aligned range
        sl = slice(st, en + 1)
        z = s[sl].copy()
        xl = np.concatenate([[x1], x[st:en]]).astype(np.int8)
        vl = np.concatenate([[v1], v[st:en]]).astype(np.int8)
        x2l = np.concatenate([[x21], x2[st:en]]).astype(np.int8)
        ut = u[sl].copy()
        a, bb, a2, b2 = xl + vl, y[sl] + ut, x2l + vl, y2[sl] + ut
        if not right:
            d = (a > z).astype(np.uint8)
            z = np.maximum(z, a)
            for val, k in ((bb, 2), (a2, 3), (b2, 4)):
                d = np.where(val > z, np.uint8(k), d)
                z = np.maximum(z, val)
        else:
            d = np.where(z > a, np.uint8(0), np.uint8(1))
            z = np.maximum(z, a)
            for val, k in ((bb, 2), (a2, 3), (b2, 4)):
                d = np.where(z > val, d, np.uint8(k))
                z = np.maximum(z, val)
        z = np.minimum(z, P.mch)
        u[sl], v[sl] = z - vl, z - ut
        tmp = z - P.q8
        a, bb = a - tmp, bb - tmp
        tmp = z - P.q28
        a2, b2 = a2 - tmp, b2 - tmp
        zero = np.int8(0)
        for val, dst, sub, bit in ((a, x, P.qe8, 0x08), (bb, y, P.qe8, 0x10), (a2, x2, P.qe28, 0x20), (b2, y2, P.qe28, 0x40)):
            c = val >= 0 if right else val > 0
            dst[sl] = np.where(c, val, zero) - sub
            d = d | np.where(c, np.uint8(bit), np.uint8(0))
        codes.append(d.astype(np.uint8))
        assert len(d) <= ncol16
        if not approx:
            if r > 0:
                H_en0 = int(H[en0 - 1]) + int(u[en0]) if en0 > 0 else int(H[en0]) + int(v[en0])
                H[st0:en0] += v[st0:en0]
                H[en0] = H_en0
                max_H, max_t = H_en0, en0
                if en0 > st0:
                    cand = H[st0:en0]
                    m = int(cand.max())
                    if m > max_H:
                        t = np.arange(st0, en0)
                        en1 = st0 + (en0 - st0) // 4 * 4
                        rank = np.where(t < en1, 1 + ((t - st0) & 3), 5) * 65536 + t
                        max_H, max_t = m, int(rank[cand == m].min()) & 0xffff
                if labels is not None and max_H > ez["max"] and int((H[st0:en0 + 1] == max_H).sum()) > 1:
                    labels["max_t_tie"] += 1
            else:
                H[0] = int(v[0]) - P.qe_pre
                max_H, max_t = int(H[0]), 0
            if en0 == tlen - 1 and H[en0] > ez["mte"]:
                ez["mte"], ez["mte_q"] = int(H[en0]), r - en
            if r - st0 == qlen - 1 and H[st0] > ez["mqe"]:
                ez["mqe"], ez["mqe_t"] = int(H[st0]), st0
            if apply_zdrop(ez, max_H, r, max_t, zdrop, P.e2, labels):
                break
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez["score"] = int(H[tlen - 1])
        else:
            if r > 0:
                if st0 <= last <= en0 and st0 <= last + 1 <= en0:
                    d0, d1 = int(v[last]), int(u[last + 1])
                    if d0 > d1:
                        H0 += d0
                    else:
                        H0, last = H0 + d1, last + 1
                elif st0 <= last <= en0:
                    H0 += int(v[last])
                else:
                    last += 1
                    H0 += int(u[last])
            else:
                H0, last = int(v[0]) - P.qe_pre, 0
            if flag & APPROX_DROP and apply_zdrop(ez, H0, r, last, zdrop, P.e2, labels):
                break
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez["score"] = H0
        last_st, last_en = st, en
    if not ez["zdropped"] and not flag & EXTZ_ONLY:
        start = (tlen - 1, qlen - 1)
    elif not ez["zdropped"] and flag & EXTZ_ONLY and ez["mqe"] + end_bonus > ez["max"]:
        ez["reach_end"] = 1
        start = (ez["mqe_t"], qlen - 1)
    elif ez["max_t"] >= 0 and ez["max_q"] >= 0:
        start = (ez["max_t"], ez["max_q"])
    else:
        return done()
    if labels is not None:
        labels["reach_end"] += ez["reach_end"]
    cig = backtrack(codes, qlen, tlen, w, start[0], start[1], labels)
    if not flag & REV_CIGAR:
        cig = cig[::-1]
    ez["n_cigar"] = len(cig)
    return done(cig)


def align_item(x, i, **kw):
    """align() of item i of a gen.Extd2Items."""
    q, t, it = x.item(i)
    return align(x.params, q, t, int(it["w"]), int(it["zdrop"]), int(it["end_bonus"]), int(it["flag"]), **kw)


def walk_end(res, qlen, tlen, flag):
    """The cell (i0, j0) the reference's walk starts from for a finished record, or None."""
    r = dict(zip(FIELDS, res))
    if not r["zdropped"] and not flag & EXTZ_ONLY:
        return tlen - 1, qlen - 1
    if r["reach_end"]:
        return r["mqe_t"], qlen - 1
    if r["max_t"] >= 0 and r["max_q"] >= 0:
        return r["max_t"], r["max_q"]
    return None
