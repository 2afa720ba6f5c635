// chain_extd2_internal.h -- the arithmetic of gb_chain_extd2 (minimap2's ksw_extd2_sse), one text for the host
// path and the kernels of chain_extd2.hip: the call's constants, a row's bounds and edge values, the score of
// a column, the update of one cell, the bookkeeping after a row and the backtrack.
//
// The reference keeps seven int8 arrays of T16 = 16 * ceil(tlen / 16) bytes indexed by the target column
// (u v x y x2 y2 s), then the target padded with zeros to T16 and the reversed query followed by zeros, in one
// allocation. Both paths keep that block, byte for byte (offsets below): the reference writes a row's scores
// in 16-byte runs from the unaligned st0, which run past en0 into the padding, into the query, and past s[]
// into the first bytes of the target; and it updates the aligned range [st, en], so cells outside the band
// hold real bytes that cells inside read one row later. Every sum is 8-bit and wraps.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gb_chain_extd2.h"
#include "gb_common.h"

namespace gbx2 {

#define GB_HD __host__ __device__ __forceinline__

constexpr int32_t kNegInf = -0x40000000;  // KSW_NEG_INF

// The constants of a call (ksw2_extd2_sse.c:68-105 over ksw_gen_simple_mat's matrix).
struct Par {
  int8_t q, e, q2, e2;     // after the swap that makes q + e the smaller sum
  int8_t mch, mis, scn;    // mat[0], mat[1] and the wildcard's score
  int8_t nqe, nqe2;        // -q - e and -q2 - e2 as bytes: the arrays' initial value and the edges'
  int8_t qe8, qe28;        // q + e and q2 + e2 as bytes
  int8_t ne, ne2, ldiff;   // the first column's v and the diagonal's u below, at and above long_thres
  int32_t qe_pre;          // q + e before the swap: H of the first cell is v[0] - qe_pre
  int32_t long_thres;
  int32_t early;           // -min_sc > 2 * (q + e): every item returns the reset record
};

inline Par make_par(const gb_chain_extd2_params &p) {
  Par P;
  int a = p.a, b = p.b, amb = p.sc_ambi;
  const int8_t ma = (int8_t)(a < 0 ? -a : a), mb = (int8_t)(b > 0 ? -b : b), mn = (int8_t)(amb > 0 ? -amb : amb);
  int q = p.q, e = p.e, q2 = p.q2, e2 = p.e2;
  P.qe_pre = q + e;
  if (q2 + e2 < q + e) std::swap(q, q2), std::swap(e, e2);
  P.q = (int8_t)q, P.e = (int8_t)e, P.q2 = (int8_t)q2, P.e2 = (int8_t)e2;
  P.mch = ma, P.mis = mb, P.scn = mn == 0 ? (int8_t)(-e2) : mn;
  P.nqe = (int8_t)(-q - e), P.nqe2 = (int8_t)(-q2 - e2), P.qe8 = (int8_t)(q + e), P.qe28 = (int8_t)(q2 + e2);
  const int min_sc = std::min((int)ma, std::min((int)mb, (int)mn));
  P.early = -min_sc > 2 * (q + e);
  int lt = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;
  if (q2 + e2 + lt * e2 > q + e + lt * e) ++lt;
  P.long_thres = lt;
  P.ne = (int8_t)(-e), P.ne2 = (int8_t)(-e2), P.ldiff = (int8_t)(lt * (e - e2) - (q2 - q) - e2);
  return P;
}

GB_HD int w8(int v) { return (int)(int8_t)v; }
GB_HD int round16(int v) { return (v + 15) / 16 * 16; }
// n_col_: the 16-byte blocks of a row of backtrack codes; w is the band after `w < 0` became max(qlen, tlen)
GB_HD int n_col(int qlen, int tlen, int w) {
  const int n = qlen < tlen ? qlen : tlen;
  return ((n < w + 1 ? n : w + 1) + 15) / 16 + 1;
}
GB_HD int eff_w(int qlen, int tlen, int w) {
  if (w < 0) w = tlen > qlen ? tlen : qlen;
  return w > 4 * GB_EXTD2_MAX_LEN ? 4 * GB_EXTD2_MAX_LEN : w;  // beyond qlen + tlen every band is the same band
}

// the block's arrays, as byte offsets
struct Lay {
  int T16, Q16;
  GB_HD int u() const { return 0; }
  GB_HD int v() const { return T16; }
  GB_HD int x() const { return 2 * T16; }
  GB_HD int y() const { return 3 * T16; }
  GB_HD int x2() const { return 4 * T16; }
  GB_HD int y2() const { return 5 * T16; }
  GB_HD int s() const { return 6 * T16; }
  GB_HD int sf() const { return 7 * T16; }
  GB_HD int qr() const { return 8 * T16; }
  GB_HD int bytes() const { return 8 * T16 + Q16 + 16; }  // kcalloc(tlen_ * 8 + qlen_ + 1, 16)
};
GB_HD Lay make_lay(int qlen, int tlen) { return Lay{round16(tlen), round16(qlen)}; }
// the block and the 32-bit H[] of T16 entries behind it
GB_HD int64_t state_bytes(int qlen, int tlen) {
  const Lay L = make_lay(qlen, tlen);
  return (int64_t)L.bytes() + 4 * (int64_t)L.T16;
}

struct Row {
  int st0, en0, st, en;  // the band's columns, and the aligned range the row updates
};
// false when the band has left the matrix (st > en): the reference sets zdropped and stops
GB_HD bool row_bounds(int r, int qlen, int tlen, int w, Row *R) {
  int st = 0, en = tlen - 1;
  if (st < r - qlen + 1) st = r - qlen + 1;
  if (en > r) en = r;
  if (st < (r - w + 1) >> 1) st = (r - w + 1) >> 1;
  if (en > (r + w) >> 1) en = (r + w) >> 1;
  if (st > en) return false;
  R->st0 = st, R->en0 = en, R->st = st / 16 * 16, R->en = (en + 16) / 16 * 16 - 1;
  return true;
}
// v of the column left of column 0, and u of the diagonal cell, in row r
GB_HD int edge_gap(const Par &P, int r) {
  return r == 0 ? P.nqe : r < P.long_thres ? P.ne : r == P.long_thres ? P.ldiff : P.ne2;
}
// the score the reference's blend leaves for a target byte and a query byte (whatever bytes they are)
GB_HD int score_of(const Par &P, int tb, int qb) {
  return (tb == 4 || qb == 4) ? P.scn : tb == qb ? P.mch : P.mis;
}

// One cell (__dp_code_block1, the left- or right-aligning choice, __dp_code_block2): z is its score, xl vl x2l
// the row above's x, v, x2 one column to the left, ut yt y2t the row above's u, y, y2 of this column.
// Returns the backtrack code.
template <bool RIGHT>
GB_HD unsigned cell(const Par &P, int z, int xl, int vl, int x2l, int ut, int yt, int y2t, int *nu, int *nv, int *nx,
                    int *ny, int *nx2, int *ny2) {
  int a = w8(xl + vl), b = w8(yt + ut), a2 = w8(x2l + vl), b2 = w8(y2t + ut);
  unsigned d;
  if (!RIGHT) {
    d = a > z ? 1u : 0u, z = a > z ? a : z;
    d = b > z ? 2u : d, z = b > z ? b : z;
    d = a2 > z ? 3u : d, z = a2 > z ? a2 : z;
    d = b2 > z ? 4u : d, z = b2 > z ? b2 : z;
  } else {
    d = z > a ? 0u : 1u, z = a > z ? a : z;
    d = z > b ? d : 2u, z = b > z ? b : z;
    d = z > a2 ? d : 3u, z = a2 > z ? a2 : z;
    d = z > b2 ? d : 4u, z = b2 > z ? b2 : z;
  }
  z = z < P.mch ? z : P.mch;
  *nu = w8(z - vl), *nv = w8(z - ut);
  int t = w8(z - P.q);
  a = w8(a - t), b = w8(b - t);
  t = w8(z - P.q2);
  a2 = w8(a2 - t), b2 = w8(b2 - t);
  const bool ca = RIGHT ? a >= 0 : a > 0, cb = RIGHT ? b >= 0 : b > 0;
  const bool ca2 = RIGHT ? a2 >= 0 : a2 > 0, cb2 = RIGHT ? b2 >= 0 : b2 > 0;
  *nx = w8((ca ? a : 0) - P.qe8), *ny = w8((cb ? b : 0) - P.qe8);
  *nx2 = w8((ca2 ? a2 : 0) - P.qe28), *ny2 = w8((cb2 ? b2 : 0) - P.qe28);
  return d | (ca ? 0x08u : 0u) | (cb ? 0x10u : 0u) | (ca2 ? 0x20u : 0u) | (cb2 ? 0x40u : 0u);
}

// ksw_apply_zdrop with is_rot = 1
GB_HD bool apply_zdrop(gb_chain_extd2_result *ez, int32_t H, int r, int t, int zdrop, int e) {
  if (H > ez->max) {
    ez->max = H, ez->max_t = t, ez->max_q = r - t;
  } else if (t >= ez->max_t && r - t >= ez->max_q) {
    const int tl = t - ez->max_t, ql = (r - t) - ez->max_q, l = tl > ql ? tl - ql : ql - tl;
    if (zdrop >= 0 && ez->max - H > zdrop + l * e) {
      ez->zdropped = 1;
      return true;
    }
  }
  return false;
}
GB_HD void reset_result(gb_chain_extd2_result *ez) {
  ez->max_q = ez->max_t = ez->mqe_t = ez->mte_q = -1;
  ez->max = 0, ez->score = ez->mqe = ez->mte = kNegInf;
  ez->n_cigar = 0, ez->zdropped = 0, ez->reach_end = 0, ez->pad = 0;
}

// The rank that decides among equal H in a row (ksw2_extd2_sse.c:329-357): the cell en0 first, then the four
// strided maxima over st0 .. en1-1 in lane order, each keeping its first column, then en1 .. en0-1 in order.
GB_HD int tie_rank(int t, int st0, int en0) {
  const int en1 = st0 + (en0 - st0) / 4 * 4;
  return t == en0 ? 0 : ((t < en1 ? 1 + ((t - st0) & 3) : 5) << 16) | t;
}

// What follows a row's sweep with the exact maximum (lines 359-366). True when the sweep stops.
GB_HD bool after_row_exact(const Par &P, gb_chain_extd2_result *ez, int r, const Row &R, int qlen, int tlen, int zdrop,
                           int32_t max_H, int max_t, int32_t H_en0, int32_t H_st0) {
  if (R.en0 == tlen - 1 && H_en0 > ez->mte) ez->mte = H_en0, ez->mte_q = r - R.en;
  if (r - R.st0 == qlen - 1 && H_st0 > ez->mqe) ez->mqe = H_st0, ez->mqe_t = R.st0;
  if (apply_zdrop(ez, max_H, r, max_t, zdrop, P.e2)) return true;
  if (r == qlen + tlen - 2 && R.en0 == tlen - 1) ez->score = H_en0;
  return false;
}
// The same with KSW_EZ_APPROX_MAX (lines 367-383): one cell is followed; u8 and v8 are the row's new bytes.
template <typename U8>
GB_HD bool after_row_approx(const Par &P, gb_chain_extd2_result *ez, int r, const Row &R, int qlen, int tlen, int zdrop,
                            int flag, const U8 *u8, const U8 *v8, int32_t *H0, int *last) {
  if (r > 0) {
    const int t = *last;
    if (t >= R.st0 && t <= R.en0 && t + 1 >= R.st0 && t + 1 <= R.en0) {
      const int d0 = (int8_t)v8[t], d1 = (int8_t)u8[t + 1];
      if (d0 > d1) *H0 += d0;
      else *H0 += d1, ++*last;
    } else if (t >= R.st0 && t <= R.en0) {
      *H0 += (int8_t)v8[t];
    } else {
      ++*last, *H0 += (int8_t)u8[*last];
    }
  } else {
    *H0 = (int8_t)v8[0] - P.qe_pre, *last = 0;
  }
  if ((flag & GB_EXTD2_APPROX_DROP) && apply_zdrop(ez, *H0, r, *last, zdrop, P.e2)) return true;
  if (r == qlen + tlen - 2 && R.en0 == tlen - 1) ez->score = *H0;
  return false;
}

// Where the backtrack starts (lines 389-398); sets reach_end. False: no walk.
GB_HD bool walk_start(gb_chain_extd2_result *ez, int qlen, int tlen, int end_bonus, int flag, int *i0, int *j0) {
  if (!ez->zdropped && !(flag & GB_EXTD2_EXTZ_ONLY)) {
    *i0 = tlen - 1, *j0 = qlen - 1;
  } else if (!ez->zdropped && (flag & GB_EXTD2_EXTZ_ONLY) && ez->mqe + end_bonus > ez->max) {
    ez->reach_end = 1;
    *i0 = ez->mqe_t, *j0 = qlen - 1;
  } else if (ez->max_t >= 0 && ez->max_q >= 0) {
    *i0 = ez->max_t, *j0 = ez->max_q;
  } else {
    return false;
  }
  return true;
}

// ksw_backtrack with is_rot = 1 and min_intron_len = 0 over codes p (rows of ncol16 bytes, a row's first byte
// is its aligned st). The words are left in walk order; the caller reverses them unless REV_CIGAR asks for
// that order. Every step lowers i, j or both, so at most i0 + j0 + 2 <= qlen + tlen words are written.
GB_HD int walk(const uint8_t *p, int64_t ncol16, int qlen, int tlen, int w, int i0, int j0, uint32_t *cigar) {
  int n = 0, i = i0, j = j0, state = 0;
  auto push = [&](uint32_t op, int len) {
    if (n == 0 || op != (cigar[n - 1] & 0xf))
      cigar[n++] = (uint32_t)len << 4 | op;
    else
      cigar[n - 1] += (uint32_t)len << 4;
  };
  while (i >= 0 && j >= 0) {
    const int r = i + j;
    Row R;
    (void)row_bounds(r, qlen, tlen, w, &R);  // a row at or before the start cell's was swept
    int force = -1;
    if (i < R.st) force = 2;
    if (i > R.en) force = 1;
    const unsigned tmp = force < 0 ? p[(int64_t)r * ncol16 + (i - R.st)] : 0u;
    if (state == 0) state = tmp & 7;
    else if (!(tmp >> (state + 2) & 1)) state = 0;
    if (state == 0) state = tmp & 7;
    if (force >= 0) state = force;
    if (state == 0) push(0, 1), --i, --j;
    else if (state == 1 || state == 3) push(2, 1), --i;
    else push(1, 1), --j;
  }
  if (i >= 0) push(2, i + 1);
  if (j >= 0) push(1, j + 1);
  return n;
}

}  // namespace gbx2
