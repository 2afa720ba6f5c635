// bsw_abea_viterbi.hip -- gb_abea_hmm_align: Viterbi event alignment with traceback (f5c / nanopolish
// profile_hmm_align, eventalign.c:703-911).
//
// The matrix and the sweep are bsw_abea_hmm.hip's: rows (events) by k-mer blocks of three states K, B, M, M and B
// reading the row above and K its own row's previous block; a lane owns NK consecutive k-mers (1, 2, 4 by size
// class, or four items of at most 16 k-mers per wave) and at step t lane l computes row t - l, taking lane
// l-1's last block by a one-lane DPP shift. The fold of a cell's six terms is the reference's max/argmax
// (ProfileHMMViterbiOutputR9::update_cell, the last index winning among equals) instead of the log-sum, so there
// is no table and no LDS. No score is stored: a cell leaves its three `from` codes, 3 bits each, as one uint16
// at [step - 1][k-mer] of the item's part of a device workspace (row r of k-mer k is step r + k / NK), so that
// the stores of one step are one contiguous run per wave.
//
// A second kernel walks the codes, one lane per item, from (last row, last k-mer, M) until a cell that came
// from the start state, writing the records back to front at the end of the item's part of a record buffer
// sized by the bound rows + k-mers - 1. It then replays the finished path forwards: a path cell's value is
// (transition + value of the path cell before it) + emission in the fill's own f32 order, because the cell
// before it on the path is the term that won the maximum; that gives every l_fm bit for bit from 2 B per cell.
//
// A third kernel packs the records: the host scans the walked lengths (item order), and a wave per item copies
// the item's records to their final place in a second buffer, which is what comes back.
//
// A call's items are cut, in item order, into chunks whose codes and records (both buffers) fit a byte budget
// (GB_ABEA_VITERBI_WS, 1 GiB); inside a chunk the items are sorted by size class and rows and waves take slots
// from an atomic work counter. GB_ABEA_HOST=1 runs the plain C++ restatement below instead; both paths share
// the cell functions and the walk.
#include <cstring>

#include "../../include/gb_bsw_abea_viterbi.h"
#include "bsw_abea_hmm_internal.h"

namespace gbvit {

using namespace gbhmm;

constexpr int kWaves = 4;        // per block of the fill
constexpr int kBlocksPerCU = 8;  // of the fill: the persistent grid fills every wave slot the registers allow
constexpr int64_t kDefaultBudget = int64_t(1) << 30;
enum { kFromSameM = 0, kFromPrevM, kFromSameB, kFromPrevB, kFromPrevK, kFromSoft };  // HMMMovementType
enum { kStK = 0, kStB, kStM };                                                      // ProfileStateR9; code bits 3 * state

// ---- the arithmetic, one text for host and device ----

// update_cell (eventalign.c:621-633): the six terms in the order SAME_M, PREV_M, SAME_B, PREV_B, PREV_K, SOFT;
// among equal maxima the last index wins, and six terms of -infinity give SOFT
GB_HD float fold6(float x0, float x1, float x2, float x3, float x4, float x5, float em, unsigned *from) {
  const float x[6] = {x0, x1, x2, x3, x4, x5};
  float mx = x0;
  unsigned f = 0;
#pragma unroll
  for (unsigned i = 1; i < 6; ++i) {
    mx = x[i] > mx ? x[i] : mx;
    f = mx == x[i] ? i : f;
  }
  *from = f;
  return mx + em;
}

// M and B of a cell from the row above: `up` is this k-mer's block, `lu` the previous k-mer's
// (eventalign.c:509-537). Returns their codes at the states' bits.
GB_HD unsigned cell_mb(const Trans &T, const State &up, const State &lu, float soft, float em, float *m, float *b) {
  unsigned fm, fb;
  *m = fold6(T.mm_self + up.m, T.mm_next + lu.m, T.bm_self + up.b, T.bm_next + lu.b, T.km + lu.k, soft, em, &fm);
  *b = fold6(T.mb + up.m, kNegInf, T.bb + up.b, kNegInf, kNegInf, kNegInf, 0.0f, &fb);
  return fm << (3 * kStM) | fb << (3 * kStB);
}
// K of a cell from the previous k-mer's block of the same row (eventalign.c:541-548)
GB_HD unsigned cell_k(const Trans &T, const State &left, float *k) {
  unsigned fk;
  *k = fold6(kNegInf, T.mk + left.m, kNegInf, T.bk + left.b, T.kk + left.k, kNegInf, 0.0f, &fk);
  return fk << (3 * kStK);
}
// the transition that `from` names for a cell of state st
GB_HD float trans_of(const Trans &T, int st, unsigned from) {
  if (st == kStM)
    return from == kFromSameM   ? T.mm_self
           : from == kFromPrevM ? T.mm_next
           : from == kFromSameB ? T.bm_self
           : from == kFromPrevB ? T.bm_next
                                : T.km;
  if (st == kStB) return from == kFromSameM ? T.mb : T.bb;
  return from == kFromPrevM ? T.mk : from == kFromPrevB ? T.bk : T.kk;
}

// get_rank / get_kmer_rank (eventalign.c:244-291): two bits per base, N and every other byte 0
GB_HD int base_rank4(char b) { return b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0; }
GB_HD int kmer_rank4(const char *s) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < kK; ++i) r = r * 4 + base_rank4(s[i]);
  return r;
}

// One item as the walk sees it. Row r of k-mer k left its codes at codes[(r + (k >> sh) - 1) * W + k].
struct WalkIn {
  const uint16_t *codes;
  const Model *model;
  const char *seq;
  const float *evs;  // row 1's event; row r's is evs[(r - 1) * stride]
  int W, sh, seq_len, rc, e_start, stride, n, nk;
  float scale, shift, var, log_var, soft0;
  Trans T;
};

// The traceback of eventalign.c:809-886, then the values. The records end at `end` (one past the last); returns
// their number, at most `bound`. Every step lowers the row, the k-mer or both, and a cell of k-mer 0 never names
// a previous block (its terms from there are -infinity, so SOFT wins the tie), so the loop's other two
// conditions only guard the buffers against codes that no fill wrote.
GB_HD int walk_item(const WalkIn &a, gb_abea_path_rec *end, int bound) {
  int r = a.n, k = a.nk - 1, st = kStM, cnt = 0;
  gb_abea_path_rec *p = end;
  while (r >= 1 && k >= 0 && cnt < bound) {
    const unsigned c = a.codes[(int64_t)(r + (k >> a.sh) - 1) * a.W + k];
    const unsigned from = (c >> (3 * st)) & 7u;
    gb_abea_path_rec rec;
    rec.event_idx = a.e_start + (r - 1) * a.stride, rec.kmer_idx = k, rec.l_fm = 0.f;
    rec.state = st == kStM ? 'M' : st == kStB ? 'B' : 'K';
    rec.pad[0] = (uint8_t)from, rec.pad[1] = 0, rec.pad[2] = 0;  // pad[0] holds the code until the replay below
    *--p = rec;
    ++cnt;
    if (from == kFromSoft) break;
    if (from == kFromPrevM || from == kFromPrevB || from == kFromPrevK) k -= 1;
    if (st != kStK) r -= 1;  // a k-mer skip is silent
    st = from <= kFromPrevM ? kStM : from <= kFromPrevB ? kStB : kStK;
  }
  float prev = kNegInf;
  for (int i = 0; i < cnt; ++i) {
    gb_abea_path_rec rec = p[i];
    const int row = (rec.event_idx - a.e_start) * a.stride + 1, ki = rec.kmer_idx;
    const int s = rec.state == 'M' ? kStM : rec.state == 'B' ? kStB : kStK;
    const unsigned from = rec.pad[0];
    const float x = from == kFromSoft ? (row == 1 && ki == 0 ? a.soft0 : kNegInf) : trans_of(a.T, s, from) + prev;
    float em = 0.0f;
    if (s == kStM)
      em = emission(a.evs[(int64_t)(row - 1) * a.stride],
                    make_kmer(a.model[kmer_rank4(kmer_at(a.seq, a.seq_len, a.rc, ki))], a.scale, a.shift, a.var, a.log_var));
    prev = x + em;
    rec.l_fm = prev, rec.pad[0] = 0;
    p[i] = rec;
  }
  return cnt;
}

// SOFT of (row 1, k-mer 0): lp_sm + pre_flank[0], with pre_flank[0] = (float)log(1 - 0.5) (eventalign.c:523)
static float soft0() { return 0.0f + (float)log(1 - 0.5); }

static inline int item_bound(const gb_abea_hmm_item &it) { return item_rows(it) + (it.seq_len - kK + 1) - 1; }

// ---- host path: the fill over two rolling rows, codes at [row - 1][k-mer] ----

struct HostScratch {
  std::vector<State> rows;
  std::vector<Kmer> kmers;
  std::vector<uint16_t> codes;
};

static int host_align(const Model *model, const char *seq, const gb_abea_hmm_item &it, const float *read_events,
                      const gb_abea_hmm_read &rd, const Trans &T, HostScratch *hs, gb_abea_path_rec *end) {
  const int nk = it.seq_len - kK + 1, n = item_rows(it), stride = it.rc ? -1 : 1;
  hs->kmers.resize((size_t)nk);
  for (int ki = 0; ki < nk; ++ki)
    hs->kmers[(size_t)ki] =
        make_kmer(model[kmer_rank4(kmer_at(seq, it.seq_len, it.rc, ki))], rd.scale, rd.shift, rd.var, rd.log_var);
  hs->rows.assign((size_t)2 * (nk + 1), State{kNegInf, kNegInf, kNegInf});  // block 0 is the start block
  hs->codes.resize((size_t)n * nk);
  State *prev = hs->rows.data(), *cur = prev + (nk + 1);
  const float *evs = read_events + it.event_start;
  for (int r = 1; r <= n; ++r) {
    const float x = evs[(int64_t)(r - 1) * stride];
    for (int ki = 0; ki < nk; ++ki) {
      const float soft = ki == 0 && r == 1 ? soft0() : kNegInf;
      State s;
      unsigned c = cell_mb(T, prev[ki + 1], prev[ki], soft, emission(x, hs->kmers[(size_t)ki]), &s.m, &s.b);
      c |= cell_k(T, cur[ki], &s.k);
      cur[ki + 1] = s;
      hs->codes[(size_t)(r - 1) * nk + ki] = (uint16_t)c;
    }
    std::swap(prev, cur);
  }
  WalkIn w;
  w.codes = hs->codes.data(), w.model = model, w.seq = seq, w.evs = evs;
  w.W = nk, w.sh = 31, w.seq_len = it.seq_len, w.rc = it.rc, w.e_start = it.event_start, w.stride = stride, w.n = n, w.nk = nk;
  w.scale = rd.scale, w.shift = rd.shift, w.var = rd.var, w.log_var = rd.log_var, w.soft0 = soft0(), w.T = T;
  return walk_item(w, end, item_bound(it));
}

// ---- device path ----

struct DItem {
  int64_t seq_off, ev_first;  // ev_first: the index of row 1's event in the events of the call
  int64_t ws_off, path_end;   // first code (in codes, a multiple of 8) and one past the last record, of the chunk's buffers
  int32_t seq_len, n_rows, out, rc;  // out: index into lens[], -1 for a filler
  int32_t e_start, bound;
  float scale, shift, var, log_var, lp_mm_self, lp_mm_next;
};

struct Args {
  const Model *model;
  const char *seqs;
  const float *events;
  const DItem *items;  // the fill: this launch's slots in order, one item each, or four with fillers at the end
  int64_t n_slots;     // the walk: the number of items, fillers included
  uint16_t *codes;
  gb_abea_path_rec *path, *packed;
  int32_t *lens;
  const int64_t *offs;  // the pack: where each item's records go, by the index that lens has
  unsigned int *next;
  float soft0;
  Trans T;
};

constexpr int lanes_shift(int nk_per_lane) { return nk_per_lane == 4 ? 2 : nk_per_lane == 2 ? 1 : 0; }
constexpr int class_nk(int c) { return c == 3 ? 4 : c == 2 ? 2 : 1; }
// codes of an item of class c: steps x W, rounded up so that the next item starts on 16 bytes
static inline int64_t item_codes(int c, int nk, int n) {
  const int NK = class_nk(c);
  return gb::round_up((int64_t)(n + (nk - 1) / NK) * gb::round_up(nk, NK), 8);
}

template <int NK, bool PACK>
__device__ __forceinline__ void fill_slot(const Args &A, int64_t slot, int lane) {
  constexpr int G = PACK ? 16 : 64;
  const int lg = lane & (G - 1), gbase = lane & ~(G - 1);
  const DItem I = A.items[PACK ? slot * 4 + (lane >> 4) : slot];
  const int nk = I.seq_len - kK + 1, n = I.n_rows;  // a filler has neither k-mers nor rows
  const int stride = I.rc ? -1 : 1;
  const char *seq = A.seqs + I.seq_off;
  const float *evs = A.events + I.ev_first;
  Trans T = A.T;
  T.mm_self = I.lp_mm_self, T.mm_next = I.lp_mm_next;

  // this lane's k-mers; anything finite for a k-mer past the item's (nothing reads what such a cell holds)
  Kmer km[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int ki = lg * NK + j;
    km[j] = Kmer{0.f, 1.f, 0.f};
    if (ki < nk) km[j] = make_kmer(A.model[kmer_rank4(kmer_at(seq, I.seq_len, I.rc, ki))], I.scale, I.shift, I.var, I.log_var);
  }
  const int llast = nk > 0 ? (nk - 1) / NK : 0;
  int steps = nk > 0 ? n + llast : 0;  // lane llast computes row n at step n + llast
  if (PACK)
    steps = max(max(__builtin_amdgcn_readlane(steps, 0), __builtin_amdgcn_readlane(steps, 16)),
                max(__builtin_amdgcn_readlane(steps, 32), __builtin_amdgcn_readlane(steps, 48)));
  else
    steps = __builtin_amdgcn_readfirstlane(steps);
  const int W = (nk + NK - 1) & ~(NK - 1);
  const bool mine = lg * NK < nk;  // lg <= llast then, so row <= n means step <= n + llast: inside the item's codes
  uint16_t *out = A.codes + I.ws_off + lg * NK;

  // rows tb + 1 .. tb + G, one event per lane of the group; a row past n gets 0, and its cells are not stored
  auto load_win = [&](int tb) {
    const int t = tb + lg + 1;
    return t <= n ? evs[(int64_t)(t - 1) * stride] : 0.f;
  };

  State S[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) S[j] = State{kNegInf, kNegInf, kNegInf};
  State nprev{kNegInf, kNegInf, kNegInf};  // lane l-1's last k-mer, one row above this step's
  float ev = 0.f;
  float w = load_win(0), wn = load_win(G);
  for (int t = 1; t <= steps; ++t) {
    const int jw = (t - 1) & (G - 1);
    if (jw == 0 && t > 1) {
      w = wn;
      wn = load_win(t - 1 + G);
    }
    ev = shr1<PACK>(ev, pick<PACK>(w, jw, gbase));  // lane l now holds row t - l's event
    // lane l-1 computed row t - l in the step before this one
    State ncur;
    ncur.m = shr1<PACK>(S[NK - 1].m, kNegInf);
    ncur.b = shr1<PACK>(S[NK - 1].b, kNegInf);
    ncur.k = shr1<PACK>(S[NK - 1].k, kNegInf);
    State lu = nprev, lc = ncur;
    unsigned code[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const State up = S[j];
      const float soft = j == 0 && lg == 0 && t == 1 ? A.soft0 : kNegInf;  // the start state enters at row 1 only
      State s;
      code[j] = cell_mb(T, up, lu, soft, emission(ev, km[j]), &s.m, &s.b);
      code[j] |= cell_k(T, lc, &s.k);
      S[j] = s, lu = up, lc = s;
    }
    const int row = t - lg;
    if (mine && row >= 1 && row <= n) {
      uint16_t *o = out + (int64_t)(t - 1) * W;
      if (NK == 1)
        *o = (uint16_t)code[0];
      else if (NK == 2)
        *reinterpret_cast<uint32_t *>(o) = code[0] | code[1] << 16;
      else
        *reinterpret_cast<uint2 *>(o) = make_uint2(code[0] | code[1] << 16, code[NK > 2 ? 2 : 0] | code[NK > 2 ? 3 : 0] << 16);
    }
    nprev = ncur;
  }
}

template <int NK, bool PACK>
__global__ __launch_bounds__(64 * kWaves) void abea_viterbi_fill_kernel(Args A) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    unsigned int p = 0;
    if (lane == 0) p = atomicAdd(A.next, 1u);
    p = __builtin_amdgcn_readfirstlane(p);
    if ((int64_t)p >= A.n_slots) break;
    fill_slot<NK, PACK>(A, (int64_t)p, lane);
    // the whole wave meets here before any lane fetches the next slot (see bsw_global.hip)
    __builtin_amdgcn_wave_barrier();
  }
}

// one lane per item of the chunk, in the fill's order (like rows and k-mers side by side)
__global__ __launch_bounds__(64) void abea_viterbi_walk_kernel(Args A) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n_slots) return;
  const DItem I = A.items[i];
  if (I.out < 0) return;
  const int nk = I.seq_len - kK + 1;
  const int sh = lanes_shift(class_nk(size_class(nk)));
  WalkIn w;
  w.codes = A.codes + I.ws_off, w.model = A.model, w.seq = A.seqs + I.seq_off, w.evs = A.events + I.ev_first;
  w.W = (nk + (1 << sh) - 1) & ~((1 << sh) - 1), w.sh = sh, w.seq_len = I.seq_len, w.rc = I.rc, w.e_start = I.e_start;
  w.stride = I.rc ? -1 : 1, w.n = I.n_rows, w.nk = nk;
  w.scale = I.scale, w.shift = I.shift, w.var = I.var, w.log_var = I.log_var, w.soft0 = A.soft0, w.T = A.T;
  w.T.mm_self = I.lp_mm_self, w.T.mm_next = I.lp_mm_next;
  A.lens[I.out] = walk_item(w, A.path + I.path_end, I.bound);
}

// a wave per item: the item's records, walked to the end of its part of `path`, go to packed[offs ..]
__global__ __launch_bounds__(256) void abea_viterbi_pack_kernel(Args A) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_slots; i += (int64_t)gridDim.x * 4) {
    const DItem I = A.items[i];
    if (I.out < 0) continue;
    const int len = A.lens[I.out];
    const gb_abea_path_rec *src = A.path + I.path_end - len;
    gb_abea_path_rec *dst = A.packed + A.offs[I.out];
    for (int j = lane; j < len; j += 64) dst[j] = src[j];
  }
}

static_assert(sizeof(Model) == 12, "gb_abea_model is three floats");
static_assert(sizeof(DItem) == 80, "DItem is packed");
static_assert(sizeof(gb_abea_path_rec) == 16, "the header's record");

struct Ws : gb::WsBase<5> {  // the calling thread's, through gb::get_ws
  gb::DevBuf<Model> d_model;
  gb::DevBuf<char> d_seqs;
  gb::DevBuf<float> d_events;
  gb::DevBuf<DItem> d_items;
  gb::DevBuf<uint16_t> d_codes;
  gb::DevBuf<gb_abea_path_rec> d_path, d_packed;
  gb::DevBuf<int32_t> d_lens;
  gb::DevBuf<int64_t> d_offs;
  gb::PinnedBuf<int64_t> h_offs;
  gb::DevBuf<unsigned int> d_ctl;
  gb::PinnedBuf<DItem> h_items;
  gb::PinnedBuf<gb_abea_path_rec> h_path;
  gb::PinnedBuf<int32_t> h_lens;
  float fill_ms = 0.f, walk_ms = 0.f;
  int64_t cells = 0, calls = 0, chunks = 0, ws_bytes = 0;
};

struct Need {
  int64_t codes, records;
  int64_t bytes() const {  // the codes, and the records walked and packed
    return codes * (int64_t)sizeof(uint16_t) + 2 * records * (int64_t)sizeof(gb_abea_path_rec);
  }
  void operator+=(const Need &o) { codes += o.codes, records += o.records; }
  void max_with(const Need &o) { codes = std::max(codes, o.codes), records = std::max(records, o.records); }
};
using Chunk = gb::Chunk<Need>;  // of the call's items

static inline Need item_need(const gb_abea_hmm_item &it) {
  const int nk = it.seq_len - kK + 1;
  return Need{item_codes(size_class(nk), nk, item_rows(it)), item_bound(it)};
}

// The chunks of a call: items in order, as many as fit GB_ABEA_VITERBI_WS or the default. Refuses the item that
// alone does not.
static int make_chunks(const char *who, const gb_abea_hmm_item *items, int64_t n_items, std::vector<Chunk> *chunks) {
  int64_t budget = 0;
  if (const int st = gb::env_number(who, "GB_ABEA_VITERBI_WS", 1, INT64_MAX, kDefaultBudget, &budget)) return st;
  const int64_t i = gb::cut_chunks(n_items, budget, [&](int64_t k) { return item_need(items[k]); }, chunks);
  GB_ARG(i < 0, "%s: item %lld needs %lld bytes of workspace, more than the budget of %lld (GB_ABEA_VITERBI_WS)", who,
         (long long)i, (long long)item_need(items[i]).bytes(), (long long)budget);
  return GB_OK;
}

// dst[0 .. bytes) = src on up to nth threads, in slices
static int copy_out(const char *who, int nth, void *dst, const void *src, size_t bytes) {
  constexpr size_t kSlice = size_t(4) << 20;
  const size_t slices = (bytes + kSlice - 1) / kSlice;
  if (slices <= 1 || nth <= 1) {
    std::memcpy(dst, src, bytes);
    return GB_OK;
  }
  std::atomic<size_t> next{0};
  return gb::parallel(who, (int)std::min<size_t>((size_t)nth, slices), [&](int) {
    for (size_t k; (k = next.fetch_add(1)) < slices;)
      std::memcpy(static_cast<char *>(dst) + k * kSlice, static_cast<const char *>(src) + k * kSlice,
                  std::min(kSlice, bytes - k * kSlice));
  });
}

// One chunk: fill, walk, pack, copy back; the chunk's records go to path[*used ..] in item order.
static int run_chunk(Ws *W, int nth, const Chunk &ch, const gb_abea_hmm_read *reads, const gb_abea_hmm_item *items,
                     const std::vector<Trans> &trans, gb_abea_path_rec *path, int64_t *path_off, int64_t *used) {
  // The items by size class, each class with the most rows first, so that the items of a packed slot are of
  // like length and the long ones do not start last. A packed class is filled up to a multiple of four.
  const int64_t n = ch.last - ch.first;
  std::vector<int32_t> order((size_t)n);
  std::vector<int64_t> pend((size_t)n);  // one past each item's records, in item order
  int64_t count[kClasses] = {0, 0, 0, 0}, first[kClasses], slots[kClasses], acc = 0;
  for (int64_t i = 0; i < n; ++i) {
    const gb_abea_hmm_item &it = items[ch.first + i];
    order[(size_t)i] = (int32_t)i;
    count[size_class(it.seq_len - kK + 1)] += 1;
    pend[(size_t)i] = (acc += item_bound(it));
  }
  auto key = [&](int32_t i) {
    const gb_abea_hmm_item &it = items[ch.first + i];
    return ((int64_t)size_class(it.seq_len - kK + 1) << 32) | (int64_t)(kMaxRows - item_rows(it));
  };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
  const int64_t fill0 = gb::round_up(count[0], 4) - count[0], total = n + fill0;
  DItem *hi = W->h_items;
  int64_t pos = 0, k = 0, ws_off = 0;
  for (int c = 0; c < kClasses; ++c) {
    first[c] = pos;
    for (int64_t j = 0; j < count[c]; ++j, ++k) {
      const int32_t i = order[(size_t)k];
      const gb_abea_hmm_item &it = items[ch.first + i];
      const gb_abea_hmm_read &rd = reads[it.read];
      const Trans &T = trans[(size_t)it.read];
      hi[pos++] = DItem{it.seq_off, rd.event_off + it.event_start, ws_off, pend[(size_t)i], it.seq_len, item_rows(it), i,
                        it.rc, it.event_start, item_bound(it), rd.scale, rd.shift, rd.var, rd.log_var, T.mm_self, T.mm_next};
      ws_off += item_codes(c, it.seq_len - kK + 1, item_rows(it));
      W->cells += (int64_t)item_rows(it) * (it.seq_len - kK + 1);
    }
    if (c == 0)
      for (int64_t j = 0; j < fill0; ++j) hi[pos++] = DItem{0, 0, 0, 0, kK - 1, 0, -1, 0, 0, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    slots[c] = c == 0 ? (count[0] + fill0) / 4 : count[c];
  }
  GB_HIP(hipMemcpyAsync(W->d_items, hi, (size_t)total * sizeof(DItem), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemsetAsync(W->d_ctl, 0, kClasses * sizeof(unsigned int), W->stream));
  Args A;
  A.model = W->d_model, A.seqs = W->d_seqs, A.events = W->d_events, A.codes = W->d_codes, A.path = W->d_path;
  A.lens = W->d_lens, A.packed = W->d_packed, A.offs = W->d_offs, A.soft0 = soft0();
  float p_next;
  make_trans(2.0, &A.T, &p_next);  // the eight transitions that do not depend on the read
  GB_HIP(hipEventRecord(W->ev[0], W->stream));
  for (int c = 0; c < kClasses; ++c) {
    if (!slots[c]) continue;
    A.items = W->d_items.get() + first[c], A.n_slots = slots[c], A.next = W->d_ctl.get() + c;
    const int64_t want = (slots[c] + kWaves - 1) / kWaves;
    const dim3 grid((unsigned)std::min<int64_t>(want, (int64_t)W->num_cus * kBlocksPerCU)), block(64 * kWaves);
    if (c == 0)
      hipLaunchKernelGGL((abea_viterbi_fill_kernel<1, true>), grid, block, 0, W->stream, A);
    else if (c == 1)
      hipLaunchKernelGGL((abea_viterbi_fill_kernel<1, false>), grid, block, 0, W->stream, A);
    else if (c == 2)
      hipLaunchKernelGGL((abea_viterbi_fill_kernel<2, false>), grid, block, 0, W->stream, A);
    else
      hipLaunchKernelGGL((abea_viterbi_fill_kernel<4, false>), grid, block, 0, W->stream, A);
    GB_HIP(hipGetLastError());
  }
  GB_HIP(hipEventRecord(W->ev[1], W->stream));
  A.items = W->d_items, A.n_slots = total, A.next = nullptr;
  hipLaunchKernelGGL(abea_viterbi_walk_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[2], W->stream));
  GB_HIP(hipMemcpyAsync(W->h_lens, W->d_lens, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  int64_t got = 0;  // the chunk's records; the exclusive scan of the lengths is where each item's go
  for (int64_t i = 0; i < n; ++i) {
    W->h_offs[i] = got;
    path_off[ch.first + i] = *used + got;
    got += W->h_lens[i];
  }
  GB_HIP(hipMemcpyAsync(W->d_offs, W->h_offs, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipEventRecord(W->ev[3], W->stream));
  const int64_t pack_blocks = std::min<int64_t>((total + 3) / 4, (int64_t)W->num_cus * 8);
  hipLaunchKernelGGL(abea_viterbi_pack_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[4], W->stream));
  GB_HIP(hipMemcpyAsync(W->h_path, W->d_packed, (size_t)got * sizeof(gb_abea_path_rec), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  float fill_ms = 0.f, walk_ms = 0.f, pack_ms = 0.f;
  GB_HIP(hipEventElapsedTime(&fill_ms, W->ev[0], W->ev[1]));
  GB_HIP(hipEventElapsedTime(&walk_ms, W->ev[1], W->ev[2]));
  GB_HIP(hipEventElapsedTime(&pack_ms, W->ev[3], W->ev[4]));
  W->fill_ms += fill_ms, W->walk_ms += walk_ms + pack_ms;
  if (const int st = copy_out("gb_abea_hmm_align", nth, path + *used, W->h_path.get(), (size_t)got * sizeof(gb_abea_path_rec)))
    return st;
  *used += got;
  return GB_OK;
}

}  // namespace gbvit

extern "C" {

int gb_abea_hmm_align_timing(float *fill_ms, float *walk_ms, int64_t *cells) {
  GB_ARG(fill_ms && walk_ms && cells, "gb_abea_hmm_align_timing: null argument");
  const gbvit::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_abea_hmm_align_timing", "gb_abea_hmm_align", &W, &gbvit::Ws::calls)) return st;
  *fill_ms = W->fill_ms, *walk_ms = W->walk_ms, *cells = W->cells;
  return GB_OK;
}

int gb_abea_hmm_align_plan(int64_t *chunks, int64_t *workspace_bytes) {
  GB_ARG(chunks && workspace_bytes, "gb_abea_hmm_align_plan: null argument");
  const gbvit::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_abea_hmm_align_plan", "gb_abea_hmm_align", &W, &gbvit::Ws::calls)) return st;
  *chunks = W->chunks, *workspace_bytes = W->ws_bytes;
  return GB_OK;
}

int gb_abea_hmm_align(const gb_abea_model *model, const char *seqs, int64_t seq_bytes, const float *event_mean,
                      int64_t n_event_total, const gb_abea_hmm_read *reads, int64_t n_reads,
                      const gb_abea_hmm_item *items, int64_t n_items, gb_abea_path_rec *path, int64_t path_cap,
                      int64_t *path_off, int64_t *path_used) {
  using namespace gbvit;
  const char *who = "gb_abea_hmm_align";
  gb::Range range_("gb.abea.hmm_align");
  try {
    GB_ARG(path_off && path_used && path_cap >= 0 && (path_cap == 0 || path), "%s: bad path arguments", who);
    std::vector<Trans> trans;
    int st = validate(who, model, GB_ABEA_VITERBI_MODEL_SIZE, 2, 0, seqs, seq_bytes, event_mean, n_event_total, reads,
                      n_reads, items, n_items, path_off, &trans);
    if (st) return st;
    if (n_items == 0) {
      path_off[0] = 0, *path_used = 0;
      return GB_OK;
    }
    int64_t need = 0;
    for (int64_t i = 0; i < n_items; ++i) {
      const gb_abea_hmm_item &it = items[i];
      GB_ARG(!(it.seq_len == kK && item_rows(it) == 2 && trans[(size_t)it.read].mm_self == kNegInf),
             "%s: item %lld has one k-mer and two rows in a read with events_per_base 1 (no path reaches its last cell)",
             who, (long long)i);
      need += item_bound(it);
    }
    const bool host = gb::env_flag("GB_ABEA_HOST");
    std::vector<Chunk> chunks;
    if (!host && (st = make_chunks(who, items, n_items, &chunks))) return st;
    if (path_cap < need) {
      *path_used = need;
      gb::set_error("%s: path_cap is %lld, the items need %lld (rows + k-mers - 1 each)", who, (long long)path_cap,
                    (long long)need);
      return GB_ERR_ARG;
    }
    if (host) {
      int nth = 1;
      if ((st = gb::thread_count(who, "GB_ABEA_THREADS", &nth))) return st;
      std::vector<gb_abea_path_rec> recs((size_t)need);
      std::vector<int64_t> pend((size_t)n_items);
      std::vector<int32_t> lens((size_t)n_items);
      int64_t acc = 0;
      for (int64_t i = 0; i < n_items; ++i) pend[(size_t)i] = (acc += item_bound(items[i]));
      std::atomic<int64_t> next{0};
      if ((st = gb::parallel(who, (int)std::min<int64_t>(nth, n_items), [&](int) {
             HostScratch hs;
             for (int64_t i; (i = next.fetch_add(1)) < n_items;) {
               const gb_abea_hmm_item &it = items[i];
               const gb_abea_hmm_read &rd = reads[it.read];
               lens[(size_t)i] = host_align(model, seqs + it.seq_off, it, event_mean + rd.event_off, rd,
                                            trans[(size_t)it.read], &hs, recs.data() + pend[(size_t)i]);
             }
           })))
        return st;
      int64_t used = 0;
      for (int64_t i = 0; i < n_items; ++i) {
        path_off[i] = used;
        std::memcpy(path + used, recs.data() + pend[(size_t)i] - lens[(size_t)i],
                    (size_t)lens[(size_t)i] * sizeof(gb_abea_path_rec));
        used += lens[(size_t)i];
      }
      path_off[n_items] = *path_used = used;
      return GB_OK;
    }
    int dev = 0, nth = 1;
    if ((st = gb::thread_count(who, "GB_ABEA_THREADS", &nth))) return st;  // for the copy into path
    GB_HIP(hipGetDevice(&dev));
    Ws *W = nullptr;
    if ((st = gb::get_ws(who, dev, &W, [](Ws *W) { return W->d_ctl.reserve(kClasses); }))) return st;
    W->calls = 0, W->cells = 0, W->fill_ms = W->walk_ms = 0.f;
    const auto big = gb::largest(chunks);  // every buffer at the largest any chunk asks of it
    const int64_t big_n = big.count;
    if ((st = W->d_model.reserve(GB_ABEA_VITERBI_MODEL_SIZE)) || (st = W->d_seqs.reserve((size_t)seq_bytes)) ||
        (st = W->d_events.reserve((size_t)n_event_total)) || (st = W->h_items.reserve((size_t)big_n + 3)) ||
        (st = W->d_items.reserve((size_t)big_n + 3)) || (st = W->d_codes.reserve((size_t)big.need.codes)) ||
        (st = W->d_path.reserve((size_t)big.need.records)) || (st = W->d_packed.reserve((size_t)big.need.records)) ||
        (st = W->h_path.reserve((size_t)big.need.records)) || (st = W->d_lens.reserve((size_t)big_n)) ||
        (st = W->h_lens.reserve((size_t)big_n)) || (st = W->d_offs.reserve((size_t)big_n)) ||
        (st = W->h_offs.reserve((size_t)big_n)))
      return st;
    GB_HIP(hipMemcpyAsync(W->d_model, model, GB_ABEA_VITERBI_MODEL_SIZE * sizeof(Model), hipMemcpyHostToDevice, W->stream));
    GB_HIP(hipMemcpyAsync(W->d_seqs, seqs, (size_t)seq_bytes, hipMemcpyHostToDevice, W->stream));
    GB_HIP(hipMemcpyAsync(W->d_events, event_mean, (size_t)n_event_total * sizeof(float), hipMemcpyHostToDevice,
                          W->stream));
    int64_t used = 0;
    for (const Chunk &c : chunks)
      if ((st = run_chunk(W, nth, c, reads, items, trans, path, path_off, &used))) return st;
    path_off[n_items] = *path_used = used;
    W->chunks = (int64_t)chunks.size(), W->ws_bytes = big.bytes;
    W->calls = 1;
    return GB_OK;
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
}

}  // extern "C"
