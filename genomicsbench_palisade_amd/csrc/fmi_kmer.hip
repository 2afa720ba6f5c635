// fmi_kmer.hip -- k-mer counting and the solid k-mer index (include/gb_fmi_kmer.h; Flye's KmerCounter::count and
// VertexIndex::buildIndexUnevenCoverage). DESIGN.md, "kmer", has the contract and the reasoning.
//
// Count: pack the reads 2 bits a base, write one canonical code per k-mer position, sort the codes with a stable
// LSD radix sort (8 bits a pass, ceil(2k / 8) passes) and reduce the runs to distinct codes and counts. No table
// has 4^k entries and no global atomic is issued anywhere. A sort pass is a per-tile digit histogram in LDS, an
// exclusive scan of the digit-major tiles x 256 table, and a scatter that ranks inside the wave by ballot matching
// and across the tile's waves through LDS. The scan is three launches (tile sums, one workgroup over the sums,
// apply), so no kernel waits for another workgroup.
//
// Index: every occurrence finds its code's rank among the distinct codes by binary search; one workgroup per read
// selects the maxKmers-th largest frequency by radix select over an LDS histogram; within-read multiplicities are
// taken only of codes whose global count exceeds tandem_freq (sort of (rank, occurrence), then a bounded walk over a
// candidate's neighbours); the kept positions are flagged in a table of two slots per occurrence laid out in global-position
// order, compacted in that order and sorted stably by rank, which leaves every list ascending. Runs, capacities and
// the filter scalars are then a host pass over the runs.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/gb_fmi_kmer.h"
#include "fmi_kmer_internal.h"
#include "gb_common.h"
#include "gb_common_wave.h"

namespace {

using gb::kmer::canonical;
using gb::kmer::find_code;
using gb::kmer::owner;
using gb::kmer::window;

constexpr int kThreads = 256, kItems = 16, kTile = kThreads * kItems;
static_assert(kTile == GB_KMER_TILE, "header and kernels disagree on the tile");
constexpr int64_t kDefaultBudget = int64_t(32) << 30;
constexpr uint32_t kStrand = 0x80000000u, kRank = 0x7FFFFFFFu;

// ---------------------------------------------------------------------------------------------- device: scans

template <typename T>
__global__ __launch_bounds__(kThreads) void k_scan_sums(const T *in, int64_t n, uint32_t *sums) {
  __shared__ int lds[4];
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  int s = 0;
  for (int j = 0; j < kItems; ++j)
    if (base + j < n) s += (int)in[base + j];
  int total;
  gb::block_scan_excl<kThreads>(s, &total, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = (uint32_t)total;
}

// one workgroup: sums[0 .. nb) to its exclusive scan in place, sums[nb] the total
__global__ __launch_bounds__(kThreads) void k_scan_top(uint32_t *sums, int64_t nb) {
  __shared__ int lds[4];
  int carry = 0;
  for (int64_t c = 0; c < nb; c += kThreads) {
    const int64_t i = c + threadIdx.x;
    const int v = i < nb ? (int)sums[i] : 0;
    int total;
    const int ex = gb::block_scan_excl<kThreads>(v, &total, lds);
    if (i < nb) sums[i] = (uint32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = (uint32_t)carry;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_scan_apply(const T *in, int64_t n, const uint32_t *sums,
                                                         uint32_t *out) {
  __shared__ int lds[4];
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  int v[kItems], s = 0;
  for (int j = 0; j < kItems; ++j) {
    v[j] = base + j < n ? (int)in[base + j] : 0;
    s += v[j];
  }
  int total;
  int ex = gb::block_scan_excl<kThreads>(s, &total, lds) + (int)sums[blockIdx.x];
  for (int j = 0; j < kItems; ++j) {
    if (base + j < n) out[base + j] = (uint32_t)ex;
    ex += v[j];
  }
}

// ----------------------------------------------------------------------------------------- device: radix sort

__global__ __launch_bounds__(kThreads) void k_radix_hist(const uint64_t *keys, int64_t n, int shift, int64_t tiles,
                                                         uint32_t *table) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x;
  for (int j = 0; j < kItems; ++j) {
    const int64_t i = base + (int64_t)j * kThreads;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1u);  // LDS
  }
  __syncthreads();
  table[(int64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// table holds the exclusive scan of the digit-major histogram: table[d * tiles + t] is where tile t's first key
// of digit d goes. Wave w owns keys [w * 1024, (w + 1) * 1024) of the tile, 64 consecutive keys a round, so
// (wave, round, lane) order is key order and the ranks below keep the sort stable.
template <bool kVals>
__global__ __launch_bounds__(kThreads) void k_radix_scatter(const uint64_t *keys, const uint64_t *vals,
                                                            uint64_t *keys_out, uint64_t *vals_out, int64_t n,
                                                            int shift, int64_t tiles, const uint32_t *table) {
  __shared__ uint32_t cnt[kThreads / 64][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = 0; i < kThreads / 64; ++i) cnt[i][threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)w * (64 * kItems) + lane;
  const uint64_t lt = (uint64_t(1) << lane) - 1;
  uint64_t key[kItems];
  uint32_t off[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + (int64_t)r * 64;
    const bool valid = i < n;
    key[r] = valid ? keys[i] : 0;
    const uint32_t d = (uint32_t)(key[r] >> shift) & 255;
    uint64_t mask = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t m = __builtin_amdgcn_ballot_w64((d >> b) & 1);
      mask &= ((d >> b) & 1) ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(mask & lt);
    off[r] = valid ? cnt[w][d] + rank : 0;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) cnt[w][d] += (uint32_t)__popcll(mask);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    uint32_t b = table[(int64_t)threadIdx.x * tiles + blockIdx.x];
    for (int i = 0; i < kThreads / 64; ++i) {
      const uint32_t c = cnt[i][threadIdx.x];
      cnt[i][threadIdx.x] = b;
      b += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + (int64_t)r * 64;
    if (i < n) {
      const uint32_t d = (uint32_t)(key[r] >> shift) & 255;
      const uint32_t o = cnt[w][d] + off[r];
      keys_out[o] = key[r];
      if (kVals) vals_out[o] = vals[i];
    }
  }
}

// ----------------------------------------------------------------------------------------------- device: count

__global__ __launch_bounds__(kThreads) void k_pack(const uint8_t *bytes, const int64_t *base_off,
                                                   const int64_t *word_off, int64_t n_seqs, int64_t n_words,
                                                   uint64_t *words) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= n_words) return;
  const int64_t r = owner(word_off, n_seqs, g);
  const int64_t j0 = (g - word_off[r]) * 32, len = base_off[r + 1] - base_off[r];
  const uint8_t *b = bytes + base_off[r] + j0;
  const int m = (int)(len - j0 < 32 ? len - j0 : 32);
  uint64_t x = 0;
  for (int j = 0; j < m; ++j) {
    const uint32_t c = (b[j] >> 1) & 3;  // A 0, C 1, T 2, G 3
    x |= (uint64_t)(c ^ (c >> 1)) << (62 - 2 * j);
  }
  words[g] = x;
}

__global__ __launch_bounds__(kThreads) void k_extract(const uint64_t *words, const int64_t *word_off,
                                                      const int64_t *kmer_off, int64_t n_seqs, int64_t n_occ, int k,
                                                      uint64_t *keys) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= n_occ) return;
  const int64_t r = owner(kmer_off, n_seqs, o);
  bool rev;
  keys[o] = canonical(window(words + word_off[r], o - kmer_off[r], k), k, &rev);
}

__global__ __launch_bounds__(kThreads) void k_heads(const uint64_t *keys, int64_t n, uint8_t *heads) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) heads[i] = i == 0 || keys[i] != keys[i - 1];
}

__global__ __launch_bounds__(kThreads) void k_runs(const uint64_t *keys, const uint8_t *heads, const uint32_t *pos,
                                                   int64_t n, uint64_t *run_key, uint32_t *run_start) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n && heads[i]) run_key[pos[i]] = keys[i], run_start[pos[i]] = (uint32_t)i;
}

// starts[nd] is n
__global__ __launch_bounds__(kThreads) void k_counts(const uint32_t *starts, int64_t nd, uint32_t *counts) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nd) counts[i] = starts[i + 1] - starts[i];
}

// per workgroup: the largest count and the number of counts >= 16 (counts stay below 2^31)
__global__ __launch_bounds__(kThreads) void k_stats(const uint32_t *counts, int64_t nd, uint32_t *part_max,
                                                    uint32_t *part_over) {
  __shared__ int lds[4];
  int mx = 0, over = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nd; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)counts[i];
    mx = max(mx, c), over += c >= 16;
  }
  int total;
  gb::block_scan_excl<kThreads>(over, &total, lds);
  mx = gb::wave_max<0>(mx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    part_max[blockIdx.x] = (uint32_t)max(max(lds[0], lds[1]), max(lds[2], lds[3]));
    part_over[blockIdx.x] = (uint32_t)total;
  }
}

// ----------------------------------------------------------------------------------------------- device: index

struct Reads {  // the resident read set
  const uint64_t *words;
  const int64_t *word_off, *kmer_off, *base_off;
  int64_t n_seqs, n_occ;
  int k;
};

// each occurrence: the rank of its canonical code among the distinct codes, and the strand bit
__global__ __launch_bounds__(kThreads) void k_lookup(Reads R, const uint64_t *codes, int64_t nd, uint32_t *rank) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= R.n_occ) return;
  const int64_t r = owner(R.kmer_off, R.n_seqs, o);
  bool rev;
  const uint64_t c = canonical(window(R.words + R.word_off[r], o - R.kmer_off[r], R.k), R.k, &rev);
  rank[o] = (uint32_t)find_code(codes, nd, c) | (rev ? kStrand : 0u);
}

// one workgroup per read: the maxk[r]-th largest (0-based) frequency of its positions, by radix select from the
// top byte down over a 256-bin LDS histogram
__global__ __launch_bounds__(kThreads) void k_select(const int64_t *kmer_off, const uint32_t *rank,
                                                     const uint32_t *counts, const int64_t *maxk,
                                                     uint32_t *min_freq) {
  __shared__ uint32_t h[256];
  __shared__ uint32_t s_prefix;
  __shared__ int64_t s_want;
  const int64_t r = blockIdx.x, o0 = kmer_off[r], n = kmer_off[r + 1] - o0;
  if (n <= 0) return;  // the whole workgroup
  if (threadIdx.x == 0) s_prefix = 0, s_want = maxk[r];
  for (int byte = 3; byte >= 0; --byte) {
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    const uint32_t high = byte == 3 ? 0u : 0xFFFFFFFFu << (8 * (byte + 1));
    for (int64_t p = threadIdx.x; p < n; p += kThreads) {
      const uint32_t f = counts[rank[o0 + p] & kRank];
      if ((f & high) == prefix) atomicAdd(&h[(f >> (8 * byte)) & 255], 1u);  // LDS
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t want = s_want;
      int d = 255;
      for (; d > 0 && want >= (int64_t)h[d]; --d) want -= h[d];
      s_want = want, s_prefix = prefix | ((uint32_t)d << (8 * byte));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) min_freq[r] = s_prefix;
}

// kept: frequency at or above the read's threshold; cand: kept and a tandem candidate
__global__ __launch_bounds__(kThreads) void k_keep(Reads R, const uint32_t *rank, const uint32_t *counts,
                                                   const uint32_t *min_freq, int32_t tandem, uint8_t *kept,
                                                   uint8_t *cand) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= R.n_occ) return;
  const uint32_t f = counts[rank[o] & kRank];
  const bool kp = f >= min_freq[owner(R.kmer_off, R.n_seqs, o)];
  kept[o] = kp;
  cand[o] = kp && tandem > 0 && f > (uint32_t)tandem;
}

__global__ __launch_bounds__(kThreads) void k_cand_compact(const uint8_t *cand, const uint32_t *pos,
                                                           const uint32_t *rank, int64_t n, uint64_t *keys,
                                                           uint64_t *vals) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o < n && cand[o]) keys[pos[o]] = rank[o] & kRank, vals[pos[o]] = (uint64_t)o;
}

// candidates sorted by (rank, occurrence): the pairs of a candidate's rank whose occurrence lies in its read are
// its neighbours, so its multiplicity in the read passes tandem exactly when more than tandem pairs around it
// match. Each side is walked for at most tandem steps.
__global__ __launch_bounds__(kThreads) void k_tandem(Reads R, const uint64_t *keys, const uint64_t *vals, int64_t n,
                                                     int32_t tandem, uint8_t *kept) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const int64_t o = (int64_t)vals[i], r = owner(R.kmer_off, R.n_seqs, o);
  const uint64_t lo = (uint64_t)R.kmer_off[r], hi = (uint64_t)R.kmer_off[r + 1];
  int32_t same = 1;
  for (int64_t j = i - 1; j >= 0 && same <= tandem && keys[j] == key && vals[j] >= lo; --j) ++same;
  for (int64_t j = i + 1; j < n && same <= tandem && keys[j] == key && vals[j] < hi; ++j) ++same;
  if (same > tandem) kept[o] = 0;
}

// Slots: read r owns slots [2 kmer_off[r], 2 kmer_off[r + 1]), its forward offsets first and then the offsets of
// its reverse complement, so slot order is global-position order. An occurrence takes the forward slot of its
// offset, or the reverse slot of L - p - k when its reverse complement was the smaller code. The reference's walk
// ends one k-mer before the read does (n = L - k), so the reverse offsets are 1 .. n.
__device__ __forceinline__ bool slot_of(const Reads &R, const uint32_t *rank, const uint32_t *counts,
                                        const uint8_t *kept, int32_t min_freq, int64_t o, int64_t *slot,
                                        int64_t *gpos) {
  if (!kept[o] || counts[rank[o] & kRank] < (uint32_t)min_freq) return false;
  const int64_t r = owner(R.kmer_off, R.n_seqs, o);
  const int64_t p = o - R.kmer_off[r], n = R.kmer_off[r + 1] - R.kmer_off[r];
  const int64_t len = R.base_off[r + 1] - R.base_off[r];
  const bool rev = rank[o] & kStrand;
  const int64_t q = rev ? len - p - R.k : p;
  *slot = 2 * R.kmer_off[r] + (rev ? n - 1 : 0) + q;
  *gpos = 2 * R.base_off[r] + (rev ? len : 0) + q;
  return true;
}

__global__ __launch_bounds__(kThreads) void k_slot_flag(Reads R, const uint32_t *rank, const uint32_t *counts,
                                                        const uint8_t *kept, int32_t min_freq, uint8_t *flags) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t slot, gpos;
  if (o < R.n_occ && slot_of(R, rank, counts, kept, min_freq, o, &slot, &gpos)) flags[slot] = 1;
}

__global__ __launch_bounds__(kThreads) void k_slot_compact(Reads R, const uint32_t *rank, const uint32_t *counts,
                                                           const uint8_t *kept, int32_t min_freq,
                                                           const uint32_t *pos, uint64_t *keys, uint64_t *vals) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t slot, gpos;
  if (o < R.n_occ && slot_of(R, rank, counts, kept, min_freq, o, &slot, &gpos))
    keys[pos[slot]] = rank[o] & kRank, vals[pos[slot]] = (uint64_t)gpos;
}

// ------------------------------------------------------------------------------------------------- host side

struct Stats {  // of the calling thread's last calls; plain data, so thread storage is fine
  float pack_ms, extract_ms, sort_ms, reduce_ms, lookup_ms, select_ms, fill_ms;
  int64_t occ, passes, ws_bytes, calls;
};
Stats &stats() {
  thread_local Stats s{};
  return s;
}

struct Ws : gb::WsBase<5> {};  // the calling thread's, through gb::get_ws

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int blocks(int64_t n) { return (int)ceil_div(n, kThreads); }
inline int64_t tiles_of(int64_t n) { return ceil_div(n, kTile); }
inline int bits_of(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 1; }

// device workspace of a count of n occurrences over n_bytes bases in n_words words: the bytes, two key buffers,
// the run heads, their scan and the run starts, the digit table and the scan's sums
int64_t count_ws_bytes(int64_t n, int64_t n_bytes) {
  return n_bytes + 16 * n + n + 4 * n + 4 * (n + 1) + 4 * (256 * tiles_of(n) + 1) + 4 * (tiles_of(256 * tiles_of(n)) + 2);
}
// of an index over n occurrences: ranks, kept and candidate flags, two slots an occurrence with their scan, four
// pair buffers, the run arrays, the per-read arrays, the table and the sums
int64_t index_ws_bytes(int64_t n, int64_t n_seqs) {
  return 4 * n + n + n + 2 * n + 8 * n + 32 * n + 12 * n + 12 * n_seqs + 4 * (256 * tiles_of(n) + 1) +
         4 * (tiles_of(std::max(2 * n, 256 * tiles_of(n))) + 2);
}

// exclusive scan of in[0 .. n) into out; sums has tiles_of(n) + 1 entries and sums[tiles_of(n)] is the total
template <typename T>
void scan(hipStream_t s, const T *in, int64_t n, uint32_t *out, uint32_t *sums) {
  const int64_t nb = tiles_of(n);
  k_scan_sums<T><<<(int)nb, kThreads, 0, s>>>(in, n, sums);
  k_scan_top<<<1, kThreads, 0, s>>>(sums, nb);
  k_scan_apply<T><<<(int)nb, kThreads, 0, s>>>(in, n, sums, out);
}
int scan_total(hipStream_t s, const uint32_t *sums, int64_t n, int64_t *total) {
  uint32_t t = 0;
  GB_HIP(hipMemcpyAsync(&t, sums + tiles_of(n), 4, hipMemcpyDeviceToHost, s));
  GB_HIP(hipStreamSynchronize(s));
  *total = t;
  return GB_OK;
}

// stable sort of n keys (and their values, if va is not null) on their low `bits` bits; the result is in
// *ka / *va, the other pair is scratch. table has 256 tiles + 1 entries, sums what their scan needs.
void radix_sort(hipStream_t s, uint64_t **ka, uint64_t **kb, uint64_t **va, uint64_t **vb, int64_t n, int bits,
                uint32_t *table, uint32_t *sums) {
  const int64_t tiles = tiles_of(n);
  for (int shift = 0; shift < bits; shift += 8) {
    k_radix_hist<<<(int)tiles, kThreads, 0, s>>>(*ka, n, shift, tiles, table);
    scan<uint32_t>(s, table, 256 * tiles, table, sums);
    if (va) {
      k_radix_scatter<true><<<(int)tiles, kThreads, 0, s>>>(*ka, *va, *kb, *vb, n, shift, tiles, table);
      std::swap(*va, *vb);
    } else {
      k_radix_scatter<false><<<(int)tiles, kThreads, 0, s>>>(*ka, nullptr, *kb, nullptr, n, shift, tiles, table);
    }
    std::swap(*ka, *kb);
  }
}

// chunks sorted on the workers, then merged pairwise
template <typename T>
int par_sort(const char *who, int nth, std::vector<T> &v) {
  const size_t n = v.size();
  const int parts = (int)std::max<size_t>(1, std::min<size_t>((size_t)nth, n / 65536));
  std::vector<size_t> cut((size_t)parts + 1);
  for (int i = 0; i <= parts; ++i) cut[(size_t)i] = n * (size_t)i / (size_t)parts;
  if (const int st = gb::parallel(who, parts, [&](int t) {
        std::sort(v.begin() + (ptrdiff_t)cut[(size_t)t], v.begin() + (ptrdiff_t)cut[(size_t)t + 1]);
      }))
    return st;
  for (int step = 1; step < parts; step *= 2)
    for (int i = 0; i + step < parts; i += 2 * step)
      std::inplace_merge(v.begin() + (ptrdiff_t)cut[(size_t)i], v.begin() + (ptrdiff_t)cut[(size_t)(i + step)],
                         v.begin() + (ptrdiff_t)cut[(size_t)std::min(i + 2 * step, parts)]);
  return GB_OK;
}

}  // namespace

struct gb_kmer_counts {
  int k = 0, dev = -1;
  bool host = true;  // also the empty handle, which never touched a device
  int64_t n_seqs = 0, n_occ = 0, n_distinct = 0, n_over15 = 0, max_count = 0;
  std::vector<int64_t> base_off, word_off, kmer_off;  // n_seqs + 1 each
  std::vector<uint64_t> h_words, h_codes;             // h_words on the host path only
  std::vector<uint32_t> h_counts;
  bool mirrored = false;  // h_codes / h_counts hold the device's
  gb::DevBuf<uint64_t> d_words, d_codes;
  gb::DevBuf<uint32_t> d_counts;
  gb::DevBuf<int64_t> d_base_off, d_word_off, d_kmer_off;
};

struct gb_kmer_idx {
  std::vector<uint64_t> codes, rep_codes;
  std::vector<int64_t> off, pos;
  int64_t rep_freq = 0;
};

namespace {

int mirror(gb_kmer_counts *h) {
  if (h->host || h->mirrored) return GB_OK;
  try {
    h->h_codes.resize((size_t)h->n_distinct), h->h_counts.resize((size_t)h->n_distinct);
  } catch (...) {
    gb::set_error("gb_kmer: out of host memory for %lld codes", (long long)h->n_distinct);
    return GB_ERR_NOMEM;
  }
  GB_HIP(gb::memcpy_big(h->h_codes.data(), h->d_codes, 8 * (size_t)h->n_distinct, hipMemcpyDeviceToHost));
  GB_HIP(gb::memcpy_big(h->h_counts.data(), h->d_counts, 4 * (size_t)h->n_distinct, hipMemcpyDeviceToHost));
  h->mirrored = true;
  return GB_OK;
}

void host_stats(gb_kmer_counts *h) {
  h->n_over15 = h->max_count = 0;
  for (uint32_t c : h->h_counts) h->n_over15 += c >= 16, h->max_count = std::max<int64_t>(h->max_count, c);
}

int count_host(const char *who, gb_kmer_counts *h, const uint8_t *bytes) {
  int nth = 1, st;
  if ((st = gb::thread_count(who, "GB_KMER_THREADS", &nth))) return st;
  const int k = h->k;
  h->h_words.assign((size_t)h->word_off[(size_t)h->n_seqs], 0);
  std::vector<uint64_t> all((size_t)h->n_occ);
  std::atomic<int64_t> next{0};
  if ((st = gb::parallel(who, (int)std::max<int64_t>(1, std::min<int64_t>(nth, h->n_seqs)), [&](int) {
         for (int64_t r; (r = next.fetch_add(1)) < h->n_seqs;) {
           uint64_t *w = h->h_words.data() + h->word_off[(size_t)r];
           const uint8_t *b = bytes + h->base_off[(size_t)r];
           const int64_t len = h->base_off[(size_t)r + 1] - h->base_off[(size_t)r];
           for (int64_t j = 0; j < len; ++j) {
             const uint32_t c = (b[j] >> 1) & 3;
             w[j >> 5] |= (uint64_t)(c ^ (c >> 1)) << (62 - 2 * (j & 31));
           }
           uint64_t *o = all.data() + h->kmer_off[(size_t)r];
           bool rev;
           for (int64_t p = 0; p + k < len; ++p) o[p] = canonical(window(w, p, k), k, &rev);
         }
       })))
    return st;
  if ((st = par_sort(who, nth, all))) return st;
  for (size_t i = 0; i < all.size();) {
    size_t j = i;
    while (j < all.size() && all[j] == all[i]) ++j;
    h->h_codes.push_back(all[i]), h->h_counts.push_back((uint32_t)(j - i));
    i = j;
  }
  h->n_distinct = (int64_t)h->h_codes.size();
  host_stats(h);
  return GB_OK;
}

int count_device(const char *who, gb_kmer_counts *h, const uint8_t *bytes, int64_t n_bytes) {
  int st;
  GB_HIP(hipGetDevice(&h->dev));
  Ws *W = nullptr;
  if ((st = gb::get_ws("gb_kmer", h->dev, &W))) return st;
  hipStream_t s = W->stream;
  const int64_t n = h->n_occ, n_seqs = h->n_seqs, n_words = h->word_off[(size_t)n_seqs], tiles = tiles_of(n);
  Stats &S = stats();

  gb::DevBuf<uint8_t> d_bytes, d_heads;
  gb::DevBuf<uint64_t> d_ka, d_kb;
  gb::DevBuf<uint32_t> d_table, d_sums, d_pos, d_starts, d_part;
  const size_t off_bytes = 8 * (size_t)(n_seqs + 1);
  if ((st = d_bytes.reserve((size_t)n_bytes)) || (st = h->d_words.reserve((size_t)n_words)) ||
      (st = h->d_base_off.reserve((size_t)n_seqs + 1)) || (st = h->d_word_off.reserve((size_t)n_seqs + 1)) ||
      (st = h->d_kmer_off.reserve((size_t)n_seqs + 1)) || (st = d_ka.reserve((size_t)n)) ||
      (st = d_kb.reserve((size_t)n)) || (st = d_table.reserve((size_t)(256 * tiles + 1))) ||
      (st = d_sums.reserve((size_t)(tiles_of(std::max(n, 256 * tiles)) + 2))) || (st = d_heads.reserve((size_t)n)) ||
      (st = d_pos.reserve((size_t)n)) || (st = d_part.reserve(2048)))
    return st;
  GB_HIP(gb::memcpy_big(d_bytes, bytes, (size_t)n_bytes, hipMemcpyHostToDevice));
  GB_HIP(hipMemcpy(h->d_base_off, h->base_off.data(), off_bytes, hipMemcpyHostToDevice));
  GB_HIP(hipMemcpy(h->d_word_off, h->word_off.data(), off_bytes, hipMemcpyHostToDevice));
  GB_HIP(hipMemcpy(h->d_kmer_off, h->kmer_off.data(), off_bytes, hipMemcpyHostToDevice));

  GB_HIP(hipEventRecord(W->ev[0], s));
  k_pack<<<blocks(n_words), kThreads, 0, s>>>(d_bytes, h->d_base_off, h->d_word_off, n_seqs, n_words, h->d_words);
  GB_HIP(hipEventRecord(W->ev[1], s));
  k_extract<<<blocks(n), kThreads, 0, s>>>(h->d_words, h->d_word_off, h->d_kmer_off, n_seqs, n, h->k, d_ka);
  GB_HIP(hipEventRecord(W->ev[2], s));
  uint64_t *ka = d_ka, *kb = d_kb;
  radix_sort(s, &ka, &kb, nullptr, nullptr, n, 2 * h->k, d_table, d_sums);
  GB_HIP(hipEventRecord(W->ev[3], s));
  k_heads<<<blocks(n), kThreads, 0, s>>>(ka, n, d_heads);
  scan<uint8_t>(s, d_heads, n, d_pos, d_sums);
  GB_HIP(hipGetLastError());
  int64_t nd = 0;
  if ((st = scan_total(s, d_sums, n, &nd))) return st;
  h->n_distinct = nd;
  if ((st = h->d_codes.reserve((size_t)nd)) || (st = h->d_counts.reserve((size_t)nd)) ||
      (st = d_starts.reserve((size_t)nd + 1)))
    return st;
  k_runs<<<blocks(n), kThreads, 0, s>>>(ka, d_heads, d_pos, n, h->d_codes, d_starts);
  const uint32_t n32 = (uint32_t)n;
  GB_HIP(hipMemcpyAsync(d_starts + nd, &n32, 4, hipMemcpyHostToDevice, s));
  k_counts<<<blocks(nd), kThreads, 0, s>>>(d_starts, nd, h->d_counts);
  const int parts = (int)std::min<int64_t>(1024, blocks(nd));
  k_stats<<<parts, kThreads, 0, s>>>(h->d_counts, nd, d_part, d_part + 1024);
  GB_HIP(hipEventRecord(W->ev[4], s));
  uint32_t part[2048];
  GB_HIP(hipMemcpyAsync(part, d_part, sizeof part, hipMemcpyDeviceToHost, s));
  GB_HIP(hipStreamSynchronize(s));
  GB_HIP(hipGetLastError());
  for (int i = 0; i < parts; ++i) {
    h->max_count = std::max<int64_t>(h->max_count, part[i]);
    h->n_over15 += part[1024 + i];
  }
  GB_HIP(hipEventElapsedTime(&S.pack_ms, W->ev[0], W->ev[1]));
  GB_HIP(hipEventElapsedTime(&S.extract_ms, W->ev[1], W->ev[2]));
  GB_HIP(hipEventElapsedTime(&S.sort_ms, W->ev[2], W->ev[3]));
  GB_HIP(hipEventElapsedTime(&S.reduce_ms, W->ev[3], W->ev[4]));
  return GB_OK;
}

// One read's kept positions on the host: (rank, global position) of each, appended to out.
void index_read_host(const gb_kmer_counts *h, int64_t r, int32_t min_freq, float select_rate, int32_t tandem,
                     std::vector<std::pair<uint32_t, int64_t>> *out, std::vector<uint32_t> *scratch) {
  const int k = h->k;
  const int64_t n = h->kmer_off[(size_t)r + 1] - h->kmer_off[(size_t)r];
  if (n <= 0) return;
  const int64_t len = h->base_off[(size_t)r + 1] - h->base_off[(size_t)r], g0 = 2 * h->base_off[(size_t)r];
  const uint64_t *w = h->h_words.data() + h->word_off[(size_t)r];
  std::vector<uint32_t> &rank = scratch[0], &freq = scratch[1], &tmp = scratch[2];
  rank.resize((size_t)n), freq.resize((size_t)n);
  for (int64_t p = 0; p < n; ++p) {
    bool rev;
    const uint64_t c = canonical(window(w, p, k), k, &rev);
    const int64_t at = find_code(h->h_codes.data(), h->n_distinct, c);
    rank[(size_t)p] = (uint32_t)at | (rev ? kStrand : 0u);
    freq[(size_t)p] = h->h_counts[(size_t)at];
  }
  const int64_t maxk = std::min<int64_t>(n - 1, (int64_t)(size_t)(select_rate * (float)n));
  tmp = freq;
  std::nth_element(tmp.begin(), tmp.begin() + maxk, tmp.end(), std::greater<uint32_t>());
  const uint32_t thr = tmp[(size_t)maxk];
  tmp.clear();
  if (tandem > 0) {  // ranks of the candidates, sorted: a run longer than tandem is dropped
    for (int64_t p = 0; p < n; ++p)
      if (freq[(size_t)p] >= thr && freq[(size_t)p] > (uint32_t)tandem) tmp.push_back(rank[(size_t)p] & kRank);
    std::sort(tmp.begin(), tmp.end());
  }
  for (int64_t p = 0; p < n; ++p) {
    const uint32_t f = freq[(size_t)p], rk = rank[(size_t)p] & kRank;
    if (f < thr || f < (uint32_t)min_freq) continue;
    if (tandem > 0 && f > (uint32_t)tandem) {
      const auto range = std::equal_range(tmp.begin(), tmp.end(), rk);
      if (range.second - range.first > tandem) continue;
    }
    const bool rev = rank[(size_t)p] & kStrand;
    out->push_back({rk, rev ? g0 + len + (len - p - k) : g0 + p});
  }
}

// From the entries sorted by (rank, position) and their runs to the result: capacities, the filter scalars, the
// repetitive set and the lists.
int finish_index(const gb_kmer_counts *h, gb_kmer_idx *x, const int64_t *gpos, int64_t n_entries,
                 const uint32_t *run_rank, const uint32_t *run_start, int64_t n_runs, int32_t min_freq,
                 float repeat_rate) {
  size_t total = 0, unique = 0;
  auto cap = [&](int64_t j) { return (size_t)((j + 1 < n_runs ? run_start[j + 1] : (uint32_t)n_entries) - run_start[j]); };
  for (int64_t j = 0; j < n_runs; ++j)
    if (cap(j) >= (size_t)min_freq) total += cap(j), ++unique;
  const float mean = (float)total / (unique + 1);
  const size_t rep = (size_t)(repeat_rate * mean);
  x->rep_freq = (int64_t)rep;
  x->off.push_back(0);
  for (int64_t j = 0; j < n_runs; ++j) {
    const uint64_t code = h->h_codes[run_rank[j]];
    if (cap(j) > rep) {
      x->rep_codes.push_back(code);
    } else if ((size_t)h->h_counts[run_rank[j]] <= rep) {
      // every kept position of the code is appended, so capacity and list length are equal by construction
      x->codes.push_back(code);
      x->pos.insert(x->pos.end(), gpos + run_start[j], gpos + run_start[j] + cap(j));
      x->off.push_back((int64_t)x->pos.size());
      if ((size_t)(x->off.back() - x->off[x->off.size() - 2]) != cap(j)) {
        gb::set_error("gb_kmer_index: list of code %llu has %lld entries for capacity %zu",
                      (unsigned long long)code, (long long)(x->off.back() - x->off[x->off.size() - 2]), cap(j));
        return GB_ERR_STATE;
      }
    }
  }
  return GB_OK;
}

int index_host(const char *who, gb_kmer_counts *h, gb_kmer_idx *x, int32_t min_freq, float select_rate,
               int32_t tandem, float repeat_rate) {
  int nth = 1, st;
  if ((st = gb::thread_count(who, "GB_KMER_THREADS", &nth))) return st;
  nth = (int)std::max<int64_t>(1, std::min<int64_t>(nth, h->n_seqs));
  // reads in blocks, so that the entries come out in read order whatever thread took a block
  const int64_t n_blocks = std::min<int64_t>(h->n_seqs, 4 * nth);
  std::vector<std::vector<std::pair<uint32_t, int64_t>>> part((size_t)n_blocks);
  std::atomic<int64_t> next{0};
  if ((st = gb::parallel(who, nth, [&](int) {
         std::vector<uint32_t> scratch[3];
         for (int64_t b; (b = next.fetch_add(1)) < n_blocks;)
           for (int64_t r = h->n_seqs * b / n_blocks; r < h->n_seqs * (b + 1) / n_blocks; ++r)
             index_read_host(h, r, min_freq, select_rate, tandem, &part[(size_t)b], scratch);
       })))
    return st;
  std::vector<std::pair<uint32_t, int64_t>> all;
  for (auto &p : part) all.insert(all.end(), p.begin(), p.end());
  if ((st = par_sort(who, nth, all))) return st;
  std::vector<int64_t> gpos(all.size());
  std::vector<uint32_t> run_rank, run_start;
  for (size_t i = 0; i < all.size(); ++i) {
    gpos[i] = all[i].second;
    if (i == 0 || all[i].first != all[i - 1].first) run_rank.push_back(all[i].first), run_start.push_back((uint32_t)i);
  }
  return finish_index(h, x, gpos.data(), (int64_t)all.size(), run_rank.data(), run_start.data(),
                      (int64_t)run_rank.size(), min_freq, repeat_rate);
}

int index_device(const char *who, gb_kmer_counts *h, gb_kmer_idx *x, int32_t min_freq, float select_rate,
                 int32_t tandem, float repeat_rate) {
  int st, dev = -1;
  GB_HIP(hipGetDevice(&dev));
  GB_ARG(dev == h->dev, "%s: the counts live on device %d and the current device is %d", who, h->dev, dev);
  const int64_t n = h->n_occ, n_seqs = h->n_seqs, nd = h->n_distinct, tiles = tiles_of(n);
  int64_t budget = 0;
  if ((st = gb::env_number(who, "GB_KMER_WS", 1, INT64_MAX, kDefaultBudget, &budget))) return st;
  const int64_t need = index_ws_bytes(n, n_seqs);
  GB_ARG(need <= budget, "%s: the index of %lld occurrences needs %lld bytes of device workspace, above the budget of %lld (GB_KMER_WS)",
         who, (long long)n, (long long)need, (long long)budget);
  if ((st = mirror(h))) return st;
  Ws *W = nullptr;
  if ((st = gb::get_ws("gb_kmer", dev, &W))) return st;
  hipStream_t s = W->stream;
  Stats &S = stats();
  S.ws_bytes = need;

  std::vector<int64_t> maxk((size_t)n_seqs);
  for (int64_t r = 0; r < n_seqs; ++r) {
    const int64_t cnt = h->kmer_off[(size_t)r + 1] - h->kmer_off[(size_t)r];
    maxk[(size_t)r] = cnt > 0 ? std::min<int64_t>(cnt - 1, (int64_t)(size_t)(select_rate * (float)cnt)) : 0;
  }
  gb::DevBuf<int64_t> d_maxk;
  gb::DevBuf<uint32_t> d_rank, d_minf, d_pos, d_table, d_sums, d_run_start;
  gb::DevBuf<uint8_t> d_kept, d_cand, d_flags;
  gb::DevBuf<uint64_t> d_ka, d_kb, d_va, d_vb, d_run_key;
  if ((st = d_maxk.reserve((size_t)n_seqs)) || (st = d_minf.reserve((size_t)n_seqs)) ||
      (st = d_rank.reserve((size_t)n)) || (st = d_kept.reserve((size_t)n)) || (st = d_cand.reserve((size_t)n)) ||
      (st = d_flags.reserve((size_t)(2 * n))) || (st = d_pos.reserve((size_t)(2 * n))) ||
      (st = d_table.reserve((size_t)(256 * tiles + 1))) ||
      (st = d_sums.reserve((size_t)(tiles_of(std::max(2 * n, 256 * tiles)) + 2))))
    return st;
  GB_HIP(hipMemcpy(d_maxk, maxk.data(), 8 * (size_t)n_seqs, hipMemcpyHostToDevice));
  const Reads R{h->d_words, h->d_word_off, h->d_kmer_off, h->d_base_off, n_seqs, n, h->k};
  const int rank_bits = bits_of((uint64_t)(nd - 1));

  GB_HIP(hipEventRecord(W->ev[0], s));
  k_lookup<<<blocks(n), kThreads, 0, s>>>(R, h->d_codes, nd, d_rank);
  GB_HIP(hipEventRecord(W->ev[1], s));
  k_select<<<(int)n_seqs, kThreads, 0, s>>>(h->d_kmer_off, d_rank, h->d_counts, d_maxk, d_minf);
  GB_HIP(hipEventRecord(W->ev[2], s));
  k_keep<<<blocks(n), kThreads, 0, s>>>(R, d_rank, h->d_counts, d_minf, tandem, d_kept, d_cand);
  uint64_t *ka, *kb, *va, *vb;
  if (tandem > 0) {
    scan<uint8_t>(s, d_cand, n, d_pos, d_sums);
    int64_t nc = 0;
    if ((st = scan_total(s, d_sums, n, &nc))) return st;
    if (nc > 0) {
      if ((st = d_ka.reserve((size_t)nc)) || (st = d_kb.reserve((size_t)nc)) || (st = d_va.reserve((size_t)nc)) ||
          (st = d_vb.reserve((size_t)nc)))
        return st;
      ka = d_ka, kb = d_kb, va = d_va, vb = d_vb;
      k_cand_compact<<<blocks(n), kThreads, 0, s>>>(d_cand, d_pos, d_rank, n, ka, va);
      radix_sort(s, &ka, &kb, &va, &vb, nc, rank_bits, d_table, d_sums);
      k_tandem<<<blocks(nc), kThreads, 0, s>>>(R, ka, va, nc, tandem, d_kept);
    }
  }
  GB_HIP(hipMemsetAsync(d_flags, 0, (size_t)(2 * n), s));
  k_slot_flag<<<blocks(n), kThreads, 0, s>>>(R, d_rank, h->d_counts, d_kept, min_freq, d_flags);
  scan<uint8_t>(s, d_flags, 2 * n, d_pos, d_sums);
  int64_t ne = 0, nr = 0;
  if ((st = scan_total(s, d_sums, 2 * n, &ne))) return st;
  std::vector<int64_t> gpos((size_t)ne);
  std::vector<uint32_t> run_rank, run_start;
  if (ne > 0) {
    if ((st = d_ka.reserve((size_t)ne)) || (st = d_kb.reserve((size_t)ne)) || (st = d_va.reserve((size_t)ne)) ||
        (st = d_vb.reserve((size_t)ne)))
      return st;
    ka = d_ka, kb = d_kb, va = d_va, vb = d_vb;
    k_slot_compact<<<blocks(n), kThreads, 0, s>>>(R, d_rank, h->d_counts, d_kept, min_freq, d_pos, ka, va);
    radix_sort(s, &ka, &kb, &va, &vb, ne, rank_bits, d_table, d_sums);
    // the flags and their scan are done with: the run heads and their scan take their place
    k_heads<<<blocks(ne), kThreads, 0, s>>>(ka, ne, d_flags);
    scan<uint8_t>(s, d_flags, ne, d_pos, d_sums);
    if ((st = scan_total(s, d_sums, ne, &nr))) return st;
    if ((st = d_run_key.reserve((size_t)nr)) || (st = d_run_start.reserve((size_t)nr))) return st;
    k_runs<<<blocks(ne), kThreads, 0, s>>>(ka, d_flags, d_pos, ne, d_run_key, d_run_start);
  }
  GB_HIP(hipEventRecord(W->ev[3], s));
  GB_HIP(hipStreamSynchronize(s));
  GB_HIP(hipGetLastError());
  if (ne > 0) {
    std::vector<uint64_t> run_key((size_t)nr);
    run_start.resize((size_t)nr), run_rank.resize((size_t)nr);
    GB_HIP(gb::memcpy_big(gpos.data(), va, 8 * (size_t)ne, hipMemcpyDeviceToHost));
    GB_HIP(gb::memcpy_big(run_key.data(), d_run_key, 8 * (size_t)nr, hipMemcpyDeviceToHost));
    GB_HIP(gb::memcpy_big(run_start.data(), d_run_start, 4 * (size_t)nr, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < nr; ++j) run_rank[(size_t)j] = (uint32_t)run_key[(size_t)j];
  }
  GB_HIP(hipEventElapsedTime(&S.lookup_ms, W->ev[0], W->ev[1]));
  GB_HIP(hipEventElapsedTime(&S.select_ms, W->ev[1], W->ev[2]));
  GB_HIP(hipEventElapsedTime(&S.fill_ms, W->ev[2], W->ev[3]));
  return finish_index(h, x, gpos.data(), ne, run_rank.data(), run_start.data(), nr, min_freq, repeat_rate);
}

}  // namespace

extern "C" {

int gb_kmer_count(int k, const uint8_t *bytes, int64_t n_bytes, const int64_t *seq_off, int64_t n_seqs,
                  gb_kmer_counts **out) {
  const char *who = "gb_kmer_count";
  gb::Range range(who);
  GB_ARG(out, "%s: null out", who);
  GB_ARG(k >= 1 && k <= GB_KMER_MAX_K, "%s: k = %d is outside 1..%d", who, k, GB_KMER_MAX_K);
  GB_ARG(n_seqs >= 0 && n_bytes >= 0, "%s: negative count (n_seqs %lld, n_bytes %lld)", who, (long long)n_seqs,
         (long long)n_bytes);
  GB_ARG(n_seqs == 0 || (seq_off && (bytes || n_bytes == 0)), "%s: null array", who);
  for (int64_t i = 0; i < n_seqs; ++i)
    GB_ARG(seq_off[i] >= 0 && seq_off[i] <= seq_off[i + 1] && seq_off[i + 1] <= n_bytes,
           "%s: read %lld has offsets %lld..%lld in an array of %lld bytes", who, (long long)i, (long long)seq_off[i],
           (long long)seq_off[i + 1], (long long)n_bytes);
  int64_t n_occ = 0;
  for (int64_t i = 0; i < n_seqs; ++i) n_occ += std::max<int64_t>(0, seq_off[i + 1] - seq_off[i] - k);
  GB_ARG(n_occ <= GB_KMER_MAX_OCC, "%s: %lld occurrences, above the %lld of one call (a count could pass uint32)", who,
         (long long)n_occ, (long long)GB_KMER_MAX_OCC);
  int st, nth = 1;
  if ((st = gb::thread_count(who, "GB_KMER_THREADS", &nth))) return st;
  {  // the first byte that is no base, in read order
    std::atomic<int64_t> next{0}, bad{n_seqs};
    if ((st = gb::parallel(who, (int)std::max<int64_t>(1, std::min<int64_t>(nth, n_seqs)), [&](int) {
           for (int64_t r; (r = next.fetch_add(1)) < n_seqs && r < bad.load();)
             for (int64_t j = seq_off[r]; j < seq_off[r + 1]; ++j) {
               const uint8_t c = bytes[j] & 0xDF;
               if (c != 'A' && c != 'C' && c != 'G' && c != 'T') {
                 int64_t b = bad.load();
                 while (r < b && !bad.compare_exchange_weak(b, r)) {}
                 break;
               }
             }
         })))
      return st;
    if (bad.load() < n_seqs) {
      const int64_t r = bad.load();
      int64_t j = seq_off[r];
      for (;; ++j) {
        const uint8_t c = bytes[j] & 0xDF;
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') break;
      }
      GB_ARG(false, "%s: read %lld has byte 0x%02x at position %lld, which is no base", who, (long long)r, bytes[j],
             (long long)(j - seq_off[r]));
    }
  }
  gb_kmer_counts *h = nullptr;
  try {
    h = new gb_kmer_counts();
    h->k = k, h->n_seqs = n_seqs;
    h->base_off.assign((size_t)n_seqs + 1, 0), h->word_off = h->base_off, h->kmer_off = h->base_off;
    for (int64_t i = 0; i < n_seqs; ++i) {
      const int64_t len = seq_off[i + 1] - seq_off[i];
      h->base_off[(size_t)i + 1] = h->base_off[(size_t)i] + len;
      h->word_off[(size_t)i + 1] = h->word_off[(size_t)i] + (len + 31) / 32;
      h->kmer_off[(size_t)i + 1] = h->kmer_off[(size_t)i] + std::max<int64_t>(0, len - k);  // the reference's walk
    }
    h->n_occ = h->kmer_off[(size_t)n_seqs];
    Stats &S = stats();
    const int64_t calls = S.calls;
    if (h->n_occ == 0) {
      S = Stats{};
    } else if (gb::env_flag("GB_KMER_HOST")) {
      S = Stats{};
      st = count_host(who, h, bytes + seq_off[0]);
    } else {
      const int64_t span = seq_off[n_seqs] - seq_off[0], need = count_ws_bytes(h->n_occ, span);
      int64_t budget = 0;
      if (!(st = gb::env_number(who, "GB_KMER_WS", 1, INT64_MAX, kDefaultBudget, &budget)) && need > budget) {
        gb::set_error("%s: %lld occurrences need %lld bytes of device workspace, above the budget of %lld (GB_KMER_WS)",
                      who, (long long)h->n_occ, (long long)need, (long long)budget);
        st = GB_ERR_ARG;
      }
      if (!st) {
        S = Stats{};
        S.ws_bytes = need;
        h->host = false;
        st = count_device(who, h, bytes + seq_off[0], span);
      }
    }
    if (!st) {
      S.occ = h->n_occ, S.passes = h->n_occ ? (2 * k + 7) / 8 : 0, S.calls = calls + 1;
    }
  } catch (...) {
    gb::set_error("%s: out of host memory", who);
    st = GB_ERR_NOMEM;
  }
  if (st) {
    delete h;
    return st;
  }
  *out = h;
  return GB_OK;
}

void gb_kmer_free(gb_kmer_counts *h) { delete h; }

int gb_kmer_counts_stats(const gb_kmer_counts *h, int64_t *n_distinct, int64_t *n_occurrences, int64_t *n_over15,
                         int64_t *max_count) {
  GB_ARG(h, "gb_kmer_counts_stats: null handle");
  if (n_distinct) *n_distinct = h->n_distinct;
  if (n_occurrences) *n_occurrences = h->n_occ;
  if (n_over15) *n_over15 = h->n_over15;
  if (max_count) *max_count = h->max_count;
  return GB_OK;
}

int gb_kmer_counts_export(gb_kmer_counts *h, uint64_t *codes, uint32_t *counts, int64_t cap, int64_t *used) {
  const char *who = "gb_kmer_counts_export";
  GB_ARG(h && used, "%s: null argument", who);
  if (cap < h->n_distinct) {
    *used = h->n_distinct;
    GB_ARG(false, "%s: room for %lld codes, %lld needed", who, (long long)cap, (long long)h->n_distinct);
  }
  GB_ARG(h->n_distinct == 0 || (codes && counts), "%s: null array", who);
  if (const int st = mirror(h)) return st;
  if (h->n_distinct) {
    memcpy(codes, h->h_codes.data(), 8 * (size_t)h->n_distinct);
    memcpy(counts, h->h_counts.data(), 4 * (size_t)h->n_distinct);
  }
  *used = h->n_distinct;
  return GB_OK;
}

int gb_kmer_counts_freq(gb_kmer_counts *h, const uint64_t *codes, int64_t n, uint32_t *freq_out) {
  const char *who = "gb_kmer_counts_freq";
  GB_ARG(h && n >= 0 && (n == 0 || (codes && freq_out)), "%s: null or negative argument", who);
  if (const int st = mirror(h)) return st;
  for (int64_t i = 0; i < n; ++i) {  // a non-canonical code is absent from the list, as from the reference's table
    const int64_t at = find_code(h->h_codes.data(), h->n_distinct, codes[i]);
    freq_out[i] = at < 0 ? 0 : h->h_counts[(size_t)at];
  }
  return GB_OK;
}

int gb_kmer_counts_hist(gb_kmer_counts *h, int64_t *hist, int64_t n_bins) {
  const char *who = "gb_kmer_counts_hist";
  GB_ARG(h && hist && n_bins >= 1, "%s: null handle or array, or no bin", who);
  if (const int st = mirror(h)) return st;
  std::fill(hist, hist + n_bins, 0);
  for (uint32_t c : h->h_counts) ++hist[std::min<int64_t>(c, n_bins - 1)];
  return GB_OK;
}

int gb_kmer_index(gb_kmer_counts *h, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
                  gb_kmer_idx **out) {
  const char *who = "gb_kmer_index";
  gb::Range range(who);
  GB_ARG(h && out, "%s: null argument", who);
  GB_ARG(min_freq >= 1, "%s: min_freq = %d (need >= 1)", who, min_freq);
  GB_ARG(select_rate > 0.0f && select_rate < 1.0f, "%s: select_rate = %g is outside (0, 1)", who, (double)select_rate);
  GB_ARG(repeat_rate >= 0.0f && repeat_rate < 1e9f, "%s: repeat_rate = %g is outside [0, 1e9)", who,
         (double)repeat_rate);
  gb_kmer_idx *x = nullptr;
  int st = GB_OK;
  Stats &S = stats();
  S.lookup_ms = S.select_ms = S.fill_ms = 0;
  try {
    x = new gb_kmer_idx();
    if (h->n_occ == 0)
      x->off.push_back(0);
    else
      st = h->host ? index_host(who, h, x, min_freq, select_rate, tandem_freq, repeat_rate)
                   : index_device(who, h, x, min_freq, select_rate, tandem_freq, repeat_rate);
  } catch (...) {
    gb::set_error("%s: out of host memory", who);
    st = GB_ERR_NOMEM;
  }
  if (st) {
    delete x;
    return st;
  }
  *out = x;
  return GB_OK;
}

void gb_kmer_idx_free(gb_kmer_idx *x) { delete x; }

int gb_kmer_idx_stats(const gb_kmer_idx *x, int64_t *n_codes, int64_t *n_entries, int64_t *n_rep_codes,
                      int64_t *repetitive_frequency) {
  GB_ARG(x, "gb_kmer_idx_stats: null handle");
  if (n_codes) *n_codes = (int64_t)x->codes.size();
  if (n_entries) *n_entries = (int64_t)x->pos.size();
  if (n_rep_codes) *n_rep_codes = (int64_t)x->rep_codes.size();
  if (repetitive_frequency) *repetitive_frequency = x->rep_freq;
  return GB_OK;
}

int gb_kmer_idx_export(const gb_kmer_idx *x, uint64_t *codes, int64_t *off, int64_t code_cap, int64_t *pos,
                       int64_t pos_cap, uint64_t *rep_codes, int64_t rep_cap) {
  const char *who = "gb_kmer_idx_export";
  GB_ARG(x, "%s: null handle", who);
  const int64_t nc = (int64_t)x->codes.size(), ne = (int64_t)x->pos.size(), nr = (int64_t)x->rep_codes.size();
  GB_ARG(!(codes || off) || (codes && off && code_cap >= nc), "%s: room for %lld codes, %lld needed", who,
         (long long)code_cap, (long long)nc);
  GB_ARG(!pos || pos_cap >= ne, "%s: room for %lld positions, %lld needed", who, (long long)pos_cap, (long long)ne);
  GB_ARG(!rep_codes || rep_cap >= nr, "%s: room for %lld repetitive codes, %lld needed", who, (long long)rep_cap,
         (long long)nr);
  if (codes) {
    if (nc) memcpy(codes, x->codes.data(), 8 * (size_t)nc);
    memcpy(off, x->off.data(), 8 * (size_t)(nc + 1));
  }
  if (pos && ne) memcpy(pos, x->pos.data(), 8 * (size_t)ne);
  if (rep_codes && nr) memcpy(rep_codes, x->rep_codes.data(), 8 * (size_t)nr);
  return GB_OK;
}

int gb_kmer_timing(float *pack_ms, float *extract_ms, float *sort_ms, float *reduce_ms, float *lookup_ms,
                   float *select_ms, float *fill_ms, int64_t *occurrences) {
  const Stats &S = stats();
  if (!S.calls) {
    gb::set_error("gb_kmer_timing: no gb_kmer_count on this thread yet");
    return GB_ERR_STATE;
  }
  if (pack_ms) *pack_ms = S.pack_ms;
  if (extract_ms) *extract_ms = S.extract_ms;
  if (sort_ms) *sort_ms = S.sort_ms;
  if (reduce_ms) *reduce_ms = S.reduce_ms;
  if (lookup_ms) *lookup_ms = S.lookup_ms;
  if (select_ms) *select_ms = S.select_ms;
  if (fill_ms) *fill_ms = S.fill_ms;
  if (occurrences) *occurrences = S.occ;
  return GB_OK;
}

int gb_kmer_plan(int64_t *tile_keys, int64_t *sort_passes, int64_t *workspace_bytes) {
  const Stats &S = stats();
  if (tile_keys) *tile_keys = kTile;
  if (sort_passes) *sort_passes = S.passes;
  if (workspace_bytes) *workspace_bytes = S.ws_bytes;
  return GB_OK;
}

}  // extern "C"
