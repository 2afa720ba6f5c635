// bsw_ksort.h -- bwa's ks_introsort and ks_combsort (ksort.h:154-226) restated for host and device,
// templated on the element and on the comparison. The sort is not stable and callers depend on the
// order it leaves among equal elements, so every detail is the reference's: n < 1 returns, n == 2 is
// one compare and swap, the depth counter with its comb-sort fallback, the median of three that swaps
// the pivot to the end, the push only of sides longer than 16, the closing insertion sort over the
// whole array. bsw_mkchain.hip keeps its own copy on 8-byte keys; this one moves whole records.
#pragma once
#include <hip/hip_runtime.h>

namespace gbks {

constexpr int kSortStack = 64;  // the pushed depths decrease strictly and start below 2 * 31

template <typename T>
__host__ __device__ inline void swap2(T *a, int i, int j) {
  const T t = a[i];
  a[i] = a[j], a[j] = t;
}

template <typename T, typename LT>
__host__ __device__ inline void insertsort(T *a, int n, LT lt) {
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && lt(a[j], a[j - 1]); --j) swap2(a, j, j - 1);
}

template <typename T, typename LT>
__host__ __device__ inline void combsort(T *a, int n, LT lt) {
  const double shrink_factor = 1.2473309501039786540366528676643;
  int do_swap, gap = n;
  do {
    if (gap > 2) {
      gap = (int)(gap / shrink_factor);
      if (gap == 9 || gap == 10) gap = 11;
    }
    do_swap = 0;
    for (int i = 0; i < n - gap; ++i) {
      const int j = i + gap;
      if (lt(a[j], a[i])) {
        swap2(a, i, j);
        do_swap = 1;
      }
    }
  } while (do_swap || gap > 2);
  if (gap != 1) insertsort(a, n, lt);
}

template <typename T, typename LT>
__host__ __device__ inline void introsort(T *a, int n, LT lt) {
  if (n < 1) return;
  if (n == 2) {
    if (lt(a[1], a[0])) swap2(a, 0, 1);
    return;
  }
  int d;
  for (d = 2; (1ll << d) < n; ++d) {
  }
  int sl[kSortStack], sr[kSortStack], sd[kSortStack], top = 0;
  int s = 0, t = n - 1;
  d <<= 1;
  for (;;) {
    if (s < t) {
      if (--d == 0) {
        combsort(a + s, t - s + 1, lt);
        t = s;
        continue;
      }
      int i = s, j = t, k = i + ((j - i) >> 1) + 1;
      if (lt(a[k], a[i])) {
        if (lt(a[k], a[j])) k = j;
      } else {
        k = lt(a[j], a[i]) ? i : j;
      }
      const T rp = a[k];
      if (k != t) swap2(a, k, t);
      for (;;) {
        do ++i;
        while (lt(a[i], rp));
        do --j;
        while (i <= j && lt(rp, a[j]));
        if (j <= i) break;
        swap2(a, i, j);
      }
      swap2(a, i, t);
      if (i - s > t - i) {
        if (i - s > 16 && top < kSortStack) sl[top] = s, sr[top] = i - 1, sd[top] = d, ++top;
        s = t - i > 16 ? i + 1 : t;
      } else {
        if (t - i > 16 && top < kSortStack) sl[top] = i + 1, sr[top] = t, sd[top] = d, ++top;
        t = i - s > 16 ? i - 1 : s;
      }
    } else {
      if (top == 0) {
        insertsort(a, n, lt);
        return;
      }
      --top;
      s = sl[top], t = sr[top], d = sd[top];
    }
  }
}

}  // namespace gbks
