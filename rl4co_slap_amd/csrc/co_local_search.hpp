// What the batched local searches share (tsp_ls.hip, cvrp_ls.hip, slap_ls.hip):
// only pieces that at least two of them use.  Each kernel keeps its own admissibility test,
// running minimum and move application; slap_ls.hip takes the bitmap and the entry-point
// helpers alone.
#pragma once

#include "co_common.hpp"

namespace co {

// where a tour kernel reads its distances: the coordinates in tour order (LDS), the
// instance's matrix staged in LDS, or the matrix through L2
constexpr int kCoords = 0, kMatLds = 1, kMatGlobal = 2;
constexpr int kStep = 63;  // strip positions a window advances by (64 lanes, one shared)

// ---------------------------------------------------------------------------
// The diagonal strip of the 2-opt moves (i, j), 1 <= i < j <= n-1, of a cyclic tour of n
// positions (tsp_ls.hip describes the walk; cvrp_ls.hip walks it too).  Element c of strip
// row q (0 <= c <= n): row q holds diagonal r = q + 1 (n - r elements, the closing one
// included) and then diagonal n-1-r (r + 1 elements).  An odd middle diagonal (n-1)/2 ends
// the strip as the first part of a last, half-filled row.  j == n marks a closing element.
struct StripMove {
  int i, j;
};

__device__ __forceinline__ StripMove strip_move(int q, int c, int n) {
  const int r = q + 1, a = n - r;
  const bool first = c < a;
  const int d = first ? r : n - 1 - r, t = first ? c : c - a;
  StripMove m;
  m.i = 1 + t;
  m.j = 1 + t + d;
  return m;
}

// A lane's place in a strip laid out in rows of `width`: element `lane` of the first
// window as (row q, column c) -- one division per lane -- and advance() to the same lane
// of the next window.
struct StripCursor {
  int q, c, step_q, step_c, width;
  __device__ __forceinline__ StripCursor(int lane, int width_)
      : q(lane / width_), c(lane - q * width_), step_q(kStep / width_),
        step_c(kStep - step_q * width_), width(width_) {}
  __device__ __forceinline__ void advance() {
    q += step_q;
    c += step_c;
    if (c >= width) {
      c -= width;
      ++q;
    }
  }
};

// D[node[ka], node[kb]] for tour positions ka, kb: from the coordinates in tour order P, or
// from the V x V matrix D (in LDS or global memory; the pointer says which)
template <int MODE>
struct TourDist {
  const float2* P;
  const int* node;
  const float* D;
  int V;
  __device__ __forceinline__ float operator()(int ka, int kb) const {
    if constexpr (MODE == kCoords) {
      const float2 p = P[ka], q = P[kb];
      return edge_len(p.x, p.y, q.x, q.y);
    } else {
      return D[node[ka] * V + node[kb]];
    }
  }
};

// The 2-opt move of a strip element in a tour of n positions with edge terms E: a lane
// evaluates ONE distance, D[t[i-1], t[j]]; D[t[i], t[j+1]] is its successor's, taken from
// the next lane (DPP wave_shl:1: lane l reads lane l + 1; lane 63 reads 0 and owns no
// move).  Every lane of the wave must call it; an idle lane (`live` false) scores move
// (1, 2) and is not `mine`.
struct TwoOptCandidate {
  float change;
  int key, i, j;  // key = i << 16 | j
  bool mine;
};

template <class Dist>
__device__ __forceinline__ TwoOptCandidate two_opt_candidate(const StripCursor& cur, bool live,
                                                             int lane, int n, const float* E,
                                                             const Dist& dist) {
  const StripMove m = strip_move(live ? cur.q : 0, live ? cur.c : 0, n);
  const float g = dist(m.i - 1, m.j);
  const float g_next = __uint_as_float(dpp_u<0x130>(__float_as_uint(g)));
  const int jn = m.j + 1 >= n ? 0 : m.j + 1;
  TwoOptCandidate cand;
  cand.change = ((g + g_next) - E[m.i]) - E[jn];
  cand.key = (m.i << 16) | m.j;
  cand.i = m.i;
  cand.j = m.j;
  cand.mine = live & (lane < kStep) & (m.j < n);
  return cand;
}

// The wave's best candidate from every lane's running (change, key) minimum, equal changes
// going to the lower key; the result is wave-uniform (scalar registers).
__device__ __forceinline__ void wave_best_move(float& best, int& bkey) {
  grp_argmin_split<64>(best, bkey);
  best = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(best)));
  bkey = __builtin_amdgcn_readfirstlane(bkey);
}

// Reverse positions p..r of every array of the pack (the wave's 64 lanes share the swaps).
template <class... T>
__device__ __forceinline__ void reverse_segment(int lane, int p, int r, T*... arrays) {
  for (int t = lane; t < ((r - p + 1) >> 1); t += 64) {
    const int u = p + t, v = r - t;
    auto swap = [&](auto* a) {
      const auto au = a[u];
      a[u] = a[v];
      a[v] = au;
    };
    (swap(arrays), ...);
  }
}

// Set bit a of a bitmap; true if it was already set (a seen a second time).
template <class Int>
__device__ __forceinline__ bool mark_once(uint32_t* bits, Int a) {
  const uint32_t bit = 1u << (a & 31);
  return atomicOr(&bits[a >> 5], bit) & bit;
}

// ---------------------------------------------------------------------------
// Entry points.

inline int clamp_iterations(int64_t max_iterations) {
  return max_iterations > INT32_MAX ? INT32_MAX : max_iterations < 0 ? 0 : (int)max_iterations;
}

// one workgroup per row; rows beyond 2^22 are reached by the kernels' grid stride
inline dim3 row_grid(int64_t B) { return dim3((unsigned)(B < (1 << 22) ? B : (1 << 22))); }

// The checks every search makes after those of its own sizes: the batch (B == 0 is CO_OK
// and launches nothing: the caller returns), exactly one distance source, the entry point's
// other required pointers (`others_given`), then the alignment -- of locs (float2),
// distances and of the entry point's other arrays (`others_aligned`).
inline int check_search_args(int64_t B, int64_t locs_batch, const float* locs,
                             const float* distances, bool others_given, bool others_aligned) {
  if (B < 0 || locs_batch <= 0 || (B > 0 && B % locs_batch != 0)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if ((locs == nullptr) == (distances == nullptr) || !others_given) return CO_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(locs) & 7) || (reinterpret_cast<uintptr_t>(distances) & 3) ||
      !others_aligned)
    return CO_E_ALIGN;
  return CO_OK;
}

}  // namespace co
