// Batched best-improvement 2-opt for TSP tours (co_tsp_two_opt; TSPEnv.local_search,
// tsp/env.py:192-197 -> tsp/local_search.py:14-74) for gfx950.
//
// Layout: one wavefront (a 64-thread workgroup) owns one row for its whole search -- all
// sweeps, the wave-wide argmin, the segment reversal and the termination test run inside
// the one launch.  LDS holds the tour, the per-position edge term
//   E[k] = D[tour[k-1], tour[k]]   (k = 0: the closing edge D[tour[n-1], tour[0]])
// and the distance source in tour order: the coordinates P[k] = locs[tour[k]] (a candidate
// then touches tour positions only), or the instance's distance matrix when it fits
// (n <= CO_TWO_OPT_STAGE_N: 4n^2 + 8(n+1) bytes <= 64 KiB); a larger matrix is read through
// L2.  The two subtracted operands of a move's `change` are E[i] and E[j+1]: the same f32
// values the reference recomputes, so `change` is bit-identical.
//
// A sweep scores the (n-1)(n-2)/2 moves (i, j), 1 <= i < j <= n-1.  Along a diagonal
// (i+1, j+1 follows i, j) the second added term of a move, D[t[i], t[j+1]], is the first
// added term of its successor, so every lane evaluates ONE distance g = D[t[i-1], t[j]] (one
// sqrt, or one matrix gather) and takes the other from the next lane.  The diagonals are
// laid end to end in a strip: diagonal d = j - i holds its n-1-d moves and then one closing
// element (j = n, read through the sentinels tour[n] = tour[0], P[n] = P[0]) that only
// supplies the last move's second term.  Diagonal r is followed by diagonal n-1-r, so each
// such pair is n+1 elements long and strip position x maps to (i, j) with one division by
// n+1 -- done once per lane, then advanced by the wave's step.  The wave walks the strip in
// windows of 64 positions that overlap by one: lanes 0..62 own a move each, lane 63 only
// feeds lane 62.  Each lane keeps a running (change, i<<16 | j) minimum, equal changes
// going to the lower key (the reference's ascending scan with a strict `<`); one wave
// reduction with the same rule gives the sweep's move.  After the reversal of tour[i..j]
// (and P[i..j]) only E[i..j+1] is recomputed, in the new (row, column) orientation.
#include "co_local_search.hpp"

using namespace co;

namespace {

static_assert(4 * CO_TWO_OPT_STAGE_N * CO_TWO_OPT_STAGE_N + 8 * (CO_TWO_OPT_STAGE_N + 1) <=
                  64 * 1024,
              "a staged matrix with the tour and edge terms must fit 64 KiB of LDS");
static_assert(CO_TWO_OPT_MAX_N < (1 << 15), "move keys pack j <= n into 16 bits");

template <int MODE>
__global__ __launch_bounds__(64) void two_opt_kernel(
    int64_t B, int n, const float* __restrict__ src, int64_t LB,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, int max_it,
    int64_t* __restrict__ out, int32_t* __restrict__ sweeps, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int* tour = reinterpret_cast<int*>(s_raw);                // n + 1 (sentinel)
  float* E = reinterpret_cast<float*>(s_raw + 4 * (n + 1));  // n (+ 1 of padding)
  uint32_t* bits = reinterpret_cast<uint32_t*>(E);  // the permutation bitmap, before E is built
  [[maybe_unused]] float2* P = reinterpret_cast<float2*>(s_raw + 8 * (n + 1));  // kCoords: n + 1
  [[maybe_unused]] float* Dl = reinterpret_cast<float*>(s_raw + 8 * (n + 1));   // kMatLds: n * n
  const int lane = threadIdx.x;
  // the strip: (n-2)(n+1)/2 elements in rows of n+1
  const int total = (n - 2) * (n + 1) / 2;
  const StripCursor start(lane, n + 1);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* arow = actions + b * sb;
    int64_t* orow = out + b * (int64_t)n;
    __syncthreads();  // the previous row's LDS reads are done
    for (int k = lane; k < ((n + 31) >> 5); k += 64) bits[k] = 0;
    __syncthreads();
    bool bad = false;
    for (int k = lane; k < n; k += 64) {
      const int64_t a = arow[(int64_t)k * st];
      if (a < 0 || a >= n) {
        bad = true;
      } else {
        tour[k] = (int)a;
        if (mark_once(bits, a)) bad = true;
      }
    }
    bad = __any(bad);
    if (bad || n < 3 || max_it <= 0) {  // wave-uniform: the row is copied
      if (bad && lane == 0) set_status(status, CO_ST_INVALID_TOUR);
      for (int k = lane; k < n; k += 64) orow[k] = arow[(int64_t)k * st];
      // n < 3: the reference's one sweep finds no candidate
      if (sweeps && lane == 0) sweeps[b] = (!bad && max_it > 0) ? 1 : 0;
      continue;
    }
    __syncthreads();
    const int64_t inst = LB == B ? b : b % LB;
    [[maybe_unused]] const float* Dg = src + inst * (int64_t)n * n;  // the matrix modes
    if (lane == 0) tour[n] = tour[0];
    if constexpr (MODE == kCoords) {
      const float2* lrow = reinterpret_cast<const float2*>(src) + inst * (int64_t)n;
      for (int k = lane; k <= n; k += 64) P[k] = lrow[tour[k == n ? 0 : k]];
    } else if constexpr (MODE == kMatLds) {
      for (int k = lane; k < n * n; k += 64) Dl[k] = Dg[k];
    }
    __syncthreads();
    // D[tour[ka], tour[kb]] for tour positions ka, kb (position n is position 0)
    const TourDist<MODE> dist{P, tour, MODE == kMatLds ? Dl : Dg, n};
    for (int k = lane; k < n; k += 64) E[k] = dist(k == 0 ? n - 1 : k - 1, k);
    __syncthreads();
    int it = 0;
    while (it < max_it) {
      float best = 0.f;  // the reference's delta = 0 with a strict `<`
      int bkey = 0x7fffffff;
      StripCursor cur = start;
      // every lane runs every window (the lane exchange needs the whole wave); the strip's
      // last element is a closing one, so the last move is at total - 2
      for (int x0 = 0; x0 < total - 1; x0 += kStep) {
        const TwoOptCandidate m = two_opt_candidate(cur, x0 + lane < total, lane, n, E, dist);
        const bool take =
            m.mine & ((m.change < best) | ((m.change == best) & (m.key < bkey)));
        best = take ? m.change : best;
        bkey = take ? m.key : bkey;
        cur.advance();
      }
      grp_argmin_split<64>(best, bkey);
      best = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(best)));
      bkey = __builtin_amdgcn_readfirstlane(bkey);
      ++it;
      if (!((double)best < -1e-6)) break;  // min_change = 0: the search ends
      const int p = bkey >> 16, r = bkey & 0xffff;  // reverse tour[p..r]
      if constexpr (MODE == kCoords) reverse_segment(lane, p, r, tour, P);
      else reverse_segment(lane, p, r, tour);
      __syncthreads();
      for (int k = p + lane; k <= r + 1; k += 64) {
        const int kk = k == n ? 0 : k;
        E[kk] = dist(kk == 0 ? n - 1 : kk - 1, kk);
      }
      __syncthreads();
    }
    for (int k = lane; k < n; k += 64) orow[k] = tour[k];
    if (sweeps && lane == 0) sweeps[b] = it;
  }
}

}  // namespace

extern "C" int co_tsp_two_opt(int64_t B, int64_t N, const float* locs, const float* distances,
                              int64_t locs_batch, const int64_t* actions, int64_t sb, int64_t st,
                              int64_t max_iterations, int64_t* actions_out, int32_t* sweeps_out,
                              int32_t* status, void* stream) {
  if (N <= 0 || N > CO_TWO_OPT_MAX_N) return CO_E_INVAL;
  const int rc = check_search_args(
      B, locs_batch, locs, distances,
      actions && actions_out && actions_out != actions && status, true);
  if (rc != CO_OK || B == 0) return rc;
  const int n = (int)N, max_it = clamp_iterations(max_iterations);
  const dim3 grid = row_grid(B);
  hipStream_t s = (hipStream_t)stream;
  const int state = 8 * (n + 1);  // tour + edge terms
#define CO_TWO_OPT(MODE, SRC, LDS)                                                              \
  hipLaunchKernelGGL(two_opt_kernel<MODE>, grid, dim3(64), (size_t)(LDS), s, B, n, SRC,         \
                     locs_batch, actions, sb, st, max_it, actions_out, sweeps_out, status)
  if (locs) CO_TWO_OPT(kCoords, locs, 2 * state);
  else if (n <= CO_TWO_OPT_STAGE_N) CO_TWO_OPT(kMatLds, distances, state + 4 * n * n);
  else CO_TWO_OPT(kMatGlobal, distances, state);
#undef CO_TWO_OPT
  return launch_status();
}
