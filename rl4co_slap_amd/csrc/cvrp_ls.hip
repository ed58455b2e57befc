// Batched giant-tour local search for CVRP rollouts (co_cvrp_local_search; CVRPEnv.improve)
// for gfx950: best-improvement 2-opt + relocate under an exact integer capacity test.
// include/co_env.h states the search; tests/cvrp_ls_ref.py restates it in numpy.
//
// Layout: as tsp_ls.hip, one wavefront (a 64-thread workgroup) owns one row for its whole
// search.  LDS holds, per tour position k (slots = min(T, 2N) + 2: the longest giant tour
// plus the sentinel position m = position 0):
//   g[k]     the node                    P[k]  its coordinates (coordinate path only)
//   E[k]     D[g[k-1], g[k]]             (k = 0: the closing edge D[g[m-1], g[0]])
//   R[k]     (D[g[k-1], g[k+1]] - E[k]) - E[k+1]: what taking g[k] out of the tour changes
//   Q[k]     the quantised demand of g[k] (int64, 0 at a depot)
//   head[k]  the load of k's route up to and including k, tail[k] from k to the route's end
//   PZ[k]    the last depot position <= k
// and the instance's distance matrix when it is given and fits (num_loc <=
// CO_CVRP_LS_STAGE_N); a larger matrix is read through L2.  g, P and Q move with a move;
// E, R, head, tail and PZ are rebuilt after it -- O(m) against the sweep's O(m^2) -- the
// loads by a segmented scan (a chunk of positions per lane, one wave scan across lanes).
//
// With these, "g[i..j] holds no depot" is PZ[j] < i, the two boundary routes a 2-opt move
// across a depot creates weigh head[i-1] + head[j] and tail[i] + tail[j+1], "gap j lies in
// i's route" is PZ[j] == PZ[i] and a relocate target weighs head[j] + tail[j+1]: every
// admissibility test is O(1).  It is made only for a candidate that would beat the lane's
// running best, so most candidates cost their f32 change alone.
//
// A sweep walks two strips in windows of 64 positions that overlap by one (lanes 0..62 own
// a candidate each, lane 63 only feeds lane 62), one distance per candidate:
//  - the 2-opt moves along diagonals, exactly tsp_ls.hip's strip (n = m);
//  - the relocate candidates row by row: row i holds j = 0..m-1 and a closing element
//    j = m.  D[c, g[j+1]] is the next element's D[g[j+1], c] on the coordinate path (the
//    same dx*dx + dy*dy), taken from the next lane; a matrix may be asymmetric, so the
//    matrix paths gather both.
// Each lane keeps a running (change, key) minimum, key = kind << 30 | i << 16 | j, equal
// changes going to the lower key (2-opt before relocate, then i, then j); one wave
// reduction with the same rule gives the sweep's move.
#include "co_local_search.hpp"

using namespace co;

namespace {

constexpr int kRelocate = 1 << 30;

static_assert(4 * (CO_CVRP_LS_STAGE_N + 1) * (CO_CVRP_LS_STAGE_N + 1) +
                      40 * (2 * CO_CVRP_LS_STAGE_N + 2) <=
                  64 * 1024,
              "a staged matrix with the tour state must fit 64 KiB of LDS");
static_assert(48 * (CO_CVRP_LS_MAX_LEN + 1) <= 64 * 1024, "the tour state must fit 64 KiB");
static_assert(CO_CVRP_LS_MAX_LEN < (1 << 14), "move keys pack i into 14 bits, j into 16");

__device__ __forceinline__ bool in_range(float x) { return x >= 0.f && x <= 4096.f; }  // no NaN
__device__ __forceinline__ int64_t quantise(float x) {
  return __double2ll_rn((double)x * 1099511627776.0);  // llrint(x * 2^40)
}

template <int MODE>
__global__ __launch_bounds__(64) void cvrp_ls_kernel(
    int64_t B, int N, int T, int slots, const float* __restrict__ src,
    const float* __restrict__ demand, const float* __restrict__ capacity, int64_t LB,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, int max_it,
    int64_t* __restrict__ out, int32_t* __restrict__ sweeps, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int64_t* head = reinterpret_cast<int64_t*>(s_raw);
  int64_t* tail = head + slots;
  int64_t* Q = tail + slots;
  unsigned char* rest = s_raw + 24 * slots;
  [[maybe_unused]] float2* P = reinterpret_cast<float2*>(rest);  // kCoords only
  if constexpr (MODE == kCoords) rest += 8 * slots;
  int* g = reinterpret_cast<int*>(rest);
  float* E = reinterpret_cast<float*>(rest + 4 * slots);
  float* R = reinterpret_cast<float*>(rest + 8 * slots);
  int* PZ = reinterpret_cast<int*>(rest + 12 * slots);
  [[maybe_unused]] float* Dl = reinterpret_cast<float*>(rest + 16 * slots);  // kMatLds: V * V
  uint32_t* bits = reinterpret_cast<uint32_t*>(E);  // the customer bitmap, before E is built
  const int lane = threadIdx.x;
  const int V = N + 1;  // nodes, depot first
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* arow = actions + b * sb;
    int64_t* orow = out + b * (int64_t)T;
    const int64_t inst = LB == B ? b : b % LB;
    const float* drow = demand + inst * (int64_t)N;
    const float cap = capacity ? capacity[inst] : 1.0f;
    __syncthreads();  // the previous row's LDS reads are done
    for (int k = lane; k < ((V + 31) >> 5); k += 64) bits[k] = 0;
    __syncthreads();
    // ---- the row check
    bool bad = !in_range(cap);
    int customers = 0;
    for (int k = lane; k < T; k += 64) {
      const int64_t a = arow[(int64_t)k * st];
      if (a < 0 || a > N) {
        bad = true;
      } else if (a > 0) {
        ++customers;
        if (mark_once(bits, a)) bad = true;
      }
    }
    for (int c = lane; c < N; c += 64) bad |= !in_range(drow[c]);
    customers = wave_sum(customers);
    bad = __any(bad) || customers != N;
    if (bad) {  // wave-uniform: the row is copied
      if (lane == 0) set_status(status, CO_ST_INVALID_TOUR);
      for (int k = lane; k < T; k += 64) orow[k] = arow[(int64_t)k * st];
      if (sweeps && lane == 0) sweeps[b] = 0;
      continue;
    }
    __syncthreads();  // the bitmap (in E's place) is no longer read
    // ---- the giant tour: g[0] = 0, the entries without a 0 after a 0, no trailing 0.  A
    // valid row keeps at most min(T, 2N) entries, so every write stays below slots - 1.
    int m = 1;
    if (lane == 0) g[0] = 0;
    for (int base = 0; base < T; base += 64) {
      const int k = base + lane;
      const int64_t a = k < T ? arow[(int64_t)k * st] : 0;
      const int64_t prev = (k > 0 && k < T) ? arow[(int64_t)(k - 1) * st] : 0;
      const bool keep = k < T && (a != 0 || prev != 0);
      const uint64_t mask = __ballot(keep);
      if (keep) g[m + __popcll(mask & below)] = (int)a;
      m += __popcll(mask);
    }
    __syncthreads();
    if (m > 1 && __builtin_amdgcn_readfirstlane(g[m - 1]) == 0) --m;
    __syncthreads();
    [[maybe_unused]] const float* Dg = src + inst * (int64_t)V * V;  // the matrix modes
    for (int k = lane; k <= m; k += 64) {  // position m is the sentinel: position 0
      const int node = k == m ? 0 : g[k];
      if (k == m) g[k] = 0;
      Q[k] = node ? quantise(drow[node - 1]) : 0;
      if constexpr (MODE == kCoords)
        P[k] = (reinterpret_cast<const float2*>(src) + inst * (int64_t)V)[node];
    }
    if constexpr (MODE == kMatLds)
      for (int k = lane; k < V * V; k += 64) Dl[k] = Dg[k];
    __syncthreads();
    const int64_t cap_q = quantise(cap) + (int64_t(1) << 20);
    // D[g[ka], g[kb]] for tour positions ka, kb <= m
    const TourDist<MODE> dist{P, g, MODE == kMatLds ? Dl : Dg, V};
    // E, R, head, tail, PZ from g, P, Q (all of them: O(m))
    auto rebuild = [&]() {
      for (int k = lane; k < m; k += 64) E[k] = dist(k == 0 ? m - 1 : k - 1, k);
      // the loads: lane l owns positions [k0, k1) of the m + 1 (the sentinel included)
      const int chunk = (m + 1 + 63) >> 6;
      const int k0 = min(lane * chunk, m + 1), k1 = min(k0 + chunk, m + 1);
      {  // forward: (load since the last depot, that depot's position or -1)
        int64_t s = 0;
        int lz = -1;
        for (int k = k0; k < k1; ++k) {
          const bool z = g[k] == 0;
          s = z ? 0 : s + Q[k];
          lz = z ? k : lz;
        }
        for (int d = 1; d < 64; d <<= 1) {  // inclusive scan: a depot of mine cuts the carry
          const int64_t os = __shfl_up(s, d, 64);
          const int olz = __shfl_up(lz, d, 64);
          if (lane >= d && lz < 0) {
            s += os;
            lz = olz;
          }
        }
        int64_t carry = __shfl_up(s, 1, 64);
        int pz = __shfl_up(lz, 1, 64);
        if (lane == 0) carry = 0, pz = 0;  // g[0] = 0 resets both at once
        for (int k = k0; k < k1; ++k) {
          const bool z = g[k] == 0;
          carry = z ? 0 : carry + Q[k];
          pz = z ? k : pz;
          head[k] = carry;
          PZ[k] = pz;
        }
      }
      {  // backward: (load up to the next depot, whether the chunk holds one)
        int64_t s = 0;
        int hz = 0;
        for (int k = k1 - 1; k >= k0; --k) {
          const bool z = g[k] == 0;
          s = z ? 0 : s + Q[k];
          hz |= z;
        }
        for (int d = 1; d < 64; d <<= 1) {
          const int64_t os = __shfl_down(s, d, 64);
          const int ohz = __shfl_down(hz, d, 64);
          if (lane + d < 64 && !hz) {
            s += os;
            hz = ohz;
          }
        }
        int64_t carry = __shfl_down(s, 1, 64);
        if (lane == 63) carry = 0;
        for (int k = k1 - 1; k >= k0; --k) {
          carry = g[k] == 0 ? 0 : carry + Q[k];
          tail[k] = carry;
        }
      }
      __syncthreads();  // E is complete
      for (int k = 1 + lane; k < m; k += 64)
        R[k] = (dist(k - 1, k + 1) - E[k]) - E[k + 1 == m ? 0 : k + 1];
      __syncthreads();
    };
    // the strips: (m-2)(m+1)/2 2-opt elements and (m-1)(m+1) relocate elements, both in
    // rows of m + 1
    const int total2 = (m - 2) * (m + 1) / 2, total_r = (m - 1) * (m + 1);
    const StripCursor start(lane, m + 1);
    int it = 0;
    while (it < max_it) {
      rebuild();
      float best = 0.f;  // only a change < 0 counts
      int bkey = 0x7fffffff;
      StripCursor cur = start;
      // every lane runs every window (the lane exchange needs the whole wave); a strip's
      // last element is a closing one, so its last candidate is at total - 2
      for (int x0 = 0; x0 < total2 - 1; x0 += kStep) {  // m < 3: no 2-opt move
        const TwoOptCandidate mv = two_opt_candidate(cur, x0 + lane < total2, lane, m, E, dist);
        if (mv.mine & ((mv.change < best) | ((mv.change == best) & (mv.key < bkey)))) {
          // a depot inside g[i..j]: both new boundary routes must fit
          const bool ok = PZ[mv.j] < mv.i || (head[mv.i - 1] + head[mv.j] <= cap_q &&
                                              tail[mv.i] + tail[mv.j + 1] <= cap_q);
          best = ok ? mv.change : best;
          bkey = ok ? mv.key : bkey;
        }
        cur.advance();
      }
      cur = start;
      for (int x0 = 0; x0 < total_r - 1; x0 += kStep) {
        const bool live = x0 + lane < total_r;
        const int i = live ? 1 + cur.q : 1, j = live ? cur.c : 0;  // j == m: the closing element
        const float d = dist(j, i);                        // D[a, c]
        float d_next;                                      // D[c, b]
        if constexpr (MODE == kCoords)
          d_next = __uint_as_float(dpp_u<0x130>(__float_as_uint(d)));
        else
          d_next = dist(i, j < m ? j + 1 : 0);
        const int jn = j + 1 >= m ? 0 : j + 1;
        const float change = ((d + d_next) - E[jn]) + R[i];
        const int key = kRelocate | (i << 16) | j;
        const bool mine = live & (lane < kStep) & (j < m) & (g[i] != 0) & (j != i) & (j != i - 1);
        if (mine & ((change < best) | ((change == best) & (key < bkey)))) {
          // another route: it must take the customer
          const bool ok = PZ[j] == PZ[i] || head[j] + tail[j + 1] + Q[i] <= cap_q;
          best = ok ? change : best;
          bkey = ok ? key : bkey;
        }
        cur.advance();
      }
      wave_best_move(best, bkey);
      ++it;
      if (!((double)best < -1e-6)) break;  // nothing applied: the search ends
      const int p = (bkey >> 16) & 0x3fff, r = bkey & 0xffff;
      __syncthreads();
      if (!(bkey & kRelocate)) {  // reverse g[p..r]
        if constexpr (MODE == kCoords) reverse_segment(lane, p, r, g, Q, P);
        else reverse_segment(lane, p, r, g, Q);
      } else {  // g[p] goes between positions r and r + 1: the positions between shift by one
        const int cg = g[p];
        const int64_t cq = Q[p];
        [[maybe_unused]] float2 cp;
        if constexpr (MODE == kCoords) cp = P[p];
        const int dir = r > p ? 1 : -1;            // the side the elements come from
        const int first = p, last = r > p ? r - 1 : r + 2;  // destinations first..last
        const int count = (last - first) * dir + 1;
        __syncthreads();
        for (int base = 0; base < count; base += 64) {  // in the order that frees positions
          const int k = first + (base + lane) * dir;
          const bool act = base + lane < count;
          int ng = 0;
          int64_t nq = 0;
          [[maybe_unused]] float2 np;
          if (act) {
            ng = g[k + dir];
            nq = Q[k + dir];
            if constexpr (MODE == kCoords) np = P[k + dir];
          }
          __syncthreads();
          if (act) {
            g[k] = ng;
            Q[k] = nq;
            if constexpr (MODE == kCoords) P[k] = np;
          }
          __syncthreads();
        }
        if (lane == 0) {
          const int dst = r > p ? r : r + 1;
          g[dst] = cg;
          Q[dst] = cq;
          if constexpr (MODE == kCoords) P[dst] = cp;
        }
      }
      __syncthreads();
    }
    // ---- the routes in order, single zeros between them, zeros up to T
    int w = 0;
    for (int base = 1; base < m; base += 64) {
      const int k = base + lane;
      const int v = k < m ? g[k] : 0, pv = k < m ? g[k - 1] : 0;
      const bool keep = k < m && (v != 0 || pv != 0);
      const uint64_t mask = __ballot(keep);
      if (keep) orow[w + __popcll(mask & below)] = v;
      w += __popcll(mask);
    }
    for (int k = w + lane; k < T; k += 64) orow[k] = 0;
    if (sweeps && lane == 0) sweeps[b] = it;
  }
}

}  // namespace

extern "C" int co_cvrp_local_search(int64_t B, int64_t N, int64_t T, const float* locs,
                                    const float* distances, const float* demand,
                                    const float* capacity, int64_t locs_batch,
                                    const int64_t* actions, int64_t sb, int64_t st,
                                    int64_t max_iterations, int64_t* actions_out,
                                    int32_t* sweeps_out, int32_t* status, void* stream) {
  if (N < 1 || T < N) return CO_E_INVAL;
  const int64_t len = (T < 2 * N ? T : 2 * N) + 1;  // the longest giant tour
  if (len > CO_CVRP_LS_MAX_LEN) return CO_E_INVAL;
  const int rc = check_search_args(
      B, locs_batch, locs, distances,
      demand && actions && actions_out && actions_out != actions && status,
      !((reinterpret_cast<uintptr_t>(demand) | reinterpret_cast<uintptr_t>(capacity)) & 3));
  if (rc != CO_OK || B == 0) return rc;
  const int n = (int)N, steps = (int)T, slots = (int)len + 1;  // + the sentinel
  const int max_it = clamp_iterations(max_iterations);
  const dim3 grid = row_grid(B);
  hipStream_t s = (hipStream_t)stream;
#define CO_CVRP_LS(MODE, SRC, LDS)                                                              \
  hipLaunchKernelGGL(cvrp_ls_kernel<MODE>, grid, dim3(64), (size_t)(LDS), s, B, n, steps,       \
                     slots, SRC, demand, capacity, locs_batch, actions, sb, st, max_it,         \
                     actions_out, sweeps_out, status)
  if (locs) CO_CVRP_LS(kCoords, locs, 48 * slots);
  else if (n <= CO_CVRP_LS_STAGE_N) CO_CVRP_LS(kMatLds, distances, 40 * slots + 4 * (n + 1) * (n + 1));
  else CO_CVRP_LS(kMatGlobal, distances, 40 * slots);
#undef CO_CVRP_LS
  return launch_status();
}
