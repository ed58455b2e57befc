// Batched best-improvement local search for TSP tours for gfx950: 2-opt alone
// (co_tsp_two_opt; TSPEnv.local_search, tsp/env.py:192-197 -> tsp/local_search.py:14-74) and
// the 2-opt + Or-opt descent (co_tsp_local_search; TSPEnv.local_search with operators=...).
// include/co_env.h states the moves, the f32 scoring order and the tie rule.  Both entry
// points launch one kernel template; OR_OPT = false compiles the Or-opt half and its LDS
// array out and is what a 2-opt-only search runs.
//
// Layout: one wavefront (a 64-thread workgroup) owns one row for its whole search -- all
// sweeps, the wave-wide argmin, the move and the termination test run inside the one
// launch.  LDS holds the tour (n + 1: the sentinel tour[n] = tour[0]), the per-position
// edge term
//   E[k] = D[tour[k-1], tour[k]]   (k = 0: the closing edge D[tour[n-1], tour[0]])
// with OR_OPT the per-segment joining edge A[i] = D[tour[i-1], tour[i+L]] of the segment
// length L being scanned, and the distance source in tour order: the coordinates
// P[k] = locs[tour[k]] (a candidate then touches tour positions only), or the instance's
// distance matrix when it fits (n <= CO_TWO_OPT_STAGE_N: 4n^2 + the state's 8(n+1) bytes,
// with A 12(n+1) + 12, <= 64 KiB); a larger matrix is read through L2.  The two subtracted
// operands of a 2-opt move's `change` are E[i] and E[j+1]: the same f32 values the
// reference recomputes, so `change` is bit-identical.
//
// The 2-opt sweep scores the (n-1)(n-2)/2 moves (i, j), 1 <= i < j <= n-1.  Along a
// diagonal (i+1, j+1 follows i, j) the second added term of a move, D[t[i], t[j+1]], is the
// first added term of its successor, so every lane evaluates ONE distance
// g = D[t[i-1], t[j]] (one sqrt, or one matrix gather) and takes the other from the next
// lane.  The diagonals are laid end to end in a strip: diagonal d = j - i holds its n-1-d
// moves and then one closing element (j = n, read through the sentinels tour[n] = tour[0],
// P[n] = P[0]) that only supplies the last move's second term.  Diagonal r is followed by
// diagonal n-1-r, so each such pair is n+1 elements long and strip position x maps to
// (i, j) with one division by n+1 -- done once per lane, then advanced by the wave's step.
// The wave walks the strip in windows of 64 positions that overlap by one: lanes 0..62 own
// a move each, lane 63 only feeds lane 62.  Each lane keeps a running (change, i<<16 | j)
// minimum, equal changes going to the lower key (the reference's ascending scan with a
// strict `<`); one wave reduction with the same rule gives the sweep's move.  After the
// reversal of tour[i..j] (and P[i..j]) only E[i..j+1] is recomputed, in the new (row,
// column) orientation.
//
// The Or-opt scan.  For one L the candidates (i, k, rev) form a table of n - L rows
// (i = 1 .. n-L) by n columns (k = 0 .. n-1).  Of a candidate's six terms, E[i], E[i+L]
// and A[i] belong to the row and E[k+1] to the column (all LDS reads); only D[c, x] and
// D[y, d] are new distances.  D[c, x] joins position k to a segment end, D[y, d] joins a
// segment end to position k+1 -- the same pair of (position, segment end) one column on.
// So a lane at (i, k) evaluates its position k against the two segment ends, as row
// ("to": D[t[k], s]) and as column ("from": D[s, t[k]]), and takes the "from" pair of
// column k+1 from the next lane (DPP wave_shl:1), as the 2-opt strip does with its one
// distance.  On coordinates "from" is "to" bit for bit ((-dx)*(-dx) = dx*dx), so a lane
// pays one sqrt per candidate (two sqrt, two candidates; L = 1: one and one); on a matrix
// the four gathers are what two candidates need anyway.  The rows are laid end to end in a
// strip of width n+1: column n is a closing element that only feeds column n-1 (through
// the sentinels), so strip position x maps to (i, k) with one division by n+1 per lane
// (StripCursor), and the wave walks it in windows of 64 that overlap by one: lanes 0..62
// own the candidates of a position, lane 63 only feeds lane 62.  A lane meets its
// candidates in the enumeration order (L, i, k, rev), so a strict `<` keeps its first
// minimum; one wave reduction (equal changes to the lower key) gives the sweep's move.
//
// Applying (L, i, k, rev) rotates the positions between the segment and the insertion
// point by L, in chunks of 64 that never read a position an earlier chunk wrote; tour, P
// and E rotate together (a shifted edge keeps its term), then the L + 2 terms whose edge
// changed -- the two joins, the closed gap and the segment's interior -- are recomputed.
#include "co_local_search.hpp"

using namespace co;

namespace {

// bytes of tour + E, and with or_opt of A too, then rounded so that P (float2) and the
// staged matrix start 16-aligned
__host__ __device__ constexpr int ls_state_bytes(int n, bool or_opt) {
  return or_opt ? (12 * (n + 1) + 15) & ~15 : 8 * (n + 1);
}

static_assert(4 * CO_TWO_OPT_STAGE_N * CO_TWO_OPT_STAGE_N +
                      ls_state_bytes(CO_TWO_OPT_STAGE_N, true) <= 64 * 1024,
              "a staged matrix with the tour, edge terms and joining edges (the larger of the "
              "two states) must fit 64 KiB of LDS");
static_assert(CO_TWO_OPT_MAX_N < (1 << 15), "2-opt move keys pack j <= n into 16 bits");
static_assert(CO_TWO_OPT_MAX_N <= 1024, "Or-opt keys pack i and k into 10 bits each");

// key of an Or-opt candidate: ascending in the enumeration order L, i, k, rev
__device__ __forceinline__ int or_key(int L, int i, int k, int rev) {
  return (((L << 10 | i) << 10 | k) << 1) | rev;
}

// OR_OPT = false: 2-opt alone -- `ops` is not read and there is no A.
template <int MODE, bool OR_OPT>
__global__ __launch_bounds__(64) void tsp_ls_kernel(
    int64_t B, int n, const float* __restrict__ src, int64_t LB,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, int max_it, int ops,
    int64_t* __restrict__ out, int32_t* __restrict__ sweeps, int32_t* __restrict__ moves,
    int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  unsigned char* s_src = s_raw + ls_state_bytes(n, OR_OPT);  // the staged distance source
  int* tour = reinterpret_cast<int*>(s_raw);                  // n + 1 (sentinel)
  float* E = reinterpret_cast<float*>(s_raw + 4 * (n + 1));   // n (+ 1 of padding)
  [[maybe_unused]] float* A = reinterpret_cast<float*>(s_raw + 8 * (n + 1));  // OR_OPT: n + 1
  uint32_t* bits = reinterpret_cast<uint32_t*>(E);  // the permutation bitmap, before E is built
  [[maybe_unused]] float2* P = reinterpret_cast<float2*>(s_src);  // kCoords: n + 1
  [[maybe_unused]] float* Dl = reinterpret_cast<float*>(s_src);   // kMatLds: n * n
  const int lane = threadIdx.x;
  const int total2 = (n - 2) * (n + 1) / 2;  // the 2-opt strip, in rows of n + 1
  const StripCursor start(lane, n + 1);      // both strips have rows of n + 1
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* arow = actions + b * sb;
    int64_t* orow = out + b * (int64_t)n;
    // here, not after the row check: the scalar 64-bit remainder is where SGPR use peaks,
    // and after the check it puts the staged-matrix 2-opt instance past the 100 SGPRs that 8
    // waves per SIMD allow
    const int64_t inst = LB == B ? b : b % LB;
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
      if (moves && lane < 2) moves[2 * b + lane] = 0;
      continue;
    }
    __syncthreads();
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
    int it = 0, n_two = 0, n_or = 0;
    while (it < max_it) {
      ++it;
      if (!OR_OPT || (ops & CO_TSP_LS_TWO_OPT)) {
        float best = 0.f;  // the reference's delta = 0 with a strict `<`
        int bkey = 0x7fffffff;
        StripCursor cur = start;
        // every lane runs every window (the lane exchange needs the whole wave); the strip's
        // last element is a closing one, so the last move is at total2 - 2
        for (int x0 = 0; x0 < total2 - 1; x0 += kStep) {
          const TwoOptCandidate m = two_opt_candidate(cur, x0 + lane < total2, lane, n, E, dist);
          const bool take =
              m.mine & ((m.change < best) | ((m.change == best) & (m.key < bkey)));
          best = take ? m.change : best;
          bkey = take ? m.key : bkey;
          cur.advance();
        }
        wave_best_move(best, bkey);
        if ((double)best < -1e-6) {
          const int p = bkey >> 16, r = bkey & 0xffff;  // reverse tour[p..r]
          if constexpr (MODE == kCoords) reverse_segment(lane, p, r, tour, P);
          else reverse_segment(lane, p, r, tour);
          __syncthreads();
          for (int k = p + lane; k <= r + 1; k += 64) {
            const int kk = k == n ? 0 : k;
            E[kk] = dist(kk == 0 ? n - 1 : kk - 1, kk);
          }
          __syncthreads();
          ++n_two;
          continue;
        }
      }
      if (!OR_OPT || !(ops & CO_TSP_LS_OR_OPT)) break;  // min_change = 0: the search ends
      float best = 0.f;
      int bkey = 0x7fffffff;
      for (int L = 1; L <= 3 && n - L - 1 >= 1; ++L) {
        for (int i = 1 + lane; i <= n - L; i += 64) A[i] = dist(i - 1, i + L);
        __syncthreads();
        const int total = (n - L) * (n + 1);  // rows i = 1 .. n-L of columns k = 0 .. n
        StripCursor cur = start;
        // the strip's last element is a closing one, so the last candidate is at total - 2
        for (int x0 = 0; x0 < total - 1; x0 += kStep) {
          const bool live = x0 + lane < total;
          const int i = 1 + (live ? cur.q : 0), k = live ? cur.c : 0, e = i + L - 1;
          // position k against the segment's ends: as row (to) and as column (from)
          const float to1 = dist(k, i), to2 = L > 1 ? dist(k, e) : to1;
          float from1 = to1, from2 = to2;
          if constexpr (MODE != kCoords) {
            from1 = dist(i, k);
            from2 = L > 1 ? dist(e, k) : from1;
          }
          const float nx1 = __uint_as_float(dpp_u<0x130>(__float_as_uint(from1)));
          const float nx2 = __uint_as_float(dpp_u<0x130>(__float_as_uint(from2)));
          const float a = A[i], ei = E[i], el = E[e + 1 == n ? 0 : e + 1];
          const float ek = E[k + 1 >= n ? 0 : k + 1];
          const bool mine = live & (lane < kStep) & (k < n) & ((k < i - 1) | (k > e));
          const float c0 = ((((a + to1) + nx2) - ei) - el) - ek;
          bool take = mine & (c0 < best);
          best = take ? c0 : best;
          bkey = take ? or_key(L, i, k, 0) : bkey;
          if (L > 1) {  // the segment reversed: c joins s2, s1 joins d
            const float c1 = ((((a + to2) + nx1) - ei) - el) - ek;
            take = mine & (c1 < best);
            best = take ? c1 : best;
            bkey = take ? or_key(L, i, k, 1) : bkey;
          }
          cur.advance();
        }
        __syncthreads();  // A is rewritten for the next L
      }
      wave_best_move(best, bkey);
      if (!((double)best < -1e-6)) break;  // neither neighbourhood improves: the search ends
      const int rev = bkey & 1, k = (bkey >> 1) & 1023, i = (bkey >> 11) & 1023, L = bkey >> 21;
      // the segment, in its new order, in lanes 0 .. L-1
      const int from = rev ? i + L - 1 - lane : i + lane;
      int seg_t = 0;
      [[maybe_unused]] float2 seg_p = make_float2(0.f, 0.f);
      if (lane < L) {
        seg_t = tour[from];
        if constexpr (MODE == kCoords) seg_p = P[from];
      }
      __syncthreads();
      // forward (k > i+L-1): positions i+L .. k move down by L; backward (k < i-1):
      // positions k+1 .. i-1 move up by L.  Each chunk reads before it writes, and reads
      // nothing an earlier chunk wrote.
      const bool fwd = k > i;
      const int cnt = fwd ? k - (i + L) + 1 : i - 1 - k;
      for (int base = 0; base < cnt; base += 64) {
        const bool ok = base + lane < cnt;
        const int dst = fwd ? i + base + lane : i + L - 1 - base - lane;
        const int sp = ok ? (fwd ? dst + L : dst - L) : 0;
        const int mt = tour[sp];
        const float me = E[sp];
        [[maybe_unused]] float2 mp = make_float2(0.f, 0.f);
        if constexpr (MODE == kCoords) mp = P[sp];
        __syncthreads();
        if (ok) {
          tour[dst] = mt;
          E[dst] = me;
          if constexpr (MODE == kCoords) P[dst] = mp;
        }
        __syncthreads();
      }
      const int q0 = fwd ? k - L + 1 : k + 1;  // where the segment lands
      if (lane < L) {
        tour[q0 + lane] = seg_t;
        if constexpr (MODE == kCoords) P[q0 + lane] = seg_p;
      }
      __syncthreads();
      // the terms whose edge changed: into the segment and inside it (q0 .. q0+L-1), out of
      // it (q0 + L), and the closed gap (forward: i; backward: i + L)
      if (lane < L + 2) {
        int kk = lane <= L ? q0 + lane : (fwd ? i : i + L);
        kk = kk >= n ? kk - n : kk;
        E[kk] = dist(kk == 0 ? n - 1 : kk - 1, kk);
      }
      __syncthreads();
      ++n_or;
    }
    for (int k = lane; k < n; k += 64) orow[k] = tour[k];
    if (sweeps && lane == 0) sweeps[b] = it;
    if (moves && lane < 2) moves[2 * b + lane] = lane ? n_or : n_two;
  }
}

// The checks and the launch of both entry points; `operators` is a valid mask (with
// OR_OPT = false it is CO_TSP_LS_TWO_OPT and the kernel does not read it).
template <bool OR_OPT>
int launch_tsp_ls(int64_t B, int64_t N, const float* locs, const float* distances,
                  int64_t locs_batch, const int64_t* actions, int64_t sb, int64_t st,
                  int64_t max_iterations, int operators, int64_t* actions_out,
                  int32_t* sweeps_out, int32_t* moves_out, int32_t* status, void* stream) {
  if (N <= 0 || N > CO_TWO_OPT_MAX_N) return CO_E_INVAL;
  const int rc = check_search_args(
      B, locs_batch, locs, distances,
      actions && actions_out && actions_out != actions && status, true);
  if (rc != CO_OK || B == 0) return rc;
  const int n = (int)N, max_it = clamp_iterations(max_iterations);
  const dim3 grid = row_grid(B);
  hipStream_t s = (hipStream_t)stream;
  const int state = ls_state_bytes(n, OR_OPT);
#define CO_TSP_LS(MODE, SRC, LDS)                                                               \
  hipLaunchKernelGGL((tsp_ls_kernel<MODE, OR_OPT>), grid, dim3(64), (size_t)(LDS), s, B, n,     \
                     SRC, locs_batch, actions, sb, st, max_it, operators, actions_out,          \
                     sweeps_out, moves_out, status)
  if (locs) CO_TSP_LS(kCoords, locs, state + 8 * (n + 1));
  else if (n <= CO_TWO_OPT_STAGE_N) CO_TSP_LS(kMatLds, distances, state + 4 * n * n);
  else CO_TSP_LS(kMatGlobal, distances, state);
#undef CO_TSP_LS
  return launch_status();
}

}  // namespace

extern "C" int co_tsp_two_opt(int64_t B, int64_t N, const float* locs, const float* distances,
                              int64_t locs_batch, const int64_t* actions, int64_t sb, int64_t st,
                              int64_t max_iterations, int64_t* actions_out, int32_t* sweeps_out,
                              int32_t* status, void* stream) {
  return launch_tsp_ls<false>(B, N, locs, distances, locs_batch, actions, sb, st, max_iterations,
                              CO_TSP_LS_TWO_OPT, actions_out, sweeps_out, nullptr, status, stream);
}

extern "C" int co_tsp_local_search(int64_t B, int64_t N, const float* locs,
                                   const float* distances, int64_t locs_batch,
                                   const int64_t* actions, int64_t sb, int64_t st,
                                   int64_t max_iterations, int operators, int64_t* actions_out,
                                   int32_t* sweeps_out, int32_t* moves_out, int32_t* status,
                                   void* stream) {
  if (operators <= 0 || (operators & ~(CO_TSP_LS_TWO_OPT | CO_TSP_LS_OR_OPT))) return CO_E_INVAL;
  const auto launch = operators == CO_TSP_LS_TWO_OPT ? launch_tsp_ls<false> : launch_tsp_ls<true>;
  return launch(B, N, locs, distances, locs_batch, actions, sb, st, max_iterations, operators,
                actions_out, sweeps_out, moves_out, status, stream);
}
