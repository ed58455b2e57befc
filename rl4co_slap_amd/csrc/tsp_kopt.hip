// The k-opt improvement MDP of TSP (TSPkoptEnv, tsp/env.py:204-549, on ImprovementEnvBase,
// envs/common/base.py:336-403) for gfx950: co_tsp_linked_list, co_tsp_real_solution,
// co_tsp_kopt_reset, co_tsp_kopt_step, co_tsp_kopt_steps and the nearest-neighbour initial
// solution co_tsp_nearest_rec (tsp/generator.py:82-94).
//
// Layout: one wavefront (a 64-thread workgroup) owns one row, rows are taken grid-stride.
// The row's state lives in LDS for the whole launch, 36 bytes per node:
//   rec[n]   the linked list (rec[i] = j: edge i -> j), int32
//   pos[n]   the node's place in the walk from node 0 (pos[0] = 0, pos[rec[0]] = 1;
//            visited_time = pos, with n for node 0)
//   ord[n]   the inverse of pos: the visiting order [0, rec[0], rec[rec[0]], ...]
//   tmp[n]   2-opt: the cyclic sequence with the path reversed; k-opt: pred, the inverse of rec
//   best[n]  co_tsp_kopt_steps: the best-so-far list, stored once after the last step
//   pj[2][n] the pointer-jumping pairs (next << 16 | distance), double buffered
//   P[n]     the coordinates, float2
// Positions come from rec by pointer jumping: node 0 is the list's end, every other node
// starts with (rec[v], 1) and ceil(log2 n) rounds of (next, d) <- (next[next], d + d[next])
// leave d = the steps to node 0, so pos = n - d.  A rec that is one n-cycle brings every
// node to 0 and gives n distinct positions; anything else does not (CO_ST_INVALID_TOUR).
//
// 2-opt (k_max == 2) never walks: with pf = pos[first], L = the nodes of the path first ->
// second and s = 2 pf + L - 1 the new cyclic sequence is S'[q] = ord[(s - q) mod n] inside
// the path's positions and ord[q] outside, node 0 sits at z = s mod n when the path holds
// position 0 (else 0), and rec'[S'[q]] = S'[q + 1], pos'[S'[q]] = (q - z) mod n -- two
// passes of n / 64 iterations.  L == n (second == pred(first)) is the whole-tour reversal.
// k-opt (k_max >= 3) is the reference's walk, by lane 0 over rec / pred in LDS, followed by
// the pointer jumping (which is also the test that the result is one n-cycle).
//
// The cost of a row is a function of (coordinates, rec) alone: every lane adds its nodes'
// edges D(i, rec[i]) (i = lane, lane + 64, ...) in f64, one xor butterfly, one rounding to
// f32 -- co_tsp_reward's summation -- so an unchanged rec costs the same bits in every
// entry point, and co_tsp_kopt_steps (state kept in LDS between the steps; per step it
// reads the action and writes the reward) equals the single-step launches bit for bit.
#include "co_local_search.hpp"

using namespace co;

namespace {

static_assert(CO_KOPT_MAX_N <= 1024 && 36 * CO_KOPT_MAX_N + 64 <= 64 * 1024,
              "a row's state must fit 64 KiB of LDS and 16-bit pointer-jumping halves");

struct KoptArgs {
  int64_t B;
  int n, K;       // K = k_max; 0: no operator (reset / step_to_solution)
  int64_t T;      // steps; 0 with bsf_out == NULL: the reset form
  const float* locs;
  int64_t LB;
  const int64_t* rec_in;
  int64_t* rec_out;               // nullable
  const int64_t* actions;         // nullable: the given rec is next_rec
  int64_t st, sb, sa;             // action element (t, b, a)
  float* cost_cur;                // [B]
  const float* bsf_in;            // nullable with bsf_out
  float* bsf_out;
  float* reward;                  // [T, B]
  float* cost_steps;              // nullable [T, B]
  int64_t* rec_best;              // rows with an improvement are overwritten
  int64_t* vt;                    // nullable [B, n]
  const int64_t* i_in;            // nullable with i_out
  int64_t* i_out;
  int64_t* order_out;             // nullable: co_tsp_real_solution
  int32_t* status;
};

struct KoptLds {
  int *rec, *pos, *ord, *tmp, *best;
  uint32_t* pj[2];
  float2* P;
  int* rn;  // the k-opt move's right nodes
  __device__ KoptLds(unsigned char* raw, int n) {
    P = reinterpret_cast<float2*>(raw);
    int* w = reinterpret_cast<int*>(raw + 8 * n);
    rec = w, pos = w + n, ord = w + 2 * n, tmp = w + 3 * n, best = w + 4 * n;
    pj[0] = reinterpret_cast<uint32_t*>(w + 5 * n);
    pj[1] = reinterpret_cast<uint32_t*>(w + 6 * n);
    rn = w + 7 * n;
  }
};

// pos / ord from rec (entries in 0..n-1) by pointer jumping; false when rec is not one
// n-cycle (pos / ord are then not to be used)
__device__ bool kopt_rank(const KoptLds& s, int n, int lane) {
  for (int v = lane; v < n; v += 64) s.pj[0][v] = v == 0 ? 0u : ((uint32_t)s.rec[v] << 16) | 1u;
  __syncthreads();
  int cur = 0;
  for (int span = 1; span < n; span <<= 1) {
    const uint32_t* a = s.pj[cur];
    uint32_t* o = s.pj[cur ^ 1];
    for (int v = lane; v < n; v += 64) {
      const uint32_t x = a[v], y = a[x >> 16];
      o[v] = (y & 0xffff0000u) | ((x & 0xffffu) + (y & 0xffffu));
    }
    __syncthreads();
    cur ^= 1;
  }
  const uint32_t* a = s.pj[cur];
  bool bad = false;
  for (int v = lane; v < n; v += 64) bad |= (a[v] >> 16) != 0;
  if (__any(bad)) return false;
  // every node reaches 0 on a simple path: 1 <= d <= n-1 for v != 0
  for (int v = lane; v < n; v += 64) {
    const int p = v == 0 ? 0 : n - (int)(a[v] & 0xffffu);
    s.pos[v] = p;
    s.ord[p] = v;
  }
  __syncthreads();
  for (int v = lane; v < n; v += 64) bad |= s.ord[s.pos[v]] != v;  // two nodes, one place
  // the others form one path into 0; node 0 must lead to its far end
  return !__any(bad) && (n == 1 || s.rec[0] == s.ord[1]);
}

__device__ float kopt_cost(const KoptLds& s, int n, int lane) {
  double acc = 0.0;
  for (int v = lane; v < n; v += 64) {
    const float2 p = s.P[v], q = s.P[s.rec[v]];
    acc += (double)edge_len(p.x, p.y, q.x, q.y);
  }
  return (float)wave_sum(acc);
}

// the DACT 2-opt move (tsp/env.py:334-359) on a valid state; first != second
__device__ void kopt_two_opt(const KoptLds& s, int n, int lane, int first, int second) {
  const int pf = s.pos[first], ps = s.pos[second];
  const int L = (ps - pf + n) % n + 1, sum = 2 * pf + L - 1;
  const int z = (n - pf) % n < L ? sum % n : 0;  // where node 0 goes
  for (int q = lane; q < n; q += 64) {
    const bool in = (q - pf + n) % n < L;
    s.tmp[q] = s.ord[in ? (sum - q + n) % n : q];
  }
  __syncthreads();
  for (int q = lane; q < n; q += 64) {
    const int v = s.tmp[q], p = (q - z + n) % n;
    s.rec[v] = s.tmp[q + 1 == n ? 0 : q + 1];
    s.pos[v] = p;
    s.ord[p] = v;
  }
  __syncthreads();
}

// the NeuOpt k-opt move (tsp/env.py:361-390): the reference's walk; act = index | left |
// right, every entry in range.  false when the result is not one n-cycle.
__device__ bool kopt_walk(const KoptLds& s, int n, int K, int lane, const int64_t* act,
                          int64_t sa) {
  for (int v = lane; v < n; v += 64) s.tmp[s.rec[v]] = v;  // pred of the old rec
  if (lane < K) s.rn[lane] = s.rec[(int)act[lane * sa]];
  __syncthreads();
  if (lane == 0) {
    for (int j = 0; j < K; ++j) s.rec[(int)act[(K + j) * sa]] = (int)act[(2 * K + j) * sa];
    int cur = (int)act[K * sa];
    for (int it = 0; it < n - 2; ++it) {
      const int next = s.rec[cur], po = s.tmp[next];
      bool right = false;
      for (int j = 0; j < K; ++j) right |= s.rn[j] == next;
      if (po != cur && !right) s.rec[next] = po;
      cur = next;
    }
  }
  __syncthreads();
  return kopt_rank(s, n, lane);
}

__global__ __launch_bounds__(64) void kopt_kernel(KoptArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int n = a.n, K = a.K, lane = threadIdx.x;
  const KoptLds s(s_raw, n);
  const int A = K == 2 ? 2 : 3 * K;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();  // the previous row's LDS reads are done
    const int64_t* rrow = a.rec_in + b * (int64_t)n;
    bool bad = false;
    for (int v = lane; v < n; v += 64) {
      const int64_t r = rrow[v];
      if (r < 0 || r >= n) bad = true;
      s.rec[v] = (r < 0 || r >= n) ? 0 : (int)r;
    }
    if (a.locs) {
      const float2* lrow =
          reinterpret_cast<const float2*>(a.locs) + (a.LB == a.B ? b : b % a.LB) * (int64_t)n;
      for (int v = lane; v < n; v += 64) s.P[v] = lrow[v];
    }
    __syncthreads();
    if (__any(bad) || !kopt_rank(s, n, lane)) {
      if (lane == 0) set_status(a.status, CO_ST_INVALID_TOUR);
      continue;
    }
    if (a.order_out) {  // co_tsp_real_solution
      for (int v = lane; v < n; v += 64) a.order_out[b * (int64_t)n + v] = s.ord[v];
      continue;
    }
    float cost = kopt_cost(s, n, lane);
    float bsf = a.bsf_in ? a.bsf_in[b] : 0.f;
    bool dirty = false, stop = false;
    for (int64_t t = 0; t < a.T && !stop; ++t) {
      if (a.actions) {
        const int64_t* act = a.actions + t * a.st + b * a.sb;
        bool oob = false;
        if (lane < A) {
          const int64_t x = act[lane * a.sa];
          oob = x < 0 || x >= n;
        }
        if (__any(oob)) {
          if (lane == 0) set_status(a.status, CO_ST_INDEX_RANGE);
          stop = true;
          break;
        }
        if (K == 2) {
          const int first = (int)act[0], second = (int)act[a.sa];
          if (first != second) kopt_two_opt(s, n, lane, first, second);
        } else if (!kopt_walk(s, n, K, lane, act, a.sa)) {
          if (lane == 0) set_status(a.status, CO_ST_INVALID_TOUR);
          stop = true;
          break;
        }
        cost = kopt_cost(s, n, lane);
      }
      const float now = cost < bsf ? cost : bsf;
      const float rew = bsf - now;
      bsf = now;
      if (rew > 0.0f) {
        for (int v = lane; v < n; v += 64) s.best[v] = s.rec[v];
        dirty = true;
      }
      if (lane == 0) {
        a.reward[t * a.B + b] = rew;
        if (a.cost_steps) a.cost_steps[t * a.B + b] = cost;
      }
    }
    if (stop) continue;  // the row's outputs are unspecified
    if (a.rec_out)
      for (int v = lane; v < n; v += 64) a.rec_out[b * (int64_t)n + v] = s.rec[v];
    if (a.vt)
      for (int v = lane; v < n; v += 64) a.vt[b * (int64_t)n + v] = v == 0 ? n : s.pos[v];
    if (dirty) {
      __syncthreads();
      for (int v = lane; v < n; v += 64) a.rec_best[b * (int64_t)n + v] = s.best[v];
    }
    if (lane == 0) {
      a.cost_cur[b] = cost;
      if (a.bsf_out) a.bsf_out[b] = bsf;
      if (a.i_out) a.i_out[b] = a.i_in[b] + a.T;
    }
  }
}

// rec[t[k]] = t[(k+1) % n] of a tour row (ImprovementEnvBase._get_linked_list_solution)
__global__ __launch_bounds__(64) void linked_list_kernel(int64_t B, int n,
                                                         const int64_t* __restrict__ tour,
                                                         int64_t sb, int64_t st,
                                                         int64_t* __restrict__ rec,
                                                         int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint32_t* bits = reinterpret_cast<uint32_t*>(s_raw);
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* trow = tour + b * sb;
    __syncthreads();
    for (int k = lane; k < ((n + 31) >> 5); k += 64) bits[k] = 0;
    __syncthreads();
    bool bad = false;
    for (int k = lane; k < n; k += 64) {
      const int64_t x = trow[(int64_t)k * st];
      if (x < 0 || x >= n) bad = true;
      else if (mark_once(bits, x)) bad = true;
    }
    if (__any(bad)) {
      if (lane == 0) set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    for (int k = lane; k < n; k += 64)
      rec[b * (int64_t)n + trow[(int64_t)k * st]] = trow[(int64_t)(k + 1 == n ? 0 : k + 1) * st];
  }
}

// the nearest-neighbour tour from node 0 as a linked list (tsp/generator.py:82-94): a
// visited node's distance counts as 1e5, the first minimum wins
__global__ __launch_bounds__(64) void nearest_rec_kernel(int64_t B, int n,
                                                         const float* __restrict__ locs,
                                                         int64_t* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float2* P = reinterpret_cast<float2*>(s_raw);
  int* nxt = reinterpret_cast<int*>(s_raw + 8 * n);
  int* seen = nxt + n;
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const float2* lrow = reinterpret_cast<const float2*>(locs) + b * (int64_t)n;
    __syncthreads();
    for (int v = lane; v < n; v += 64) {
      P[v] = lrow[v];
      nxt[v] = 0;
      seen[v] = v == 0;
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < n - 1; ++it) {
      const float2 c = P[cur];
      float best = __builtin_inff();
      int bi = 0x7fffffff;
      for (int v = lane; v < n; v += 64) {
        const float d = seen[v] ? 1e5f : edge_len(c.x, c.y, P[v].x, P[v].y);
        if (d < best) best = d, bi = v;
      }
      wave_argmin(best, bi);
      bi = __builtin_amdgcn_readfirstlane(bi);
      if (bi < 0 || bi >= n) break;  // every distance a NaN: the list stays short of a cycle
      if (lane == 0) {
        nxt[cur] = bi;
        seen[bi] = 1;
      }
      __syncthreads();
      cur = bi;
    }
    for (int v = lane; v < n; v += 64) rec[b * (int64_t)n + v] = nxt[v];
  }
}

int kopt_launch(const KoptArgs& a, void* stream) {
  const size_t lds = 36 * (size_t)a.n + 64;
  hipLaunchKernelGGL(kopt_kernel, row_grid(a.B), dim3(64), lds, (hipStream_t)stream, a);
  return launch_status();
}

inline bool kopt_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N > 0 && N <= CO_KOPT_MAX_N; }

}  // namespace

extern "C" int co_tsp_linked_list(int64_t B, int64_t N, const int64_t* tour, int64_t sb,
                                  int64_t st, int64_t* rec, int32_t* status, void* stream) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!tour || !rec || rec == tour || !status) return CO_E_INVAL;
  hipLaunchKernelGGL(linked_list_kernel, row_grid(B), dim3(64), 4 * (((size_t)N + 31) >> 5),
                     (hipStream_t)stream, B, (int)N, tour, sb, st, rec, status);
  return launch_status();
}

extern "C" int co_tsp_real_solution(int64_t B, int64_t N, const int64_t* rec, int64_t* solution,
                                    int32_t* status, void* stream) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!rec || !solution || !status) return CO_E_INVAL;
  KoptArgs a{};
  a.B = B, a.n = (int)N, a.rec_in = rec, a.order_out = solution, a.status = status;
  return kopt_launch(a, stream);
}

extern "C" int co_tsp_kopt_reset(int64_t B, int64_t N, const float* locs, int64_t locs_batch,
                                 const int64_t* rec, float* cost, int64_t* visited_time,
                                 int32_t* status, void* stream) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (locs_batch <= 0 || B % locs_batch != 0) return CO_E_INVAL;
  if (!locs || !rec || !cost || !status) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  KoptArgs a{};
  a.B = B, a.n = (int)N, a.locs = locs, a.LB = locs_batch, a.rec_in = rec, a.cost_cur = cost;
  a.vt = visited_time, a.status = status;
  return kopt_launch(a, stream);
}

extern "C" int co_tsp_kopt_steps(int64_t B, int64_t N, int64_t k_max, int64_t steps,
                                 const float* locs, int64_t locs_batch, const int64_t* actions,
                                 int64_t act_stride_t, int64_t act_stride_b,
                                 int64_t act_stride_a, int64_t* rec_current,
                                 float* cost_current, float* cost_bsf, int64_t* rec_best,
                                 int64_t* visited_time, int64_t* i, float* reward,
                                 float* cost_steps, int32_t* status, void* stream) {
  if (!kopt_sizes_ok(B, N) || k_max < 2 || k_max > CO_KOPT_MAX_K || steps < 0)
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (locs_batch <= 0 || B % locs_batch != 0) return CO_E_INVAL;
  if (!locs || !rec_current || !cost_current || !cost_bsf || !rec_best ||
      rec_best == rec_current || !visited_time || !status || (steps > 0 && (!actions || !reward)))
    return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  KoptArgs a{};
  a.B = B, a.n = (int)N, a.K = (int)k_max, a.T = steps, a.locs = locs, a.LB = locs_batch;
  a.rec_in = rec_current, a.rec_out = rec_current, a.actions = actions;
  a.st = act_stride_t, a.sb = act_stride_b, a.sa = act_stride_a;
  a.cost_cur = cost_current, a.bsf_in = cost_bsf, a.bsf_out = cost_bsf, a.reward = reward;
  a.cost_steps = cost_steps, a.rec_best = rec_best, a.vt = visited_time, a.i_in = i, a.i_out = i;
  a.status = status;
  return kopt_launch(a, stream);
}

extern "C" int co_tsp_kopt_step(int64_t B, int64_t N, int64_t k_max, const float* locs,
                                int64_t locs_batch, const int64_t* rec_in, const int64_t* action,
                                int64_t act_stride_b, int64_t act_stride_a, int64_t* rec_out,
                                float* cost_current, const float* cost_bsf_in,
                                float* cost_bsf_out, float* reward, int64_t* rec_best,
                                int64_t* visited_time, const int64_t* i_in, int64_t* i_out,
                                int32_t* status, void* stream) {
  if (!kopt_sizes_ok(B, N) || (action && (k_max < 2 || k_max > CO_KOPT_MAX_K)))
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (locs_batch <= 0 || B % locs_batch != 0) return CO_E_INVAL;
  if (!locs || !rec_in || !rec_out || !cost_current || !cost_bsf_in || !cost_bsf_out ||
      !reward || !rec_best || rec_best == rec_out || rec_best == rec_in || !visited_time ||
      !status || (action && (!i_in || !i_out)))
    return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  KoptArgs a{};
  a.B = B, a.n = (int)N, a.K = action ? (int)k_max : 0, a.T = 1, a.locs = locs;
  a.LB = locs_batch, a.rec_in = rec_in, a.rec_out = rec_out, a.actions = action;
  a.sb = act_stride_b, a.sa = act_stride_a, a.cost_cur = cost_current, a.bsf_in = cost_bsf_in;
  a.bsf_out = cost_bsf_out, a.reward = reward, a.rec_best = rec_best, a.vt = visited_time;
  if (action) a.i_in = i_in, a.i_out = i_out;
  a.status = status;
  return kopt_launch(a, stream);
}

extern "C" int co_tsp_nearest_rec(int64_t B, int64_t N, const float* locs, int64_t* rec,
                                  void* stream) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !rec) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  hipLaunchKernelGGL(nearest_rec_kernel, row_grid(B), dim3(64), 16 * (size_t)N,
                     (hipStream_t)stream, B, (int)N, locs, rec);
  return launch_status();
}
