// Segmented best-of-K selection for gfx950 (co_best_of, co_tsp_best_of): the step that
// follows a K-candidate rollout (augmentations x starts x samples) in policy evaluation.
// Candidate k of instance b is row e = k*B + b (batchify's repeat-major layout).
//
// co_tsp_best_of: one workgroup per instance.  The instance's coordinates are staged in
// LDS once (8N bytes) and shared by all K candidates.  A group of G lanes owns a candidate
// row: the lanes load the row's entries (t = sl + G*i: G consecutive int64 per load
// instruction for contiguous rows), store them as u16 in the group's LDS row so that every
// lane can read its successor's node, gather both endpoints from the LDS coordinates, sum
// tsp.hip's edge_len in f64 and reduce over the group.  Each group keeps the best (reward,
// k) of the candidates it has seen, the groups of a wave and the waves of the block are
// reduced with torch.max's order, and the block copies the winning row.  The block has as
// many groups as there are candidates (up to 1024 threads), so a large K on few instances
// still has 16 waves loading rows; K is not split over workgroups (no workspace, no second
// pass, no atomics on the outputs).
//
// co_best_of: a block takes 64 consecutive instances; lane = instance, the four waves
// take k = w, w + 4, ... (each load instruction reads 64 consecutive rewards of one k), the
// waves' results meet in LDS, then wave w copies the winning rows of instances w, w + 4, ...
#include "co_common.hpp"

using namespace co;

namespace {

constexpr int kNoCandidate = 0x7fffffff;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dynamic LDS of tsp_best_of_kernel: the coordinates, per group a u16 row with a slot for
// every (lane, entry) of the group (pitch = G * EPL >= N) and a visited bitmap
inline size_t bo_lds_bytes(int N, int groups, int pitch) {
  return (size_t)8 * N + (size_t)groups * pitch * 2 + (size_t)groups * ((N + 31) / 32) * 4;
}

template <int G, int EPL, bool CONTIG>
__global__ __launch_bounds__(1024) void tsp_best_of_kernel(
    int64_t B, int N, int K, const float2* __restrict__ locs, const int64_t* __restrict__ actions,
    int64_t sb, int64_t st, int check, float* __restrict__ all_reward,
    float* __restrict__ best_reward, int64_t* __restrict__ best_idx,
    int64_t* __restrict__ best_actions, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bo_smem[];
  __shared__ float s_v[16];
  __shared__ int s_k[16];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_in_block();
  const int groups = blockDim.x / G, grp = tid / G, sl = lane % G;
  constexpr int pitch = G * EPL;
  const int words = (N + 31) >> 5;
  float2* C = reinterpret_cast<float2*>(bo_smem);
  uint16_t* row = reinterpret_cast<uint16_t*>(bo_smem + (size_t)8 * N) + (size_t)grp * pitch;
  uint32_t* bits = reinterpret_cast<uint32_t*>(bo_smem + (size_t)8 * N + (size_t)groups * pitch * 2) +
                   (size_t)grp * words;
  const int64_t b = blockIdx.x;
  const float2* lrow = locs + b * (int64_t)N;
  for (int t = tid; t < N; t += blockDim.x) C[t] = lrow[t];
  __syncthreads();

  // (-inf, the group's first k): nothing later is "larger" than an all -inf column's first;
  // a group without a candidate keeps (-inf, kNoCandidate), which loses to every real one
  float bv = -__builtin_inff();
  int bk = grp < K ? grp : kNoCandidate;
  bool bad = false, range = false;
  const int rounds = (K + groups - 1) / groups;  // block-uniform: every lane stays active
  for (int r = 0; r < rounds; ++r) {
    const int k = r * groups + grp;
    const bool valid = k < K;
    const int64_t e = (int64_t)(valid ? k : 0) * B + b;
    const int64_t* arow = actions + e * sb;
    // (branch-free per entry: a lane past the row's end or of a group without a candidate
    // reads entry 0 of candidate 0 and keeps its results out with selects)
    int a[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const int t = sl + G * i;
      const bool live = valid && t < N;
      const int tt = live ? t : 0;
      const int64_t v = CONTIG ? arow[tt] : arow[(int64_t)tt * st];
      const bool oor = v < 0 || v >= N;
      a[i] = oor ? -1 : (int)v;
      range |= live && oor;
      row[t] = oor ? (uint16_t)0xffff : (uint16_t)v;  // t < G * EPL: a slot of its own
    }
    if (check)
      for (int q = sl; q < words; q += G) bits[q] = 0;
    wave_lds_sync();
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const int t = sl + G * i;
      const bool in_row = t < N, ok = in_row && a[i] >= 0;
      if (check) {  // block-uniform
        const uint32_t bit = ok ? 1u << (a[i] & 31) : 0u;
        const uint32_t old = atomicOr(&bits[ok ? a[i] >> 5 : 0], bit);
        bad |= valid && in_row && (!ok || (old & bit) != 0);
      }
      const uint16_t nx = row[(t + 1 >= N) ? 0 : t + 1];  // the closing edge wraps
      const bool use = ok && nx != 0xffff;
      const float2 p = C[ok ? a[i] : 0], q = C[use ? nx : 0];
      const float len = edge_len(p.x, p.y, q.x, q.y);
      acc += use ? (double)len : 0.0;
    }
    acc = grp_sum_f64<G>(acc);
    const float rew = -(float)acc;
    if (valid && all_reward && sl == 0) all_reward[e] = rew;
    // the group's k only grows: a later candidate wins when it is larger, or the first NaN
    const bool take = valid && (rew > bv || (rew != rew && bv == bv));
    bv = take ? rew : bv;
    bk = take ? k : bk;
    wave_lds_sync();  // the next round rewrites the row and the bitmap
  }
  if (__any(bad) && lane == 0) set_status(status, CO_ST_INVALID_TOUR);
  if (__any(range) && lane == 0) set_status(status, CO_ST_INDEX_RANGE);

  wave_argmax(bv, bk);
  if (lane == 0) {
    s_v[w] = bv;
    s_k[w] = bk;
  }
  __syncthreads();
  const int nw = blockDim.x >> 6;
  bv = s_v[0];
  bk = s_k[0];
  for (int q = 1; q < nw; ++q)
    if (argmax_better(s_v[q], s_k[q], bv, bk)) {
      bv = s_v[q];
      bk = s_k[q];
    }
  if (tid == 0) {
    best_reward[b] = bv;
    best_idx[b] = bk;
  }
  if (best_actions) {
    const int64_t* src = actions + ((int64_t)bk * B + b) * sb;
    int64_t* dst = best_actions + b * (int64_t)N;
    for (int t = tid; t < N; t += blockDim.x) dst[t] = CONTIG ? src[t] : src[(int64_t)t * st];
  }
}

__global__ __launch_bounds__(256) void best_of_kernel(int64_t B, int K, int64_t T,
                                                      const float* __restrict__ reward,
                                                      const int64_t* __restrict__ actions,
                                                      int64_t sb, int64_t st,
                                                      float* __restrict__ best_reward,
                                                      int64_t* __restrict__ best_idx,
                                                      int64_t* __restrict__ best_actions) {
  __shared__ float s_v[4][64];
  __shared__ int s_k[4][64];
  const int w = wave_in_block(), lane = lane_id();
  const int64_t b0 = (int64_t)blockIdx.x * 64, b = b0 + lane;
  const bool valid = b < B;
  float bv = -__builtin_inff();
  int bk = kNoCandidate;
  if (valid) {
#pragma unroll 4
    for (int k = w; k < K; k += 4) {
      const float v = reward[(int64_t)k * B + b];
      if (argmax_better(v, k, bv, bk)) {
        bv = v;
        bk = k;
      }
    }
  }
  s_v[w][lane] = bv;
  s_k[w][lane] = bk;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (argmax_better(s_v[q][lane], s_k[q][lane], bv, bk)) {
        bv = s_v[q][lane];
        bk = s_k[q][lane];
      }
    s_k[0][lane] = bk;
    if (valid) {
      best_reward[b] = bv;
      best_idx[b] = bk;
    }
  }
  if (!best_actions) return;  // block-uniform
  __syncthreads();
  for (int r = w; r < 64 && b0 + r < B; r += 4) {
    const int64_t* src = actions + ((int64_t)s_k[0][r] * B + b0 + r) * sb;
    int64_t* dst = best_actions + (b0 + r) * T;
    for (int64_t t = lane; t < T; t += 64) dst[t] = src[t * st];
  }
}

// threads of a co_tsp_best_of block: a group per candidate, whole waves, 64..1024
inline int bo_block_threads(int64_t K, int G) {
  int64_t th = (K * G + 63) / 64 * 64;
  return (int)(th < 64 ? 64 : th > 1024 ? 1024 : th);
}

}  // namespace

extern "C" int co_best_of(int64_t B, int64_t K, int64_t T, const float* reward,
                          const int64_t* actions, int64_t sb, int64_t st, float* best_reward,
                          int64_t* best_idx, int64_t* best_actions, int32_t* status,
                          void* stream) {
  (void)status;  // the selection has no data-dependent failure
  if (B < 0 || K <= 0 || T < 0 || K > 0x7ffffffe) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!reward || !best_reward || !best_idx) return CO_E_INVAL;
  if (T == 0) best_actions = nullptr;
  if (best_actions && (!actions || best_actions == actions)) return CO_E_INVAL;
  const unsigned grid = cover_grid(B, 64);
  if (grid == 0) return CO_E_INVAL;
  hipLaunchKernelGGL(best_of_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, B, (int)K, T,
                     reward, actions, sb, st, best_reward, best_idx, best_actions);
  return launch_status();
}

extern "C" int co_tsp_best_of(int64_t B, int64_t N, int64_t K, const float* locs,
                              const int64_t* actions, int64_t sb, int64_t st, int check,
                              float* all_reward, float* best_reward, int64_t* best_idx,
                              int64_t* best_actions, int32_t* status, void* stream) {
  if (B < 0 || N <= 0 || K <= 0 || N > 1024 || K > 0x7ffffffe || B > 0x7fffffff)
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !best_reward || !best_idx || (check && !status)) return CO_E_INVAL;
  if (best_actions == actions) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  const float2* l2 = reinterpret_cast<const float2*>(locs);
  hipStream_t s = (hipStream_t)stream;
#define CO_BO2(GG, EE, CC)                                                                     \
  do {                                                                                         \
    const int th = bo_block_threads(K, GG);                                                    \
    const size_t lds = bo_lds_bytes((int)N, th / GG, GG * EE);                                         \
    if (lds > 60 * 1024) return CO_E_INVAL; /* cannot happen for N <= 1024 */                  \
    hipLaunchKernelGGL((tsp_best_of_kernel<GG, EE, CC>), dim3((unsigned)B), dim3(th), lds, s,  \
                       B, (int)N, (int)K, l2, actions, sb, st, check, all_reward, best_reward, \
                       best_idx, best_actions, status);                                        \
  } while (0)
#define CO_BO(GG, EE)            \
  do {                           \
    if (st == 1) CO_BO2(GG, EE, true); \
    else CO_BO2(GG, EE, false);  \
  } while (0)
  if (N <= 20) CO_BO(4, 5);  // TSP-20: 5 entries a lane
  else if (N <= 32) CO_BO(4, 8);
  else if (N <= 64) CO_BO(8, 8);
  else if (N <= 112) CO_BO(16, 7);  // TSP-100: 7 entries a lane
  else if (N <= 128) CO_BO(16, 8);
  else if (N <= 256) CO_BO(32, 8);
  else if (N <= 512) CO_BO(64, 8);
  else CO_BO(64, 16);
#undef CO_BO
#undef CO_BO2
  return launch_status();
}
