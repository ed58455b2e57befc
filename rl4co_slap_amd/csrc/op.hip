// The orienteering problem (rl4co/envs/routing/op/env.py) for gfx950: reset, the step, the
// mask alone, T preset steps in one launch, and the reward with check_solution_validity's two
// tests.  include/co_env.h (OP) states the semantics; this file is their device form.
//
// Layout (op_rows_kernel, op_reward_kernel): a group of G lanes owns one row, 64 / G rows per
// wave, G the smallest of 1 / 2 / 4 / ... / 32 with 32 G >= N + 1, workgroups of four waves
// over the batch.  Lane sl holds columns 32 sl .. 32 sl + 31 of the row's visited set as one
// bit word, and every lane of the group holds the row scalars (tour length, prize, current
// node and its coordinates, i, visited[0]).  A preset step is the action (the same address
// on every lane of the group: one broadcast load), locs[a] and prize[a] by address (again
// one address a group), one bit test (a ds_bpermute of the word that holds the action's
// bit) and one bit edit: O(1) per row.  Only after the last step does each lane compute its
// 32 columns of the mask (a distance each) and expand and store the byte rows once.  No LDS,
// no barrier, no scratch.  The file is built with -ffp-contract=off: every f32 operation
// below is rounded on its own, as the header states and the host build computes.
//
// The reward walks the tour in order on every lane of the group (f64 sums in tour order)
// with "seen" as the same bit words; the length test's NC bounds are the lanes' own columns.
#include "co_common.hpp"

using namespace co;

namespace {

typedef uint32_t op_u32_align1 __attribute__((aligned(1)));

struct OpArgs {
  int64_t B;
  int N, T;
  const int64_t* actions;  // T >= 1
  int64_t st, sb;
  // reset: the state is fresh, locs / prize / max_length are made from these and stored
  const float2 *depot, *locs_in;
  const float *prize_in, *ml_in;
  float2* locs_out;
  float *prize_out, *ml_out;
  // otherwise the post-reset tensors
  const float2* locs;
  const float *prize, *ml;
  const uint8_t *mask_in, *vis_in;
  uint8_t *vis_out, *mask_out;
  const float *tl_in, *pz_in;
  float *tl_out, *pz_out;
  const int64_t *cur_in, *i_in;
  int64_t *cur_out, *i_out;
  uint8_t *done, *reward, *feasible;
  float* length;
  int32_t* status;
};

constexpr int kOpWaves = 4;

// columns c0 .. c0 + 31 of a byte row of NC columns as a bit word (a non-zero byte: 1)
__device__ __forceinline__ uint32_t op_load_bits(const uint8_t* row, int c0, int NC) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // every load issued before the first use
    const int c = c0 + 4 * j;
    uint32_t x = 0u;
    if (c + 4 <= NC) {
      x = *reinterpret_cast<const op_u32_align1*>(row + c);
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (c + q < NC) x |= (uint32_t)row[c + q] << (8 * q);
    }
    w[j] = x;
  }
  uint32_t bits = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t x = w[j];
    // bit 7 of every non-zero byte, down to bit 0, then the four byte flags to bits 24..27
    const uint32_t nz = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
    bits |= ((nz * 0x01020408u) >> 24 & 0xfu) << (4 * j);
  }
  return bits;
}

// the reverse: bits -> 0 / 1 bytes of columns c0 .. c0 + 31, the row's live columns only
__device__ __forceinline__ void op_store_bits(uint8_t* row, int c0, int NC, uint32_t bits) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + 4 * j;
    const uint32_t x = (((bits >> (4 * j)) & 0xfu) * 0x00204081u) & 0x01010101u;
    if (c + 4 <= NC) {
      *reinterpret_cast<op_u32_align1*>(row + c) = x;
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (c + q < NC) row[c + q] = (uint8_t)(x >> (8 * q));
    }
  }
}

// the bits of a lane's word that are columns of the row
__device__ __forceinline__ uint32_t op_live(int c0, int NC) {
  const int n = NC - c0;
  return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : (1u << n) - 1u);
}

__device__ __forceinline__ int op_clamp(int64_t a, int N) {
  return a < 0 ? 0 : (a > N ? N : (int)a);
}

template <int G>
__global__ __launch_bounds__(64 * kOpWaves) void op_rows_kernel(const OpArgs p) {
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int N = p.N, NC = N + 1, T = p.T;
  const int64_t b0 = ((int64_t)blockIdx.x * kOpWaves + w) * RW + grp;
  const bool valid = b0 < p.B;  // rows past B re-read row B-1 and store nothing
  const int64_t b = valid ? b0 : p.B - 1;
  const int64_t row = b * NC;
  const bool fresh = p.depot != nullptr;
  const int c0 = 32 * sl;
  const uint32_t live = op_live(c0, NC);

  // ---- the state: the visited bits and, on every lane, the row scalars
  uint32_t vis = 0u;
  float tl = 0.f, pz = 0.f, mlb = 0.f;
  int64_t iv = 0, cur = 0;
  float2 cl;  // locs[clamp(current_node, 0, N)]
  if (fresh) {  // op/env.py:110-151
    cl = p.depot[b];
    mlb = p.ml_in[b];
  } else {
    vis = op_load_bits(p.vis_in + row, c0, NC) & live;
    tl = p.tl_in[b];
    cur = p.cur_in[b];
    if (p.pz_in) pz = p.pz_in[b];
    if (p.i_in) iv = p.i_in[b];
    cl = p.locs[row + op_clamp(cur, N)];
  }
  bool v0 = ((uint32_t)__shfl((int)vis, gbase, 64) & 1u) != 0u;  // visited[0]
  bool dn = false;

  // ---- the preset steps (op/env.py:74-108)
  for (int t = 0; t < T; ++t) {
    const int64_t a = p.actions[t * p.st + b * p.sb];
    const bool bad = a < 0 || a > N;
    const int ac = op_clamp(a, N);
    const float2 la = p.locs[row + ac];
    const float pa = p.prize[row + ac];
    const float leg = edge_len(la.x, la.y, cl.x, cl.y);
    if (p.feasible) {  // action_mask[b, a] of the state before this step
      bool f;
      if (t == 0) {
        f = p.mask_in[row + ac] != 0;
      } else {
        const uint32_t word = (uint32_t)__shfl((int)vis, gbase + (ac >> 5), 64);
        const bool seen = (word >> (ac & 31)) & 1u;
        f = ac == 0 || !(seen || v0 || tl + leg > p.ml[row + ac]);
      }
      if (valid && sl == 0) p.feasible[(int64_t)t * p.B + b] = !bad && f;
    }
    if (valid && bad && sl == 0) set_status(p.status, CO_ST_INDEX_RANGE);
    if (!bad) {
      tl = tl + leg;
      pz = pz + pa;
      if (sl == (ac >> 5)) vis |= 1u << (ac & 31);
      v0 |= ac == 0;
    }
    dn = a == 0 && iv > 0;
    iv += 1;
    cur = a;
    cl = la;
    if (p.length && valid && sl == 0) p.length[(int64_t)t * p.B + b] = tl;
  }

  // ---- the mask of the final state (op/env.py:153-169): this lane's 32 columns
  uint32_t open = 0u;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    const int c = c0 + k;
    if (c < NC) {
      float2 q;
      float ml;
      if (fresh) {
        q = c == 0 ? cl : p.locs_in[b * N + (c - 1)];
        ml = (mlb - edge_len(cl.x, cl.y, q.x, q.y)) - 1e-6f;  // cl is the depot: T == 0
        if (valid) {
          p.locs_out[row + c] = q;
          p.prize_out[row + c] = c == 0 ? 0.f : p.prize_in[b * N + (c - 1)];
          p.ml_out[row + c] = ml;
        }
      } else {
        q = p.locs[row + c];
        ml = p.ml[row + c];
      }
      const bool exceeds = tl + edge_len(q.x, q.y, cl.x, cl.y) > ml;
      if (!exceeds) open |= 1u << k;
    }
  }
  uint32_t mask = v0 ? 0u : (open & ~vis);
  if (sl == 0) mask |= 1u;
  if (!valid) return;
  op_store_bits(p.mask_out + row, c0, NC, mask & live);
  if (p.vis_out) op_store_bits(p.vis_out + row, c0, NC, vis);
  // the row scalars, spread over the group's lanes
  if (sl == 0 && p.tl_out) p.tl_out[b] = tl;
  if (sl == 1 % G && p.pz_out) p.pz_out[b] = pz;
  if (sl == 2 % G && p.cur_out) p.cur_out[b] = cur;
  if (sl == 3 % G && p.i_out) p.i_out[b] = iv;
  if (sl == 4 % G && p.done) p.done[b] = dn;
  if (sl == 5 % G && p.reward) p.reward[b] = 0;
}

int op_groups(int NC) {  // lanes per row: 32 columns each
  int g = 1;
  while (32 * g < NC) g *= 2;
  return g;
}

int op_launch(const OpArgs& a, void* stream) {
  const int G = op_groups(a.N + 1);
  const int64_t rows_per_wg = (int64_t)(64 / G) * kOpWaves;
  const unsigned grid = cover_grid(a.B, (int)rows_per_wg, 64 * kOpWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_OP(GG) \
  hipLaunchKernelGGL((op_rows_kernel<GG>), dim3(grid), dim3(64 * kOpWaves), 0, s, a)
  switch (G) {
    case 1: CO_OP(1); break;
    case 2: CO_OP(2); break;
    case 4: CO_OP(4); break;
    case 8: CO_OP(8); break;
    case 16: CO_OP(16); break;
    default: CO_OP(32);
  }
#undef CO_OP
  return launch_status();
}

// reward + validity: the tour in order on every lane of the row's group
template <int G>
__global__ __launch_bounds__(64 * kOpWaves) void op_reward_kernel(
    int64_t B, int N, int T, const float* __restrict__ prize, int64_t PB,
    const float2* __restrict__ locs, const float* __restrict__ mlen, int64_t LB,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, int check,
    float* __restrict__ reward, int32_t* status) {
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int NC = N + 1;
  const uint64_t gm = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const int64_t b0 = ((int64_t)blockIdx.x * kOpWaves + w) * RW + grp;
  const bool valid = b0 < B;
  const int64_t b = valid ? b0 : B - 1;
  const float* prow = prize + (PB == B ? b : b % PB) * (int64_t)NC;
  const int64_t lb = check ? (LB == B ? b : b % LB) * (int64_t)NC : 0;
  const float2* lrow = locs + lb;  // read with check only
  const int64_t* arow = actions + b * sb;
  uint32_t seen = 0u;  // customers 32 sl .. 32 sl + 31 met so far
  bool dup = false, range = false, have = false, have0 = false;
  float px = 0.f, py = 0.f, fx = 0.f, fy = 0.f;  // the previous and the first tour point
  double sum = 0.0, len = 0.0;
  int64_t a = arow[0];
  const int64_t a0 = a;
  for (int t = 0; t < T; ++t) {
    const int64_t an = t + 1 < T ? arow[(int64_t)(t + 1) * st] : 0;  // issued a step ahead
    const bool in = a >= 0 && a <= N;
    range |= !in;
    const int ac = in ? (int)a : 0;
    if (in) sum += (double)prow[ac];
    if (check) {  // wave-uniform
      float qx = 0.f, qy = 0.f;
      if (in) {
        const float2 q = lrow[ac];
        qx = q.x, qy = q.y;
        if (have) len += (double)edge_len(px, py, qx, qy);
      }
      if (t == 0) fx = qx, fy = qy, have0 = in;
      const uint32_t wv = (uint32_t)__shfl((int)seen, gbase + (ac >> 5), 64);
      dup |= in && ac != 0 && ((wv >> (ac & 31)) & 1u);
      if (in && sl == (ac >> 5)) seen |= 1u << (ac & 31);
      px = qx, py = qy, have = in;
    }
    a = an;
  }
  bool over = false;
  if (check) {
    if (have && have0) len += (double)edge_len(px, py, fx, fy);
    const float flen = (float)len;
    const float2 dep = lrow[0];
    const float* mrow = mlen + lb;
    bool mine = false;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const int c = 32 * sl + k;
      if (c < NC) {
        const float2 q = lrow[c];
        const float bound = ((mrow[c] + edge_len(dep.x, dep.y, q.x, q.y)) + 1e-6f) + 1e-5f;
        mine |= !(flen <= bound);
      }
    }
    over = ((__ballot(mine) >> gbase) & gm) != 0ull;
  }
  if (valid && sl == 0) {
    reward[b] = T == 1 ? 0.f : (float)sum;
    if (range) set_status(status, CO_ST_INDEX_RANGE);
    if (T == 1 && a0 != 0) set_status(status, CO_ST_OP_SINGLE_NONZERO);
    if (check && dup) set_status(status, CO_ST_OP_DUPLICATE);
    if (check && !dup && over) set_status(status, CO_ST_OP_LENGTH);
  }
}

inline bool op_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N >= 1 && N <= CO_OP_MAX_N; }
inline bool op_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

}  // namespace

extern "C" int co_op_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                           const float* prize_in, const float* max_length_in, float* locs_out,
                           float* prize_out, float* max_length_out, float* tour_length,
                           float* total_prize, int64_t* cur, int64_t* i, uint8_t* visited,
                           uint8_t* mask, void* stream) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !prize_in || !max_length_in || !locs_out || !prize_out ||
      !max_length_out || !tour_length || !total_prize || !cur || !i || !visited || !mask)
    return CO_E_INVAL;
  if (op_mis8(depot) || op_mis8(locs_in) || op_mis8(locs_out)) return CO_E_ALIGN;
  OpArgs a{};
  a.B = B, a.N = (int)N, a.T = 0;
  a.depot = reinterpret_cast<const float2*>(depot);
  a.locs_in = reinterpret_cast<const float2*>(locs_in);
  a.prize_in = prize_in, a.ml_in = max_length_in;
  a.locs_out = reinterpret_cast<float2*>(locs_out);
  a.prize_out = prize_out, a.ml_out = max_length_out;
  a.vis_out = visited, a.mask_out = mask;
  a.tl_out = tour_length, a.pz_out = total_prize, a.cur_out = cur, a.i_out = i;
  return op_launch(a, stream);
}

extern "C" int co_op_step(int64_t B, int64_t N, const int64_t* action, const float* locs,
                          const float* prize, const float* max_length,
                          const uint8_t* visited_in, uint8_t* visited_out,
                          const float* tl_in, float* tl_out, const float* pz_in, float* pz_out,
                          const int64_t* cur_in, int64_t* cur_out, const int64_t* i_in,
                          int64_t* i_out, uint8_t* done, uint8_t* reward, uint8_t* mask,
                          int32_t* status, void* stream) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !locs || !prize || !max_length || !visited_in || !visited_out || !tl_in ||
      !tl_out || !pz_in || !pz_out || !cur_in || !cur_out || !i_in || !i_out || !done ||
      !reward || !mask)
    return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  OpArgs a{};
  a.B = B, a.N = (int)N, a.T = 1;
  a.actions = action, a.st = 0, a.sb = 1;
  a.locs = reinterpret_cast<const float2*>(locs), a.prize = prize, a.ml = max_length;
  a.vis_in = visited_in, a.vis_out = visited_out, a.mask_out = mask;
  a.tl_in = tl_in, a.tl_out = tl_out, a.pz_in = pz_in, a.pz_out = pz_out;
  a.cur_in = cur_in, a.cur_out = cur_out, a.i_in = i_in, a.i_out = i_out;
  a.done = done, a.reward = reward, a.status = status;
  return op_launch(a, stream);
}

extern "C" int co_op_action_mask(int64_t B, int64_t N, const float* locs,
                                 const float* max_length, const uint8_t* visited,
                                 const float* tour_length, const int64_t* cur, uint8_t* mask,
                                 void* stream) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !max_length || !visited || !tour_length || !cur || !mask) return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  OpArgs a{};
  a.B = B, a.N = (int)N, a.T = 0;
  a.locs = reinterpret_cast<const float2*>(locs), a.ml = max_length;
  a.vis_in = visited, a.tl_in = tour_length, a.cur_in = cur, a.mask_out = mask;
  return op_launch(a, stream);
}

extern "C" int co_op_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions, int64_t st,
                           int64_t sb, const float* locs, const float* prize,
                           const float* max_length, const uint8_t* mask_in, uint8_t* visited,
                           float* tour_length, float* total_prize, int64_t* cur, int64_t* i,
                           uint8_t* done, uint8_t* reward, uint8_t* mask, uint8_t* feasible,
                           float* length, int32_t* status, void* stream) {
  if (!op_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !locs || !prize || !max_length || !visited || !tour_length || !total_prize ||
      !cur || !i || !done || !reward || !mask || (feasible && !mask_in) || mask == mask_in)
    return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  OpArgs a{};
  a.B = B, a.N = (int)N, a.T = (int)T;
  a.actions = actions, a.st = st, a.sb = sb;
  a.locs = reinterpret_cast<const float2*>(locs), a.prize = prize, a.ml = max_length;
  a.mask_in = mask_in, a.vis_in = visited, a.vis_out = visited, a.mask_out = mask;
  a.tl_in = tour_length, a.tl_out = tour_length, a.pz_in = total_prize, a.pz_out = total_prize;
  a.cur_in = cur, a.cur_out = cur, a.i_in = i, a.i_out = i;
  a.done = done, a.reward = reward, a.feasible = feasible, a.length = length;
  a.status = status;
  return op_launch(a, stream);
}

extern "C" int co_op_reward(int64_t B, int64_t N, int64_t T, const float* prize,
                            int64_t prize_batch, const float* locs, const float* max_length,
                            int64_t locs_batch, const int64_t* actions, int64_t sb, int64_t st,
                            int check, float* reward, int32_t* status, void* stream) {
  if (!op_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (prize_batch <= 0 || (B > 0 && B % prize_batch != 0)) return CO_E_INVAL;
  if (check && (locs_batch <= 0 || (B > 0 && B % locs_batch != 0))) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!prize || !actions || !reward || (check && (!locs || !max_length || !status)))
    return CO_E_INVAL;
  if (check && op_mis8(locs)) return CO_E_ALIGN;
  const int G = op_groups((int)N + 1);
  const unsigned grid = cover_grid(B, (64 / G) * kOpWaves, 64 * kOpWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_OP_R(GG)                                                                         \
  hipLaunchKernelGGL((op_reward_kernel<GG>), dim3(grid), dim3(64 * kOpWaves), 0, s, B,      \
                     (int)N, (int)T, prize, prize_batch, reinterpret_cast<const float2*>(locs), \
                     max_length, locs_batch, actions, sb, st, check, reward, status)
  switch (G) {
    case 1: CO_OP_R(1); break;
    case 2: CO_OP_R(2); break;
    case 4: CO_OP_R(4); break;
    case 8: CO_OP_R(8); break;
    case 16: CO_OP_R(16); break;
    default: CO_OP_R(32);
  }
#undef CO_OP_R
  return launch_status();
}
