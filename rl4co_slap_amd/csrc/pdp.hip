// The pickup-and-delivery problem (rl4co/envs/routing/pdp/env.py) for gfx950: reset, the
// step, T preset steps in one launch, and the reward with check_solution_validity's two
// tests.  include/co_env.h (PDP) states the semantics; this file is their device form.
//
// Layout (pdp_rows_kernel, pdp_reward_kernel): a group of G lanes owns one row, 64 / G rows
// per wave, G the smallest of 1 / 2 / 4 / ... / 64 with 32 G >= N + 1.  Lane sl holds columns
// 32 sl .. 32 sl + 31 of the row's two sets (available, to_deliver) as one bit word each, so
// a step is the action (the same address on every lane of the group: one broadcast load),
// one bit test (a ds_bpermute of the word that holds the action's bit) and two bit edits on
// the lanes that hold the action's and the pair's bit.  The byte rows are read once (eight
// byte-aligned dwords per lane and row, squeezed to bits) and, after the last step, expanded
// and stored once.  `done` is a ballot over the group.  No LDS, no barrier, no scratch.
//
// The reward walks the tour in order on every lane of the group (f64 sum in tour order, as
// the header states it) and keeps "seen" as the same bit words: a value met twice or outside
// 0..T-1 fails the permutation test, a delivery met before its pickup the precedence test.
#include "co_common.hpp"

using namespace co;

namespace {

typedef uint32_t pdp_u32_align1 __attribute__((aligned(1)));

struct PdpArgs {
  int64_t B;
  int N, T;
  const int64_t* actions;  // T >= 1
  int64_t st, sb;
  const float2 *depot, *locs_in;  // reset: locs_out = cat(depot, locs_in), the state is fresh
  float2* locs_out;
  const uint8_t *mask_in, *av_in, *td_in;
  uint8_t *av_out, *td_out, *mask_out;
  const int64_t* i_in;
  int64_t *i_out, *cur_out;
  uint8_t *done, *reward, *terminated, *feasible;
  int32_t* status;
};

constexpr int kPdpWaves = 4;

// columns c0 .. c0 + 31 of a byte row of NC columns as a bit word (a non-zero byte: 1)
__device__ __forceinline__ uint32_t pdp_load_bits(const uint8_t* row, int c0, int NC) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // every load issued before the first use
    const int c = c0 + 4 * j;
    uint32_t x = 0u;
    if (c + 4 <= NC) {
      x = *reinterpret_cast<const pdp_u32_align1*>(row + c);
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
__device__ __forceinline__ void pdp_store_bits(uint8_t* row, int c0, int NC, uint32_t bits) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + 4 * j;
    const uint32_t x = (((bits >> (4 * j)) & 0xfu) * 0x00204081u) & 0x01010101u;
    if (c + 4 <= NC) {
      *reinterpret_cast<pdp_u32_align1*>(row + c) = x;
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (c + q < NC) row[c + q] = (uint8_t)(x >> (8 * q));
    }
  }
}

// the bits of a lane's word that are columns of the row
__device__ __forceinline__ uint32_t pdp_live(int c0, int NC) {
  const int n = NC - c0;
  return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : (1u << n) - 1u);
}

template <int G>
__global__ __launch_bounds__(64 * kPdpWaves) void pdp_rows_kernel(const PdpArgs p) {
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int N = p.N, NC = N + 1, h = N / 2, T = p.T;
  const int64_t b0 = ((int64_t)blockIdx.x * kPdpWaves + w) * RW + grp;
  const bool valid = b0 < p.B;  // rows past B re-read row B-1 and store nothing
  const int64_t b = valid ? b0 : p.B - 1;
  const int64_t row = b * NC;
  const bool fresh = p.depot != nullptr;
  const uint64_t gm = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const int c0 = 32 * sl;
  const uint32_t live = pdp_live(c0, NC);

  uint32_t av, td;
  if (fresh) {  // pdp/env.py:113-135
    av = live;
    td = live & pdp_live(c0, h + 1);
  } else {
    av = pdp_load_bits(p.av_in + row, c0, NC);
    td = pdp_load_bits(p.td_in + row, c0, NC);
  }
  int64_t iv = (fresh || !p.i_in) ? 0 : p.i_in[b];
  int64_t cur = 0;

  // ---- the preset steps (pdp/env.py:67-89)
  for (int t = 0; t < T; ++t) {
    const int64_t a = p.actions[t * p.st + b * p.sb];
    const bool bad = a < 0 || a > N;
    const int ac = bad ? 0 : (int)a;
    int pr = ac + h;
    pr = pr >= NC ? pr - NC : pr;
    if (p.feasible) {  // action_mask[b, a] of the state before this step
      bool f;
      if (t == 0) {
        f = p.mask_in[row + ac] != 0;
      } else {
        const uint32_t word = (uint32_t)__shfl((int)(av & td), gbase + (ac >> 5), 64);
        f = (word >> (ac & 31)) & 1u;
      }
      if (valid && sl == 0) p.feasible[(int64_t)t * p.B + b] = !bad && f;
    }
    if (valid && bad && sl == 0) set_status(p.status, CO_ST_INDEX_RANGE);
    if (!bad && sl == (ac >> 5)) av &= ~(1u << (ac & 31));
    if (!bad && sl == (pr >> 5)) td |= 1u << (pr & 31);
    cur = a;
  }

  // ---- the rows and the row scalars
  const uint32_t mask = (fresh && T == 0) ? (sl == 0 ? 1u : 0u) : (av & td);
  const bool left = ((__ballot((av & live) != 0u) >> gbase) & gm) != 0ull;
  if (!valid) return;
  pdp_store_bits(p.av_out + row, c0, NC, av & live);
  pdp_store_bits(p.td_out + row, c0, NC, td & live);
  pdp_store_bits(p.mask_out + row, c0, NC, mask & live);
  if (fresh)
    for (int c = sl; c < NC; c += G)
      p.locs_out[row + c] = c == 0 ? p.depot[b] : p.locs_in[b * N + (c - 1)];
  // the row scalars, spread over the group's lanes
  if (sl == 0) p.i_out[b] = iv + T;
  if (sl == 1 % G) p.cur_out[b] = cur;
  if (sl == 2 % G) p.done[b] = T == 0 ? 0 : !left;
  if (sl == 3 % G && p.reward) p.reward[b] = 0;
  if (sl == 4 % G && p.terminated) p.terminated[b] = 0;
}

int pdp_groups(int NC) {  // lanes per row: 32 columns each
  int g = 1;
  while (32 * g < NC) g *= 2;
  return g;
}

int pdp_launch(const PdpArgs& a, void* stream) {
  const int G = pdp_groups(a.N + 1);
  const int64_t rows_per_wg = (int64_t)(64 / G) * kPdpWaves;
  const unsigned grid = cover_grid(a.B, (int)rows_per_wg, 64 * kPdpWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_PDP(GG) \
  hipLaunchKernelGGL((pdp_rows_kernel<GG>), dim3(grid), dim3(64 * kPdpWaves), 0, s, a)
  switch (G) {
    case 1: CO_PDP(1); break;
    case 2: CO_PDP(2); break;
    case 4: CO_PDP(4); break;
    case 8: CO_PDP(8); break;
    case 16: CO_PDP(16); break;
    case 32: CO_PDP(32); break;
    default: CO_PDP(64);
  }
#undef CO_PDP
  return launch_status();
}

// reward + validity: the tour in order on every lane of the row's group
template <int G>
__global__ __launch_bounds__(64 * kPdpWaves) void pdp_reward_kernel(
    int64_t B, int N, int T, const float2* __restrict__ locs, int64_t LB,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, int check,
    float* __restrict__ reward, int32_t* status) {
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int T2 = T / 2;
  const int64_t b0 = ((int64_t)blockIdx.x * kPdpWaves + w) * RW + grp;
  const bool valid = b0 < B;
  const int64_t b = valid ? b0 : B - 1;
  const float2* lrow = locs + (LB == B ? b : b % LB) * (int64_t)(N + 1);
  const int64_t* arow = actions + b * sb;
  const float2 dep = lrow[0];
  uint32_t seen = 0u;  // values 32 sl .. 32 sl + 31 met so far
  bool dup = false, prec = false, range = false;
  float px = dep.x, py = dep.y;
  bool have = true;  // the previous tour point is in range
  double len = 0.0;
  int64_t a = arow[0];
  for (int t = 0; t < T; ++t) {
    const int64_t an = t + 1 < T ? arow[(int64_t)(t + 1) * st] : 0;  // issued a step ahead
    const bool in = a >= 0 && a <= N;
    range |= !in;
    float qx = 0.f, qy = 0.f;
    if (in) {
      const float2 q = lrow[a];
      qx = q.x, qy = q.y;
      if (have) len += (double)edge_len(px, py, qx, qy);
    }
    if (check) {  // wave-uniform
      const bool perm = a >= 0 && a < T;
      const int v = perm ? (int)a : 0;
      const int pk = v > T2 ? v - T2 : v;  // a delivery's pickup
      const uint32_t wv = (uint32_t)__shfl((int)seen, gbase + (v >> 5), 64);
      const uint32_t wp = (uint32_t)__shfl((int)seen, gbase + (pk >> 5), 64);
      dup |= !perm || ((wv >> (v & 31)) & 1u);
      prec |= perm && v > T2 && !((wp >> (pk & 31)) & 1u);
      if (perm && sl == (v >> 5)) seen |= 1u << (v & 31);
    }
    px = qx, py = qy, have = in;
    a = an;
  }
  if (have) len += (double)edge_len(px, py, dep.x, dep.y);
  if (valid && sl == 0) {
    reward[b] = -(float)len;
    if (range) set_status(status, CO_ST_INDEX_RANGE);
    if (check && dup) set_status(status, CO_ST_PDP_NOT_ALL_NODES);
    if (check && !dup && prec) set_status(status, CO_ST_PDP_PRECEDENCE);
  }
}

inline bool pdp_sizes_ok(int64_t B, int64_t N) {
  return B >= 0 && N >= 2 && N <= CO_PDP_MAX_N && N % 2 == 0;
}
inline bool pdp_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

}  // namespace

extern "C" int co_pdp_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                            float* locs_out, uint8_t* available, uint8_t* to_deliver,
                            uint8_t* mask, int64_t* cur, int64_t* i, uint8_t* done,
                            uint8_t* terminated, void* stream) {
  if (!pdp_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !locs_out || !available || !to_deliver || !mask || !cur || !i ||
      !done || !terminated)
    return CO_E_INVAL;
  if (pdp_mis8(depot) || pdp_mis8(locs_in) || pdp_mis8(locs_out)) return CO_E_ALIGN;
  PdpArgs a{};
  a.B = B, a.N = (int)N, a.T = 0;
  a.depot = reinterpret_cast<const float2*>(depot);
  a.locs_in = reinterpret_cast<const float2*>(locs_in);
  a.locs_out = reinterpret_cast<float2*>(locs_out);
  a.av_out = available, a.td_out = to_deliver, a.mask_out = mask;
  a.i_out = i, a.cur_out = cur, a.done = done, a.terminated = terminated;
  return pdp_launch(a, stream);
}

extern "C" int co_pdp_step(int64_t B, int64_t N, const int64_t* action, const uint8_t* av_in,
                           const uint8_t* td_in, uint8_t* av_out, uint8_t* td_out,
                           uint8_t* mask, const int64_t* i_in, int64_t* i_out,
                           int64_t* cur_out, uint8_t* done, uint8_t* reward, int32_t* status,
                           void* stream) {
  if (!pdp_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !av_in || !td_in || !av_out || !td_out || !mask || !i_in || !i_out ||
      !cur_out || !done || !reward)
    return CO_E_INVAL;
  PdpArgs a{};
  a.B = B, a.N = (int)N, a.T = 1;
  a.actions = action, a.st = 0, a.sb = 1;
  a.av_in = av_in, a.td_in = td_in, a.av_out = av_out, a.td_out = td_out, a.mask_out = mask;
  a.i_in = i_in, a.i_out = i_out, a.cur_out = cur_out, a.done = done, a.reward = reward;
  a.status = status;
  return pdp_launch(a, stream);
}

extern "C" int co_pdp_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                            int64_t st, int64_t sb, const uint8_t* mask_in, uint8_t* available,
                            uint8_t* to_deliver, uint8_t* mask, int64_t* i, int64_t* cur,
                            uint8_t* done, uint8_t* reward, uint8_t* feasible, int32_t* status,
                            void* stream) {
  if (!pdp_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !available || !to_deliver || !mask || !i || !cur || !done || !reward ||
      (feasible && !mask_in) || mask == mask_in)
    return CO_E_INVAL;
  PdpArgs a{};
  a.B = B, a.N = (int)N, a.T = (int)T;
  a.actions = actions, a.st = st, a.sb = sb;
  a.mask_in = mask_in, a.av_in = available, a.td_in = to_deliver;
  a.av_out = available, a.td_out = to_deliver, a.mask_out = mask;
  a.i_in = i, a.i_out = i, a.cur_out = cur, a.done = done, a.reward = reward;
  a.feasible = feasible, a.status = status;
  return pdp_launch(a, stream);
}

extern "C" int co_pdp_reward(int64_t B, int64_t N, int64_t T, const float* locs,
                             int64_t locs_batch, const int64_t* actions, int64_t sb, int64_t st,
                             int check, float* reward, int32_t* status, void* stream) {
  if (!pdp_sizes_ok(B, N) || T < 1 || T > 2048 || (check && T % 2 == 0))
    return CO_E_INVAL;
  if (locs_batch <= 0 || (B > 0 && B % locs_batch != 0)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !reward || (check && !status)) return CO_E_INVAL;
  if (pdp_mis8(locs)) return CO_E_ALIGN;
  // the seen words cover the values 0..T-1 of the permutation test and the columns 0..N
  const int G = pdp_groups((int)(T > N + 1 ? T : N + 1));
  const unsigned grid = cover_grid(B, (64 / G) * kPdpWaves, 64 * kPdpWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_PDP_R(GG)                                                                       \
  hipLaunchKernelGGL((pdp_reward_kernel<GG>), dim3(grid), dim3(64 * kPdpWaves), 0, s, B,   \
                     (int)N, (int)T, reinterpret_cast<const float2*>(locs), locs_batch,    \
                     actions, sb, st, check, reward, status)
  switch (G) {
    case 1: CO_PDP_R(1); break;
    case 2: CO_PDP_R(2); break;
    case 4: CO_PDP_R(4); break;
    case 8: CO_PDP_R(8); break;
    case 16: CO_PDP_R(16); break;
    case 32: CO_PDP_R(32); break;
    default: CO_PDP_R(64);
  }
#undef CO_PDP_R
  return launch_status();
}
