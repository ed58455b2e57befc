// CVRP with time windows (rl4co/envs/routing/cvrptw/env.py) for gfx950: reset, the fused
// step (time update + CVRP step + get_action_mask), the stand-alone mask, T preset steps
// in one launch, and the time-window part of check_solution_validity.  include/co_env.h
// states the semantics; this file is their device form.
//
// Layout (cvrptw_rows_kernel): a group of G lanes owns one row, 64 / G rows per wave, lane
// sl holds columns c = sl + G j (j < U) in registers -- coordinates, window start / end,
// demand, and for more than one step the durations; the visited row is one bit per held
// column.  G is the smallest of 8 / 16 / 32 / 64 with 2 G >= N + 1, so small N fills the
// lanes; past 128 columns G = 64 and U grows to 4 / 8 / 16.  Column loads are coalesced
// across the group and all issued before the first use.  A value of the action's column
// (its coordinates, window, duration, demand, visited bit) is a register select plus one
// ds_bpermute from the lane that holds it, so no load depends on the action but the
// action's own and, on a single step, distances_in[a] and durations[a].  Row sums (done,
// the depot column's "some customer open") are DPP / ballot operations on the group.  No
// LDS on the data path, no workgroup barrier; `not_done`: one atomic per workgroup.
//
// Steps in one launch: between two steps only row scalars change (time, used capacity, the
// current node's coordinates, one visited bit), and the leg of step t >= 1 is the one
// distance dist(locs[current], locs[a]) -- the element the single step's mask call would
// have stored -- so the N + 1 square roots and the mask run once, after the last step.
#include "co_common.hpp"

using namespace co;

namespace {

__device__ __forceinline__ float tw_ldf(const void* p, int dt, int64_t i) {
  if (dt == CO_DT_F32) return static_cast<const float*>(p)[i];
  if (dt == CO_DT_I32) return (float)static_cast<const int32_t*>(p)[i];
  return (float)static_cast<const int64_t*>(p)[i];
}

// co_env.h "Distance": every operation rounded on its own (built with -ffp-contract=off)
__device__ __forceinline__ float tw_dist(float px, float py, float qx, float qy) {
  const float dx = px - qx, dy = py - qy;
  return sqrtf(dx * dx + dy * dy);
}

// torch.max(a, b): NaN when either is NaN
__device__ __forceinline__ float tw_max(float p, float s) {
  return (p != p || s != s) ? __builtin_nanf("") : (p > s ? p : s);
}

// the reference's `.int()`: toward zero; -2^31 for a NaN or a value outside int32
__device__ __forceinline__ float tw_trunc(float x) {
  return (x >= -2147483648.f && x < 2147483648.f) ? (float)(int32_t)x : -2147483648.f;
}

struct TwArgs {
  int64_t B;
  int N, T;
  const int64_t* actions;  // T >= 1
  int64_t st, sb;
  const float2 *depot, *locs_in;  // reset: locs = cat(depot, locs_in), the state is fresh
  float vcap_fill;
  const float2* locs;
  float2* locs_out;
  const float *demand, *used_in, *vcap;
  float *used_out, *vcap_out;
  const uint8_t* vis_in;
  uint8_t* vis_out;
  const float* t_in;
  float* t_out;
  const int64_t* cur_in;
  int64_t* cur_out;
  const float* dist_in;
  const void* dur;
  int dur_dt;
  const void* tw;
  int tw_dt;
  uint8_t *done, *reward;
  float2* cur_loc;
  float* dist;
  uint8_t *mask, *feasible;
  float* time;
  int32_t *status, *not_done;
};

constexpr int kTwWaves = 4;

template <int U>
__device__ __forceinline__ float tw_pick(const float (&r)[U], int j) {
  float v = r[0];
#pragma unroll
  for (int k = 1; k < U; ++k) {
    const float rk = r[k];  // read first: a select of values, not of addresses
    v = j == k ? rk : v;
  }
  return v;
}

template <int G, int U>
__global__ __launch_bounds__(64 * kTwWaves) void cvrptw_rows_kernel(const TwArgs p) {
  static_assert(U <= 32, "one visited bit per held column");
  __shared__ int s_left[kTwWaves];
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int N = p.N, NC = N + 1, T = p.T;
  const int64_t b0 = ((int64_t)blockIdx.x * kTwWaves + w) * RW + grp;
  const bool valid = b0 < p.B;  // rows past B re-read row B-1 and store nothing
  const int64_t b = valid ? b0 : p.B - 1;
  const int64_t row = b * NC;
  const bool fresh = p.depot != nullptr;
  const uint64_t gm = G == 64 ? ~0ull : ((1ull << G) - 1ull);

  // ---- the row's columns
  float X[U], Y[U], TWS[U], TWE[U], DEM[U], DUR[U];
  uint32_t visb = 0u;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int c0 = sl + G * j;
    const int c = c0 < NC ? c0 : 0;
    float2 xy;
    if (fresh)
      xy = c == 0 ? p.depot[b] : p.locs_in[b * N + (c - 1)];
    else
      xy = p.locs[row + c];
    X[j] = xy.x;
    Y[j] = xy.y;
    TWS[j] = tw_ldf(p.tw, p.tw_dt, 2 * (row + c));
    TWE[j] = tw_ldf(p.tw, p.tw_dt, 2 * (row + c) + 1);
    DEM[j] = p.demand[b * N + (c >= 1 ? c - 1 : 0)];
    DUR[j] = T > 1 ? tw_ldf(p.dur, p.dur_dt, row + c) : 0.f;
    if (!fresh && p.vis_in[row + c] != 0) visb |= 1u << j;
  }
  float used = fresh ? 0.f : p.used_in[b];
  const float cap = fresh ? p.vcap_fill : p.vcap[b];
  float tnow = fresh ? 0.f : p.t_in[b];
  int64_t cur = (fresh || !p.cur_in) ? 0 : p.cur_in[b];
  float cx = 0.f, cy = 0.f;

  auto bcast = [&](const float(&r)[U], int col) {
    return __shfl(tw_pick<U>(r, col / G), gbase + col % G, 64);
  };
  // "some customer open" of the CVRP mask (cvrp/env.py:146-148) under the present state
  auto any_open = [&]() {
    bool open = false;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int c = sl + G * j;
      open |= c >= 1 && c < NC && !((visb >> j) & 1u) && !(DEM[j] + used > cap);
    }
    return ((__ballot(open) >> gbase) & gm) != 0ull;
  };

  // ---- the preset steps (cvrptw/env.py:117-134, cvrp/env.py:73-105)
  for (int t = 0; t < T; ++t) {
    const int64_t a = p.actions[t * p.st + b * p.sb];
    const bool bad = a < 0 || a > N;
    if (valid && bad && sl == 0) set_status(p.status, CO_ST_INDEX_RANGE);
    const int ac = (int)(a < 0 ? 0 : (a > N ? N : a));
    const float ax = bcast(X, ac), ay = bcast(Y, ac);
    const float dleg = t == 0 ? p.dist_in[row + ac] : tw_dist(cx, cy, ax, ay);
    const float du = T > 1 ? bcast(DUR, ac) : tw_ldf(p.dur, p.dur_dt, row + ac);
    const int dcol = (int)(a - 1 < 0 ? 0 : (a - 1 > N - 1 ? N - 1 : a - 1)) + 1;
    const float dm = bcast(DEM, dcol);
    if (p.feasible) {  // action_mask[b, a] of the state before this step
      const bool anyo = any_open();
      const bool vis_a = (__shfl(visb, gbase + ac % G, 64) >> (ac / G)) & 1u;
      const bool cv = ac == 0 ? !((cur == 0) && anyo) : (!vis_a && !(dm + used > cap));
      const bool reach = tnow + dleg <= bcast(TWE, ac);
      if (valid && sl == 0) p.feasible[(int64_t)t * p.B + b] = !bad && cv && reach;
    }
    const float m01 = a != 0 ? 1.0f : 0.0f;
    tnow = m01 * (tw_max(tnow + dleg, bcast(TWS, ac)) + du);
    used = (used + dm) * m01;
    if (!bad && sl == ac % G) visb |= 1u << (ac / G);
    cur = a;
    cx = ax;
    cy = ay;
    if (p.time && valid && sl == 0) p.time[(int64_t)t * p.B + b] = tnow;
  }
  if (T == 0) {
    const int cc = (int)(cur < 0 ? 0 : (cur > N ? N : cur));
    cx = bcast(X, cc);
    cy = bcast(Y, cc);
  }

  // ---- get_action_mask on the state (cvrptw/env.py:103-115, cvrp/env.py:137-149)
  const bool anyo = any_open();
  const bool dep = !((cur == 0) && anyo);
  uint32_t cnt = 0u;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int c = sl + G * j;
    const bool live = c < NC;
    const bool v = (visb >> j) & 1u;
    cnt += live && v;
    const float d = tw_dist(cx, cy, X[j], Y[j]);
    const bool cv = c == 0 ? dep : (!v && !(DEM[j] + used > cap));
    const bool reach = tnow + d <= TWE[j];
    if (valid && live) {
      p.dist[row + c] = d;
      p.mask[row + c] = cv && reach;
      if (p.vis_out) p.vis_out[row + c] = v;
      if (p.locs_out) p.locs_out[row + c] = make_float2(X[j], Y[j]);
    }
  }
  cnt = grp_reduce<G>(cnt, [](uint32_t x, uint32_t y) { return x + y; });
  if (valid) {  // the row scalars, spread over the group's lanes
    if (sl == 0 && p.used_out) p.used_out[b] = used;
    if (sl == 1 && p.cur_out) p.cur_out[b] = cur;
    if (sl == 2 && p.done) p.done[b] = (int)cnt == NC;
    if (sl == 3 && p.reward) p.reward[b] = 0;
    if (sl == 4 && p.t_out) p.t_out[b] = tnow;
    if (sl == 5) p.cur_loc[b] = make_float2(cx, cy);
    if (sl == 6 && p.vcap_out) p.vcap_out[b] = cap;
  }
  if (p.not_done) {  // one atomic per workgroup
    const int left = valid && sl == 0 && (int)cnt != NC;
    const int wl = (int)wave_sum((uint32_t)left);
    if (lane == 0) s_left[w] = wl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int q = 0; q < kTwWaves; ++q) tot += s_left[q];
      if (tot) atomicAdd(p.not_done, tot);
    }
  }
}

int tw_launch(const TwArgs& a, void* stream) {
  const int NC = a.N + 1;
  const int G = NC <= 16 ? 8 : NC <= 32 ? 16 : NC <= 64 ? 32 : 64;
  const int U = NC <= 128 ? 2 : NC <= 256 ? 4 : NC <= 512 ? 8 : 16;
  const int64_t rows_per_wg = (int64_t)(64 / G) * kTwWaves;
  const unsigned grid = cover_grid(a.B, (int)rows_per_wg, 64 * kTwWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_TW(GG, UU) \
  hipLaunchKernelGGL((cvrptw_rows_kernel<GG, UU>), dim3(grid), dim3(64 * kTwWaves), 0, s, a)
  if (G == 8) CO_TW(8, 2);
  else if (G == 16) CO_TW(16, 2);
  else if (G == 32) CO_TW(32, 2);
  else if (U == 2) CO_TW(64, 2);
  else if (U == 4) CO_TW(64, 4);
  else if (U == 8) CO_TW(64, 8);
  else CO_TW(64, 16);
#undef CO_TW
  return launch_status();
}

// The time-window part of check_solution_validity (cvrptw/env.py:176-218), a thread per
// row: the instance tests over the row's columns, then the truncating scan over its actions.
__global__ __launch_bounds__(256) void cvrptw_check_kernel(
    int64_t B, int N, int64_t T, const float* __restrict__ locs,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, const void* dur, int dur_dt,
    const void* tw, int tw_dt, int32_t* status) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int NC = N + 1;
  const int64_t row = b * NC;
  const float* lr = locs + 2 * row;
  const float deadline0 = tw_ldf(tw, tw_dt, 1);  // time_windows[0, 0, 1]: batch row 0's depot
  int32_t bits = 0;
  for (int c = 0; c < NC; ++c) {
    const float s = tw_ldf(tw, tw_dt, 2 * (row + c)), e = tw_ldf(tw, tw_dt, 2 * (row + c) + 1);
    const float du = tw_ldf(dur, dur_dt, row + c);
    const float d0 = tw_dist(lr[0], lr[1], lr[2 * c], lr[2 * c + 1]);
    if (s < 0.f || e < 0.f) bits |= CO_ST_TW_NEGATIVE;
    if (!((s + d0) + du <= deadline0)) bits |= CO_ST_TW_DEPOT_RETURN;
    if (du < 0.f) bits |= CO_ST_DURATION_NEGATIVE;
    if (!(s < e)) bits |= CO_ST_TW_INFEASIBLE;
  }
  float t = 0.f;
  int64_t prev = 0;
  for (int64_t k = 0; k < T; ++k) {
    const int64_t a = actions[b * sb + k * st];
    if (a < 0 || a > N) {
      bits |= CO_ST_INDEX_RANGE;
      break;
    }
    const float d = tw_dist(lr[2 * prev], lr[2 * prev + 1], lr[2 * a], lr[2 * a + 1]);
    t = tw_max(tw_trunc(t + d), tw_ldf(tw, tw_dt, 2 * (row + a)));
    if (!(t <= tw_ldf(tw, tw_dt, 2 * (row + a) + 1))) bits |= CO_ST_TW_DEADLINE;
    t = t + tw_ldf(dur, dur_dt, row + a);
    if (a == 0) t = 0.f;
    prev = a;
  }
  if (bits) set_status(status, bits);
}

inline bool tw_dt_ok(int dt) { return dt == CO_DT_F32 || dt == CO_DT_I32 || dt == CO_DT_I64; }
inline bool tw_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

}  // namespace

extern "C" int co_cvrptw_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                               const float* demand, float vcap, const void* tw, int tw_dt,
                               float* locs_out, int64_t* cur, float* time, float* used,
                               float* vcap_out, uint8_t* visited, float* cur_loc, float* dist,
                               uint8_t* mask, void* stream) {
  if (B < 0 || N <= 0 || N > CO_CVRPTW_MAX_N) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !demand || !tw || !locs_out || !cur || !time || !used || !vcap_out ||
      !visited || !cur_loc || !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt)) return CO_E_MODE;
  if (tw_mis8(depot) || tw_mis8(locs_in) || tw_mis8(locs_out) || tw_mis8(cur_loc))
    return CO_E_ALIGN;
  TwArgs a{};
  a.B = B, a.N = (int)N, a.T = 0;
  a.depot = reinterpret_cast<const float2*>(depot);
  a.locs_in = reinterpret_cast<const float2*>(locs_in);
  a.vcap_fill = vcap;
  a.locs_out = reinterpret_cast<float2*>(locs_out);
  a.demand = demand, a.used_out = used, a.vcap_out = vcap_out, a.vis_out = visited;
  a.t_out = time, a.cur_out = cur, a.tw = tw, a.tw_dt = tw_dt;
  a.cur_loc = reinterpret_cast<float2*>(cur_loc), a.dist = dist, a.mask = mask;
  return tw_launch(a, stream);
}

extern "C" int co_cvrptw_step(int64_t B, int64_t N, const int64_t* action, const float* locs,
                              const float* demand, const float* used_in, float* used_out,
                              const float* vcap, const uint8_t* vis_in, uint8_t* vis_out,
                              const float* t_in, const float* dist_in, const void* dur,
                              int dur_dt, const void* tw, int tw_dt, float* t_out,
                              int64_t* cur_out, uint8_t* done, uint8_t* reward, float* cur_loc,
                              float* dist, uint8_t* mask, int32_t* status, int32_t* not_done,
                              void* stream) {
  if (B < 0 || N <= 0 || N > CO_CVRPTW_MAX_N) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !locs || !demand || !used_in || !used_out || !vcap || !vis_in || !vis_out ||
      !t_in || !dist_in || !dur || !tw || !t_out || !cur_out || !done || !reward || !cur_loc ||
      !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  TwArgs a{};
  a.B = B, a.N = (int)N, a.T = 1;
  a.actions = action, a.st = 0, a.sb = 1;
  a.locs = reinterpret_cast<const float2*>(locs);
  a.demand = demand, a.used_in = used_in, a.used_out = used_out, a.vcap = vcap;
  a.vis_in = vis_in, a.vis_out = vis_out, a.t_in = t_in, a.t_out = t_out, a.cur_out = cur_out;
  a.dist_in = dist_in, a.dur = dur, a.dur_dt = dur_dt, a.tw = tw, a.tw_dt = tw_dt;
  a.done = done, a.reward = reward, a.cur_loc = reinterpret_cast<float2*>(cur_loc);
  a.dist = dist, a.mask = mask, a.status = status, a.not_done = not_done;
  return tw_launch(a, stream);
}

extern "C" int co_cvrptw_action_mask(int64_t B, int64_t N, const float* locs, const float* demand,
                                     const float* used, const float* vcap,
                                     const uint8_t* visited, const int64_t* cur,
                                     const float* time, const void* tw, int tw_dt,
                                     float* cur_loc, float* dist, uint8_t* mask, void* stream) {
  if (B < 0 || N <= 0 || N > CO_CVRPTW_MAX_N) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !demand || !used || !vcap || !visited || !cur || !time || !tw || !cur_loc ||
      !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  TwArgs a{};
  a.B = B, a.N = (int)N, a.T = 0;
  a.locs = reinterpret_cast<const float2*>(locs);
  a.demand = demand, a.used_in = used, a.vcap = vcap, a.vis_in = visited, a.t_in = time;
  a.cur_in = cur, a.tw = tw, a.tw_dt = tw_dt;
  a.cur_loc = reinterpret_cast<float2*>(cur_loc), a.dist = dist, a.mask = mask;
  return tw_launch(a, stream);
}

extern "C" int co_cvrptw_check(int64_t B, int64_t N, int64_t T, const float* locs,
                               const int64_t* actions, int64_t sb, int64_t st, const void* dur,
                               int dur_dt, const void* tw, int tw_dt, int32_t* status,
                               void* stream) {
  if (B < 0 || N <= 0 || N > CO_CVRPTW_MAX_N || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || (T > 0 && !actions) || !dur || !tw || !status) return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  const unsigned grid = cover_grid(B, 256);
  if (grid == 0) return CO_E_INVAL;
  hipLaunchKernelGGL(cvrptw_check_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, B,
                     (int)N, T, locs, actions, sb, st, dur, dur_dt, tw, tw_dt, status);
  return launch_status();
}

extern "C" int co_cvrptw_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                               int64_t st, int64_t sb, const float* locs, const float* demand,
                               float* used, const float* vcap, uint8_t* visited, float* time_io,
                               int64_t* cur, const float* dist_in, const void* dur, int dur_dt,
                               const void* tw, int tw_dt, uint8_t* done, uint8_t* reward,
                               float* cur_loc, float* dist, uint8_t* mask, uint8_t* feasible,
                               float* time, int32_t* status, int32_t* not_done, void* stream) {
  if (B < 0 || N <= 0 || N > CO_CVRPTW_MAX_N || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !locs || !demand || !used || !vcap || !visited || !time_io || !cur ||
      !dist_in || !dur || !tw || !done || !reward || !cur_loc || !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  TwArgs a{};
  a.B = B, a.N = (int)N, a.T = (int)T;
  a.actions = actions, a.st = st, a.sb = sb;
  a.locs = reinterpret_cast<const float2*>(locs);
  a.demand = demand, a.used_in = used, a.used_out = used, a.vcap = vcap;
  a.vis_in = visited, a.vis_out = visited, a.t_in = time_io, a.t_out = time_io;
  a.cur_in = cur, a.cur_out = cur;
  a.dist_in = dist_in, a.dur = dur, a.dur_dt = dur_dt, a.tw = tw, a.tw_dt = tw_dt;
  a.done = done, a.reward = reward, a.cur_loc = reinterpret_cast<float2*>(cur_loc);
  a.dist = dist, a.mask = mask, a.feasible = feasible, a.time = time;
  a.status = status, a.not_done = not_done;
  return tw_launch(a, stream);
}
