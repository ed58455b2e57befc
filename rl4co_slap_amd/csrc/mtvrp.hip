// Multi-task VRP (rl4co/envs/routing/mtvrp/env.py) for gfx950: reset, the fused step (state
// update + get_action_mask), the stand-alone mask, T preset steps in one launch, the reward
// and check_solution_validity.  include/co_env.h (MTVRP) states the semantics; this file is
// their device form.  Every row of a batch carries its own variant: open route, backhauls,
// a route-length limit and time windows are per-row data, not kernel modes.
//
// Layout (mtvrp_rows_kernel, as cvrptw_rows_kernel): a group of G lanes owns one row, 64 / G
// rows per wave, lane sl holds columns c = sl + G j (j < U) in registers -- coordinates,
// window start / end, service time, the two demands -- and the visited row as one bit per
// held column.  G is the smallest of 8 / 16 / 32 / 64 with 2 G >= N + 1; past 128 columns
// G = 64 and U grows to 4 / 8 / 16.  Column loads are coalesced across the group and all
// issued before the first use.  A value of the action's column is a register select plus one
// ds_bpermute from the lane that holds it (every held value is read before the select), so
// no load depends on the action but the action's own.  The distance to the depot d_j0 is
// recomputed from the depot's coordinates (one broadcast per row) where it is needed: the
// mask needs all N + 1 once, a step's `feasible` needs the action's alone, so holding it
// would cost U registers for nothing.  "Some customer can be visited", the count of
// unvisited linehaul columns and done are ballot / DPP operations on the group.  No LDS on
// the data path, no workgroup barrier; `not_done`: one atomic per workgroup.
//
// Steps in one launch: between two steps only row scalars change (time, route length, the
// two used capacities, the current node's coordinates and backhaul flag, one visited bit,
// the linehaul count), so the N + 1 mask columns run once, after the last step.  `feasible`
// of a customer column is that column's expressions alone; of the depot column it is true
// unless the row stands at the depot, and only then (a depot -> depot action, tested for the
// wave) is the whole row's mask evaluated.
#include "co_common.hpp"

using namespace co;

namespace {

// co_env.h "Distance": every operation rounded on its own (built with -ffp-contract=off)
__device__ __forceinline__ float mt_dist(float px, float py, float qx, float qy) {
  const float dx = px - qx, dy = py - qy;
  return sqrtf(dx * dx + dy * dy);
}

// torch.max(a, b): NaN when either is NaN
__device__ __forceinline__ float mt_max(float p, float s) {
  return (p != p || s != s) ? __builtin_nanf("") : (p > s ? p : s);
}

// the row scalars the mask reads
struct MtRow {
  float tnow, rlen, ul, ub, cap, speed, limit, nopen, twe0;
  bool lhm, cbh;
};

// can[c] before the depot column's overwrite (mtvrp/env.py:220-275), c's values given
__device__ __forceinline__ bool mt_can(const MtRow& r, float dij, float dj0, float tws, float twe,
                                       float svc, float dl, float db, bool vis) {
  const float arr = r.tnow + dij / r.speed;
  const bool reach = arr < twe;
  const bool depot_ok = ((mt_max(arr, tws) + svc) + dj0 / r.speed) * r.nopen < r.twe0;
  const bool over = (r.rlen + dij) + dj0 * r.nopen > r.limit;
  const bool dem = (r.lhm && !(dl + r.ul > r.cap) && !r.cbh && dl > 0.f) ||
                   (!(db + r.ub > r.cap) && db > 0.f);
  return reach && depot_ok && dem && !over && !vis;
}

struct MtArgs {
  int64_t B;
  int N, T, fresh;  // fresh: the reset state (zeros, at the depot), no state input is read
  const int64_t* actions;  // T >= 1
  int64_t st, sb;
  const float2 *locs, *tw;
  const float *svc, *dl, *db, *cap, *speed, *limit;
  const uint8_t* open;
  const uint8_t* vis_in;
  uint8_t* vis_out;
  const int64_t* cur_in;
  int64_t* cur_out;
  const float *t_in, *len_in, *ul_in, *ub_in;
  float *t_out, *len_out, *ul_out, *ub_out;
  uint8_t* done;
  float* reward;
  uint8_t *mask, *feasible;
  float *time, *rlen;
  int32_t *status, *not_done;
};

constexpr int kMtWaves = 4;

template <int U>
__device__ __forceinline__ float mt_pick(const float (&r)[U], int j) {
  float v = r[0];
#pragma unroll
  for (int k = 1; k < U; ++k) {
    const float rk = r[k];  // read first: a select of values, not of addresses
    v = j == k ? rk : v;
  }
  return v;
}

template <int G, int U>
__global__ __launch_bounds__(64 * kMtWaves) void mtvrp_rows_kernel(const MtArgs p) {
  static_assert(U <= 32, "one visited bit per held column");
  __shared__ int s_left[kMtWaves];
  constexpr int RW = 64 / G;
  const int lane = lane_id(), w = wave_in_block(), sl = lane % G, grp = lane / G;
  const int gbase = grp * G;
  const int N = p.N, NC = N + 1, T = p.T;
  const int64_t b0 = ((int64_t)blockIdx.x * kMtWaves + w) * RW + grp;
  const bool valid = b0 < p.B;  // rows past B re-read row B-1 and store nothing
  const int64_t b = valid ? b0 : p.B - 1;
  const int64_t row = b * NC;
  const bool fresh = p.fresh != 0;
  const uint64_t gm = G == 64 ? ~0ull : ((1ull << G) - 1ull);

  // ---- the row's columns
  float X[U], Y[U], TWS[U], TWE[U], SVC[U], DL[U], DB[U];
  uint32_t visb = 0u;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int c0 = sl + G * j;
    const int c = c0 < NC ? c0 : 0;
    const float2 xy = p.locs[row + c], win = p.tw[row + c];
    X[j] = xy.x;
    Y[j] = xy.y;
    TWS[j] = win.x;
    TWE[j] = win.y;
    SVC[j] = p.svc[row + c];
    DL[j] = p.dl[row + c];
    DB[j] = p.db[row + c];
    if (!fresh && p.vis_in[row + c] != 0) visb |= 1u << j;
  }
  MtRow r;
  r.tnow = fresh ? 0.f : p.t_in[b];
  r.rlen = fresh ? 0.f : p.len_in[b];
  r.ul = fresh ? 0.f : p.ul_in[b];
  r.ub = fresh ? 0.f : p.ub_in[b];
  r.cap = p.cap[b];
  r.speed = p.speed[b];
  r.limit = p.limit[b];
  r.nopen = p.open[b] != 0 ? 0.0f : 1.0f;
  int64_t cur = fresh ? 0 : p.cur_in[b];

  auto bcast = [&](const float(&v)[U], int col) {
    return __shfl(mt_pick<U>(v, col / G), gbase + col % G, 64);
  };
  const float x0 = __shfl(X[0], gbase, 64), y0 = __shfl(Y[0], gbase, 64);
  r.twe0 = __shfl(TWE[0], gbase, 64);
  float cx, cy;
  {
    const int cc = (int)(cur < 0 ? 0 : (cur > N ? N : cur));
    cx = bcast(X, cc);
    cy = bcast(Y, cc);
    r.cbh = bcast(DB, cc) > 0.f;
  }
  // unvisited columns with a linehaul demand: lh_missing = (count > 0)
  uint32_t lhc = 0u;
#pragma unroll
  for (int j = 0; j < U; ++j)
    lhc += (sl + G * j < NC) && !((visb >> j) & 1u) && DL[j] > 0.f;
  lhc = grp_reduce<G>(lhc, [](uint32_t x, uint32_t y) { return x + y; });
  r.lhm = lhc > 0u;

  // can[c] of the held columns as bits; returns "some customer column can be visited"
  auto row_can = [&](uint32_t& canb) {
    bool anyc = false;
    canb = 0u;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int c = sl + G * j;
      const float dij = mt_dist(cx, cy, X[j], Y[j]);
      const float dj0 = mt_dist(X[j], Y[j], x0, y0);
      const bool can =
          mt_can(r, dij, dj0, TWS[j], TWE[j], SVC[j], DL[j], DB[j], (visb >> j) & 1u);
      if (can) canb |= 1u << j;
      anyc |= can && c >= 1 && c < NC;
    }
    return ((__ballot(anyc) >> gbase) & gm) != 0ull;
  };

  // ---- the preset steps (mtvrp/env.py:100-162)
  for (int t = 0; t < T; ++t) {
    const int64_t a = p.actions[t * p.st + b * p.sb];
    const bool bad = a < 0 || a > N;
    if (valid && bad && sl == 0) set_status(p.status, CO_ST_INDEX_RANGE);
    const int ac = (int)(a < 0 ? 0 : (a > N ? N : a));
    const float ax = bcast(X, ac), ay = bcast(Y, ac);
    const float tws_a = bcast(TWS, ac), twe_a = bcast(TWE, ac), svc_a = bcast(SVC, ac);
    const float dl_a = bcast(DL, ac), db_a = bcast(DB, ac);
    const bool vis_a = (__shfl(visb, gbase + ac % G, 64) >> (ac / G)) & 1u;
    const float leg = mt_dist(cx, cy, ax, ay);
    if (p.feasible) {  // action_mask[b, a] of the state before this step
      bool f;
      const bool dd = !bad && ac == 0 && cur == 0;
      bool anyc = false;
      if (__any(dd)) {  // wave-uniform: every lane evaluates, the depot -> depot rows use it
        uint32_t canb;
        anyc = row_can(canb);
      }
      if (ac == 0)
        f = !(cur == 0 && anyc);
      else
        f = mt_can(r, leg, mt_dist(ax, ay, x0, y0), tws_a, twe_a, svc_a, dl_a, db_a, vis_a);
      if (valid && sl == 0) p.feasible[(int64_t)t * p.B + b] = !bad && f;
    }
    if (!bad) {
      const float m01 = a != 0 ? 1.0f : 0.0f;
      r.tnow = m01 * (mt_max(r.tnow + leg / r.speed, tws_a) + svc_a);
      r.rlen = m01 * (r.rlen + leg);
      r.ul = m01 * (r.ul + dl_a);
      r.ub = m01 * (r.ub + db_a);
      if (!vis_a && dl_a > 0.f) --lhc;
      r.lhm = lhc > 0u;
      if (sl == ac % G) visb |= 1u << (ac / G);
      cur = a;
      cx = ax;
      cy = ay;
      r.cbh = db_a > 0.f;
    }
    if (valid && sl == 0) {
      if (p.time) p.time[(int64_t)t * p.B + b] = r.tnow;
      if (p.rlen) p.rlen[(int64_t)t * p.B + b] = r.rlen;
    }
  }

  // ---- get_action_mask on the state (mtvrp/env.py:212-279)
  uint32_t canb;
  const bool anyc = row_can(canb);
  const bool dep = !((cur == 0) && anyc);
  uint32_t cnt = 0u;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int c = sl + G * j;
    const bool live = c < NC;
    const bool v = (visb >> j) & 1u;
    cnt += live && v;
    if (valid && live) {
      p.mask[row + c] = c == 0 ? dep : (bool)((canb >> j) & 1u);
      if (p.vis_out) p.vis_out[row + c] = v;
    }
  }
  cnt = grp_reduce<G>(cnt, [](uint32_t x, uint32_t y) { return x + y; });
  if (valid) {  // the row scalars, spread over the group's lanes
    if (sl == 0 && p.t_out) p.t_out[b] = r.tnow;
    if (sl == 1 && p.len_out) p.len_out[b] = r.rlen;
    if (sl == 2 && p.ul_out) p.ul_out[b] = r.ul;
    if (sl == 3 && p.ub_out) p.ub_out[b] = r.ub;
    if (sl == 4 && p.cur_out) p.cur_out[b] = cur;
    if (sl == 5 && p.done) p.done[b] = (int)cnt == NC;
    if (sl == 6 && p.reward) p.reward[b] = 0.f;
  }
  if (p.not_done) {  // one atomic per workgroup
    const int left = valid && sl == 0 && (int)cnt != NC;
    const int wl = (int)wave_sum((uint32_t)left);
    if (lane == 0) s_left[w] = wl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int q = 0; q < kMtWaves; ++q) tot += s_left[q];
      if (tot) atomicAdd(p.not_done, tot);
    }
  }
}

int mt_launch(const MtArgs& a, void* stream) {
  const int NC = a.N + 1;
  const int G = NC <= 16 ? 8 : NC <= 32 ? 16 : NC <= 64 ? 32 : 64;
  const int U = NC <= 128 ? 2 : NC <= 256 ? 4 : NC <= 512 ? 8 : 16;
  const int64_t rows_per_wg = (int64_t)(64 / G) * kMtWaves;
  const unsigned grid = cover_grid(a.B, (int)rows_per_wg, 64 * kMtWaves);
  if (grid == 0) return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
#define CO_MT(GG, UU) \
  hipLaunchKernelGGL((mtvrp_rows_kernel<GG, UU>), dim3(grid), dim3(64 * kMtWaves), 0, s, a)
  if (G == 8) CO_MT(8, 2);
  else if (G == 16) CO_MT(16, 2);
  else if (G == 32) CO_MT(32, 2);
  else if (U == 2) CO_MT(64, 2);
  else if (U == 4) CO_MT(64, 4);
  else if (U == 8) CO_MT(64, 8);
  else CO_MT(64, 16);
#undef CO_MT
  return launch_status();
}

// MTVRPEnv._get_reward (mtvrp/env.py:281-291), a thread per row: the legs depot -> a_0 ->
// ... -> a_{T-1} -> depot summed in f64 and rounded once, a leg into the depot skipped on an
// open row.  Once per episode, so the strided action reads are left as they are.
__global__ __launch_bounds__(256) void mtvrp_reward_kernel(
    int64_t B, int N, int64_t T, const float2* __restrict__ locs,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st,
    const uint8_t* __restrict__ open, float* __restrict__ reward, int32_t* status) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float2* lr = locs + b * (int64_t)(N + 1);
  const bool op = open[b] != 0;
  const float2 dep = lr[0];
  float2 prev = dep;
  bool prev_ok = true, range = false;
  double acc = 0.0;
  for (int64_t k = 0; k < T; ++k) {
    const int64_t a = actions[b * sb + k * st];
    if (a < 0 || a > N) {
      range = true;
      prev_ok = false;
      continue;
    }
    const float2 q = lr[a];
    if (prev_ok && !(a == 0 && op)) acc += (double)mt_dist(prev.x, prev.y, q.x, q.y);
    prev = q;
    prev_ok = true;
  }
  if (prev_ok && !op) acc += (double)mt_dist(prev.x, prev.y, dep.x, dep.y);
  reward[b] = -(float)acc;
  if (range) set_status(status, CO_ST_INDEX_RANGE);
}

// check_solution_validity (mtvrp/env.py:294-365), a thread per row; the "visited once" set
// of a row is a bit row in LDS of the thread's own ((N + 32) / 32 words).
constexpr int kMtCheckThreads = 64;
__global__ __launch_bounds__(kMtCheckThreads) void mtvrp_check_kernel(
    int64_t B, int N, int64_t T, const float2* __restrict__ locs,
    const int64_t* __restrict__ actions, int64_t sb, int64_t st, const float2* __restrict__ tw,
    const float* __restrict__ svc, const float* __restrict__ dl, const float* __restrict__ db,
    const float* __restrict__ cap, const float* __restrict__ limit,
    const uint8_t* __restrict__ open, int32_t* status) {
  extern __shared__ uint32_t s_seen[];
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int NC = N + 1, words = (N + 32) >> 5;
  uint32_t* seen = s_seen + (int)threadIdx.x * words;
  const int64_t row = b * NC;
  const float2* lr = locs + row;
  int32_t bits = 0;
  // "Invalid tour": every customer exactly once, every other entry the depot
  for (int k = 0; k < words; ++k) seen[k] = 0u;
  int64_t nonzero = 0;
  bool range = false, dup = false;
  for (int64_t k = 0; k < T; ++k) {
    const int64_t a = actions[b * sb + k * st];
    if (a < 0 || a > N) {
      range = true;
    } else if (a != 0) {
      ++nonzero;
      const uint32_t bit = 1u << (a & 31);
      dup |= (seen[a >> 5] & bit) != 0u;
      seen[a >> 5] |= bit;
    }
  }
  if (range) bits |= CO_ST_INDEX_RANGE;
  if (range || dup || nonzero != N) bits |= CO_ST_INVALID_TOUR;
  const float lim = limit[b], twe0 = tw[row].y, vc = cap[b];
  if (!(lim >= 0.f)) bits |= CO_ST_MT_LIMIT_NEGATIVE;
  const float2 dep = lr[0];
  for (int c = 0; c < NC; ++c) {
    const float2 win = tw[row + c];
    const float s = svc[row + c];
    const float d0 = mt_dist(lr[c].x, lr[c].y, dep.x, dep.y);
    if (!(win.x >= 0.f) || !(win.y >= 0.f)) bits |= CO_ST_MT_TW_NEGATIVE;
    if (!(s >= 0.f)) bits |= CO_ST_MT_SERVICE_NEGATIVE;
    if (!(win.x < win.y)) bits |= CO_ST_MT_TW_INFEASIBLE;
    if (!((win.x + d0) + s <= twe0)) bits |= CO_ST_MT_DEPOT_RETURN;
  }
  if (!range) {
    const bool op = open[b] != 0;
    float t = 0.f, len = 0.f, ul = 0.f, ub = 0.f;
    float2 prev = dep;
    for (int64_t k = 0; k < T; ++k) {
      const int64_t a = actions[b * sb + k * st];
      const float2 q = lr[a], win = tw[row + a];
      const float d = mt_dist(prev.x, prev.y, q.x, q.y);
      len = len + d * ((op && a == 0) ? 0.0f : 1.0f);
      if (!(len <= lim)) bits |= CO_ST_MT_ROUTE_LIMIT;
      if (a == 0) len = 0.f;
      t = mt_max(t + d, win.x);
      if (!(t <= win.y)) bits |= CO_ST_MT_DEADLINE;
      t = t + svc[row + a];
      if (a == 0) t = 0.f;
      const float m01 = a != 0 ? 1.0f : 0.0f;
      ul = ul * m01 + dl[row + a];
      ub = ub * m01 + db[row + a];
      if (!(ul <= vc)) bits |= CO_ST_MT_OVER_LINEHAUL;
      if (!(ub <= vc)) bits |= CO_ST_MT_OVER_BACKHAUL;
      prev = q;
    }
  }
  if (bits) set_status(status, bits);
}

inline bool mt_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N > 0 && N <= CO_MTVRP_MAX_N; }
inline bool mt_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

// the per-instance inputs every rows entry takes
inline bool mt_instance(MtArgs& a, const co_mtvrp_instance* in) {
  if (!in || !in->locs || !in->time_windows || !in->service_time || !in->demand_linehaul ||
      !in->demand_backhaul || !in->vehicle_capacity || !in->speed || !in->distance_limit ||
      !in->open_route)
    return false;
  a.locs = reinterpret_cast<const float2*>(in->locs);
  a.tw = reinterpret_cast<const float2*>(in->time_windows);
  a.svc = in->service_time, a.dl = in->demand_linehaul, a.db = in->demand_backhaul;
  a.cap = in->vehicle_capacity, a.speed = in->speed, a.limit = in->distance_limit;
  a.open = in->open_route;
  return true;
}
inline bool mt_misaligned(const MtArgs& a) { return mt_mis8(a.locs) || mt_mis8(a.tw); }

}  // namespace

extern "C" int co_mtvrp_reset(int64_t B, int64_t N, const co_mtvrp_instance* in, int64_t* cur, float* time, float* route_len,
                              float* used_l, float* used_b, uint8_t* visited, uint8_t* mask,
                              void* stream) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  MtArgs a{};
  if (!mt_instance(a, in)) return CO_E_INVAL;
  if (!cur || !time || !route_len || !used_l || !used_b || !visited || !mask) return CO_E_INVAL;
  if (mt_misaligned(a)) return CO_E_ALIGN;
  a.B = B, a.N = (int)N, a.T = 0, a.fresh = 1;
  a.cur_out = cur, a.t_out = time, a.len_out = route_len, a.ul_out = used_l, a.ub_out = used_b;
  a.vis_out = visited, a.mask = mask;
  return mt_launch(a, stream);
}

extern "C" int co_mtvrp_step(int64_t B, int64_t N, const int64_t* action, const co_mtvrp_instance* in, const int64_t* cur_in, const float* t_in,
                             const float* len_in, const float* ul_in, const float* ub_in,
                             const uint8_t* vis_in, int64_t* cur_out, float* t_out,
                             float* len_out, float* ul_out, float* ub_out, uint8_t* vis_out,
                             uint8_t* done, float* reward, uint8_t* mask, int32_t* status,
                             int32_t* not_done, void* stream) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  MtArgs a{};
  if (!mt_instance(a, in)) return CO_E_INVAL;
  if (!action || !cur_in || !t_in || !len_in || !ul_in || !ub_in || !vis_in || !cur_out ||
      !t_out || !len_out || !ul_out || !ub_out || !vis_out || !done || !reward || !mask)
    return CO_E_INVAL;
  if (mt_misaligned(a)) return CO_E_ALIGN;
  a.B = B, a.N = (int)N, a.T = 1;
  a.actions = action, a.st = 0, a.sb = 1;
  a.cur_in = cur_in, a.t_in = t_in, a.len_in = len_in, a.ul_in = ul_in, a.ub_in = ub_in;
  a.vis_in = vis_in, a.cur_out = cur_out, a.t_out = t_out, a.len_out = len_out;
  a.ul_out = ul_out, a.ub_out = ub_out, a.vis_out = vis_out;
  a.done = done, a.reward = reward, a.mask = mask, a.status = status, a.not_done = not_done;
  return mt_launch(a, stream);
}

extern "C" int co_mtvrp_action_mask(int64_t B, int64_t N, const co_mtvrp_instance* in, const int64_t* cur, const float* time,
                                    const float* route_len, const float* used_l,
                                    const float* used_b, const uint8_t* visited, uint8_t* mask,
                                    void* stream) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  MtArgs a{};
  if (!mt_instance(a, in)) return CO_E_INVAL;
  if (!cur || !time || !route_len || !used_l || !used_b || !visited || !mask) return CO_E_INVAL;
  if (mt_misaligned(a)) return CO_E_ALIGN;
  a.B = B, a.N = (int)N, a.T = 0;
  a.cur_in = cur, a.t_in = time, a.len_in = route_len, a.ul_in = used_l, a.ub_in = used_b;
  a.vis_in = visited, a.mask = mask;
  return mt_launch(a, stream);
}

extern "C" int co_mtvrp_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                              int64_t st, int64_t sb, const co_mtvrp_instance* in, int64_t* cur, float* time_io,
                              float* route_len, float* used_l, float* used_b, uint8_t* visited,
                              uint8_t* done, float* reward, uint8_t* mask, uint8_t* feasible,
                              float* time, float* rlen, int32_t* status, int32_t* not_done,
                              void* stream) {
  if (!mt_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  MtArgs a{};
  if (!mt_instance(a, in)) return CO_E_INVAL;
  if (!actions || !cur || !time_io || !route_len || !used_l || !used_b || !visited || !done ||
      !reward || !mask)
    return CO_E_INVAL;
  if (mt_misaligned(a)) return CO_E_ALIGN;
  a.B = B, a.N = (int)N, a.T = (int)T;
  a.actions = actions, a.st = st, a.sb = sb;
  a.cur_in = cur, a.cur_out = cur, a.t_in = time_io, a.t_out = time_io;
  a.len_in = route_len, a.len_out = route_len, a.ul_in = used_l, a.ul_out = used_l;
  a.ub_in = used_b, a.ub_out = used_b, a.vis_in = visited, a.vis_out = visited;
  a.done = done, a.reward = reward, a.mask = mask;
  a.feasible = feasible, a.time = time, a.rlen = rlen;
  a.status = status, a.not_done = not_done;
  return mt_launch(a, stream);
}

extern "C" int co_mtvrp_reward(int64_t B, int64_t N, int64_t T, const float* locs,
                               const int64_t* actions, int64_t sb, int64_t st,
                               const uint8_t* open, float* reward, int32_t* status,
                               void* stream) {
  if (!mt_sizes_ok(B, N) || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || (T > 0 && !actions) || !open || !reward) return CO_E_INVAL;
  if (mt_mis8(locs)) return CO_E_ALIGN;
  const unsigned grid = cover_grid(B, 256);
  if (grid == 0) return CO_E_INVAL;
  hipLaunchKernelGGL(mtvrp_reward_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, B,
                     (int)N, T, reinterpret_cast<const float2*>(locs), actions, sb, st, open,
                     reward, status);
  return launch_status();
}

extern "C" int co_mtvrp_check(int64_t B, int64_t N, int64_t T, const co_mtvrp_instance* in,
                              const int64_t* actions, int64_t sb, int64_t st, int32_t* status,
                              void* stream) {
  if (!mt_sizes_ok(B, N) || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!in || !in->locs || (T > 0 && !actions) || !in->time_windows || !in->service_time ||
      !in->demand_linehaul || !in->demand_backhaul || !in->vehicle_capacity ||
      !in->distance_limit || !in->open_route || !status)
    return CO_E_INVAL;
  if (mt_mis8(in->locs) || mt_mis8(in->time_windows)) return CO_E_ALIGN;
  const unsigned grid = cover_grid(B, kMtCheckThreads, kMtCheckThreads);
  if (grid == 0) return CO_E_INVAL;
  const size_t shmem = sizeof(uint32_t) * kMtCheckThreads * (size_t)((N + 32) >> 5);
  hipLaunchKernelGGL(mtvrp_check_kernel, dim3(grid), dim3(kMtCheckThreads), shmem,
                     (hipStream_t)stream, B, (int)N, T,
                     reinterpret_cast<const float2*>(in->locs), actions, sb, st,
                     reinterpret_cast<const float2*>(in->time_windows), in->service_time,
                     in->demand_linehaul, in->demand_backhaul, in->vehicle_capacity,
                     in->distance_limit, in->open_route, status);
  return launch_status();
}
