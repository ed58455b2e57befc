// Host (CPU) build of the env step / mask / reward / decode entry points of
// include/co_env.h, for TensorDicts that live on the CPU (BASELINE config 1: the
// reference's CPU TensorDict path, tsp/env.py:95-120 allocating on td.device).
//
// Same C ABI and the same semantics as the gfx950 kernels (every function below cites
// the reference lines it restates; the header documents the contract), plain host
// pointers, the trailing `stream` argument ignored.  Data-dependent failures are OR-ed
// into *status exactly as on the device.  Single-threaded, reentrant, no allocation
// beyond per-call row scratch, no global state.  Built by g++ (rl4co_slap_amd/csrc/
// build.py, -ffp-contract=off, no fast-math); tests/test_host_asan.py rebuilds it with
// -fsanitize=address,undefined and runs its indexing paths.
//
// Decode math is ATen's CPU log_softmax evaluation: SLEEF expf_u10 / logf_u1 (FMA
// variants) and vec::map_reduce_all's 16-lane summation order, the same restatement as
// csrc/co_math.hpp; tanh clipping is the correctly rounded tanh (f64 evaluation, one
// rounding), as on the device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/co_env.h"

#define CO_HOST_API extern "C" __attribute__((visibility("default")))

namespace {

inline void set_status(int32_t* status, int32_t bits) {
  if (status) *status |= bits;
}

inline float edge_len(float x0, float y0, float x1, float y1) {
  const float dx = x1 - x0, dy = y1 - y0;
  return std::sqrt(dx * dx + dy * dy);  // torch.norm(p=2) over 2 elements, no FMA
}

// ---- what the three local searches' entry points share (the searches themselves do not)
inline int64_t ls_clamp_iterations(int64_t max_iterations) {
  return max_iterations > INT32_MAX ? INT32_MAX : max_iterations;
}

// the batch (B == 0 is CO_OK: the caller returns), exactly one distance source and the
// entry point's other required pointers
inline int ls_check_args(int64_t B, int64_t LB, const float* locs, const float* distances,
                         bool others_given) {
  if (B < 0 || LB <= 0 || (B > 0 && B % LB != 0)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if ((locs == nullptr) == (distances == nullptr) || !others_given) return CO_E_INVAL;
  return CO_OK;
}

// D[a][c] of instance `inst` of V nodes: its matrix when one is given, else from its
// coordinates
struct LsDist {
  const float *lr, *dm;
  int64_t V;
  LsDist(const float* locs, const float* distances, int64_t inst, int64_t V_)
      : lr(locs ? locs + inst * V_ * 2 : nullptr),
        dm(distances ? distances + inst * V_ * V_ : nullptr), V(V_) {}
  float operator()(int64_t a, int64_t c) const {
    return dm ? dm[a * V + c] : edge_len(lr[2 * a], lr[2 * a + 1], lr[2 * c], lr[2 * c + 1]);
  }
};

// ---- SLEEF xexpf (u10, FMA) / xlogf_u1 (FMA), as ATen's vectorised CPU kernels call them
float aten_expf(float d) {
  const float qf = std::nearbyint(d * 1.442695040888963407359924681001892137426645954152985934135449406931f);
  const int q = (int)qf;
  float s = std::fma(qf, -0.693145751953125f, d);
  s = std::fma(qf, -1.428606765330187045e-06f, s);
  float u = 0.000198527617612853646278381f;
  u = std::fma(u, s, 0.00139304355252534151077271f);
  u = std::fma(u, s, 0.00833336077630519866943359f);
  u = std::fma(u, s, 0.0416664853692054748535156f);
  u = std::fma(u, s, 0.166666671633720397949219f);
  u = std::fma(u, s, 0.5f);
  u = 1.0f + std::fma(s * s, u, s);
  u = std::ldexp(u, q);  // one rounding: both halves of SLEEF's vldexp2 are normal
  if (d < -104.f) u = 0.f;
  if (100.f < d) u = INFINITY;
  return u;
}

float aten_logf(float d) {
  const float dd = d * (1.0f / 0.75f);
  uint32_t bits;
  std::memcpy(&bits, &dd, 4);
  const int e = (int)((bits >> 23) & 0xffu) - 127;
  const float m = std::ldexp(d, -e);
  const float ef = (float)e;
  float sx = 0.69314718246459960938f * ef;
  float sy = std::fma(-1.904654323148236017e-09f, ef, std::fma(0.69314718246459960938f, ef, -sx));
  const float nx = -1.0f + m;
  float ny;
  {
    const float v = nx - -1.0f;
    ny = (-1.0f - (nx - v)) + (m - v);
  }
  const float qx = 1.0f + m;
  float qy;
  {
    const float v = qx - 1.0f;
    qy = (1.0f - (qx - v)) + (m - v);
  }
  float xx, xy;
  {
    const float t = 1.0f / qx;
    xx = nx * t;
    const float u = std::fma(t, nx, -xx);
    const float v = std::fma(-qy, t, std::fma(-qx, t, 1.0f));
    xy = std::fma(xx, v, std::fma(ny, t, u));
  }
  const float x2 = xx * xx;
  float t = +0.3027294874e+0f;
  t = std::fma(t, x2, +0.3996108174e+0f);
  t = std::fma(t, x2, +0.6666694880e+0f);
  {
    const float s2 = sx + xx * 2.0f;
    sy = (((sx - s2) + xx * 2.0f) + sy) + xy * 2.0f;
    sx = s2;
  }
  {
    const float w = (x2 * xx) * t;
    const float s2 = sx + w;
    sy = ((sx - s2) + w) + sy;
    sx = s2;
  }
  float r = sx + sy;
  if (d == INFINITY) r = INFINITY;
  if (d < 0.f || d != d) r = NAN;
  if (d == 0.f) r = -INFINITY;
  return r;
}

// correctly rounded tanh (up to f64 double rounding): one rounding of the f64 tanh
float tanh_cr(float x) { return (float)std::tanh((double)x); }

// vec::map_reduce_all's exp-sum order (AVX512: 16 accumulators, then the xor-8/4/2/1
// butterfly); rows narrower than 16 are summed left to right
float aten_row_sum(const float* e, int n) {
  if (n < 16) {
    float s = e[0];
    for (int c = 1; c < n; ++c) s += e[c];
    return s;
  }
  float acc[16];
  for (int r = 0; r < 16; ++r) acc[r] = e[r];
  int c = 16;
  for (; c + 16 <= n; c += 16)
    for (int r = 0; r < 16; ++r) acc[r] += e[c + r];
  for (int r = 0; c + r < n; ++r) acc[r] += e[c + r];  // the tail vector (zero padded)
  for (int h = 8; h >= 1; h >>= 1)
    for (int r = 0; r < h; ++r) acc[r] += acc[r + h];
  return acc[0];
}

// torch.argmax ordering: NaN beats everything, equal values keep the lower index
inline bool argmax_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}

// Philox-4x32-10 (Salmon et al. 2011), counter (offset, row): the device's draw
uint32_t philox_u32(uint64_t seed, uint64_t offset, uint64_t row) {
  uint32_t c0 = (uint32_t)offset, c1 = (uint32_t)(offset >> 32), c2 = (uint32_t)row,
           c3 = (uint32_t)(row >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

}  // namespace

// ---------------------------------------------------------------------------- TSP
// tsp/env.py:95-120
CO_HOST_API int co_tsp_reset(int64_t B, int64_t N, uint8_t* mask, int64_t* first, int64_t* cur,
                             int64_t* i, float* reward, void*) {
  if (B < 0 || N <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mask || !first || !cur || !i || !reward) return CO_E_INVAL;
  std::memset(mask, 1, (size_t)(B * N));
  for (int64_t b = 0; b < B; ++b) {
    first[b] = 0;
    cur[b] = 0;
    i[b] = 0;
    reward[b] = 0.f;
  }
  return CO_OK;
}

// tsp/env.py:67-93
CO_HOST_API int co_tsp_step(int64_t B, int64_t N, const int64_t* action, const uint8_t* mask_in,
                            uint8_t* mask_out, const int64_t* i_in, int64_t* i_out,
                            const int64_t* first_in, int64_t* first_out, int64_t* current_out,
                            uint8_t* done, uint8_t* reward, int first_mode,
                            const int32_t* first_flag, int32_t* status, void*) {
  if (B < 0 || N <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !mask_in || !mask_out || !i_in || !i_out || !first_out || !done || !reward)
    return CO_E_INVAL;
  if (first_mode == 2 && !first_flag) return CO_E_INVAL;
  if (first_mode == 0 && !first_in) return CO_E_INVAL;
  const bool take = first_mode == 1 || (first_mode == 2 && *first_flag != 0);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t a = action[b];
    const uint8_t* mi = mask_in + b * N;
    uint8_t* mo = mask_out + b * N;
    if (mo != mi) std::memcpy(mo, mi, (size_t)N);
    if (a < 0 || a >= N)
      set_status(status, CO_ST_INDEX_RANGE);  // torch.scatter raises; nothing cleared
    else
      mo[a] = 0;
    int64_t left = 0;
    for (int64_t c = 0; c < N; ++c) left += mo[c] != 0;
    const int64_t f = take ? a : first_in[b];
    first_out[b] = f;
    i_out[b] = i_in[b] + 1;
    if (current_out) current_out[b] = a;
    done[b] = left == 0;
    reward[b] = 0;
  }
  return CO_OK;
}

// envs/common/base.py:182-188 + tsp/env.py:157-173 (validity: sorted row == arange(T))
CO_HOST_API int co_tsp_reward(int64_t B, int64_t N, int64_t T, const float* locs, int64_t LB,
                              const int64_t* actions, int64_t sb, int64_t st, int check,
                              float* reward, int32_t* status, void*) {
  if (B < 0 || N <= 0 || T <= 0 || T > (1 << 24)) return CO_E_INVAL;
  if (LB <= 0 || (B > 0 && B % LB != 0)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !reward || (check && !status)) return CO_E_INVAL;
  std::vector<uint8_t> seen(check ? (size_t)T : 0);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + (b % LB) * N * 2;
    const int64_t* ar = actions + b * sb;
    bool bad = false;
    if (check) std::fill(seen.begin(), seen.end(), 0);
    double len = 0.0;
    int64_t prev = -1, first = -1;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = ar[t * st];
      if (a < 0 || a >= N) {
        set_status(status, CO_ST_INDEX_RANGE);
        bad = true;
        prev = -1;
        continue;
      }
      if (check) {
        if (a >= T || seen[a]) bad = true;
        else seen[a] = 1;
      }
      if (t == 0) first = a;
      if (prev >= 0) len += edge_len(lr[2 * prev], lr[2 * prev + 1], lr[2 * a], lr[2 * a + 1]);
      prev = a;
    }
    if (prev >= 0 && first >= 0)  // closing edge (roll by -1)
      len += edge_len(lr[2 * prev], lr[2 * prev + 1], lr[2 * first], lr[2 * first + 1]);
    reward[b] = -(float)len;
    if (check && bad) set_status(status, CO_ST_INVALID_TOUR);
  }
  return CO_OK;
}

// tsp/env.py:192-197 -> tsp/local_search.py:14-74: best-improvement 2-opt, the reference's
// scalar double loop per row (one move per sweep; strict `<` from delta = 0 in ascending
// (i, j) order, so equal changes keep the first; the -1e-6 tests in double): the descent
// below with the 2-opt neighbourhood alone.  The reference skips a move when
// `prev == tour[j] || next == tour[i]`; on a permutation with 1 <= i < j <= n-1 that never
// holds, so the shared loop has no such test.
CO_HOST_API int co_tsp_two_opt(int64_t B, int64_t N, const float* locs, const float* distances,
                               int64_t LB, const int64_t* actions, int64_t sb, int64_t st,
                               int64_t max_iterations, int64_t* actions_out,
                               int32_t* sweeps_out, int32_t* status, void* stream) {
  return co_tsp_local_search(B, N, locs, distances, LB, actions, sb, st, max_iterations,
                             CO_TSP_LS_TWO_OPT, actions_out, sweeps_out, nullptr, status, stream);
}

// The 2-opt + Or-opt descent of include/co_env.h, as plain loops in the header's
// enumeration order (2-opt: i, j; Or-opt: L, i, k, rev) with a strict `<` from 0, so equal
// changes keep the first; every change is the header's left-to-right f32 expression.
CO_HOST_API int co_tsp_local_search(int64_t B, int64_t N, const float* locs,
                                    const float* distances, int64_t LB, const int64_t* actions,
                                    int64_t sb, int64_t st, int64_t max_iterations,
                                    int operators, int64_t* actions_out, int32_t* sweeps_out,
                                    int32_t* moves_out, int32_t* status, void*) {
  if (N <= 0 || N > CO_TWO_OPT_MAX_N) return CO_E_INVAL;
  if (operators <= 0 || (operators & ~(CO_TSP_LS_TWO_OPT | CO_TSP_LS_OR_OPT))) return CO_E_INVAL;
  const int rc = ls_check_args(B, LB, locs, distances,
                               actions && actions_out && actions_out != actions && status);
  if (rc != CO_OK || B == 0) return rc;
  const int64_t n = N;
  const int64_t max_it = ls_clamp_iterations(max_iterations);
  std::vector<int64_t> tour((size_t)n), seg;
  std::vector<uint8_t> seen((size_t)n);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* ar = actions + b * sb;
    int64_t* out = actions_out + b * n;
    std::fill(seen.begin(), seen.end(), 0);
    bool bad = false;
    for (int64_t k = 0; k < n; ++k) {
      const int64_t a = ar[k * st];
      out[k] = a;
      tour[(size_t)k] = a;
      if (a < 0 || a >= n || seen[(size_t)a]) bad = true;
      else seen[(size_t)a] = 1;
    }
    if (sweeps_out) sweeps_out[b] = 0;
    if (moves_out) moves_out[2 * b] = moves_out[2 * b + 1] = 0;
    if (bad) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    const LsDist D(locs, distances, b % LB, n);
    auto t = [&](int64_t k) { return tour[(size_t)(k >= n ? k - n : k)]; };  // cyclic
    int64_t it = 0;
    int32_t n_two = 0, n_or = 0;
    while (it < max_it) {
      ++it;
      if (operators & CO_TSP_LS_TWO_OPT) {
        int64_t p = 0, q = 0;
        float delta = 0.f;
        for (int64_t i = 1; i < n - 1; ++i)
          for (int64_t j = i + 1; j < n; ++j) {
            const int64_t prev = t(i - 1), next = t(j + 1), ti = t(i), tj = t(j);
            const float change = ((D(prev, tj) + D(ti, next)) - D(prev, ti)) - D(tj, next);
            if (change < delta) {
              p = i;
              q = j;
              delta = change;
            }
          }
        if ((double)delta < -1e-6) {
          std::reverse(tour.begin() + p, tour.begin() + q + 1);
          ++n_two;
          continue;
        }
      }
      if (!(operators & CO_TSP_LS_OR_OPT)) break;
      int64_t bl = 0, bi = 0, bk = 0, brev = 0;
      float delta = 0.f;
      for (int64_t L = 1; L <= 3; ++L) {
        if (n - L - 1 < 1) continue;
        for (int64_t i = 1; i + L - 1 <= n - 1; ++i) {
          const int64_t a = t(i - 1), s1 = t(i), s2 = t(i + L - 1), nb = t(i + L);
          for (int64_t k = 0; k < n; ++k) {
            if (k >= i - 1 && k <= i + L - 1) continue;
            const int64_t c = t(k), d = t(k + 1);
            for (int64_t rev = 0; rev < (L > 1 ? 2 : 1); ++rev) {
              const int64_t x = rev ? s2 : s1, y = rev ? s1 : s2;
              const float change =
                  ((((D(a, nb) + D(c, x)) + D(y, d)) - D(a, s1)) - D(s2, nb)) - D(c, d);
              if (change < delta) {
                bl = L;
                bi = i;
                bk = k;
                brev = rev;
                delta = change;
              }
            }
          }
        }
      }
      if (!((double)delta < -1e-6)) break;
      // take the segment out, then put it back (reversed if asked) directly after node c
      const int64_t c = t(bk);
      seg.assign(tour.begin() + bi, tour.begin() + bi + bl);
      if (brev) std::reverse(seg.begin(), seg.end());
      tour.erase(tour.begin() + bi, tour.begin() + bi + bl);
      const auto at = std::find(tour.begin(), tour.end(), c);
      tour.insert(at + 1, seg.begin(), seg.end());
      ++n_or;
    }
    for (int64_t k = 0; k < n; ++k) out[k] = tour[(size_t)k];
    if (sweeps_out) sweeps_out[b] = (int32_t)it;
    if (moves_out) {
      moves_out[2 * b] = n_two;
      moves_out[2 * b + 1] = n_or;
    }
  }
  return CO_OK;
}

CO_HOST_API int co_any_eq_i64(const int64_t* x, int64_t n, int64_t value, int32_t* flag, void*) {
  if (n < 0 || !flag || (n > 0 && !x)) return CO_E_INVAL;
  int32_t f = 0;
  for (int64_t k = 0; k < n; ++k) f |= x[k] == value;
  *flag = f;
  return CO_OK;
}

// ---------------------------------------------------------------------------- CVRP
namespace {
// co_cvrp_local_search's state of one row: the giant tour and, per position k, the load of
// k's route up to and including k (head), from k to the route's end (tail; tail[m] = 0) and
// the last zero at or before k (pz).  With these every admissibility test is O(1).
struct GiantTour {
  int64_t m = 0;
  std::vector<int64_t> g, q, head, tail, pz;  // q: quantised demand of node id
  void rebuild() {
    head.assign((size_t)m + 1, 0);
    tail.assign((size_t)m + 1, 0);
    pz.assign((size_t)m + 1, 0);
    for (int64_t k = 1; k < m; ++k) {
      const bool z = g[(size_t)k] == 0;
      head[(size_t)k] = z ? 0 : head[(size_t)k - 1] + q[(size_t)g[(size_t)k]];
      pz[(size_t)k] = z ? k : pz[(size_t)k - 1];
    }
    for (int64_t k = m - 1; k >= 1; --k)
      tail[(size_t)k] = g[(size_t)k] == 0 ? 0 : tail[(size_t)k + 1] + q[(size_t)g[(size_t)k]];
  }
  int64_t at(int64_t k) const { return g[(size_t)(k >= m ? k - m : k)]; }  // cyclic
};

inline bool cvrp_ls_scalar_ok(float x) { return std::isfinite(x) && x >= 0.f && x <= 4096.f; }
inline int64_t cvrp_ls_q(float x) { return std::llrint((double)x * 1099511627776.0); }  // 2^40

// cvrp/env.py:137-149: mask_loc = visited[1:] | (demand + used > capacity);
// depot feasible unless (current == 0 and some customer is feasible)
void cvrp_mask_row(int64_t N, const float* dem, float used, float cap, const uint8_t* vis,
                   int64_t cur, uint8_t* mask) {
  bool any = false;
  for (int64_t c = 1; c <= N; ++c) {
    const bool masked = vis[c] != 0 || (dem[c - 1] + used > cap);
    mask[c] = !masked;
    any |= !masked;
  }
  mask[0] = !((cur == 0) && any);
}
}  // namespace

// cvrp/env.py:107-135
CO_HOST_API int co_cvrp_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                              const float* demand, float vcap, float* locs_out, int64_t* cur,
                              float* used, float* vcap_out, uint8_t* visited, uint8_t* mask,
                              void*) {
  if (B < 0 || N <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !demand || !locs_out || !cur || !used || !vcap_out || !visited ||
      !mask)
    return CO_E_INVAL;
  for (int64_t b = 0; b < B; ++b) {
    float* lo = locs_out + b * (N + 1) * 2;
    lo[0] = depot[2 * b];
    lo[1] = depot[2 * b + 1];
    std::memcpy(lo + 2, locs_in + b * N * 2, sizeof(float) * 2 * (size_t)N);
    uint8_t* vr = visited + b * (N + 1);
    std::memset(vr, 0, (size_t)(N + 1));
    cur[b] = 0;
    used[b] = 0.f;
    vcap_out[b] = vcap;
    cvrp_mask_row(N, demand + b * N, 0.f, vcap, vr, 0, mask + b * (N + 1));
  }
  return CO_OK;
}

// cvrp/env.py:73-105 (+ get_action_mask)
CO_HOST_API int co_cvrp_step(int64_t B, int64_t N, const int64_t* action, const float* demand,
                             const float* used_in, float* used_out, const float* vcap,
                             const uint8_t* vis_in, uint8_t* vis_out, int64_t* cur_out,
                             uint8_t* done, uint8_t* reward, uint8_t* mask, int32_t* status,
                             int32_t* not_done, void*) {
  if (B < 0 || N <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !demand || !used_in || !used_out || !vcap || !vis_in || !vis_out || !done ||
      !reward || !mask)
    return CO_E_INVAL;
  int32_t left_all = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t a = action[b];
    const bool bad = a < 0 || a > N;
    if (bad) set_status(status, CO_ST_INDEX_RANGE);
    const float* dem = demand + b * N;
    int64_t di = a - 1;
    di = di < 0 ? 0 : (di > N - 1 ? N - 1 : di);
    const float u = (used_in[b] + dem[di]) * ((a != 0) ? 1.0f : 0.0f);  // env.py:83-85
    const uint8_t* vi = vis_in + b * (N + 1);
    uint8_t* vo = vis_out + b * (N + 1);
    if (vo != vi) std::memcpy(vo, vi, (size_t)(N + 1));
    if (!bad) vo[a] = 1;
    int64_t vsum = 0;
    for (int64_t c = 0; c <= N; ++c) vsum += vo[c];
    used_out[b] = u;
    if (cur_out) cur_out[b] = a;
    done[b] = vsum == N + 1;
    left_all += vsum != N + 1;
    reward[b] = 0;
    cvrp_mask_row(N, dem, u, vcap[b], vo, a, mask + b * (N + 1));
  }
  if (not_done) *not_done += left_all;
  return CO_OK;
}

CO_HOST_API int co_cvrp_action_mask(int64_t B, int64_t N, const float* demand, const float* used,
                                    const float* vcap, const uint8_t* visited, const int64_t* cur,
                                    uint8_t* mask, void*) {
  if (B < 0 || N <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!demand || !used || !vcap || !visited || !cur || !mask) return CO_E_INVAL;
  for (int64_t b = 0; b < B; ++b)
    cvrp_mask_row(N, demand + b * N, used[b], vcap[b], visited + b * (N + 1), cur[b],
                  mask + b * (N + 1));
  return CO_OK;
}

// cvrp/env.py:151-190: reward over [depot] + locs[actions] (closed), validity (sorted tail
// == 1..N, zeros before) and the sequential f32 capacity scan
CO_HOST_API int co_cvrp_reward(int64_t B, int64_t N, int64_t T, const float* locs,
                               const int64_t* actions, int64_t sb, int64_t st,
                               const float* demand, const float* vcap, int check, float* reward,
                               int32_t* status, void*) {
  if (B < 0 || N <= 0 || T <= 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !reward) return CO_E_INVAL;
  if (check && (!demand || !vcap || !status)) return CO_E_INVAL;
  std::vector<uint8_t> seen(check ? (size_t)(N + 1) : 0);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + b * (N + 1) * 2;
    const int64_t* ar = actions + b * sb;
    double len = 0.0;
    int64_t prev = 0;  // the depot
    bool prev_ok = true, range = false, bad = false;
    int64_t nonzero = 0;
    if (check) std::fill(seen.begin(), seen.end(), 0);
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = ar[t * st];
      const bool ok = a >= 0 && a <= N;
      if (!ok) {
        range = true;
        bad = true;
        prev_ok = false;
        continue;
      }
      if (prev_ok)
        len += edge_len(lr[2 * prev], lr[2 * prev + 1], lr[2 * a], lr[2 * a + 1]);
      if (check && a != 0) {
        ++nonzero;
        if (seen[a]) bad = true;
        seen[a] = 1;
      }
      prev = a;
      prev_ok = true;
    }
    if (prev_ok) len += edge_len(lr[2 * prev], lr[2 * prev + 1], lr[0], lr[1]);
    reward[b] = -(float)len;
    if (range) set_status(status, CO_ST_INDEX_RANGE);
    if (!check) continue;
    if (bad || nonzero != N) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    const float cap = vcap[b], lim = cap + 1e-5f;
    float used = 0.f;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = ar[t * st];
      used += a == 0 ? -cap : demand[b * N + a - 1];
      if (used < 0.f) used = 0.f;
      if (!(used <= lim)) {
        set_status(status, CO_ST_OVER_CAPACITY);
        break;
      }
    }
  }
  return CO_OK;
}

// Giant-tour 2-opt + relocate (no reference counterpart that can be reproduced: cvrp/
// local_search.py hands the instance to PyVRP).  The header states the search; this is its
// plain scalar form: candidates in tie order (2-opt, then relocate; i, then j ascending)
// against a strict `<` from 0, so equal changes keep the first.
CO_HOST_API int co_cvrp_local_search(int64_t B, int64_t N, int64_t T, const float* locs,
                                     const float* distances, const float* demand,
                                     const float* capacity, int64_t LB, const int64_t* actions,
                                     int64_t sb, int64_t st, int64_t max_iterations,
                                     int64_t* actions_out, int32_t* sweeps_out, int32_t* status,
                                     void*) {
  if (N < 1 || T < N) return CO_E_INVAL;
  if ((T < 2 * N ? T : 2 * N) + 1 > CO_CVRP_LS_MAX_LEN) return CO_E_INVAL;
  const int rc = ls_check_args(
      B, LB, locs, distances, demand && actions && actions_out && actions_out != actions && status);
  if (rc != CO_OK || B == 0) return rc;
  const int64_t V = N + 1;  // nodes, depot first
  const int64_t max_it = ls_clamp_iterations(max_iterations);
  GiantTour gt;
  gt.q.assign((size_t)V, 0);
  std::vector<uint8_t> seen((size_t)V);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* ar = actions + b * sb;
    int64_t* out = actions_out + b * T;
    const int64_t inst = b % LB;
    const float* dr = demand + inst * N;
    const float cap = capacity ? capacity[inst] : 1.0f;
    std::fill(seen.begin(), seen.end(), 0);
    bool bad = !cvrp_ls_scalar_ok(cap);
    int64_t customers = 0;
    gt.g.assign(1, 0);
    for (int64_t k = 0; k < T; ++k) {
      const int64_t a = ar[k * st];
      out[k] = a;
      if (a < 0 || a > N || (a > 0 && seen[(size_t)a])) {
        bad = true;
        continue;
      }
      seen[(size_t)a] = 1;
      customers += a > 0;
      if (a != 0 || gt.g.back() != 0) gt.g.push_back(a);
    }
    for (int64_t c = 0; c < N; ++c) {
      if (!cvrp_ls_scalar_ok(dr[c])) bad = true;
      else gt.q[(size_t)c + 1] = cvrp_ls_q(dr[c]);
    }
    if (sweeps_out) sweeps_out[b] = 0;
    if (bad || customers != N) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    if (gt.g.size() > 1 && gt.g.back() == 0) gt.g.pop_back();
    const int64_t m = gt.m = (int64_t)gt.g.size();
    const int64_t cap_q = cvrp_ls_q(cap) + (int64_t(1) << 20);
    const LsDist D(locs, distances, inst, V);
    std::vector<int64_t>& g = gt.g;
    int64_t it = 0;
    while (it < max_it) {
      ++it;
      gt.rebuild();
      float best = 0.f;
      int kind = -1;
      int64_t bi = 0, bj = 0;
      for (int64_t i = 1; i < m - 1; ++i)
        for (int64_t j = i + 1; j < m; ++j) {
          const int64_t p = g[(size_t)i - 1], x = g[(size_t)i], y = g[(size_t)j], n = gt.at(j + 1);
          const float change = ((D(p, y) + D(x, n)) - D(p, x)) - D(y, n);
          if (!(change < best)) continue;
          if (gt.pz[(size_t)j] >= i &&  // a depot inside: both new boundary routes must fit
              (gt.head[(size_t)i - 1] + gt.head[(size_t)j] > cap_q ||
               gt.tail[(size_t)i] + gt.tail[(size_t)j + 1] > cap_q))
            continue;
          best = change;
          kind = 0;
          bi = i;
          bj = j;
        }
      for (int64_t i = 1; i < m; ++i) {
        const int64_t c = g[(size_t)i];
        if (c == 0) continue;
        const int64_t p = g[(size_t)i - 1], n = gt.at(i + 1);
        const float gain = (D(p, n) - D(p, c)) - D(c, n);
        for (int64_t j = 0; j < m; ++j) {
          if (j == i || j == i - 1) continue;
          const int64_t a = g[(size_t)j], e = gt.at(j + 1);
          const float change = ((D(a, c) + D(c, e)) - D(a, e)) + gain;
          if (!(change < best)) continue;
          if (gt.pz[(size_t)j] != gt.pz[(size_t)i] &&  // another route: it must take c
              gt.head[(size_t)j] + gt.tail[(size_t)j + 1] + gt.q[(size_t)c] > cap_q)
            continue;
          best = change;
          kind = 1;
          bi = i;
          bj = j;
        }
      }
      if (kind < 0 || !((double)best < -1e-6)) break;
      if (kind == 0) std::reverse(g.begin() + bi, g.begin() + bj + 1);
      else if (bj > bi) std::rotate(g.begin() + bi, g.begin() + bi + 1, g.begin() + bj + 1);
      else std::rotate(g.begin() + bj + 1, g.begin() + bi, g.begin() + bi + 1);
    }
    int64_t w = 0;
    for (int64_t k = 1; k < m; ++k)
      if (g[(size_t)k] != 0 || (w > 0 && out[w - 1] != 0)) out[w++] = g[(size_t)k];
    for (; w < T; ++w) out[w] = 0;
    if (sweeps_out) sweeps_out[b] = (int32_t)it;
  }
  return CO_OK;
}

// ---------------------------------------------------------------------------- SLAP
// slap/env.py:95-129
CO_HOST_API int co_slap_reset(int64_t B, int64_t L, int64_t P, uint8_t* mask, float* to_choose,
                              int64_t* it, float* reward, float* ratio, uint8_t* done,
                              uint8_t* terminated, void*) {
  if (B < 0 || L <= 0 || P <= 0) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mask || !to_choose || !it || !reward) return CO_E_INVAL;
  for (int64_t b = 0; b < B; ++b) {
    for (int64_t l = 0; l < L; ++l) mask[b * L + l] = l != 0;
    for (int64_t p = 0; p < P; ++p) to_choose[b * P + p] = (float)p;
    if (ratio)
      for (int64_t l = 0; l < L; ++l) ratio[b * L + l] = 0.f;
    it[b] = 0;
    reward[b] = 0.f;
    if (done) done[b] = 0;
    if (terminated) terminated[b] = 0;
  }
  return CO_OK;
}

// slap/env.py:38-93 (negative indices wrap like python advanced indexing)
CO_HOST_API int co_slap_step(int64_t B, int64_t L, int64_t P, const int64_t* action,
                             const float* to_choose, int64_t tc_stride, const int32_t* assign_in,
                             int32_t* assign_out, const uint8_t* mask_in, uint8_t* mask_out,
                             const int64_t* i_in, int64_t* i_out, uint8_t* done, uint8_t* reward,
                             int32_t* status, void*) {
  if (B < 0 || L <= 0 || P <= 0 || L > (1 << 30)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !assign_in || !assign_out || !mask_in || !mask_out || !i_in || !i_out ||
      !done || !reward || (!to_choose && (tc_stride < 0 || tc_stride >= P)))
    return CO_E_INVAL;
  for (int64_t b = 0; b < B; ++b) {
    if (assign_out != assign_in)
      std::memcpy(assign_out + b * P, assign_in + b * P, sizeof(int32_t) * (size_t)P);
    if (mask_out != mask_in) std::memcpy(mask_out + b * L, mask_in + b * L, (size_t)L);
    int64_t a = action[b];
    if (a < 0) a += L;
    if (a < 0 || a >= L)
      set_status(status, CO_ST_INDEX_RANGE);
    else
      mask_out[b * L + a] = 0;
    // .to(torch.int), env.py:52; to_choose NULL: the uniform product tc_stride
    int64_t p = to_choose ? (int64_t)(int)to_choose[b * tc_stride] : tc_stride;
    if (p < 0) p += P;
    if (p < 0 || p >= P)
      set_status(status, CO_ST_INDEX_RANGE);
    else
      assign_out[b * P + p] = (int32_t)action[b];  // env.py:53-54
    done[b] = i_in[b] == P - 1;
    i_out[b] = i_in[b] + 1;
    reward[b] = 0;
  }
  return CO_OK;
}

// slap/env.py:131-143: orders added one by one in f32, each a closed tour in pick order
CO_HOST_API int co_slap_reward(int64_t B, int64_t L, int64_t P, int64_t O, int64_t K,
                               const int32_t* assignment, const int64_t* picklist,
                               const float* locs, float* reward, int32_t* status, void*) {
  if (B < 0 || L <= 0 || P <= 0 || O <= 0 || K <= 0 || O * K > (1 << 16)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!assignment || !picklist || !locs || !reward) return CO_E_INVAL;
  std::vector<int64_t> loc((size_t)K);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + b * L * 2;
    float total = 0.f;
    for (int64_t o = 0; o < O; ++o) {
      for (int64_t k = 0; k < K; ++k) {
        int64_t p = picklist[(b * O + o) * K + k];
        if (p < 0) p += P;
        int64_t l = 0;
        if (p < 0 || p >= P) {
          set_status(status, CO_ST_INDEX_RANGE);
        } else {
          l = assignment[b * P + p];
          if (l < 0) l += L;  // the -1 of an unassigned product wraps
          if (l < 0 || l >= L) {
            set_status(status, CO_ST_INDEX_RANGE);
            l = 0;
          }
        }
        loc[(size_t)k] = l;
      }
      float len = 0.f;
      for (int64_t k = 0; k < K; ++k) {
        const int64_t p0 = loc[(size_t)k], p1 = loc[(size_t)((k + 1) % K)];
        len += edge_len(lr[2 * p0], lr[2 * p0 + 1], lr[2 * p1], lr[2 * p1 + 1]);
      }
      total += -len;
    }
    reward[b] = total;
  }
  return CO_OK;
}

// Product swap + move-to-free-slot on the integer QAP objective (the reference has no SLAP
// local search).  The header states the search; this is its scalar form on the table
// C[p][l] = sum_r W[p][r] Q[l][s_r] + W[r][p] Q[s_r][l], updated after each applied move:
// candidates in tie order (moves, then swaps; p, then x or q ascending) against a strict
// `<` from 0, so equal changes keep the first.
CO_HOST_API int co_slap_local_search(int64_t B, int64_t L, int64_t P, int64_t O, int64_t K,
                                     const float* locs, const float* distances, int64_t LB,
                                     const int64_t* picklist, const int32_t* assignment,
                                     int64_t max_iterations, int32_t* assign_out,
                                     int32_t* sweeps_out, int64_t* cost_out, int32_t* status,
                                     void*) {
  if (P < 1 || P > CO_SLAP_LS_MAX_PRODUCTS || L < P || L > CO_SLAP_LS_MAX_SLOTS)
    return CO_E_INVAL;
  if (O < 1 || K < 1 || O > 65536 || K > 65536 || O * K > 65536) return CO_E_INVAL;
  const int rc = ls_check_args(
      B, LB, locs, distances,
      picklist && assignment && assign_out && assign_out != assignment && status);
  if (rc != CO_OK || B == 0) return rc;
  const int64_t max_it = ls_clamp_iterations(max_iterations);
  std::vector<int64_t> W((size_t)(P * P)), C((size_t)(P * L)), s((size_t)P), dcol((size_t)L),
      drow((size_t)L);
  std::vector<uint8_t> occ((size_t)L);
  for (int64_t b = 0; b < B; ++b) {
    const int32_t* ar = assignment + b * P;
    int32_t* out = assign_out + b * P;
    const int64_t inst = b % LB;
    const int64_t* pl = picklist + inst * O * K;
    const LsDist D(locs, distances, inst, L);
    const float *lr = D.lr, *dm = D.dm;
    bool bad = false, bad_pl = false;
    std::fill(occ.begin(), occ.end(), 0);
    for (int64_t p = 0; p < P; ++p) {
      const int64_t v = out[p] = ar[p];
      if (v < 0 || v >= L || occ[(size_t)v]) {
        bad = true;
        continue;
      }
      occ[(size_t)v] = 1;
      s[(size_t)p] = v;
    }
    std::fill(W.begin(), W.end(), 0);
    for (int64_t o = 0; o < O; ++o)
      for (int64_t k = 0; k < K; ++k) {
        const int64_t a = pl[o * K + k], c = pl[o * K + (k + 1) % K];
        if (a < 0 || a >= P) bad_pl = true;
        else if (c >= 0 && c < P && a != c) ++W[(size_t)(a * P + c)];
      }
    if (lr) {
      for (int64_t k = 0; k < 2 * L; ++k) bad |= !(std::fabs(lr[k]) <= 262144.f);
    } else {
      for (int64_t k = 0; k < L * L; ++k) bad |= !(dm[k] >= 0.f && dm[k] <= 1048576.f);
    }
    if (sweeps_out) sweeps_out[b] = 0;
    if (cost_out) cost_out[b] = -1;
    if (bad || bad_pl) {
      set_status(status, (bad ? CO_ST_INVALID_TOUR : 0) | (bad_pl ? CO_ST_INDEX_RANGE : 0));
      continue;
    }
    auto Q = [&](int64_t u, int64_t v) -> int64_t {
      return (int64_t)std::llrint((double)D(u, v) * 1048576.0);  // 2^20
    };
    for (int64_t p = 0; p < P; ++p)
      for (int64_t l = 0; l < L; ++l) {
        int64_t acc = 0;
        for (int64_t r = 0; r < P; ++r) {
          const int64_t w1 = W[(size_t)(p * P + r)], w2 = W[(size_t)(r * P + p)];
          if (w1) acc += w1 * Q(l, s[(size_t)r]);
          if (w2) acc += w2 * Q(s[(size_t)r], l);
        }
        C[(size_t)(p * L + l)] = acc;
      }
    int64_t it = 0;
    while (it < max_it) {
      ++it;
      int64_t best = 0, bp = 0, bx = 0;
      int kind = -1;
      for (int64_t p = 0; p < P; ++p) {
        const int64_t ca = C[(size_t)(p * L + s[(size_t)p])];
        for (int64_t x = 1; x < L; ++x) {
          if (occ[(size_t)x]) continue;
          const int64_t d = C[(size_t)(p * L + x)] - ca;
          if (d < best) best = d, kind = 0, bp = p, bx = x;
        }
      }
      for (int64_t p = 0; p < P; ++p)
        for (int64_t q = p + 1; q < P; ++q) {
          const int64_t a = s[(size_t)p], c = s[(size_t)q];
          int64_t d = (C[(size_t)(p * L + c)] - C[(size_t)(p * L + a)]) +
                      (C[(size_t)(q * L + a)] - C[(size_t)(q * L + c)]);
          const int64_t w = W[(size_t)(p * P + q)] + W[(size_t)(q * P + p)];
          if (w) d += w * (((Q(a, c) + Q(c, a)) - Q(a, a)) - Q(c, c));
          if (d < best) best = d, kind = 1, bp = p, bx = q;
        }
      if (kind < 0) break;
      const int64_t a = s[(size_t)bp], x = kind ? s[(size_t)bx] : bx;
      for (int64_t l = 0; l < L; ++l) {
        dcol[(size_t)l] = Q(l, x) - Q(l, a);
        drow[(size_t)l] = Q(x, l) - Q(a, l);
      }
      for (int64_t r = 0; r < P; ++r) {
        int64_t c1 = W[(size_t)(r * P + bp)], c2 = W[(size_t)(bp * P + r)];
        if (kind) c1 -= W[(size_t)(r * P + bx)], c2 -= W[(size_t)(bx * P + r)];
        if (c1 == 0 && c2 == 0) continue;
        for (int64_t l = 0; l < L; ++l)
          C[(size_t)(r * L + l)] += c1 * dcol[(size_t)l] + c2 * drow[(size_t)l];
      }
      s[(size_t)bp] = x;
      if (kind) s[(size_t)bx] = a;
      else occ[(size_t)a] = 0, occ[(size_t)x] = 1;
    }
    for (int64_t p = 0; p < P; ++p) out[p] = (int32_t)s[(size_t)p];
    if (sweeps_out) sweeps_out[b] = (int32_t)it;
    if (cost_out) {
      int64_t f = 0;
      for (int64_t a = 0; a < P; ++a)
        for (int64_t c = 0; c < P; ++c)
          if (W[(size_t)(a * P + c)]) f += W[(size_t)(a * P + c)] * Q(s[(size_t)a], s[(size_t)c]);
      cost_out[b] = f;
    }
  }
  return CO_OK;
}

// ---------------------------------------------------------------------------- ops
// utils/ops.py:65-77
CO_HOST_API int co_gather_by_index(const void* src, int64_t outer, int64_t src_len,
                                   int64_t inner_bytes, int64_t src_stride_outer,
                                   int64_t src_stride_len, const int64_t* idx, int64_t idx_len,
                                   int64_t idx_stride_outer, int64_t idx_stride_len, void* dst,
                                   int32_t* status, void*) {
  if (outer < 0 || src_len < 0 || inner_bytes <= 0 || idx_len < 0) return CO_E_INVAL;
  if (outer == 0 || idx_len == 0) return CO_OK;
  if (!src || !idx || !dst) return CO_E_INVAL;
  const unsigned char* s = static_cast<const unsigned char*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  for (int64_t o = 0; o < outer; ++o)
    for (int64_t m = 0; m < idx_len; ++m) {
      const int64_t j = idx[o * idx_stride_outer + m * idx_stride_len];
      unsigned char* out = d + (o * idx_len + m) * inner_bytes;
      if (j < 0 || j >= src_len) {
        set_status(status, CO_ST_INDEX_RANGE);
        std::memset(out, 0, (size_t)inner_bytes);
      } else {
        std::memcpy(out, s + o * src_stride_outer + j * src_stride_len, (size_t)inner_bytes);
      }
    }
  return CO_OK;
}

// ------------------------------------------------------------------ policy evaluation
// tasks/eval.py:137-144: unbatchify -> max(dim=1) -> gather_by_index over the [K, B] layout
CO_HOST_API int co_best_of(int64_t B, int64_t K, int64_t T, const float* reward,
                           const int64_t* actions, int64_t sb, int64_t st, float* best_reward,
                           int64_t* best_idx, int64_t* best_actions, int32_t*, void*) {
  if (B < 0 || K <= 0 || T < 0 || K > 0x7ffffffe) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!reward || !best_reward || !best_idx) return CO_E_INVAL;
  if (T == 0) best_actions = nullptr;
  if (best_actions && (!actions || best_actions == actions)) return CO_E_INVAL;
  for (int64_t b = 0; b < B; ++b) {
    float bv = reward[b];
    int bk = 0;
    for (int64_t k = 1; k < K; ++k)
      if (argmax_better(reward[k * B + b], (int)k, bv, bk)) {
        bv = reward[k * B + b];
        bk = (int)k;
      }
    best_reward[b] = bv;
    best_idx[b] = bk;
    if (best_actions) {
      const int64_t* src = actions + (bk * B + b) * sb;
      for (int64_t t = 0; t < T; ++t) best_actions[b * T + t] = src[t * st];
    }
  }
  return CO_OK;
}

// the same with every candidate scored as co_tsp_reward scores it, on the un-replicated locs
CO_HOST_API int co_tsp_best_of(int64_t B, int64_t N, int64_t K, const float* locs,
                               const int64_t* actions, int64_t sb, int64_t st, int check,
                               float* all_reward, float* best_reward, int64_t* best_idx,
                               int64_t* best_actions, int32_t* status, void*) {
  if (B < 0 || N <= 0 || K <= 0 || N > 1024 || K > 0x7ffffffe || B > 0x7fffffff)
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !best_reward || !best_idx || (check && !status)) return CO_E_INVAL;
  if (best_actions == actions) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  for (int64_t b = 0; b < B; ++b) {
    float bv = 0.f;
    int bk = -1;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t e = k * B + b;
      float r;
      // one row against instance b: co_tsp_reward with the row's own base pointers
      const int rc = co_tsp_reward(1, N, N, locs + b * N * 2, 1, actions + e * sb, sb, st, check,
                                   &r, status, nullptr);
      if (rc != CO_OK) return rc;
      if (all_reward) all_reward[e] = r;
      if (bk < 0 || argmax_better(r, (int)k, bv, bk)) {
        bv = r;
        bk = (int)k;
      }
    }
    best_reward[b] = bv;
    best_idx[b] = bk;
    if (best_actions) {
      const int64_t* src = actions + (bk * B + b) * sb;
      for (int64_t t = 0; t < N; ++t) best_actions[b * N + t] = src[t * st];
    }
  }
  return CO_OK;
}

// ---------------------------------------------------------------------------- decode
// decoding.py:141-191 (tanh clip -> mask -> /T -> log_softmax), 327-399 (greedy argmax,
// sampling by inverse CDF of a Philox draw keyed by (seed, offset, row), evaluate)
CO_HOST_API int co_decode_step(int64_t B, int64_t N, const float* logits, int64_t stride,
                               const uint8_t* mask, float clip, float temp, int mode,
                               const int64_t* action_in, int64_t* action_out, float* logp_sel,
                               float* logp_full, uint64_t seed, uint64_t offset, int32_t* status,
                               void*) {
  // the host path is always exact: the fast / certified math flags select nothing here
  mode &= ~(CO_DECODE_FAST | CO_DECODE_CERTIFIED);
  if (B < 0 || N <= 0 || mode < 0 || mode > 2) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!logits || !action_out || !logp_sel) return CO_E_INVAL;
  if (mode == CO_DECODE_EVALUATE && !action_in) return CO_E_INVAL;
  std::vector<float> x((size_t)N), e((size_t)N);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = logits + b * stride;
    float m = -INFINITY;
    for (int64_t c = 0; c < N; ++c) {
      float v = lr[c];
      if (clip > 0.f) v = tanh_cr(v) * clip;
      if (mask && !mask[b * N + c]) v = -INFINITY;
      if (temp != 1.f) v = v / temp;
      x[(size_t)c] = v;
      m = std::fmax(m, v);  // as the device (fmaxf): a NaN logit makes every logp NaN anyway
    }
    for (int64_t c = 0; c < N; ++c) {
      x[(size_t)c] = x[(size_t)c] - m;
      e[(size_t)c] = aten_expf(x[(size_t)c]);
    }
    const float Lg = aten_logf(aten_row_sum(e.data(), (int)N));
    for (int64_t c = 0; c < N; ++c) x[(size_t)c] = x[(size_t)c] - Lg;  // (x - m) - L
    int64_t sel = 0;
    if (mode == CO_DECODE_GREEDY) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = 0; c < (int)N; ++c)
        if (argmax_better(x[(size_t)c], c, bv, bi)) {
          bv = x[(size_t)c];
          bi = c;
        }
      sel = bi == 0x7fffffff ? 0 : bi;
    } else if (mode == CO_DECODE_SAMPLING) {
      const uint32_t r = philox_u32(seed, offset, (uint64_t)b);
      const float u = (float)(r >> 8) * (1.0f / 16777216.0f);
      float total = 0.f;
      for (int64_t c = 0; c < N; ++c) total += std::exp(x[(size_t)c]);
      const float target = u * total;
      float run = 0.f;
      int64_t hit = -1, last = -1;
      for (int64_t c = 0; c < N; ++c) {
        const float p = std::exp(x[(size_t)c]);
        run += p;
        if (p > 0.f) {
          last = c;
          if (run > target && hit < 0) hit = c;
        }
      }
      sel = hit >= 0 ? hit : (last >= 0 ? last : 0);
    } else {
      const int64_t a = action_in[b];
      if (a < 0 || a >= N) set_status(status, CO_ST_INDEX_RANGE);
      sel = (a < 0 || a >= N) ? 0 : a;
    }
    action_out[b] = mode == CO_DECODE_EVALUATE ? action_in[b] : sel;
    logp_sel[b] = x[(size_t)sel];
    if (logp_full) std::memcpy(logp_full + b * N, x.data(), sizeof(float) * (size_t)N);
    if (mode != CO_DECODE_EVALUATE && mask && !mask[b * N + sel])
      set_status(status, CO_ST_INFEASIBLE);
  }
  return CO_OK;
}

// ---------------------------------------------------------------------------
// The k-opt improvement MDP of TSP (TSPkoptEnv, tsp/env.py:204-549; the header has the
// semantics).  The operators follow the linked list directly -- pred and a walk -- where the
// device works on positions, so the two builds check each other.
namespace {

inline bool kopt_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N > 0 && N <= CO_KOPT_MAX_N; }

// order = [0, rec[0], ...] and pos (its inverse) when rec is one N-cycle; false otherwise
bool kopt_rank(const int64_t* rec, int64_t N, std::vector<int64_t>& order,
               std::vector<int64_t>& pos) {
  for (int64_t v = 0; v < N; ++v)
    if (rec[v] < 0 || rec[v] >= N) return false;
  std::fill(pos.begin(), pos.end(), -1);
  int64_t cur = 0;
  for (int64_t k = 0; k < N; ++k) {
    if (pos[(size_t)cur] >= 0) return false;  // back at a node before all were seen
    pos[(size_t)cur] = k;
    order[(size_t)k] = cur;
    cur = rec[cur];
  }
  return cur == 0;
}

float kopt_cost(const float* lr, const int64_t* rec, int64_t N) {
  double acc = 0.0;
  for (int64_t v = 0; v < N; ++v)
    acc += (double)edge_len(lr[2 * v], lr[2 * v + 1], lr[2 * rec[v]], lr[2 * rec[v] + 1]);
  return (float)acc;
}

// one row, one step on rec (valid on entry); false with the status bit set on a failure
bool kopt_apply(int64_t N, int64_t K, const int64_t* act, int64_t sa, int64_t* rec,
                std::vector<int64_t>& pred, std::vector<int64_t>& order,
                std::vector<int64_t>& pos, int32_t* status) {
  const int64_t A = K == 2 ? 2 : 3 * K;
  for (int64_t j = 0; j < A; ++j)
    if (act[j * sa] < 0 || act[j * sa] >= N) {
      set_status(status, CO_ST_INDEX_RANGE);
      return false;
    }
  for (int64_t v = 0; v < N; ++v) pred[(size_t)rec[v]] = v;
  if (K == 2) {
    const int64_t first = act[0], second = act[sa];
    if (first == second) return true;
    const int64_t before = pred[(size_t)first], after = rec[second];
    const bool whole = before == second;
    // turn the links of first -> ... -> second round (pred is of the old list)
    for (int64_t cur = second; cur != first; cur = pred[(size_t)cur]) rec[cur] = pred[(size_t)cur];
    rec[first] = whole ? second : after;
    if (!whole) rec[before] = second;
    return true;
  }
  int64_t right_nodes[CO_KOPT_MAX_K];
  for (int64_t j = 0; j < K; ++j) right_nodes[j] = rec[act[j * sa]];
  for (int64_t j = 0; j < K; ++j) rec[act[(K + j) * sa]] = act[(2 * K + j) * sa];
  int64_t cur = act[K * sa];
  for (int64_t it = 0; it < N - 2; ++it) {
    const int64_t next = rec[cur], po = pred[(size_t)next];
    bool right = false;
    for (int64_t j = 0; j < K; ++j) right |= right_nodes[j] == next;
    if (po != cur && !right) rec[next] = po;
    cur = next;
  }
  if (!kopt_rank(rec, N, order, pos)) {
    set_status(status, CO_ST_INVALID_TOUR);
    return false;
  }
  return true;
}

// the shared body of reset / step / steps (the device's kopt_kernel, row by row)
int kopt_rows(int64_t B, int64_t N, int64_t K, int64_t T, const float* locs, int64_t LB,
              const int64_t* rec_in, int64_t* rec_out, const int64_t* actions, int64_t st,
              int64_t sb, int64_t sa, float* cost_cur, const float* bsf_in, float* bsf_out,
              float* reward, float* cost_steps, int64_t* rec_best, int64_t* vt,
              const int64_t* i_in, int64_t* i_out, int32_t* status) {
  std::vector<int64_t> rec((size_t)N), best((size_t)N), pred((size_t)N), order((size_t)N),
      pos((size_t)N);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + (b % LB) * N * 2;
    std::copy(rec_in + b * N, rec_in + (b + 1) * N, rec.begin());
    if (!kopt_rank(rec.data(), N, order, pos)) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    float cost = kopt_cost(lr, rec.data(), N);
    float bsf = bsf_in ? bsf_in[b] : 0.f;
    bool dirty = false, stop = false;
    for (int64_t t = 0; t < T; ++t) {
      if (actions) {
        if (!kopt_apply(N, K, actions + t * st + b * sb, sa, rec.data(), pred, order, pos,
                        status)) {
          stop = true;
          break;
        }
        cost = kopt_cost(lr, rec.data(), N);
      }
      const float now = cost < bsf ? cost : bsf;
      const float rew = bsf - now;
      bsf = now;
      if (rew > 0.0f) {
        best = rec;
        dirty = true;
      }
      reward[t * B + b] = rew;
      if (cost_steps) cost_steps[t * B + b] = cost;
    }
    if (stop) continue;
    if (rec_out) std::copy(rec.begin(), rec.end(), rec_out + b * N);
    if (vt) {
      kopt_rank(rec.data(), N, order, pos);
      for (int64_t v = 0; v < N; ++v) vt[b * N + v] = v == 0 ? N : pos[(size_t)v];
    }
    if (dirty) std::copy(best.begin(), best.end(), rec_best + b * N);
    cost_cur[b] = cost;
    if (bsf_out) bsf_out[b] = bsf;
    if (i_out) i_out[b] = i_in[b] + T;
  }
  return CO_OK;
}

}  // namespace

CO_HOST_API int co_tsp_linked_list(int64_t B, int64_t N, const int64_t* tour, int64_t sb,
                                   int64_t st, int64_t* rec, int32_t* status, void*) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!tour || !rec || rec == tour || !status) return CO_E_INVAL;
  std::vector<uint8_t> seen((size_t)N);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* tr = tour + b * sb;
    std::fill(seen.begin(), seen.end(), 0);
    bool bad = false;
    for (int64_t k = 0; k < N && !bad; ++k) {
      const int64_t x = tr[k * st];
      if (x < 0 || x >= N || seen[(size_t)x]) bad = true;
      else seen[(size_t)x] = 1;
    }
    if (bad) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    for (int64_t k = 0; k < N; ++k) rec[b * N + tr[k * st]] = tr[(k + 1 == N ? 0 : k + 1) * st];
  }
  return CO_OK;
}

CO_HOST_API int co_tsp_real_solution(int64_t B, int64_t N, const int64_t* rec, int64_t* solution,
                                     int32_t* status, void*) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!rec || !solution || !status) return CO_E_INVAL;
  std::vector<int64_t> order((size_t)N), pos((size_t)N);
  for (int64_t b = 0; b < B; ++b) {
    if (!kopt_rank(rec + b * N, N, order, pos)) {
      set_status(status, CO_ST_INVALID_TOUR);
      continue;
    }
    std::copy(order.begin(), order.end(), solution + b * N);
  }
  return CO_OK;
}

CO_HOST_API int co_tsp_kopt_reset(int64_t B, int64_t N, const float* locs, int64_t LB,
                                  const int64_t* rec, float* cost, int64_t* visited_time,
                                  int32_t* status, void*) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (LB <= 0 || B % LB != 0) return CO_E_INVAL;
  if (!locs || !rec || !cost || !status) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  return kopt_rows(B, N, 0, 0, locs, LB, rec, nullptr, nullptr, 0, 0, 0, cost, nullptr, nullptr,
                   nullptr, nullptr, nullptr, visited_time, nullptr, nullptr, status);
}

CO_HOST_API int co_tsp_kopt_steps(int64_t B, int64_t N, int64_t k_max, int64_t steps,
                                  const float* locs, int64_t LB, const int64_t* actions,
                                  int64_t st, int64_t sb, int64_t sa, int64_t* rec_current,
                                  float* cost_current, float* cost_bsf, int64_t* rec_best,
                                  int64_t* visited_time, int64_t* i, float* reward,
                                  float* cost_steps, int32_t* status, void*) {
  if (!kopt_sizes_ok(B, N) || k_max < 2 || k_max > CO_KOPT_MAX_K || steps < 0)
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (LB <= 0 || B % LB != 0) return CO_E_INVAL;
  if (!locs || !rec_current || !cost_current || !cost_bsf || !rec_best ||
      rec_best == rec_current || !visited_time || !status || (steps > 0 && (!actions || !reward)))
    return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  return kopt_rows(B, N, k_max, steps, locs, LB, rec_current, rec_current, actions, st, sb, sa,
                   cost_current, cost_bsf, cost_bsf, reward, cost_steps, rec_best, visited_time,
                   i, i, status);
}

CO_HOST_API int co_tsp_kopt_step(int64_t B, int64_t N, int64_t k_max, const float* locs,
                                 int64_t LB, const int64_t* rec_in, const int64_t* action,
                                 int64_t sb, int64_t sa, int64_t* rec_out, float* cost_current,
                                 const float* cost_bsf_in, float* cost_bsf_out, float* reward,
                                 int64_t* rec_best, int64_t* visited_time, const int64_t* i_in,
                                 int64_t* i_out, int32_t* status, void*) {
  if (!kopt_sizes_ok(B, N) || (action && (k_max < 2 || k_max > CO_KOPT_MAX_K)))
    return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (LB <= 0 || B % LB != 0) return CO_E_INVAL;
  if (!locs || !rec_in || !rec_out || !cost_current || !cost_bsf_in || !cost_bsf_out ||
      !reward || !rec_best || rec_best == rec_out || rec_best == rec_in || !visited_time ||
      !status || (action && (!i_in || !i_out)))
    return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  return kopt_rows(B, N, action ? k_max : 0, 1, locs, LB, rec_in, rec_out, action, 0, sb, sa,
                   cost_current, cost_bsf_in, cost_bsf_out, reward, nullptr, rec_best,
                   visited_time, action ? i_in : nullptr, action ? i_out : nullptr, status);
}

CO_HOST_API int co_tsp_nearest_rec(int64_t B, int64_t N, const float* locs, int64_t* rec, void*) {
  if (!kopt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !rec) return CO_E_INVAL;
  if (reinterpret_cast<uintptr_t>(locs) & 7) return CO_E_ALIGN;
  std::vector<uint8_t> seen((size_t)N);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + b * N * 2;
    int64_t* r = rec + b * N;
    std::fill(r, r + N, 0);
    std::fill(seen.begin(), seen.end(), 0);
    seen[0] = 1;
    int64_t cur = 0;
    for (int64_t it = 0; it < N - 1; ++it) {
      float best = INFINITY;
      int64_t bi = -1;
      for (int64_t v = 0; v < N; ++v) {
        const float d = seen[(size_t)v] ? 1e5f
                                        : edge_len(lr[2 * cur], lr[2 * cur + 1], lr[2 * v], lr[2 * v + 1]);
        if (d < best) best = d, bi = v;
      }
      if (bi < 0) break;
      r[cur] = bi;
      seen[(size_t)bi] = 1;
      cur = bi;
    }
  }
  return CO_OK;
}

// -------------------------------------------------------------------------- CVRPTW
// cvrptw/env.py in its plain scalar form; co_env.h states the semantics.  co_cvrptw_steps
// is literally `steps` single steps per row, each with its full distance vector.
namespace {
inline float tw_ldf(const void* p, int dt, int64_t i) {
  if (dt == CO_DT_F32) return static_cast<const float*>(p)[i];
  if (dt == CO_DT_I32) return (float)static_cast<const int32_t*>(p)[i];
  return (float)static_cast<const int64_t*>(p)[i];
}
inline float tw_dist(float px, float py, float qx, float qy) {
  const float dx = px - qx, dy = py - qy;
  return std::sqrt(dx * dx + dy * dy);
}
inline float tw_max(float p, float s) {
  return (p != p || s != s) ? __builtin_nanf("") : (p > s ? p : s);
}
inline float tw_trunc(float x) {
  return (x >= -2147483648.f && x < 2147483648.f) ? (float)(int32_t)x : -2147483648.f;
}
inline bool tw_dt_ok(int dt) { return dt == CO_DT_F32 || dt == CO_DT_I32 || dt == CO_DT_I64; }
inline bool tw_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N > 0 && N <= CO_CVRPTW_MAX_N; }
inline bool tw_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

// get_action_mask (cvrptw/env.py:103-115) of one row; lr = the row's [NC, 2] coordinates,
// twr = the row's first window element index
void tw_mask_row(int64_t N, const float* lr, const float* dem, float used, float cap,
                 const uint8_t* vis, int64_t cur, float tnow, const void* tw, int tw_dt,
                 int64_t twr, float* cur_loc, float* dist, uint8_t* mask) {
  const int64_t cc = cur < 0 ? 0 : (cur > N ? N : cur);
  const float cx = lr[2 * cc], cy = lr[2 * cc + 1];
  cur_loc[0] = cx;
  cur_loc[1] = cy;
  cvrp_mask_row(N, dem, used, cap, vis, cur, mask);
  for (int64_t c = 0; c <= N; ++c) {
    const float d = tw_dist(cx, cy, lr[2 * c], lr[2 * c + 1]);
    dist[c] = d;
    mask[c] = mask[c] && (tnow + d <= tw_ldf(tw, tw_dt, twr + 2 * c + 1));
  }
}

// one step of one row on its state (cvrptw/env.py:117-134, cvrp/env.py:73-105); returns
// whether the action was in range.  dleg = distances_in[clamp(a)]
bool tw_step_row(int64_t N, int64_t a, const float* dem, float& used, uint8_t* vis, float& tnow,
                 float dleg, const void* dur, int dur_dt, int64_t durr, const void* tw,
                 int tw_dt, int64_t twr) {
  const bool bad = a < 0 || a > N;
  const int64_t ac = a < 0 ? 0 : (a > N ? N : a);
  int64_t di = a - 1;
  di = di < 0 ? 0 : (di > N - 1 ? N - 1 : di);
  const float m01 = a != 0 ? 1.0f : 0.0f;
  tnow = m01 * (tw_max(tnow + dleg, tw_ldf(tw, tw_dt, twr + 2 * ac)) +
                tw_ldf(dur, dur_dt, durr + ac));
  used = (used + dem[di]) * m01;
  if (!bad) vis[a] = 1;
  return !bad;
}
}  // namespace

CO_HOST_API int co_cvrptw_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                                const float* demand, float vcap, const void* tw, int tw_dt,
                                float* locs_out, int64_t* cur, float* time, float* used,
                                float* vcap_out, uint8_t* visited, float* cur_loc, float* dist,
                                uint8_t* mask, void*) {
  if (!tw_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !demand || !tw || !locs_out || !cur || !time || !used || !vcap_out ||
      !visited || !cur_loc || !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt)) return CO_E_MODE;
  if (tw_mis8(depot) || tw_mis8(locs_in) || tw_mis8(locs_out) || tw_mis8(cur_loc))
    return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    float* lo = locs_out + b * NC * 2;
    lo[0] = depot[2 * b];
    lo[1] = depot[2 * b + 1];
    std::memcpy(lo + 2, locs_in + b * N * 2, sizeof(float) * 2 * (size_t)N);
    std::memset(visited + b * NC, 0, (size_t)NC);
    cur[b] = 0;
    time[b] = 0.f;
    used[b] = 0.f;
    vcap_out[b] = vcap;
    tw_mask_row(N, lo, demand + b * N, 0.f, vcap, visited + b * NC, 0, 0.f, tw, tw_dt,
                2 * b * NC, cur_loc + 2 * b, dist + b * NC, mask + b * NC);
  }
  return CO_OK;
}

CO_HOST_API int co_cvrptw_step(int64_t B, int64_t N, const int64_t* action, const float* locs,
                               const float* demand, const float* used_in, float* used_out,
                               const float* vcap, const uint8_t* vis_in, uint8_t* vis_out,
                               const float* t_in, const float* dist_in, const void* dur,
                               int dur_dt, const void* tw, int tw_dt, float* t_out,
                               int64_t* cur_out, uint8_t* done, uint8_t* reward, float* cur_loc,
                               float* dist, uint8_t* mask, int32_t* status, int32_t* not_done,
                               void*) {
  if (!tw_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !locs || !demand || !used_in || !used_out || !vcap || !vis_in || !vis_out ||
      !t_in || !dist_in || !dur || !tw || !t_out || !cur_out || !done || !reward || !cur_loc ||
      !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  int32_t left = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t a = action[b];
    const int64_t ac = a < 0 ? 0 : (a > N ? N : a);
    uint8_t* vo = vis_out + b * NC;
    if (vo != vis_in + b * NC) std::memcpy(vo, vis_in + b * NC, (size_t)NC);
    float used = used_in[b], tnow = t_in[b];
    if (!tw_step_row(N, a, demand + b * N, used, vo, tnow, dist_in[b * NC + ac], dur, dur_dt,
                     b * NC, tw, tw_dt, 2 * b * NC))
      set_status(status, CO_ST_INDEX_RANGE);
    int64_t vsum = 0;
    for (int64_t c = 0; c < NC; ++c) vsum += vo[c];
    used_out[b] = used;
    t_out[b] = tnow;
    cur_out[b] = a;
    done[b] = vsum == NC;
    left += vsum != NC;
    reward[b] = 0;
    tw_mask_row(N, locs + b * NC * 2, demand + b * N, used, vcap[b], vo, a, tnow, tw, tw_dt,
                2 * b * NC, cur_loc + 2 * b, dist + b * NC, mask + b * NC);
  }
  if (not_done) *not_done += left;
  return CO_OK;
}

CO_HOST_API int co_cvrptw_action_mask(int64_t B, int64_t N, const float* locs,
                                      const float* demand, const float* used, const float* vcap,
                                      const uint8_t* visited, const int64_t* cur,
                                      const float* time, const void* tw, int tw_dt,
                                      float* cur_loc, float* dist, uint8_t* mask, void*) {
  if (!tw_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !demand || !used || !vcap || !visited || !cur || !time || !tw || !cur_loc ||
      !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b)
    tw_mask_row(N, locs + b * NC * 2, demand + b * N, used[b], vcap[b], visited + b * NC, cur[b],
                time[b], tw, tw_dt, 2 * b * NC, cur_loc + 2 * b, dist + b * NC, mask + b * NC);
  return CO_OK;
}

CO_HOST_API int co_cvrptw_check(int64_t B, int64_t N, int64_t T, const float* locs,
                                const int64_t* actions, int64_t sb, int64_t st, const void* dur,
                                int dur_dt, const void* tw, int tw_dt, int32_t* status, void*) {
  if (!tw_sizes_ok(B, N) || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || (T > 0 && !actions) || !dur || !tw || !status) return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  const int64_t NC = N + 1;
  const float deadline0 = tw_ldf(tw, tw_dt, 1);  // time_windows[0, 0, 1]
  for (int64_t b = 0; b < B; ++b) {
    const int64_t row = b * NC;
    const float* lr = locs + 2 * row;
    int32_t bits = 0;
    for (int64_t c = 0; c < NC; ++c) {
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
  return CO_OK;
}

CO_HOST_API int co_cvrptw_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                                int64_t st, int64_t sb, const float* locs, const float* demand,
                                float* used, const float* vcap, uint8_t* visited, float* time_io,
                                int64_t* cur, const float* dist_in, const void* dur, int dur_dt,
                                const void* tw, int tw_dt, uint8_t* done, uint8_t* reward,
                                float* cur_loc, float* dist, uint8_t* mask, uint8_t* feasible,
                                float* time, int32_t* status, int32_t* not_done, void*) {
  if (!tw_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !locs || !demand || !used || !vcap || !visited || !time_io || !cur ||
      !dist_in || !dur || !tw || !done || !reward || !cur_loc || !dist || !mask)
    return CO_E_INVAL;
  if (!tw_dt_ok(tw_dt) || !tw_dt_ok(dur_dt)) return CO_E_MODE;
  if (tw_mis8(locs) || tw_mis8(cur_loc)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  std::vector<float> dv((size_t)NC);
  std::vector<uint8_t> mv((size_t)NC);
  int32_t left = 0;
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + b * NC * 2;
    const float* dem = demand + b * N;
    uint8_t* vis = visited + b * NC;
    float u = used[b], tnow = time_io[b], cl[2];
    int64_t c_now = cur[b];
    std::copy(dist_in + b * NC, dist_in + (b + 1) * NC, dv.begin());
    if (feasible) {  // the mask of the input state on the caller's distances
      cvrp_mask_row(N, dem, u, vcap[b], vis, c_now, mv.data());
      for (int64_t c = 0; c < NC; ++c)
        mv[(size_t)c] = mv[(size_t)c] &&
                        (tnow + dv[(size_t)c] <= tw_ldf(tw, tw_dt, 2 * (b * NC + c) + 1));
    }
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[t * st + b * sb];
      const int64_t ac = a < 0 ? 0 : (a > N ? N : a);
      const bool bad = a < 0 || a > N;
      if (feasible) feasible[t * B + b] = !bad && mv[(size_t)ac];
      if (!tw_step_row(N, a, dem, u, vis, tnow, dv[(size_t)ac], dur, dur_dt, b * NC, tw, tw_dt,
                       2 * b * NC))
        set_status(status, CO_ST_INDEX_RANGE);
      c_now = a;
      if (time) time[t * B + b] = tnow;
      tw_mask_row(N, lr, dem, u, vcap[b], vis, a, tnow, tw, tw_dt, 2 * b * NC, cl, dv.data(),
                  mv.data());
    }
    int64_t vsum = 0;
    for (int64_t c = 0; c < NC; ++c) vsum += vis[c];
    used[b] = u;
    time_io[b] = tnow;
    cur[b] = c_now;
    done[b] = vsum == NC;
    left += vsum != NC;
    reward[b] = 0;
    cur_loc[2 * b] = cl[0];
    cur_loc[2 * b + 1] = cl[1];
    std::copy(dv.begin(), dv.end(), dist + b * NC);
    std::copy(mv.begin(), mv.end(), mask + b * NC);
  }
  if (not_done) *not_done += left;
  return CO_OK;
}

// -------------------------------------------------------------------------- MTVRP
// mtvrp/env.py in its plain scalar form; co_env.h states the semantics.  co_mtvrp_steps is
// literally `steps` single steps per row, each followed by its full mask.
namespace {
struct MtInst {  // one row's inputs
  int64_t N;
  const float *lr, *tw, *svc, *dl, *db;
  float cap, speed, limit, nopen;
};
struct MtState {
  int64_t cur;
  float t, len, ul, ub;
};
inline bool mt_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N > 0 && N <= CO_MTVRP_MAX_N; }

inline MtInst mt_row(int64_t N, int64_t b, const co_mtvrp_instance* in) {
  const int64_t NC = N + 1;
  return MtInst{N, in->locs + 2 * b * NC, in->time_windows + 2 * b * NC,
                in->service_time + b * NC, in->demand_linehaul + b * NC,
                in->demand_backhaul + b * NC, in->vehicle_capacity[b],
                in->speed ? in->speed[b] : 1.f, in->distance_limit[b],
                in->open_route[b] != 0 ? 0.0f : 1.0f};
}
// every member but (with_speed = false: co_mtvrp_check) speed is there
inline bool mt_inst_ok(const co_mtvrp_instance* in, bool with_speed = true) {
  return in && in->locs && in->time_windows && in->service_time && in->demand_linehaul &&
         in->demand_backhaul && in->vehicle_capacity && (in->speed || !with_speed) &&
         in->distance_limit && in->open_route;
}

// get_action_mask (mtvrp/env.py:212-279) of one row
void mt_mask_row(const MtInst& in, const MtState& s, const uint8_t* vis, uint8_t* mask) {
  const int64_t N = in.N;
  const int64_t cc = s.cur < 0 ? 0 : (s.cur > N ? N : s.cur);
  const float cx = in.lr[2 * cc], cy = in.lr[2 * cc + 1], twe0 = in.tw[1];
  bool lhm = false;
  for (int64_t c = 0; c <= N; ++c) lhm = lhm || (!vis[c] && in.dl[c] > 0.f);
  const bool cbh = in.db[cc] > 0.f;
  bool anyc = false;
  for (int64_t c = 0; c <= N; ++c) {
    const float dij = tw_dist(cx, cy, in.lr[2 * c], in.lr[2 * c + 1]);
    const float dj0 = tw_dist(in.lr[2 * c], in.lr[2 * c + 1], in.lr[0], in.lr[1]);
    const float arr = s.t + dij / in.speed;
    const bool reach = arr < in.tw[2 * c + 1];
    const bool depot_ok =
        ((tw_max(arr, in.tw[2 * c]) + in.svc[c]) + dj0 / in.speed) * in.nopen < twe0;
    const bool over = (s.len + dij) + dj0 * in.nopen > in.limit;
    const bool dem = (lhm && !(in.dl[c] + s.ul > in.cap) && !cbh && in.dl[c] > 0.f) ||
                     (!(in.db[c] + s.ub > in.cap) && in.db[c] > 0.f);
    const bool can = reach && depot_ok && dem && !over && !vis[c];
    mask[c] = can;
    anyc = anyc || (c >= 1 && can);
  }
  mask[0] = !(s.cur == 0 && anyc);
}

// one step of one row (mtvrp/env.py:100-162); false for an action outside 0..N, which
// leaves the state as it was
bool mt_step_row(const MtInst& in, MtState& s, uint8_t* vis, int64_t a) {
  if (a < 0 || a > in.N) return false;
  const int64_t cc = s.cur < 0 ? 0 : (s.cur > in.N ? in.N : s.cur);
  const float leg = tw_dist(in.lr[2 * cc], in.lr[2 * cc + 1], in.lr[2 * a], in.lr[2 * a + 1]);
  const float m01 = a != 0 ? 1.0f : 0.0f;
  s.t = m01 * (tw_max(s.t + leg / in.speed, in.tw[2 * a]) + in.svc[a]);
  s.len = m01 * (s.len + leg);
  s.ul = m01 * (s.ul + in.dl[a]);
  s.ub = m01 * (s.ub + in.db[a]);
  vis[a] = 1;
  s.cur = a;
  return true;
}
}  // namespace

CO_HOST_API int co_mtvrp_reset(int64_t B, int64_t N, const co_mtvrp_instance* in, int64_t* cur, float* time, float* route_len,
                               float* used_l, float* used_b, uint8_t* visited, uint8_t* mask,
                               void*) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mt_inst_ok(in) || !cur || !time ||
      !route_len || !used_l || !used_b || !visited || !mask)
    return CO_E_INVAL;
  if (tw_mis8(in->locs) || tw_mis8(in->time_windows)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    std::memset(visited + b * NC, 0, (size_t)NC);
    cur[b] = 0;
    time[b] = route_len[b] = used_l[b] = used_b[b] = 0.f;
    mt_mask_row(mt_row(N, b, in),
                MtState{0, 0.f, 0.f, 0.f, 0.f}, visited + b * NC, mask + b * NC);
  }
  return CO_OK;
}

CO_HOST_API int co_mtvrp_step(int64_t B, int64_t N, const int64_t* action, const co_mtvrp_instance* inst, const int64_t* cur_in,
                              const float* t_in, const float* len_in, const float* ul_in,
                              const float* ub_in, const uint8_t* vis_in, int64_t* cur_out,
                              float* t_out, float* len_out, float* ul_out, float* ub_out,
                              uint8_t* vis_out, uint8_t* done, float* reward, uint8_t* mask,
                              int32_t* status, int32_t* not_done, void*) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mt_inst_ok(inst) || !action ||
      !cur_in || !t_in || !len_in || !ul_in || !ub_in || !vis_in || !cur_out || !t_out ||
      !len_out || !ul_out || !ub_out || !vis_out || !done || !reward || !mask)
    return CO_E_INVAL;
  if (tw_mis8(inst->locs) || tw_mis8(inst->time_windows)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  int32_t left = 0;
  for (int64_t b = 0; b < B; ++b) {
    const MtInst in = mt_row(N, b, inst);
    uint8_t* vo = vis_out + b * NC;
    if (vo != vis_in + b * NC) std::memcpy(vo, vis_in + b * NC, (size_t)NC);
    MtState s{cur_in[b], t_in[b], len_in[b], ul_in[b], ub_in[b]};
    if (!mt_step_row(in, s, vo, action[b])) set_status(status, CO_ST_INDEX_RANGE);
    int64_t vsum = 0;
    for (int64_t c = 0; c < NC; ++c) vsum += vo[c] != 0;
    cur_out[b] = s.cur, t_out[b] = s.t, len_out[b] = s.len, ul_out[b] = s.ul, ub_out[b] = s.ub;
    done[b] = vsum == NC;
    left += vsum != NC;
    reward[b] = 0.f;
    mt_mask_row(in, s, vo, mask + b * NC);
  }
  if (not_done) *not_done += left;
  return CO_OK;
}

CO_HOST_API int co_mtvrp_action_mask(int64_t B, int64_t N, const co_mtvrp_instance* in, const int64_t* cur, const float* time,
                                     const float* route_len, const float* used_l,
                                     const float* used_b, const uint8_t* visited, uint8_t* mask,
                                     void*) {
  if (!mt_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mt_inst_ok(in) || !cur || !time ||
      !route_len || !used_l || !used_b || !visited || !mask)
    return CO_E_INVAL;
  if (tw_mis8(in->locs) || tw_mis8(in->time_windows)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b)
    mt_mask_row(mt_row(N, b, in),
                MtState{cur[b], time[b], route_len[b], used_l[b], used_b[b]}, visited + b * NC,
                mask + b * NC);
  return CO_OK;
}

CO_HOST_API int co_mtvrp_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                               int64_t st, int64_t sb, const co_mtvrp_instance* inst, int64_t* cur, float* time_io,
                               float* route_len, float* used_l, float* used_b, uint8_t* visited,
                               uint8_t* done, float* reward, uint8_t* mask, uint8_t* feasible,
                               float* time, float* rlen, int32_t* status, int32_t* not_done,
                               void*) {
  if (!mt_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mt_inst_ok(inst) || !actions ||
      !cur || !time_io || !route_len || !used_l || !used_b || !visited || !done || !reward ||
      !mask)
    return CO_E_INVAL;
  if (tw_mis8(inst->locs) || tw_mis8(inst->time_windows)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  int32_t left = 0;
  for (int64_t b = 0; b < B; ++b) {
    const MtInst in = mt_row(N, b, inst);
    uint8_t *vis = visited + b * NC, *mv = mask + b * NC;
    MtState s{cur[b], time_io[b], route_len[b], used_l[b], used_b[b]};
    mt_mask_row(in, s, vis, mv);  // the mask of the input state
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[t * st + b * sb];
      const bool bad = a < 0 || a > N;
      if (feasible) feasible[t * B + b] = !bad && mv[a];
      if (!mt_step_row(in, s, vis, a)) set_status(status, CO_ST_INDEX_RANGE);
      if (time) time[t * B + b] = s.t;
      if (rlen) rlen[t * B + b] = s.len;
      mt_mask_row(in, s, vis, mv);
    }
    int64_t vsum = 0;
    for (int64_t c = 0; c < NC; ++c) vsum += vis[c] != 0;
    cur[b] = s.cur, time_io[b] = s.t, route_len[b] = s.len, used_l[b] = s.ul, used_b[b] = s.ub;
    done[b] = vsum == NC;
    left += vsum != NC;
    reward[b] = 0.f;
  }
  if (not_done) *not_done += left;
  return CO_OK;
}

CO_HOST_API int co_mtvrp_reward(int64_t B, int64_t N, int64_t T, const float* locs,
                                const int64_t* actions, int64_t sb, int64_t st,
                                const uint8_t* open, float* reward, int32_t* status, void*) {
  if (!mt_sizes_ok(B, N) || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || (T > 0 && !actions) || !open || !reward) return CO_E_INVAL;
  if (tw_mis8(locs)) return CO_E_ALIGN;
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + 2 * b * (N + 1);
    const bool op = open[b] != 0;
    int64_t prev = 0;
    bool prev_ok = true, range = false;
    double acc = 0.0;
    for (int64_t k = 0; k < T; ++k) {
      const int64_t a = actions[b * sb + k * st];
      if (a < 0 || a > N) {
        range = true;
        prev_ok = false;
        continue;
      }
      if (prev_ok && !(a == 0 && op))
        acc += (double)tw_dist(lr[2 * prev], lr[2 * prev + 1], lr[2 * a], lr[2 * a + 1]);
      prev = a;
      prev_ok = true;
    }
    if (prev_ok && !op) acc += (double)tw_dist(lr[2 * prev], lr[2 * prev + 1], lr[0], lr[1]);
    reward[b] = -(float)acc;
    if (range) set_status(status, CO_ST_INDEX_RANGE);
  }
  return CO_OK;
}

CO_HOST_API int co_mtvrp_check(int64_t B, int64_t N, int64_t T, const co_mtvrp_instance* inst,
                               const int64_t* actions, int64_t sb, int64_t st, int32_t* status,
                               void*) {
  if (!mt_sizes_ok(B, N) || T < 0 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!mt_inst_ok(inst, false) || (T > 0 && !actions) || !status) return CO_E_INVAL;
  if (tw_mis8(inst->locs) || tw_mis8(inst->time_windows)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  std::vector<uint8_t> seen((size_t)NC);
  for (int64_t b = 0; b < B; ++b) {
    const MtInst in = mt_row(N, b, inst);
    int32_t bits = 0;
    std::fill(seen.begin(), seen.end(), 0);
    int64_t nonzero = 0;
    bool range = false, dup = false;
    for (int64_t k = 0; k < T; ++k) {
      const int64_t a = actions[b * sb + k * st];
      if (a < 0 || a > N) {
        range = true;
      } else if (a != 0) {
        ++nonzero;
        dup = dup || seen[(size_t)a];
        seen[(size_t)a] = 1;
      }
    }
    if (range) bits |= CO_ST_INDEX_RANGE;
    if (range || dup || nonzero != N) bits |= CO_ST_INVALID_TOUR;
    const float twe0 = in.tw[1];
    if (!(in.limit >= 0.f)) bits |= CO_ST_MT_LIMIT_NEGATIVE;
    for (int64_t c = 0; c < NC; ++c) {
      const float s = in.tw[2 * c], e = in.tw[2 * c + 1];
      const float d0 = tw_dist(in.lr[2 * c], in.lr[2 * c + 1], in.lr[0], in.lr[1]);
      if (!(s >= 0.f) || !(e >= 0.f)) bits |= CO_ST_MT_TW_NEGATIVE;
      if (!(in.svc[c] >= 0.f)) bits |= CO_ST_MT_SERVICE_NEGATIVE;
      if (!(s < e)) bits |= CO_ST_MT_TW_INFEASIBLE;
      if (!((s + d0) + in.svc[c] <= twe0)) bits |= CO_ST_MT_DEPOT_RETURN;
    }
    if (!range) {
      const bool op = in.nopen == 0.0f;
      float t = 0.f, len = 0.f, ul = 0.f, ub = 0.f;
      int64_t prev = 0;
      for (int64_t k = 0; k < T; ++k) {
        const int64_t a = actions[b * sb + k * st];
        const float d = tw_dist(in.lr[2 * prev], in.lr[2 * prev + 1], in.lr[2 * a],
                                in.lr[2 * a + 1]);
        len = len + d * ((op && a == 0) ? 0.0f : 1.0f);
        if (!(len <= in.limit)) bits |= CO_ST_MT_ROUTE_LIMIT;
        if (a == 0) len = 0.f;
        t = tw_max(t + d, in.tw[2 * a]);
        if (!(t <= in.tw[2 * a + 1])) bits |= CO_ST_MT_DEADLINE;
        t = t + in.svc[a];
        if (a == 0) t = 0.f;
        const float m01 = a != 0 ? 1.0f : 0.0f;
        ul = ul * m01 + in.dl[a];
        ub = ub * m01 + in.db[a];
        if (!(ul <= in.cap)) bits |= CO_ST_MT_OVER_LINEHAUL;
        if (!(ub <= in.cap)) bits |= CO_ST_MT_OVER_BACKHAUL;
        prev = a;
      }
    }
    if (bits) set_status(status, bits);
  }
  return CO_OK;
}

// ---------------------------------------------------------------------------- PDP
// include/co_env.h (PDP): pdp/env.py:20-234, a plain loop per row.
namespace {
inline bool pdp_sizes_ok(int64_t B, int64_t N) {
  return B >= 0 && N >= 2 && N <= CO_PDP_MAX_N && N % 2 == 0;
}
inline bool pdp_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }

// one step on a row's two sets (env.py:67-89); false: the action is outside 0..N
inline bool pdp_row_step(int64_t N, int64_t a, uint8_t* av, uint8_t* td) {
  if (a < 0 || a > N) return false;
  av[a] = 0;
  td[(a + N / 2) % (N + 1)] = 1;
  return true;
}

// mask = available & to_deliver on 0 / 1 bytes; -> a column of available is left
inline bool pdp_row_mask(int64_t NC, uint8_t* av, uint8_t* td, uint8_t* mask) {
  bool left = false;
  for (int64_t c = 0; c < NC; ++c) {
    av[c] = av[c] != 0;
    td[c] = td[c] != 0;
    mask[c] = av[c] & td[c];
    left |= av[c] != 0;
  }
  return left;
}
}  // namespace

// pdp/env.py:108-151
CO_HOST_API int co_pdp_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                             float* locs_out, uint8_t* available, uint8_t* to_deliver,
                             uint8_t* mask, int64_t* cur, int64_t* i, uint8_t* done,
                             uint8_t* terminated, void*) {
  if (!pdp_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !locs_out || !available || !to_deliver || !mask || !cur || !i ||
      !done || !terminated)
    return CO_E_INVAL;
  if (pdp_mis8(depot) || pdp_mis8(locs_in) || pdp_mis8(locs_out)) return CO_E_ALIGN;
  const int64_t NC = N + 1, h = N / 2;
  for (int64_t b = 0; b < B; ++b) {
    float* lo = locs_out + b * NC * 2;
    lo[0] = depot[2 * b];
    lo[1] = depot[2 * b + 1];
    std::memcpy(lo + 2, locs_in + b * N * 2, (size_t)N * 2 * sizeof(float));
    for (int64_t c = 0; c < NC; ++c) {
      available[b * NC + c] = 1;
      to_deliver[b * NC + c] = c <= h;
      mask[b * NC + c] = c == 0;
    }
    cur[b] = 0;
    i[b] = 0;
    done[b] = 0;
    terminated[b] = 0;
  }
  return CO_OK;
}

// pdp/env.py:67-106
CO_HOST_API int co_pdp_step(int64_t B, int64_t N, const int64_t* action, const uint8_t* av_in,
                            const uint8_t* td_in, uint8_t* av_out, uint8_t* td_out,
                            uint8_t* mask, const int64_t* i_in, int64_t* i_out,
                            int64_t* cur_out, uint8_t* done, uint8_t* reward, int32_t* status,
                            void*) {
  if (!pdp_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !av_in || !td_in || !av_out || !td_out || !mask || !i_in || !i_out ||
      !cur_out || !done || !reward)
    return CO_E_INVAL;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    uint8_t *av = av_out + b * NC, *td = td_out + b * NC;
    if (av != av_in + b * NC) std::memcpy(av, av_in + b * NC, (size_t)NC);
    if (td != td_in + b * NC) std::memcpy(td, td_in + b * NC, (size_t)NC);
    if (!pdp_row_step(N, action[b], av, td)) set_status(status, CO_ST_INDEX_RANGE);
    done[b] = !pdp_row_mask(NC, av, td, mask + b * NC);
    reward[b] = 0;
    i_out[b] = i_in[b] + 1;
    cur_out[b] = action[b];
  }
  return CO_OK;
}

// `steps` co_pdp_step calls; feasible: the mask's value for a_t before step t
CO_HOST_API int co_pdp_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions,
                             int64_t st, int64_t sb, const uint8_t* mask_in,
                             uint8_t* available, uint8_t* to_deliver, uint8_t* mask, int64_t* i,
                             int64_t* cur, uint8_t* done, uint8_t* reward, uint8_t* feasible,
                             int32_t* status, void*) {
  if (!pdp_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !available || !to_deliver || !mask || !i || !cur || !done || !reward ||
      (feasible && !mask_in) || mask == mask_in)
    return CO_E_INVAL;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    uint8_t *av = available + b * NC, *td = to_deliver + b * NC;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[t * st + b * sb];
      const bool in = a >= 0 && a <= N;
      if (feasible)
        feasible[t * B + b] =
            in && (t == 0 ? mask_in[b * NC + a] != 0 : (av[a] != 0 && td[a] != 0));
      if (!pdp_row_step(N, a, av, td)) set_status(status, CO_ST_INDEX_RANGE);
      cur[b] = a;
    }
    done[b] = !pdp_row_mask(NC, av, td, mask + b * NC);
    reward[b] = 0;
    i[b] += T;
  }
  return CO_OK;
}

// pdp/env.py:189-216: the reward and, with check, the two validity tests in tour order
CO_HOST_API int co_pdp_reward(int64_t B, int64_t N, int64_t T, const float* locs, int64_t LB,
                              const int64_t* actions, int64_t sb, int64_t st, int check,
                              float* reward, int32_t* status, void*) {
  if (!pdp_sizes_ok(B, N) || T < 1 || T > 2048 || (check && T % 2 == 0)) return CO_E_INVAL;
  if (LB <= 0 || (B > 0 && B % LB != 0)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !actions || !reward || (check && !status)) return CO_E_INVAL;
  if (pdp_mis8(locs)) return CO_E_ALIGN;
  const int64_t NC = N + 1, T2 = T / 2;
  std::vector<uint8_t> seen(check ? (size_t)T : 0);
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + (b % LB) * NC * 2;
    bool dup = false, prec = false, have = true;
    float px = lr[0], py = lr[1];
    double len = 0.0;
    if (check) std::fill(seen.begin(), seen.end(), 0);
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[b * sb + t * st];
      const bool in = a >= 0 && a <= N;
      float qx = 0.f, qy = 0.f;
      if (in) {
        qx = lr[2 * a], qy = lr[2 * a + 1];
        if (have) len += (double)edge_len(px, py, qx, qy);
      } else {
        set_status(status, CO_ST_INDEX_RANGE);
      }
      if (check) {
        if (a < 0 || a >= T || seen[a]) {
          dup = true;
        } else {
          if (a > T2 && !seen[a - T2]) prec = true;
          seen[a] = 1;
        }
      }
      px = qx, py = qy, have = in;
    }
    if (have) len += (double)edge_len(px, py, lr[0], lr[1]);
    reward[b] = -(float)len;
    if (check && dup) set_status(status, CO_ST_PDP_NOT_ALL_NODES);
    if (check && !dup && prec) set_status(status, CO_ST_PDP_PRECEDENCE);
  }
  return CO_OK;
}

// ----------------------------------------------------------------------------- OP
// include/co_env.h (OP): op/env.py:24-262, a plain loop per row.
namespace {
inline bool op_sizes_ok(int64_t B, int64_t N) { return B >= 0 && N >= 1 && N <= CO_OP_MAX_N; }
inline bool op_mis8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }
inline int64_t op_clamp(int64_t a, int64_t N) { return a < 0 ? 0 : (a > N ? N : a); }

// env.py:153-169 for one column of a row's state; cl = locs[clamp(current_node)]
inline bool op_open(const float* lr, const float* ml, const uint8_t* vis, float tl,
                    const float* cl, int64_t c) {
  if (c == 0) return true;
  const bool exceeds = tl + edge_len(lr[2 * c], lr[2 * c + 1], cl[0], cl[1]) > ml[c];
  return !(vis[c] != 0 || vis[0] != 0 || exceeds);
}

inline void op_row_mask(int64_t NC, const float* lr, const float* ml, const uint8_t* vis,
                        float tl, int64_t cur, uint8_t* mask) {
  const float* cl = lr + 2 * op_clamp(cur, NC - 1);
  for (int64_t c = 0; c < NC; ++c) mask[c] = op_open(lr, ml, vis, tl, cl, c);
}

// env.py:74-108 on a row's state (vis holds 0 / 1 bytes); false: a is outside 0..N
inline bool op_row_step(int64_t N, int64_t a, const float* lr, const float* pr, uint8_t* vis,
                        float& tl, float& pz, int64_t& cur, int64_t& i, uint8_t& done) {
  const bool in = a >= 0 && a <= N;
  if (in) {
    const float* cl = lr + 2 * op_clamp(cur, N);
    tl = tl + edge_len(lr[2 * a], lr[2 * a + 1], cl[0], cl[1]);
    pz = pz + pr[a];
    vis[a] = 1;
  }
  done = a == 0 && i > 0;
  i += 1;
  cur = a;
  return in;
}
}  // namespace

// op/env.py:110-151
CO_HOST_API int co_op_reset(int64_t B, int64_t N, const float* depot, const float* locs_in,
                            const float* prize_in, const float* max_length_in, float* locs_out,
                            float* prize_out, float* max_length_out, float* tour_length,
                            float* total_prize, int64_t* cur, int64_t* i, uint8_t* visited,
                            uint8_t* mask, void*) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!depot || !locs_in || !prize_in || !max_length_in || !locs_out || !prize_out ||
      !max_length_out || !tour_length || !total_prize || !cur || !i || !visited || !mask)
    return CO_E_INVAL;
  if (op_mis8(depot) || op_mis8(locs_in) || op_mis8(locs_out)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    float *lo = locs_out + b * NC * 2, *po = prize_out + b * NC, *mo = max_length_out + b * NC;
    lo[0] = depot[2 * b];
    lo[1] = depot[2 * b + 1];
    std::memcpy(lo + 2, locs_in + b * N * 2, (size_t)N * 2 * sizeof(float));
    po[0] = 0.f;
    std::memcpy(po + 1, prize_in + b * N, (size_t)N * sizeof(float));
    for (int64_t c = 0; c < NC; ++c) {
      mo[c] = (max_length_in[b] - edge_len(lo[0], lo[1], lo[2 * c], lo[2 * c + 1])) - 1e-6f;
      visited[b * NC + c] = 0;
    }
    tour_length[b] = 0.f;
    total_prize[b] = 0.f;
    cur[b] = 0;
    i[b] = 0;
    op_row_mask(NC, lo, mo, visited + b * NC, 0.f, 0, mask + b * NC);
  }
  return CO_OK;
}

// op/env.py:74-108
CO_HOST_API int co_op_step(int64_t B, int64_t N, const int64_t* action, const float* locs,
                           const float* prize, const float* max_length,
                           const uint8_t* visited_in, uint8_t* visited_out, const float* tl_in,
                           float* tl_out, const float* pz_in, float* pz_out,
                           const int64_t* cur_in, int64_t* cur_out, const int64_t* i_in,
                           int64_t* i_out, uint8_t* done, uint8_t* reward, uint8_t* mask,
                           int32_t* status, void*) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!action || !locs || !prize || !max_length || !visited_in || !visited_out || !tl_in ||
      !tl_out || !pz_in || !pz_out || !cur_in || !cur_out || !i_in || !i_out || !done ||
      !reward || !mask)
    return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    const float* lr = locs + b * NC * 2;
    uint8_t* vis = visited_out + b * NC;
    for (int64_t c = 0; c < NC; ++c) vis[c] = visited_in[b * NC + c] != 0;
    float tl = tl_in[b], pz = pz_in[b];
    int64_t cur = cur_in[b], iv = i_in[b];
    if (!op_row_step(N, action[b], lr, prize + b * NC, vis, tl, pz, cur, iv, done[b]))
      set_status(status, CO_ST_INDEX_RANGE);
    tl_out[b] = tl, pz_out[b] = pz, cur_out[b] = cur, i_out[b] = iv;
    reward[b] = 0;
    op_row_mask(NC, lr, max_length + b * NC, vis, tl, cur, mask + b * NC);
  }
  return CO_OK;
}

// op/env.py:153-169
CO_HOST_API int co_op_action_mask(int64_t B, int64_t N, const float* locs,
                                  const float* max_length, const uint8_t* visited,
                                  const float* tour_length, const int64_t* cur, uint8_t* mask,
                                  void*) {
  if (!op_sizes_ok(B, N)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!locs || !max_length || !visited || !tour_length || !cur || !mask) return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b)
    op_row_mask(NC, locs + b * NC * 2, max_length + b * NC, visited + b * NC, tour_length[b],
                cur[b], mask + b * NC);
  return CO_OK;
}

// `steps` co_op_step calls; feasible: the mask's value for a_t before step t
CO_HOST_API int co_op_steps(int64_t B, int64_t N, int64_t T, const int64_t* actions, int64_t st,
                            int64_t sb, const float* locs, const float* prize,
                            const float* max_length, const uint8_t* mask_in, uint8_t* visited,
                            float* tour_length, float* total_prize, int64_t* cur, int64_t* i,
                            uint8_t* done, uint8_t* reward, uint8_t* mask, uint8_t* feasible,
                            float* length, int32_t* status, void*) {
  if (!op_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!actions || !locs || !prize || !max_length || !visited || !tour_length || !total_prize ||
      !cur || !i || !done || !reward || !mask || (feasible && !mask_in) || mask == mask_in)
    return CO_E_INVAL;
  if (op_mis8(locs)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  for (int64_t b = 0; b < B; ++b) {
    const float *lr = locs + b * NC * 2, *ml = max_length + b * NC;
    uint8_t* vis = visited + b * NC;
    for (int64_t c = 0; c < NC; ++c) vis[c] = vis[c] != 0;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[t * st + b * sb];
      const bool in = a >= 0 && a <= N;
      if (feasible)
        feasible[t * B + b] =
            in && (t == 0 ? mask_in[b * NC + a] != 0
                          : op_open(lr, ml, vis, tour_length[b], lr + 2 * op_clamp(cur[b], N), a));
      if (!op_row_step(N, a, lr, prize + b * NC, vis, tour_length[b], total_prize[b], cur[b],
                       i[b], done[b]))
        set_status(status, CO_ST_INDEX_RANGE);
      if (length) length[t * B + b] = tour_length[b];
    }
    reward[b] = 0;
    op_row_mask(NC, lr, ml, vis, tour_length[b], cur[b], mask + b * NC);
  }
  return CO_OK;
}

// op/env.py:171-214: the prize sum and, with check, the two validity tests in tour order
CO_HOST_API int co_op_reward(int64_t B, int64_t N, int64_t T, const float* prize, int64_t PB,
                             const float* locs, const float* max_length, int64_t LB,
                             const int64_t* actions, int64_t sb, int64_t st, int check,
                             float* reward, int32_t* status, void*) {
  if (!op_sizes_ok(B, N) || T < 1 || T > (1 << 20)) return CO_E_INVAL;
  if (PB <= 0 || (B > 0 && B % PB != 0)) return CO_E_INVAL;
  if (check && (LB <= 0 || (B > 0 && B % LB != 0))) return CO_E_INVAL;
  if (B == 0) return CO_OK;
  if (!prize || !actions || !reward || (check && (!locs || !max_length || !status)))
    return CO_E_INVAL;
  if (check && op_mis8(locs)) return CO_E_ALIGN;
  const int64_t NC = N + 1;
  std::vector<uint8_t> seen(check ? (size_t)NC : 0);
  for (int64_t b = 0; b < B; ++b) {
    const float* pr = prize + (b % PB) * NC;
    const float* lr = check ? locs + (b % LB) * NC * 2 : nullptr;
    bool dup = false, have = false, have0 = false;
    float px = 0.f, py = 0.f, fx = 0.f, fy = 0.f;
    double sum = 0.0, len = 0.0;
    if (check) std::fill(seen.begin(), seen.end(), 0);
    for (int64_t t = 0; t < T; ++t) {
      const int64_t a = actions[b * sb + t * st];
      const bool in = a >= 0 && a <= N;
      if (in)
        sum += (double)pr[a];
      else
        set_status(status, CO_ST_INDEX_RANGE);
      if (check) {
        float qx = 0.f, qy = 0.f;
        if (in) {
          qx = lr[2 * a], qy = lr[2 * a + 1];
          if (have) len += (double)edge_len(px, py, qx, qy);
          if (a != 0 && seen[a]) dup = true;
          seen[a] = 1;
        }
        if (t == 0) fx = qx, fy = qy, have0 = in;
        px = qx, py = qy, have = in;
      }
    }
    reward[b] = T == 1 ? 0.f : (float)sum;
    if (T == 1 && actions[b * sb] != 0) set_status(status, CO_ST_OP_SINGLE_NONZERO);
    if (!check) continue;
    if (dup) {
      set_status(status, CO_ST_OP_DUPLICATE);
      continue;
    }
    if (have && have0) len += (double)edge_len(px, py, fx, fy);
    const float flen = (float)len;
    const float* ml = max_length + (b % LB) * NC;
    bool over = false;
    for (int64_t c = 0; c < NC; ++c) {
      const float bound = ((ml[c] + edge_len(lr[0], lr[1], lr[2 * c], lr[2 * c + 1])) + 1e-6f) + 1e-5f;
      over |= !(flen <= bound);
    }
    if (over) set_status(status, CO_ST_OP_LENGTH);
  }
  return CO_OK;
}

CO_HOST_API const char* co_build_info(void) {
  return "rl4co_slap_amd co_env: host (CPU) build of the env / decode entry points";
}
