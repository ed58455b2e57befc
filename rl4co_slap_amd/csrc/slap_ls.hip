// Batched local search for SLAP assignments (co_slap_local_search; SLAPEnv.improve) for
// gfx950: best-improvement move-to-free-slot + product swap on the exact integer QAP
// objective.  include/co_env.h states the search; tests/slap_ls_ref.py restates it in numpy.
//
// Layout: as tsp_ls.hip and cvrp_ls.hip, one wavefront (a 64-thread workgroup) owns one row
// for its whole search.  LDS holds
//   W[a][c]  the flow counts, uint16 (W <= O * (K / 2) <= 32768), rows padded to an even
//            length and built from the picklist with 32-bit LDS adds of 1 << 16 * (c & 1)
//   s[p]     the slot of product p        occ  one bit per slot: a product sits there
//   XY[l]    the coordinates (coordinate path); a matrix is read through L2
//   C[p][l]  the QAP table, int64 (table scheme: where CO_SLAP_LS_TABLE_FITS(P, L))
// Q[u][v] = llrint(D[u][v] * 2^20) is never stored: it is one distance (coordinates: a
// sqrt) and one f64 multiply + convert where it is needed.
//
// With c(p, l) = sum_r W[p][r] Q[l][s_r] + W[r][p] Q[s_r][l] (W[p][p] = 0: s_p does not
// enter), a move (p, x) changes F by c(p, x) - c(p, s_p) and a swap (p, q), a = s_p,
// b = s_q, by c(p, b) - c(p, a) + c(q, a) - c(q, b)
//            + (W[p][q] + W[q][p]) (Q[a][b] + Q[b][a] - Q[a][a] - Q[b][b]).
// The table scheme reads c from C, the direct scheme sums its O(P) terms per use; every
// term is an exact int64, so the two give the same bits.  After p: a -> x is applied,
//   C[r][l] += W[r][p] (Q[l][x] - Q[l][a]) + W[p][r] (Q[x][l] - Q[a][l]),
// and a swap is that with the coefficients W[r][p] - W[r][q] and W[p][r] - W[q][r]: lane r
// reads row r's two coefficients once, then a lane owns column l, computes the two Q
// differences once and walks the rows r whose coefficients (v_readlane) are not both zero.
//
// A sweep walks the moves product by product (p wave-uniform, a lane per slot x, 64 slots a
// pass) and the swaps as the P * P square (a lane per (p, q), 64 a pass, p < q kept).  A
// lane meets its candidates in ascending key order (kind << 30 | p << 16 | x), so a strict
// `<` keeps the lowest key of equal changes; the wave reduction is an int64 min and then
// the min key among the lanes that hold it.
#include "co_local_search.hpp"

using namespace co;

namespace {

constexpr int kMatrix = 1;  // beside kCoords: a matrix, read through L2
constexpr int kSwap = 1 << 30;

constexpr int round8(int x) { return (x + 7) & ~7; }
// the LDS bytes of a row's state; never above the header's bound, which decides the scheme
constexpr int lds_bytes(int P, int L, int mode, bool table) {
  return (table ? 8 * P * L : 0) + (mode == kCoords ? 8 * L : 0) + round8(4 * P) +
         round8(4 * ((L + 31) >> 5)) + round8(2 * P * (P + (P & 1)));
}
constexpr bool bound_holds(int P, int L) {
  return lds_bytes(P, L, kCoords, false) <= CO_SLAP_LS_STATE_BYTES(P, L);
}
static_assert(bound_holds(1, 1) && bound_holds(1, 1024) && bound_holds(127, 127) &&
                  bound_holds(127, 1023) && bound_holds(128, 1024),
              "CO_SLAP_LS_STATE_BYTES must bound the state without the table");
static_assert(CO_SLAP_LS_STATE_BYTES(CO_SLAP_LS_MAX_PRODUCTS, CO_SLAP_LS_MAX_SLOTS) <=
                  CO_SLAP_LS_LDS_BYTES && CO_SLAP_LS_LDS_BYTES <= 64 * 1024,
              "the direct scheme's state must fit 64 KiB of LDS at the maximum sizes");
static_assert(CO_SLAP_LS_MAX_PRODUCTS <= 128, "a lane holds the update coefficients of two rows");
static_assert(CO_SLAP_LS_MAX_PRODUCTS < (1 << 14) && CO_SLAP_LS_MAX_SLOTS < (1 << 16),
              "move keys pack p into 14 bits, x into 16");

__device__ __forceinline__ int64_t quantise(float d) {
  return __double2ll_rn((double)d * 1048576.0);  // llrint(d * 2^20)
}

template <int MODE, bool TABLE>
__global__ __launch_bounds__(64) void slap_ls_kernel(
    int64_t B, int P, int L, int OK, int K, const float* __restrict__ src, int64_t LB,
    const int64_t* __restrict__ picklist, const int32_t* __restrict__ assignment, int max_it,
    int32_t* __restrict__ out, int32_t* __restrict__ sweeps, int64_t* __restrict__ cost,
    int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int Pp = P + (P & 1);  // W's row length
  unsigned char* at = s_raw;
  [[maybe_unused]] int64_t* C = reinterpret_cast<int64_t*>(at);  // TABLE: P * L
  if constexpr (TABLE) at += 8 * P * L;
  [[maybe_unused]] float2* XY = reinterpret_cast<float2*>(at);  // kCoords: L
  if constexpr (MODE == kCoords) at += 8 * L;
  int* s = reinterpret_cast<int*>(at);
  at += round8(4 * P);
  uint32_t* occ = reinterpret_cast<uint32_t*>(at);
  at += round8(4 * ((L + 31) >> 5));
  uint32_t* W32 = reinterpret_cast<uint32_t*>(at);
  const uint16_t* W = reinterpret_cast<const uint16_t*>(at);
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int32_t* arow = assignment + b * (int64_t)P;
    int32_t* orow = out + b * (int64_t)P;
    const int64_t inst = LB == B ? b : b % LB;
    const int64_t* pl = picklist + inst * (int64_t)OK;
    [[maybe_unused]] const float* Dg = src + inst * (int64_t)L * L;  // kMatrix
    __syncthreads();  // the previous row's LDS reads are done
    for (int k = lane; k < ((L + 31) >> 5); k += 64) occ[k] = 0;
    for (int k = lane; k < ((P * Pp) >> 1); k += 64) W32[k] = 0;
    __syncthreads();
    // ---- the row check, filling s, occ, W and the coordinates
    bool bad = false, bad_pl = false;
    for (int p = lane; p < P; p += 64) {
      const int v = arow[p];
      if (v < 0 || v >= L) {
        bad = true;
      } else {
        s[p] = v;
        if (mark_once(occ, v)) bad = true;
      }
    }
    for (int idx = lane; idx < OK; idx += 64) {
      const int k = idx % K;
      const int64_t a = pl[idx], c = pl[k + 1 == K ? idx - k : idx + 1];
      if (a < 0 || a >= P) {
        bad_pl = true;
      } else if (c >= 0 && c < P && a != c) {
        const int e = (int)a * Pp + (int)c;
        atomicAdd(&W32[e >> 1], 1u << ((e & 1) << 4));
      }
    }
    if constexpr (MODE == kCoords) {
      const float2* lr = reinterpret_cast<const float2*>(src) + inst * (int64_t)L;
      for (int l = lane; l < L; l += 64) {
        const float2 xy = lr[l];
        XY[l] = xy;
        bad |= !(fabsf(xy.x) <= 262144.f && fabsf(xy.y) <= 262144.f);  // no NaN, no inf
      }
    } else {
      for (int k = lane; k < L * L; k += 64) {
        const float d = Dg[k];
        bad |= !(d >= 0.f && d <= 1048576.f);
      }
    }
    bad = __any(bad);
    bad_pl = __any(bad_pl);
    if (bad || bad_pl) {  // wave-uniform: the row is copied
      if (lane == 0)
        set_status(status, (bad ? CO_ST_INVALID_TOUR : 0) | (bad_pl ? CO_ST_INDEX_RANGE : 0));
      for (int p = lane; p < P; p += 64) orow[p] = arow[p];
      if (lane == 0) {
        if (sweeps) sweeps[b] = 0;
        if (cost) cost[b] = -1;
      }
      continue;
    }
    __syncthreads();
    // Q[u][v] for slots u, v < L
    auto qd = [&](int u, int v) -> int64_t {
      if constexpr (MODE == kCoords) {
        const float2 a = XY[u], c = XY[v];
        return quantise(edge_len(a.x, a.y, c.x, c.y));
      } else {
        return quantise(Dg[u * L + v]);
      }
    };
    // c(p, l) from its O(P) terms
    auto cdirect = [&](int p, int l) -> int64_t {
      int64_t acc = 0;
      for (int r = 0; r < P; ++r) {
        const int64_t w1 = W[p * Pp + r], w2 = W[r * Pp + p];
        if ((w1 | w2) == 0) continue;
        const int sr = s[r];
        if constexpr (MODE == kCoords)
          acc += (w1 + w2) * qd(l, sr);  // dx*dx + dy*dy: symmetric to the bit
        else
          acc += w1 * qd(l, sr) + w2 * qd(sr, l);
      }
      return acc;
    };
    auto cval = [&](int p, int l) -> int64_t {
      if constexpr (TABLE)
        return C[p * L + l];
      else
        return cdirect(p, l);
    };
    if constexpr (TABLE) {
      for (int p = 0; p < P; ++p)
        for (int l = lane; l < L; l += 64) C[p * L + l] = cdirect(p, l);
      __syncthreads();
    }
    const int p0 = lane / P, q0 = lane - p0 * P;  // the swap square's per-lane start
    const int step_p = 64 / P, step_q = 64 - step_p * P;
    int it = 0;
    while (it < max_it) {
      int64_t best = 0;  // only a change < 0 counts
      int bkey = 0x7fffffff;
      for (int p = 0; p < P; ++p) {
        const int a = s[p];
        const int64_t ca = cval(p, a);
        for (int x0 = 1; x0 < L; x0 += 64) {
          const int x = x0 + lane;
          if (x < L && !((occ[x >> 5] >> (x & 31)) & 1)) {
            const int64_t d = cval(p, x) - ca;
            if (d < best) {
              best = d;
              bkey = (p << 16) | x;
            }
          }
        }
      }
      int p = p0, q = q0;
      for (int t0 = 0; t0 < P * P; t0 += 64) {
        if (t0 + lane < P * P && p < q) {
          const int a = s[p], c = s[q];
          int64_t d = (cval(p, c) - cval(p, a)) + (cval(q, a) - cval(q, c));
          const int64_t w = (int64_t)W[p * Pp + q] + (int64_t)W[q * Pp + p];
          if (w != 0) {
            if constexpr (MODE == kCoords)
              d += w * (2 * qd(a, c));  // Q[a][a] = 0 and Q is symmetric
            else
              d += w * (((qd(a, c) + qd(c, a)) - qd(a, a)) - qd(c, c));
          }
          if (d < best) {
            best = d;
            bkey = kSwap | (p << 16) | q;
          }
        }
        p += step_p;
        q += step_q;
        if (q >= P) {
          q -= P;
          ++p;
        }
      }
      int64_t m = best;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int64_t o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
      }
      const int key = wave_min_int(best == m ? bkey : 0x7fffffff);
      ++it;
      if (m >= 0) break;  // nothing applied: the search ends
      const int mp = (key >> 16) & 0x3fff, mx = key & 0xffff;
      const bool swap = (key & kSwap) != 0;
      const int a = s[mp];                // p leaves slot a ...
      const int x = swap ? s[mx] : mx;    // ... for slot x, which product mx gives up in a swap
      __syncthreads();
      if constexpr (TABLE) {
        // lanes r and r - 64 hold row r's two coefficients; the row loop broadcasts them
        int c1v[2], c2v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r = lane + 64 * h;
          int c1 = 0, c2 = 0;
          if (r < P) {
            c1 = W[r * Pp + mp];
            c2 = W[mp * Pp + r];
            if (swap) {
              c1 -= W[r * Pp + mx];
              c2 -= W[mx * Pp + r];
            }
          }
          c1v[h] = c1;
          c2v[h] = c2;
        }
        // every lane runs every pass: the broadcast reads lanes that own no column in it
        for (int l0 = 0; l0 < L; l0 += 64) {
          const bool live = l0 + lane < L;
          const int l = live ? l0 + lane : L - 1;
          const int64_t dcol = qd(l, x) - qd(l, a);
          int64_t drow = dcol;
          if constexpr (MODE != kCoords) drow = qd(x, l) - qd(a, l);
          for (int r = 0; r < P; ++r) {
            const int c1 = __builtin_amdgcn_readlane(r < 64 ? c1v[0] : c1v[1], r & 63);
            const int c2 = __builtin_amdgcn_readlane(r < 64 ? c2v[0] : c2v[1], r & 63);
            if ((c1 | c2) == 0) continue;  // wave-uniform
            if (live) C[r * L + l] += (int64_t)c1 * dcol + (int64_t)c2 * drow;
          }
        }
      }
      if (lane == 0) {
        s[mp] = x;
        if (swap) {
          s[mx] = a;
        } else {
          occ[a >> 5] &= ~(1u << (a & 31));
          occ[x >> 5] |= 1u << (x & 31);
        }
      }
      __syncthreads();
    }
    for (int k = lane; k < P; k += 64) orow[k] = s[k];
    if (sweeps && lane == 0) sweeps[b] = it;
    if (cost) {  // F of the returned row
      int64_t f = 0;
      for (int a = 0; a < P; ++a)
        for (int c = lane; c < P; c += 64) {
          const int64_t w = W[a * Pp + c];
          if (w != 0) f += w * qd(s[a], s[c]);
        }
      f = wave_sum(f);
      if (lane == 0) cost[b] = f;
    }
  }
}

}  // namespace

extern "C" int co_slap_local_search_scheme(int64_t B, int64_t L, int64_t P, int64_t O, int64_t K,
                                           const float* locs, const float* distances,
                                           int64_t locs_batch, const int64_t* picklist,
                                           const int32_t* assignment, int64_t max_iterations,
                                           int32_t* assign_out, int32_t* sweeps_out,
                                           int64_t* cost_out, int32_t scheme, int32_t* status,
                                           void* stream) {
  if (P < 1 || P > CO_SLAP_LS_MAX_PRODUCTS || L < P || L > CO_SLAP_LS_MAX_SLOTS)
    return CO_E_INVAL;
  if (O < 1 || K < 1 || O > 65536 || K > 65536 || O * K > 65536) return CO_E_INVAL;
  if (scheme != CO_SLAP_LS_AUTO && scheme != CO_SLAP_LS_DIRECT && scheme != CO_SLAP_LS_TABLE)
    return CO_E_INVAL;
  const bool fits = CO_SLAP_LS_TABLE_FITS(P, L);
  if (scheme == CO_SLAP_LS_TABLE && !fits) return CO_E_INVAL;
  const int rc = check_search_args(
      B, locs_batch, locs, distances,
      picklist && assignment && assign_out && assign_out != assignment && status,
      !((reinterpret_cast<uintptr_t>(picklist) | reinterpret_cast<uintptr_t>(cost_out)) & 7));
  if (rc != CO_OK || B == 0) return rc;
  const bool table = scheme == CO_SLAP_LS_TABLE || (scheme == CO_SLAP_LS_AUTO && fits);
  const int p = (int)P, l = (int)L, ok = (int)(O * K), k = (int)K;
  const int max_it = clamp_iterations(max_iterations);
  if (lds_bytes(p, l, kCoords, table) > CO_SLAP_LS_LDS_BYTES) return CO_E_INVAL;  // cannot be
  const dim3 grid = row_grid(B);
  hipStream_t s = (hipStream_t)stream;
#define CO_SLAP_LS(MODE, TABLE, SRC)                                                           \
  hipLaunchKernelGGL((slap_ls_kernel<MODE, TABLE>), grid, dim3(64),                            \
                     (size_t)lds_bytes(p, l, MODE, TABLE), s, B, p, l, ok, k, SRC, locs_batch, \
                     picklist, assignment, max_it, assign_out, sweeps_out, cost_out, status)
  if (locs) {
    if (table) CO_SLAP_LS(kCoords, true, locs);
    else CO_SLAP_LS(kCoords, false, locs);
  } else if (table) {
    CO_SLAP_LS(kMatrix, true, distances);
  } else {
    CO_SLAP_LS(kMatrix, false, distances);
  }
#undef CO_SLAP_LS
  return launch_status();
}

extern "C" int co_slap_local_search(int64_t B, int64_t L, int64_t P, int64_t O, int64_t K,
                                    const float* locs, const float* distances,
                                    int64_t locs_batch, const int64_t* picklist,
                                    const int32_t* assignment, int64_t max_iterations,
                                    int32_t* assign_out, int32_t* sweeps_out, int64_t* cost_out,
                                    int32_t* status, void* stream) {
  return co_slap_local_search_scheme(B, L, P, O, K, locs, distances, locs_batch, picklist,
                                     assignment, max_iterations, assign_out, sweeps_out,
                                     cost_out, CO_SLAP_LS_AUTO, status, stream);
}
