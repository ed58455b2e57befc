// The decode step fused with an env's transition (co_tsp_decode_step, co_slap_decode_step,
// co_cvrp_decode_step): one launcher for the three envs, one greedy body for TSP and CVRP and
// the sampling / evaluate body CVRP runs on, on the row engines of decode_common.hpp.  The
// kernels that missed the refactor's gates on these bodies keep their hand-written form:
// TSP's step kernel (decode_tsp.hip) and both SLAP kernels (decode_env.hip).  Included by
// decode_tsp.hip and decode_env.hip, which hold the env-step types and the kernels.
//
// The bodies own the frame (lane split, the wave's row group, the row engine) and the
// shared tail (status bits, action, logp, the log-likelihood sum).  They never branch on
// the env: what differs per env is the env-step type's (TspStep, CvrpStep), a small by-value
// struct with
//   static constexpr int kDiagCut      0, or a co_diag.hpp timing cut: 2 makes the greedy body
//                                      skip the decode, 1 is the env's own (no transition)
//   void fetch(base, B, grp, lead)     start fetching the state the transition reads, before
//                                      the logits and before the frame computes anything of
//                                      the row: the wave's row group [base, base + 64 / RL)
//                                      by LDS-DMA, or row base + grp into the registers of
//                                      the group's `lead` lane (the one store_row runs on)
//   bool apply(row, valid, r, grp, sl, c0, a, N, status)
//                                      group-wide (every lane of the wave calls it): action a
//                                      edits the mask, and the rows and state the lane group stores
//                                      together go out; a staged env waits for its stage
//                                      first.  false: a is out of the env's range
//   float* ll_out(), float ll_in(grp)  the log-likelihood accumulator (NULL: none) and the
//                                      row's fetched value
//   void store_row(r, grp, a)          lane 0 of a valid row: the row's remaining scalars
#pragma once
#include "decode_common.hpp"

namespace {

// Greedy (GreedyRow; certified / exact / fast per OPT): one row group per wave.
template <int RL, int EPL, int VW, int OPT, class Env>
__device__ __forceinline__ void fused_greedy_body(float* lds, int64_t B, int N, const float* logits,
                                                  int64_t lstride, const uint8_t* mask_in,
                                                  float clip, float temp, int64_t* action_out,
                                                  float* logp_sel, int32_t* status, Env env) {
  constexpr int RPW = 64 / RL;
  const int lane = lane_id(), sl = lane % RL, grp = lane / RL, c0 = sl * EPL;
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
  // one row group per wave: the grid covers B (no grid-stride loop, so no values are
  // hoisted into registers across row groups -- r04: certified 71 -> fewer VGPRs)
  const int64_t base = wid * RPW;
  if (base >= B) return;  // wave-uniform
  env.fetch(base, B, grp, sl == 0);
  const int64_t row = base + grp;
  const bool valid = row < B;
  const int64_t r = valid ? row : 0;
  GreedyRow<RL, EPL, VW> g;
  const float* lrow = logits + r * lstride;
  const uint8_t* mrow = mask_in + r * (int64_t)N;
  g.load(valid, N, lrow, mrow, c0);
  // The certified fallbacks read the raw row again (greedy_row).  On the long-row buckets
  // (EPL >= 16) they get a row pointer the optimizer cannot equate with lrow: there it folded
  // the second read into the first and kept the EPL raw logits live across the fast pass,
  // which cost four certified kernels an occupancy step (<64,32,3,9>: 122 -> 130 VGPRs).
  const float* lrow_again = lrow;
  if constexpr (EPL >= 16) asm("" : "+v"(lrow_again));
  float lp = 0.f, L = 0.f;
  int sel = (int)(row % N);
  if (Env::kDiagCut != 2)
    sel = greedy_row<OPT>(g, valid, N, clip, temp, sl, c0, group_scratch<RL, EPL>(lds, grp), L, lp,
                          lrow_again, mrow);
  else
    lp = g.v[0];  // keep the loads
  const bool feas0 = g.allowed(0);
  const bool ok = env.apply(g, valid, r, grp, sl, c0, sel, N, status);
  if (valid && sl == 0) {
    // L is finite or NaN (the exp-sum is >= 1 unless NaN); finite means the argmax
    // element is unmasked, NaN means index 0 was taken
    if (L != L && !feas0) set_status(status, CO_ST_INFEASIBLE);
    if (!ok) set_status(status, CO_ST_INDEX_RANGE);
    action_out[r] = sel;
    if (logp_sel) logp_sel[r] = lp;
    if (float* ll = env.ll_out()) ll[r] = env.ll_in(grp) + lp;  // get_log_likelihood's sum
    env.store_row(r, grp, (int64_t)sel);
  }
}

// Sampling / evaluate (DecodeRow, exact math unless fast): one row group per wave.  Written
// without a loop: inside a `#pragma unroll` loop of one iteration the optimizer hoisted the
// row's address arithmetic above the staged envs' LDS-DMA loops, where it stayed live (up to
// 21 VGPRs and an occupancy step).
template <int RL, int EPL, bool VEC, int OPT, class Env>
__device__ __forceinline__ void fused_step_body(float* lds, int64_t B, int N, const float* logits,
                                                int64_t lstride, const uint8_t* mask_in, float clip,
                                                float temp, int mode, const int64_t* action_in,
                                                int64_t* action_out, float* logp_sel, uint64_t seed,
                                                uint64_t offset, int32_t* status, Env env) {
  constexpr int RPW = 64 / RL;
  const int lane = lane_id(), sl = lane % RL, grp = lane / RL, c0 = sl * EPL;
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
  const int64_t base = wid * RPW;
  if (base >= B) return;  // wave-uniform
  env.fetch(base, B, grp, sl == 0);
  const int64_t row = base + grp;
  const bool valid = row < B;
  const int64_t r = valid ? row : 0;
  const int64_t a_in = (mode == CO_DECODE_EVALUATE && valid) ? action_in[r] : 0;
  DecodeRow<RL, EPL, VEC, OPT> d;
  d.run(valid, N, logits + r * lstride, mask_in + r * (int64_t)N, clip, temp, mode, a_in, seed,
        offset, row, sl, grp, group_scratch<RL, EPL>(lds, grp));
  const int64_t a = mode == CO_DECODE_EVALUATE ? a_in : (int64_t)d.sel;
  const bool ok = env.apply(d, valid, r, grp, sl, c0, a, N, status);
  if (valid && sl == 0) {
    if (mode == CO_DECODE_EVALUATE && (a_in < 0 || a_in >= N))
      set_status(status, CO_ST_INDEX_RANGE);  // the logp gather (decoding.py:365)
    if (mode != CO_DECODE_EVALUATE && !d.feas) set_status(status, CO_ST_INFEASIBLE);
    if (!ok) set_status(status, CO_ST_INDEX_RANGE);
    action_out[r] = a;
    if (logp_sel) logp_sel[r] = d.lp;
    if (float* ll = env.ll_out()) ll[r] = env.ll_in(grp) + d.lp;
    env.store_row(r, grp, a);
  }
}

// ---------------------------------------------------------------------------
// The host side of a fused entry point: the decode half's arguments, their checks, the
// dispatch of the env's two kernel families and the two-launch route.
template <int RL_, int EPL_, auto V_, int OPT_>
struct RowCfg {  // one dispatch case, handed to the entry point's launch callbacks
  static constexpr int RL = RL_, EPL = EPL_, OPT = OPT_;
  static constexpr auto V = V_;  // GreedyRow's load width / DecodeRow's VEC
};

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

struct FusedDecode {
  int64_t B, N;  // N: the row length
  const float* logits;
  int64_t lstride;
  const uint8_t* mask_in;
  float clip, temp;
  int mword;  // the entry point's mode word; `m` after parse()
  const int64_t* action_in;
  int64_t* action_out;
  float* logp_sel;
  uint64_t seed, offset;
  uint8_t* mask_out;
  int32_t* status;
  void* stream;
  DecodeMode m{};

  bool parse() { return m.parse(mword); }
  bool pointers_ok() const {
    return logits && mask_in && action_out && mask_out &&
           (m.mode != CO_DECODE_EVALUATE || action_in);
  }
  int rows_per_wave() const { return row_bucket(N).rows_per_wave(); }
  // does a stage of `dwords` per wave fit beside the row engines' static LDS?
  static size_t stage_bytes(int dwords) { return (size_t)4 * dwords * 4; }
  bool stage_fits(int dwords) const {
    return stage_bytes(dwords) + (size_t)4 * 64 * row_bucket(N).greedy_epl() * 4 <= 64 * 1024;
  }

  // greedy(RowCfg, grid) / step(RowCfg, grid) launch the env's kernel of that case on
  // 256-thread blocks.  step_unr: the step kernels' UNR; vec_store_ok: the env's own
  // condition on the step kernels' VEC path (DecodeRow::store_mask needs a 4-byte aligned
  // mask row).
  template <class G, class S>
  int launch(int step_unr, bool vec_store_ok, G greedy, S step) const {
    const float clip = this->clip, temp = this->temp;
    const bool cert = m.cert, fast = m.fast;
    const int64_t N = this->N;
#define CO_FUSED_CALL(F, RL, EPL, V) F(RowCfg<RL, EPL, V, OPT>{}, grid)
    if (m.mode == CO_DECODE_GREEDY) {
      const dim3 grid(decode_grid(B, (int)N));
      if (grid.x == 0) return CO_E_INVAL;
#define CO_FUSED_G(RL, EPL, V) \
  CO_OPT_DISPATCH_G(CO_FUSED_CALL, greedy, RL, (EPL < 4 ? 4 : EPL), V)
      switch (greedy_vw(N, lstride, logits, mask_in, mask_out, nullptr)) {
        case 4: CO_ROW_DISPATCH(CO_FUSED_G, 4); break;
        case 2: CO_ROW_CASE(CO_FUSED_G, 2, 0); break;  // N < 4
        default: CO_ROW_DISPATCH(CO_FUSED_G, 3);
      }
#undef CO_FUSED_G
      return launch_status();
    }
    const dim3 grid(decode_grid(B, (int)N, step_unr));
    if (grid.x == 0) return CO_E_INVAL;
#define CO_FUSED_S(RL, EPL, V) CO_OPT_DISPATCH(CO_FUSED_CALL, step, RL, EPL, V)
    if (decode_vec_ok(logits, lstride, mask_in, N) && vec_store_ok) {
      CO_ROW_DISPATCH(CO_FUSED_S, true);
    } else {
      CO_ROW_DISPATCH(CO_FUSED_S, false);
    }
#undef CO_FUSED_S
#undef CO_FUSED_CALL
    return launch_status();
  }

  // The two launches the fused step replaces (a stage beyond the LDS, misaligned state):
  // co_decode_step, then env_step(actions) = the env's own step entry point.  There is no
  // log-likelihood accumulation on this route.
  template <class F>
  int two_launches(const float* ll_accum, F env_step) const {
    if (ll_accum) return CO_E_INVAL;
    const int rc = co_decode_step(B, N, logits, lstride, mask_in, clip, temp, mword, action_in,
                                  action_out, logp_sel, nullptr, seed, offset, status, stream);
    if (rc != CO_OK) return rc;
    return env_step(m.mode == CO_DECODE_EVALUATE ? action_in : action_out);
  }
};

}  // namespace
