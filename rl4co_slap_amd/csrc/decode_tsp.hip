// co_tsp_decode_step: the decode step fused with TSPEnv._step (decode_fused.hpp bodies).
// The row's logits and action_mask are read once; the selected action's env transition
// (tsp/env.py:67-93) is applied by the same lane group: mask_out = mask_in minus the
// action, done = nothing left (group ballot), i + 1, first_node.  654 B per TSP-100
// row-step.
#include "decode_fused.hpp"

namespace {

// The env-step type of TSP: the row's scalars go into registers before the logits.
struct TspStep {
  static constexpr int kDiagCut = 0;
  uint8_t* mask_out;
  const int64_t* i_in;
  int64_t* i_out;
  const int64_t* first_in;
  int64_t* first_out;
  int take_first;
  uint8_t* done;
  uint8_t* step_reward;
  float* ll_accum;
  int64_t iv = 0, fv = 0;
  float acc = 0.f;
  bool left = false;  // an action of the row is still allowed after this one

  __device__ __forceinline__ void fetch(int64_t base, int64_t B, int grp, bool lead) {
    const int64_t r = base + grp;
    if (r >= B || !lead) return;
    iv = i_in[r];
    if (!take_first) fv = first_in[r];
    if (ll_accum) acc = ll_accum[r];
  }
  // the selected byte leaves the mask words in registers, the row is stored back
  template <int RL, int EPL, int VW>
  __device__ __forceinline__ bool apply(GreedyRow<RL, EPL, VW>& g, bool valid, int64_t r, int grp,
                                        int, int c0, int a, int N, int32_t*) {
    const unsigned long long gmask = RL == 64 ? ~0ull : (((1ull << RL) - 1ull) << (grp * RL));
    g.clear(a, c0);
    const bool any = g.any_allowed();
    if (valid) g.store_mask(N, mask_out + r * (int64_t)N, c0);
    left = (__ballot(any) & gmask) != 0;
    return true;
  }
  __device__ __forceinline__ float* ll_out() const { return ll_accum; }
  __device__ __forceinline__ float ll_in(int) const { return acc; }
  __device__ __forceinline__ void store_row(int64_t r, int, int64_t a) const {
    i_out[r] = iv + 1;
    first_out[r] = take_first ? a : fv;
    done[r] = !left;
    step_reward[r] = 0;
  }
};

// Greedy on the GreedyRow engine (the POMO / multistart-greedy hot loop); same outputs as
// tsp_decode_step_kernel in greedy mode.
template <int RL, int EPL, int VW, int OPT>
__global__ __launch_bounds__(256) void tsp_decode_greedy_kernel(
    int64_t B, int N, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, uint8_t* __restrict__ mask_out, const int64_t* __restrict__ i_in,
    int64_t* __restrict__ i_out, const int64_t* __restrict__ first_in,
    int64_t* __restrict__ first_out, int take_first, uint8_t* __restrict__ done,
    uint8_t* __restrict__ step_reward, float* __restrict__ ll_accum, int32_t* status) {
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  fused_greedy_body<RL, EPL, VW, OPT>(
      lds, B, N, logits, lstride, mask_in, clip, temp, action_out, logp_sel, status,
      TspStep{mask_out, i_in, i_out, first_in, first_out, take_first, done, step_reward, ll_accum});
}

// Sampling / evaluate: this kernel keeps its hand-written form, instruction for instruction
// (its machine code is the parent's, byte for byte, so it needs no speed gate).  On
// decode_fused.hpp's step body (with TspStep) eleven of its instantiations on the 64-lane
// buckets lost an occupancy step (e.g. <64,32,true,4>: 112 -> 133 VGPRs): the mask edit as
// two passes (clear, then any-left) instead of the one loop below accounts for most of it;
// with DecodeRow::store_mask alone 96 instantiations still changed code.  UNR rows per lane
// group (CO_DECODE_UNR): plain geometry.
template <int RL, int EPL, bool VEC, int OPT, int UNR = CO_DECODE_UNR>
__global__ __launch_bounds__(256) void tsp_decode_step_kernel(
    int64_t B, int N, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int mode,
    const int64_t* __restrict__ action_in, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, uint64_t seed, uint64_t offset, uint8_t* __restrict__ mask_out,
    const int64_t* __restrict__ i_in, int64_t* __restrict__ i_out,
    const int64_t* __restrict__ first_in, int64_t* __restrict__ first_out, int take_first,
    uint8_t* __restrict__ done, uint8_t* __restrict__ step_reward, float* __restrict__ ll_accum,
    int32_t* status) {
  constexpr int RPW = 64 / RL;
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  const int lane = lane_id(), sl = lane % RL, grp = lane / RL;
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
  const unsigned long long gmask = RL == 64 ? ~0ull : (((1ull << RL) - 1ull) << (grp * RL));
  // one row group of UNR rows per lane group per wave (the grid covers B); every load of
  // all UNR rows (logits, mask, i, first_node, action, ll accumulator) is issued before
  // any row's math
  const int64_t base = wid * RPW * UNR;
  if (base >= B) return;  // wave-uniform
  DecodeRow<RL, EPL, VEC, OPT> d[UNR];
  int64_t rr[UNR], ain[UNR], iv[UNR], fv[UNR];
  bool vv[UNR];
  float acc[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int64_t row = base + u * RPW + grp;
    vv[u] = row < B;
    rr[u] = vv[u] ? row : 0;
    ain[u] = (mode == CO_DECODE_EVALUATE && vv[u]) ? action_in[rr[u]] : 0;
    iv[u] = vv[u] ? i_in[rr[u]] : 0;
    fv[u] = (vv[u] && !take_first) ? first_in[rr[u]] : 0;
    acc[u] = (vv[u] && ll_accum) ? ll_accum[rr[u]] : 0.f;
    d[u].load(vv[u], N, logits + rr[u] * lstride, mask_in + rr[u] * (int64_t)N, sl);
  }
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const bool valid = vv[u];
    const int64_t r = rr[u], a_in = ain[u];
    d[u].compute(valid, N, clip, temp, mode, a_in, seed, offset, base + u * RPW + grp, sl,
                 grp, group_scratch<RL, EPL>(lds, grp));
    bool any_left = false;
    uint8_t* orow = mask_out + r * (int64_t)N;
    const int c0 = sl * EPL;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (c0 + k == d[u].sel) d[u].mk[k] = 0;
      any_left |= (valid && c0 + k < N && d[u].mk[k] != 0);
    }
    if (VEC) {
#pragma unroll
      for (int j = 0; j < EPL / 4; ++j)
        if (valid && c0 + 4 * j < N)
          *reinterpret_cast<uint32_t*>(orow + c0 + 4 * j) =
              (uint32_t)d[u].mk[4 * j] | ((uint32_t)d[u].mk[4 * j + 1] << 8) |
              ((uint32_t)d[u].mk[4 * j + 2] << 16) | ((uint32_t)d[u].mk[4 * j + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (valid && c0 + k < N) orow[c0 + k] = d[u].mk[k];
    }
    const bool left = (__ballot(any_left) & gmask) != 0;
    if (valid && sl == 0) {
      if (mode == CO_DECODE_EVALUATE && (a_in < 0 || a_in >= N))
        set_status(status, CO_ST_INDEX_RANGE);
      if (mode != CO_DECODE_EVALUATE && !d[u].feas) set_status(status, CO_ST_INFEASIBLE);
      const int64_t a = mode == CO_DECODE_EVALUATE ? a_in : (int64_t)d[u].sel;
      action_out[r] = a;
      if (logp_sel) logp_sel[r] = d[u].lp;
      if (ll_accum) ll_accum[r] = acc[u] + d[u].lp;  // get_log_likelihood's sum, per step
      i_out[r] = iv[u] + 1;
      first_out[r] = take_first ? a : fv[u];
      done[r] = !left;
      step_reward[r] = 0;
    }
  }
}

}  // namespace

extern "C" int co_tsp_decode_step(int64_t B, int64_t N, const float* logits, int64_t lstride,
                                  const uint8_t* mask_in, float clip, float temp, int mode,
                                  const int64_t* action_in, int64_t* action_out,
                                  float* logp_sel, uint64_t seed, uint64_t offset,
                                  uint8_t* mask_out, const int64_t* i_in, int64_t* i_out,
                                  const int64_t* first_in, int64_t* first_out, int first_mode,
                                  uint8_t* done, uint8_t* step_reward, float* ll_accum,
                                  int32_t* status, void* stream) {
  if (B < 0 || N <= 0 || N > 64 * 32) return CO_E_INVAL;
  FusedDecode f{B,         N,          logits,   lstride, mask_in, clip,     temp,   mode,
                action_in, action_out, logp_sel, seed,    offset,  mask_out, status, stream};
  if (!f.parse() || first_mode < 0 || first_mode > 1) return CO_E_MODE;
  if (B == 0) return CO_OK;
  if (!f.pointers_ok() || !i_in || !i_out || !first_out || !done || !step_reward ||
      (first_mode == 0 && !first_in))
    return CO_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
  return f.launch(
      CO_DECODE_UNR, aligned4(mask_out),
      [&](auto c, dim3 grid) {
        using C = decltype(c);
        hipLaunchKernelGGL((tsp_decode_greedy_kernel<C::RL, C::EPL, C::V, C::OPT>), grid, dim3(256),
                           0, s, B, (int)N, logits, lstride, mask_in, clip, temp, action_out,
                           logp_sel, mask_out, i_in, i_out, first_in, first_out, first_mode, done,
                           step_reward, ll_accum, status);
      },
      [&](auto c, dim3 grid) {
        using C = decltype(c);
        hipLaunchKernelGGL((tsp_decode_step_kernel<C::RL, C::EPL, C::V, C::OPT>), grid, dim3(256), 0,
                           s, B, (int)N, logits, lstride, mask_in, clip, temp, f.m.mode, action_in,
                           action_out, logp_sel, seed, offset, mask_out, i_in, i_out, first_in,
                           first_out, first_mode, done, step_reward, ll_accum, status);
      });
}
