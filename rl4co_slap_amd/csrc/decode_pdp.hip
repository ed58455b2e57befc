// co_pdp_decode_step: the decode step fused with PDPEnv._step (decode_fused.hpp bodies).  The
// row's logits and action_mask are read once; the selected action's transition
// (pdp/env.py:67-106) is applied by the same lane group on the row's two byte rows, which
// every lane fetched for its own columns before the logits: available minus the action,
// to_deliver plus the pair, mask_out = available & to_deliver (never an edit of mask_in: the
// reset mask is not that product), done = nothing available (group ballot), i + 1,
// current_node.  1,048 B per PDP-100 row-step (include/co_env.h).
//
// N + 1 is odd, so the 16-byte / 4-byte aligned row engines (GreedyRow's VW = 4, DecodeRow's
// VEC) never apply: only the byte-wise cases are instantiated and dispatched (VW = 3, VW = 2
// for the row of three, VEC = false).
#include "decode_fused.hpp"

namespace {

// The env-step type of PDP (decode_fused.hpp): lane sl of the row's group keeps its EPL
// columns of both byte rows as EPL / 4 words each.
template <int RL, int EPL>
struct PdpStep {
  static constexpr int kDiagCut = 0;
  static constexpr int W = EPL / 4;
  const uint8_t *av_in, *td_in;
  uint8_t *av_out, *td_out, *mask_out;
  const int64_t* i_in;
  int64_t *i_out, *cur_out;
  uint8_t *done, *step_reward;
  float* ll_accum;
  int NC;
  uint32_t av[W] = {}, td[W] = {};
  int64_t iv = 0;
  float acc = 0.f;
  bool left = false;  // a column of the row is still available after this action

  __device__ __forceinline__ void fetch(int64_t base, int64_t B, int grp, bool lead) {
    using M = typename Chunk<3>::M;
    const int64_t r = base + grp;
    if (r >= B) return;
    const int c0 = (lane_id() % RL) * EPL;
    const uint8_t *arow = av_in + r * (int64_t)NC, *trow = td_in + r * (int64_t)NC;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int c = c0 + 4 * j;
      if (c + 4 <= NC) {
        av[j] = *reinterpret_cast<const M*>(arow + c);
        td[j] = *reinterpret_cast<const M*>(trow + c);
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (c + q < NC) {
            av[j] |= (uint32_t)arow[c + q] << (8 * q);
            td[j] |= (uint32_t)trow[c + q] << (8 * q);
          }
      }
    }
    if (!lead) return;
    iv = i_in[r];
    if (ll_accum) acc = ll_accum[r];
  }

  // a non-zero byte -> 1 (co_pdp_step's reading of its input rows)
  __device__ __forceinline__ static uint32_t flags(uint32_t x) {
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
  }

  template <class Row, class A>
  __device__ __forceinline__ bool apply(Row&, bool valid, int64_t r, int grp, int, int c0, A a_raw,
                                        int, int32_t*) {
    using M = typename Chunk<3>::M;
    const unsigned long long gmask = RL == 64 ? ~0ull : (((1ull << RL) - 1ull) << (grp * RL));
    const int64_t a64 = (int64_t)a_raw;
    const bool bad = a64 < 0 || a64 >= NC;
    const int a = bad ? -8 : (int)a64;
    int pr = a + (NC - 1) / 2;
    pr = bad ? -8 : (pr >= NC ? pr - NC : pr);
    uint8_t *adst = av_out + r * (int64_t)NC, *tdst = td_out + r * (int64_t)NC,
            *mdst = mask_out + r * (int64_t)NC;
    uint32_t any = 0u;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int c = c0 + 4 * j;
      uint32_t x = flags(av[j]), y = flags(td[j]);
      const int oa = a - c, op = pr - c;
      if ((unsigned)oa < 4u) x &= ~(0xffu << (8 * oa));
      if ((unsigned)op < 4u) y |= 1u << (8 * op);
      any |= x;
      const uint32_t m = x & y;
      if (valid && c + 4 <= NC) {
        *reinterpret_cast<M*>(adst + c) = (M)x;
        *reinterpret_cast<M*>(tdst + c) = (M)y;
        *reinterpret_cast<M*>(mdst + c) = (M)m;
      } else if (valid && c < NC) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (c + q < NC) {
            adst[c + q] = (uint8_t)(x >> (8 * q));
            tdst[c + q] = (uint8_t)(y >> (8 * q));
            mdst[c + q] = (uint8_t)(m >> (8 * q));
          }
      }
    }
    left = (__ballot(valid && any != 0u) & gmask) != 0;
    return !bad;
  }
  __device__ __forceinline__ float* ll_out() const { return ll_accum; }
  __device__ __forceinline__ float ll_in(int) const { return acc; }
  __device__ __forceinline__ void store_row(int64_t r, int, int64_t a) const {
    i_out[r] = iv + 1;
    cur_out[r] = a;
    done[r] = !left;
    step_reward[r] = 0;
  }
};

struct PdpEpi {  // the env half's arguments
  const uint8_t *av_in, *td_in;
  uint8_t *av_out, *td_out, *mask_out;
  const int64_t* i_in;
  int64_t *i_out, *cur_out;
  uint8_t *done, *step_reward;
  float* ll_accum;
  int NC;
  template <int RL, int EPL>
  __device__ __forceinline__ PdpStep<RL, EPL> step() const {
    return {av_in, td_in, av_out, td_out, mask_out, i_in, i_out, cur_out, done, step_reward,
            ll_accum, NC};
  }
};

template <int RL, int EPL, int VW, int OPT>
__global__ __launch_bounds__(256) void pdp_decode_greedy_kernel(
    int64_t B, int NC, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, int32_t* status, PdpEpi e) {
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  fused_greedy_body<RL, EPL, VW, OPT>(lds, B, NC, logits, lstride, mask_in, clip, temp, action_out,
                                      logp_sel, status, e.step<RL, EPL>());
}

template <int RL, int EPL, int OPT>
__global__ __launch_bounds__(256) void pdp_decode_step_kernel(
    int64_t B, int NC, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int mode,
    const int64_t* __restrict__ action_in, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, uint64_t seed, uint64_t offset, int32_t* status, PdpEpi e) {
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  fused_step_body<RL, EPL, false, OPT>(lds, B, NC, logits, lstride, mask_in, clip, temp, mode,
                                       action_in, action_out, logp_sel, seed, offset, status,
                                       e.step<RL, EPL>());
}

}  // namespace

extern "C" int co_pdp_decode_step(int64_t B, int64_t Nloc, const float* logits, int64_t lstride,
                                  const uint8_t* mask_in, float clip, float temp, int mode,
                                  const int64_t* action_in, int64_t* action_out,
                                  float* logp_sel, uint64_t seed, uint64_t offset,
                                  const uint8_t* av_in, const uint8_t* td_in, uint8_t* av_out,
                                  uint8_t* td_out, uint8_t* mask_out, const int64_t* i_in,
                                  int64_t* i_out, int64_t* cur_out, uint8_t* done,
                                  uint8_t* step_reward, float* ll_accum, int32_t* status,
                                  void* stream) {
  if (B < 0 || Nloc < 2 || Nloc > CO_PDP_MAX_N || Nloc % 2 != 0) return CO_E_INVAL;
  const int64_t N = Nloc + 1;  // the row length, odd and at most 2047: the row engines take it
  FusedDecode f{B,         N,          logits,   lstride, mask_in, clip,     temp,   mode,
                action_in, action_out, logp_sel, seed,    offset,  mask_out, status, stream};
  if (!f.parse()) return CO_E_MODE;
  if (B == 0) return CO_OK;
  if (!f.pointers_ok() || !av_in || !td_in || !av_out || !td_out || !i_in || !i_out || !cur_out ||
      !done || !step_reward)
    return CO_E_INVAL;
  // Nothing is staged and every row up to CO_PDP_MAX_N + 1 columns fits the register row
  // engines, so the fused kernels take every size.  The one case they leave to the two
  // launches (FusedDecode::two_launches) is a mask edited in place: the certified fallback
  // reads the row's mask a second time, which must still be the input, and between the two
  // launches the stream orders the decode's reads before the step's stores.
  if (mask_out == mask_in)
    return f.two_launches(ll_accum, [&](const int64_t* actions) {
      return co_pdp_step(B, Nloc, actions, av_in, td_in, av_out, td_out, mask_out, i_in, i_out,
                         cur_out, done, step_reward, status, stream);
    });
  const PdpEpi epi{av_in, td_in, av_out,      td_out,   mask_out, i_in,
                   i_out, cur_out, done,      step_reward, ll_accum, (int)N};
  hipStream_t s = (hipStream_t)stream;
  const bool cert = f.m.cert, fast = f.m.fast;
#define CO_PDP_CALL(F, RL, EPL, V) F(RL, EPL, V)
  if (f.m.mode == CO_DECODE_GREEDY) {
    const dim3 grid(decode_grid(B, (int)N));
    if (grid.x == 0) return CO_E_INVAL;
#define CO_PDP_GREEDY(RL, EPL, V)                                                                 \
  hipLaunchKernelGGL((pdp_decode_greedy_kernel<RL, EPL, V, OPT>), grid, dim3(256), 0, s, B, (int)N, \
                     logits, lstride, mask_in, clip, temp, action_out, logp_sel, status, epi)
#define CO_PDP_G(RL, EPL, V) CO_OPT_DISPATCH_G(CO_PDP_CALL, CO_PDP_GREEDY, RL, (EPL < 4 ? 4 : EPL), V)
    if (N < 4) {
      CO_ROW_CASE(CO_PDP_G, 2, 0);  // the row of three
    } else {
      CO_ROW_DISPATCH(CO_PDP_G, 3);
    }
#undef CO_PDP_G
#undef CO_PDP_GREEDY
    return launch_status();
  }
  const dim3 grid(decode_grid(B, (int)N, 1));
  if (grid.x == 0) return CO_E_INVAL;
#define CO_PDP_STEP(RL, EPL, V)                                                                  \
  hipLaunchKernelGGL((pdp_decode_step_kernel<RL, EPL, OPT>), grid, dim3(256), 0, s, B, (int)N,   \
                     logits, lstride, mask_in, clip, temp, f.m.mode, action_in, action_out,      \
                     logp_sel, seed, offset, status, epi)
#define CO_PDP_S(RL, EPL, V) CO_OPT_DISPATCH(CO_PDP_CALL, CO_PDP_STEP, RL, EPL, V)
  CO_ROW_DISPATCH(CO_PDP_S, false);
#undef CO_PDP_S
#undef CO_PDP_STEP
#undef CO_PDP_CALL
  return launch_status();
}
