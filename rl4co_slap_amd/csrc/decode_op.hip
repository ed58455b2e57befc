// co_op_decode_step: the decode step fused with OPEnv._step (decode_fused.hpp bodies).  The
// row's logits and action_mask are read once; the selected action's transition
// (op/env.py:74-108, the mask of :153-169) is applied by the same lane group, every lane on
// the columns of visited, locs and max_length it fetched before the logits: the leg from
// the current node and the action's prize by address (one address a group: broadcast
// loads), visited plus the action, the lane's columns of the new mask (a distance each),
// done from the action.  2,102 B per OP-100 row-step (include/co_env.h).
//
// N + 1 is even or odd, so the aligned row engines (GreedyRow's VW = 4, DecodeRow's VEC)
// apply as they do for CVRP; the 2,048-column bucket is never reached (CO_OP_MAX_N + 1 =
// 1,024) and is not instantiated.
#include "decode_fused.hpp"

namespace {

struct OpEpi {  // the env half's arguments
  const float2* locs;
  const float *prize, *ml;
  const uint8_t* vis_in;
  uint8_t* vis_out;
  const float *tl_in, *pz_in;
  float *tl_out, *pz_out;
  const int64_t *cur_in, *i_in;
  int64_t *cur_out, *i_out;
  uint8_t *done, *step_reward, *mask_out;
  float* ll_accum;
  int NC;
};

// The env-step type of OP (decode_fused.hpp): lane sl of the row's group keeps its EPL
// columns of visited (EPL / 4 words of bytes), locs and max_length, and every lane the row
// scalars the new mask needs.
template <int RL, int EPL>
struct OpStep {
  static constexpr int kDiagCut = 0;
  static constexpr int W = EPL / 4;
  OpEpi e;
  uint32_t vis[W] = {};
  float lx[EPL] = {}, ly[EPL] = {}, ml[EPL] = {};
  float tl = 0.f, pz = 0.f, cx = 0.f, cy = 0.f, acc = 0.f;
  int64_t iv = 0;
  bool v0 = false, dn = false;

  __device__ __forceinline__ void fetch(int64_t base, int64_t B, int grp, bool lead) {
    using M = typename Chunk<3>::M;
    const int64_t r = base + grp;
    if (r >= B) return;
    const int NC = e.NC;
    const int c0 = (lane_id() % RL) * EPL;
    const int64_t row = r * (int64_t)NC;
    const uint8_t* vrow = e.vis_in + row;
    const int64_t cur = e.cur_in[r];
    tl = e.tl_in[r];
    v0 = vrow[0] != 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int c = c0 + 4 * j;
      if (c + 4 <= NC) {
        vis[j] = *reinterpret_cast<const M*>(vrow + c);
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (c + q < NC) vis[j] |= (uint32_t)vrow[c + q] << (8 * q);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c + q < NC) {
          const float2 p = e.locs[row + c + q];
          lx[4 * j + q] = p.x, ly[4 * j + q] = p.y;
          ml[4 * j + q] = e.ml[row + c + q];
        }
    }
    const float2 pc = e.locs[row + (cur < 0 ? 0 : (cur >= NC ? NC - 1 : cur))];
    cx = pc.x, cy = pc.y;
    if (!lead) return;
    pz = e.pz_in[r];
    iv = e.i_in[r];
    if (e.ll_accum) acc = e.ll_accum[r];
  }

  // a non-zero byte -> 1 (co_op_step's reading of its input row)
  __device__ __forceinline__ static uint32_t flags(uint32_t x) {
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
  }

  template <class Row, class A>
  __device__ __forceinline__ bool apply(Row&, bool valid, int64_t r, int, int, int c0, A a_raw,
                                        int, int32_t*) {
    using M = typename Chunk<3>::M;
    const int NC = e.NC;
    const int64_t a64 = (int64_t)a_raw;
    const bool bad = a64 < 0 || a64 >= NC;
    const int ac = a64 < 0 ? 0 : (a64 >= NC ? NC - 1 : (int)a64);
    const int64_t row = r * (int64_t)NC;
    const float2 la = e.locs[row + ac];  // one address a group
    const float pa = e.prize[row + ac];
    const float leg = edge_len(la.x, la.y, cx, cy);
    if (!bad) {
      tl = tl + leg;
      pz = pz + pa;
      v0 |= ac == 0;
    }
    dn = a64 == 0 && iv > 0;
    const int as = bad ? -8 : ac;
    uint8_t *vdst = e.vis_out + row, *mdst = e.mask_out + row;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int c = c0 + 4 * j;
      uint32_t x = flags(vis[j]);
      const int oa = as - c;
      if ((unsigned)oa < 4u) x |= 1u << (8 * oa);
      uint32_t open = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool exceeds = tl + edge_len(lx[4 * j + q], ly[4 * j + q], la.x, la.y) > ml[4 * j + q];
        open |= (exceeds ? 0u : 1u) << (8 * q);
      }
      uint32_t m = v0 ? 0u : (open & ~x & 0x01010101u);
      if (c == 0) m |= 1u;
      if (valid && c + 4 <= NC) {
        *reinterpret_cast<M*>(vdst + c) = (M)x;
        *reinterpret_cast<M*>(mdst + c) = (M)m;
      } else if (valid && c < NC) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (c + q < NC) {
            vdst[c + q] = (uint8_t)(x >> (8 * q));
            mdst[c + q] = (uint8_t)(m >> (8 * q));
          }
      }
    }
    return !bad;
  }
  __device__ __forceinline__ float* ll_out() const { return e.ll_accum; }
  __device__ __forceinline__ float ll_in(int) const { return acc; }
  __device__ __forceinline__ void store_row(int64_t r, int, int64_t a) const {
    e.tl_out[r] = tl;
    e.pz_out[r] = pz;
    e.i_out[r] = iv + 1;
    e.cur_out[r] = a;
    e.done[r] = dn;
    e.step_reward[r] = 0;
  }
};

template <int RL, int EPL, int VW, int OPT>
__global__ __launch_bounds__(256) void op_decode_greedy_kernel(
    int64_t B, int NC, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, int32_t* status, OpEpi e) {
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  fused_greedy_body<RL, EPL, VW, OPT>(lds, B, NC, logits, lstride, mask_in, clip, temp, action_out,
                                      logp_sel, status, OpStep<RL, EPL>{e});
}

template <int RL, int EPL, bool VEC, int OPT>
__global__ __launch_bounds__(256) void op_decode_step_kernel(
    int64_t B, int NC, const float* __restrict__ logits, int64_t lstride,
    const uint8_t* __restrict__ mask_in, float clip, float temp, int mode,
    const int64_t* __restrict__ action_in, int64_t* __restrict__ action_out,
    float* __restrict__ logp_sel, uint64_t seed, uint64_t offset, int32_t* status, OpEpi e) {
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * EPL];
  fused_step_body<RL, EPL, VEC, OPT>(lds, B, NC, logits, lstride, mask_in, clip, temp, mode,
                                     action_in, action_out, logp_sel, seed, offset, status,
                                     OpStep<RL, EPL>{e});
}

// the row buckets a row of at most CO_OP_MAX_N + 1 columns can reach
#define CO_OP_ROWS(LAUNCH, V)                            \
  if (N <= kRowCap[0]) CO_ROW_CASE(LAUNCH, V, 0);        \
  else if (N <= kRowCap[1]) CO_ROW_CASE(LAUNCH, V, 1);   \
  else if (N <= kRowCap[2]) CO_ROW_CASE(LAUNCH, V, 2);   \
  else if (N <= kRowCap[3]) CO_ROW_CASE(LAUNCH, V, 3);   \
  else if (N <= kRowCap[4]) CO_ROW_CASE(LAUNCH, V, 4);   \
  else if (N <= kRowCap[5]) CO_ROW_CASE(LAUNCH, V, 5);   \
  else CO_ROW_CASE(LAUNCH, V, 6)
static_assert(CO_OP_MAX_N + 1 <= kRowCap[6], "the OP rows end at the 1,024-column bucket");

}  // namespace

extern "C" int co_op_decode_step(int64_t B, int64_t Nloc, const float* logits, int64_t lstride,
                                 const uint8_t* mask_in, float clip, float temp, int mode,
                                 const int64_t* action_in, int64_t* action_out,
                                 float* logp_sel, uint64_t seed, uint64_t offset,
                                 const co_op_instance* instance, const uint8_t* vis_in, uint8_t* vis_out, const float* tl_in,
                                 float* tl_out, const float* pz_in, float* pz_out,
                                 const int64_t* cur_in, int64_t* cur_out, const int64_t* i_in,
                                 int64_t* i_out, uint8_t* done, uint8_t* step_reward,
                                 uint8_t* mask_out, float* ll_accum, int32_t* status,
                                 void* stream) {
  if (B < 0 || Nloc < 1 || Nloc > CO_OP_MAX_N) return CO_E_INVAL;
  const int64_t N = Nloc + 1;  // the row length
  FusedDecode f{B,         N,          logits,   lstride, mask_in, clip,     temp,   mode,
                action_in, action_out, logp_sel, seed,    offset,  mask_out, status, stream};
  if (!f.parse()) return CO_E_MODE;
  if (B == 0) return CO_OK;
  if (!instance) return CO_E_INVAL;
  const float *locs = instance->locs, *prize = instance->prize,
              *max_length = instance->max_length;
  if (!f.pointers_ok() || !locs || !prize || !max_length || !vis_in || !vis_out || !tl_in ||
      !tl_out || !pz_in || !pz_out || !cur_in || !cur_out || !i_in || !i_out || !done ||
      !step_reward)
    return CO_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(locs) & 7) != 0) return CO_E_ALIGN;
  // Nothing is staged, so the fused kernels take every size.  The one case they leave to the
  // two launches (FusedDecode::two_launches) is a mask edited in place: the certified
  // fallback reads the row's mask a second time, which must still be the input, and between
  // the two launches the stream orders the decode's reads before the step's stores.
  if (mask_out == mask_in)
    return f.two_launches(ll_accum, [&](const int64_t* actions) {
      return co_op_step(B, Nloc, actions, locs, prize, max_length, vis_in, vis_out, tl_in, tl_out,
                        pz_in, pz_out, cur_in, cur_out, i_in, i_out, done, step_reward, mask_out,
                        status, stream);
    });
  const OpEpi epi{reinterpret_cast<const float2*>(locs), prize, max_length, vis_in, vis_out,
                  tl_in, pz_in, tl_out, pz_out, cur_in, i_in, cur_out, i_out, done, step_reward,
                  mask_out, ll_accum, (int)N};
  hipStream_t s = (hipStream_t)stream;
  const bool cert = f.m.cert, fast = f.m.fast;
#define CO_OP_CALL(F, RL, EPL, V) F(RL, EPL, V)
  if (f.m.mode == CO_DECODE_GREEDY) {
    const dim3 grid(decode_grid(B, (int)N));
    if (grid.x == 0) return CO_E_INVAL;
#define CO_OP_GREEDY(RL, EPL, V)                                                                  \
  hipLaunchKernelGGL((op_decode_greedy_kernel<RL, EPL, V, OPT>), grid, dim3(256), 0, s, B, (int)N, \
                     logits, lstride, mask_in, clip, temp, action_out, logp_sel, status, epi)
#define CO_OP_G(RL, EPL, V) CO_OPT_DISPATCH_G(CO_OP_CALL, CO_OP_GREEDY, RL, (EPL < 4 ? 4 : EPL), V)
    // the transition stores the mask row itself, byte-wise: only the loads decide the width
    switch (greedy_vw(N, lstride, logits, mask_in, nullptr, nullptr)) {
      case 4: CO_OP_ROWS(CO_OP_G, 4); break;
      case 2: CO_ROW_CASE(CO_OP_G, 2, 0); break;  // N < 4
      default: CO_OP_ROWS(CO_OP_G, 3);
    }
#undef CO_OP_G
#undef CO_OP_GREEDY
    return launch_status();
  }
  const dim3 grid(decode_grid(B, (int)N, 1));
  if (grid.x == 0) return CO_E_INVAL;
#define CO_OP_STEP(RL, EPL, V)                                                                   \
  hipLaunchKernelGGL((op_decode_step_kernel<RL, EPL, V, OPT>), grid, dim3(256), 0, s, B, (int)N, \
                     logits, lstride, mask_in, clip, temp, f.m.mode, action_in, action_out,      \
                     logp_sel, seed, offset, status, epi)
#define CO_OP_S(RL, EPL, V) CO_OPT_DISPATCH(CO_OP_CALL, CO_OP_STEP, RL, EPL, V)
  if (decode_vec_ok(logits, lstride, mask_in, N)) {
    CO_OP_ROWS(CO_OP_S, true);
  } else {
    CO_OP_ROWS(CO_OP_S, false);
  }
#undef CO_OP_S
#undef CO_OP_STEP
#undef CO_OP_CALL
  return launch_status();
}
