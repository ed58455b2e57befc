// Sanitizer driver for the host OP entries (co_op_reset / _step / _action_mask / _steps /
// _reward of csrc/host/co_env_host.cpp), compiled together with it under
// -fsanitize=address,undefined by tests/test_host_asan_op.py: exactly-sized heap buffers (any
// out-of-bounds index is an ASan report), whole random-feasible episodes at the row of two, on
// both sides of a row of 32 columns and at CO_OP_MAX_N, through single steps and co_op_steps
// in both action layouts, actions far out of range, the reward with its status bits and the
// prize_batch / locs_batch layout, the argument errors and the empty batch.  Exit 0 = clean.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2027);

static int run(int64_t B, int64_t N) {
  const int64_t NC = N + 1;
  std::uniform_real_distribution<float> unit(0.f, 1.f);
  std::vector<float> depot(B * 2), locs_in(B * N * 2), prize_in(B * N), ml_in(B);
  for (auto& v : depot) v = unit(rng);
  for (auto& v : locs_in) v = unit(rng);
  for (auto& v : prize_in) v = (float)(1 + rng() % 100) / 100.f;
  for (auto& v : ml_in) v = 1.5f + 1.5f * unit(rng);
  std::vector<float> locs(B * NC * 2, 7.f), prize(B * NC, 7.f), ml(B * NC, 7.f), tl(B, 7.f),
      pz(B, 7.f);
  std::vector<int64_t> cur(B, -1), it(B, -1);
  std::vector<uint8_t> vis(B * NC, 9), mask(B * NC, 9);
  CHECK_OK(co_op_reset(B, N, depot.data(), locs_in.data(), prize_in.data(), ml_in.data(),
                       locs.data(), prize.data(), ml.data(), tl.data(), pz.data(), cur.data(),
                       it.data(), vis.data(), mask.data(), nullptr));
  for (int64_t b = 0; b < B; ++b) {
    CHECK(locs[b * NC * 2] == depot[b * 2] && locs[b * NC * 2 + 2] == locs_in[b * N * 2]);
    CHECK(prize[b * NC] == 0.f && prize[b * NC + N] == prize_in[b * N + N - 1]);
    CHECK(tl[b] == 0.f && pz[b] == 0.f && cur[b] == 0 && it[b] == 0 && mask[b * NC] == 1);
    for (int64_t c = 0; c < NC; ++c) CHECK(vis[b * NC + c] == 0 && mask[b * NC + c] <= 1);
  }
  const std::vector<uint8_t> vis0 = vis, mask0 = mask;
  // a random-feasible episode through single steps, out of place; done rows pad with 0
  std::vector<int64_t> acts;  // [T, B]
  std::vector<uint8_t> vis2(B * NC), mask2(B * NC), done(B, 0), rew(B), fin(B, 0);
  std::vector<float> tl2(B), pz2(B);
  std::vector<int64_t> cur2(B), it2(B), act(B);
  int64_t T = 0;
  while (!std::all_of(fin.begin(), fin.end(), [](uint8_t f) { return f == 1; }) && T < 48) {
    for (int64_t b = 0; b < B; ++b) {
      std::vector<int64_t> open;
      for (int64_t c = 1; c < NC; ++c)
        if (mask[b * NC + c]) open.push_back(c);
      act[b] = open.empty() || (T > 2 && rng() % 8 == 0) ? 0 : open[rng() % open.size()];
      acts.push_back(act[b]);
    }
    int32_t status = 0;
    CHECK_OK(co_op_step(B, N, act.data(), locs.data(), prize.data(), ml.data(), vis.data(),
                        vis2.data(), tl.data(), tl2.data(), pz.data(), pz2.data(), cur.data(),
                        cur2.data(), it.data(), it2.data(), done.data(), rew.data(), mask2.data(),
                        &status, nullptr));
    CHECK(status == 0);
    vis.swap(vis2), mask.swap(mask2), tl.swap(tl2), pz.swap(pz2), cur.swap(cur2), it.swap(it2);
    ++T;
    std::vector<uint8_t> alone(B * NC, 9);
    CHECK_OK(co_op_action_mask(B, N, locs.data(), ml.data(), vis.data(), tl.data(), cur.data(),
                               alone.data(), nullptr));
    CHECK(alone == mask);
    for (int64_t b = 0; b < B; ++b) {
      CHECK(cur[b] == act[b] && it[b] == T && rew[b] == 0);
      CHECK(done[b] == (act[b] == 0 && T > 1));
      fin[b] |= done[b];
    }
  }
  // the same episode in one call, step-major and row-major
  std::vector<int64_t> rows(B * T);  // [B, T]
  for (int64_t t = 0; t < T; ++t)
    for (int64_t b = 0; b < B; ++b) rows[b * T + t] = acts[t * B + b];
  for (int layout = 0; layout < 2; ++layout) {
    std::vector<uint8_t> v3 = vis0, m3(B * NC, 9), d3(B, 9), r3(B, 9), feas(T * B, 9);
    std::vector<float> t3(B, 0.f), p3(B, 0.f), len(T * B, 7.f);
    std::vector<int64_t> i3(B, 0), c3(B, 0);
    int32_t status = 0;
    CHECK_OK(co_op_steps(B, N, T, layout ? rows.data() : acts.data(), layout ? 1 : B,
                         layout ? T : 1, locs.data(), prize.data(), ml.data(), mask0.data(),
                         v3.data(), t3.data(), p3.data(), c3.data(), i3.data(), d3.data(),
                         r3.data(), m3.data(), feas.data(), len.data(), &status, nullptr));
    CHECK(status == 0 && v3 == vis && m3 == mask && t3 == tl && p3 == pz && i3 == it && c3 == cur);
    CHECK(std::all_of(feas.begin(), feas.end(), [](uint8_t f) { return f == 1; }));
    CHECK(d3 == done && len[(T - 1) * B] == tl[0]);
    // without feasible / length
    v3 = vis0, std::fill(t3.begin(), t3.end(), 0.f), std::fill(p3.begin(), p3.end(), 0.f);
    std::fill(i3.begin(), i3.end(), 0), std::fill(c3.begin(), c3.end(), 0);
    CHECK_OK(co_op_steps(B, N, T, acts.data(), B, 1, locs.data(), prize.data(), ml.data(), nullptr,
                         v3.data(), t3.data(), p3.data(), c3.data(), i3.data(), d3.data(),
                         r3.data(), m3.data(), nullptr, nullptr, &status, nullptr));
    CHECK(status == 0 && v3 == vis && m3 == mask && t3 == tl);
  }
  // the reward: valid tours, then a duplicate, a short budget and indices far out of range
  std::vector<float> reward(B, 7.f), reward2(B, 7.f);
  int32_t status = 0;
  CHECK_OK(co_op_reward(B, N, T, prize.data(), B, locs.data(), ml.data(), B, rows.data(), T, 1, 1,
                        reward.data(), &status, nullptr));
  CHECK(status == 0);
  CHECK_OK(co_op_reward(B, N, T, prize.data(), B, locs.data(), ml.data(), B, acts.data(), 1, B, 1,
                        reward2.data(), &status, nullptr));
  CHECK(status == 0 && reward == reward2);
  CHECK_OK(co_op_reward(B, N, T, prize.data(), 1, nullptr, nullptr, 1, rows.data(), T, 1, 0,
                        reward2.data(), nullptr, nullptr));  // every row on instance 0
  CHECK(reward2[0] == reward[0]);
  const int64_t r = B - 1;
  std::vector<int64_t> bad = rows;
  if (T >= 2 && bad[r * T] != 0) {
    bad[r * T + 1] = bad[r * T];
    CHECK_OK(co_op_reward(B, N, T, prize.data(), B, locs.data(), ml.data(), B, bad.data(), T, 1, 1,
                          reward2.data(), &status, nullptr));
    CHECK(status == CO_ST_OP_DUPLICATE);
    status = 0;
    std::vector<float> tight = ml;
    for (int64_t c = 0; c < NC; ++c) tight[r * NC + c] -= 8.f;
    CHECK_OK(co_op_reward(B, N, T, prize.data(), B, locs.data(), tight.data(), B, rows.data(), T,
                          1, 1, reward2.data(), &status, nullptr));
    CHECK(status == CO_ST_OP_LENGTH);
  }
  status = 0;
  std::vector<int64_t> single(B, 0);
  single[r] = N;
  CHECK_OK(co_op_reward(B, N, 1, prize.data(), B, locs.data(), ml.data(), B, single.data(), 1, 1,
                        1, reward2.data(), &status, nullptr));
  CHECK(status == CO_ST_OP_SINGLE_NONZERO && reward2[r] == 0.f);
  const int64_t far[] = {-1, N + 1, -(int64_t(1) << 40), int64_t(1) << 40};
  for (int64_t f : far) {
    bad = rows, status = 0;
    bad[r * T] = f;
    CHECK_OK(co_op_reward(B, N, T, prize.data(), B, locs.data(), ml.data(), B, bad.data(), T, 1, 1,
                          reward2.data(), &status, nullptr));
    CHECK(status & CO_ST_INDEX_RANGE);
    std::fill(act.begin(), act.end(), f);
    std::vector<uint8_t> v3(B * NC, 9), m3(B * NC), d3(B), r3(B), feas(2 * B, 9);
    std::vector<float> t3(B, 7.f), p3(B, 7.f), zero(B, 0.f), len(2 * B, 7.f);
    std::vector<int64_t> i3(B, -1), c3(B, -1), i0(B, 0), c0(B, 0);
    std::vector<int64_t> two(2 * B, f);
    status = 0;
    CHECK_OK(co_op_step(B, N, act.data(), locs.data(), prize.data(), ml.data(), vis0.data(),
                        v3.data(), zero.data(), t3.data(), zero.data(), p3.data(), c0.data(),
                        c3.data(), i0.data(), i3.data(), d3.data(), r3.data(), m3.data(), &status,
                        nullptr));
    CHECK(status == CO_ST_INDEX_RANGE && v3 == vis0 && c3[0] == f && i3[0] == 1);
    CHECK(t3[0] == 0.f && p3[0] == 0.f && d3[0] == 0);
    status = 0;
    v3 = vis0, t3 = zero, p3 = zero, i3 = i0, c3 = c0;
    CHECK_OK(co_op_steps(B, N, 2, two.data(), B, 1, locs.data(), prize.data(), ml.data(),
                         mask0.data(), v3.data(), t3.data(), p3.data(), c3.data(), i3.data(),
                         d3.data(), r3.data(), m3.data(), feas.data(), len.data(), &status,
                         nullptr));
    CHECK(status == CO_ST_INDEX_RANGE && v3 == vis0 && i3[0] == 2 && t3[0] == 0.f);
    CHECK(std::all_of(feas.begin(), feas.end(), [](uint8_t x) { return x == 0; }));
  }
  return 0;
}

int main() {
  const int64_t cases[][2] = {{1, 1}, {5, 1}, {3, 4}, {7, 30}, {7, 31}, {7, 32}, {2, 255},
                              {2, CO_OP_MAX_N}};
  for (const auto& c : cases)
    if (run(c[0], c[1])) return 1;
  // argument errors (decided before the empty batch) and the empty batch
  const int64_t wrong[] = {CO_OP_MAX_N + 1, 0, -2};
  for (int64_t n : wrong) {
    CHECK(co_op_reset(0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_op_step(0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_op_action_mask(0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          CO_E_INVAL);
    CHECK(co_op_steps(0, n, 1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_op_reward(0, n, 3, nullptr, 1, nullptr, nullptr, 1, nullptr, 0, 0, 0, nullptr,
                       nullptr, nullptr) == CO_E_INVAL);
  }
  CHECK(co_op_reset(0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_op_steps(0, 4, 3, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    nullptr) == CO_OK);
  CHECK(co_op_reward(0, 4, 5, nullptr, 1, nullptr, nullptr, 1, nullptr, 0, 0, 1, nullptr, nullptr,
                     nullptr) == CO_OK);
  CHECK(co_op_reward(2, 4, 5, nullptr, 1, nullptr, nullptr, 1, nullptr, 0, 0, 1, nullptr, nullptr,
                     nullptr) == CO_E_INVAL);  // NULL pointers
  std::vector<float> l(11), p(5), m(5);
  std::vector<int64_t> a(5);
  float rw;
  int32_t st = 0;
  CHECK(co_op_reward(1, 4, 5, p.data(), 1, l.data() + 1, m.data(), 1, a.data(), 5, 1, 1, &rw, &st,
                     nullptr) == CO_E_ALIGN);
  CHECK(co_op_reward(3, 4, 5, p.data(), 2, l.data(), m.data(), 1, a.data(), 5, 1, 1, &rw, &st,
                     nullptr) == CO_E_INVAL);
  std::printf("host op: ran clean\n");
  return 0;
}
