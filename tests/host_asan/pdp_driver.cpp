// Sanitizer driver for the host PDP entries (co_pdp_reset / _step / _steps / _reward of
// csrc/host/co_env_host.cpp), compiled together with it under -fsanitize=address,undefined
// by tests/test_host_asan_pdp.py: exactly-sized heap buffers (any out-of-bounds index is an
// ASan report), whole random-feasible episodes at the row of three, on both sides of a row
// of 32 columns and at CO_PDP_MAX_N, through single steps and co_pdp_steps in both action
// layouts, actions far out of range, the reward with both validity bits and the locs_batch
// layout, the argument errors and the empty batch.  Exit 0 = clean.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2026);

static int run(int64_t B, int64_t N) {
  const int64_t NC = N + 1, h = N / 2;
  std::vector<float> depot(B * 2), locs_in(B * N * 2), locs(B * NC * 2);
  for (auto& v : depot) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  for (auto& v : locs_in) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  std::vector<uint8_t> av(B * NC, 9), td(B * NC, 9), mask(B * NC, 9), done(B, 9), term(B, 9);
  std::vector<int64_t> cur(B, -1), it(B, -1);
  CHECK_OK(co_pdp_reset(B, N, depot.data(), locs_in.data(), locs.data(), av.data(), td.data(),
                        mask.data(), cur.data(), it.data(), done.data(), term.data(), nullptr));
  for (int64_t b = 0; b < B; ++b) {
    CHECK(locs[b * NC * 2] == depot[b * 2] && locs[b * NC * 2 + 2] == locs_in[b * N * 2]);
    for (int64_t c = 0; c < NC; ++c)
      CHECK(av[b * NC + c] == 1 && td[b * NC + c] == (c <= h) && mask[b * NC + c] == (c == 0));
    CHECK(cur[b] == 0 && it[b] == 0 && done[b] == 0 && term[b] == 0);
  }
  const std::vector<uint8_t> av0 = av, td0 = td, mask0 = mask;
  // a random-feasible episode through single steps, out of place
  std::vector<int64_t> acts(NC * B);  // [T, B]
  std::vector<uint8_t> av2(B * NC), td2(B * NC), mask2(B * NC), rew(B);
  std::vector<int64_t> it2(B), act(B);
  for (int64_t t = 0; t < NC; ++t) {
    for (int64_t b = 0; b < B; ++b) {
      std::vector<int64_t> open;
      for (int64_t c = 0; c < NC; ++c)
        if (mask[b * NC + c]) open.push_back(c);
      CHECK(!open.empty());
      act[b] = acts[t * B + b] = open[rng() % open.size()];
    }
    int32_t status = 0;
    CHECK_OK(co_pdp_step(B, N, act.data(), av.data(), td.data(), av2.data(), td2.data(),
                         mask2.data(), it.data(), it2.data(), cur.data(), done.data(), rew.data(),
                         &status, nullptr));
    CHECK(status == 0);
    av.swap(av2), td.swap(td2), mask.swap(mask2), it.swap(it2);
    for (int64_t b = 0; b < B; ++b)
      CHECK(cur[b] == act[b] && it[b] == t + 1 && rew[b] == 0 && done[b] == (t == NC - 1));
  }
  // the same episode in one call, step-major and row-major
  std::vector<int64_t> rows(B * NC);  // [B, T]
  for (int64_t t = 0; t < NC; ++t)
    for (int64_t b = 0; b < B; ++b) rows[b * NC + t] = acts[t * B + b];
  for (int layout = 0; layout < 2; ++layout) {
    std::vector<uint8_t> a3 = av0, t3 = td0, m3(B * NC, 9), d3(B, 9), r3(B, 9), feas(NC * B, 9);
    std::vector<int64_t> i3(B, 0), c3(B, -1);
    int32_t status = 0;
    CHECK_OK(co_pdp_steps(B, N, NC, layout ? rows.data() : acts.data(), layout ? 1 : B,
                          layout ? NC : 1, mask0.data(), a3.data(), t3.data(), m3.data(), i3.data(),
                          c3.data(), d3.data(), r3.data(), feas.data(), &status, nullptr));
    CHECK(status == 0 && a3 == av && t3 == td && m3 == mask && i3 == it && c3 == cur);
    CHECK(std::all_of(feas.begin(), feas.end(), [](uint8_t f) { return f == 1; }));
    CHECK(std::all_of(d3.begin(), d3.end(), [](uint8_t f) { return f == 1; }));
  }
  // the reward: valid tours, then a swapped pair, a duplicate and indices far out of range
  std::vector<float> reward(B, 7.f), reward2(B, 7.f);
  int32_t status = 0;
  CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), B, rows.data(), NC, 1, 1, reward.data(), &status,
                         nullptr));
  CHECK(status == 0);
  CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), B, acts.data(), 1, B, 1, reward2.data(), &status,
                         nullptr));
  CHECK(status == 0 && reward == reward2);
  CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), 1, rows.data(), NC, 1, 0, reward2.data(), nullptr,
                         nullptr));  // every row on instance 0
  CHECK(reward2[0] == reward[0]);
  const int64_t r = B - 1;
  std::vector<int64_t> bad = rows;
  int64_t* row = bad.data() + r * NC;
  const int64_t p = std::find_if(row, row + NC, [&](int64_t a) { return a >= 1 && a <= h; }) - row;
  const int64_t d = std::find(row, row + NC, row[p] + h) - row;
  std::swap(row[p], row[d]);
  CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), B, bad.data(), NC, 1, 1, reward2.data(), &status,
                         nullptr));
  CHECK(status == CO_ST_PDP_PRECEDENCE);
  bad = rows, status = 0;
  bad[r * NC + NC - 1] = bad[r * NC];
  CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), B, bad.data(), NC, 1, 1, reward2.data(), &status,
                         nullptr));
  CHECK(status == CO_ST_PDP_NOT_ALL_NODES);
  const int64_t far[] = {-1, N + 1, -(int64_t(1) << 40), int64_t(1) << 40};
  for (int64_t f : far) {
    bad = rows, status = 0;
    bad[r * NC + 1] = f;
    CHECK_OK(co_pdp_reward(B, N, NC, locs.data(), B, bad.data(), NC, 1, 1, reward2.data(), &status,
                           nullptr));
    CHECK(status == (CO_ST_INDEX_RANGE | CO_ST_PDP_NOT_ALL_NODES));
    std::fill(act.begin(), act.end(), f);
    std::vector<uint8_t> a3 = av0, t3 = td0, m3(B * NC), d3(B), r3(B), feas(2 * B, 9);
    std::vector<int64_t> i3(B, 0), c3(B);
    std::vector<int64_t> two(2 * B, f);
    status = 0;
    CHECK_OK(co_pdp_step(B, N, act.data(), av0.data(), td0.data(), a3.data(), t3.data(), m3.data(),
                         i3.data(), it2.data(), c3.data(), d3.data(), r3.data(), &status, nullptr));
    CHECK(status == CO_ST_INDEX_RANGE && a3 == av0 && t3 == td0 && c3[0] == f && it2[0] == 1);
    status = 0;
    CHECK_OK(co_pdp_steps(B, N, 2, two.data(), B, 1, mask0.data(), a3.data(), t3.data(), m3.data(),
                          i3.data(), c3.data(), d3.data(), r3.data(), feas.data(), &status, nullptr));
    CHECK(status == CO_ST_INDEX_RANGE && a3 == av0 && t3 == td0 && i3[0] == 2);
    CHECK(std::all_of(feas.begin(), feas.end(), [](uint8_t x) { return x == 0; }));
  }
  return 0;
}

int main() {
  const int64_t cases[][2] = {{1, 2}, {5, 2}, {3, 4}, {7, 30}, {7, 32}, {2, 254}, {2, CO_PDP_MAX_N}};
  for (const auto& c : cases)
    if (run(c[0], c[1])) return 1;
  // argument errors (decided before the empty batch) and the empty batch
  const int64_t wrong[] = {CO_PDP_MAX_N + 2, 7, 1, 0, -2};
  for (int64_t n : wrong) {
    CHECK(co_pdp_reset(0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_pdp_step(0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_pdp_steps(0, n, 1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr) == CO_E_INVAL);
    CHECK(co_pdp_reward(0, n, 3, nullptr, 1, nullptr, 0, 0, 0, nullptr, nullptr, nullptr) ==
          CO_E_INVAL);
  }
  CHECK(co_pdp_reset(0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_pdp_steps(0, 4, 3, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_pdp_reward(0, 4, 5, nullptr, 1, nullptr, 0, 0, 1, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_pdp_reward(0, 4, 4, nullptr, 1, nullptr, 0, 0, 1, nullptr, nullptr, nullptr) ==
        CO_E_INVAL);  // an even number of steps with check
  CHECK(co_pdp_reward(2, 4, 5, nullptr, 1, nullptr, 0, 0, 1, nullptr, nullptr, nullptr) ==
        CO_E_INVAL);  // NULL pointers
  std::vector<float> l(11);
  std::vector<int64_t> a(5);
  float rw;
  int32_t st = 0;
  CHECK(co_pdp_reward(1, 4, 5, l.data() + 1, 1, a.data(), 5, 1, 1, &rw, &st, nullptr) ==
        CO_E_ALIGN);
  CHECK(co_pdp_reward(3, 4, 5, l.data(), 2, a.data(), 5, 1, 1, &rw, &st, nullptr) == CO_E_INVAL);
  std::printf("host pdp: ran clean\n");
  return 0;
}
