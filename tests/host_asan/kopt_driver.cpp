// Sanitizer driver for the host k-opt improvement entries (co_tsp_linked_list,
// co_tsp_real_solution, co_tsp_kopt_reset / _step / _steps, co_tsp_nearest_rec of
// csrc/host/co_env_host.cpp), compiled together with it under -fsanitize=address,undefined
// by tests/test_host_asan_kopt.py: exactly-sized heap buffers (any out-of-bounds index is an
// ASan report), row-major, padded and step-major layouts, every 2-opt pair of small tours,
// random in-range k-opt actions (valid or not: an invalid result only sets its bit),
// out-of-range actions, broken lists, the fused call against the single steps and the
// argument errors.  Exit 0 = clean.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2026);

static std::vector<int64_t> random_rec(int64_t B, int64_t N) {
  std::vector<int64_t> tour(N), rec(B * N);
  for (int64_t b = 0; b < B; ++b) {
    std::iota(tour.begin(), tour.end(), 0);
    std::shuffle(tour.begin(), tour.end(), rng);
    for (int64_t k = 0; k < N; ++k) rec[b * N + tour[k]] = tour[(k + 1) % N];
  }
  return rec;
}

static bool is_cycle(const int64_t* rec, int64_t N) {
  std::vector<char> seen(N, 0);
  int64_t cur = 0;
  for (int64_t k = 0; k < N; ++k) {
    if (cur < 0 || cur >= N || seen[cur]) return false;
    seen[cur] = 1;
    cur = rec[cur];
  }
  return cur == 0;
}

static int run_lists(int64_t B, int64_t N, int layout) {
  const int64_t sb = layout == 0 ? N : layout == 1 ? N + 3 : 1, st = layout == 2 ? B : 1;
  std::vector<int64_t> tour(layout == 1 ? B * (N + 3) - 3 : B * N, -7), rec(B * N, -7),
      order(B * N, -7), row(N);
  for (int64_t b = 0; b < B; ++b) {
    std::iota(row.begin(), row.end(), 0);
    std::shuffle(row.begin(), row.end(), rng);
    std::rotate(row.begin(), std::find(row.begin(), row.end(), 0), row.end());
    for (int64_t k = 0; k < N; ++k) tour[b * sb + k * st] = row[k];
  }
  int32_t status = 0;
  CHECK_OK(co_tsp_linked_list(B, N, tour.data(), sb, st, rec.data(), &status, nullptr));
  CHECK(status == 0);
  CHECK_OK(co_tsp_real_solution(B, N, rec.data(), order.data(), &status, nullptr));
  CHECK(status == 0);
  for (int64_t b = 0; b < B; ++b)
    for (int64_t k = 0; k < N; ++k) CHECK(order[b * N + k] == tour[b * sb + k * st]);
  if (N > 1) {  // a repeated node, an entry out of range: the bit, the row not written
    tour[(B - 1) * sb + st] = tour[(B - 1) * sb];
    std::fill(rec.begin(), rec.end(), -7);
    CHECK_OK(co_tsp_linked_list(B, N, tour.data(), sb, st, rec.data(), &status, nullptr));
    CHECK(status == CO_ST_INVALID_TOUR && rec[(B - 1) * N] == -7);
    tour[(B - 1) * sb] = N;
    status = 0;
    CHECK_OK(co_tsp_linked_list(B, N, tour.data(), sb, st, rec.data(), &status, nullptr));
    CHECK(status == CO_ST_INVALID_TOUR);
  }
  return 0;
}

static int run_steps(int64_t B, int64_t N, int64_t K, int64_t T, int64_t LB, int spoil) {
  const int64_t A = K == 2 ? 2 : 3 * K;
  std::vector<float> locs(LB * N * 2);
  for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  std::vector<int64_t> rec0 = random_rec(B, N), acts(T * B * A);
  for (auto& v : acts) v = (int64_t)(rng() % (uint64_t)N);
  if (spoil == 1 && T > 0) acts[(T - 1) * B * A + A - 1] = N;  // out of range, row 0
  if (spoil == 2 && T > 0) acts[0] = -1;
  std::vector<float> cost0(B), cost(B), bsf(B), rew(B), costm(B), bsfm(B), rews(T * B),
      per(T * B);
  std::vector<int64_t> vt(B * N), vtm(B * N), rec(rec0), best(rec0), recm(rec0), bestm(rec0),
      i(B, 0), im(B, 0);
  int32_t status = 0, statusm = 0;
  CHECK_OK(co_tsp_kopt_reset(B, N, locs.data(), LB, rec0.data(), cost0.data(), vt.data(),
                             &status, nullptr));
  CHECK(status == 0);
  for (int64_t b = 0; b < B; ++b) CHECK(vt[b * N] == N && vt[b * N + rec0[b * N]] == (N > 1 ? 1 : N));
  bsf = cost0, bsfm = cost0;
  for (int64_t t = 0; t < T; ++t) {  // in place: rec_out over rec_in, bsf_out over bsf_in
    status = 0;
    CHECK_OK(co_tsp_kopt_step(B, N, K, locs.data(), LB, rec.data(), acts.data() + t * B * A, A, 1,
                              rec.data(), cost.data(), bsf.data(), bsf.data(), rew.data(),
                              best.data(), vt.data(), i.data(), i.data(), &status, nullptr));
    CHECK(K > 2 || spoil || status == 0);
    if (status) break;  // a failed row keeps its old state; the comparison below is skipped
  }
  CHECK_OK(co_tsp_kopt_steps(B, N, K, T, locs.data(), LB, acts.data(), B * A, A, 1, recm.data(),
                             costm.data(), bsfm.data(), bestm.data(), vtm.data(), im.data(),
                             rews.data(), per.data(), &statusm, nullptr));
  if (K == 2 && !spoil) {
    CHECK(statusm == 0);
    for (int64_t b = 0; b < B; ++b) CHECK(is_cycle(recm.data() + b * N, N) && is_cycle(bestm.data() + b * N, N));
  }
  // (a k-opt row may have ended on an invalid result before its spoilt last step)
  if ((spoil == 2 || (spoil == 1 && K == 2)) && T > 0) CHECK(statusm & CO_ST_INDEX_RANGE);
  if (statusm == 0 && status == 0 && T > 0) {  // every row valid: the fused call is the T steps
    CHECK(rec == recm && best == bestm && vt == vtm && i == im && cost == costm && bsf == bsfm);
    for (int64_t b = 0; b < B; ++b) CHECK(rews[(T - 1) * B + b] == rew[b] && per[(T - 1) * B + b] == cost[b]);
  }
  // step_to_solution: the list itself; i stays
  std::vector<int64_t> out(B * N);
  status = 0;
  CHECK_OK(co_tsp_kopt_step(B, N, 0, locs.data(), LB, rec0.data(), nullptr, 0, 0, out.data(),
                            cost.data(), cost0.data(), bsf.data(), rew.data(), best.data(),
                            vt.data(), nullptr, nullptr, &status, nullptr));
  CHECK(status == 0 && out == rec0);
  for (int64_t b = 0; b < B; ++b) CHECK(cost[b] == cost0[b] && rew[b] == 0.f);
  return 0;
}

static int run_pairs(int64_t N) {
  for (int64_t f = 0; f < N; ++f)
    for (int64_t s = 0; s < N; ++s) {
      std::vector<float> locs(N * 2);
      for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
      std::vector<int64_t> rec = random_rec(1, N), best(rec), out(N), vt(N), act{f, s}, i{0}, i2{0};
      float cost, bsf = 1e9f, bsf2, rew;
      int32_t status = 0;
      CHECK_OK(co_tsp_kopt_step(1, N, 2, locs.data(), 1, rec.data(), act.data(), 2, 1, out.data(),
                                &cost, &bsf, &bsf2, &rew, best.data(), vt.data(), i.data(),
                                i2.data(), &status, nullptr));
      CHECK(status == 0 && is_cycle(out.data(), N) && i2[0] == 1 && best == out);
      if (f == s) CHECK(out == rec);
    }
  return 0;
}

int main() {
  const int64_t sizes[][2] = {{1, 1}, {3, 2}, {5, 3}, {4, 7}, {2, 64}, {3, 65}, {2, 1024}};
  for (const auto& c : sizes) {
    for (int layout = 0; layout < 3; ++layout)
      if (run_lists(c[0], c[1], layout)) return 1;
    for (int64_t K : {2, 3, 4, 16})
      for (int spoil = 0; spoil < 3; ++spoil)
        for (int64_t T : {0, 1, 5})
          if (run_steps(c[0], c[1], K, c[1] > 100 ? std::min<int64_t>(T, 1) : T, 1 + (c[0] % 2 == 0), spoil)) return 1;
  }
  for (int64_t N = 1; N <= 6; ++N)
    if (run_pairs(N)) return 1;
  // broken lists
  {
    std::vector<float> locs(12, 0.5f);
    std::vector<int64_t> two{1, 0, 3, 4, 5, 2}, dup{1, 2, 3, 4, 5, 5}, far{1, 2, 3, 4, 5, 600},
        out(6), vt(6);
    float cost;
    for (auto* r : {&two, &dup, &far}) {
      int32_t st = 0;
      CHECK_OK(co_tsp_kopt_reset(1, 6, locs.data(), 1, r->data(), &cost, vt.data(), &st, nullptr));
      CHECK(st == CO_ST_INVALID_TOUR);
      st = 0;
      CHECK_OK(co_tsp_real_solution(1, 6, r->data(), out.data(), &st, nullptr));
      CHECK(st == CO_ST_INVALID_TOUR);
    }
  }
  // the nearest-neighbour list
  for (int64_t N : {1, 2, 9, 130}) {
    std::vector<float> locs(3 * N * 2);
    for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
    std::vector<int64_t> rec(3 * N, -7);
    CHECK_OK(co_tsp_nearest_rec(3, N, locs.data(), rec.data(), nullptr));
    for (int64_t b = 0; b < 3; ++b) CHECK(is_cycle(rec.data() + b * N, N));
  }
  // argument errors and the empty batch
  std::vector<float> l(16), c(4);
  std::vector<int64_t> a(16), o(16), v(16);
  int32_t st = 0;
  CHECK(co_tsp_kopt_reset(1, 1025, l.data(), 1, a.data(), c.data(), v.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_reset(-1, 4, l.data(), 1, a.data(), c.data(), v.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_reset(3, 4, l.data(), 2, a.data(), c.data(), v.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_reset(1, 4, nullptr, 1, a.data(), c.data(), v.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_reset(1, 4, l.data() + 1, 1, a.data(), c.data(), v.data(), &st, nullptr) == CO_E_ALIGN);
  CHECK(co_tsp_kopt_reset(0, 4, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_tsp_kopt_steps(1, 4, 1, 1, l.data(), 1, a.data(), 4, 4, 1, o.data(), c.data(), c.data() + 1,
                          v.data(), v.data() + 4, nullptr, c.data() + 2, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_steps(1, 4, 17, 1, l.data(), 1, a.data(), 4, 4, 1, o.data(), c.data(), c.data() + 1,
                          v.data(), v.data() + 4, nullptr, c.data() + 2, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_steps(1, 4, 2, 1, l.data(), 1, a.data(), 4, 4, 1, o.data(), c.data(), c.data() + 1,
                          o.data(), v.data() + 4, nullptr, c.data() + 2, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_kopt_steps(0, 4, 2, 1, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_tsp_kopt_step(0, 4, 2, nullptr, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_tsp_linked_list(1, 1025, a.data(), 4, 1, o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_linked_list(1, 4, a.data(), 4, 1, a.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_linked_list(0, 4, nullptr, 4, 1, nullptr, nullptr, nullptr) == CO_OK);
  CHECK(co_tsp_real_solution(1, 0, a.data(), o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_nearest_rec(1, 1025, l.data(), o.data(), nullptr) == CO_E_INVAL);
  CHECK(co_tsp_nearest_rec(0, 4, nullptr, nullptr, nullptr) == CO_OK);
  std::printf("host kopt: ran clean\n");
  return 0;
}
