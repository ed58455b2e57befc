// Sanitizer driver for the host co_tsp_two_opt (csrc/host/co_env_host.cpp), compiled
// together with it under -fsanitize=address,undefined by tests/test_host_asan.py:
// exactly-sized heap buffers (any out-of-bounds index is an ASan report), both distance
// sources, row-major and step-major actions, a multistart coordinate batch, N in
// {1, 3, 4, 65}, an invalid row, max_iterations = 0 and the argument errors.  Each result
// is checked to be a permutation no longer than its input.  Exit 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2024);

static double tour_len(const std::vector<float>& D, int64_t n, const int64_t* t) {
  double s = 0;
  for (int64_t k = 0; k < n; ++k) s += D[t[k] * n + t[(k + 1) % n]];
  return s;
}

static int run(int64_t B, int64_t LB, int64_t N, bool matrix, bool step_major, int64_t max_it,
               int64_t bad_row) {
  std::vector<float> locs(LB * N * 2), D(LB * N * N);
  for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  for (int64_t b = 0; b < LB; ++b)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t j = 0; j < N; ++j) {
        const float dx = locs[(b * N + j) * 2] - locs[(b * N + i) * 2];
        const float dy = locs[(b * N + j) * 2 + 1] - locs[(b * N + i) * 2 + 1];
        D[(b * N + i) * N + j] = std::sqrt(dx * dx + dy * dy);
      }
  std::vector<int64_t> rows(B * N), acts(B * N), out(B * N, -7);
  for (int64_t b = 0; b < B; ++b) {
    for (int64_t k = 0; k < N; ++k) rows[b * N + k] = k;
    std::shuffle(rows.begin() + b * N, rows.begin() + (b + 1) * N, rng);
  }
  if (bad_row >= 0 && bad_row < B) rows[bad_row * N + N - 1] = N > 1 ? rows[bad_row * N] : N + 3;
  const int64_t sb = step_major ? 1 : N, st = step_major ? B : 1;
  for (int64_t b = 0; b < B; ++b)
    for (int64_t k = 0; k < N; ++k) acts[b * sb + k * st] = rows[b * N + k];
  std::vector<int32_t> sweeps(B, -1);
  int32_t status = 0;
  CHECK(co_tsp_two_opt(B, N, matrix ? nullptr : locs.data(), matrix ? D.data() : nullptr, LB,
                       acts.data(), sb, st, max_it, out.data(), sweeps.data(), &status,
                       nullptr) == CO_OK);
  CHECK((status == CO_ST_INVALID_TOUR) == (bad_row >= 0 && bad_row < B));
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* in = rows.data() + b * N;
    const int64_t* o = out.data() + b * N;
    if (b == bad_row || max_it <= 0 || N < 3) {
      CHECK(std::equal(in, in + N, o));
      CHECK(sweeps[b] == (b == bad_row || max_it <= 0 ? 0 : 1));
      continue;
    }
    std::vector<int64_t> sorted(o, o + N);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t k = 0; k < N; ++k) CHECK(sorted[k] == k);
    CHECK(sweeps[b] >= 1 && sweeps[b] <= max_it);
    const std::vector<float> Db(D.begin() + (b % LB) * N * N, D.begin() + (b % LB + 1) * N * N);
    CHECK(tour_len(Db, N, o) <= tour_len(Db, N, in) + 1e-4);
  }
  // sweeps_out is optional
  CHECK(co_tsp_two_opt(B, N, matrix ? nullptr : locs.data(), matrix ? D.data() : nullptr, LB,
                       acts.data(), sb, st, max_it, out.data(), nullptr, &status,
                       nullptr) == CO_OK);
  return 0;
}

int main() {
  for (int64_t N : {1, 3, 4, 65})
    for (bool matrix : {false, true})
      for (bool step_major : {false, true}) {
        if (run(6, 6, N, matrix, step_major, 1000, -1)) return 1;
        if (run(6, 3, N, matrix, step_major, 1000, 2)) return 1;  // multistart + invalid row
        if (run(5, 5, N, matrix, step_major, 0, -1)) return 1;
        if (run(5, 5, N, matrix, step_major, 2, 4)) return 1;
      }
  // argument errors and the empty batch
  std::vector<float> l(8 * 2), d(8 * 8);
  std::vector<int64_t> a(8), o(8);
  int32_t st = 0;
  CHECK(co_tsp_two_opt(1, 8, l.data(), d.data(), 1, a.data(), 8, 1, 5, o.data(), nullptr, &st,
                       nullptr) == CO_E_INVAL);
  CHECK(co_tsp_two_opt(1, 8, nullptr, nullptr, 1, a.data(), 8, 1, 5, o.data(), nullptr, &st,
                       nullptr) == CO_E_INVAL);
  CHECK(co_tsp_two_opt(1, CO_TWO_OPT_MAX_N + 1, l.data(), nullptr, 1, a.data(), 8, 1, 5,
                       o.data(), nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_two_opt(0, 8, nullptr, nullptr, 1, nullptr, 8, 1, 5, nullptr, nullptr, nullptr,
                       nullptr) == CO_OK);
  std::printf("host two_opt: ran clean\n");
  return 0;
}
