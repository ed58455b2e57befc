// Sanitizer driver for the host co_cvrp_local_search (csrc/host/co_env_host.cpp), compiled
// together with it under -fsanitize=address,undefined by tests/test_host_asan.py:
// exactly-sized heap buffers (any out-of-bounds index is an ASan report), both distance
// sources, row-major and step-major actions, a multistart instance batch, N in
// {1, 2, 3, 21, 65}, explicit and default capacity, invalid rows, max_iterations = 0 and
// the argument errors.  Each result is checked to visit every customer once, to keep every
// route within capacity and to be no longer than its input.  Exit 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2025);

static double route_len(const float* D, int64_t V, const int64_t* t, int64_t T) {
  double s = 0;
  int64_t prev = 0;
  for (int64_t k = 0; k < T; ++k) {
    s += D[prev * V + t[k]];
    prev = t[k];
  }
  return s + D[prev * V];
}

static int run(int64_t B, int64_t LB, int64_t N, bool matrix, bool step_major, bool with_cap,
               int64_t max_it, int64_t bad_row) {
  const int64_t V = N + 1, T = 2 * N + 3;
  std::vector<float> locs(LB * V * 2), D(LB * V * V), demand(LB * N), cap(LB, 1.0f);
  for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  for (auto& v : demand) v = (float)std::uniform_int_distribution<int>(1, 9)(rng) / 30.0f;
  for (int64_t b = 0; b < LB; ++b)
    for (int64_t i = 0; i < V; ++i)
      for (int64_t j = 0; j < V; ++j) {
        const float dx = locs[(b * V + j) * 2] - locs[(b * V + i) * 2];
        const float dy = locs[(b * V + j) * 2 + 1] - locs[(b * V + i) * 2 + 1];
        D[(b * V + i) * V + j] = std::sqrt(dx * dx + dy * dy);
      }
  // random permutations cut where the running load would pass the capacity
  std::vector<int64_t> rows(B * T, 0), acts(B * T), out(B * T, -7);
  for (int64_t b = 0; b < B; ++b) {
    std::vector<int64_t> perm(N);
    for (int64_t k = 0; k < N; ++k) perm[k] = k + 1;
    std::shuffle(perm.begin(), perm.end(), rng);
    int64_t w = 0;
    float used = 0.f;
    for (int64_t c : perm) {
      const float d = demand[(b % LB) * N + c - 1];
      if (used + d > 1.0f) {
        rows[b * T + w++] = 0;
        used = 0.f;
      }
      rows[b * T + w++] = c;
      used += d;
    }
  }
  if (bad_row >= 0 && bad_row < B) rows[bad_row * T] = N > 1 ? rows[bad_row * T + 1] : N + 3;
  const int64_t sb = step_major ? 1 : T, st = step_major ? B : 1;
  for (int64_t b = 0; b < B; ++b)
    for (int64_t k = 0; k < T; ++k) acts[b * sb + k * st] = rows[b * T + k];
  std::vector<int32_t> sweeps(B, -1);
  int32_t status = 0;
  const float* lp = matrix ? nullptr : locs.data();
  const float* dp = matrix ? D.data() : nullptr;
  const float* cp = with_cap ? cap.data() : nullptr;
  CHECK(co_cvrp_local_search(B, N, T, lp, dp, demand.data(), cp, LB, acts.data(), sb, st, max_it,
                             out.data(), sweeps.data(), &status, nullptr) == CO_OK);
  const bool has_bad = bad_row >= 0 && bad_row < B;  // a duplicate, a missing customer or N + 3
  CHECK((status == CO_ST_INVALID_TOUR) == has_bad);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* in = rows.data() + b * T;
    const int64_t* o = out.data() + b * T;
    if (b == bad_row && has_bad) {
      CHECK(std::equal(in, in + T, o));
      CHECK(sweeps[b] == 0);
      continue;
    }
    std::vector<int64_t> seen(V, 0);
    float used = 0.f;
    for (int64_t k = 0; k < T; ++k) {
      CHECK(o[k] >= 0 && o[k] <= N);
      if (o[k] == 0) {
        used = 0.f;
        continue;
      }
      CHECK(!seen[o[k]]++);
      used += demand[(b % LB) * N + o[k] - 1];
      CHECK(b == bad_row || used <= 1.0f + 1e-5f);
    }
    for (int64_t c = 1; c <= N; ++c) CHECK(seen[c] == 1);
    CHECK(max_it <= 0 ? sweeps[b] == 0 : (sweeps[b] >= 1 && sweeps[b] <= max_it));
    const float* Db = D.data() + (b % LB) * V * V;
    CHECK(route_len(Db, V, o, T) <= route_len(Db, V, in, T) + 1e-4);
  }
  // sweeps_out is optional
  CHECK(co_cvrp_local_search(B, N, T, lp, dp, demand.data(), cp, LB, acts.data(), sb, st, max_it,
                             out.data(), nullptr, &status, nullptr) == CO_OK);
  return 0;
}

int main() {
  for (int64_t N : {1, 2, 3, 21, 65})
    for (bool matrix : {false, true})
      for (bool step_major : {false, true}) {
        if (run(6, 6, N, matrix, step_major, true, 1000, -1)) return 1;
        if (run(6, 3, N, matrix, step_major, false, 1000, 2)) return 1;  // multistart + bad row
        if (run(5, 5, N, matrix, step_major, false, 0, -1)) return 1;
        if (run(5, 5, N, matrix, step_major, true, 2, 4)) return 1;
      }
  // argument errors and the empty batch
  std::vector<float> l(9 * 2), d(9 * 9), dem(8);
  std::vector<int64_t> a(12), o(12);
  int32_t st = 0;
  CHECK(co_cvrp_local_search(1, 8, 12, l.data(), d.data(), dem.data(), nullptr, 1, a.data(), 12,
                             1, 5, o.data(), nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_cvrp_local_search(1, 8, 12, nullptr, nullptr, dem.data(), nullptr, 1, a.data(), 12, 1,
                             5, o.data(), nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_cvrp_local_search(1, 8, 7, l.data(), nullptr, dem.data(), nullptr, 1, a.data(), 7, 1,
                             5, o.data(), nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_cvrp_local_search(1, 600, 1024, l.data(), nullptr, dem.data(), nullptr, 1, a.data(),
                             1024, 1, 5, o.data(), nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_cvrp_local_search(0, 8, 12, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 12, 1, 5,
                             nullptr, nullptr, nullptr, nullptr) == CO_OK);
  std::printf("host cvrp_local_search: ran clean\n");
  return 0;
}
