// Sanitizer driver for the host co_slap_local_search (csrc/host/co_env_host.cpp), compiled
// together with it under -fsanitize=address,undefined by tests/test_host_asan.py:
// exactly-sized heap buffers (any out-of-bounds index is an ASan report), both distance
// sources, a multistart instance batch, (P, L) in {(1, 2), (2, 3), (5, 8), (20, 100),
// (31, 32), (64, 130)}, rows that fail each part of the check, max_iterations = 0 and the
// argument errors.  Each result is checked to be an assignment whose recomputed objective is
// cost_out and no higher than the input's.  Exit 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2026);

static int64_t objective(const float* D, int64_t L, const int64_t* pl, int64_t O, int64_t K,
                         const int32_t* s) {
  int64_t f = 0;
  for (int64_t o = 0; o < O; ++o)
    for (int64_t k = 0; k < K; ++k) {
      const int64_t a = pl[o * K + k], c = pl[o * K + (k + 1) % K];
      if (a != c) f += std::llrint((double)D[s[a] * L + s[c]] * 1048576.0);
    }
  return f;
}

// bad: 0 none, 1 duplicate slot, 2 slot -1, 3 slot L, 4 picklist entry P, 5 NaN source
static int run(int64_t B, int64_t LB, int64_t P, int64_t L, bool matrix, int64_t max_it, int bad) {
  const int64_t O = 6, K = 4, bad_row = B - 1;
  std::vector<float> locs(LB * L * 2), D(LB * L * L);
  for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 10.f)(rng);
  for (int64_t b = 0; b < LB; ++b)
    for (int64_t i = 0; i < L; ++i)
      for (int64_t j = 0; j < L; ++j) {
        const float dx = locs[(b * L + j) * 2] - locs[(b * L + i) * 2];
        const float dy = locs[(b * L + j) * 2 + 1] - locs[(b * L + i) * 2 + 1];
        D[(b * L + i) * L + j] = std::sqrt(dx * dx + dy * dy);
      }
  std::vector<int64_t> pl(LB * O * K);
  for (auto& v : pl) v = std::uniform_int_distribution<int64_t>(0, P - 1)(rng);
  std::vector<int32_t> rows(B * P), out(B * P, -7), sweeps(B, -1);
  std::vector<int64_t> cost(B, -7);
  for (int64_t b = 0; b < B; ++b) {
    std::vector<int32_t> perm(L);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin() + (b % 2), perm.end(), rng);  // odd rows keep clear of slot 0
    std::copy(perm.begin() + (b % 2), perm.begin() + (b % 2) + P, rows.begin() + b * P);
  }
  const int64_t bad_inst = bad_row % LB;
  if (bad == 1 && P > 1) rows[bad_row * P + 1] = rows[bad_row * P];
  if (bad == 1 && P == 1) bad = 2;
  if (bad == 2) rows[bad_row * P] = -1;
  if (bad == 3) rows[bad_row * P + P - 1] = (int32_t)L;
  if (bad == 4) pl[bad_inst * O * K + 5] = P;
  if (bad == 5) (matrix ? D[bad_inst * L * L + 1] : locs[bad_inst * L * 2 + 1]) = NAN;
  int32_t status = 0;
  const float* lp = matrix ? nullptr : locs.data();
  const float* dp = matrix ? D.data() : nullptr;
  CHECK(co_slap_local_search(B, L, P, O, K, lp, dp, LB, pl.data(), rows.data(), max_it,
                             out.data(), sweeps.data(), cost.data(), &status, nullptr) == CO_OK);
  CHECK(status == (bad == 0 ? 0 : bad == 4 ? CO_ST_INDEX_RANGE : CO_ST_INVALID_TOUR));
  for (int64_t b = 0; b < B; ++b) {
    const int32_t* in = rows.data() + b * P;
    const int32_t* o = out.data() + b * P;
    if (bad && b % LB == bad_inst && (bad >= 4 || b == bad_row)) {
      CHECK(std::equal(in, in + P, o));
      CHECK(sweeps[b] == 0 && cost[b] == -1);
      continue;
    }
    std::vector<int> seen(L, 0);
    for (int64_t p = 0; p < P; ++p) {
      CHECK(o[p] >= 0 && o[p] < L);
      CHECK(!seen[o[p]]++);
    }
    CHECK(max_it <= 0 ? sweeps[b] == 0 : (sweeps[b] >= 1 && sweeps[b] <= max_it));
    const float* Db = D.data() + (b % LB) * L * L;
    const int64_t* plb = pl.data() + (b % LB) * O * K;
    CHECK(objective(Db, L, plb, O, K, o) == cost[b]);
    CHECK(cost[b] <= objective(Db, L, plb, O, K, in));
  }
  // sweeps_out and cost_out are optional
  CHECK(co_slap_local_search(B, L, P, O, K, lp, dp, LB, pl.data(), rows.data(), max_it,
                             out.data(), nullptr, nullptr, &status, nullptr) == CO_OK);
  return 0;
}

int main() {
  const int64_t shapes[][2] = {{1, 2}, {2, 3}, {5, 8}, {20, 100}, {31, 32}, {64, 130}};
  for (const auto& sh : shapes)
    for (bool matrix : {false, true}) {
      if (run(6, 6, sh[0], sh[1], matrix, 1000, 0)) return 1;
      if (run(6, 3, sh[0], sh[1], matrix, 1000, 0)) return 1;  // multistart
      if (run(5, 5, sh[0], sh[1], matrix, 0, 0)) return 1;
      for (int bad = 1; bad <= 5; ++bad)
        if (run(6, 3, sh[0], sh[1], matrix, 2, bad)) return 1;
    }
  // argument errors and the empty batch
  std::vector<float> l(8 * 2), d(8 * 8);
  std::vector<int64_t> pl(12);
  std::vector<int32_t> a(5), o(5);
  int32_t st = 0;
  CHECK(co_slap_local_search(1, 8, 5, 4, 3, l.data(), d.data(), 1, pl.data(), a.data(), 5,
                             o.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_slap_local_search(1, 8, 5, 4, 3, nullptr, nullptr, 1, pl.data(), a.data(), 5,
                             o.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_slap_local_search(1, 4, 5, 4, 3, l.data(), nullptr, 1, pl.data(), a.data(), 5,
                             o.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_slap_local_search(1, 1025, 5, 4, 3, l.data(), nullptr, 1, pl.data(), a.data(), 5,
                             o.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_slap_local_search(1, 8, 5, 4, 3, l.data(), nullptr, 1, pl.data(), a.data(), 5,
                             a.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_slap_local_search(0, 8, 5, 4, 3, nullptr, nullptr, 1, nullptr, nullptr, 5, nullptr,
                             nullptr, nullptr, nullptr, nullptr) == CO_OK);
  std::printf("host slap_local_search: ran clean\n");
  return 0;
}
