// Sanitizer driver for the host co_best_of and co_tsp_best_of (csrc/host/co_env_host.cpp),
// compiled together with it under -fsanitize=address,undefined by
// tests/test_host_asan_best_of.py: exactly-sized heap buffers (any out-of-bounds index is an
// ASan report), row-major, padded and step-major action rows, a few (B, K, N) of
// tests/best_of_cases.py, the nullable outputs, a non-permutation and an out-of-range index
// among the losers, NaN / signed-zero rewards and the argument errors.  Each result is
// checked against a plain loop over the candidates.  Exit 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2025);

// layout 0: rows [E, T]; 1: rows padded to T + 3; 2: step-major [T, E]
static void strides(int layout, int64_t E, int64_t T, int64_t* sb, int64_t* st, size_t* size) {
  *sb = layout == 0 ? T : layout == 1 ? T + 3 : 1;
  *st = layout == 2 ? E : 1;
  *size = (size_t)(layout == 1 ? E * (T + 3) - 3 : E * T);  // the last row's padding is absent
}

static int first_best(const float* r, int64_t B, int64_t K, int64_t b) {
  int best = 0;
  for (int64_t k = 0; k < K; ++k) {
    const float v = r[k * B + b], c = r[best * B + b];
    if (v != v) return c != c ? best : (int)k;  // the first NaN
    if (c == c && v > c) best = (int)k;
  }
  return best;
}

static int run_tsp(int64_t B, int64_t K, int64_t N, int layout, int spoil) {
  const int64_t E = K * B;
  int64_t sb, st;
  size_t size;
  strides(layout, E, N, &sb, &st, &size);
  std::vector<float> locs(B * N * 2);
  for (auto& v : locs) v = std::uniform_real_distribution<float>(0.f, 1.f)(rng);
  std::vector<int64_t> rows(E * N), acts(size, -7);
  for (int64_t e = 0; e < E; ++e) {
    for (int64_t t = 0; t < N; ++t) rows[e * N + t] = t;
    std::shuffle(rows.begin() + e * N, rows.begin() + (e + 1) * N, rng);
  }
  if (spoil == 1 && N > 1) rows[(E - 1) * N + 1] = rows[(E - 1) * N];  // not a permutation
  if (spoil == 2) rows[(E - 1) * N] = N + 5;                           // out of range
  for (int64_t e = 0; e < E; ++e)
    for (int64_t t = 0; t < N; ++t) acts[e * sb + t * st] = rows[e * N + t];
  std::vector<float> all(E, -1.f), best(B, -1.f), ref(E);
  std::vector<int64_t> idx(B, -1), out(B * N, -7);
  int32_t status = 0;
  CHECK_OK(co_tsp_best_of(B, N, K, locs.data(), acts.data(), sb, st, 1, all.data(), best.data(),
                          idx.data(), out.data(), &status, nullptr));
  CHECK(status == (spoil == 1 ? CO_ST_INVALID_TOUR
                              : spoil == 2 ? (CO_ST_INVALID_TOUR | CO_ST_INDEX_RANGE) : 0));
  int32_t st2 = 0;
  CHECK_OK(co_tsp_reward(E, N, N, locs.data(), B, acts.data(), sb, st, 0, ref.data(), &st2,
                         nullptr));
  for (int64_t e = 0; e < E; ++e) CHECK(all[e] == ref[e]);  // the host build shares the sum
  for (int64_t b = 0; b < B; ++b) {
    const int k = first_best(all.data(), B, K, b);
    CHECK(idx[b] == k && best[b] == all[k * B + b]);
    CHECK(std::equal(out.begin() + b * N, out.begin() + (b + 1) * N, rows.begin() + (k * B + b) * N));
  }
  // the nullable outputs, and check = 0 without a status word
  std::vector<float> best2(B);
  std::vector<int64_t> idx2(B);
  CHECK_OK(co_tsp_best_of(B, N, K, locs.data(), acts.data(), sb, st, 0, nullptr, best2.data(),
                          idx2.data(), nullptr, nullptr, nullptr));
  CHECK(idx2 == idx && std::equal(best.begin(), best.end(), best2.begin()));
  return 0;
}

static int run_select(int64_t B, int64_t K, int64_t T, int layout, int kind) {
  const int64_t E = K * B;
  int64_t sb, st;
  size_t size;
  strides(layout, E, T, &sb, &st, &size);
  std::vector<float> r(E);
  for (auto& v : r) v = (float)std::uniform_int_distribution<int>(-3, 3)(rng);
  if (kind == 1)
    for (auto& v : r) v = (rng() & 1) ? 0.f : -0.f;
  if (kind == 2 && K > 1)
    for (int64_t b = 0; b < B; ++b) {
      r[(1 + rng() % (K - 1)) * B + b] = std::numeric_limits<float>::quiet_NaN();
      r[(1 + rng() % (K - 1)) * B + b] = std::numeric_limits<float>::quiet_NaN();
    }
  std::vector<int64_t> acts(size);
  for (auto& v : acts) v = (int64_t)rng();
  std::vector<float> best(B);
  std::vector<int64_t> idx(B), out(B * T);
  CHECK_OK(co_best_of(B, K, T, r.data(), acts.data(), sb, st, best.data(), idx.data(),
                      out.data(), nullptr, nullptr));
  for (int64_t b = 0; b < B; ++b) {
    const int k = first_best(r.data(), B, K, b);
    CHECK(idx[b] == k);
    const float want = r[k * B + b];
    CHECK(want != want ? best[b] != best[b] : (best[b] == want && std::signbit(best[b]) == std::signbit(want)));
    for (int64_t t = 0; t < T; ++t) CHECK(out[b * T + t] == acts[(k * B + b) * sb + t * st]);
  }
  CHECK_OK(co_best_of(B, K, 0, r.data(), nullptr, 0, 0, best.data(), idx.data(), nullptr, nullptr,
                      nullptr));
  return 0;
}

int main() {
  const int64_t cases[][3] = {{3, 1, 2}, {64, 7, 3}, {257, 2, 7}, {3, 64, 64}, {1, 63, 63},
                              {1, 800, 100}, {3, 5, 1024}};  // (B, K, N)
  for (const auto& c : cases)
    for (int layout = 0; layout < 3; ++layout) {
      for (int spoil = 0; spoil < 3; ++spoil)
        if (run_tsp(c[0], c[1], c[2], layout, c[1] > 1 ? spoil : 0)) return 1;
      for (int kind = 0; kind < 3; ++kind)
        if (run_select(c[0], c[1], std::min<int64_t>(c[2], 9), layout, kind)) return 1;
    }
  // argument errors and the empty batch
  std::vector<float> l(16), r(8);
  std::vector<int64_t> a(16), o(16), ix(4);
  int32_t st = 0;
  CHECK(co_tsp_best_of(-1, 4, 2, l.data(), a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 4, 0, l.data(), a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 1025, 2, l.data(), a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 4, 2, nullptr, a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 4, 2, l.data(), a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       a.data(), &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 4, 2, l.data(), a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), nullptr, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_best_of(2, 4, 2, l.data() + 1, a.data(), 4, 1, 1, nullptr, r.data(), ix.data(),
                       o.data(), &st, nullptr) == CO_E_ALIGN);
  CHECK(co_tsp_best_of(0, 4, 2, nullptr, nullptr, 4, 1, 1, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr) == CO_OK);
  CHECK(co_best_of(2, 0, 4, r.data(), a.data(), 4, 1, r.data(), ix.data(), o.data(), nullptr,
                   nullptr) == CO_E_INVAL);
  CHECK(co_best_of(2, 2, 4, r.data(), nullptr, 4, 1, r.data(), ix.data(), o.data(), nullptr,
                   nullptr) == CO_E_INVAL);
  CHECK(co_best_of(2, 2, 4, r.data(), a.data(), 4, 1, r.data(), ix.data(), a.data(), nullptr,
                   nullptr) == CO_E_INVAL);
  CHECK(co_best_of(0, 2, 4, nullptr, nullptr, 4, 1, nullptr, nullptr, nullptr, nullptr,
                   nullptr) == CO_OK);
  std::printf("host best_of: ran clean\n");
  return 0;
}
