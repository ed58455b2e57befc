// Sanitizer driver for the host co_tsp_local_search (csrc/host/co_env_host.cpp), compiled
// together with it under -fsanitize=address,undefined by tests/test_host_asan_tsp_ls.py:
// exactly-sized heap buffers (any out-of-bounds index is an ASan report).
//  - forced moves: on the identity tour of a matrix that is 10 everywhere except the three
//    edges a designated Or-opt move (L, i, k, rev) creates (1 each), that move is the only
//    best one; n in {3, 4, 7, 65}, every L that has a move, at both ends of the position
//    range (i = 1, i+L-1 = n-1, k = 0, k = n-1), both orientations.  One sweep must give
//    the tour with the segment re-inserted after position k;
//  - random runs: both distance sources, every operator mask, row-major and step-major
//    actions, a multistart coordinate batch, an invalid row, max_iterations = 0, with and
//    without sweeps_out / moves_out; each result is a permutation that keeps position 0
//    and is no longer than its input;
//  - the argument errors.  Exit 0 = clean.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/co_env.h"
#include "check.h"

static std::mt19937_64 rng(2025);

static double tour_len(const std::vector<float>& D, int64_t n, const int64_t* t) {
  double s = 0;
  for (int64_t k = 0; k < n; ++k) s += D[t[k] * n + t[(k + 1) % n]];
  return s;
}

static int forced(int64_t n, int64_t L, int64_t i, int64_t k, int rev) {
  std::vector<float> D(n * n, 10.f);
  const int64_t a = i - 1, s1 = i, s2 = i + L - 1, b = (i + L) % n, c = k, d = (k + 1) % n;
  const int64_t x = rev ? s2 : s1, y = rev ? s1 : s2;
  D[a * n + b] = D[c * n + x] = D[y * n + d] = 1.f;
  std::vector<int64_t> in(n), out(n, -7), want;
  for (int64_t p = 0; p < n; ++p) in[p] = p;
  for (int64_t p = 0; p < n; ++p) {
    if (p < i || p > s2) want.push_back(p);
    if (p == k)
      for (int64_t u = 0; u < L; ++u) want.push_back(rev ? s2 - u : s1 + u);
  }
  CHECK((int64_t)want.size() == n);
  int32_t status = 0, sweeps = -1, moves[2] = {-1, -1};
  CHECK(co_tsp_local_search(1, n, nullptr, D.data(), 1, in.data(), n, 1, 1, CO_TSP_LS_OR_OPT,
                            out.data(), &sweeps, moves, &status, nullptr) == CO_OK);
  CHECK(status == 0 && sweeps == 1 && moves[0] == 0 && moves[1] == 1);
  CHECK(out == want);
  return 0;
}

static int run(int64_t B, int64_t LB, int64_t N, bool matrix, bool step_major, int64_t max_it,
               int ops, int64_t bad_row) {
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
  std::vector<int32_t> sweeps(B, -1), moves(2 * B, -1);
  int32_t status = 0;
  CHECK(co_tsp_local_search(B, N, matrix ? nullptr : locs.data(), matrix ? D.data() : nullptr,
                            LB, acts.data(), sb, st, max_it, ops, out.data(), sweeps.data(),
                            moves.data(), &status, nullptr) == CO_OK);
  CHECK((status == CO_ST_INVALID_TOUR) == (bad_row >= 0 && bad_row < B));
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* in = rows.data() + b * N;
    const int64_t* o = out.data() + b * N;
    if (b == bad_row || max_it <= 0 || N < 3) {
      CHECK(std::equal(in, in + N, o));
      CHECK(sweeps[b] == (b == bad_row || max_it <= 0 ? 0 : 1));
      CHECK(moves[2 * b] == 0 && moves[2 * b + 1] == 0);
      continue;
    }
    std::vector<int64_t> sorted(o, o + N);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t k = 0; k < N; ++k) CHECK(sorted[k] == k);
    CHECK(o[0] == in[0]);
    CHECK(sweeps[b] >= 1 && sweeps[b] <= max_it);
    CHECK(moves[2 * b] >= 0 && moves[2 * b + 1] >= 0);
    CHECK(moves[2 * b] + moves[2 * b + 1] <= sweeps[b]);
    CHECK(moves[2 * b] + moves[2 * b + 1] >= sweeps[b] - 1);
    if (!(ops & CO_TSP_LS_TWO_OPT)) CHECK(moves[2 * b] == 0);
    if (!(ops & CO_TSP_LS_OR_OPT)) CHECK(moves[2 * b + 1] == 0);
    const std::vector<float> Db(D.begin() + (b % LB) * N * N, D.begin() + (b % LB + 1) * N * N);
    CHECK(tour_len(Db, N, o) <= tour_len(Db, N, in) + 1e-4);
  }
  // sweeps_out and moves_out are optional
  CHECK(co_tsp_local_search(B, N, matrix ? nullptr : locs.data(), matrix ? D.data() : nullptr,
                            LB, acts.data(), sb, st, max_it, ops, out.data(), nullptr, nullptr,
                            &status, nullptr) == CO_OK);
  return 0;
}

int main() {
  int forced_runs = 0;
  for (int64_t n : {3, 4, 7, 65})
    for (int64_t L = 1; L <= 3 && n - L - 1 >= 1; ++L)
      for (int64_t i : {(int64_t)1, n - L})
        for (int64_t k : {(int64_t)0, n - 1}) {
          if (k >= i - 1 && k <= i + L - 1) continue;
          for (int rev = 0; rev < (L > 1 ? 2 : 1); ++rev) {
            if (forced(n, L, i, k, rev)) return 1;
            ++forced_runs;
          }
        }
  CHECK(forced_runs == 28);
  for (int64_t N : {1, 3, 4, 7, 65})
    for (bool matrix : {false, true})
      for (int ops : {CO_TSP_LS_TWO_OPT, CO_TSP_LS_OR_OPT, CO_TSP_LS_TWO_OPT | CO_TSP_LS_OR_OPT}) {
        if (run(6, 6, N, matrix, false, 1000, ops, -1)) return 1;
        if (run(6, 3, N, matrix, true, 1000, ops, 2)) return 1;  // multistart + invalid row
        if (run(5, 5, N, matrix, true, 0, ops, -1)) return 1;
        if (run(5, 5, N, matrix, false, 2, ops, 4)) return 1;
      }
  // argument errors and the empty batch
  std::vector<float> l(8 * 2), d(8 * 8);
  std::vector<int64_t> a(8), o(8);
  int32_t st = 0;
  const int both = CO_TSP_LS_TWO_OPT | CO_TSP_LS_OR_OPT;
  CHECK(co_tsp_local_search(1, 8, l.data(), d.data(), 1, a.data(), 8, 1, 5, both, o.data(),
                            nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_local_search(1, 8, nullptr, nullptr, 1, a.data(), 8, 1, 5, both, o.data(),
                            nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_local_search(1, CO_TWO_OPT_MAX_N + 1, l.data(), nullptr, 1, a.data(), 8, 1, 5,
                            both, o.data(), nullptr, nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_local_search(1, 8, l.data(), nullptr, 1, a.data(), 8, 1, 5, 0, o.data(), nullptr,
                            nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_local_search(1, 8, l.data(), nullptr, 1, a.data(), 8, 1, 5, 4, o.data(), nullptr,
                            nullptr, &st, nullptr) == CO_E_INVAL);
  CHECK(co_tsp_local_search(0, 8, nullptr, nullptr, 1, nullptr, 8, 1, 5, both, nullptr, nullptr,
                            nullptr, nullptr, nullptr) == CO_OK);
  std::printf("host tsp_local_search: ran clean\n");
  return 0;
}
