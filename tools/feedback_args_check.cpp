// Stand-alone host check of insite_feedback.h's argument validation: every call here returns before any HIP call, so it
// needs no device.  Meant for a sanitizer build of the host code, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I<csrc> \
//         -o feedback_args_check <csrc>/insite_feedback.hip -x c++ tools/feedback_args_check.cpp -fsanitize=address,undefined
// (<csrc>: the package's csrc directory).  Besides the header's list it sweeps the leading dimensions and the rule table
// over boundary values (near 2^31, 2^62 and 2^63; arms, periods and flags at and past their bounds) with n_rows = 0, so
// that nothing launches, and with rows and a NULL `choice`, so that the call gets through every check and still returns
// before the launch: no signed overflow may happen on the way to either answer, and the rule table is read inside its
// n_rules rows only (it is allocated exactly, so the address sanitizer sees a read past it).  Exit status 0 and
// "0 failure(s)" when every status is the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "insite_feedback.h"
static int fails = 0;
#define EXPECT(e, want) do { long long got_ = (long long)(e); if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #e, got_, (long long)(want)); ++fails; } } while (0)
int main() {
  std::vector<double> x(4096, 0.0);
  std::vector<int8_t> sc(4096, 0);
  std::vector<int32_t> ch(64, 0);
  int8_t exps[7 * 3] = {0,0,0, 1,0,0, 0,1,0, 0,0,1, 1,1,0, 1,0,1, 0,1,1};
  double q[16] = {0.025, 0.5, 0.975, 0, 1, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8, 0.9, 0.25, 0.75, 0.5};
  double ac[4] = {0.0, 0.01, -0.01, 0.5};
  double* d = x.data();
  auto table = [](int K) {  // exactly K rows on the heap: (1, 0, 1 + j, j % 2)
    std::vector<int32_t> r((size_t)K * 4);
    for (int j = 0; j < K; ++j) { r[4 * j] = 1; r[4 * j + 1] = 0; r[4 * j + 2] = 1 + j; r[4 * j + 3] = j % 2; }
    return r;
  };
  // N = 5, T = 12, K = 3, Q = 3: ld_theta 6, ld_w 12, ld_out 54, ld_sched 36
  auto call = [&](int64_t N, int T, int K, int64_t ldt, int64_t ldw, int64_t ldo, int64_t lds, int sense = 1, int R = 9,
                  int Q = 3, int A = 2, int F = 7, int m = 0, const int32_t* rules = nullptr, bool with_sched = true,
                  bool with_choice = true) {
    std::vector<int32_t> r = table(K > 0 && K <= 64 ? K : 1);
    return insite_feedback_rules_f64(d, d, d, ldt, rules ? rules : r.data(), K, d, ldw, d, ac, sense, d, exps, F, N, T, 2, A,
                                     0.1, m, 5, 1e-3, R, q, Q, with_choice ? ch.data() : nullptr, d, d, ldo,
                                     with_sched ? sc.data() : nullptr, lds, nullptr);
  };
  EXPECT(insite_feedback_abi_version(), 1);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36), INSITE_OK);
  EXPECT(call(-1, 12, 3, 6, 12, 54, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 0, 3, 6, 12, 54, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 0, 6, 12, 54, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, -1, 6, 12, 54, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 17, 34, 12, 17 * 3 * 6, 17 * 12), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 16, 32, 12, 16 * 3 * 6, 16 * 12), INSITE_OK);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 0), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 2), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, -1), INSITE_OK);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 1), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 513), INSITE_E_UNSUPPORTED);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 512), INSITE_OK);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 9, 0), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 3 * 3 * 20, 36, 1, 9, 17), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 3 * 3 * 19, 36, 1, 9, 16), INSITE_OK);
  EXPECT(call(0, 12, 3, 6, 12, 3 * 3 * 19 - 1, 36, 1, 9, 16), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 9, 3, 5), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 9, 3, 2, 10), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, 36, 1, 9, 3, 2, 7, 2), INSITE_E_UNSUPPORTED);
  for (int ld = 1; ld < 12; ++ld) EXPECT(call(0, 12, 3, 6, ld, 54, 36), INSITE_E_INVALID_ARG);
  for (int ld = 1; ld < 6; ++ld) EXPECT(call(0, 12, 3, ld, 12, 54, 36), INSITE_E_INVALID_ARG);
  for (int ld = -1; ld < 36; ++ld) EXPECT(call(0, 12, 3, 6, 12, 54, ld), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 6, 12, 54, -1, 1, 9, 3, 2, 7, 0, nullptr, false), INSITE_OK);   // no schedule: ld_sched unread
  EXPECT(call(0, 12, 3, 0, 0, 54, 36), INSITE_OK);
  EXPECT(call(5, 12, 3, 6, 12, 53, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(5, 12, 3, 6, 12, 54, 36, 1, 9, 3, 2, 7, 0, nullptr, true, false), INSITE_E_INVALID_ARG);   // NULL choice
  EXPECT(insite_feedback_rules_f64(d, d, d, 6, nullptr, 3, d, 12, d, ac, 1, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, q, 3,
                                   ch.data(), d, d, 54, sc.data(), 36, nullptr), INSITE_E_INVALID_ARG);   // NULL rules
  double qbad[3] = {0.5, 1.5, 0.1};
  {
    std::vector<int32_t> r = table(3);
    EXPECT(insite_feedback_rules_f64(d, d, d, 6, r.data(), 3, d, 12, d, ac, 1, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, qbad,
                                     3, ch.data(), d, d, 54, sc.data(), 36, nullptr), INSITE_E_INVALID_ARG);
    EXPECT(insite_feedback_rules_f64(d, d, d, 6, r.data(), 3, d, 12, d, nullptr, 1, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9,
                                     q, 3, ch.data(), d, d, 54, nullptr, 0, nullptr), INSITE_OK);   // NULL arm_cost, sched
  }
  // the rule table: every field of every row at and past its bounds, for every arm count
  const int32_t vals[] = {0, 1, 2, 3, 4, 5, 127, 128, 255, 256, 65536, INT32_MAX, INT32_MAX - 1, -1, -2, INT32_MIN, INT32_MIN + 1};
  long long r_ok = 0, r_bad = 0;
  for (int A = 1; A <= 4; ++A) for (int K : {1, 3, 16}) for (int row : {0, K - 1}) for (int col = 0; col < 4; ++col)
    for (int32_t v : vals) {
      std::vector<int32_t> r = table(K);
      for (int j = 0; j < K; ++j) r[4 * j] = A - 1;   // a valid table for this arm count
      r[4 * row + col] = v;
      const bool ok = col < 2 ? (v >= 0 && v < A) : (col == 2 ? v >= 1 : (v == 0 || v == 1));
      for (int64_t N : {(int64_t)0, (int64_t)5}) {
        const int32_t st = call(N, 12, K, 2 * K, 12, (int64_t)K * 18, (int64_t)K * 12, 1, 9, 3, A, 7, 0, r.data(), true, false);
        // with rows the NULL choice refuses a valid table too: never INSITE_OK there
        const int32_t want = ok && N == 0 ? INSITE_OK : INSITE_E_INVALID_ARG;
        if (st != want) { std::printf("FAIL rules A=%d K=%d row=%d col=%d v=%d N=%lld: %d\n", A, K, row, col, v, (long long)N, st); ++fails; }
        (st == INSITE_OK ? r_ok : r_bad)++;
      }
    }
  // the sweep of the leading dimensions: every combination answers INSITE_OK or INSITE_E_INVALID_ARG and nothing
  // overflows on the way.  With n_rows = 0 nothing can launch; with rows a NULL `choice` stops the call after the checks.
  const int64_t big[] = {0, 1, 2, 5, 6, 11, 12, 13, 32, 36, 54, (int64_t)1 << 31, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) + 1,
                         (int64_t)1 << 62, ((int64_t)1 << 62) - 1, ((int64_t)1 << 62) + 1, INT64_MAX, INT64_MAX - 1,
                         INT64_MAX / 2, INT64_MAX / 3, INT64_MAX / 4, -1, INT64_MIN};
  const int64_t rows[] = {0, 1, 5, (int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX};
  const int Ks[] = {1, 2, 3, 16};
  const int Ts[] = {1, 12, 2147483647};
  long long n_ok = 0, n_bad = 0, n_other = 0;
  for (int64_t N : rows) for (int K : Ks) for (int T : Ts) for (int64_t ldt : big) for (int64_t ldx : big) for (int64_t ldy : big) {
    // ldx plays ld_w and ld_out in turn, ldy ld_sched (with and without a schedule), so the sweep stays cubic
    for (int which = 0; which < 2; ++which) for (int ws = 0; ws < 2; ++ws) {
      const int64_t ldw = which == 0 ? ldx : 0;
      const int64_t ldo = which == 1 ? ldx : (int64_t)K * 3 * 6;
      const int32_t st = call(N, T, K, ldt, ldw, ldo, ldy, 1, 9, 3, 2, 7, 0, nullptr, ws == 1, false);
      if (st == INSITE_OK) { ++n_ok; if (N != 0) { std::printf("FAIL launch path reached at N=%lld\n", (long long)N); ++fails; } }
      else if (st == INSITE_E_INVALID_ARG) ++n_bad;
      else ++n_other;
      // the documented bounds, restated: whatever the sweep accepts with n_rows = 0 obeys them
      if (st == INSITE_OK && ((ldt != 0 && ldt < 2 * (int64_t)K) || ldt < 0 || (ldw != 0 && ldw < T) || ldw < 0 ||
                              ldo < (int64_t)K * 3 * 6 || (ws == 1 && ldy < (int64_t)K * T))) {
        std::printf("FAIL accepted ldt=%lld ldw=%lld ldo=%lld lds=%lld T=%d K=%d\n", (long long)ldt, (long long)ldw,
                    (long long)ldo, (long long)ldy, T, K);
        ++fails;
      }
    }
  }
  EXPECT(n_other, 0);
  // the accepted side at the extremes
  EXPECT(call(0, 12, 2, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62), INSITE_OK);
  EXPECT(call(0, 2147483647, 16, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX), INSITE_OK);
  EXPECT(call(0, 2147483647, 16, 32, 0, 288, (int64_t)16 * 2147483647 - 1), INSITE_E_INVALID_ARG);
  EXPECT(call(5, 12, 3, (int64_t)1 << 62, 12, 54, 36, 1, 9, 3, 2, 7, 0, nullptr, true, false), INSITE_E_INVALID_ARG);   // 4 ld_theta leaves int64
  std::printf("rules: %lld accepted, %lld refused; sweep: %lld accepted (n_rows = 0), %lld refused; %d failure(s)\n", r_ok,
              r_bad, n_ok, n_bad, fails);
  return fails ? 1 : 0;
}
