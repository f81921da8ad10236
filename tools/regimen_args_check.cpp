// Stand-alone host check of insite_regimen.h's argument validation: every call here returns before any HIP call, so it
// needs no device.  Meant for a sanitizer build of the host code, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I<csrc> \
//         -o regimen_args_check <csrc>/insite_regimen.hip -x c++ tools/regimen_args_check.cpp -fsanitize=address,undefined
// (<csrc>: the package's csrc directory).  Besides the header's list it sweeps the stride and leading-dimension
// arithmetic at extreme values (near 2^31, 2^62 and 2^63) with n_rows = 0, so that nothing launches, and with rows and
// one NULL pointer, so that the call gets through every stride check and still returns before the launch: no signed
// overflow may happen on the way to either answer.  Exit status 0 and "0 failure(s)" when every status is the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "insite_regimen.h"
static int fails = 0;
#define EXPECT(e, want) do { long long got_ = (long long)(e); if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #e, got_, (long long)(want)); ++fails; } } while (0)
int main() {
  std::vector<double> x(4096, 0.0);
  std::vector<int8_t> arm(4096, 0);
  std::vector<int32_t> ch(64, 0);
  int8_t exps[7 * 3] = {0,0,0, 1,0,0, 0,1,0, 0,0,1, 1,1,0, 1,0,1, 0,1,1};
  double q[16] = {0.025, 0.5, 0.975, 0, 1, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8, 0.9, 0.25, 0.75, 0.5};
  double* d = x.data();
  // N = 5, T = 12, K = 3, Q = 3: ld_plan 12, plan_stride 60, ld_w 12, ld_out 36
  auto call = [&](int64_t N, int T, int K, int64_t ps, int64_t ldp, int64_t ldw, int64_t ldo, int sense = 1, int R = 9,
                  int Q = 3, int A = 2, int F = 7, int m = 0, const double* y0 = nullptr) {
    return insite_regimen_choice_f64(y0 ? y0 : d, d, arm.data(), K, ps, ldp, d, ldw, d, sense, d, exps, F, N, T, 2, A, 0.1,
                                     m, 5, 1e-3, R, q, Q, ch.data(), d, d, ldo, nullptr, 0, nullptr);
  };
  EXPECT(insite_regimen_abi_version(), 1);
  EXPECT(insite_regimen_workspace_bytes(1000000, 60, 2, 7, 256, 3, 8), 0);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36), INSITE_OK);
  EXPECT(call(-1, 12, 3, 60, 12, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 0, 3, 60, 12, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 0, 60, 12, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, -1, 60, 12, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 17, 60, 12, 12, 17 * 2 * 6), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 16, 60, 12, 12, 16 * 2 * 6), INSITE_OK);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 0), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 2), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, -1), INSITE_OK);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 1), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 513), INSITE_E_UNSUPPORTED);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 512), INSITE_OK);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 9, 0), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 3 * 2 * 20, 1, 9, 17), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 3 * 2 * 19, 1, 9, 16), INSITE_OK);
  EXPECT(call(0, 12, 3, 60, 12, 12, 3 * 2 * 19 - 1, 1, 9, 16), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 9, 3, 5), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 9, 3, 2, 10), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 60, 12, 12, 36, 1, 9, 3, 2, 7, 2), INSITE_E_UNSUPPORTED);
  for (int ld = 1; ld < 12; ++ld) {
    EXPECT(call(0, 12, 3, 60, ld, 12, 36), INSITE_E_INVALID_ARG);
    EXPECT(call(0, 12, 3, 60, 12, ld, 36), INSITE_E_INVALID_ARG);
  }
  EXPECT(call(0, 12, 3, 11, 0, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(0, 12, 3, 12, 0, 0, 36), INSITE_OK);
  EXPECT(call(5, 12, 3, 59, 12, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(5, 12, 3, 64, 13, 12, 36), INSITE_E_INVALID_ARG);
  EXPECT(call(5, 12, 3, 60, 12, 12, 35), INSITE_E_INVALID_ARG);
  double qbad[3] = {0.5, 1.5, 0.1};
  EXPECT(insite_regimen_choice_f64(d, d, arm.data(), 3, 60, 12, d, 12, d, 1, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, qbad, 3,
                                   ch.data(), d, d, 36, nullptr, 0, nullptr), INSITE_E_INVALID_ARG);
  EXPECT(insite_regimen_choice_f64(d, d, arm.data(), 3, 60, 12, d, 12, d, 1, d, exps, 7, 5, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, q, 3,
                                   nullptr, d, d, 36, nullptr, 0, nullptr), INSITE_E_INVALID_ARG);
  // the sweep: every combination answers INSITE_OK or INSITE_E_INVALID_ARG and nothing overflows on the way.  With
  // n_rows = 0 nothing can launch; with rows a NULL `choice` stops the call after the stride checks.
  const int64_t big[] = {0, 1, 11, 12, 13, 60, (int64_t)1 << 31, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) + 1,
                         (int64_t)1 << 62, ((int64_t)1 << 62) - 1, ((int64_t)1 << 62) + 1, INT64_MAX, INT64_MAX - 1,
                         INT64_MAX / 2, INT64_MAX / 3, -1, INT64_MIN};
  const int64_t rows[] = {0, 1, 5, (int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX};
  const int Ks[] = {1, 2, 3, 16};
  const int Ts[] = {1, 12, 2147483647};
  long long n_ok = 0, n_bad = 0, n_other = 0;
  for (int64_t N : rows) for (int K : Ks) for (int T : Ts) for (int64_t ps : big) for (int64_t ldp : big)
    for (int64_t ldx : big) {
      // ldx plays ld_w and ld_out in turn (the other stays valid), so the sweep stays cubic
      for (int which = 0; which < 2; ++which) {
        const int64_t ldw = which == 0 ? ldx : 0;
        const int64_t ldo = which == 1 ? ldx : (int64_t)K * 2 * 6;
        const int32_t st = insite_regimen_choice_f64(d, d, arm.data(), K, ps, ldp, d, ldw, d, 1, d, exps, 7, N, T, 2, 2, 0.1,
                                                     0, 5, 1e-3, 9, q, 3, nullptr, d, d, ldo, nullptr, 0, nullptr);
        // an accepted shape with rows is refused for the NULL choice; with n_rows = 0 it is the no-op
        if (st == INSITE_OK) { ++n_ok; if (N != 0) { std::printf("FAIL launch path reached at N=%lld\n", (long long)N); ++fails; } }
        else if (st == INSITE_E_INVALID_ARG) ++n_bad;
        else ++n_other;
        // the documented bounds, restated: whatever the sweep accepts with n_rows = 0 obeys them
        if (st == INSITE_OK && (ps < T || (ldp != 0 && ldp < T) || (ldw != 0 && ldw < T) || ldo < (int64_t)K * 2 * 6 ||
                                ldp < 0 || ldw < 0)) {
          std::printf("FAIL accepted ps=%lld ldp=%lld ldw=%lld ldo=%lld T=%d K=%d\n", (long long)ps, (long long)ldp,
                      (long long)ldw, (long long)ldo, T, K);
          ++fails;
        }
      }
    }
  EXPECT(n_other, 0);
  // the accepted side at the extremes: one shared plan vector at the largest stride that keeps K = 2 inside int64
  EXPECT(call(0, 12, 2, (int64_t)1 << 62, 0, 0, 24), INSITE_OK);
  EXPECT(call(0, 12, 2, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62), INSITE_OK);
  EXPECT(call(0, 12, 3, (int64_t)1 << 62, 0, 0, 36), INSITE_E_INVALID_ARG);   // 2 plan_stride leaves int64
  EXPECT(call(5, 12, 2, (int64_t)1 << 62, (int64_t)1 << 61, 12, 24), INSITE_E_INVALID_ARG);   // 5 ld_plan > plan_stride
  std::printf("sweep: %lld accepted (n_rows = 0), %lld refused; %d failure(s)\n", n_ok, n_bad, fails);
  return fails ? 1 : 0;
}
