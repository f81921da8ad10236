// Stand-alone host check of insite_cohort.h's argument validation and workspace query: every call here returns
// before any HIP call, so it needs no device.  Meant for a sanitizer build of the host code, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I<csrc> \
//         -o cohort_args_check <csrc>/insite_cohort.hip -x c++ tools/cohort_args_check.cpp -fsanitize=address,undefined
// (<csrc>: the package's csrc directory).  Exit status 0 and "0 failure(s)" when every status is the header's.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "insite_cohort.h"
static int fails = 0;
#define EXPECT(e, want) do { long long got_ = (long long)(e); if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #e, got_, (long long)(want)); ++fails; } } while (0)
int main() {
  std::vector<double> x(4096, 0.0);
  std::vector<int8_t> arm(4096, 0);
  std::vector<int32_t> grp(64, 0);
  int8_t exps[7 * 3] = {0,0,0, 1,0,0, 0,1,0, 0,0,1, 1,1,0, 1,0,1, 0,1,1};
  double q[3] = {0.025, 0.5, 0.975};
  double* d = x.data();
  auto sums = [&](int64_t N, int T, int A, int R, int G, int wt, int64_t off, void* ws, size_t wsn, int F = 7, int m = 0) {
    return insite_cohort_effect_sums_f64(d, d, arm.data(), 12, arm.data(), 12, d, exps, F, N, T, 2, A, 0.1, m, 5, 1e-3, R,
                                         grp.data(), G, wt, 7u, off, d, 12, d, ws, wsn, nullptr);
  };
  EXPECT(insite_cohort_abi_version(), 1);
  EXPECT(sums(5, 12, 2, 9, 3, 1, 0, nullptr, 0), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 3, 1, 0, d, 8), INSITE_E_INVALID_ARG);
  EXPECT(sums(-1, 12, 2, 9, 3, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 0, 2, 9, 3, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 5, 9, 3, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 1, 3, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 4097, 3, 1, 0, d, 1 << 20), INSITE_E_UNSUPPORTED);
  EXPECT(sums(5, 12, 2, 9, 65, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 0, 1, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 3, 2, 0, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 3, 1, -1, d, 1 << 20), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 3, 1, 0, d, 1 << 20, 10), INSITE_E_INVALID_ARG);
  EXPECT(sums(5, 12, 2, 9, 3, 1, 0, d, 1 << 20, 7, 2), INSITE_E_UNSUPPORTED);
  EXPECT(sums(0, 12, 2, 4096, 64, 0, 0, nullptr, 0), INSITE_OK);
  EXPECT(insite_cohort_effect_finalize_f64(d, 12, d, 9, 3, 2, 12, q, 3, nullptr, 12, nullptr), INSITE_E_INVALID_ARG);
  EXPECT(insite_cohort_effect_finalize_f64(d, 12, d, 4097, 3, 2, 12, q, 3, d, 12, nullptr), INSITE_E_UNSUPPORTED);
  EXPECT(insite_cohort_effect_finalize_f64(d, 12, d, 9, 3, 3, 12, q, 3, d, 12, nullptr), INSITE_E_INVALID_ARG);
  double qbad[3] = {0.5, 1.5, 0.1};
  EXPECT(insite_cohort_effect_finalize_f64(d, 12, d, 9, 3, 2, 12, qbad, 3, d, 12, nullptr), INSITE_E_INVALID_ARG);
  EXPECT(insite_cohort_effect_f64(d, d, arm.data(), 12, arm.data(), 12, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, grp.data(),
                                  3, 1, 7u, 0, d, 12, d, q, 3, nullptr, 12, nullptr, 0, nullptr), INSITE_E_INVALID_ARG);
  EXPECT(insite_cohort_effect_f64(d, d, arm.data(), 12, arm.data(), 12, d, exps, 7, 0, 12, 2, 2, 0.1, 0, 5, 1e-3, 9, grp.data(),
                                  3, 1, 7u, 0, d, 12, d, q, 3, d, 12, nullptr, 0, nullptr), INSITE_OK);
  // the workspace query over a sweep of shapes: below 1 GiB or 0, never overflowing
  const int64_t Ns[] = {1, 63, 64, 65, 5000, 1000000, 100000000, (int64_t)1 << 40};
  const int Ts[] = {1, 16, 17, 60, 64, 65, 255, 100000, 2147483647};
  const int Rs[] = {2, 64, 65, 256, 4096};
  const int Gs[] = {1, 8, 64};
  size_t worst = 0;
  for (int64_t N : Ns) for (int T : Ts) for (int R : Rs) for (int G : Gs) {
    const size_t b = insite_cohort_effect_workspace_bytes(N, T, 4, 9, R, G);
    if (b >= ((size_t)1 << 30)) { std::printf("FAIL workspace %zu at N=%lld T=%d R=%d G=%d\n", b, (long long)N, T, R, G); ++fails; }
    if (b > worst) worst = b;
  }
  EXPECT(insite_cohort_effect_workspace_bytes(1000000, 60, 4, 9, 4096, 64) > 0, 1);
  EXPECT(insite_cohort_effect_workspace_bytes(10, 60, 2, 7, 4097, 1), 0);
  std::printf("largest workspace %zu bytes; %d failure(s)\n", worst, fails);
  return fails ? 1 : 0;
}
