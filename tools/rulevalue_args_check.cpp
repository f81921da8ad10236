// Stand-alone host check of insite_rulevalue.h's argument validation and workspace query: every call here returns
// before any HIP call, so it needs no device.  Meant for a sanitizer build of the host code, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I<csrc> \
//         -o rulevalue_args_check <csrc>/insite_rulevalue.hip -x c++ tools/rulevalue_args_check.cpp \
//         -fsanitize=address,undefined
// (<csrc>: the package's csrc directory).  Besides the header's lists it puts every field of the first and of the last
// rule at and past its bounds with the rule table allocated exactly (a read past 4 n_rules ints is the sanitizer's to
// find), and sweeps ld_theta, ld_w, ld_out, patient_offset and n_rows at extreme values (near 2^31, 2^62 and 2^63):
// with n_rows = 0 nothing can launch; with rows a NULL `sums` (a NULL `out` for the finalize call) stops the call
// after every stride check and before the launch.  No signed overflow may happen on the way to either answer.  Exit
// status 0 and "0 failure(s)" when every status is the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "insite_rulevalue.h"
static int fails = 0;
static long long calls = 0;
#define EXPECT(e, want) do { long long got_ = (long long)(e); ++calls; if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #e, got_, (long long)(want)); ++fails; } } while (0)

struct Args {
  int64_t N = 0, ldt = 6, ldw = 12, off = 0, ldo = 6;
  int T = 12, K = 3, sense = 1, R = 9, G = 2, Q = 3, A = 2, F = 7, m = 0, U = 2, sub = 5, wt = 1;
  double dt = 0.1;
  bool null_sums = false, null_out = false, null_ws = false, null_q = false, null_rules = false, null_ac = false;
  size_t wsb = (size_t)1 << 20;
  const int32_t* rules = nullptr;  // nullptr: the default table of K valid rules
};

int main() {
  std::vector<double> x(8192, 0.0);
  std::vector<int32_t> iv(4096, 0);
  int8_t exps[7 * 3] = {0,0,0, 1,0,0, 0,1,0, 0,0,1, 1,1,0, 1,0,1, 0,1,1};
  double q[17] = {0.025, 0.5, 0.975, 0, 1, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8, 0.9, 0.25, 0.75, 0.5, 0.5};
  double ac[4] = {0.0, 0.01, -0.01, 0.02};
  double* d = x.data();
  // a rule table of exactly 4 K ints, on the heap so that a read past it is caught
  auto table = [](int K) {
    std::vector<int32_t> t((size_t)(K > 0 ? K : 0) * 4);
    for (int j = 0; j < K; ++j) { t[4 * j] = j & 1; t[4 * j + 1] = (j + 1) & 1; t[4 * j + 2] = 1 + j % 5; t[4 * j + 3] = j & 1; }
    return t;
  };
  // N = 5, T = 12, K = 3, G = 2, Q = 3: ld_theta 6, ld_w 12, ld_out 6
  auto sums = [&](const Args& a) {
    std::vector<int32_t> t = table(a.K);
    const int32_t* rl = a.null_rules ? nullptr : (a.rules ? a.rules : t.data());
    return insite_rulevalue_sums_f64(d, d, d, a.ldt, rl, a.K, d, a.ldw, d, a.null_ac ? nullptr : ac, a.sense, d, exps,
                                     a.F, a.N, a.T, a.U, a.A, a.dt, a.m, a.sub, 1e-3, a.R, iv.data(), a.G, a.wt, 3u,
                                     a.off, iv.data(), iv.data(), a.null_ws ? nullptr : d, a.wsb,
                                     a.null_sums ? nullptr : d, d, nullptr);
  };
  auto value = [&](const Args& a) {
    std::vector<int32_t> t = table(a.K);
    const int32_t* rl = a.null_rules ? nullptr : (a.rules ? a.rules : t.data());
    return insite_rulevalue_f64(d, d, d, a.ldt, rl, a.K, d, a.ldw, d, a.null_ac ? nullptr : ac, a.sense, d, exps, a.F,
                                a.N, a.T, a.U, a.A, a.dt, a.m, a.sub, 1e-3, a.R, iv.data(), a.G, a.wt, 3u, a.off,
                                iv.data(), iv.data(), a.null_ws ? nullptr : d, a.wsb, a.null_sums ? nullptr : d, d,
                                a.null_q ? nullptr : q, a.Q, a.null_out ? nullptr : d, a.ldo, d, iv.data(), nullptr);
  };
  auto fin = [&](const Args& a) {
    return insite_rulevalue_finalize_f64(a.null_sums ? nullptr : d, d, a.R, a.G, a.K, a.sense, a.null_q ? nullptr : q,
                                         a.Q, a.null_out ? nullptr : d, a.ldo, d, iv.data(), nullptr);
  };
#define WITH(field, v, call, want) do { Args a_; a_.field = v; EXPECT(call(a_), want); } while (0)
  EXPECT(insite_rulevalue_abi_version(), 1);
  // the workspace query
  EXPECT(insite_rulevalue_workspace_bytes(1000, 60, 2, 7, 256, 8, 8), 4000 + 16 * (8 * 4 * 29 * 64 * 8));
  EXPECT(insite_rulevalue_workspace_bytes(1, 1, 1, 1, 2, 1, 1), 8 + 8 * 64 * 8);
  EXPECT(insite_rulevalue_workspace_bytes(0, 60, 2, 7, 256, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(-1, 60, 2, 7, 256, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 0, 2, 7, 256, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 5, 7, 256, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 10, 256, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 7, 1, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 7, 4097, 8, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 7, 256, 65, 8), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 7, 256, 8, 17), 0);
  EXPECT(insite_rulevalue_workspace_bytes(10, 60, 2, 7, 256, 8, 0), 0);
  for (int64_t n : {(int64_t)1 << 31, (int64_t)1 << 40, (int64_t)1 << 61, ((int64_t)1 << 61) - 2,
                    ((int64_t)1 << 61) - 64, (int64_t)1 << 62, INT64_MAX, INT64_MAX / 4, INT64_MAX / 4 + 1}) {
    const size_t b = insite_rulevalue_workspace_bytes(n, 60, 2, 7, 4096, 64, 16);
    ++calls;
    // either refused or the assignment plus partials below 1 GiB
    if (b != 0 && (b < (size_t)n * 4 || b - (size_t)((n * 4 + 7) / 8 * 8) >= ((size_t)1 << 30))) {
      std::printf("FAIL workspace_bytes(%lld) = %zu\n", (long long)n, b);
      ++fails;
    }
  }
  // the three calls: the accepted no-op and every refusal of the header's lists
  { Args a; EXPECT(sums(a), INSITE_OK); EXPECT(value(a), INSITE_OK); }
  for (int which = 0; which < 2; ++which) {
    auto call = [&](const Args& a) { return which ? value(a) : sums(a); };
    WITH(N, -1, call, INSITE_E_INVALID_ARG);
    WITH(T, 0, call, INSITE_E_INVALID_ARG);
    WITH(K, 0, call, INSITE_E_INVALID_ARG);
    WITH(K, -1, call, INSITE_E_INVALID_ARG);
    WITH(K, 17, call, INSITE_E_INVALID_ARG);        // ld_theta 6 < 2 K: an invalid argument goes before the cap
    { Args a; a.K = 17; a.ldt = 34; EXPECT(call(a), INSITE_E_UNSUPPORTED); }
    { Args a; a.K = 16; a.ldt = 32; EXPECT(call(a), INSITE_OK); }
    { Args a; a.K = 1; a.ldt = 2; EXPECT(call(a), INSITE_OK); }
    WITH(null_rules, true, call, INSITE_E_INVALID_ARG);
    WITH(null_ac, true, call, INSITE_OK);
    WITH(sense, 0, call, INSITE_E_INVALID_ARG);
    WITH(sense, 2, call, INSITE_E_INVALID_ARG);
    WITH(sense, -1, call, INSITE_OK);
    WITH(R, 1, call, INSITE_E_INVALID_ARG);
    WITH(R, 4097, call, INSITE_E_UNSUPPORTED);
    WITH(R, 4096, call, INSITE_OK);
    WITH(G, 0, call, INSITE_E_INVALID_ARG);
    WITH(G, 65, call, INSITE_E_UNSUPPORTED);
    WITH(G, 64, call, INSITE_OK);
    WITH(A, 0, call, INSITE_E_INVALID_ARG);
    WITH(A, 5, call, INSITE_E_INVALID_ARG);
    WITH(A, 1, call, INSITE_E_INVALID_ARG);          // the default table uses arm 1
    WITH(F, 0, call, INSITE_E_INVALID_ARG);
    WITH(F, 10, call, INSITE_E_INVALID_ARG);
    WITH(U, 4, call, INSITE_E_INVALID_ARG);
    WITH(m, 2, call, INSITE_E_UNSUPPORTED);
    WITH(sub, 0, call, INSITE_E_INVALID_ARG);
    WITH(dt, -1.0, call, INSITE_E_INVALID_ARG);
    WITH(wt, 2, call, INSITE_E_INVALID_ARG);
    WITH(wt, 0, call, INSITE_OK);
    WITH(off, -1, call, INSITE_E_INVALID_ARG);
    WITH(off, INT64_MAX, call, INSITE_OK);   // n_rows = 0
    for (int ld = 1; ld < 6; ++ld) WITH(ldt, ld, call, INSITE_E_INVALID_ARG);
    for (int ld = 1; ld < 12; ++ld) WITH(ldw, ld, call, INSITE_E_INVALID_ARG);
    { Args a; a.ldt = 0; a.ldw = 0; EXPECT(call(a), INSITE_OK); }
    // every field of the first and of the last rule, at and past its bounds, the table allocated exactly
    for (int K : {1, 3, 16})
      for (int j : {0, K - 1})
        for (int col = 0; col < 4; ++col) {
          const int32_t lo = col == 2 ? 1 : 0, hi = col == 2 ? INT32_MAX : 1;
          const int32_t vals[] = {lo, hi, lo - 1, (int32_t)(col == 2 ? INT32_MIN : hi + 1), -1, INT32_MIN,
                                  (int32_t)(col == 2 ? 0 : INT32_MAX), 256, 1 << 16};
          for (int32_t v : vals) {
            std::vector<int32_t> t = table(K);
            t[4 * j + col] = v;
            Args a;
            a.K = K; a.ldt = 2 * K; a.rules = t.data();
            const bool ok = v >= lo && v <= hi;
            EXPECT(call(a), ok ? INSITE_OK : INSITE_E_INVALID_ARG);
            a.N = 5; a.null_sums = true;             // with rows: refused either way, for the rule or for the NULL
            EXPECT(call(a), INSITE_E_INVALID_ARG);
          }
        }
    { Args a; a.N = 5; a.off = INT64_MAX - 3; a.null_sums = true; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    { Args a; a.N = 5; a.null_sums = true; EXPECT(call(a), INSITE_E_INVALID_ARG); }   // the NULL sums alone
    { Args a; a.N = 5; a.null_ws = true; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    { Args a; a.N = 5; a.wsb = 100; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    { Args a; a.N = 5; a.wsb = insite_rulevalue_workspace_bytes(5, 12, 2, 7, 9, 2, 3) - 1; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    { Args a; a.K = 17; a.ldt = 34; a.sense = 0; EXPECT(call(a), INSITE_E_INVALID_ARG); }   // invalid goes before a cap
  }
  for (int which = 0; which < 2; ++which) {
    // the finalize call (rows or not: it has none) and the finalize half of the combined call with n_rows = 0
    auto call = [&](const Args& a) { return which ? value(a) : fin(a); };
    WITH(null_out, true, call, INSITE_E_INVALID_ARG);
    WITH(null_q, true, call, INSITE_E_INVALID_ARG);
    WITH(Q, 0, call, INSITE_E_INVALID_ARG);
    WITH(ldo, 5, call, INSITE_E_INVALID_ARG);
    WITH(ldo, -6, call, INSITE_E_INVALID_ARG);
    WITH(R, 1, call, INSITE_E_INVALID_ARG);
    WITH(G, 0, call, INSITE_E_INVALID_ARG);
    WITH(K, 0, call, INSITE_E_INVALID_ARG);
    WITH(sense, 3, call, INSITE_E_INVALID_ARG);
    { Args a; a.Q = 17; a.ldo = 20; a.null_out = !which; EXPECT(call(a), which ? INSITE_E_UNSUPPORTED : INSITE_E_INVALID_ARG); }
    { Args a; a.Q = 17; a.ldo = 19; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    { Args a; a.Q = 16; a.ldo = 18; EXPECT(call(a), INSITE_E_INVALID_ARG); }
    if (which) { Args a; a.Q = 16; a.ldo = 19; EXPECT(call(a), INSITE_OK); }
  }
  { Args a; a.null_sums = true; EXPECT(fin(a), INSITE_E_INVALID_ARG); }
  // the caps of the finalize call proper: every pointer valid, so only a cap can stop it (a valid call would launch)
  { Args a; a.R = 4097; EXPECT(fin(a), INSITE_E_UNSUPPORTED); }
  { Args a; a.G = 65; EXPECT(fin(a), INSITE_E_UNSUPPORTED); }
  { Args a; a.K = 17; EXPECT(fin(a), INSITE_E_UNSUPPORTED); }
  { Args a; a.Q = 17; a.ldo = 20; EXPECT(fin(a), INSITE_E_UNSUPPORTED); }
  double qbad[3] = {0.5, 1.5, 0.1};
  EXPECT(insite_rulevalue_finalize_f64(d, d, 9, 2, 3, 1, qbad, 3, d, 6, d, iv.data(), nullptr), INSITE_E_INVALID_ARG);

  // the sweep: every combination answers INSITE_OK or INSITE_E_INVALID_ARG and nothing overflows on the way
  const int64_t big[] = {0, 1, 5, 6, 7, 11, 12, 13, 32, (int64_t)1 << 31, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) + 1,
                         (int64_t)1 << 62, ((int64_t)1 << 62) - 1, ((int64_t)1 << 62) + 1, INT64_MAX, INT64_MAX - 1,
                         INT64_MAX / 2, INT64_MAX / 3, -1, INT64_MIN};
  const int64_t rows[] = {0, 1, 5, (int64_t)1 << 31, (int64_t)1 << 40, (int64_t)1 << 62, INT64_MAX};
  const int Ks[] = {1, 3, 16};
  const int Ts[] = {1, 12, 2147483647};
  long long n_ok = 0, n_bad = 0, n_other = 0;
  for (int64_t N : rows) for (int K : Ks) for (int T : Ts) for (int64_t ldt : big) for (int64_t ldw : big)
    for (int64_t off : big) {
      Args a;
      a.N = N; a.K = K; a.T = T; a.ldt = ldt; a.ldw = ldw; a.off = off;
      a.null_sums = true;   // with rows: the call gets through every stride check and stops here
      const int32_t st = sums(a);
      ++calls;
      if (st == INSITE_OK) { ++n_ok; if (N != 0) { std::printf("FAIL launch path reached at N=%lld\n", (long long)N); ++fails; } }
      else if (st == INSITE_E_INVALID_ARG) ++n_bad;
      else ++n_other;
      if (st == INSITE_OK && ((ldt != 0 && ldt < 2 * K) || (ldw != 0 && ldw < T) || ldt < 0 || ldw < 0 || off < 0)) {
        std::printf("FAIL accepted ldt=%lld ldw=%lld off=%lld T=%d K=%d\n", (long long)ldt, (long long)ldw,
                    (long long)off, T, K);
        ++fails;
      }
    }
  EXPECT(n_other, 0);
  // ld_out of the finalize call and of the combined call, every (G, K, Q) corner
  long long f_bad = 0, f_ok = 0;
  for (int64_t ldo : big) for (int G : {1, 2, 64}) for (int K : {1, 3, 16}) for (int Q : {1, 3, 16}) {
    Args a;
    a.ldo = ldo; a.G = G; a.K = K; a.ldt = 2 * K; a.Q = Q; a.null_out = true;
    EXPECT(fin(a), INSITE_E_INVALID_ARG);          // the NULL out, whatever ld_out
    a.null_out = false;
    const int32_t st = value(a);                   // n_rows = 0: nothing launches
    ++calls;
    if (st == INSITE_OK) {
      ++f_ok;
      if (ldo < 3 + Q) { std::printf("FAIL accepted ld_out=%lld Q=%d\n", (long long)ldo, Q); ++fails; }
    } else if (st == INSITE_E_INVALID_ARG) ++f_bad;
    else { std::printf("FAIL value(ld_out=%lld) = %d\n", (long long)ldo, st); ++fails; }
  }
  // the accepted side at the extremes
  { Args a; a.ldt = a.ldw = (int64_t)1 << 62; EXPECT(sums(a), INSITE_OK); }
  { Args a; a.ldt = a.ldw = INT64_MAX; a.off = INT64_MAX; EXPECT(sums(a), INSITE_OK); }     // n_rows = 0: last row 0
  { Args a; a.N = 2; a.ldt = INT64_MAX; a.null_sums = true; EXPECT(sums(a), INSITE_E_INVALID_ARG); }   // 6 + ld_theta leaves int64
  { Args a; a.G = 1; a.K = 1; a.ldt = 2; a.ldo = INT64_MAX / 12; EXPECT(value(a), INSITE_OK); }        // 11 ld_out + 6 fits
  { Args a; a.G = 1; a.K = 1; a.ldt = 2; a.ldo = INT64_MAX / 11 + 1; EXPECT(value(a), INSITE_E_INVALID_ARG); }
  std::printf("%lld calls; sweep: %lld accepted (n_rows = 0), %lld refused; ld_out: %lld accepted, %lld refused; "
              "%d failure(s)\n", calls, n_ok, n_bad, f_ok, f_bad, fails);
  return fails ? 1 : 0;
}
