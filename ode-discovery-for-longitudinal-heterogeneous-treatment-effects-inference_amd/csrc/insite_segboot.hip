// insite_segboot.hip — patient-level Poisson bootstrap of the treatment-segment discovery on MI355X (gfx950):
// include/insite_segboot.h, DESIGN.md §9o.
//
// Kernels:
//   seg_moments_kernel    lane = patient, one pass over the lane's samples: the per-(patient, arm) five moments of
//                         the segment cut of gram_seg_kernel (insite_hip.hip), written instead of contracted.  A
//                         wave's [64, n_arms 5] rows are contiguous in mom_out and go out through LDS.
//   segboot_gram_kernel   boot_gram_kernel's GEMM (insite_boot.hip: M = 16 replicates, K = 4 patients, N = 16 entry
//                         columns on v_mfma_f64_16x16x4f64, the Poisson weights made in registers) with another B
//                         operand: a patient's entry of EVERY arm it has rows in, under the one weight of the patient.
//   boot_finalize_kernel  (insite_bootplan.h) the waves' partials -> G | b in a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "insite_segboot.h"
#include "insite_affine.h"
#include "insite_bootplan.h"

namespace {

// ---------------------------------------------------------------------------------------------
// seg_moments_kernel
// ---------------------------------------------------------------------------------------------
// The streaming form of gram_seg_kernel, per lane and step j < L (own segment, arm a_j): library input x_j,
// derivative d_j = (xs_{j+1} - xs_j) / dt; if sample j + 1 ends that segment (j + 1 = L or a_{j+1} != a_j) it is
// added to the same arm as the segment's last sample: input x_{j+1}, derivative d_j.  So per step the lane adds
// (n, sx, sxx, n d, d sx), n = 1 + end, to arm a_j: one select per arm.  Smoothed: inside a segment xs_i =
// (x_i + x_{i+1}) / 2 except at its first and last sample (raw); the derivative uses xs, the library the raw samples.
// Here a wave takes one 64-patient tile over the WHOLE trajectory (no pieces: a lane's moments are complete when its
// loop ends, so there are no atomics and the order of every sum is the order of the steps).  Loads as there: chunks of
// kSmKC steps through buffer descriptors based at the wave's first patient (wave-uniform base, 32-bit per-lane
// offsets; time-major: consecutive lanes read consecutive addresses, patient-major: a stride of ldx), every load
// issued unconditionally, the next chunk in flight while the current one is consumed; lanes past N and steps past
// the stored range read through offsets the hardware drops, and samples past the lane's own L (they may be NaN) are
// masked after the load.
constexpr int kSmKC = 4;  // steps per register chunk

template <int NARM, bool SMOOTH1>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4)))
seg_moments_kernel(const double* __restrict__ x, int64_t xsp, int64_t xsk, const int8_t* __restrict__ arm, int64_t asp,
                   int64_t ask, const int32_t* __restrict__ seq_len, int n_steps, int64_t N, int n_arms, double inv_dt,
                   double* __restrict__ mom_out) {
  __shared__ double smem[kWavesPerBlock * kWave * 5 * NARM];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  double* ps = smem + wid * (kWave * 5 * NARM);
  const int n5 = 5 * n_arms;  // <= 5 NARM

  const int64_t n_tiles = (N + kWave - 1) / kWave;
  const int64_t nW = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wid; tile < n_tiles; tile += nW) {
    const int64_t p0 = tile * kWave;
    const int64_t p = p0 + lane;
    const bool valid = p < N;
    int L = valid ? seq_len[p] : 0;
    if (L > n_steps - 1) L = n_steps - 1;
    if (L < 0) L = 0;
    const int Lw = wave_max_i(L);  // one past the last step the wave processes
    double mo[NARM][5];
#pragma unroll
    for (int a = 0; a < NARM; ++a)
#pragma unroll
      for (int j = 0; j < 5; ++j) mo[a][j] = 0.0;
    const int nvalid = (int)(N - p0 < kWave ? N - p0 : kWave);
    const unsigned xvo = valid ? (unsigned)((int64_t)lane * xsp * 8) : kOOB;
    const unsigned avo = valid ? (unsigned)((int64_t)lane * asp) : kOOB;
    auto x_rsrc = [&](int kb) {  // samples kb .. kb + KC of the wave's patients
      int rows = n_steps - kb;
      if (rows > kSmKC + 1) rows = kSmKC + 1;
      const int bytes = rows > 0 ? (int)(((int64_t)(nvalid - 1) * xsp + (int64_t)(rows - 1) * xsk + 1) * 8) : 0;
      return __builtin_amdgcn_make_buffer_rsrc((void*)(x + p0 * xsp + (int64_t)(rows > 0 ? kb : 0) * xsk), (short)0,
                                               bytes, 0x00020000);
    };
    auto a_rsrc = [&](int kb) {  // arms kb .. kb + KC - 1 (stored steps < n_steps - 1)
      int rows = n_steps - 1 - kb;
      if (rows > kSmKC) rows = kSmKC;
      const int bytes = rows > 0 ? (int)((int64_t)(nvalid - 1) * asp + (int64_t)(rows - 1) * ask + 1) : 0;
      return __builtin_amdgcn_make_buffer_rsrc((void*)(arm + p0 * asp + (int64_t)(rows > 0 ? kb : 0) * ask), (short)0,
                                               bytes, 0x00020000);
    };
    const unsigned xstep = (unsigned)(xsk * 8), astep = (unsigned)ask;
    if (0 < Lw) {
      double xj;
      int aj;
      int aprev = -1;  // arm of sample j - 1 (SMOOTH1: segment-start test)
      {
        const __amdgpu_buffer_rsrc_t rx = x_rsrc(0), ra = a_rsrc(0);
        xj = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rx, xvo, 0, 0));  // sample 0 <= L
        const int a0 = (int)(int8_t)__builtin_amdgcn_raw_buffer_load_b8(ra, avo, 0, 0);
        aj = 0 < L ? a0 : -1;
      }
      constexpr int NX = kSmKC + (SMOOTH1 ? 1 : 0);
      // raw chunk registers; the masks (k <= L, k < L) are applied at the use, so a prefetched chunk is not waited
      // for when it is issued
      auto load = [&](double (&xr)[NX], int (&ar)[kSmKC], int k0) {
        const __amdgpu_buffer_rsrc_t rx = x_rsrc(k0 + 1), ra = a_rsrc(k0 + 1);
#pragma unroll
        for (int j = 0; j < NX; ++j)
          xr[j] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rx, xvo + j * xstep, 0, 0));
#pragma unroll
        for (int j = 0; j < kSmKC; ++j)
          ar[j] = (int)(int8_t)__builtin_amdgcn_raw_buffer_load_b8(ra, avo + j * astep, 0, 0);
      };
      auto process = [&](const double (&xr)[NX], const int (&ar)[kSmKC], int k0) {
#pragma unroll
        for (int j = 0; j < kSmKC; ++j) {
          const double x1 = (k0 + 1 + j <= L) ? xr[j] : 0.0;
          const int a1 = (k0 + 1 + j < L) ? ar[j] : -1;
          const bool endf = a1 != aj;  // sample j + 1 closes j's segment (also at j + 1 = L)
          const double xo = xj;        // library input: the raw sample (the smoothing feeds x_dot only)
          double xso, xs1;
          if constexpr (SMOOTH1) {
            const double x2 = (k0 + 2 + j <= L) ? xr[j + 1] : 0.0;
            xso = (aj != aprev) ? xj : 0.5 * (xj + x1);
            xs1 = endf ? x1 : 0.5 * (x1 + x2);
          } else {
            xso = xj;
            xs1 = x1;
          }
          const double d = (xs1 - xso) * inv_dt;
          const double xc = endf ? x1 : 0.0;
          const double n = endf ? 2.0 : 1.0;
          const double sx = xo + xc;
          const double sxx = fma(xo, xo, xc * xc);
          const double sd = d * n;
          const double sdx = d * sx;
#pragma unroll
          for (int a = 0; a < NARM; ++a) {
            const double w = (aj == a) ? 1.0 : 0.0;  // aj = -1 past the lane's own samples
            mo[a][0] = fma(w, n, mo[a][0]);
            mo[a][1] = fma(w, sx, mo[a][1]);
            mo[a][2] = fma(w, sxx, mo[a][2]);
            mo[a][3] = fma(w, sd, mo[a][3]);
            mo[a][4] = fma(w, sdx, mo[a][4]);
          }
          aprev = aj;
          aj = a1;
          xj = x1;
        }
      };
      double xA[NX], xB[NX];
      int aA[kSmKC], aB[kSmKC];
      // two chunks in flight: chunk c + 1 is requested before chunk c is consumed (buffers alternate)
      load(xA, aA, 0);
      for (int k0 = 0; k0 < Lw;) {
        if (k0 + kSmKC < Lw) load(xB, aB, k0 + kSmKC);
        process(xA, aA, k0);
        k0 += kSmKC;
        if (k0 >= Lw) break;
        if (k0 + kSmKC < Lw) load(xA, aA, k0 + kSmKC);
        process(xB, aB, k0);
        k0 += kSmKC;
      }
    }
    // the wave's rows [nvalid, n_arms 5] are one contiguous run of mom_out: lane-major into LDS, out in address order
    wave_lds_sync();
#pragma unroll
    for (int a = 0; a < NARM; ++a)
      if (a < n_arms) {
#pragma unroll
        for (int j = 0; j < 5; ++j) ps[lane * n5 + 5 * a + j] = mo[a][j];
      }
    wave_lds_sync();
    double* out = mom_out + p0 * n5;
    const int tot = nvalid * n5;
    for (int i = lane; i < tot; i += kWave) out[i] = ps[i];
  }
}

// ---------------------------------------------------------------------------------------------
// segboot_gram_kernel
// ---------------------------------------------------------------------------------------------
// boot_gram_kernel's structure (insite_boot.hip), unchanged: block = one wave; blockIdx.x a contiguous run of
// 8-patient groups aligned in the GLOBAL patient index, blockIdx.y a group of RT replicate tiles, blockIdx.z a chunk
// of CT 16-column tiles of the n_arms nE entry columns (column c = a nE + e: entry e of arm a); the lane (replicate
// lane & 15, kq = lane >> 4) hashes the Threefry pair (base >> 1) + kq once per replicate tile and gets the weights
// of slots 2 kq and 2 kq + 1; accumulators in registers over the wave's whole run, then the wave's partial
// [rpad][cpad].
// The B operand differs.  The LDS row of a patient is {m_0..m_8 | mom[a][0..4], a < n_arms | 1 | visited}: 9 +
// 5 n_arms + 2 <= 31 doubles at the odd stride 31; visited holds bit a iff the slot is inside the shard and
// mom[a][0] > 0 -- the patient has rows in arm a.  Column (a, e) reads m_i m_k mom[a][slot] and keeps it iff bit a is
// set (a select in place of boot_gram_kernel's arm compare), so the one weight of the patient multiplies its entries
// of every arm it visits.  A column past n_arms nE tests a bit no row sets.
constexpr int kSbMom = INSITE_MAX_TERMS;                      // first moment slot of a row
constexpr int kSbPs = kSbMom + 5 * INSITE_MAX_ARMS + 2;       // 31
static_assert(kSbPs % 2 == 1, "odd LDS stride");

template <int RT, int CT>
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2)))
segboot_gram_kernel(const double* __restrict__ mom, const double* __restrict__ u, int64_t N, int64_t off, int n_arms,
                    AffineGramLib lib, uint32_t seed, int R, int ncol, int64_t g0, int64_t nG, int64_t gpw,
                    int64_t rpad, int64_t cpad, double* __restrict__ partial) {
  __shared__ double ps[8 * kSbPs];
  const int lane = threadIdx.x;
  const int col = lane & 15, kq = lane >> 4;
  const int rt0 = blockIdx.y * RT;
  const int ct0 = blockIdx.z * CT;
  const int n5 = 5 * n_arms;
  const int one_slot = kSbMom + n5, vis_slot = one_slot + 1;

  // this lane's entry columns, packed: the LDS slots of m_i | m_k (or the 1) << 8 | the moment << 16 | the arm's bit
  // of visited << 24 (bit 8: no such column)
  int c_desc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int c = (ct0 + t) * 16 + col;
    const bool ok = c < ncol;
    const int a = ok ? c / lib.nE : 0;
    const int e = ok ? c - a * lib.nE : 0;
    const int i = lib.ei[e], k = lib.ek[e];
    const int exi = (lib.ucode[i] >> 24) & 0xff;
    const int exk = k >= 0 ? (lib.ucode[k] >> 24) & 0xff : 0;
    const int ma = kSbMom + 5 * a;
    c_desc[t] = i | (k >= 0 ? k : one_slot) << 8 | (ma + (k >= 0 ? exi + exk : 3 + exi)) << 16 |
                (ok ? a : 8) << 24;
  }
  dbl4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[rt][t] = dbl4{0.0, 0.0, 0.0, 0.0};

  const int s1 = lane >> 3, j1 = lane & 7;  // expansion: slot of this lane, and its row entries j1 + 8 t
  const int64_t gi_lo = (int64_t)blockIdx.x * gpw;
  const int64_t gi_hi = gi_lo + gpw < nG ? gi_lo + gpw : nG;
  for (int64_t gi = gi_lo; gi < gi_hi; ++gi) {
    const int64_t base = g0 + 8 * gi;  // global index of slot 0 (a multiple of 8)
    {
      const int64_t p = base + s1 - off;
      const bool valid = p >= 0 && p < N;
      const int64_t pc = valid ? p : 0;
      double uu[INSITE_MAX_STATICS];
#pragma unroll
      for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? u[pc * lib.U + t] : 0.0;
      double* row = ps + s1 * kSbPs;
      const double* mp = mom + pc * n5;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = j1 + 8 * t;
        if (c < kSbMom) {
          if (c < lib.F) row[c] = monomial_code(lib.ucode[c] & 0xffffff, uu);
        } else if (c < one_slot) {
          const double v = mp[c - kSbMom];
          row[c] = v;
        } else if (c == one_slot) {
          row[c] = 1.0;
        } else if (c == vis_slot) {
          int vis = 0;
#pragma unroll
          for (int a = 0; a < INSITE_MAX_ARMS; ++a)
            if (a < n_arms && valid && mp[5 * a] > 0.0) vis |= 1 << a;
          row[c] = (double)vis;
        }
      }
    }
    wave_lds_sync();
    double bv[2][CT];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double* row = ps + (2 * kq + h) * kSbPs;
      const int vis = (int)row[vis_slot];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int d = c_desc[t];
        const double v = row[d & 0xff] * row[(d >> 8) & 0xff] * row[(d >> 16) & 0xff];
        bv[h][t] = (vis >> (d >> 24)) & 1 ? v : 0.0;
      }
    }
    wave_lds_sync();
    const uint64_t q = (uint64_t)(base >> 1) + (uint64_t)kq;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if ((rt0 + rt) * 16 < R) {  // (uniform)
        const uint32_t r = (uint32_t)((rt0 + rt) * 16 + col);
        uint32_t wa = (uint32_t)q, wb = (uint32_t)(q >> 32);
        threefry2x32_20(seed, r, wa, wb);
        const double w0 = r == 0u ? 1.0 : (double)poisson1_weight(wa);
        const double w1 = r == 0u ? 1.0 : (double)poisson1_weight(wb);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, bv[0][t], acc[rt][t], 0, 0, 0);
          acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1, bv[1][t], acc[rt][t], 0, 0, 0);
        }
      }
    }
  }
  // the wave's partial [rpad][cpad]: rows (rt0 + rt) 16 + kq + 4 j < rpad, columns (ct0 + t) 16 + col < cpad
  double* out = partial + (int64_t)blockIdx.x * rpad * cpad;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out[(int64_t)((rt0 + rt) * 16 + kq + 4 * j) * cpad + (ct0 + t) * 16 + col] = acc[rt][t][j];
}

int32_t run_segboot_gram(const double* mom, const double* u, int64_t patient_offset, int64_t n_patients,
                         int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms, int32_t n_replicates,
                         uint32_t seed, void* workspace, size_t workspace_bytes, double* G_out, double* b_out,
                         void* stream) {
  if (n_patients < 0 || patient_offset < 0 || patient_offset > INT64_MAX - n_patients - 8 || !G_out || !b_out ||
      n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_replicates < 1)
    return INSITE_E_INVALID_ARG;
  if (n_patients > 0 && (!mom || (n_statics > 0 && !u))) return INSITE_E_INVALID_ARG;
  AffineGramLib lib;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, &lib);
  if (st != INSITE_OK) return st;
  if (n_replicates > INSITE_BOOT_MAX_REPLICATES) return INSITE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < insite_segboot_workspace_bytes(n_patients, n_arms, n_terms, n_replicates))
    return INSITE_E_WORKSPACE;
  if (n_patients == 0) return INSITE_OK;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const BtPlan pl = bt_plan(n_patients, n_arms, lib.nE, n_replicates);
  const int64_t g0 = patient_offset & ~(int64_t)7;
  const int64_t nG = (patient_offset + n_patients - g0 + 7) / 8;  // <= (N + 7) / 8 + 1
  const int64_t gpw = (nG + pl.n_px - 1) / pl.n_px;
  double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + kBtHeader);
  if (n_statics == 0) u = mom;  // never read
  const dim3 grid((unsigned)pl.n_px, (unsigned)pl.n_rg, (unsigned)pl.n_z);
#define INSITE_SEGBOOT_LAUNCH(RT, CT)                                                                              \
  segboot_gram_kernel<RT, CT><<<grid, kWave, 0, hs>>>(mom, u, n_patients, patient_offset, n_arms, lib, seed,       \
                                                      n_replicates, pl.ncol, g0, nG, gpw, pl.rpad, pl.cpad, part)
  switch (pl.ct) {
    case 1: INSITE_SEGBOOT_LAUNCH(kBtRt, 1); break;
    case 2: INSITE_SEGBOOT_LAUNCH(kBtRt, 2); break;
    case 3: INSITE_SEGBOOT_LAUNCH(kBtRt, 3); break;
    case 4: INSITE_SEGBOOT_LAUNCH(kBtRt, 4); break;
    default: INSITE_SEGBOOT_LAUNCH(kBtRt - 1, 5); break;
  }
#undef INSITE_SEGBOOT_LAUNCH
  const int64_t n_out = (int64_t)n_replicates * pl.ncol;
  boot_finalize_kernel<<<dim3((unsigned)((n_out + kBtFinBlock - 1) / kBtFinBlock)), kBtFinBlock, 0, hs>>>(
      part, pl.n_px, pl.rpad, pl.cpad, n_replicates, n_arms, lib, G_out, b_out);
  return launch_status();
}

template <int NARM>
void launch_seg_moments(bool smooth, hipStream_t hs, const double* x, int64_t xsp, int64_t xsk, const int8_t* arm,
                        int64_t asp, int64_t ask, const int32_t* seq_len, int n_steps, int64_t N, int n_arms,
                        double inv_dt, double* mom_out) {
  const int64_t n_tiles = (N + kWave - 1) / kWave;
  int64_t blocks = (n_tiles + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > (1 << 20)) blocks = 1 << 20;  // the tile loop strides over the grid
  const dim3 grid((unsigned)blocks);
  if (smooth)
    seg_moments_kernel<NARM, true><<<grid, kBlock, 0, hs>>>(x, xsp, xsk, arm, asp, ask, seq_len, n_steps, N, n_arms,
                                                           inv_dt, mom_out);
  else
    seg_moments_kernel<NARM, false><<<grid, kBlock, 0, hs>>>(x, xsp, xsk, arm, asp, ask, seq_len, n_steps, N, n_arms,
                                                            inv_dt, mom_out);
}

}  // namespace

extern "C" {

int32_t insite_segboot_abi_version(void) { return INSITE_SEGBOOT_ABI_VERSION; }

int32_t insite_segboot_moments_f64(const double* x, int64_t ldx, const int8_t* arm, int64_t ld_arm, int32_t layout,
                                   int32_t n_steps, const int32_t* seq_len, int64_t n_patients, int32_t n_arms,
                                   int32_t fd_kind, double dt, double* mom_out, void* stream) {
  const bool tm = layout == INSITE_LAYOUT_TIME_MAJOR;
  if (layout != INSITE_LAYOUT_PATIENT_MAJOR && !tm) return INSITE_E_INVALID_ARG;
  if (n_patients < 0 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || !(dt > 0.0) || n_steps < 1 || ldx < 1 || ld_arm < 1)
    return INSITE_E_INVALID_ARG;
  if (tm ? (ldx < n_patients || ld_arm < n_patients) : (ldx < n_steps || ld_arm < n_steps - 1))
    return INSITE_E_INVALID_ARG;
  if (n_patients > 0 && (!x || !arm || !seq_len || !mom_out)) return INSITE_E_INVALID_ARG;
  if (fd_kind != INSITE_FD_ORDER1 && fd_kind != INSITE_FD_SMOOTHED1) return INSITE_E_UNSUPPORTED;
  // 32-bit buffer offsets: a chunk of kSmKC + 2 steps (time-major) or a wave's 64 rows (patient-major)
  const int64_t span = tm ? (int64_t)(kSmKC + 2) : (int64_t)kWave;
  if (ldx > ((int64_t)1 << 31) / (8 * span) || ld_arm > ((int64_t)1 << 31) / span) return INSITE_E_UNSUPPORTED;
  if (n_patients == 0) return INSITE_OK;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const int64_t xsp = tm ? 1 : ldx, xsk = tm ? ldx : 1;
  const int64_t asp = tm ? 1 : ld_arm, ask = tm ? ld_arm : 1;
  const double inv_dt = 1.0 / dt;
  const bool sm = fd_kind == INSITE_FD_SMOOTHED1;
  if (n_arms <= 1)
    launch_seg_moments<1>(sm, hs, x, xsp, xsk, arm, asp, ask, seq_len, n_steps, n_patients, n_arms, inv_dt, mom_out);
  else if (n_arms <= 2)
    launch_seg_moments<2>(sm, hs, x, xsp, xsk, arm, asp, ask, seq_len, n_steps, n_patients, n_arms, inv_dt, mom_out);
  else
    launch_seg_moments<4>(sm, hs, x, xsp, xsk, arm, asp, ask, seq_len, n_steps, n_patients, n_arms, inv_dt, mom_out);
  return launch_status();
}

size_t insite_segboot_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t n_replicates) {
  if (n_patients < 0 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_terms < 1 || n_terms > INSITE_MAX_TERMS ||
      n_replicates < 1 || n_replicates > INSITE_BOOT_MAX_REPLICATES)
    return 0;
  // one partial [rpad][cpad] per wave of the patient dimension
  const BtPlan pl = bt_plan(n_patients, n_arms, n_terms * (n_terms + 1) / 2 + n_terms, n_replicates);
  return kBtHeader + (size_t)pl.n_px * (size_t)pl.rpad * (size_t)pl.cpad * sizeof(double);
}

int32_t insite_segboot_gram_f64(const double* mom, const double* u, int64_t patient_offset, int64_t n_patients,
                                int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms,
                                int32_t n_replicates, uint32_t seed, void* workspace, size_t workspace_bytes,
                                double* G_out, double* b_out, void* stream) {
  return run_segboot_gram(mom, u, patient_offset, n_patients, n_statics, n_arms, exps, n_terms, n_replicates, seed,
                          workspace, workspace_bytes, G_out, b_out, stream);
}

int32_t insite_segboot_fit_f64(const double* mom, const double* u, int64_t patient_offset, int64_t n_patients,
                               int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms,
                               int32_t n_replicates, uint32_t seed, double threshold, double alpha, int32_t max_iter,
                               int32_t unbias, void* workspace, size_t workspace_bytes, double* G_out, double* b_out,
                               double* coef_out, int8_t* mask_out, int32_t* iters_out, void* stream) {
  if (!coef_out || !bt_solver_params_ok(threshold, alpha, 1.0, 0.0, max_iter)) return INSITE_E_INVALID_ARG;
  const int32_t st = run_segboot_gram(mom, u, patient_offset, n_patients, n_statics, n_arms, exps, n_terms,
                                      n_replicates, seed, workspace, workspace_bytes, G_out, b_out, stream);
  if (st != INSITE_OK || n_patients == 0) return st;
  return insite_stlsq_f64(G_out, b_out, (int64_t)n_replicates * n_arms, n_terms, threshold, alpha, max_iter, unbias,
                          coef_out, mask_out, iters_out, stream);
}

}  // extern "C"
