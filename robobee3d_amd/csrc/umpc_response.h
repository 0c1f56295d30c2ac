// Frequency response of recorded rollouts (umpcBatchResponseInit / umpcBatchResponse / umpcBatchResponseFit,
// include/umpc_mi355x.h): a three-parameter sine fit y_k ~ a0 + a1 cos phi_k + a2 sin phi_k per robot and position axis, of
// p (state rows 0..2) and of pdes (reference rows 0..2), at the robot's own frequency nu[b] -- the Bode point of each robot of
// a (trajFreq x draws) sweep. Two stages, as a score has raw sums before means: the accumulation kernel adds the 33 sums of
// the normal equations per robot in one pass over the step history (once per chunk of a chunked run), the fit kernel solves
// them once.
//
// Accumulation kernel. The shape is the score kernel's (umpc_score.h): one lane per robot, robot index fastest, every load of
// a wavefront one coalesced row segment (256 B in fp32); a block of 64 robots is kRespSlices = 4 wavefronts, slice s takes steps
// s, s + 4, s + 8, .. of the call, two steps per trip. A step reads 6 words per robot (state rows 0..2, reference rows 0..2),
// so a wavefront has 12 row segments requested before the first is used (6 with a constant reference, whose words are
// fetched once per robot) and up to 12 wavefronts of a CU stream at a time. Which reference there is is a template parameter,
// and the accumulation is written with selects (see the note in umpc_score.h: branches around the loads drain the queue).
// The phase is u = k nu - floor(k nu) with ONE IEEE double multiply of (double)k and nu (__dmul_rn: never contracted), then
// sincospi(2 u) in fp64: exact zeros and ones at the quarter points, a few ulp elsewhere, whatever k is -- a step0 of 10^6 and
// a chunked call see the same phase as the undivided one. The inputs are widened exactly and every product and sum is fp64:
// ~50 fp64 multiply-adds and one sincospi per robot-step against 24 B of loads in fp32.
// Each lane carries the 33 partial sums of its slice in registers (66 VGPRs). The slices meet once, in LDS: slices 1..3 park
// their 33 doubles per robot (3 x 33 x 64 x 8 B = 50 688 B: three blocks, 12 wavefronts, fit a CU -- the score kernel's eight
// slices would be 118 KB and one block), slice 0 adds them in the fixed order 1, 2, 3 and adds the total into `sums`.
// Nothing crosses robots and the slice count is a constant: a robot's sums depend on its own columns and on (step0, count)
// alone -- bit-equal from run to run and between a column block and the same columns of the whole batch. No atomics, no
// temporaries.
//
// Fit kernel. One lane per robot, fp64 throughout, rounded to the dtype at the store: the Cholesky factor of the normal
// matrix in the variable order (1, cos, sin), shared by the six right-hand sides of a robot (y and r of three axes), in
// exactly the operation order of score.response_fit_reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_score.h"

namespace umpc {

constexpr int kRespSumRows = 33, kRespRows = 12;
constexpr int kRespSlices = 4;      // wavefronts per block of 64 robots = ways a call's step range is split
constexpr int kRespCommon = 6, kRespAxis = 9;      // n, skipped, sum c, s, cc, cs; then 9 rows per axis
constexpr int kRespFold = 11;                      // rows of `sums` in flight at a time in the final fold (33 = 3 x 11)

// pointers as the kernel reads them: the host has moved them to the first slice of the call (state: slice first + after)
template <typename T>
struct RespArgs {
  const T *state;         // [..][18][B]
  const T *reftab;        // [..][9][B] or null
  const T *ref;           // [9][B], read when reftab is null
  const double *nu;       // [B] revolutions per step
  double *sums;           // [33][B] in/out
  int B, count;
  long long step0;
};

// col = the block's first robot, the same in every lane, i = the wavefront's step; the inputs are widened here, exactly
template <typename T, bool NT, bool TAB>
__device__ __forceinline__ void resp_load(const RespArgs<T> &a, size_t B, size_t col, unsigned lane, long long i,
                                          const T (&rc)[3], T (&y)[3], T (&r)[3]) {
  const T *st = a.state + ((size_t)i * 18 * B + col);
#pragma unroll
  for (int j = 0; j < 3; ++j) y[j] = score_ld<NT>(st + (size_t)j * B + lane);
  if (TAB) {
    const T *rt = a.reftab + ((size_t)i * 9 * B + col);
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = score_ld<NT>(rt + (size_t)j * B + lane);
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = rc[j];
  }
}

// what step k adds to the 33 sums of a robot; a step with a word or a phase that is not finite adds one to `skipped` and
// +0 to every other row
template <typename T>
__device__ __forceinline__ void resp_step(long long k, double nu, const T (&yv)[3], const T (&rv)[3], double (&q)[kRespSumRows]) {
  const double x = __dmul_rn((double)k, nu);
  const double u = x - floor(x);
  double s, c;
  sincospi(2.0 * u, &s, &c);
  bool ok = __builtin_isfinite(u);
#pragma unroll
  for (int j = 0; j < 3; ++j) ok = ok & __builtin_isfinite(yv[j]) & __builtin_isfinite(rv[j]);
  q[0] += ok ? 1.0 : 0.0;
  q[1] += ok ? 0.0 : 1.0;
  q[2] += ok ? c : 0.0;
  q[3] += ok ? s : 0.0;
  q[4] += ok ? c * c : 0.0;
  q[5] += ok ? c * s : 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double y = (double)yv[j], r = (double)rv[j];
    double *a = q + kRespCommon + kRespAxis * j;
    a[0] += ok ? y : 0.0;
    a[1] += ok ? y * c : 0.0;
    a[2] += ok ? y * s : 0.0;
    a[3] += ok ? y * y : 0.0;
    a[4] += ok ? r : 0.0;
    a[5] += ok ? r * c : 0.0;
    a[6] += ok ? r * s : 0.0;
    a[7] += ok ? r * r : 0.0;
    a[8] += ok ? y * r : 0.0;
  }
}

template <typename T, bool NT, bool TAB>
__global__ __launch_bounds__(64 * kRespSlices) void umpc_response_kernel(const RespArgs<T> a) {
  __shared__ double lds[kRespSlices - 1][kRespSumRows][64];
  // (blockDim = (64, kRespSlices): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const size_t B = (size_t)a.B, col = (size_t)blockIdx.x * 64, b = col + lane;
  const bool live = b < B;                 // (a lane past the batch loads nothing, but meets the barrier)
  double q[kRespSumRows];
#pragma unroll
  for (int r = 0; r < kRespSumRows; ++r) q[r] = 0.0;
  if (live) {
    T rc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) rc[j] = TAB ? T(0) : a.ref[(size_t)j * B + b];
    const double nu = a.nu[b];
    // two steps per trip: the loads of both are issued before the first is used
    int i = slice;                         // (count <= 2^31 - 1 - 2 kRespSlices, umpcBatchResponse: no sum here wraps)
    for (; i + kRespSlices < a.count; i += 2 * kRespSlices) {
      T y0[3], r0[3], y1[3], r1[3];
      resp_load<T, NT, TAB>(a, B, col, (unsigned)lane, i, rc, y0, r0);
      resp_load<T, NT, TAB>(a, B, col, (unsigned)lane, i + kRespSlices, rc, y1, r1);
      resp_step<T>(a.step0 + i, nu, y0, r0, q);
      resp_step<T>(a.step0 + i + kRespSlices, nu, y1, r1, q);
    }
    if (i < a.count) {
      T y0[3], r0[3];
      resp_load<T, NT, TAB>(a, B, col, (unsigned)lane, i, rc, y0, r0);
      resp_step<T>(a.step0 + i, nu, y0, r0, q);
    }
  }
  if (slice > 0) {
#pragma unroll
    for (int r = 0; r < kRespSumRows; ++r) lds[slice - 1][r][lane] = q[r];
  }
  __syncthreads();
  if (slice > 0 || !live) return;
  // the slices in the fixed order 0, 1, 2, 3, then the call's total into the sums, eleven rows at a time: their old
  // values are requested before the fold and stored after it (written as `sm[r B] += q[r]` the 33 rows are 33 dependent
  // round trips; all 33 at once cost a wavefront per SIMD in registers)
  double *sm = a.sums + b;
#pragma unroll
  for (int r0 = 0; r0 < kRespSumRows; r0 += kRespFold) {
    double old[kRespFold];
#pragma unroll
    for (int r = 0; r < kRespFold; ++r) old[r] = sm[(size_t)(r0 + r) * B];
#pragma unroll
    for (int r = 0; r < kRespFold; ++r) {
#pragma unroll
      for (int s = 0; s < kRespSlices - 1; ++s) q[r0 + r] += lds[s][r0 + r][lane];
    }
#pragma unroll
    for (int r = 0; r < kRespFold; ++r) sm[(size_t)(r0 + r) * B] = old[r] + q[r0 + r];
  }
}

// a = M^-1 rhs through the factor (l11, l21, l31, l22, l32, l33) of M = L L^T
struct RespFactor { double l11, l21, l31, l22, l32, l33; };
__device__ __forceinline__ void resp_solve(const RespFactor &f, double b0, double b1, double b2, double (&a)[3]) {
  const double z0 = b0 / f.l11;
  const double z1 = (b1 - f.l21 * z0) / f.l22;
  const double z2 = ((b2 - f.l31 * z0) - f.l32 * z1) / f.l33;
  a[2] = z2 / f.l33;
  a[1] = (z1 - f.l32 * a[2]) / f.l22;
  a[0] = ((z0 - f.l21 * a[1]) - f.l31 * a[2]) / f.l11;
}

template <typename T>
__global__ __launch_bounds__(256) void umpc_response_fit_kernel(const double *sums, T *resp, int B_) {
  const size_t B = (size_t)B_, b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double *sm = sums + b;
  const double n = sm[0], skipped = sm[B], Sc = sm[2 * B], Ss = sm[3 * B], Scc = sm[4 * B], Scs = sm[5 * B];
  const double Sss = n - Scc, tol = 1e-9 * n, nan = __builtin_nan("");
  // Cholesky in the variable order (1, cos, sin); the pivots are d1, d2, d3 (a NaN pivot fails its test)
  RespFactor f;
  const double d1 = n;
  f.l11 = sqrt(d1);
  f.l21 = Sc / f.l11; f.l31 = Ss / f.l11;
  const double d2 = Scc - f.l21 * f.l21;
  f.l22 = sqrt(d2);
  f.l32 = (Scs - f.l21 * f.l31) / f.l22;
  const double d3 = (Sss - f.l31 * f.l31) - f.l32 * f.l32;
  f.l33 = sqrt(d3);
  const bool fit = (n >= 3.0) & (d1 > tol) & (d2 > tol) & (d3 > tol);
  for (int j = 0; j < 3; ++j) {
    const double *x = sm + (size_t)(kRespCommon + kRespAxis * j) * B;
    T *o = resp + (size_t)j * kRespRows * B + b;
    o[B] = T(skipped);
    if (!fit) {
      o[0] = T(0);
      for (int r = 2; r < kRespRows; ++r) o[(size_t)r * B] = T(nan);
      continue;
    }
    const double y0 = x[0], y1 = x[B], y2 = x[2 * B], Syy = x[3 * B];
    double ay[3], ar[3];
    resp_solve(f, y0, y1, y2, ay);
    resp_solve(f, x[4 * B], x[5 * B], x[6 * B], ar);
    const double yamp2 = ay[1] * ay[1] + ay[2] * ay[2], ramp2 = ar[1] * ar[1] + ar[2] * ar[2];
    // Y = a1 - i a2: Y conj(R) = re + i im, H = Y / R = (re + i im) / |R|^2
    const double re = ay[1] * ar[1] + ay[2] * ar[2], im = ay[1] * ar[2] - ay[2] * ar[1];
    const bool href = ramp2 > 0.0;
    const double res = (Syy - ((ay[0] * y0 + ay[1] * y1) + ay[2] * y2)) / n;
    const double e1 = ay[1] - ar[1], e2 = ay[2] - ar[2];
    const double at = atan2(im, re), pi = 3.14159265358979323846;
    const double phase = at == -pi ? pi : at;      // (-pi, pi]: atan2 gives -pi for im = -0, re < 0
    o[0] = T(n);
    o[2 * B] = T(yamp2);
    o[3 * B] = T(ramp2);
    o[4 * B] = T(href ? sqrt(yamp2 / ramp2) : nan);
    o[5 * B] = T(href ? phase : nan);
    o[6 * B] = T(href ? re / ramp2 : nan);
    o[7 * B] = T(href ? im / ramp2 : nan);
    o[8 * B] = T(ay[0]);
    o[9 * B] = T(ar[0]);
    o[10 * B] = T(res > 0.0 ? res : 0.0);
    o[11 * B] = T(e1 * e1 + e2 * e2);
  }
}

}  // namespace umpc
