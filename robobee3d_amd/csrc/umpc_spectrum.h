// Error spectra of recorded rollouts (umpcBatchSpectrumInit / umpcBatchSpectrum / umpcBatchSpectrumPower /
// umpcBatchSpectrumGroups, include/umpc_mi355x.h): per robot the projection of a 3-channel signal -- the tracking error
// p - pdes, the attitude error s - sdes or the recorded command -- onto K windowed cosine / sine pairs over a window of the
// step history, in one pass; from the raw sums a periodogram and a chatter score per robot; per group of robots (the draws
// of one grid cell) the periodogram summed over its members. umpcBatchResponse fits ONE frequency the caller knows; this finds
// the oscillation nobody asked for.
//
// Sums kernel. The shape of the response kernel (umpc_response.h): one lane per robot, robot index fastest, every load of a
// wavefront one coalesced row segment, two steps per trip so that the loads of both are issued before the first is used. A
// step reads 6 words per robot (3 with the command, which has no reference; 3 with a constant reference, fetched once).
// The cosines and sines are NOT computed here: row basis_first + i of a host-made fp64 table [W][1 + 2 K] holds the window
// weight w and, per frequency j, w cos and w sin of the step. Every lane of a wavefront is at the same step, so the row is
// wave-uniform: it is fetched with UNIFORM loads into scalar registers (checked in the ISA: s_load_dwordx2 / x4 / x16 of the row
// inside the loop, no vector load and no LDS for it) and each product takes its table word as the scalar operand.
// No sincos on the device: the kernel is bit-identical to the numpy mirror, and a projection onto ANY temporal basis.
// Frequencies are cut into tiles of KT (a template parameter, 8 or 16) and the tile is blockIdx.y: a lane carries
// 8 + 6 KT fp64 accumulators (n, skipped, sum w y and sum w y y per channel; C_j and S_j per channel and frequency of the
// tile) -- 104 at KT = 16, the lag-moments kernel's regime of two waves per SIMD out of the unified register file, 56 at
// KT = 8, three waves per SIMD: the faster one at the shape of record and the one the library launches. Every tile folds the 8 common sums (a few operations); tile 0 alone writes them. A tile that K cuts short reads
// the last frequency again in the slots past it and stores nothing from them: the loop has no test per frequency.
// A step enters for a robot when every word it reads is finite; otherwise `skipped` counts it and its value is +0 in every
// product, so that every other row receives +0 (the basis must be finite). Selects, no branches: see umpc_score.h.
// The step range is split over UMPC_SPEC_SLICES = 2 wavefronts per block of 64 robots: slice s folds steps s, s + 2, .. in
// order. The slices meet once in LDS: slice 1 parks its accumulators (104 x 64 doubles = 53 248 B at KT = 16: three blocks
// fit a CU's 160 KiB; four slices would park 159 744 B and leave one block of four wavefronts per CU, three slices two
// blocks of three), slice 0 adds them and then adds the total into `sums`: partials in the order 0, 1, then sums += total.
// Nothing crosses robots, and neither the tile size nor the number of tiles enters a sum: a robot's sums depend on its own
// columns, the basis rows and `count` alone -- bit-equal from run to run, between a column block and the same columns of the
// whole batch, and between KT = 8 and KT = 16. No atomics, no temporaries.
//
// Power kernel. One lane per robot, fp64, registers only, rounded to the dtype at the store: the mean through the window's
// own transform, the periodogram P_j = 4 (A_j^2 + B_j^2) / W0^2 and the rows of score.SPEC_*, in exactly the operation order
// of score.spectrum_power_reference (two passes over the robot's sums: the bandwidth needs the centroid).
//
// Groups kernel. One wavefront per (group, channel) on the tables of umpcBatchGroupIndex: the member walk of the dispersion
// kernel (lane l takes members l, l + 64, ..), one accumulator per frequency, and lag_tree's fold -- v_permlane32_swap /
// v_permlane16_swap for the stages 32 and 16, __shfl_xor below -- over one or two trees of 32 frequencies. A row is a function
// of the group's member list alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_propagator.h"

// wavefronts per block of 64 robots = ways a call's step range is split; part of the order of summation, mirrored in
// robobee3d_amd/_lib.py and robobee3d_amd/score.py
#define UMPC_SPEC_SLICES 2

namespace umpc {

constexpr int kSpecSlices = UMPC_SPEC_SLICES;
constexpr int kSpecMaxK = 64, kSpecRows = 12;
constexpr int kSpecCommon = 8;      // n, skipped, then (sum w y, sum w y y) per channel: the sums every tile carries
constexpr int kSpecRefNone = 0, kSpecRefConst = 1, kSpecRefTable = 2;

// pointers as the kernel reads them: the host has moved them to the first slice AND the first row of the call (state:
// slice first + after, row 0 or 9; the command: slice first of the out record, row 0; reference: row 0 or 6; basis: row
// basis_first)
template <typename T>
struct SpecArgs {
  const T *y;             // [..][ystride][B]
  const T *reftab;        // [..][9][B], kSpecRefTable
  const T *ref;           // [3][B] of the constant reference, kSpecRefConst
  const double *basis;    // [..][1 + 2 K]
  double *sums;           // [2 + 3 (2 + 2 K)][B] in/out
  int B, count, K, ystride;
};

// col = the block's first robot, the same in every lane, i = the wavefront's step
template <typename T, int REF>
__device__ __forceinline__ void spec_load(const SpecArgs<T> &a, size_t B, size_t col, unsigned lane, long long i, const T (&rc)[3],
                                          T (&y)[3], T (&r)[3]) {
  const T *st = a.y + ((size_t)i * a.ystride * B + col);
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = st[(size_t)c * B + lane];
  if (REF == kSpecRefTable) {
    const T *rt = a.reftab + ((size_t)i * 9 * B + col);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = rt[(size_t)c * B + lane];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = rc[c];      // (zeros without a reference)
  }
}

// what one step adds to the 8 + 6 KT sums of a robot. row = the step's basis row (wave-uniform), j0 = the tile's first
// frequency. FULL: the tile lies inside K; otherwise the slots past K read frequency K - 1 again (never stored).
template <typename T, int REF, int KT, bool FULL>
__device__ __forceinline__ void spec_step(const double *row, int j0, int K, const T (&yv)[3], const T (&rv)[3],
                                          double (&q)[kSpecCommon + 6 * KT]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) ok = ok & __builtin_isfinite(yv[c]) & (REF == kSpecRefNone ? true : __builtin_isfinite(rv[c]));
  q[0] += ok ? 1.0 : 0.0;
  q[1] += ok ? 0.0 : 1.0;
  const double w = row[0];
  double v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // the difference in the dtype, one rounding, then widened exactly; a step that does not enter has v = +0
    const T d = REF == kSpecRefNone ? yv[c] : yv[c] - rv[c];
    v[c] = ok ? (double)d : 0.0;
    const double t = __dmul_rn(w, v[c]);
    q[2 + 2 * c] += t;
    q[3 + 2 * c] += __dmul_rn(t, v[c]);
  }
#pragma unroll
  for (int jj = 0; jj < KT; ++jj) {
    const int j = FULL ? j0 + jj : (j0 + jj < K ? j0 + jj : K - 1);
    const double bc = row[1 + 2 * j], bs = row[2 + 2 * j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      q[kSpecCommon + (c * KT + jj) * 2] += __dmul_rn(v[c], bc);
      q[kSpecCommon + (c * KT + jj) * 2 + 1] += __dmul_rn(v[c], bs);
    }
  }
}

// the steps slice, slice + S, .. of the call, two per trip: the loads of both are issued before the first is used
template <typename T, int REF, int KT, bool FULL>
__device__ __forceinline__ void spec_walk(const SpecArgs<T> &a, size_t B, size_t col, unsigned lane, int slice, int j0, const T (&rc)[3],
                                          double (&q)[kSpecCommon + 6 * KT]) {
  const int K = a.K;
  const size_t bstride = 1 + 2 * (size_t)K;
  int i = slice;                           // (count <= 2^31 - 1 - 2 kSpecSlices, umpcBatchSpectrum: no sum here wraps)
  for (; i + kSpecSlices < a.count; i += 2 * kSpecSlices) {
    T y0[3], r0[3], y1[3], r1[3];
    spec_load<T, REF>(a, B, col, lane, i, rc, y0, r0);
    spec_load<T, REF>(a, B, col, lane, i + kSpecSlices, rc, y1, r1);
    spec_step<T, REF, KT, FULL>(a.basis + (size_t)i * bstride, j0, K, y0, r0, q);
    spec_step<T, REF, KT, FULL>(a.basis + (size_t)(i + kSpecSlices) * bstride, j0, K, y1, r1, q);
  }
  if (i < a.count) {
    T y0[3], r0[3];
    spec_load<T, REF>(a, B, col, lane, i, rc, y0, r0);
    spec_step<T, REF, KT, FULL>(a.basis + (size_t)i * bstride, j0, K, y0, r0, q);
  }
}

// (two waves per SIMD at KT = 16; three at KT = 8 in fp32 -- fp64 tables with KT = 8 spill three words at three)
template <typename T, int REF, int KT>
__global__ __launch_bounds__(64 * kSpecSlices, KT > 8 || sizeof(T) == 8 ? 2 : 3) void umpc_spectrum_kernel(const SpecArgs<T> a) {
  constexpr int NQ = kSpecCommon + 6 * KT;
  static_assert(KT % 4 == 0, "the final fold takes four frequencies at a time");
  __shared__ double lds[kSpecSlices - 1][NQ][64];
  // (blockDim = (64, kSpecSlices): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int tile = blockIdx.y, j0 = tile * KT, K = a.K;
  const size_t B = (size_t)a.B, col = (size_t)blockIdx.x * 64, b = col + lane;
  const bool live = b < B;                 // (a lane past the batch loads nothing, but meets the barrier)
  double q[NQ];
#pragma unroll
  for (int r = 0; r < NQ; ++r) q[r] = 0.0;
  if (live) {
    T rc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rc[c] = REF == kSpecRefConst ? a.ref[(size_t)c * B + b] : T(0);
    if (j0 + KT <= K) spec_walk<T, REF, KT, true>(a, B, col, (unsigned)lane, slice, j0, rc, q);
    else spec_walk<T, REF, KT, false>(a, B, col, (unsigned)lane, slice, j0, rc, q);
  }
  if (slice > 0) {
#pragma unroll
    for (int r = 0; r < NQ; ++r) lds[slice - 1][r][lane] = q[r];
  }
  __syncthreads();
  if (slice > 0 || !live) return;
  // the slices in the fixed order 0, 1, .., then the call's total into the sums, eight rows at a time: their old values are
  // requested before the fold and stored after it, as in the response kernel
  double *sm = a.sums + b;
  const size_t chan = 2 + 2 * (size_t)K;       // rows per channel
  if (tile == 0) {
    double old[kSpecCommon];
#pragma unroll
    for (int r = 0; r < kSpecCommon; ++r) {
      const size_t row = r < 2 ? (size_t)r : 2 + (size_t)((r - 2) >> 1) * chan + ((r - 2) & 1);
      old[r] = sm[row * B];
    }
#pragma unroll
    for (int r = 0; r < kSpecCommon; ++r) {
#pragma unroll
      for (int s = 0; s < kSpecSlices - 1; ++s) q[r] += lds[s][r][lane];
    }
#pragma unroll
    for (int r = 0; r < kSpecCommon; ++r) {
      const size_t row = r < 2 ? (size_t)r : 2 + (size_t)((r - 2) >> 1) * chan + ((r - 2) & 1);
      sm[row * B] = old[r] + q[r];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int g = 0; g < KT / 4; ++g) {
      // frequencies j0 + 4 g .. j0 + 4 g + 3 of channel c: eight consecutive rows of `sums`, eight consecutive accumulators
      const int at = kSpecCommon + c * 2 * KT + 8 * g;
      double *rows = sm + (2 + (size_t)c * chan + 2 + 2 * (size_t)(j0 + 4 * g)) * B;
      double old[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) old[e] = j0 + 4 * g + (e >> 1) < K ? rows[(size_t)e * B] : 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int s = 0; s < kSpecSlices - 1; ++s) q[at + e] += lds[s][at + e][lane];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (j0 + 4 * g + (e >> 1) < K) rows[(size_t)e * B] = old[e] + q[at + e];
    }
  }
}

// ---- power -----------------------------------------------------------------------------------------------------------
// the window's column sums and the frequencies travel in the launch arguments
template <typename T>
struct SpecPowerArgs {
  double wsum[1 + 2 * kSpecMaxK], freq[kSpecMaxK];
  const double *sums;     // [2 + 3 (2 + 2 K)][B]
  T *power;               // [3][K][B]
  T *spec;                // [3][12][B]
  double nrows;
  int B, K, jsplit;
};

// P_j of one channel of one robot: the mean is removed through the window's own transform
__device__ __forceinline__ double spec_power(const double *ch, size_t B, int j, double m, double wc, double ws, double w02) {
  const double A = ch[(size_t)(2 + 2 * j) * B] - m * wc, Bq = ch[(size_t)(3 + 2 * j) * B] - m * ws;
  return (4.0 * (A * A + Bq * Bq)) / w02;
}

template <typename T>
__global__ __launch_bounds__(256) void umpc_spectrum_power_kernel(const SpecPowerArgs<T> a) {
  const size_t B = (size_t)a.B, b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int K = a.K;
  const double *sm = a.sums + b;
  const double n = sm[0], skipped = sm[B], w0 = a.wsum[0], w02 = w0 * w0, nan = __builtin_nan("");
  const bool counts = (skipped > 0.0) | (n != a.nrows) | !(n >= 2.0);
  for (int c = 0; c < 3; ++c) {
    const double *ch = sm + (2 + (size_t)c * (2 + 2 * (size_t)K)) * B;
    const double m = ch[0] / w0, var = ch[B] / w0 - m * m;
    double total = 0.0, peak = 0.0, cnum = 0.0, high = 0.0;
    int jpeak = 0;
    for (int j = 0; j < K; ++j) {
      const double P = spec_power(ch, B, j, m, a.wsum[1 + 2 * j], a.wsum[2 + 2 * j], w02);
      total += P;
      const bool better = (j == 0) | (P > peak);      // the first maximum
      peak = better ? P : peak;
      jpeak = better ? j : jpeak;
      cnum += a.freq[j] * P;
      high += j >= a.jsplit ? P : 0.0;
    }
    const double cen = cnum / total;
    const bool refused = counts | !(total > 0.0) | !__builtin_isfinite(total);
    T *pw = a.power + (size_t)c * K * B + b;
    double bnum = 0.0;
    for (int j = 0; j < K; ++j) {
      const double P = spec_power(ch, B, j, m, a.wsum[1 + 2 * j], a.wsum[2 + 2 * j], w02);
      const double d = a.freq[j] - cen;
      bnum += (d * d) * P;
      pw[(size_t)j * B] = T(refused ? nan : P);
    }
    T *o = a.spec + (size_t)c * kSpecRows * B + b;
    o[0] = T(refused ? 0.0 : n);
    o[B] = T(skipped);
    o[2 * B] = T(refused ? nan : m);
    o[3 * B] = T(refused ? nan : var);
    o[4 * B] = T(refused ? nan : total);
    o[5 * B] = T(refused ? nan : (double)jpeak);
    o[6 * B] = T(refused ? nan : a.freq[jpeak]);
    o[7 * B] = T(refused ? nan : peak);
    o[8 * B] = T(refused ? nan : peak / total);
    o[9 * B] = T(refused ? nan : cen);
    o[10 * B] = T(refused ? nan : __dsqrt_rn(bnum / total));
    o[11 * B] = T(refused ? nan : high / total);
  }
}

// ---- groups ----------------------------------------------------------------------------------------------------------
template <typename T>
struct SpecGroupArgs {
  const T *power;         // [3][K][B]
  const T *spec;          // [3][12][B]
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  double *gspec;          // [G][3][2 + K]
  int B, K;
};

// frequencies 32 t .. 32 t + 31 by the halving tree of lag_tree: lane l ends with frequency 32 t + (l >> 1)
template <int NT, int TREE>
__device__ __forceinline__ double spec_tree(const double (&q)[32 * NT], int lane) {
  double x32[32], x16[16], x8[8], x4[4], x2[2], x1[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) x32[j] = q[32 * TREE + j];
  lag_halve_swap<16, 32>(x32, x16);
  lag_halve_swap<8, 16>(x16, x8);
  disp_halve<4>(x8, x4, (lane & 8) != 0, 8);
  disp_halve<2>(x4, x2, (lane & 4) != 0, 4);
  disp_halve<1>(x2, x1, (lane & 2) != 0, 2);
  return x1[0] + __shfl_xor(x1[0], 1);
}

// NT = trees of 32 frequencies a lane carries (K <= 32 NT). A slot past K reads frequency K - 1 and folds +0.
template <typename T, int NT>
__global__ __launch_bounds__(64) void umpc_spectrum_groups_kernel(const SpecGroupArgs<T> a) {
  const int lane = threadIdx.x, g = blockIdx.x, c = blockIdx.y, K = a.K;
  const auto [lo, n] = group_window(a.offset, g);
  const size_t B = (size_t)a.B;
  const int32_t *mem = a.order + lo;
  const T *pw = a.power + (size_t)c * K * B, *enter = a.spec + (size_t)c * kSpecRows * B;
  double q[32 * NT];
#pragma unroll
  for (int s = 0; s < 32 * NT; ++s) q[s] = 0.0;
  int cnt[2] = {0, 0};
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane;
    const bool live = m < n;
    const int b = mem[live ? m : n - 1];
    const bool ok = live & (enter[b] > T(0));
    cnt[0] += __popcll(__ballot(ok));
    cnt[1] += __popcll(__ballot(live & !ok));
    T v[32 * NT];
#pragma unroll
    for (int s = 0; s < 32 * NT; ++s) v[s] = pw[(size_t)(s < K ? s : K - 1) * B + b];
#pragma unroll
    for (int s = 0; s < 32 * NT; ++s) q[s] += (ok & (s < K)) ? (double)v[s] : 0.0;
  }
  double *row = a.gspec + ((size_t)g * 3 + c) * (2 + K);
  const int r = lane >> 1;
  const bool even = (lane & 1) == 0;
  const double t0 = spec_tree<NT, 0>(q, lane);
  if (even & (r < K)) row[2 + r] = t0;
  if constexpr (NT > 1) {
    const double t1 = spec_tree<NT, 1>(q, lane);
    if (even & (32 + r < K)) row[2 + 32 + r] = t1;
  }
  if (lane < 2) row[lane] = (double)(lane == 0 ? cnt[0] : cnt[1]);
}

}  // namespace umpc
