// Bootstrap intervals of a sweep's cost table (umpcBatchScoreBootstrap, include/umpc_mi355x.h): the draws of a grid cell are
// resampled with replacement R times ON the device, a statistic (the mean, or a nearest-rank quantile) is taken of every
// resample, and each cell gets its point estimate, the mean and standard error of its R replicates and their percentile
// interval. Nothing of size [R, B] exists anywhere: a wavefront holds a cell of up to 64 in its registers and draws, gathers
// and reduces there; what reaches memory is reps [G][R] and boot [G][5 + nq].
//
// The draw. Slot m of replicate r of a cell with nsc scored values takes v[j], j = min(nsc - 1, floor(u * nsc)) in double,
// u = u01(seed, (r << 32) + m, salt 41): the counter hash of batch._u01. It depends on (seed, r, m, nsc) and on nothing
// else -- not on the cell, G, the grid or the launch --, so cells with equal nsc are resampled with the SAME indices:
// common random numbers across cells. The hash is computed where it is used (64-bit integer VALU, two wrap-around
// multiplies), not tabulated: see "hash or table" in DESIGN.md.
//
// Three steps on one stream.
// 1. umpc_boot_compact_kernel, one wavefront per cell: the values that enter (boot_score_value: the rule of
//    quant_score_value, optionally minus the same expression of a second table) are written in member-list order at
//    work[offset[g] + rank], rank from the ballot of the trip and a running count as in umpc_group_index_kernel; nsc goes to
//    work[B + g]. From here on nothing knows about scores: the replicate kernels see v[0 .. nsc) as doubles.
// 2. The replicate kernels on a grid (cell, slice of R), launched one behind the other; a block leaves the one that is
//    not its own, as in umpc_quantile.h.
//    A. nsc <= 64, umpc_boot_rep_kernel: a WAVEFRONT owns chunks of 64 consecutive replicates. Lane m holds v[m] (one
//    coalesced load per chunk loop, kept for every replicate). Per replicate: the hash, one double multiply, one
//    conversion, and v[j] by ds_bpermute (two dwords). Mean: lanes >= nsc carry +0, the 64 values meet in a butterfly over
//    lane ^ 1, 2, 4, 8, 16 (DPP and ds_swizzle: quant_partner) and lane ^ 63 (after five stages both halves are uniform,
//    so ^63 is as good as ^32), all lanes end with the same bits, one division by nsc. Quantile: quant_sort64 on the
//    images of the gathered values, then one quant_from_lane at quant_rank(stat_p, nsc). Two replicates per trip, so that
//    one's DPP wait states are filled by the other's. Replicate r0 + i of a chunk is kept by lane i: a chunk leaves as one
//    coalesced 512-B store. No LDS memory, no barrier, no scratch.
//    B. nsc > 64, umpc_boot_mean_block_kernel / umpc_boot_quantile_block_kernel: correct for any size, not tuned. The
//    block takes one replicate at a time and gathers work[offset[g] + j] through L2. Mean: thread t adds slots t, t + 256,
//    .. in that order, then a fixed tree over the 256 partial sums in LDS. Quantile: quant_block_row<uint64_t> with a keyof
//    that goes through the resample index (the index is hashed again on each of the 8 passes).
//    Either path also forms the point estimate -- the same statistic, the same order of summation, identity indices -- and
//    writes it to boot[g][2].
// 3. umpc_boot_row_kernel, one block per cell over reps[g][0 .. R): the percentile columns by quant_block_row, the mean of
//    the replicates accumulated in double-double (TwoSum per addend, thread-strided, a fixed LDS tree), then a second pass
//    for sum (t_r - mean)^2 in plain doubles in the same order (boot_row_moments).
// Orders of summation. A replicate's sum: path A the butterfly above, path B thread-strided then the tree: functions of nsc
// alone. The row's: thread-strided then the tree: functions of R alone. Nothing is atomic; two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_quantile.h"

namespace umpc {

constexpr int kBootWaves = 4;
constexpr int kBootThreads = 64 * kBootWaves;     // = kQuantThreads: quant_block_row strides by that
static_assert(kBootThreads == kQuantThreads, "quant_block_row walks a cell with kQuantThreads threads");
constexpr int kBootMean = 0, kBootQuantile = 1;   // UMPC_BOOT_MEAN, UMPC_BOOT_QUANTILE
constexpr int kBootRows = 5;                      // UMPC_BOOT_ROWS
constexpr unsigned long long kBootSalt = 41;

template <typename T>
struct BootCompactArgs {
  const T *score, *other;   // [12][B]; other may be null
  const int32_t *order, *offset;
  double *work;             // [B + G]
  int B, num, den;
};

struct BootArgs {
  const int32_t *offset;    // [G + 1]
  const double *work;       // [B + G]: the scored values of cell g at offset[g] .., nsc of cell g at B + g
  double *boot;             // [G][5 + nq]
  double *reps;             // [G][R]
  unsigned long long c0;    // seed * 0x9E3779B97F4A7C15 + salt
  double stat_p;
  int B, R;
  QuantProbs q;
};

// ---- the draw ---------------------------------------------------------------------------------------------------------
// batch._u01 behind the counter's offset: two multiply-xorshift rounds, the top 53 bits
__device__ __forceinline__ double boot_u01(unsigned long long c0, unsigned long long idx) {
  unsigned long long v = idx + c0;
  v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ull;
  v ^= v >> 27; v *= 0x94D049BB133111EBull;
  v ^= v >> 31;
  return (double)(v >> 11) * 0x1p-53;             // exact: 53 bits, a power of two
}
// the member slot m of replicate r takes, 0 <= j < nsc (nsc >= 1): one IEEE double multiply, truncation, a clamp
__device__ __forceinline__ int boot_index(unsigned long long c0, int r, int m, int nsc) {
  const double u = boot_u01(c0, ((unsigned long long)(unsigned)r << 32) + (unsigned long long)(unsigned)m);
  const int j = (int)(u * (double)nsc);
  return j < nsc - 1 ? j : nsc - 1;
}

// ---- a wavefront's statistic ------------------------------------------------------------------------------------------
// one butterfly stage of the fp64 sum: every lane adds the value of lane ^ P (both partners add the same two values)
template <int P, int NS>
__device__ __forceinline__ void boot_add_stage(uint64_t (&b)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s)
    b[s] = (uint64_t)__double_as_longlong(__longlong_as_double((long long)b[s]) +
                                          __longlong_as_double((long long)quant_partner(b[s], P)));
}

// NS sets of 64 lane values, of which lanes 0 .. nsc - 1 count (1 <= nsc <= 64): x[s] becomes the statistic in every lane.
// k = quant_rank(stat_p, nsc) for the quantile.
template <int STAT, int NS>
__device__ __forceinline__ void boot_wave_stat(double (&x)[NS], int nsc, int k, int lane) {
  if (STAT == kBootMean) {
    uint64_t b[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) b[s] = (uint64_t)__double_as_longlong(lane < nsc ? x[s] : 0.0);
    boot_add_stage<1>(b); boot_add_stage<2>(b); boot_add_stage<4>(b); boot_add_stage<8>(b); boot_add_stage<16>(b);
    boot_add_stage<63>(b);                              // both halves are uniform by now: ^63 serves as ^32
#pragma unroll
    for (int s = 0; s < NS; ++s) x[s] = __longlong_as_double((long long)b[s]) / (double)nsc;
  } else {
    uint64_t key[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) key[s] = lane < nsc ? quant_image(x[s]) : ~0ull;
    quant_sort64(key, lane);
#pragma unroll
    for (int s = 0; s < NS; ++s) x[s] = quant_value(quant_from_lane(key[s], k));
  }
}

// ---- 1. compaction ----------------------------------------------------------------------------------------------------
// the value of robot b and whether it enters: quant_score_value's rule on one table, or on both and their difference
template <typename T, bool PAIR>
__device__ __forceinline__ double boot_score_value(const BootCompactArgs<T> &e, int b, bool &ok) {
  double x = score_table_value(e.score, (size_t)e.B, e.num, e.den, b, ok);
  if (PAIR) {
    bool ok2;
    x = x - score_table_value(e.other, (size_t)e.B, e.num, e.den, b, ok2);
    ok &= ok2;
  }
  ok &= __builtin_isfinite(x);
  return x;
}

template <typename T, bool PAIR>
__global__ __launch_bounds__(64) void umpc_boot_compact_kernel(const BootCompactArgs<T> e) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  const int32_t *mem = e.order + lo;
  double *v = e.work + lo;
  int at = 0;
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane;
    bool ok = false;
    double x = 0.0;
    if (m < n) x = boot_score_value<T, PAIR>(e, mem[m], ok);
    const unsigned long long bal = __ballot(ok);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    if (ok) v[at + rank] = x;                        // at + rank < n: at most one slot per member
    at += __popcll(bal);
  }
  if (lane == 0) e.work[(size_t)e.B + g] = (double)at;
}

// ---- 2A. replicates of a cell of up to 64 -------------------------------------------------------------------------------
template <int STAT>
__global__ __launch_bounds__(kBootThreads) void umpc_boot_rep_kernel(const BootArgs e) {
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const int lo = __builtin_amdgcn_readfirstlane(e.offset[g]);
  const int nsc = __builtin_amdgcn_readfirstlane((int)e.work[(size_t)e.B + g]);
  if (nsc > 64) return;                                 // the block kernels'
  const int R = e.R, cols = kBootRows + e.q.nq;
  double *reps = e.reps + (size_t)g * R;
  const int stride = (int)gridDim.y * kBootWaves * 64;
  int r0 = ((int)blockIdx.y * kBootWaves + wave) * 64;
  if (nsc == 0) {                                       // nothing is read: NaN replicates, a NaN point estimate
    for (; r0 < R; r0 += stride)
      if (r0 + lane < R) reps[r0 + lane] = __builtin_nan("");
    if (blockIdx.y == 0 && wave == 0 && lane == 0) e.boot[(size_t)g * cols + 2] = __builtin_nan("");
    return;
  }
  const double v = e.work[lo + (lane < nsc ? lane : nsc - 1)];
  const int k = quant_rank(e.stat_p, nsc);
  if (blockIdx.y == 0 && wave == 0) {                   // the point estimate: the statistic of v itself
    double x[1] = {v};
    boot_wave_stat<STAT, 1>(x, nsc, k, lane);
    if (lane == 0) e.boot[(size_t)g * cols + 2] = x[0];
  }
  for (; r0 < R; r0 += stride) {
    const int cnt = R - r0 < 64 ? R - r0 : 64;
    double res = 0.0;
    for (int t = 0; t < cnt; t += 2) {                  // (cnt odd: replicate r0 + cnt is formed and not stored)
      double x[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) x[s] = __shfl(v, boot_index(e.c0, r0 + t + s, lane, nsc));
      boot_wave_stat<STAT, 2>(x, nsc, k, lane);
#pragma unroll
      for (int s = 0; s < 2; ++s) res = lane == t + s ? x[s] : res;
    }
    if (lane < cnt) reps[r0 + lane] = res;
  }
}

// ---- 2B. replicates of a larger cell ------------------------------------------------------------------------------------
// the 256 values of red[] into red[0], a fixed tree; the barrier in front orders the writes of red[] before it
__device__ __forceinline__ double boot_block_sum(double *red, int tid) {
#pragma unroll
  for (int w = kBootThreads / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (tid < w) red[tid] += red[tid + w];
  }
  __syncthreads();
  const double s = red[0];
  __syncthreads();                                      // (red[] is written again by the caller's next row)
  return s;
}

// the sum over the nsc slots of replicate r (IDENT: of v itself) by the block
template <bool IDENT>
__device__ __forceinline__ double boot_block_mean(const double *v, unsigned long long c0, int r, int nsc, int tid, double *red) {
  double acc = 0.0;
  for (int m = tid; m < nsc; m += kBootThreads) acc += v[IDENT ? m : boot_index(c0, r, m, nsc)];
  red[tid] = acc;
  return boot_block_sum(red, tid) / (double)nsc;
}

__global__ __launch_bounds__(kBootThreads) void umpc_boot_mean_block_kernel(const BootArgs e) {
  __shared__ double red[kBootThreads];
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y), tid = wave * 64 + lane;
  const int g = blockIdx.x;
  const int lo = __builtin_amdgcn_readfirstlane(e.offset[g]);
  const int nsc = __builtin_amdgcn_readfirstlane((int)e.work[(size_t)e.B + g]);
  if (nsc <= 64) return;                                // umpc_boot_rep_kernel's
  const double *v = e.work + lo;
  double *reps = e.reps + (size_t)g * e.R;
  if (blockIdx.y == 0) {
    const double t = boot_block_mean<true>(v, e.c0, 0, nsc, tid, red);
    if (tid == 0) e.boot[(size_t)g * (kBootRows + e.q.nq) + 2] = t;
  }
  for (int r = blockIdx.y; r < e.R; r += gridDim.y) {
    const double t = boot_block_mean<false>(v, e.c0, r, nsc, tid, red);
    if (tid == 0) reps[r] = t;
  }
}

struct BootQuantLds {
  QuantLds q;
  double row[2 + kQuantMaxProbs];     // quant_block_row's row: scored, skipped, the order statistics
};

__global__ __launch_bounds__(kBootThreads) void umpc_boot_quantile_block_kernel(const BootArgs e) {
  __shared__ BootQuantLds lds;
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y), tid = wave * 64 + lane;
  const int g = blockIdx.x;
  const int lo = __builtin_amdgcn_readfirstlane(e.offset[g]);
  const int nsc = __builtin_amdgcn_readfirstlane((int)e.work[(size_t)e.B + g]);
  if (nsc <= 64) return;                                // umpc_boot_rep_kernel's
  const double *v = e.work + lo;
  double *reps = e.reps + (size_t)g * e.R;
  const unsigned long long c0 = e.c0;
  if (tid < kQuantMaxProbs) lds.q.p[tid] = e.stat_p;    // one probability: the statistic's (quant_block_init's part)
  if (blockIdx.y == 0) {
    quant_block_row<uint64_t>([&](int m, bool &ok) { ok = true; return quant_image(v[m]); }, nsc, 1, lane, wave, lds.q, lds.row);
    if (tid == 0) e.boot[(size_t)g * (kBootRows + e.q.nq) + 2] = lds.row[2];
  }
  for (int r = blockIdx.y; r < e.R; r += gridDim.y) {
    quant_block_row<uint64_t>([&](int m, bool &ok) { ok = true; return quant_image(v[boot_index(c0, r, m, nsc)]); }, nsc, 1, lane,
                              wave, lds.q, lds.row);
    if (tid == 0) reps[r] = lds.row[2];                 // (behind the row's last barrier; the next row is written three barriers on)
  }
}

// ---- 3. the row of a cell from its R replicates -------------------------------------------------------------------------
// s + e = a + b exactly (Knuth)
__device__ __forceinline__ void boot_two_sum(double a, double b, double &s, double &e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

struct BootRowLds {
  QuantLds q;
  double row[2 + kQuantMaxProbs];
  double hi[kBootThreads], lo[kBootThreads];
};

// the mean of t[0 .. R) and the sum of the squares about it, by the block (also the band kernel's, umpc_band.h, on a row in LDS):
// double-double partial sums, thread-strided, then a fixed tree; then a second pass in plain doubles in the same order
__device__ __forceinline__ void boot_row_moments(const double *t, int R, int tid, BootRowLds &lds, double &mean, double &ss) {
  double hi = 0.0, lo = 0.0;
  for (int r = tid; r < R; r += kBootThreads) {
    double s, err;
    boot_two_sum(hi, t[r], s, err);
    hi = s; lo += err;
  }
  lds.hi[tid] = hi; lds.lo[tid] = lo;
#pragma unroll
  for (int w = kBootThreads / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (tid < w) {
      double s, err;
      boot_two_sum(lds.hi[tid], lds.hi[tid + w], s, err);
      err += lds.lo[tid] + lds.lo[tid + w];
      const double h = s + err;                         // |err| << |s|: Fast2Sum
      lds.hi[tid] = h; lds.lo[tid] = err - (h - s);
    }
  }
  __syncthreads();
  mean = lds.hi[0] / (double)R;
  __syncthreads();
  // their spread about that mean, second pass
  double acc = 0.0;
  for (int r = tid; r < R; r += kBootThreads) { const double d = t[r] - mean; acc += d * d; }
  lds.hi[tid] = acc;
  ss = boot_block_sum(lds.hi, tid);
}

__global__ __launch_bounds__(kBootThreads) void umpc_boot_row_kernel(const BootArgs e) {
  __shared__ BootRowLds lds;
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y), tid = wave * 64 + lane;
  const int g = blockIdx.x;
  const int n = group_window(e.offset, g).n;
  const int nsc = __builtin_amdgcn_readfirstlane((int)e.work[(size_t)e.B + g]);
  const int R = e.R, nq = e.q.nq;
  double *boot = e.boot + (size_t)g * (kBootRows + nq);
  const double *t = e.reps + (size_t)g * R;
  if (tid < 2) boot[tid] = (double)(tid == 0 ? nsc : n - nsc);
  if (nsc == 0) {                                       // (column 2 is the replicate kernel's)
    if (tid >= 3 && tid < kBootRows + nq) boot[tid] = __builtin_nan("");
    return;
  }
  // the percentile interval: nearest-rank elements of the R replicates
  quant_block_init(e.q, tid, lds.q);
  quant_block_row<uint64_t>([&](int r, bool &ok) { ok = true; return quant_image(t[r]); }, R, nq, lane, wave, lds.q, lds.row);
  if (tid < nq) boot[kBootRows + tid] = lds.row[2 + tid];
  // their mean and their spread about it
  double mean, ss;
  boot_row_moments(t, R, tid, lds, mean, ss);
  if (tid == 0) { boot[3] = mean; boot[4] = __builtin_sqrt(ss / (double)(R - 1)); }
}

}  // namespace umpc
