// Ensemble quantiles of recorded rollouts (umpcBatchEnsembleQuantiles / umpcBatchScoreQuantiles, include/umpc_mi355x.h): the
// order statistics of a group of robots (the draws of one grid cell of a sweep) -- per step over a term of the scoring
// kernel (e_p, e_s or the clipped moments squared), or once over a per-robot score. The median curve with a percentile band
// is what a Monte-Carlo study draws and what the rows of umpc_ensemble.h cannot give: one diverged draw owns the mean and the
// maximum of its cell, it moves a median by one rank. The answer is an ELEMENT of the cell (nearest rank, no interpolation):
// v[k], k = min(n - 1, max(0, ceil(p n) - 1)), over the n scored members in ascending order. It depends on the member set
// alone, so there is no order of evaluation to fix and nothing to round.
//
// Keys. A value travels as its order-preserving unsigned image (sign bit flipped for x >= 0, all bits for x < 0: the total
// order of the values is the order of the unsigned integers, -0 < +0), 32 bits in fp32 and 64 in fp64 (two dwords in every
// cross-lane move). A member that is not scored, and a lane without a member, carries the all-ones key: the image of a NaN,
// which no scored value has, so the n scored keys are the first n of the sorted order.
//
// Grid as in the ensemble kernel: one block per (group, slice of the step range), blockDim (64, kQuantWaves); the loader
// score_load and the expressions score_terms of umpc_score.h are used as they are, so a member is scored exactly when the
// ensemble kernel scores it and its term has the same bits. The path is chosen per block from n = offset[g + 1] - offset[g]:
// the two paths are two kernels launched one behind the other on that grid, and a block leaves the one that is not its own.
//
// A. n <= 64 (cell = b // 64, INTEGRATION.md: the fast case). A WAVEFRONT owns whole steps, two per trip, the loads of both
// issued before the first word is used. Lane l holds member l's key and the 64 keys are sorted IN REGISTERS by a bitonic
// network of 21 compare-exchange stages in its one-direction form: runs of k / 2 ascending keys are merged by comparing lane
// with lane ^ (k - 1) first (the second run read backwards), then with lane ^ j, j = k / 4, .., 1, and in every stage the lower
// lane of a pair keeps the smaller key. The partner's key comes by DPP in 18 stages (quad_perm for ^1, ^2, ^3,
// row_half_mirror for ^7, row_mirror for ^15, row_ror:8 for ^8, and ^4 as row_half_mirror then quad_perm [3,2,1,0]), by
// ds_swizzle in bit mode for ^31 and ^16 (the LDS crossbar, no LDS memory) and by one ds_bpermute for ^63. (The form has no
// stride-32 stage, which v_permlane32_swap would serve: lane ^ 63 swaps the halves AND mirrors them.) A stage is one
// unsigned compare, one scalar xor and one select per dword: the lane keeps its own key when (own < partner) equals "this
// lane keeps the smaller", one of six lane masks that leave the step loop. No LDS allocation, no barrier, no scratch. After
// the sort lane k holds v[k]: lane 2 + j forms its own rank from probs[j] and the ballot count n and fetches v[k] with one
// ds_bpermute per dword; lanes 0 .. 1 + nq store the row. Rank counting (each lane counts the keys below its own against 64
// v_readlane broadcasts) was the other candidate: 64 x (readlane, compare, add-with-carry) is at least 192 instructions per
// dword-key against 21 x 3 + 5 here, and it needs a tie-break on top. The network it is.
// Measured (profiles/quantile_timing.txt; B = 65 536 as 1 024 cells of 64, 200 steps, fp32, seven probabilities): 0.161 ms =
// 4.7 TB/s over the algorithmic bytes, 10.6x faster than e_p and a sort in torch, 0.51x the ensemble kernel's time.
//
// B. n > 64: correct for any n, not tuned. The block's four wavefronts take one step at a time and select by radix, most
// significant digit first, 8 bits per pass (4 passes in fp32, 8 in fp64) on the same unsigned image. Pass 0 has one
// histogram (no prefix yet; its total is n scored, which fixes the ranks); every later pass has one histogram of 256
// integer counters per requested rank, because the prefixes differ from the first digit on. Counters are integer LDS adds;
// then wavefront w scans the histograms of ranks w, w + 4: four counters per lane, a fixed shuffle scan, and the one lane
// whose interval holds the rank appends its digit to the prefix. The keys are formed again from the tables on every pass
// (the terms are deterministic), so LDS does not grow with n: 8 x 256 x 4 B + 168 B.
//
// umpcBatchScoreQuantiles runs the same two routines on double keys (score[num][b], or the IEEE quotient score[num][b] /
// score[den][b]): one block per group, its first wavefront alone when n <= 64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_score.h"

namespace umpc {

constexpr int kQuantMaxProbs = 8;
constexpr int kQuantWaves = 4;      // wavefronts per block: they share nothing on path A, one step at a time on path B
constexpr int kQuantThreads = 64 * kQuantWaves;
constexpr int kQuantBins = 256;     // one radix digit of path B

struct QuantProbs {
  double p[kQuantMaxProbs];
  int nq;
};

template <typename T>
struct QuantArgs {
  ScoreArgs<T> t;         // the tables as the scoring kernel reads them (score, status, tol2 unused); t.count = steps
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  double *quant;          // [count][G][2 + nq]
  int G;
  QuantProbs q;
};

template <typename T>
struct ScoreQuantArgs {
  const T *score;         // [12][B]
  const int32_t *order, *offset;
  double *quant;          // [G][2 + nq]
  int B, num, den;
  QuantProbs q;
};

struct QuantLds {
  int hist[kQuantMaxProbs][kQuantBins];
  unsigned long long prefix[kQuantMaxProbs];
  double p[kQuantMaxProbs];       // probs, parked once per block: path B's loop holds no launch argument it can do without
  int r[kQuantMaxProbs];
  int nsc;
};

__device__ __forceinline__ uint32_t quant_image(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ uint64_t quant_image(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ float quant_value(uint32_t u) { return __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u); }
__device__ __forceinline__ double quant_value(uint64_t u) {
  return __longlong_as_double((long long)((u >> 63) ? u ^ 0x8000000000000000ull : ~u));
}

// k of the order statistic for probability p among n >= 1 values: one IEEE double multiply
__device__ __forceinline__ int quant_rank(double p, int n) {
  int k = (int)__builtin_ceil(p * (double)n) - 1;       // (0 <= p <= 1: the product is at most n, an int)
  k = k < 0 ? 0 : k;
  return k > n - 1 ? n - 1 : k;
}

// probs[j] for a j that is not a compile-time constant: selects over the launch arguments, no indexed copy of them
__device__ __forceinline__ double quant_prob(const QuantProbs &q, int j) {
  double p = 0.0;
#pragma unroll
  for (int i = 0; i < kQuantMaxProbs; ++i) p = j == i ? q.p[i] : p;
  return p;
}

// before the first quant_block_row of a block (its first barrier orders these writes before their first use)
__device__ __forceinline__ void quant_block_init(const QuantProbs &q, int tid, QuantLds &l) {
  if (tid < kQuantMaxProbs) l.p[tid] = quant_prob(q, tid);
}

// the dword of lane ^ x for the 11 patterns of the network: x = 1, 2, 4, 8, 16 (a butterfly inside a sorted-pair merge) and
// x = 3, 7, 15, 31, 63 (the mirror that opens the merge of two ascending runs of 2, 4, .., 32)
__device__ __forceinline__ uint32_t quant_xor_lane(uint32_t x, int pattern) {
  const int v = (int)x;
  switch (pattern) {
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);      // quad_perm:[1,0,3,2]
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);      // quad_perm:[2,3,0,1]
    case 3: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x1B, 0xF, 0xF, true);      // quad_perm:[3,2,1,0]
    case 4: {
      const int m = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);              // row_half_mirror: l ^ 7
      return (uint32_t)__builtin_amdgcn_update_dpp(0, m, 0x1B, 0xF, 0xF, true);            // quad_perm:[3,2,1,0]: ^ 3
    }
    case 7: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);     // row_half_mirror
    case 8: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, true);     // row_ror:8
    case 15: return (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);    // row_mirror
    case 16: return (uint32_t)__builtin_amdgcn_ds_swizzle(v, 0x401F);                      // bit mode: and 0x1f, xor 0x10
    case 31: return (uint32_t)__builtin_amdgcn_ds_swizzle(v, 0x7C1F);                      // bit mode: and 0x1f, xor 0x1f
    default: return (uint32_t)__shfl_xor(v, 63);                                           // across the halves: ds_bpermute
  }
}
__device__ __forceinline__ uint32_t quant_partner(uint32_t x, int pattern) { return quant_xor_lane(x, pattern); }
__device__ __forceinline__ uint64_t quant_partner(uint64_t x, int pattern) {
  return ((uint64_t)quant_xor_lane((uint32_t)(x >> 32), pattern) << 32) | quant_xor_lane((uint32_t)x, pattern);
}
__device__ __forceinline__ uint32_t quant_from_lane(uint32_t x, int k) { return (uint32_t)__shfl((int)x, k); }
__device__ __forceinline__ uint64_t quant_from_lane(uint64_t x, int k) {
  return ((uint64_t)quant_from_lane((uint32_t)(x >> 32), k) << 32) | quant_from_lane((uint32_t)x, k);
}

// The 64 keys of a wavefront in ascending order of the lane: the bitonic network in its one-direction form, 21 stages.
// Runs of k / 2 ascending keys are merged into runs of k: the first stage compares lane with lane ^ (k - 1) (the second run
// read backwards), the others lane with lane ^ j, j = k / 4, .., 1. In every stage the lower lane of a pair keeps the smaller
// key, so which lanes keep the smaller is one of SIX masks (bit log2 j or log2 (k / 2) of the lane is clear).
// NS independent sets of keys go through the network together: a stage of one fills the wait states of the other's DPP reads.
template <typename U, int NS>
__device__ __forceinline__ void quant_sort64(U (&x)[NS], int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const bool keep_min = (lane & j) == 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const U b = quant_partner(x[s], j == (k >> 1) ? k - 1 : j);
        x[s] = ((x[s] < b) == keep_min) ? x[s] : b;
      }
    }
  }
}

// one row from the SORTED keys of a wavefront: nsc = scored keys among them (the others are all-ones), n = members of the
// group, p = probs[lane - 2] in lanes 2 .. 1 + nq
template <typename U>
__device__ __forceinline__ void quant_wave_row(U key, int nsc, int n, double p, int nq, int lane, double *row) {
  const U sel = quant_from_lane(key, quant_rank(p, nsc > 0 ? nsc : 1));
  // (selects on purpose: a chain of lane tests over three conversions becomes a switch with branches)
  const double cnt = (double)(lane == 0 ? nsc : n - nsc), val = (double)quant_value(sel);
  const bool head = lane < 2, none = nsc == 0;
  const double v = head ? cnt : none ? __builtin_nan("") : val;
  if (lane < 2 + nq) row[lane] = v;
}

// Path B. keyof(m, ok): the key of member m of the group and whether it is scored; called once per pass.
template <typename U, typename F>
__device__ __forceinline__ void quant_block_row(F keyof, int n, int nq, int lane, int wave, QuantLds &l, double *row) {
  constexpr int kPasses = (int)sizeof(U);
  const int tid = wave * 64 + lane;
  U prefix[kQuantMaxProbs];
#pragma unroll
  for (int j = 0; j < kQuantMaxProbs; ++j) prefix[j] = 0;
  int nsc = 0;
  for (int pass = 0; pass < kPasses; ++pass) {
    const int shift = 8 * (kPasses - 1 - pass);
    const int nh = pass == 0 ? 1 : nq;
    for (int j = 0; j < nh; ++j) l.hist[j][tid] = 0;
    __syncthreads();
    for (int m = tid; m < n; m += kQuantThreads) {
      bool ok;
      const U u = keyof(m, ok);
      if (ok) {
        const U low = u >> shift;
        const int d = (int)(low & 255);
        if (pass == 0) {
          atomicAdd(&l.hist[0][d], 1);
        } else {
          const U hi = low >> 8;
#pragma unroll
          for (int j = 0; j < kQuantMaxProbs; ++j)
            if (j < nq && hi == prefix[j]) atomicAdd(&l.hist[j][d], 1);
        }
      }
    }
    __syncthreads();
    for (int j = wave; j < nq; j += kQuantWaves) {
      const int *h = l.hist[pass == 0 ? 0 : j] + 4 * lane;
      const int c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
      const int s = (c0 + c1) + (c2 + c3);
      int incl = s;
#pragma unroll
      for (int w = 1; w < 64; w <<= 1) { const int o = __shfl_up(incl, w); incl += lane >= w ? o : 0; }
      const int total = __shfl(incl, 63);
      const U old = pass == 0 ? U(0) : (U)l.prefix[j];
      const int r = pass == 0 ? (total > 0 ? quant_rank(l.p[j], total) : -1) : l.r[j];
      if (pass == 0 && j == 0 && lane == 0) l.nsc = total;
      const int excl = incl - s;
      if (r >= excl && r < incl) {                      // one lane
        int rr = r - excl, d = 0;
        if (rr >= c0) { rr -= c0; d = 1; if (rr >= c1) { rr -= c1; d = 2; if (rr >= c2) { rr -= c2; d = 3; } } }
        l.prefix[j] = (unsigned long long)((old << 8) | (U)(4 * lane + d));
        l.r[j] = rr;
      }
    }
    __syncthreads();
    nsc = l.nsc;
    if (nsc == 0) break;                                // (the same in every thread of the block)
#pragma unroll
    for (int j = 0; j < kQuantMaxProbs; ++j)
      if (j < nq) prefix[j] = (U)l.prefix[j];
  }
  if (tid < 2 + nq) {
    double v = tid == 0 ? (double)nsc : (double)(n - nsc);
    if (tid >= 2) v = nsc > 0 ? (double)quant_value((U)l.prefix[tid - 2]) : __builtin_nan("");
    row[tid] = v;
  }
  __syncthreads();                                      // the next row's first pass writes what this one has just read
}

template <typename T>
using QuantKeyOf = decltype(quant_image(T(0)));

// (a template parameter: a run-time choice among the three members makes hipcc index the struct in private memory)
template <int TERM, typename T>
__device__ __forceinline__ T quant_term(const ScoreTerms<T> &t) {
  return TERM == 0 ? t.ep : TERM == 1 ? t.es : t.tt;
}

// NS steps (i, i + stride, ..) of one group of n <= 64 members by one wavefront: the loads of all NS before the first use
template <typename T, bool TAB, bool OUT, int TERM, int NS>
__device__ __forceinline__ void quant_steps(const QuantArgs<T> &e, int n, int b, const T (&rc)[6], double p, int lane, int g,
                                            long long i, long long stride) {
  using U = QuantKeyOf<T>;
  const size_t B = (size_t)e.t.B;
  const int cols = 2 + e.q.nq;
  // the member is the same at every step: its column is added to the table pointers once, here (loop-invariant, in vector
  // registers), and score_load is called for column 0, lane 0 -- what stays scalar per load is the row offset alone
  ScoreArgs<T> a = e.t;
  a.state += b;
  if (TAB) a.reftab += b;
  if (OUT) a.out += b;
  ScoreStep<T> v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) score_load<T, false, TAB, OUT, false>(a, B, 0, 0u, i + s * stride, rc, v[s]);
  __builtin_amdgcn_sched_barrier(0);      // (or the scheduler sinks the second step's loads below the first step's sort)
  U key[NS];
  int nsc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const ScoreTerms<T> t = score_terms(a.taulim, v[s]);
    const bool ok = (lane < n) & t.ok;
    key[s] = ok ? quant_image(quant_term<TERM>(t)) : ~U(0);
    nsc[s] = __popcll(__ballot(ok));
  }
  quant_sort64(key, lane);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    quant_wave_row<U>(key[s], nsc[s], n, p, e.q.nq, lane, e.quant + ((size_t)(i + s * stride) * e.G + g) * cols);
}

// the key of member m of a group at step i, for path B: formed from the tables on every call
template <typename T, bool TAB, bool OUT, int TERM>
struct QuantStepKey {
  const ScoreArgs<T> &a;
  const int32_t *mem;
  long long i;
  __device__ __forceinline__ QuantKeyOf<T> operator()(int m, bool &ok) const {
    const size_t B = (size_t)a.B;
    const int b = mem[m];
    T rc[6];
    score_const_ref<T, TAB>(a, B, b, rc);
    ScoreStep<T> v;
    score_load<T, false, TAB, OUT, false>(a, B, 0, (unsigned)b, i, rc, v);
    const ScoreTerms<T> t = score_terms(a.taulim, v);
    ok = t.ok;
    return quant_image(quant_term<TERM>(t));
  }
};

// path B of the ensemble-quantile kernel: the steps blockIdx.y, + gridDim.y, .. of one group of n > 64 members by the block
template <typename T, bool TAB, bool OUT, int TERM>
__device__ __forceinline__ void quant_block_steps(const QuantArgs<T> &e, const int32_t *mem, int n, int g, int lane, int wave,
                                                  QuantLds &lds) {
  const int cols = 2 + e.q.nq;
  quant_block_init(e.q, wave * 64 + lane, lds);
  for (long long i = blockIdx.y; i < e.t.count; i += gridDim.y)
    quant_block_row<QuantKeyOf<T>>(QuantStepKey<T, TAB, OUT, TERM>{e.t, mem, i}, n, e.q.nq, lane, wave, lds,
                                   e.quant + ((size_t)i * e.G + g) * cols);
}

// Path B as a kernel of its own, launched behind the path A kernel on the same grid: a block whose group has n <= 64 leaves
// at once here, a block whose group has n > 64 leaves at once there. (One kernel with both paths holds path B's launch
// arguments in scalar registers across path A's loop: 40 scalar spills in the hot loop and a private frame in three forms.)
template <typename T, bool TAB, bool OUT, int TERM>
__global__ __launch_bounds__(kQuantThreads) void umpc_ens_quantile_block_kernel(const QuantArgs<T> e) {
  __shared__ QuantLds lds;
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  if (n <= 64) return;
  quant_block_steps<T, TAB, OUT, TERM>(e, e.order + lo, n, g, lane, wave, lds);
}

template <typename T, bool TAB, bool OUT, int TERM>
__global__ __launch_bounds__(kQuantThreads) void umpc_ens_quantile_kernel(const QuantArgs<T> e) {
  // (blockDim = (64, kQuantWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  if (n > 64) return;                                   // umpc_ens_quantile_block_kernel's
  const long long count = e.t.count;
  const int32_t *mem = e.order + lo;
  const int cols = 2 + e.q.nq;
  const ScoreArgs<T> &a = e.t;
  const size_t B = (size_t)a.B;
  const long long stride = (long long)gridDim.y * kQuantWaves;
  long long i = (long long)blockIdx.y * kQuantWaves + wave;
  if (n == 0) {                                         // nothing is read: n = 0, skipped = 0, NaN
    for (; i < count; i += stride)
      if (lane < cols) e.quant[((size_t)i * e.G + g) * cols + lane] = lane < 2 ? 0.0 : __builtin_nan("");
    return;
  }
  // a lane past the end of the list reads the last member again (a valid address, an L1 hit) and carries the largest key
  const int b = mem[lane < n ? lane : n - 1];
  T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  if (!TAB) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { rc[j] = a.ref[(size_t)j * B + b]; rc[3 + j] = a.ref[(size_t)(6 + j) * B + b]; }
  }
  const double p = quant_prob(e.q, lane - 2);
  for (; i + stride < count; i += 2 * stride) quant_steps<T, TAB, OUT, TERM, 2>(e, n, b, rc, p, lane, g, i, stride);
  if (i < count) quant_steps<T, TAB, OUT, TERM, 1>(e, n, b, rc, p, lane, g, i, stride);
}

// the value of robot b in a score table, score[num][b] or the IEEE double quotient score[num][b] / score[den][b], and whether
// the robot has one (the rule of umpcBatchScoreGroups: row 0 > 0)
template <typename T>
__device__ __forceinline__ double score_table_value(const T *score, size_t B, int num, int den, int b, bool &ok) {
  const T n0 = score[b];
  double x = (double)score[(size_t)num * B + b];
  if (den >= 0) x = x / (double)score[(size_t)den * B + b];
  ok = n0 > T(0);
  return x;
}
// for umpcBatchScoreQuantiles: it enters when it is finite, too
template <typename T>
__device__ __forceinline__ double quant_score_value(const ScoreQuantArgs<T> &e, int b, bool &ok) {
  const double x = score_table_value(e.score, (size_t)e.B, e.num, e.den, b, ok);
  ok = ok & __builtin_isfinite(x);
  return x;
}

template <typename T>
__global__ __launch_bounds__(kQuantThreads) void umpc_score_quantile_kernel(const ScoreQuantArgs<T> e) {
  __shared__ QuantLds lds;
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  const int32_t *mem = e.order + lo;
  double *row = e.quant + (size_t)g * (2 + e.q.nq);
  if (n > 64) {
    auto keyof = [&](int m, bool &ok) { return quant_image(quant_score_value(e, mem[m], ok)); };
    quant_block_init(e.q, wave * 64 + lane, lds);
    quant_block_row<uint64_t>(keyof, n, e.q.nq, lane, wave, lds, row);
    return;
  }
  if (wave != 0) return;
  bool ok = false;
  double x = 0.0;
  if (lane < n) x = quant_score_value(e, mem[lane], ok);
  uint64_t key[1] = {ok ? quant_image(x) : ~0ull};
  quant_sort64(key, lane);
  quant_wave_row<uint64_t>(key[0], __popcll(__ballot(ok)), n, quant_prob(e.q, lane - 2), e.q.nq, lane, row);
}

}  // namespace umpc
