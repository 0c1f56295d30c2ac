// Scoring of recorded rollouts (umpcBatchScore / umpcBatchScoreGroups, include/umpc_mi355x.h): the last stage of a sweep.
// A step history [steps+1][18][B] + [steps][9][B] + [steps][B] and a reference table [steps][9][B] go in, a score
// [12][B] per robot and a table [G][8] per group of robots (a grid cell of a gain sweep) come out.
//
// Scoring kernel. One lane per robot, robot index fastest: every load of a wavefront is one coalesced row segment
// (256 B in fp32). A step reads 15 of the 37 words it recorded (state rows 0..2 and 9..11, reference rows 0..2 and 6..8, out
// rows 1..2, the status), 60 B per robot-step in fp32, each exactly once: the kernel is a pure stream with ~40 flops per
// 60 B, far under the machine balance, so all that matters is the number of loads in flight. B = 65 536 is 1 024 blocks of
// 64 robots -- one wavefront per SIMD if a block were one wavefront, i.e. one step's 15 loads (3.8 KB) in flight per SIMD
// against an HBM miss of ~900 cycles. So a block of 64 robots is kScoreSlices = 8 wavefronts: slice s takes steps s, s + 8,
// s + 16, .. of the call (the 8 wavefronts of a block read 8 ADJACENT table slices at any time), two steps per trip. Which
// tables there are (reference table or constant, out, status) is a template parameter, chosen once on the host, and the
// accumulation is written with selects instead of branches: the compiled loop body is straight-line code -- all 30 loads
// of a trip (28 / 26 / 24 / .. without a record) are issued first, then counted waits vmcnt(29), vmcnt(28), .. as the words
// are used (checked in the ISA; with run-time null tests or `&&` chains hipcc branches around loads and drains the queue
// several times per trip). fp32: 101 VGPRs, 4 wavefronts per SIMD = 2 blocks = 16 wavefronts per CU, each with up to
// 30 x 256 B requested; fp64: 154 VGPRs, one block per CU, the same bytes. Measured (profiles/score_timing.txt): 4.4 TB/s, 5.5 with nt loads. The table
// step and the block's first robot are wave-uniform (readfirstlane of threadIdx.y); hipcc nevertheless forms most addresses
// as 64-bit vector adds (global_load_dword v, v[a:b], off), one v_lshl_add_u64 per load -- ALU work the kernel has to spare.
// The slices meet once, in LDS: slices 1..7 park their 13 partial values per robot, slice 0 adds them in
// the fixed order 1, 2, .., 7 and folds the total into `score`. Nothing crosses robots and the slice count is a constant,
// so a robot's result depends on its own columns and on (count) alone: a block of a sharded job equals the same columns of
// the undivided batch bit for bit, and two runs are equal bit for bit. No atomics, no temporaries, one pass.
// Counts, maxima, "last" and the first / last step over the threshold do not depend on the order of summation and are the
// same however a step range is cut into calls; the four sum rows are sums of non-negative terms in an order that depends
// on the cut (relative difference <= (steps + 8) u).
//
// Group kernel. One workgroup per group scans group[] in a fixed stride; each thread folds its robots in index order into
// fp64 partials, then a fixed-shape LDS tree over the 256 threads: bit-reproducible, no floating-point atomics. G x B id
// reads (served by L2 after the first group), which is nothing next to the history the score came from.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_scalar.h"

namespace umpc {

constexpr int kScoreRows = 12, kGScoreRows = 8;
constexpr int kScoreSlices = 8;     // wavefronts per block of 64 robots = ways a call's step range is split
constexpr int kScoreNF = 7, kScoreNI = 6;   // floating-point / integer partial values per robot and slice

// pointers as the kernel reads them: the host has moved them to the first slice of the call (state: slice first + after)
template <typename T>
struct ScoreArgs {
  const T *state;         // [..][18][B]
  const T *out;           // [..][9][B] or null
  const int32_t *status;  // [..][B] or null
  const T *reftab;        // [..][9][B] or null
  const T *ref;           // [9][B], read when reftab is null
  T *score;               // [12][B] in/out
  int B, count;
  long long step0;
  T tol2, taulim;
};

template <typename T>
struct ScoreStep {
  T p[3], s[3], rp[3], rs[3], tau[2];
  int32_t st;
};

template <typename T>
struct ScorePart {
  T sum_ep = T(0), max_ep = T(0), last_ep = T(0), sum_es = T(0), max_es = T(0), sum_tau = T(0), sum_p2 = T(0);
  int n = 0, nbad = 0, nskip = 0, ilast = -1, ifirst_over = -1, ilast_over = -1;   // i = step index inside the call
};

template <bool NT, typename V>
__device__ __forceinline__ V score_ld(const V *p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}

// col = the block's first robot, the same in every lane, i = the wavefront's step. Which tables there are is a template
// parameter, so the loads of a step are straight-line code: nothing branches around a load, nothing waits between them.
template <typename T, bool NT, bool TAB, bool OUT, bool STAT>
__device__ __forceinline__ void score_load(const ScoreArgs<T> &a, size_t B, size_t col, unsigned lane, long long i,
                                           const T (&rc)[6], ScoreStep<T> &v) {
  const T *st = a.state + ((size_t)i * 18 * B + col);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    v.p[j] = score_ld<NT>(st + (size_t)j * B + lane);
    v.s[j] = score_ld<NT>(st + (size_t)(9 + j) * B + lane);
  }
  if (TAB) {
    const T *r = a.reftab + ((size_t)i * 9 * B + col);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v.rp[j] = score_ld<NT>(r + (size_t)j * B + lane);
      v.rs[j] = score_ld<NT>(r + (size_t)(6 + j) * B + lane);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) { v.rp[j] = rc[j]; v.rs[j] = rc[3 + j]; }
  }
  if (OUT) {
    const T *o = a.out + ((size_t)i * 9 * B + col);
    v.tau[0] = score_ld<NT>(o + B + lane);
    v.tau[1] = score_ld<NT>(o + 2 * B + lane);
  } else {
    v.tau[0] = v.tau[1] = T(0);
  }
  v.st = STAT ? score_ld<NT>(a.status + ((size_t)i * B + col) + lane) : 1;
}

// rc = the six words robot b reads of a constant reference (rows 0..2 and 6..8), fetched once per robot; zeros, and never
// read, with a reference table. (ens_steps and umpc_ens_quantile_kernel keep these lines written out: with the call hipcc
// allocates their scalar registers in another order.)
template <typename T, bool TAB, typename I>
__device__ __forceinline__ void score_const_ref(const ScoreArgs<T> &a, size_t B, I b, T (&rc)[6]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) { rc[j] = TAB ? T(0) : a.ref[(size_t)j * B + b]; rc[3 + j] = TAB ? T(0) : a.ref[(size_t)(6 + j) * B + b]; }
}

// the members of group g are order[lo .. lo + n): the same in every lane, said to the compiler
struct GroupWindow { int lo, n; };
__device__ __forceinline__ GroupWindow group_window(const int32_t *offset, int g) {
  const int lo = __builtin_amdgcn_readfirstlane(offset[g]);
  return {lo, __builtin_amdgcn_readfirstlane(offset[g + 1]) - lo};
}

// what one robot-step contributes, in the dtype: the one place these expressions are written (the scoring kernel folds them
// over the steps of a robot, the ensemble kernel of umpc_ensemble.h over the robots of a step)
template <typename T>
struct ScoreTerms {
  bool ok;              // every word the step read is finite
  T d[3], ep, es, p2, tt;
};

// Branch-free on purpose: `&` instead of `&&` and selects instead of an `if (ok)` body. With short-circuit tests the
// compiler sinks the loads of the later words into the branches of the earlier tests, and a step's loads are then issued
// and waited for a few at a time.
template <typename T>
__device__ __forceinline__ ScoreTerms<T> score_terms(T taulim, const ScoreStep<T> &v) {
  ScoreTerms<T> t;
  bool ok = __builtin_isfinite(v.tau[0]) & __builtin_isfinite(v.tau[1]);   // (zeros without an out table)
#pragma unroll
  for (int j = 0; j < 3; ++j)
    ok = ok & __builtin_isfinite(v.p[j]) & __builtin_isfinite(v.s[j]) & __builtin_isfinite(v.rp[j]) & __builtin_isfinite(v.rs[j]);
  t.ok = ok;
  const T d0 = v.p[0] - v.rp[0], d1 = v.p[1] - v.rp[1], d2 = v.p[2] - v.rp[2];
  t.d[0] = d0; t.d[1] = d1; t.d[2] = d2;
  t.ep = (d0 * d0 + d1 * d1) + d2 * d2;
  const T c0 = v.s[0] - v.rs[0], c1 = v.s[1] - v.rs[1], c2 = v.s[2] - v.rs[2];
  t.es = (c0 * c0 + c1 * c1) + c2 * c2;
  t.p2 = (v.p[0] * v.p[0] + v.p[1] * v.p[1]) + v.p[2] * v.p[2];
  // the moments as the plant saw them (closed_loop_step clips them at +-taulim before the substeps)
  const T t1 = umpc_min(umpc_max(v.tau[0], -taulim), taulim), t2 = umpc_min(umpc_max(v.tau[1], -taulim), taulim);
  t.tt = t1 * t1 + t2 * t2;
  return t;
}

template <typename T>
__device__ __forceinline__ void score_step(const ScoreArgs<T> &a, int i, const ScoreStep<T> &v, ScorePart<T> &q) {
  const ScoreTerms<T> t = score_terms(a.taulim, v);
  const bool ok = t.ok;
  const T ep = t.ep, es = t.es, p2 = t.p2, tt = t.tt;
  const bool over = ok & (ep > a.tol2);
  // a skipped step adds +0 to sums of non-negative terms and takes no part in a max of non-negative terms: no rounding
  q.n += ok; q.nskip += !ok;
  q.sum_ep += ok ? ep : T(0); q.max_ep = umpc_max(q.max_ep, ok ? ep : T(0));
  q.last_ep = ok ? ep : q.last_ep; q.ilast = ok ? i : q.ilast;
  q.sum_es += ok ? es : T(0); q.max_es = umpc_max(q.max_es, ok ? es : T(0));
  q.sum_tau += ok ? tt : T(0); q.sum_p2 += ok ? p2 : T(0);
  q.nbad += ok & (v.st != 1);
  q.ifirst_over = (over & (q.ifirst_over < 0)) ? i : q.ifirst_over;
  q.ilast_over = over ? i : q.ilast_over;
}

template <typename T, bool NT, bool TAB, bool OUT, bool STAT>
__global__ __launch_bounds__(64 * kScoreSlices, sizeof(T) == 4 ? 4 : 2) void umpc_score_kernel(const ScoreArgs<T> a) {
  __shared__ T ldsf[kScoreSlices - 1][kScoreNF][64];
  __shared__ int ldsi[kScoreSlices - 1][kScoreNI][64];
  // (blockDim = (64, kScoreSlices): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const size_t B = (size_t)a.B, col = (size_t)blockIdx.x * 64, b = col + lane;
  const bool live = b < B;                 // (a lane past the batch loads nothing, but meets the barrier)
  ScorePart<T> q;
  if (live) {
    T rc[6];
    score_const_ref<T, TAB>(a, B, b, rc);
    // two steps per trip: the loads of both are issued before the first is used
    int i = slice;                         // (count <= 2^31 - 1 - 2 kScoreSlices, umpcBatchScore: no sum here wraps)
    for (; i + kScoreSlices < a.count; i += 2 * kScoreSlices) {
      ScoreStep<T> v0, v1;
      score_load<T, NT, TAB, OUT, STAT>(a, B, col, (unsigned)lane, i, rc, v0);
      score_load<T, NT, TAB, OUT, STAT>(a, B, col, (unsigned)lane, i + kScoreSlices, rc, v1);
      score_step(a, i, v0, q);
      score_step(a, i + kScoreSlices, v1, q);
    }
    if (i < a.count) {
      ScoreStep<T> v0;
      score_load<T, NT, TAB, OUT, STAT>(a, B, col, (unsigned)lane, i, rc, v0);
      score_step(a, i, v0, q);
    }
  }
  if (slice > 0) {
    T(*f)[64] = ldsf[slice - 1];
    int(*n)[64] = ldsi[slice - 1];
    f[0][lane] = q.sum_ep; f[1][lane] = q.max_ep; f[2][lane] = q.last_ep; f[3][lane] = q.sum_es; f[4][lane] = q.max_es;
    f[5][lane] = q.sum_tau; f[6][lane] = q.sum_p2;
    n[0][lane] = q.n; n[1][lane] = q.nbad; n[2][lane] = q.nskip; n[3][lane] = q.ilast; n[4][lane] = q.ifirst_over;
    n[5][lane] = q.ilast_over;
  }
  __syncthreads();
  if (slice > 0 || !live) return;
  // the slices in the fixed order 0, 1, .., 7
#pragma unroll
  for (int s = 0; s < kScoreSlices - 1; ++s) {
    const T(*f)[64] = ldsf[s];
    const int(*n)[64] = ldsi[s];
    q.sum_ep += f[0][lane]; q.max_ep = umpc_max(q.max_ep, f[1][lane]);
    q.sum_es += f[3][lane]; q.max_es = umpc_max(q.max_es, f[4][lane]);
    q.sum_tau += f[5][lane]; q.sum_p2 += f[6][lane];
    q.n += n[0][lane]; q.nbad += n[1][lane]; q.nskip += n[2][lane];
    if (n[3][lane] > q.ilast) { q.ilast = n[3][lane]; q.last_ep = f[2][lane]; }
    const int fo = n[4][lane], lo = n[5][lane];
    if (fo >= 0 && (q.ifirst_over < 0 || fo < q.ifirst_over)) q.ifirst_over = fo;
    if (lo > q.ilast_over) q.ilast_over = lo;
  }
  T *sc = a.score + b;
  sc[0] += T(q.n);
  sc[1 * B] += q.sum_ep;
  sc[2 * B] = umpc_max(sc[2 * B], q.max_ep);
  if (q.ilast >= 0) sc[3 * B] = q.last_ep;
  sc[4 * B] += q.sum_es;
  sc[5 * B] = umpc_max(sc[5 * B], q.max_es);
  if (OUT) sc[6 * B] += q.sum_tau;
  sc[7 * B] += q.sum_p2;
  if (STAT) sc[8 * B] += T(q.nbad);
  if (q.ifirst_over >= 0) {
    const T kf = T(a.step0 + q.ifirst_over), kl = T(a.step0 + q.ilast_over);
    const T of = sc[9 * B];
    sc[9 * B] = of < T(0) ? kf : umpc_min(of, kf);
    sc[10 * B] = umpc_max(sc[10 * B], kl);
  }
  sc[11 * B] += T(q.nskip);
}

template <typename T>
__global__ __launch_bounds__(256) void umpc_score_init_kernel(T *score, int B_) {
  const size_t B = (size_t)B_, b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
#pragma unroll
  for (int r = 0; r < kScoreRows; ++r) score[(size_t)r * B + b] = (r == 9 || r == 10) ? T(-1) : T(0);
}

template <typename T>
__global__ __launch_bounds__(256) void umpc_score_groups_kernel(const T *score, const int32_t *group, int B_, double *gstat) {
  __shared__ double red[kGScoreRows][256];
  const int g = blockIdx.x, tid = threadIdx.x;
  const size_t B = (size_t)B_;
  double acc[kGScoreRows] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t b = tid; b < B; b += 256) {
    if (group[b] != g) continue;
    const double n = (double)score[b];
    acc[0] += 1.0;
    if (n > 0) {
      acc[1] += 1.0;
      acc[2] += (double)score[1 * B + b] / n;
      acc[3] = umpc_max(acc[3], (double)score[2 * B + b]);
      acc[4] += (double)score[6 * B + b] / n;
      acc[5] += (double)score[7 * B + b] / n;
    }
    if (score[9 * B + b] >= T(0)) acc[6] += 1.0;
    acc[7] += (double)score[8 * B + b];
  }
#pragma unroll
  for (int r = 0; r < kGScoreRows; ++r) red[r][tid] = acc[r];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int r = 0; r < kGScoreRows; ++r)
        red[r][tid] = r == 3 ? umpc_max(red[r][tid], red[r][tid + w]) : red[r][tid] + red[r][tid + w];
    }
    __syncthreads();
  }
  if (tid < kGScoreRows) gstat[(size_t)g * kGScoreRows + tid] = red[tid][0];
}

}  // namespace umpc
