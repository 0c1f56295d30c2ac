// Bootstrap confidence bands of ensemble curves (umpcBatchEnsembleBootstrap, include/umpc_mi355x.h): for every recorded step
// and every grid cell the draws of the cell are resampled R times ON the device, a statistic (the mean, or a nearest-rank
// quantile) is taken of every resample of the step's term, and the step gets its point estimate, the mean and standard
// error of its R replicates and their percentile band; over the steps of the window every replicate keeps the largest
// studentised distance max_i |t_{i,r} - point_i| / se_i, whose quantiles are the critical values of a SIMULTANEOUS band
// point_i +- crit * se_i (sup-t). The pieces are those of umpc_quantile.h and umpc_bootstrap.h, unchanged: the counter hash
// boot_index, the ds_bpermute gather, boot_wave_stat (fp64 butterfly / 21-stage sort), quant_block_row, boot_row_moments.
//
// One pass, one kernel, nothing of size R * B or K * G * R anywhere. One workgroup of four wavefronts owns a cell and walks
// the steps of the window in order. Per step:
// 1. The values. A cell of up to 64 members: EVERY wavefront loads the members' words itself (lane = member; score_load /
//    score_terms as the quantile kernel, so a member is scored exactly when umpcBatchEnsembleQuantiles scores it and its term
//    has the same bits), subtracts the same term of the second history when there is one, and compacts by ballot: the
//    scored value of rank k goes to lane k by one ds_permute per dword. Four times the loads (L1 hits) and no barrier, no
//    LDS. A larger cell: wavefront 0 compacts into the cell's own segment of `work` in member-list order (the loop of
//    umpc_boot_compact_kernel), the count crosses in LDS, and with nsc <= 64 every wavefront takes v from there.
// 2. The R replicates go to LDS (dynamic, R doubles). nsc <= 64: a wavefront owns chunks of 64 replicates and forms them as
//    umpc_boot_rep_kernel does, four per trip; the order of summation is that kernel's, a function of nsc alone, so a step of
//    a cell equals umpcBatchScore(count = 1) + umpcBatchScoreBootstrap on it bit for bit. nsc > 64: boot_block_mean /
//    quant_block_row through the resample index, one replicate at a time: correct for any size, not tuned.
//    The resample index depends on (seed, r, slot, nsc) alone: while nsc does not change, replicate r draws the SAME members
//    at every step -- it resamples whole trajectories, which is what makes max_i meaningful. When a draw drops out
//    mid-window its later steps are resampled with the indices of the new count.
// 3. The row from LDS: percentiles by quant_block_row, mean and spread by boot_row_moments (the code of umpc_boot_row_kernel),
//    and whether the R replicates are all the same double (bits compared with replicate 0, one block-wide OR). A step ENTERS
//    the simultaneous statistic when nsc >= 2 and they are not: a rule on the replicates, not on se > 0.
// 4. Thread t folds |t_r - point| / se of its replicates r = t, t + 256, .. into running maxima in REGISTERS
//    (4 doubles for R <= 1024, 16 for any R up to 4096: two forms); a comparison that a NaN never wins.
// After the last step the maxima go to sup[g] and, through the LDS row, into one more quant_block_row: crit[g].
// No atomics, no scratch; every order of summation fixed: two calls give the same bits, and a cell's rows depend on the
// cell alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_bootstrap.h"

namespace umpc {

constexpr int kBandRows = 6;                                  // UMPC_BAND_ROWS
constexpr int kBandMaxReps = 4096;                            // UMPC_BAND_MAX_REPS
constexpr int kBandHold = kBandMaxReps / kBootThreads;        // running maxima per thread, any R
constexpr int kBandHoldFew = 4;                               // R <= 1024: the form that leaves registers for a fourth block per CU
constexpr int kBandTrip = 4;                                  // replicates per trip of a wavefront

template <typename T>
struct BandArgs {
  ScoreArgs<T> t;           // the tables as the scoring kernel reads them (score, status, tol2 unused); t.count = steps
  const T *ostate, *oout;   // the second run's state and out tables, moved like t.state and t.out; ostate null without one
  const int32_t *order, *offset;
  double *band;             // [count][G][6 + nq]
  double *crit, *sup;       // [G][1 + nl], [G][R]; both null: the pointwise rows only
  double *work;             // [B + G]
  unsigned long long c0;    // seed * 0x9E3779B97F4A7C15 + salt
  double stat_p;
  int G, R, term;
  QuantProbs q, lv;         // the percentile columns, the levels of crit
};

struct BandLds {
  BootRowLds r;
  double p[kQuantMaxProbs], lv[kQuantMaxProbs];   // probs and levels, parked once: the step loop holds no launch argument it can do without
  int nsc;
};

// the term of robot b at step i of one history and whether the step is scored there. Which tables there are is the same
// in every lane (launch arguments): four straight-line loaders behind scalar branches
template <typename T>
__device__ __forceinline__ T band_term(const ScoreArgs<T> &a, int term, int b, long long i, bool &ok) {
  const size_t B = (size_t)a.B;
  ScoreStep<T> v;
  T rc[6];
  if (a.reftab) {
    score_const_ref<T, true>(a, B, b, rc);
    if (a.out) score_load<T, false, true, true, false>(a, B, 0, (unsigned)b, i, rc, v);
    else score_load<T, false, true, false, false>(a, B, 0, (unsigned)b, i, rc, v);
  } else {
    score_const_ref<T, false>(a, B, b, rc);
    if (a.out) score_load<T, false, false, true, false>(a, B, 0, (unsigned)b, i, rc, v);
    else score_load<T, false, false, false, false>(a, B, 0, (unsigned)b, i, rc, v);
  }
  const ScoreTerms<T> t = score_terms(a.taulim, v);
  ok = t.ok;
  const T ep = t.ep, es = t.es, tt = t.tt;              // (scalars first: a run-time choice among members indexes the struct)
  return term == 0 ? ep : term == 1 ? es : tt;
}

// the value of robot b at step i and whether it enters: the term, or the term minus that of the second run in double
template <typename T>
__device__ __forceinline__ double band_value(const BandArgs<T> &e, int b, long long i, bool &ok) {
  double x = (double)band_term(e.t, e.term, b, i, ok);
  if (e.ostate) {
    ScoreArgs<T> o = e.t;                                 // the same reference, B and taulim
    o.state = e.ostate; o.out = e.oout;
    bool ok2;
    x = x - (double)band_term(o, e.term, b, i, ok2);
    ok = ok & ok2 & __builtin_isfinite(x);
  }
  return x;
}

// lane `dst` receives this lane's x (dst is a permutation of the lanes)
__device__ __forceinline__ double band_send(double x, int dst) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_permute(dst << 2, (int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_permute(dst << 2, (int)(unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// BIG: the kernel of the cells above 64 members, launched behind the other one on the same grid; a block leaves the one that
// is not its own, as in umpc_quantile.h (one kernel with both holds the large cells' scalars across the small cells' loop).
// HOLD: the running maxima a thread keeps, R <= HOLD * 256. The replicate loop needs a quarter of the registers of the phases
// around it, so what hides its cross-lane latencies is not other wavefronts (the stand-alone replicate kernel runs eight per
// SIMD) but kBandTrip independent replicates per trip, and with HOLD = 4 a fourth block per CU: 1 024 cells in one round.
template <typename T, int STAT, bool BIG, int HOLD>
__global__ __launch_bounds__(kBootThreads, HOLD == kBandHoldFew ? 4 : 2) void umpc_band_kernel(const BandArgs<T> e) {
  __shared__ BandLds lds;
  extern __shared__ __attribute__((aligned(8))) double band_reps[];     // [R]: the replicates of the step in hand
  double *reps = band_reps;
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y), tid = wave * 64 + lane;
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  if (BIG ? n <= 64 : n > 64) return;
  const int32_t *mem = e.order + lo;
  const int R = e.R, nq = e.q.nq, nl = e.lv.nq, cols = kBandRows + nq;
  if (tid < kQuantMaxProbs) { lds.p[tid] = quant_prob(e.q, tid); lds.lv[tid] = quant_prob(e.lv, tid); }
  const long long count = e.t.count;
  const bool simul = e.sup != nullptr;
  const unsigned long long c0 = e.c0;
  double mx[HOLD];
#pragma unroll
  for (int k = 0; k < HOLD; ++k) mx[k] = 0.0;
  int entered = 0;
  // a lane past the end of the list reads the last member again and does not enter
  const int mine = (!BIG && n > 0) ? mem[lane < n ? lane : n - 1] : 0;

  for (long long i = 0; i < count; ++i) {
    double *row = e.band + ((size_t)i * e.G + g) * cols;
    // ---- 1. the values of the step: v[0 .. nsc) in member-list order ------------------------------------------------
    int nsc = 0;
    double v = 0.0;
    if (!BIG) {
      bool ok = false;
      double x = 0.0;
      if (n > 0) x = band_value(e, mine, i, ok);
      ok = ok & (lane < n);
      const unsigned long long bal = __ballot(ok);
      nsc = __popcll(bal);
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
      v = band_send(x, ok ? rank : nsc + (lane - rank));      // the others behind the scored ones: never read
    } else {
      if (wave == 0) {
        double *w = e.work + lo;
        int at = 0;
        for (int m0 = 0; m0 < n; m0 += 64) {
          const int m = m0 + lane;
          bool ok = false;
          double x = 0.0;
          if (m < n) x = band_value(e, mem[m], i, ok);
          const unsigned long long bal = __ballot(ok);
          const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          if (ok) w[at + rank] = x;                        // at + rank < n: at most one slot per member
          at += __popcll(bal);
        }
        if (lane == 0) lds.nsc = at;
      }
      __syncthreads();
      nsc = lds.nsc;
      if (nsc > 0 && nsc <= 64) v = e.work[lo + (lane < nsc ? lane : nsc - 1)];
    }
    nsc = __builtin_amdgcn_readfirstlane(nsc);
    if (nsc == 0) {                                       // (the same in every wavefront of the block)
      if (tid < cols) row[tid] = tid == 0 ? 0.0 : tid == 1 ? (double)n : tid == 5 ? 0.0 : __builtin_nan("");
      __syncthreads();                                    // (lds.nsc is written again by the next step)
      continue;
    }
    // ---- 2. the point estimate (in every thread) and the R replicates (in LDS) ---------------------------------------
    const int k = quant_rank(e.stat_p, nsc);
    double point;
    if (!BIG || nsc <= 64) {
      {
        double x[1] = {v};
        boot_wave_stat<STAT, 1>(x, nsc, k, lane);
        point = x[0];
      }
      for (int r0 = wave * 64; r0 < R; r0 += kBootThreads) {
        const int cnt = R - r0 < 64 ? R - r0 : 64;
        double res = 0.0;
        for (int t = 0; t < cnt; t += kBandTrip) {        // (replicates past r0 + cnt are formed and not stored)
          double x[kBandTrip];
#pragma unroll
          for (int s = 0; s < kBandTrip; ++s) x[s] = __shfl(v, boot_index(c0, r0 + t + s, lane, nsc));
          boot_wave_stat<STAT, kBandTrip>(x, nsc, k, lane);
#pragma unroll
          for (int s = 0; s < kBandTrip; ++s) res = lane == t + s ? x[s] : res;
        }
        if (lane < cnt) reps[r0 + lane] = res;
      }
    } else {
      const double *w = e.work + lo;
      if (STAT == kBootMean) {
        point = boot_block_mean<true>(w, c0, 0, nsc, tid, lds.r.hi);
        for (int r = 0; r < R; ++r) {
          const double t = boot_block_mean<false>(w, c0, r, nsc, tid, lds.r.hi);
          if (tid == 0) reps[r] = t;
        }
      } else {
        if (tid < kQuantMaxProbs) lds.r.q.p[tid] = e.stat_p;      // one probability: the statistic's
        quant_block_row<uint64_t>([&](int m, bool &ok) { ok = true; return quant_image(w[m]); }, nsc, 1, lane, wave, lds.r.q,
                                  lds.r.row);
        point = lds.r.row[2];
        for (int r = 0; r < R; ++r) {
          quant_block_row<uint64_t>([&](int m, bool &ok) { ok = true; return quant_image(w[boot_index(c0, r, m, nsc)]); }, nsc, 1,
                                    lane, wave, lds.r.q, lds.r.row);
          if (tid == 0) reps[r] = lds.r.row[2];           // (behind the row's last barrier; the next row is written three barriers on)
        }
      }
    }
    __syncthreads();
    // ---- 3. the row of the step from its replicates ---------------------------------------------------------------------
    if (tid < kQuantMaxProbs) lds.r.q.p[tid] = lds.p[tid];    // (its own thread wrote lds.p[tid])
    quant_block_row<uint64_t>([&](int r, bool &ok) { ok = true; return quant_image(reps[r]); }, R, nq, lane, wave, lds.r.q,
                              lds.r.row);
    if (tid < nq) row[kBandRows + tid] = lds.r.row[2 + tid];
    double mean, ss;
    boot_row_moments(reps, R, tid, lds.r, mean, ss);
    const double se = __builtin_sqrt(ss / (double)(R - 1));
    const long long first = __double_as_longlong(reps[0]);
    int differs = 0;
    for (int r = tid; r < R; r += kBootThreads) differs |= __double_as_longlong(reps[r]) != first;
    const bool enters = (__syncthreads_or(differs) != 0) & (nsc >= 2);
    if (tid == 0) {
      row[0] = (double)nsc; row[1] = (double)(n - nsc); row[2] = point; row[3] = mean; row[4] = se;
      row[5] = enters ? 1.0 : 0.0;
    }
    // ---- 4. the studentised distances of this thread's replicates ---------------------------------------------------------
    if (simul && enters) {
      ++entered;
#pragma unroll
      for (int j = 0; j < HOLD; ++j) {
        const int r = tid + j * kBootThreads;
        if (r < R) {
          const double d = __builtin_fabs(reps[r] - point) / se;
          mx[j] = d > mx[j] ? d : mx[j];
        }
      }
    }
    __syncthreads();                                      // the next step writes reps and the LDS block
  }
  if (!simul) return;
  // ---- sup[g] and its quantiles -------------------------------------------------------------------------------------------
  double *crit = e.crit + (size_t)g * (1 + nl), *sup = e.sup + (size_t)g * R;
  if (tid == 0) crit[0] = (double)entered;
#pragma unroll
  for (int j = 0; j < HOLD; ++j) {
    const int r = tid + j * kBootThreads;
    if (r < R) {
      const double s = entered > 0 ? mx[j] : __builtin_nan("");
      reps[r] = s;
      sup[r] = s;
    }
  }
  if (entered == 0) {
    if (tid < nl) crit[1 + tid] = __builtin_nan("");
    return;
  }
  __syncthreads();
  if (tid < kQuantMaxProbs) lds.r.q.p[tid] = lds.lv[tid];
  quant_block_row<uint64_t>([&](int r, bool &ok) { ok = true; return quant_image(reps[r]); }, R, nl, lane, wave, lds.r.q, lds.r.row);
  if (tid < nl) crit[1 + tid] = lds.r.row[2 + tid];
}

}  // namespace umpc
