// libumpc_mi355x.so, scoring: the entry points on recorded rollouts (umpcBatchScoreInit .. umpcBatchTransfer) and their
// host launchers. The kernels are the stand-alone ones of umpc_score.h, umpc_ensemble.h, umpc_quantile.h, umpc_bootstrap.h,
// umpc_band.h, umpc_response.h, umpc_dispersion.h, umpc_propagator.h, umpc_sensitivity.h, umpc_spectrum.h, umpc_gram.h and
// umpc_transfer.h: nothing here reads the step path or a generated header.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "umpc_handle.h"
#include "umpc_score.h"    // scoring of recorded rollouts (umpcBatchScore / umpcBatchScoreGroups)
#include "umpc_ensemble.h" // per-step, per-group statistics of recorded rollouts (umpcBatchEnsemble)
#include "umpc_quantile.h" // per-step, per-group order statistics (umpcBatchEnsembleQuantiles / umpcBatchScoreQuantiles)
#include "umpc_bootstrap.h" // bootstrap intervals of a per-group cost table (umpcBatchScoreBootstrap)
#include "umpc_band.h"     // bootstrap bands of per-step, per-group curves (umpcBatchEnsembleBootstrap)
#include "umpc_response.h" // per-robot sine fit at the robot's own frequency (umpcBatchResponse / umpcBatchResponseFit)
#include "umpc_dispersion.h" // per-step, per-group moments, ellipsoids and Mahalanobis scores (umpcBatchDispersion ..)
#include "umpc_propagator.h" // per-step, per-group lagged moments and the affine map between two steps (umpcBatchLagMoments ..)
#include "umpc_sensitivity.h" // per-step, per-group binned sums over the drawn inputs and their correlation ratios (umpcBatchSensitivity ..)
#include "umpc_spectrum.h" // per-robot projections onto a temporal basis, periodograms and their per-group sums (umpcBatchSpectrum ..)
#include "umpc_gram.h"     // per-group Gram matrix of the error trajectories (fp64 MFMA) and weighted sums over a group's draws (umpcBatchGram ..)
#include "umpc_transfer.h" // per-robot projections of an input and an output, per-group cross-spectra, transfer function and coherence (umpcBatchCrossSpectrum ..)

// UMPC_SCORE_NT=1 reads the tables with non-temporal loads (A/B timing, tools/time_score.py)
static bool score_nt() {
  static const bool v = [] { const char *e_ = getenv("UMPC_SCORE_NT"); return e_ && atoi(e_) != 0; }();
  return v;
}

// UMPC_SPEC_KT=16 runs the sums kernel of umpcBatchSpectrum with tiles of 16 frequencies instead of 8 (A/B timing,
// tools/time_spectrum.py: 8 is the faster one at the shape of record; the sums do not depend on it)
static int spec_kt() {
  static const int v = [] { const char *e_ = getenv("UMPC_SPEC_KT"); return e_ && atoi(e_) == 16 ? 16 : 8; }();
  return v;
}

// UMPC_XS_KT=8 runs the sums kernel of umpcBatchCrossSpectrum with tiles of 8 frequencies instead of 4 (A/B timing,
// tools/time_transfer.py: 4 is the faster one at the shape of record; the sums do not depend on it). Read at every call, so
// that one process can run both.
static int xs_kt() {
  const char *e_ = getenv("UMPC_XS_KT");
  return e_ && atoi(e_) == 8 ? 8 : 4;
}

// ---- what the entry points on the recorded tables share (umpcBatchScore .. umpcBatchResponse) ----------------------------
// the recorded tables and the window of a call, as the C ABI passes them
struct ScoreWindow {
  const void *state_hist, *out_hist;
  const int32_t *status_hist;
  const void *ref_tab, *ref;
  long long first, count, ref_first;
  int after;
};

// the tables as the kernels read them: the pointers moved to the first slice of the call (state: slice first + after)
template <typename T>
static umpc::ScoreArgs<T> score_args(const umpc_batch_t *h, const ScoreWindow &w, double tol_p, long long step0, void *score) {
  const size_t B = (size_t)h->B;
  umpc::ScoreArgs<T> a;
  a.state = (const T *)w.state_hist + (size_t)(w.first + (w.after ? 1 : 0)) * 18 * B;
  a.out = w.out_hist ? (const T *)w.out_hist + (size_t)w.first * 9 * B : nullptr;
  a.status = w.status_hist ? w.status_hist + (size_t)w.first * B : nullptr;
  a.reftab = w.ref_tab ? (const T *)w.ref_tab + (size_t)w.ref_first * 9 * B : nullptr;
  a.ref = (const T *)w.ref;
  a.score = (T *)score;
  a.B = h->B; a.count = (int)w.count; a.step0 = step0;
  a.tol2 = (T)(tol_p * tol_p); a.taulim = (T)h->prm.taulim;
  return a;
}

// slices of the step range on a grid (group, slice) of blocks of `waves` wavefronts: enough blocks to fill the device when G
// is small, never fewer than two steps per wavefront while there are that many (which wavefront or block takes a step does
// not enter its row)
static unsigned step_slices(int G, long long count, int waves) {
  long long gy = (4096 + G - 1) / G;
  const long long most = (count + 2 * waves - 1) / (2 * waves);
  if (gy > most) gy = most;
  if (gy > 65535) gy = 65535;
  return (unsigned)gy;
}

// the probabilities travel in the launch arguments
static umpc::QuantProbs quant_probs(const double *probs, int nq) {
  umpc::QuantProbs q;
  for (int j = 0; j < umpc::kQuantMaxProbs; ++j) q.p[j] = j < nq ? probs[j] : 0.0;
  q.nq = nq;
  return q;
}

// The checks below return a refusal (refuse, umpc_handle.h) as it is.
static int check_one_reference(const char *fn, const ScoreWindow &w) {
  return (w.ref_tab != nullptr) == (w.ref != nullptr)
             ? refuse(fn, "exactly one of ref_tab (a reference per step) and ref (a constant reference) must be given") : 0;
}
// (umpcBatchScore has a step0 and a count limit of its own next to these)
static int check_window(const char *fn, const ScoreWindow &w) {
  if (check_one_reference(fn, w)) return -1;
  if (w.count < 0 || w.first < 0 || w.ref_first < 0) return refuse(fn, "bad argument (count, first, ref_first >= 0)");
  return w.count > 0x7fffffffLL ? refuse(fn, "count too large for one call (2^31 - 1 steps at the most)") : 0;
}
static int check_tol(const char *fn, double tol_p) {
  return !(tol_p >= 0) || !(tol_p <= 1.79769313486231570815e308) ? refuse(fn, "bad argument (tol_p must be finite and >= 0)") : 0;
}
static int check_groups(const char *fn, int G) { return G < 1 ? refuse(fn, "bad argument (G >= 1)") : 0; }
// nq in 1 .. UMPC_QUANT_MAX_PROBS and every probability in [0, 1] (a NaN fails both comparisons)
static int check_probs(const char *fn, const double *probs, int nq) {
  bool ok = nq >= 1 && nq <= UMPC_QUANT_MAX_PROBS;
  for (int j = 0; ok && j < nq; ++j) ok = probs[j] >= 0.0 && probs[j] <= 1.0;
  return ok ? 0 : refuse(fn, "bad argument (1 to 8 probabilities, each in [0, 1])");
}
static int check_factors(const char *fn, int F, int M) {
  return F < 1 || F > UMPC_SENS_MAX_FACTORS || M < 2 || M > UMPC_SENS_MAX_BINS ? refuse(fn, "bad argument (1 <= F <= 6 factors, 2 <= M <= 8 bins)") : 0;
}
static int check_rows(const char *fn, int num, int den) {
  return num < 0 || num >= UMPC_SCORE_ROWS || den < -1 || den >= UMPC_SCORE_ROWS ? refuse(fn, "bad argument (num in 0..11, den in -1..11)") : 0;
}

// the entry points have checked the arguments
template <typename T>
static int launch_score(umpc_batch_t *h, const ScoreWindow &w, long long step0, double tol_p, void *score, void *stream) {
  const umpc::ScoreArgs<T> a = score_args<T>(h, w, tol_p, step0, score);
  const dim3 grid((unsigned)((h->B + 63) / 64)), block(64, umpc::kScoreSlices);
  // which tables there are is decided HERE, once: each combination is a kernel of its own whose loop has no branch
  const int form = (score_nt() ? 8 : 0) | (a.reftab ? 4 : 0) | (a.out ? 2 : 0) | (a.status ? 1 : 0);
#define UMPC_SCORE_FORM(f)                                                                                              \
  case f:                                                                                                               \
    hipLaunchKernelGGL((umpc::umpc_score_kernel<T, ((f) & 8) != 0, ((f) & 4) != 0, ((f) & 2) != 0, ((f) & 1) != 0>), grid, \
                       block, 0, (hipStream_t)stream, a);                                                               \
    break;
  switch (form) {
    UMPC_SCORE_FORM(0) UMPC_SCORE_FORM(1) UMPC_SCORE_FORM(2) UMPC_SCORE_FORM(3) UMPC_SCORE_FORM(4) UMPC_SCORE_FORM(5)
    UMPC_SCORE_FORM(6) UMPC_SCORE_FORM(7) UMPC_SCORE_FORM(8) UMPC_SCORE_FORM(9) UMPC_SCORE_FORM(10) UMPC_SCORE_FORM(11)
    UMPC_SCORE_FORM(12) UMPC_SCORE_FORM(13) UMPC_SCORE_FORM(14) UMPC_SCORE_FORM(15)
  }
#undef UMPC_SCORE_FORM
  return launch_status("umpcBatchScore");
}

template <typename T>
static int launch_ensemble(umpc_batch_t *h, const ScoreWindow &w, double tol_p, const int32_t *order, const int32_t *offset, int G,
                           double *ens, void *stream) {
  umpc::EnsArgs<T> e;
  e.t = score_args<T>(h, w, tol_p, 0, nullptr);
  e.order = order; e.offset = offset; e.ens = ens; e.G = G;
  const dim3 grid((unsigned)G, step_slices(G, w.count, umpc::kEnsWaves)), block(64, umpc::kEnsWaves);
  const int form = (w.ref_tab ? 4 : 0) | (w.out_hist ? 2 : 0) | (w.status_hist ? 1 : 0);
#define UMPC_ENS_FORM(f)                                                                                                \
  case f:                                                                                                               \
    hipLaunchKernelGGL((umpc::umpc_ensemble_kernel<T, ((f) & 4) != 0, ((f) & 2) != 0, ((f) & 1) != 0>), grid, block, 0,   \
                       (hipStream_t)stream, e);                                                                         \
    break;
  switch (form) {
    UMPC_ENS_FORM(0) UMPC_ENS_FORM(1) UMPC_ENS_FORM(2) UMPC_ENS_FORM(3) UMPC_ENS_FORM(4) UMPC_ENS_FORM(5)
    UMPC_ENS_FORM(6) UMPC_ENS_FORM(7)
  }
#undef UMPC_ENS_FORM
  return launch_status("umpcBatchEnsemble");
}

// (w carries no status record and there is no tube: the kernels read neither)
template <typename T>
static int launch_ens_quantiles(umpc_batch_t *h, const ScoreWindow &w, const int32_t *order, const int32_t *offset, int G, int term,
                                const double *probs, int nq, double *quant, void *stream) {
  umpc::QuantArgs<T> e;
  e.t = score_args<T>(h, w, 0.0, 0, nullptr);
  e.order = order; e.offset = offset; e.quant = quant; e.G = G;
  e.q = quant_probs(probs, nq);
  const dim3 grid((unsigned)G, step_slices(G, w.count, umpc::kQuantWaves)), block(64, umpc::kQuantWaves);
  const int form = term * 4 + (w.ref_tab ? 2 : 0) + (w.out_hist ? 1 : 0);
#define UMPC_QUANT_FORM(f)                                                                                              \
  case f:                                                                                                               \
    hipLaunchKernelGGL((umpc::umpc_ens_quantile_kernel<T, ((f) & 2) != 0, ((f) & 1) != 0, (f) / 4>), grid, block, 0,      \
                       (hipStream_t)stream, e);                                                                         \
    hipLaunchKernelGGL((umpc::umpc_ens_quantile_block_kernel<T, ((f) & 2) != 0, ((f) & 1) != 0, (f) / 4>), grid, block, 0, \
                       (hipStream_t)stream, e);                                                                         \
    break;
  switch (form) {
    UMPC_QUANT_FORM(0) UMPC_QUANT_FORM(1) UMPC_QUANT_FORM(2) UMPC_QUANT_FORM(3) UMPC_QUANT_FORM(4) UMPC_QUANT_FORM(5)
    UMPC_QUANT_FORM(6) UMPC_QUANT_FORM(7) UMPC_QUANT_FORM(9) UMPC_QUANT_FORM(11)       // (term 2 needs out: forms 8 and 10 do not exist)
  }
#undef UMPC_QUANT_FORM
  return launch_status("umpcBatchEnsembleQuantiles");
}

template <typename T>
static int launch_score_quantiles(umpc_batch_t *h, const void *score, int num, int den, const int32_t *order, const int32_t *offset,
                                  int G, const double *probs, int nq, double *quant, void *stream) {
  umpc::ScoreQuantArgs<T> e;
  e.score = (const T *)score; e.order = order; e.offset = offset; e.quant = quant;
  e.B = h->B; e.num = num; e.den = den;
  e.q = quant_probs(probs, nq);
  hipLaunchKernelGGL(umpc::umpc_score_quantile_kernel<T>, dim3((unsigned)G), dim3(64, umpc::kQuantWaves), 0, (hipStream_t)stream, e);
  return launch_status("umpcBatchScoreQuantiles");
}

// compaction, the replicates of the small and of the large cells, the rows
template <typename T>
static int launch_score_bootstrap(umpc_batch_t *h, const void *score, const void *other, int num, int den, const int32_t *order,
                                  const int32_t *offset, int G, int stat, double stat_p, int R, unsigned long long seed,
                                  const double *probs, int nq, double *boot, double *reps, double *work, void *stream) {
  umpc::BootCompactArgs<T> c;
  c.score = (const T *)score; c.other = (const T *)other; c.order = order; c.offset = offset; c.work = work;
  c.B = h->B; c.num = num; c.den = den;
  umpc::BootArgs e;
  e.offset = offset; e.work = work; e.boot = boot; e.reps = reps;
  e.c0 = seed * 0x9E3779B97F4A7C15ull + umpc::kBootSalt;      // (wraps: the hash is arithmetic modulo 2^64)
  e.stat_p = stat_p; e.B = h->B; e.R = R;
  e.q = quant_probs(probs, nq);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 block(64, umpc::kBootWaves);
  if (other) hipLaunchKernelGGL((umpc::umpc_boot_compact_kernel<T, true>), dim3((unsigned)G), dim3(64), 0, s, c);
  else hipLaunchKernelGGL((umpc::umpc_boot_compact_kernel<T, false>), dim3((unsigned)G), dim3(64), 0, s, c);
  // a wavefront of the small-cell kernel takes chunks of 64 replicates; a block of the large-cell kernels one replicate
  const int chunks = (R + 63) / 64;
  const dim3 grid_a((unsigned)G, (unsigned)((chunks + umpc::kBootWaves - 1) / umpc::kBootWaves));
  int gy = (4096 + G - 1) / G;
  if (gy > R) gy = R;
  const dim3 grid_b((unsigned)G, (unsigned)gy);
  if (stat == UMPC_BOOT_MEAN) {
    hipLaunchKernelGGL(umpc::umpc_boot_rep_kernel<umpc::kBootMean>, grid_a, block, 0, s, e);
    hipLaunchKernelGGL(umpc::umpc_boot_mean_block_kernel, grid_b, block, 0, s, e);
  } else {
    hipLaunchKernelGGL(umpc::umpc_boot_rep_kernel<umpc::kBootQuantile>, grid_a, block, 0, s, e);
    hipLaunchKernelGGL(umpc::umpc_boot_quantile_block_kernel, grid_b, block, 0, s, e);
  }
  hipLaunchKernelGGL(umpc::umpc_boot_row_kernel, dim3((unsigned)G), block, 0, s, e);
  return launch_status("umpcBatchScoreBootstrap");
}

// one block per cell walks the window; the replicates of the step in hand are its dynamic LDS
template <typename T>
static int launch_ens_bootstrap(umpc_batch_t *h, const ScoreWindow &w, const void *other_state, const void *other_out,
                                const int32_t *order, const int32_t *offset, int G, int term, int stat, double stat_p, int R,
                                unsigned long long seed, const double *probs, int nq, const double *levels, int nl, double *band,
                                double *crit, double *sup, double *work, void *stream) {
  umpc::BandArgs<T> e;
  e.t = score_args<T>(h, w, 0.0, 0, nullptr);
  ScoreWindow wo = w;
  wo.state_hist = other_state; wo.out_hist = other_out;
  const umpc::ScoreArgs<T> o = score_args<T>(h, wo, 0.0, 0, nullptr);
  e.ostate = other_state ? o.state : nullptr; e.oout = o.out;
  e.order = order; e.offset = offset; e.band = band; e.crit = crit; e.sup = sup; e.work = work;
  e.c0 = seed * 0x9E3779B97F4A7C15ull + umpc::kBootSalt;      // (wraps: the hash is arithmetic modulo 2^64)
  e.stat_p = stat_p; e.G = G; e.R = R; e.term = term;
  e.q = quant_probs(probs, nq);
  e.lv = quant_probs(levels, nl);
  const dim3 grid((unsigned)G), block(64, umpc::kBootWaves);
  const size_t lds = (size_t)R * sizeof(double);
  const hipStream_t s = (hipStream_t)stream;
  // the cells of up to 64 members (in the form that holds R / 256 running maxima per thread), then the larger ones
  const bool few = R <= umpc::kBandHoldFew * umpc::kBootThreads;
#define UMPC_BAND_FORM(STAT)                                                                                             \
  if (few) hipLaunchKernelGGL((umpc::umpc_band_kernel<T, STAT, false, umpc::kBandHoldFew>), grid, block, lds, s, e);      \
  else hipLaunchKernelGGL((umpc::umpc_band_kernel<T, STAT, false, umpc::kBandHold>), grid, block, lds, s, e);             \
  hipLaunchKernelGGL((umpc::umpc_band_kernel<T, STAT, true, umpc::kBandHold>), grid, block, lds, s, e);
  if (stat == UMPC_BOOT_MEAN) { UMPC_BAND_FORM(umpc::kBootMean) } else { UMPC_BAND_FORM(umpc::kBootQuantile) }
#undef UMPC_BAND_FORM
  return launch_status("umpcBatchEnsembleBootstrap");
}

// (w carries neither an out nor a status record: the kernel reads state rows 0..2 and reference rows 0..2)
template <typename T>
static int launch_response(umpc_batch_t *h, const ScoreWindow &w, const double *nu, long long step0, double *sums, void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, step0, nullptr);
  umpc::RespArgs<T> a;
  a.state = t.state; a.reftab = t.reftab; a.ref = t.ref; a.nu = nu; a.sums = sums;
  a.B = t.B; a.count = t.count; a.step0 = step0;
  const dim3 grid((unsigned)((h->B + 63) / 64)), block(64, umpc::kRespSlices);
  const hipStream_t s = (hipStream_t)stream;
  const int form = (score_nt() ? 2 : 0) | (a.reftab ? 1 : 0);
  switch (form) {
    case 0: hipLaunchKernelGGL((umpc::umpc_response_kernel<T, false, false>), grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL((umpc::umpc_response_kernel<T, false, true>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((umpc::umpc_response_kernel<T, true, false>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((umpc::umpc_response_kernel<T, true, true>), grid, block, 0, s, a); break;
  }
  return launch_status("umpcBatchResponse");
}

// (w carries neither an out nor a status record: the kernel reads state rows 0..2, 12..14 and reference rows 0..5)
template <typename T>
static int launch_dispersion(umpc_batch_t *h, const ScoreWindow &w, const int32_t *order, const int32_t *offset, int G, double *mom,
                             void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::DispArgs<T> a;
  a.state = t.state; a.reftab = t.reftab; a.ref = t.ref; a.order = order; a.offset = offset; a.mom = mom;
  a.B = t.B; a.count = t.count; a.G = G;
  const dim3 grid((unsigned)G, step_slices(G, w.count, umpc::kDispWaves)), block(64, umpc::kDispWaves);
  if (a.reftab) hipLaunchKernelGGL((umpc::umpc_dispersion_kernel<T, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_dispersion_kernel<T, false>), grid, block, 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchDispersion");
}

// (the window of launch_dispersion; the tables hold w.count + lag slices from their first)
template <typename T>
static int launch_lag_moments(umpc_batch_t *h, const ScoreWindow &w, int lag, const int32_t *order, const int32_t *offset, int G,
                              double *xmom, void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::LagArgs<T> a;
  a.t.state = t.state; a.t.reftab = t.reftab; a.t.ref = t.ref; a.t.order = order; a.t.offset = offset; a.t.mom = xmom;
  a.t.B = t.B; a.t.count = t.count; a.t.G = G; a.lag = lag;
  // (one row per wavefront and trip: as many slices as there are rows for a block's wavefronts, at the most)
  const dim3 grid((unsigned)G, step_slices(G, 2 * w.count, umpc::kLagWaves)), block(64, umpc::kLagWaves);
  if (a.t.reftab) hipLaunchKernelGGL((umpc::umpc_lagmom_kernel<T, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_lagmom_kernel<T, false>), grid, block, 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchLagMoments");
}

template <typename T>
static int launch_mahalanobis(umpc_batch_t *h, const ScoreWindow &w, const double *ell, const int32_t *group, int G, long long step0,
                              double limit, void *msc, void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, step0, nullptr);
  umpc::MahaArgs<T> a;
  a.state = t.state; a.reftab = t.reftab; a.ref = t.ref; a.ell = ell; a.group = group; a.msc = (T *)msc;
  a.B = t.B; a.count = t.count; a.G = G; a.step0 = step0; a.limit = (T)limit;
  const dim3 grid((unsigned)((h->B + 63) / 64)), block(64, umpc::kMahaSlices);
  if (a.reftab) hipLaunchKernelGGL((umpc::umpc_mahalanobis_kernel<T, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_mahalanobis_kernel<T, false>), grid, block, 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchMahalanobis");
}

// one block per (group, factor) and one row of blocks for the robots outside every group
template <typename T>
static int launch_factor_bins(umpc_batch_t *h, const void *factors, int F, const int32_t *order, const int32_t *offset, int G, int M,
                              int32_t *bins, void *stream) {
  umpc::BinArgs<T> a;
  a.factors = (const T *)factors; a.order = order; a.offset = offset; a.bins = bins;
  a.B = h->B; a.G = G; a.M = M;
  hipLaunchKernelGGL(umpc::umpc_factor_bins_kernel<T>, dim3((unsigned)G + 1u, (unsigned)F), dim3(umpc::kBinThreads), 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchFactorBins");
}

// (w carries no status record and there is no tube, as in launch_ens_quantiles; F <= 3 runs the form with 26 sums per lane)
template <typename T>
static int launch_sensitivity(umpc_batch_t *h, const ScoreWindow &w, const int32_t *order, const int32_t *offset, int G, int term,
                              const int32_t *bins, int F, int M, double *sens, void *stream) {
  umpc::SensArgs<T> e;
  e.t = score_args<T>(h, w, 0.0, 0, nullptr);
  e.order = order; e.offset = offset; e.bins = bins; e.sens = sens;
  e.G = G; e.F = F; e.M = M; e.term = term;
  // (one row per wavefront and trip, as in launch_lag_moments)
  const dim3 grid((unsigned)G, step_slices(G, 2 * w.count, umpc::kSensWaves)), block(64, umpc::kSensWaves);
  const int form = (F > 3 ? 4 : 0) | (w.ref_tab ? 2 : 0) | (w.out_hist ? 1 : 0);
#define UMPC_SENS_FORM(f)                                                                                               \
  case f:                                                                                                               \
    hipLaunchKernelGGL((umpc::umpc_sensitivity_kernel<T, ((f) & 2) != 0, ((f) & 1) != 0, ((f) & 4) ? 6 : 3>), grid, block, 0, \
                       (hipStream_t)stream, e);                                                                         \
    break;
  switch (form) {
    UMPC_SENS_FORM(0) UMPC_SENS_FORM(1) UMPC_SENS_FORM(2) UMPC_SENS_FORM(3) UMPC_SENS_FORM(4) UMPC_SENS_FORM(5)
    UMPC_SENS_FORM(6) UMPC_SENS_FORM(7)
  }
#undef UMPC_SENS_FORM
  return launch_status("umpcBatchSensitivity");
}

template <typename T>
static int launch_score_sensitivity(umpc_batch_t *h, const void *score, const int32_t *order, const int32_t *offset, int G, int num,
                                    int den, const int32_t *bins, int F, int M, double *sens, void *stream) {
  umpc::ScoreSensArgs<T> e;
  e.score = (const T *)score; e.order = order; e.offset = offset; e.bins = bins; e.sens = sens;
  e.B = h->B; e.num = num; e.den = den; e.F = F; e.M = M;
  if (F > 3) hipLaunchKernelGGL((umpc::umpc_score_sensitivity_kernel<T, 6>), dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, e);
  else hipLaunchKernelGGL((umpc::umpc_score_sensitivity_kernel<T, 3>), dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, e);
  return launch_status("umpcBatchScoreSensitivity");
}

// (the window is that of launch_response; signal UMPC_SPEC_U reads rows 0..2 of the out record and no reference)
template <typename T>
static int launch_spectrum(umpc_batch_t *h, int signal, const ScoreWindow &w, const double *basis, long long basis_first, int K,
                           double *sums, void *stream) {
  const size_t B = (size_t)h->B;
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::SpecArgs<T> a;
  const int yrow = signal == UMPC_SPEC_ES ? 9 : 0, rrow = signal == UMPC_SPEC_ES ? 6 : 0;
  const bool cmd = signal == UMPC_SPEC_U;
  a.y = cmd ? t.out : t.state + (size_t)yrow * B;
  a.ystride = cmd ? 9 : 18;
  a.reftab = !cmd && t.reftab ? t.reftab + (size_t)rrow * B : nullptr;
  a.ref = !cmd && t.ref ? t.ref + (size_t)rrow * B : nullptr;
  a.basis = basis + (size_t)basis_first * (1 + 2 * (size_t)K);
  a.sums = sums;
  a.B = h->B; a.count = (int)w.count; a.K = K;
  const int kt = spec_kt();
  const dim3 grid((unsigned)((h->B + 63) / 64), (unsigned)((K + kt - 1) / kt)), block(64, umpc::kSpecSlices);
  const hipStream_t s = (hipStream_t)stream;
  const int ref = cmd ? umpc::kSpecRefNone : a.reftab ? umpc::kSpecRefTable : umpc::kSpecRefConst;
#define UMPC_SPEC_FORM(R)                                                                                               \
  case R:                                                                                                               \
    if (kt == 8) hipLaunchKernelGGL((umpc::umpc_spectrum_kernel<T, R, 8>), grid, block, 0, s, a);                         \
    else hipLaunchKernelGGL((umpc::umpc_spectrum_kernel<T, R, 16>), grid, block, 0, s, a);                                \
    break;
  switch (ref) { UMPC_SPEC_FORM(0) UMPC_SPEC_FORM(1) UMPC_SPEC_FORM(2) }
#undef UMPC_SPEC_FORM
  return launch_status("umpcBatchSpectrum");
}

template <typename T>
static int launch_spectrum_power(umpc_batch_t *h, const double *sums, const double *wsum, const double *freq_hz, int K,
                                 long long nrows, int jsplit, void *power, void *spec, void *stream) {
  umpc::SpecPowerArgs<T> a;
  for (int j = 0; j < 1 + 2 * umpc::kSpecMaxK; ++j) a.wsum[j] = j < 1 + 2 * K ? wsum[j] : 0.0;
  for (int j = 0; j < umpc::kSpecMaxK; ++j) a.freq[j] = j < K ? freq_hz[j] : 0.0;
  a.sums = sums; a.power = (T *)power; a.spec = (T *)spec;
  a.nrows = (double)nrows; a.B = h->B; a.K = K; a.jsplit = jsplit;
  hipLaunchKernelGGL(umpc::umpc_spectrum_power_kernel<T>, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchSpectrumPower");
}

// one wavefront per (group, channel); K <= 32 runs the form with one tree of 32 frequencies per lane
template <typename T>
static int launch_spectrum_groups(umpc_batch_t *h, const void *power, const void *spec, const int32_t *order, const int32_t *offset,
                                  int G, int K, double *gspec, void *stream) {
  umpc::SpecGroupArgs<T> a;
  a.power = (const T *)power; a.spec = (const T *)spec; a.order = order; a.offset = offset; a.gspec = gspec;
  a.B = h->B; a.K = K;
  const dim3 grid((unsigned)G, 3u);
  if (K > 32) hipLaunchKernelGGL((umpc::umpc_spectrum_groups_kernel<T, 2>), grid, dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_spectrum_groups_kernel<T, 1>), grid, dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchSpectrumGroups");
}

// x and y of a pair as the kernel reads them (umpc_transfer.h): the tracking and the attitude pair read two tables as they
// are, the push pair the impulse table and p - pdes
template <typename T>
static int launch_cross_spectrum(umpc_batch_t *h, int pair, const ScoreWindow &w, const void *imp_tab, long long imp_first,
                                 const double *basis, long long basis_first, int K, double *xsums, void *stream) {
  const size_t B = (size_t)h->B;
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::XsArgs<T> a;
  const bool push = pair == UMPC_XS_PUSH, att = pair == UMPC_XS_ATT;
  a.x = push ? (const T *)imp_tab + (size_t)imp_first * 6 * B : t.reftab + (size_t)(att ? 6 : 0) * B;
  a.xstride = push ? 6 : 9;
  a.y = t.state + (size_t)(att ? 9 : 0) * B;
  a.reftab = push ? t.reftab : nullptr;
  a.ref = push ? t.ref : nullptr;
  a.basis = basis + (size_t)basis_first * (1 + 2 * (size_t)K);
  a.sums = xsums;
  a.B = h->B; a.count = (int)w.count; a.K = K;
  const int kt = xs_kt();
  const dim3 grid((unsigned)((h->B + 63) / 64), (unsigned)((K + kt - 1) / kt)), block(64, umpc::kSpecSlices);
  const hipStream_t s = (hipStream_t)stream;
  const int form = !push ? umpc::kXsTwoTables : a.reftab ? umpc::kXsPushTable : umpc::kXsPushConst;
#define UMPC_XS_FORM(F)                                                                                                 \
  case F:                                                                                                               \
    if (kt == 8) hipLaunchKernelGGL((umpc::umpc_xspec_kernel<T, F, 8>), grid, block, 0, s, a);                            \
    else hipLaunchKernelGGL((umpc::umpc_xspec_kernel<T, F, 4>), grid, block, 0, s, a);                                    \
    break;
  switch (form) { UMPC_XS_FORM(0) UMPC_XS_FORM(1) UMPC_XS_FORM(2) }
#undef UMPC_XS_FORM
  return launch_status("umpcBatchCrossSpectrum");
}

// (the window of launch_dispersion; one block per cell, whatever G and the window)
template <typename T>
static int launch_gram(umpc_batch_t *h, const ScoreWindow &w, const int32_t *order, const int32_t *offset, int G, const double *scale,
                       int accumulate, double *gram, void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::GramArgs<T> a;
  a.t.state = t.state; a.t.reftab = t.reftab; a.t.ref = t.ref; a.t.order = order; a.t.offset = offset; a.t.mom = nullptr;
  a.t.B = t.B; a.t.count = t.count; a.t.G = G;
  for (int c = 0; c < 6; ++c) a.scale[c] = scale[c];
  a.gram = gram; a.accumulate = accumulate;
  const dim3 grid((unsigned)G), block(64, umpc::kGramWaves);
  if (a.t.reftab) hipLaunchKernelGGL((umpc::umpc_gram_kernel<T, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_gram_kernel<T, false>), grid, block, 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchGram");
}

// (the window and the grid of launch_dispersion)
template <typename T>
static int launch_project(umpc_batch_t *h, const ScoreWindow &w, const int32_t *order, const int32_t *offset, int G,
                          const double *weights, int M, double *proj, void *stream) {
  const umpc::ScoreArgs<T> t = score_args<T>(h, w, 0.0, 0, nullptr);
  umpc::ProjArgs<T> a;
  a.t.state = t.state; a.t.reftab = t.reftab; a.t.ref = t.ref; a.t.order = order; a.t.offset = offset; a.t.mom = nullptr;
  a.t.B = t.B; a.t.count = t.count; a.t.G = G;
  a.weights = weights; a.proj = proj; a.M = M;
  const dim3 grid((unsigned)G, step_slices(G, w.count, umpc::kDispWaves)), block(64, umpc::kDispWaves);
  if (a.t.reftab) hipLaunchKernelGGL((umpc::umpc_project_kernel<T, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((umpc::umpc_project_kernel<T, false>), grid, block, 0, (hipStream_t)stream, a);
  return launch_status("umpcBatchProject");
}

static int check_freqs(const char *fn, int K) {
  return K < 1 || K > UMPC_SPEC_MAX_K ? refuse(fn, "bad argument (1 <= K <= 64 frequencies)") : 0;
}

extern "C" {

int umpcBatchScoreInit(umpc_batch_t *h, void *score, void *stream) {
  if (!h || !score) { umpc_set_error("umpcBatchScoreInit: bad argument"); return -1; }
  const dim3 grid((unsigned)((h->B + 255) / 256));
  if (h->dtype == UMPC_F32) hipLaunchKernelGGL(umpc::umpc_score_init_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (float *)score, h->B);
  else hipLaunchKernelGGL(umpc::umpc_score_init_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (double *)score, h->B);
  return launch_status("umpcBatchScoreInit");
}
int umpcBatchScore(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist,
                   const void *ref_tab, const void *ref, long long first, long long count, long long ref_first,
                   long long step0, double tol_p, int after, void *score, void *stream) {
  const char *fn = "umpcBatchScore";
  const ScoreWindow w = {state_hist, out_hist, status_hist, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!score || !state_hist) return refuse(fn, "bad argument (score and state_hist must be given)");
  if (check_one_reference(fn, w)) return -1;
  if (count < 0 || first < 0 || ref_first < 0 || step0 < 0) return refuse(fn, "bad argument (count, first, ref_first, step0 >= 0)");
  if (check_tol(fn, tol_p)) return -1;
  if (count > 0x7fffffffLL - 2 * umpc::kScoreSlices) return refuse(fn, "count too large for one call (2^31 - 17 steps at the most)");
  // counts and step numbers are scalars of the dtype: fp32 holds integers exactly up to 2^24. Row 0 never exceeds the
  // number of steps scored, which is at most step0 + count when step0 counts the steps from the start of the run.
  if (h->dtype == UMPC_F32 && step0 + count > (1LL << 24))
    return refuse(fn, "step0 + count passes 2^24, the largest step number and count an fp32 score holds exactly (score in fp64, or in parts)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_score<float>(h, w, step0, tol_p, score, stream)
                              : launch_score<double>(h, w, step0, tol_p, score, stream);
}
int umpcBatchScoreGroups(umpc_batch_t *h, const void *score, const int32_t *group, int G, double *gstat, void *stream) {
  if (!h || !score || !group || !gstat || G < 1) return refuse("umpcBatchScoreGroups", "bad argument (score, group, gstat and G >= 1 must be given)");
  if (h->dtype == UMPC_F32)
    hipLaunchKernelGGL(umpc::umpc_score_groups_kernel<float>, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, (const float *)score, group, h->B, gstat);
  else
    hipLaunchKernelGGL(umpc::umpc_score_groups_kernel<double>, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, (const double *)score, group, h->B, gstat);
  return launch_status("umpcBatchScoreGroups");
}
int umpcBatchGroupIndex(umpc_batch_t *h, const int32_t *group, int G, int32_t *order, int32_t *offset, void *stream) {
  if (!h || !group || !order || !offset || G < 1) return refuse("umpcBatchGroupIndex", "bad argument (group, order, offset and G >= 1 must be given)");
  hipLaunchKernelGGL(umpc::umpc_group_index_kernel, dim3((unsigned)G + 1u), dim3(64), 0, (hipStream_t)stream, group, h->B, G, order, offset);
  return launch_status("umpcBatchGroupIndex");
}
int umpcBatchEnsemble(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist,
                      const void *ref_tab, const void *ref, long long first, long long count, long long ref_first,
                      double tol_p, int after, const int32_t *order, const int32_t *offset, int G,
                      double *ens, void *stream) {
  const char *fn = "umpcBatchEnsemble";
  const ScoreWindow w = {state_hist, out_hist, status_hist, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !ens) return refuse(fn, "bad argument (state_hist, order, offset and ens must be given)");
  if (check_window(fn, w) || check_tol(fn, tol_p) || check_groups(fn, G)) return -1;
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_ensemble<float>(h, w, tol_p, order, offset, G, ens, stream)
                              : launch_ensemble<double>(h, w, tol_p, order, offset, G, ens, stream);
}
int umpcBatchEnsembleQuantiles(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *ref_tab,
                               const void *ref, long long first, long long count, long long ref_first, int after,
                               const int32_t *order, const int32_t *offset, int G, int term, const double *probs,
                               int nq, double *quant, void *stream) {
  const char *fn = "umpcBatchEnsembleQuantiles";
  const ScoreWindow w = {state_hist, out_hist, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !probs || !quant) return refuse(fn, "bad argument (state_hist, order, offset, probs and quant must be given)");
  if (check_window(fn, w) || check_groups(fn, G) || check_probs(fn, probs, nq)) return -1;
  if (term < UMPC_TERM_EP || term > UMPC_TERM_TAU) return refuse(fn, "bad argument (term is UMPC_TERM_EP, UMPC_TERM_ES or UMPC_TERM_TAU)");
  if (term == UMPC_TERM_TAU && !out_hist) return refuse(fn, "UMPC_TERM_TAU needs out_hist (the moments are read from it)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_ens_quantiles<float>(h, w, order, offset, G, term, probs, nq, quant, stream)
                              : launch_ens_quantiles<double>(h, w, order, offset, G, term, probs, nq, quant, stream);
}
int umpcBatchScoreQuantiles(umpc_batch_t *h, const void *score, int num, int den, const int32_t *order,
                            const int32_t *offset, int G, const double *probs, int nq, double *quant, void *stream) {
  const char *fn = "umpcBatchScoreQuantiles";
  if (!h || !score || !order || !offset || !probs || !quant) return refuse(fn, "bad argument (h, score, order, offset, probs and quant must be given)");
  if (check_groups(fn, G) || check_probs(fn, probs, nq) || check_rows(fn, num, den)) return -1;
  return h->dtype == UMPC_F32 ? launch_score_quantiles<float>(h, score, num, den, order, offset, G, probs, nq, quant, stream)
                              : launch_score_quantiles<double>(h, score, num, den, order, offset, G, probs, nq, quant, stream);
}
int umpcBatchScoreBootstrap(umpc_batch_t *h, const void *score, const void *other, int num, int den,
                            const int32_t *order, const int32_t *offset, int G, int stat, double stat_p,
                            int R, unsigned long long seed, const double *probs, int nq,
                            double *boot, double *reps, double *work, void *stream) {
  const char *fn = "umpcBatchScoreBootstrap";
  if (!score || !order || !offset || !probs) return refuse(fn, "bad argument (score, order, offset and probs must be given)");
  if (!boot || !reps || !work) return refuse(fn, "bad argument (boot [G][5 + nq], reps [G][R] and work [B + G] must be given)");
  if (check_groups(fn, G)) return -1;
  if (R < 2 || R > UMPC_BOOT_MAX_REPS) return refuse(fn, "bad argument (2 <= R <= 1048576 replicates)");
  if (stat != UMPC_BOOT_MEAN && stat != UMPC_BOOT_QUANTILE) return refuse(fn, "bad argument (stat is UMPC_BOOT_MEAN or UMPC_BOOT_QUANTILE)");
  if (!(stat_p >= 0.0 && stat_p <= 1.0)) return refuse(fn, "bad argument (stat_p in [0, 1])");
  if (check_probs(fn, probs, nq) || check_rows(fn, num, den)) return -1;
  // (the handle last: every other refusal can be met without one; nothing above reads it)
  if (!h) return refuse(fn, "bad argument (no handle)");
  return h->dtype == UMPC_F32
             ? launch_score_bootstrap<float>(h, score, other, num, den, order, offset, G, stat, stat_p, R, seed, probs, nq, boot, reps, work, stream)
             : launch_score_bootstrap<double>(h, score, other, num, den, order, offset, G, stat, stat_p, R, seed, probs, nq, boot, reps, work, stream);
}
int umpcBatchEnsembleBootstrap(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *other_state,
                               const void *other_out, const void *ref_tab, const void *ref, long long first, long long count,
                               long long ref_first, int after, const int32_t *order, const int32_t *offset, int G, int term,
                               int stat, double stat_p, int R, unsigned long long seed, const double *probs, int nq,
                               const double *levels, int nl, double *band, double *crit, double *sup, double *work,
                               void *stream) {
  const char *fn = "umpcBatchEnsembleBootstrap";
  const ScoreWindow w = {state_hist, out_hist, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!state_hist || !order || !offset || !probs) return refuse(fn, "bad argument (state_hist, order, offset and probs must be given)");
  if (!band || !work) return refuse(fn, "bad argument (band [count][G][6 + nq] and work [B + G] must be given)");
  if ((crit != nullptr) != (sup != nullptr)) return refuse(fn, "bad argument (crit [G][1 + nl] and sup [G][R] are given together or not at all)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  if (R < 2 || R > UMPC_BAND_MAX_REPS) return refuse(fn, "bad argument (2 <= R <= 4096 replicates)");
  if (stat != UMPC_BOOT_MEAN && stat != UMPC_BOOT_QUANTILE) return refuse(fn, "bad argument (stat is UMPC_BOOT_MEAN or UMPC_BOOT_QUANTILE)");
  if (!(stat_p >= 0.0 && stat_p <= 1.0)) return refuse(fn, "bad argument (stat_p in [0, 1])");
  if (check_probs(fn, probs, nq)) return -1;
  if (crit) {
    bool ok = levels != nullptr && nl >= 1 && nl <= UMPC_QUANT_MAX_PROBS;
    for (int j = 0; ok && j < nl; ++j) ok = levels[j] >= 0.0 && levels[j] <= 1.0;
    if (!ok) return refuse(fn, "bad argument (1 to 8 levels, each in [0, 1], with crit and sup)");
  } else if (nl != 0) {
    return refuse(fn, "bad argument (levels without crit and sup: nl must be 0)");
  }
  if (term < UMPC_TERM_EP || term > UMPC_TERM_TAU) return refuse(fn, "bad argument (term is UMPC_TERM_EP, UMPC_TERM_ES or UMPC_TERM_TAU)");
  if (term == UMPC_TERM_TAU && !out_hist) return refuse(fn, "UMPC_TERM_TAU needs out_hist (the moments are read from it)");
  if (other_out && !other_state) return refuse(fn, "bad argument (other_out without other_state)");
  if (other_state && (other_out != nullptr) != (out_hist != nullptr))
    return refuse(fn, "other_state needs other_out exactly when out_hist is given (both runs are scored by the same rule)");
  // (the handle last: every other refusal can be met without one; nothing above reads it)
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32
             ? launch_ens_bootstrap<float>(h, w, other_state, other_out, order, offset, G, term, stat, stat_p, R, seed, probs, nq, levels, nl, band, crit, sup, work, stream)
             : launch_ens_bootstrap<double>(h, w, other_state, other_out, order, offset, G, term, stat, stat_p, R, seed, probs, nq, levels, nl, band, crit, sup, work, stream);
}
int umpcBatchResponseInit(umpc_batch_t *h, double *sums, void *stream) {
  const char *fn = "umpcBatchResponseInit";
  if (!h || !sums) return refuse(fn, "bad argument (h and sums must be given)");
  const hipError_t e = hipMemsetAsync(sums, 0, sizeof(double) * UMPC_RSUM_ROWS * (size_t)h->B, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(e, fn);
}
int umpcBatchResponse(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, const double *nu,
                      long long first, long long count, long long ref_first, long long step0, int after, double *sums,
                      void *stream) {
  const char *fn = "umpcBatchResponse";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !nu || !sums) return refuse(fn, "bad argument (state_hist, nu and sums must be given)");
  if (check_window(fn, w)) return -1;
  if (count > 0x7fffffffLL - 2 * umpc::kRespSlices) return refuse(fn, "count too large for one call (2^31 - 9 steps at the most)");
  // k = step0 + i enters the phase as a double: every step number of the call must be one exactly
  if (step0 < 0 || step0 > (1LL << 53) - count) return refuse(fn, "bad argument (0 <= step0, step0 + count <= 2^53)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_response<float>(h, w, nu, step0, sums, stream)
                              : launch_response<double>(h, w, nu, step0, sums, stream);
}
int umpcBatchResponseFit(umpc_batch_t *h, const double *sums, void *resp, void *stream) {
  const char *fn = "umpcBatchResponseFit";
  if (!h || !sums || !resp) return refuse(fn, "bad argument (h, sums and resp must be given)");
  const dim3 grid((unsigned)((h->B + 255) / 256));
  if (h->dtype == UMPC_F32)
    hipLaunchKernelGGL(umpc::umpc_response_fit_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, sums, (float *)resp, h->B);
  else
    hipLaunchKernelGGL(umpc::umpc_response_fit_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, sums, (double *)resp, h->B);
  return launch_status(fn);
}
int umpcBatchDispersion(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, long long first,
                        long long count, long long ref_first, int after, const int32_t *order, const int32_t *offset, int G,
                        double *mom, void *stream) {
  const char *fn = "umpcBatchDispersion";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !mom) return refuse(fn, "bad argument (state_hist, order, offset and mom must be given)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_dispersion<float>(h, w, order, offset, G, mom, stream)
                              : launch_dispersion<double>(h, w, order, offset, G, mom, stream);
}
int umpcBatchDispersionEllipsoids(umpc_batch_t *h, const double *mom, long long count, int G, double *ell, void *stream) {
  const char *fn = "umpcBatchDispersionEllipsoids";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!mom || !ell) return refuse(fn, "bad argument (mom and ell must be given)");
  if (count < 0 || count > 0x7fffffffLL) return refuse(fn, "bad argument (0 <= count <= 2^31 - 1)");
  if (check_groups(fn, G)) return -1;
  if (count == 0) return 0;
  const long long rows = count * G;
  if ((rows + 255) / 256 > 0x7fffffffLL) return refuse(fn, "count x G too large for one call (2^39 rows at the most)");
  hipLaunchKernelGGL(umpc::umpc_dispersion_ellipsoid_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     mom, rows, ell);
  return launch_status(fn);
}
int umpcBatchMahalanobisInit(umpc_batch_t *h, void *msc, void *stream) {
  const char *fn = "umpcBatchMahalanobisInit";
  if (!h || !msc) return refuse(fn, "bad argument (h and msc must be given)");
  const dim3 grid((unsigned)((h->B + 255) / 256));
  if (h->dtype == UMPC_F32) hipLaunchKernelGGL(umpc::umpc_mahalanobis_init_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (float *)msc, h->B);
  else hipLaunchKernelGGL(umpc::umpc_mahalanobis_init_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (double *)msc, h->B);
  return launch_status(fn);
}
int umpcBatchMahalanobis(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, const double *ell,
                         const int32_t *group, int G, long long first, long long count, long long ref_first, long long step0,
                         int after, double limit, void *msc, void *stream) {
  const char *fn = "umpcBatchMahalanobis";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !ell || !group || !msc) return refuse(fn, "bad argument (state_hist, ell, group and msc must be given)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  if (step0 < 0) return refuse(fn, "bad argument (step0 >= 0)");
  if (!(limit > 0) || !(limit <= 1.79769313486231570815e308)) return refuse(fn, "bad argument (limit must be finite and > 0)");
  if (count > 0x7fffffffLL - 2 * umpc::kMahaSlices) return refuse(fn, "count too large for one call (2^31 - 17 steps at the most)");
  // counts and step numbers are scalars of the dtype, as in umpcBatchScore
  if (h->dtype == UMPC_F32 && step0 + count > (1LL << 24))
    return refuse(fn, "step0 + count passes 2^24, the largest step number and count an fp32 score holds exactly (score in fp64, or in parts)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_mahalanobis<float>(h, w, ell, group, G, step0, limit, msc, stream)
                              : launch_mahalanobis<double>(h, w, ell, group, G, step0, limit, msc, stream);
}
int umpcBatchLagMoments(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, long long first,
                        long long count, long long ref_first, int after, int lag, const int32_t *order, const int32_t *offset, int G,
                        double *xmom, void *stream) {
  const char *fn = "umpcBatchLagMoments";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !xmom) return refuse(fn, "bad argument (state_hist, order, offset and xmom must be given)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  if (lag < 1 || lag > (1 << 20)) return refuse(fn, "bad argument (1 <= lag <= 2^20)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_lag_moments<float>(h, w, lag, order, offset, G, xmom, stream)
                              : launch_lag_moments<double>(h, w, lag, order, offset, G, xmom, stream);
}
int umpcBatchPropagators(umpc_batch_t *h, const double *xmom, long long count, int G, double *prop, void *stream) {
  const char *fn = "umpcBatchPropagators";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!xmom || !prop) return refuse(fn, "bad argument (xmom and prop must be given)");
  if (count < 0 || count > 0x7fffffffLL) return refuse(fn, "bad argument (0 <= count <= 2^31 - 1)");
  if (check_groups(fn, G)) return -1;
  if (count == 0) return 0;
  const long long rows = count * G, blocks = (rows + umpc::kPropBlock - 1) / umpc::kPropBlock;
  if (blocks > 0x7fffffffLL) return refuse(fn, "count x G too large for one call (2^39 rows at the most)");
  hipLaunchKernelGGL(umpc::umpc_propagator_kernel, dim3((unsigned)blocks), dim3(umpc::kPropBlock), 0, (hipStream_t)stream, xmom, rows,
                     prop);
  return launch_status(fn);
}

int umpcBatchFactorBins(umpc_batch_t *h, const void *factors, int F, const int32_t *order, const int32_t *offset, int G, int M,
                        int32_t *bins, void *stream) {
  const char *fn = "umpcBatchFactorBins";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!factors || !order || !offset || !bins) return refuse(fn, "bad argument (factors, order, offset and bins must be given)");
  if (check_groups(fn, G) || check_factors(fn, F, M)) return -1;
  return h->dtype == UMPC_F32 ? launch_factor_bins<float>(h, factors, F, order, offset, G, M, bins, stream)
                              : launch_factor_bins<double>(h, factors, F, order, offset, G, M, bins, stream);
}
int umpcBatchSensitivity(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *ref_tab, const void *ref,
                         long long first, long long count, long long ref_first, int after, const int32_t *order,
                         const int32_t *offset, int G, int term, const int32_t *bins, int F, int M, double *sens, void *stream) {
  const char *fn = "umpcBatchSensitivity";
  const ScoreWindow w = {state_hist, out_hist, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !bins || !sens) return refuse(fn, "bad argument (state_hist, order, offset, bins and sens must be given)");
  if (check_window(fn, w) || check_groups(fn, G) || check_factors(fn, F, M)) return -1;
  if (term < UMPC_TERM_EP || term > UMPC_TERM_TAU) return refuse(fn, "bad argument (term is UMPC_TERM_EP, UMPC_TERM_ES or UMPC_TERM_TAU)");
  if (term == UMPC_TERM_TAU && !out_hist) return refuse(fn, "UMPC_TERM_TAU needs out_hist (the moments are read from it)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_sensitivity<float>(h, w, order, offset, G, term, bins, F, M, sens, stream)
                              : launch_sensitivity<double>(h, w, order, offset, G, term, bins, F, M, sens, stream);
}
int umpcBatchSensitivityIndices(umpc_batch_t *h, const double *sens, long long count, int G, int F, int M, double *idx, void *stream) {
  const char *fn = "umpcBatchSensitivityIndices";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!sens || !idx) return refuse(fn, "bad argument (sens and idx must be given)");
  if (count < 0 || count > 0x7fffffffLL) return refuse(fn, "bad argument (0 <= count <= 2^31 - 1)");
  if (check_groups(fn, G) || check_factors(fn, F, M)) return -1;
  if (count == 0) return 0;
  const long long rows = count * G, blocks = (rows + umpc::kSensIdxBlock - 1) / umpc::kSensIdxBlock;
  if (blocks > 0x7fffffffLL) return refuse(fn, "count x G too large for one call (2^39 rows at the most)");
  hipLaunchKernelGGL(umpc::umpc_sensitivity_indices_kernel, dim3((unsigned)blocks), dim3(umpc::kSensIdxBlock), 0, (hipStream_t)stream,
                     sens, rows, F, M, idx);
  return launch_status(fn);
}
int umpcBatchScoreSensitivity(umpc_batch_t *h, const void *score, const int32_t *order, const int32_t *offset, int G, int num, int den,
                              const int32_t *bins, int F, int M, double *sens, void *stream) {
  const char *fn = "umpcBatchScoreSensitivity";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!score || !order || !offset || !bins || !sens) return refuse(fn, "bad argument (score, order, offset, bins and sens must be given)");
  if (check_groups(fn, G) || check_factors(fn, F, M) || check_rows(fn, num, den)) return -1;
  return h->dtype == UMPC_F32 ? launch_score_sensitivity<float>(h, score, order, offset, G, num, den, bins, F, M, sens, stream)
                              : launch_score_sensitivity<double>(h, score, order, offset, G, num, den, bins, F, M, sens, stream);
}

int umpcBatchSpectrumInit(umpc_batch_t *h, int K, double *sums, void *stream) {
  const char *fn = "umpcBatchSpectrumInit";
  if (!h || !sums) return refuse(fn, "bad argument (h and sums must be given)");
  if (check_freqs(fn, K)) return -1;
  const hipError_t e = hipMemsetAsync(sums, 0, sizeof(double) * (2 + 3 * (2 + 2 * (size_t)K)) * (size_t)h->B, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(e, fn);
}
int umpcBatchSpectrum(umpc_batch_t *h, int signal, const void *state_hist, const void *out_hist, const void *ref_tab,
                      const void *ref, const double *basis, long long basis_first, int K, long long first, long long count,
                      long long ref_first, int after, double *sums, void *stream) {
  const char *fn = "umpcBatchSpectrum";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (signal < UMPC_SPEC_EP || signal > UMPC_SPEC_U) return refuse(fn, "bad argument (signal is UMPC_SPEC_EP, UMPC_SPEC_ES or UMPC_SPEC_U)");
  if (!basis || !sums) return refuse(fn, "bad argument (basis and sums must be given)");
  if (check_freqs(fn, K)) return -1;
  const bool cmd = signal == UMPC_SPEC_U;
  if (cmd && !out_hist) return refuse(fn, "UMPC_SPEC_U needs out_hist (the command is read from it)");
  if (!cmd && !state_hist) return refuse(fn, "bad argument (state_hist must be given)");
  // (the command has no reference: ref_tab and ref are not read with it)
  const ScoreWindow w = {state_hist, out_hist, nullptr, cmd ? nullptr : ref_tab, cmd ? nullptr : ref, first, count, ref_first, after};
  if (!cmd && check_one_reference(fn, w)) return -1;
  if (count < 0 || first < 0 || ref_first < 0 || basis_first < 0) return refuse(fn, "bad argument (count, first, ref_first, basis_first >= 0)");
  if (count > 0x7fffffffLL - 2 * umpc::kSpecSlices) return refuse(fn, "count too large for one call (2^31 - 5 steps at the most)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_spectrum<float>(h, signal, w, basis, basis_first, K, sums, stream)
                              : launch_spectrum<double>(h, signal, w, basis, basis_first, K, sums, stream);
}
int umpcBatchSpectrumPower(umpc_batch_t *h, const double *sums, const double *wsum, const double *freq_hz, int K, long long nrows,
                           int jsplit, void *power, void *spec, void *stream) {
  const char *fn = "umpcBatchSpectrumPower";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!sums || !wsum || !freq_hz || !power || !spec) return refuse(fn, "bad argument (sums, wsum, freq_hz, power and spec must be given)");
  if (check_freqs(fn, K)) return -1;
  if (nrows < 0 || nrows > (1LL << 53)) return refuse(fn, "bad argument (0 <= nrows <= 2^53)");
  if (jsplit < 0 || jsplit > K) return refuse(fn, "bad argument (0 <= jsplit <= K)");
  return h->dtype == UMPC_F32 ? launch_spectrum_power<float>(h, sums, wsum, freq_hz, K, nrows, jsplit, power, spec, stream)
                              : launch_spectrum_power<double>(h, sums, wsum, freq_hz, K, nrows, jsplit, power, spec, stream);
}
int umpcBatchSpectrumGroups(umpc_batch_t *h, const void *power, const void *spec, const int32_t *order, const int32_t *offset, int G,
                            int K, double *gspec, void *stream) {
  const char *fn = "umpcBatchSpectrumGroups";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!power || !spec || !order || !offset || !gspec) return refuse(fn, "bad argument (power, spec, order, offset and gspec must be given)");
  if (check_groups(fn, G) || check_freqs(fn, K)) return -1;
  return h->dtype == UMPC_F32 ? launch_spectrum_groups<float>(h, power, spec, order, offset, G, K, gspec, stream)
                              : launch_spectrum_groups<double>(h, power, spec, order, offset, G, K, gspec, stream);
}

int umpcBatchCrossSpectrumInit(umpc_batch_t *h, int K, double *xsums, void *stream) {
  const char *fn = "umpcBatchCrossSpectrumInit";
  if (!h || !xsums) return refuse(fn, "bad argument (h and xsums must be given)");
  if (check_freqs(fn, K)) return -1;
  const hipError_t e = hipMemsetAsync(xsums, 0, sizeof(double) * (2 + 6 * (2 + 2 * (size_t)K)) * (size_t)h->B, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(e, fn);
}
int umpcBatchCrossSpectrum(umpc_batch_t *h, int pair, const void *state_hist, const void *ref_tab, const void *ref, const void *imp_tab,
                           const double *basis, long long basis_first, int K, long long first, long long count, long long ref_first,
                           long long imp_first, int after, double *xsums, void *stream) {
  const char *fn = "umpcBatchCrossSpectrum";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (pair < UMPC_XS_TRACK || pair > UMPC_XS_PUSH) return refuse(fn, "bad argument (pair is UMPC_XS_TRACK, UMPC_XS_ATT or UMPC_XS_PUSH)");
  if (!state_hist || !basis || !xsums) return refuse(fn, "bad argument (state_hist, basis and xsums must be given)");
  if (check_freqs(fn, K)) return -1;
  const bool push = pair == UMPC_XS_PUSH;
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (push) {
    if (!imp_tab) return refuse(fn, "UMPC_XS_PUSH needs imp_tab (the input is read from it)");
    if (check_one_reference(fn, w)) return -1;
  } else if (!ref_tab || ref) {
    return refuse(fn, "UMPC_XS_TRACK and UMPC_XS_ATT need ref_tab and no ref (the input is the reference per step: a constant one has no spectrum)");
  }
  if (count < 0 || first < 0 || ref_first < 0 || imp_first < 0 || basis_first < 0)
    return refuse(fn, "bad argument (count, first, ref_first, imp_first, basis_first >= 0)");
  if (count > 0x7fffffffLL - 2 * umpc::kSpecSlices) return refuse(fn, "count too large for one call (2^31 - 5 steps at the most)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_cross_spectrum<float>(h, pair, w, imp_tab, imp_first, basis, basis_first, K, xsums, stream)
                              : launch_cross_spectrum<double>(h, pair, w, imp_tab, imp_first, basis, basis_first, K, xsums, stream);
}
int umpcBatchCrossSpectrumGroups(umpc_batch_t *h, const double *xsums, const double *wsum, int K, long long nrows, const int32_t *order,
                                 const int32_t *offset, int G, double *gx, void *stream) {
  const char *fn = "umpcBatchCrossSpectrumGroups";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!xsums || !wsum || !order || !offset || !gx) return refuse(fn, "bad argument (xsums, wsum, order, offset and gx must be given)");
  if (check_groups(fn, G) || check_freqs(fn, K)) return -1;
  if (nrows < 0 || nrows > (1LL << 53)) return refuse(fn, "bad argument (0 <= nrows <= 2^53)");
  umpc::XsGroupArgs a;
  for (int j = 0; j < 1 + 2 * umpc::kSpecMaxK; ++j) a.wsum[j] = j < 1 + 2 * K ? wsum[j] : 0.0;
  a.sums = xsums; a.order = order; a.offset = offset; a.gx = gx;
  a.nrows = (double)nrows; a.B = h->B; a.K = K;
  const dim3 grid((unsigned)G, 3u, (unsigned)((K + umpc::kXsGroupTile - 1) / umpc::kXsGroupTile));
  hipLaunchKernelGGL(umpc::umpc_xspec_groups_kernel, grid, dim3(64), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}
int umpcBatchTransfer(umpc_batch_t *h, const double *gx, int G, int K, double *tf, void *stream) {
  const char *fn = "umpcBatchTransfer";
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!gx || !tf) return refuse(fn, "bad argument (gx and tf must be given)");
  if (check_groups(fn, G) || check_freqs(fn, K)) return -1;
  const long long rows = (long long)G * 3 * K;
  hipLaunchKernelGGL(umpc::umpc_transfer_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gx, rows, K, tf);
  return launch_status(fn);
}

int umpcBatchGram(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, long long first, long long count,
                  long long ref_first, int after, const int32_t *order, const int32_t *offset, int G, const double *scale,
                  int accumulate, double *gram, void *stream) {
  const char *fn = "umpcBatchGram";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !scale || !gram) return refuse(fn, "bad argument (state_hist, order, offset, scale and gram must be given)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  for (int c = 0; c < 6; ++c)
    if (!(scale[c] >= 0) || !(scale[c] <= 1.79769313486231570815e308)) return refuse(fn, "bad argument (the six scales must be finite and >= 0)");
  if (accumulate != 0 && accumulate != 1) return refuse(fn, "bad argument (accumulate is 0 or 1)");
  if (count == 0 && accumulate) return 0;      // (count == 0 without accumulate writes the table of an empty window)
  return h->dtype == UMPC_F32 ? launch_gram<float>(h, w, order, offset, G, scale, accumulate, gram, stream)
                              : launch_gram<double>(h, w, order, offset, G, scale, accumulate, gram, stream);
}
int umpcBatchProject(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, long long first, long long count,
                     long long ref_first, int after, const int32_t *order, const int32_t *offset, int G, const double *weights, int M,
                     double *proj, void *stream) {
  const char *fn = "umpcBatchProject";
  const ScoreWindow w = {state_hist, nullptr, nullptr, ref_tab, ref, first, count, ref_first, after};
  if (!h) return refuse(fn, "bad argument (no handle)");
  if (!state_hist || !order || !offset || !weights || !proj) return refuse(fn, "bad argument (state_hist, order, offset, weights and proj must be given)");
  if (check_window(fn, w) || check_groups(fn, G)) return -1;
  if (M < 1 || M > UMPC_PROJ_MAX) return refuse(fn, "bad argument (1 <= M <= 4 weight vectors)");
  if (count == 0) return 0;
  return h->dtype == UMPC_F32 ? launch_project<float>(h, w, order, offset, G, weights, M, proj, stream)
                              : launch_project<double>(h, w, order, offset, G, weights, M, proj, stream);
}

}  // extern "C"
