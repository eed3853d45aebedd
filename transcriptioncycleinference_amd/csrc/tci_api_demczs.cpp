// tci_api_demczs.cpp -- the C ABI of the DE-MC(zs) sampler (include/tci.h, tci_demczs_run): every check before any
// device work, the uploads, generation 0, then per generation the proposal kernel, ONE batched likelihood launch on the
// trial buffer under the active mask and the decision kernel (tci_demczs.hip), timed as one stretch, the group
// reductions on the device chain, and the copies of what the caller asked for. tci_demczs_run_bounds is the same run
// (zs_run) with the census' counters and the orientation rows beside it; with both features off no buffer is
// allocated, no kernel launched and no copy made beyond tci_demczs_run_rank's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "tci_api_internal.h"

using namespace tci_api;

namespace {

const char* const kWho = "tci_demczs_run";
const char* const kWhoBounds = "tci_demczs_run_bounds";

std::string at(int64_t k, int64_t j) { return "cell " + std::to_string(k) + ", index " + std::to_string(j); }

// the rows of pop0 ("member") or z0 ("row") of cell k: every entry j < P finite and inside the bounds
int rows_check(tci_ctx* ctx, const std::string& who, const char* name, const char* unit, const double* x, int64_t k,
               int64_t n_rows, int64_t P, int64_t ld, const double* lower, const double* upper) {
  for (int64_t i = 0; i < n_rows; ++i) {
    const double* r = x + (k * n_rows + i) * ld;
    for (int64_t j = 0; j < P; ++j) {
      const bool finite = std::isfinite(r[j]);
      if (finite && r[j] >= lower[k * ld + j] && r[j] <= upper[k * ld + j]) continue;
      return fail(ctx, TCI_EINVAL, who + name + " of cell " + std::to_string(k) + ", " + unit + " " + std::to_string(i) +
                                       ", index " + std::to_string(j) + (finite ? " is outside [lower, upper]" : " is not finite"));
    }
  }
  return TCI_OK;
}

// Every check of a tci_demczs_run call, in the header's order. *keep_k0, *keep_rows: the kept rows the reductions use.
int zs_check(tci_ctx* ctx, const char* entry, const tci_demczs_options& o, const double* pop0, const double* z0, int64_t ld,
             const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower, const double* upper,
             const double* mu, const double* sig, const double* jitter, const double* s2, int64_t log_rows, bool reduce,
             const tci_chainrhat_options* ropt, const tci_chainess_options* eopt, bool ess,
             const tci_chainrank_options* kopt, tci_chainrank_options* k_opt, int64_t* keep_k0, int64_t* keep_rows) {
  const std::string who = std::string(entry) + ": ";
  if (n_sel < 1) return fail(ctx, TCI_EINVAL, who + "n_sel must be >= 1");
  if (o.flags != 0) return fail(ctx, TCI_EINVAL, who + "flags is reserved and must be 0");
  if (o.n_gen < 0) return fail(ctx, TCI_EINVAL, who + "n_gen must be >= 0");
  if (o.thin < 0) return fail(ctx, TCI_EINVAL, who + "thin must be >= 0");
  if (o.jump_every < 0) return fail(ctx, TCI_EINVAL, who + "jump_every must be >= 0");
  if (o.stats_from < 0) return fail(ctx, TCI_EINVAL, who + "stats_from must be >= 0");
  if (o.updatesigma != 0 && o.updatesigma != 1) return fail(ctx, TCI_EINVAL, who + "updatesigma must be 0 or 1");
  if (!(o.CR >= 0.0 && o.CR <= 1.0)) return fail(ctx, TCI_EINVAL, who + "CR must be in [0, 1]");
  if (!std::isfinite(o.gamma0)) return fail(ctx, TCI_EINVAL, who + "gamma0 must be finite");
  if (o.append_every < 1) return fail(ctx, TCI_EINVAL, who + "append_every must be >= 1");
  if (!(o.p_snooker >= 0.0 && o.p_snooker <= 1.0)) return fail(ctx, TCI_EINVAL, who + "p_snooker must be in [0, 1]");
  if (log_rows < 0) return fail(ctx, TCI_EINVAL, who + "log_rows must be >= 0");
  if (n_pop < 1 || n_pop > 4096) return fail(ctx, TCI_EINVAL, who + "n_pop must be in [1, 4096]");
  if (m0 < 3) return fail(ctx, TCI_EINVAL, who + "m0 must be >= 3 (the archive gives three distinct rows)");
  if (n_sel > (((int64_t)1 << 31) - 1) / n_pop) return fail(ctx, TCI_EINVAL, who + "n_sel * n_pop must stay below 2^31");
  if (o.n_gen >= ((int64_t)1 << 31) - 1) return fail(ctx, TCI_EINVAL, who + "n_gen must stay below 2^31 - 1");
  if (m0 >= ((int64_t)1 << 24) || m0 + n_pop * (o.n_gen / o.append_every) >= ((int64_t)1 << 24))
    return fail(ctx, TCI_EINVAL, who + "the archive (m0 + n_pop * (n_gen / append_every) rows) must stay below 2^24 rows");
  if (ld < 1 || ld > ((int64_t)1 << 24)) return fail(ctx, TCI_ERANGE, who + "ld must be in [1, 2^24]");
  for (int64_t k = 0; k < n_sel; ++k) {
    const int32_t c = cell_id[k];
    if (c < 0 || c >= ctx->n_cells)
      return fail(ctx, TCI_ERANGE, who + "cell " + std::to_string(k) + ": cell id " + std::to_string(c) + " out of range");
    if (ld < 7 + ctx->meta[(size_t)c].n)
      return fail(ctx, TCI_ERANGE, who + "cell " + std::to_string(k) + ": theta needs " +
                                       std::to_string(7 + ctx->meta[(size_t)c].n) + " entries (ld=" + std::to_string(ld) + ")");
  }
  for (int64_t k = 0; k < n_sel; ++k) {
    const int64_t N = ctx->meta[(size_t)cell_id[k]].n, P = 7 + N;
    for (int64_t j = 0; j < P; ++j) {
      if (!std::isfinite(mu[k * ld + j])) return fail(ctx, TCI_EINVAL, who + "prior_mu of " + at(k, j) + " is not finite");
      if (!(sig[k * ld + j] > 0)) return fail(ctx, TCI_EINVAL, who + "prior_sig of " + at(k, j) + " is NaN or <= 0");
    }
    for (int64_t j = 0; j < P; ++j)
      if (!std::isfinite(jitter[k * ld + j]) || !(jitter[k * ld + j] >= 0))
        return fail(ctx, TCI_EINVAL, who + "jitter of " + at(k, j) + " is not finite and >= 0");
    if (!std::isfinite(s2[k]) || !(s2[k] > 0))
      return fail(ctx, TCI_EINVAL, who + "sigma2_0 of cell " + std::to_string(k) + " is not finite and > 0");
    if (o.updatesigma && N < 1)
      return fail(ctx, TCI_EINVAL, who + "cell " + std::to_string(k) + ": nobs / 2 must be >= 1 with updatesigma");
  }
  for (int64_t k = 0; k < n_sel; ++k) {
    const int rc = rows_check(ctx, who, "pop0", "member", pop0, k, n_pop, 7 + ctx->meta[(size_t)cell_id[k]].n, ld, lower, upper);
    if (rc != TCI_OK) return rc;
  }
  for (int64_t k = 0; k < n_sel; ++k) {
    const int rc = rows_check(ctx, who, "z0", "row", z0, k, m0, 7 + ctx->meta[(size_t)cell_id[k]].n, ld, lower, upper);
    if (rc != TCI_OK) return rc;
  }
  *keep_k0 = *keep_rows = 0;
  if (reduce) {
    if (o.thin < 1) return fail(ctx, TCI_EINVAL, who + "the group reductions need the kept rows (thin >= 1)");
    *keep_k0 = (o.stats_from + o.thin - 1) / o.thin;
    *keep_rows = o.n_gen / o.thin + 1 - *keep_k0;
    if (*keep_rows < 2)
      return fail(ctx, TCI_EINVAL, who + "fewer than 2 kept rows at or past stats_from (n_rows < 2)");
    if (ropt && ropt->flags != 0) return fail(ctx, TCI_EINVAL, who + "flags is reserved and must be 0");
    if (ess && eopt && eopt->max_lag < 0) return fail(ctx, TCI_EINVAL, who + "max_lag must be >= 0");
    if (ess && eopt && eopt->flags != 0) return fail(ctx, TCI_EINVAL, who + "flags is reserved and must be 0");
    if (k_opt) {
      const int rc = chainrank_opts(ctx, entry, kopt, k_opt);
      if (rc != TCI_OK) return rc;
    }
  }
  return TCI_OK;
}

// The checks of tci_demczs_run_bounds' own arguments, after zs_check and before any device work.
int bounds_check(tci_ctx* ctx, const tci_bounds_options& bo, const tci_bounds_outputs* bout) {
  const std::string who = std::string(kWhoBounds) + ": ";
  if (bo.mode != TCI_BOUNDS_REJECT && bo.mode != TCI_BOUNDS_REFLECT)
    return fail(ctx, TCI_EINVAL, who + "mode must be TCI_BOUNDS_REJECT (0) or TCI_BOUNDS_REFLECT (1)");
  if (bo.census != 0 && bo.census != 1) return fail(ctx, TCI_EINVAL, who + "census must be 0 or 1");
  if (bo.flags != 0) return fail(ctx, TCI_EINVAL, who + "flags is reserved and must be 0");
  if (!bout) return TCI_OK;
  if (!bo.census) {
    const char* f = bout->n_cross ? "n_cross" : bout->oob_lo ? "oob_lo" : bout->oob_hi ? "oob_hi" : bout->n_left ? "n_left" : nullptr;
    if (f) return fail(ctx, TCI_EINVAL, who + f + " is a census output and census is 0");
  }
  if (bo.mode != TCI_BOUNDS_REFLECT) {
    const char* f = bout->n_refl ? "n_refl" : bout->n_reflected ? "n_reflected" : bout->orient ? "orient" : nullptr;
    if (f) return fail(ctx, TCI_EINVAL, who + f + " is a reflection output and mode is TCI_BOUNDS_REJECT");
  }
  return TCI_OK;
}

int zs_run(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
           const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower, const double* upper,
           const double* prior_mu, const double* prior_sig, const double* jitter, const double* sigma2_0,
           tci_demczs_outputs* out, const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout,
           const tci_chainess_options* eopt, tci_chainess_outputs* eout, const tci_chainrank_options* kopt,
           tci_chainrank_outputs* kout, const tci_bounds_options* bopt, tci_bounds_outputs* bout);

}  // namespace

extern "C" {

int tci_demczs_defaults(tci_demczs_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->n_gen = 1000;
  o->thin = 1;
  o->jump_every = 10;
  o->updatesigma = 1;
  o->CR = 0.2;
  o->append_every = 10;
  o->p_snooker = 0.1;
  return TCI_OK;
}

int tci_demczs_run(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                   const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                   const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                   const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                   tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout) {
  return tci_demczs_run_rank(ctx, opt, pop0, z0, ld, cell_id, n_sel, n_pop, m0, lower, upper, prior_mu, prior_sig, jitter,
                             sigma2_0, out, ropt, rout, eopt, eout, nullptr, nullptr);
}

int tci_demczs_run_rank(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                        const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                        const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                        const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                        tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout,
                        const tci_chainrank_options* kopt, tci_chainrank_outputs* kout) {
  return zs_run(ctx, opt, pop0, z0, ld, cell_id, n_sel, n_pop, m0, lower, upper, prior_mu, prior_sig, jitter, sigma2_0, out,
                ropt, rout, eopt, eout, kopt, kout, nullptr, nullptr);
}

int tci_bounds_defaults(tci_bounds_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  return TCI_OK;
}

int tci_demczs_run_bounds(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                          const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                          const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                          const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                          tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout,
                          const tci_chainrank_options* kopt, tci_chainrank_outputs* kout, const tci_bounds_options* bopt,
                          tci_bounds_outputs* bout) {
  return zs_run(ctx, opt, pop0, z0, ld, cell_id, n_sel, n_pop, m0, lower, upper, prior_mu, prior_sig, jitter, sigma2_0, out,
                ropt, rout, eopt, eout, kopt, kout, bopt, bout);
}

}  // extern "C"

namespace {

int zs_run(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
           const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower, const double* upper,
           const double* prior_mu, const double* prior_sig, const double* jitter, const double* sigma2_0,
           tci_demczs_outputs* out, const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout,
           const tci_chainess_options* eopt, tci_chainess_outputs* eout, const tci_chainrank_options* kopt,
           tci_chainrank_outputs* kout, const tci_bounds_options* bopt, tci_bounds_outputs* bout) {
  if (!ctx) return TCI_EINVAL;
  const char* const kWho = bopt || bout ? kWhoBounds : ::kWho;  // the entry point the caller came through
  if (!pop0 || !z0 || !cell_id || !lower || !upper || !prior_mu || !prior_sig || !jitter || !sigma2_0 || !out)
    return fail(ctx, TCI_EINVAL, std::string(kWho) + ": null argument");
  tci_demczs_options o;
  tci_demczs_defaults(&o);
  if (opt) o = *opt;
  const bool reduce = rout || eout || kout;
  tci_chainrank_options k_opt{};
  int64_t keep_k0 = 0, keep_rows = 0;
  int rc = zs_check(ctx, kWho, o, pop0, z0, ld, cell_id, n_sel, n_pop, m0, lower, upper, prior_mu, prior_sig, jitter, sigma2_0,
                    out->log_rows, reduce, ropt, eopt, eout != nullptr, kopt, kout ? &k_opt : nullptr, &keep_k0, &keep_rows);
  if (rc != TCI_OK) return rc;
  tci_bounds_options bo;
  tci_bounds_defaults(&bo);
  if (bopt) bo = *bopt;
  rc = bounds_check(ctx, bo, bout);
  if (rc != TCI_OK) return rc;
  const bool reflect = bo.mode == TCI_BOUNDS_REFLECT, census = bo.census != 0;
  const bool bounds = reflect || census;  // neither: the kernels and the buffers of tci_demczs_run_rank, nothing else
  const tci_bounds_outputs none{};
  const tci_bounds_outputs& bo_out = bout ? *bout : none;

  const size_t n = (size_t)n_sel, L = (size_t)ld, B = n * (size_t)n_pop;
  const int64_t M_cap = m0 + n_pop * (o.n_gen / o.append_every);
  const size_t Mc = (size_t)M_cap;
  const size_t n_keep = o.thin > 0 ? (size_t)(o.n_gen / o.thin) + 1 : 0;
  const bool want_chain = out->chain || out->s2chain || out->sschain || out->prichain || reduce;
  const size_t K = want_chain ? n_keep : 0;  // kept rows the device holds
  const bool want_log = out->logr || out->accepted || out->trial_oob || out->ljac || out->snooker || bo_out.n_left || bo_out.n_refl;
  const size_t G = want_log ? (size_t)std::min<int64_t>(out->log_rows, o.n_gen) : 0;
  const double gamma0 = o.gamma0 > 0.0 ? o.gamma0 : 2.38;

  // the products that grow with n_gen: beyond size_t they cannot fit any device either
  const size_t lim = ~(size_t)0 / sizeof(double);
  if ((K && B * (L + 3) > lim / K) || (G && B > lim / G) || n * L > lim / Mc)
    return fail(ctx, TCI_ENOMEM,
                std::string(kWho) + ": the chain, the archive or the logs (more than 2^64 bytes) do not fit the device");

  std::vector<int32_t> row_cell, npar, nacc, noob, nnull, cens0;
  std::vector<int64_t> keys;
  RhatGroups groups;
  try {
    row_cell.resize(B);
    npar.resize(B);
    nacc.resize(B);
    noob.resize(B);
    nnull.resize(B);
    keys.resize(n);
    if (census) cens0.resize(B * L);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(kWho) + ": host allocation failed");
  }
  for (size_t b = 0; b < B; ++b) {
    row_cell[b] = cell_id[b / (size_t)n_pop];
    npar[b] = 7 + ctx->meta[(size_t)row_cell[b]].n;
  }
  for (size_t k = 0; k < n; ++k) keys[k] = o.keys ? o.keys[k] : (int64_t)k;
  if (census)  // the three counters start at 0, their padding at -1
    for (size_t b = 0; b < B; ++b)
      for (size_t j = 0; j < L; ++j) cens0[b * L + j] = j < (size_t)npar[b] ? 0 : -1;
  if (reduce) {
    std::vector<int32_t> group;
    try {
      group.resize(B);
    } catch (const std::bad_alloc&) {
      return fail(ctx, TCI_ENOMEM, std::string(kWho) + ": host allocation failed");
    }
    for (size_t b = 0; b < B; ++b) group[b] = (int32_t)(b / (size_t)n_pop);
    rc = chainrhat_groups(ctx, kWho, ropt, keep_rows, (int64_t)B, ld, npar.data(), group.data(), n_sel, &groups);
    if (rc != TCI_OK) return rc;
  }

  // every device buffer of the call, as requested below
  const size_t GB = G * B;
  const size_t requested =
      (K * B * (L + 3) + (n * Mc + 2 * B) * L + 6 * B + 5 * n * L + n + (out->logr ? GB : 0) + (out->ljac ? GB : 0)) *
          sizeof(double) +
      2 * B + (out->accepted ? GB : 0) + (out->trial_oob ? GB : 0) + (out->snooker ? GB : 0) +
      (n + 5 * B) * sizeof(int32_t) + n * sizeof(int64_t) +
      (bounds ? 3 * B + (census ? 3 * B * L : 0) + (bo_out.n_left ? GB : 0) + (bo_out.n_refl ? GB : 0) : 0) * sizeof(int32_t) +
      (reflect ? 2 * B * L : 0);
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  auto dalloc = [&](size_t count) { return e == hipSuccess ? A.alloc<double>(count, &e) : nullptr; };
  auto balloc = [&](size_t count) { return e == hipSuccess ? A.alloc<uint8_t>(count, &e) : nullptr; };
  auto ialloc = [&](size_t count) { return e == hipSuccess ? A.alloc<int32_t>(count, &e) : nullptr; };
  double* d_chain = dalloc(K * B * L);
  double* d_kept = dalloc(3 * K * B);  // s2chain, sschain, prichain
  double* d_arch = dalloc(n * Mc * L);
  double* d_pop = dalloc(B * L);
  double* d_trial = dalloc(B * L);
  double* d_row = dalloc(6 * B);        // ss, pri, s2 of the chains, then ss, pri and ljac of the trials
  double* d_cellv = dalloc(5 * n * L);  // lower, upper, mu, sig, jitter
  double* d_s20 = dalloc(n);
  double* d_logr = dalloc(out->logr ? G * B : 0);
  double* d_ljlog = dalloc(out->ljac ? G * B : 0);
  uint8_t* d_flags = balloc(2 * B);  // active, move
  uint8_t* d_acclog = balloc(out->accepted ? G * B : 0);
  uint8_t* d_ooblog = balloc(out->trial_oob ? G * B : 0);
  uint8_t* d_snklog = balloc(out->snooker ? G * B : 0);
  int32_t* d_cell = ialloc(n);
  int32_t* d_rowcell = ialloc(B);
  int32_t* d_npar = ialloc(B);
  int32_t* d_cnt = ialloc(3 * B);  // n_acc, n_oob, n_null
  int64_t* d_keys = e == hipSuccess ? A.alloc<int64_t>(n, &e) : nullptr;
  // tci_demczs_run_bounds' own buffers, each allocated only when its feature is on: with both off the call makes
  // tci_demczs_run_rank's allocations and no other
  int32_t* d_cens = census ? ialloc(3 * B * L) : nullptr;               // n_cross, oob_lo, oob_hi
  int32_t* d_prop = bounds ? ialloc(3 * B) : nullptr;                   // n_left and n_refl of the trials, n_reflected
  int32_t* d_leftlog = bo_out.n_left && G ? ialloc(G * B) : nullptr;
  int32_t* d_refllog = bo_out.n_refl && G ? ialloc(G * B) : nullptr;
  uint8_t* d_orient = reflect ? balloc(2 * B * L) : nullptr;            // of the chains, then of the trials
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(kWho) + ": the populations, the archive and the chain (" +
                                     std::to_string(requested) +
                                     " bytes) do not fit the device");
  }
  double *d_ss = d_row, *d_pri = d_row + B, *d_s2 = d_row + 2 * B, *d_ss_t = d_row + 3 * B, *d_pri_t = d_row + 4 * B,
         *d_lj = d_row + 5 * B;
  double *d_lo = d_cellv, *d_up = d_cellv + n * L, *d_mu = d_cellv + 2 * n * L, *d_sig = d_cellv + 3 * n * L,
         *d_jit = d_cellv + 4 * n * L;
  double *d_s2c = d_kept, *d_ssc = d_kept + K * B, *d_pric = d_kept + 2 * K * B;
  uint8_t *d_active = d_flags, *d_move = d_flags + B;
  int32_t *d_nacc = d_cnt, *d_noob = d_cnt + B, *d_nnull = d_cnt + 2 * B;
  hipStream_t s = ctx->stream;
  const auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); };
  TCI_HIP(ctx, up(d_pop, pop0, B * L * sizeof(double)));
  for (size_t k = 0; k < n; ++k)  // cell k's m0 starting rows lead its M_cap archive rows
    TCI_HIP(ctx, up(d_arch + k * Mc * L, z0 + k * (size_t)m0 * L, (size_t)m0 * L * sizeof(double)));
  TCI_HIP(ctx, up(d_lo, lower, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_up, upper, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_mu, prior_mu, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_sig, prior_sig, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_jit, jitter, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_s20, sigma2_0, n * sizeof(double)));
  TCI_HIP(ctx, up(d_cell, cell_id, n * sizeof(int32_t)));
  TCI_HIP(ctx, up(d_rowcell, row_cell.data(), B * sizeof(int32_t)));
  TCI_HIP(ctx, up(d_npar, npar.data(), B * sizeof(int32_t)));
  TCI_HIP(ctx, up(d_keys, keys.data(), n * sizeof(int64_t)));
  tci::ZsBounds bx{};
  tci::ZsDecideBounds dx{};
  if (bounds) {
    TCI_HIP(ctx, hipMemsetAsync(d_prop, 0, 3 * B * sizeof(int32_t), s));
    bx.reflect = reflect;
    dx.n_left_t = bx.n_left_t = d_prop;
    dx.n_refl_t = bx.n_refl_t = d_prop + B;
    dx.n_reflected = d_prop + 2 * B;
    dx.n_left_log = d_leftlog;
    dx.n_refl_log = d_refllog;
  }
  if (census) {
    for (int c = 0; c < 3; ++c) TCI_HIP(ctx, up(d_cens + (size_t)c * B * L, cens0.data(), B * L * sizeof(int32_t)));
    bx.n_cross = d_cens;
    bx.oob_lo = d_cens + B * L;
    bx.oob_hi = d_cens + 2 * B * L;
  }
  if (reflect) {
    TCI_HIP(ctx, hipMemsetAsync(d_orient, 0, 2 * B * L, s));
    bx.orient = dx.orient = d_orient;
    dx.orient_t = bx.orient_t = d_orient + B * L;
  }

  auto launch = [&]() -> int {
    // generation 0: the prior and the SS of the chains' starts, then s2, the counters and kept row 0
    int rc = tci::launch_zs_propose(ctx->kp, d_cell, d_keys, d_pop, d_arch, d_lo, d_up, d_mu, d_sig, d_jit, n_sel, n_pop, m0,
                                    M_cap, ld, 0, false, o.seed, gamma0, o.CR, o.p_snooker, d_trial, d_pri, d_lj, d_move,
                                    d_active, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, d_pop, ld, d_rowcell, nullptr, (int64_t)B, d_ss, nullptr, 0, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch_zs_decide(ctx->kp, d_cell, d_keys, d_s20, d_trial, d_ss_t, d_pri_t, d_lj, d_move, d_active, n_sel,
                                 n_pop, M_cap, ld, 0, o.seed, o.updatesigma != 0, K ? 0 : -1, -1, -1, d_pop, d_arch, d_ss,
                                 d_pri, d_s2, d_nacc, d_noob, d_nnull, d_chain, d_s2c, d_ssc, d_pric, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, (void*)s);
    for (int64_t g = 1; g <= o.n_gen && rc == TCI_OK; ++g) {
      const bool jump = o.jump_every > 0 && g % o.jump_every == 0;
      const int64_t log_row = (size_t)g <= G ? g - 1 : -1;
      const int64_t keep_row = K && g % o.thin == 0 ? g / o.thin : -1;
      const int64_t M_g = m0 + n_pop * ((g - 1) / o.append_every);
      const int64_t app_row = g % o.append_every == 0 ? M_g : -1;
      rc = tci::launch_zs_propose(ctx->kp, d_cell, d_keys, d_pop, d_arch, d_lo, d_up, d_mu, d_sig, d_jit, n_sel, n_pop, M_g,
                                  M_cap, ld, g, jump, o.seed, gamma0, o.CR, o.p_snooker, d_trial, d_pri_t, d_lj, d_move,
                                  d_active, (void*)s, bounds ? &bx : nullptr);
      // one launch for every chain: a null or out-of-bounds row takes the kernel's inactive-row path
      if (rc == TCI_OK)
        rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, d_trial, ld, d_rowcell, d_active, (int64_t)B, d_ss_t, nullptr, 0,
                         (void*)s);
      if (rc == TCI_OK)
        rc = tci::launch_zs_decide(ctx->kp, d_cell, d_keys, d_s20, d_trial, d_ss_t, d_pri_t, d_lj, d_move, d_active, n_sel,
                                   n_pop, M_cap, ld, g, o.seed, o.updatesigma != 0, keep_row, app_row, log_row, d_pop, d_arch,
                                   d_ss, d_pri, d_s2, d_nacc, d_noob, d_nnull, d_chain, d_s2c, d_ssc, d_pric,
                                   out->logr ? d_logr : nullptr, out->accepted ? d_acclog : nullptr,
                                   out->trial_oob ? d_ooblog : nullptr, out->ljac ? d_ljlog : nullptr,
                                   out->snooker ? d_snklog : nullptr, (void*)s, bounds ? &dx : nullptr);
    }
    return rc;
  };
  float ms = 0.f;
  rc = timed_launch(ctx, kWho, {"DE-MC(zs) kernel launch", "DE-MC(zs) kernels", "DE-MC(zs) copy",
                     "a launch refused sizes the checks had passed (n_sel, n_pop, the archive, ld or the generation)"},
                    launch,
                    {{out->pop, d_pop, B * L * sizeof(double)},
                     {out->ss, d_ss, B * sizeof(double)},
                     {out->s2, d_s2, B * sizeof(double)},
                     {nacc.data(), d_nacc, B * sizeof(int32_t)},
                     {noob.data(), d_noob, B * sizeof(int32_t)},
                     {nnull.data(), d_nnull, B * sizeof(int32_t)},
                     {out->archive, d_arch, n * Mc * L * sizeof(double)},
                     {K ? (void*)out->chain : nullptr, d_chain, K * B * L * sizeof(double)},
                     {K ? (void*)out->s2chain : nullptr, d_s2c, K * B * sizeof(double)},
                     {K ? (void*)out->sschain : nullptr, d_ssc, K * B * sizeof(double)},
                     {K ? (void*)out->prichain : nullptr, d_pric, K * B * sizeof(double)},
                     {G ? (void*)out->logr : nullptr, d_logr, G * B * sizeof(double)},
                     {G ? (void*)out->ljac : nullptr, d_ljlog, G * B * sizeof(double)},
                     {G ? (void*)out->accepted : nullptr, d_acclog, G * B},
                     {G ? (void*)out->trial_oob : nullptr, d_ooblog, G * B},
                     {G ? (void*)out->snooker : nullptr, d_snklog, G * B},
                     {bo_out.n_cross, bx.n_cross, B * L * sizeof(int32_t)},
                     {bo_out.oob_lo, bx.oob_lo, B * L * sizeof(int32_t)},
                     {bo_out.oob_hi, bx.oob_hi, B * L * sizeof(int32_t)},
                     {G ? (void*)bo_out.n_left : nullptr, d_leftlog, G * B * sizeof(int32_t)},
                     {G ? (void*)bo_out.n_refl : nullptr, d_refllog, G * B * sizeof(int32_t)},
                     {bo_out.n_reflected, dx.n_reflected, B * sizeof(int32_t)},
                     {bo_out.orient, d_orient, B * L}},
                    &ms);
  if (rc != TCI_OK) return rc;
  for (size_t b = 0; b < B; ++b) {
    if (out->accept_rate) out->accept_rate[b] = o.n_gen > 0 ? (double)nacc[b] / (double)o.n_gen : NAN;
    if (out->n_oob) out->n_oob[b] = noob[b];
    if (out->n_null) out->n_null[b] = nnull[b];
    if (out->n_evals) out->n_evals[b] = 1 + o.n_gen - (int64_t)noob[b] - (int64_t)nnull[b];
  }
  out->n_keep = (int64_t)n_keep;
  out->n_archive = M_cap;
  out->kernel_ms = ms;
  if (rout || eout) {
    rc = chainrhat_device(ctx, kWho, d_chain + (size_t)keep_k0 * B * L, d_s2c + (size_t)keep_k0 * B, keep_rows, (int64_t)B,
                          ld, d_npar, groups, n_sel, rout, eout && eopt ? eopt->max_lag : 0, eout);
    if (rc != TCI_OK) return rc;
  }
  if (kout)
    return chainrank_device(ctx, kWho, d_chain + (size_t)keep_k0 * B * L, d_s2c + (size_t)keep_k0 * B, keep_rows, (int64_t)B,
                            ld, d_npar, groups, n_sel, k_opt, kout);
  return TCI_OK;
}

}  // namespace
