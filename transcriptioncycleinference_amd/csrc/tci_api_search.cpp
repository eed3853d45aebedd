// tci_api_search.cpp -- the C ABI of the mode search (include/tci.h, tci_modesearch): every check before any device
// work, the uploads, then per generation the trial kernel, the batched likelihood kernel on the trial buffer and the
// selection kernel (tci_modesearch.hip), timed as one stretch, and the copies of what the caller asked for.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "tci_api_internal.h"

using namespace tci_api;

namespace {

const char* const kWho = "tci_modesearch";

std::string at(int64_t k, int64_t j) { return "cell " + std::to_string(k) + ", index " + std::to_string(j); }

// Every check of a tci_modesearch call, in the header's order.
int search_check(tci_ctx* ctx, const tci_modesearch_options& o, const double* pop0, int64_t ld, const int32_t* cell_id,
                 int64_t n_sel, int64_t n_pop, const double* lower, const double* upper, const double* mu,
                 const double* sig, const double* s2) {
  const std::string who = std::string(kWho) + ": ";
  if (n_sel < 1) return fail(ctx, TCI_EINVAL, who + "n_sel must be >= 1");
  if (o.flags != 0) return fail(ctx, TCI_EINVAL, who + "flags is reserved and must be 0");
  if (o.n_gen < 0) return fail(ctx, TCI_EINVAL, who + "n_gen must be >= 0");
  if (!std::isfinite(o.F) || !(o.F > 0.0 && o.F <= 2.0)) return fail(ctx, TCI_EINVAL, who + "F must be finite and in (0, 2]");
  if (!(o.CR >= 0.0 && o.CR <= 1.0)) return fail(ctx, TCI_EINVAL, who + "CR must be in [0, 1]");
  if (n_pop < 4 || n_pop > 4096) return fail(ctx, TCI_EINVAL, who + "n_pop must be in [4, 4096]");
  if (n_sel > (((int64_t)1 << 31) - 1) / n_pop) return fail(ctx, TCI_EINVAL, who + "n_sel * n_pop must stay below 2^31");
  if (ld < 1 || ld > ((int64_t)1 << 24)) return fail(ctx, TCI_ERANGE, who + "ld must be in [1, 2^24]");
  if (o.n_gen >= ((int64_t)1 << 31) / n_sel) return fail(ctx, TCI_EINVAL, who + "(n_gen + 1) * n_sel must stay below 2^31");
  for (int64_t k = 0; k < n_sel; ++k) {
    const int32_t c = cell_id[k];
    if (c < 0 || c >= ctx->n_cells)
      return fail(ctx, TCI_ERANGE, who + "cell " + std::to_string(k) + ": cell id " + std::to_string(c) + " out of range");
    if (ld < 7 + ctx->meta[(size_t)c].n)
      return fail(ctx, TCI_ERANGE, who + "cell " + std::to_string(k) + ": theta needs " +
                                       std::to_string(7 + ctx->meta[(size_t)c].n) + " entries (ld=" + std::to_string(ld) + ")");
  }
  for (int64_t k = 0; k < n_sel; ++k) {
    const int64_t P = 7 + ctx->meta[(size_t)cell_id[k]].n;
    for (int64_t j = 0; j < P; ++j) {
      if (!std::isfinite(mu[k * ld + j])) return fail(ctx, TCI_EINVAL, who + "prior_mu of " + at(k, j) + " is not finite");
      if (!(sig[k * ld + j] > 0)) return fail(ctx, TCI_EINVAL, who + "prior_sig of " + at(k, j) + " is NaN or <= 0");
    }
    if (!std::isfinite(s2[k]) || !(s2[k] > 0))
      return fail(ctx, TCI_EINVAL, who + "s2 of cell " + std::to_string(k) + " is not finite and > 0");
  }
  for (int64_t k = 0; k < n_sel; ++k) {
    const int64_t P = 7 + ctx->meta[(size_t)cell_id[k]].n;
    for (int64_t i = 0; i < n_pop; ++i) {
      const double* x = pop0 + (k * n_pop + i) * ld;
      for (int64_t j = 0; j < P; ++j) {
        const bool finite = std::isfinite(x[j]);
        if (finite && x[j] >= lower[k * ld + j] && x[j] <= upper[k * ld + j]) continue;
        return fail(ctx, TCI_EINVAL, who + "pop0 of cell " + std::to_string(k) + ", member " + std::to_string(i) + ", index " +
                                         std::to_string(j) + (finite ? " is outside [lower, upper]" : " is not finite"));
      }
    }
  }
  return TCI_OK;
}

}  // namespace

extern "C" {

int tci_modesearch_defaults(tci_modesearch_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->n_gen = 500;
  o->F = 0.5;
  o->CR = 0.9;
  return TCI_OK;
}

int tci_modesearch(tci_ctx* ctx, const tci_modesearch_options* opt, const double* pop0, int64_t ld,
                   const int32_t* cell_id, int64_t n_sel, int64_t n_pop, const double* lower, const double* upper,
                   const double* prior_mu, const double* prior_sig, const double* s2, tci_modesearch_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!pop0 || !cell_id || !lower || !upper || !prior_mu || !prior_sig || !s2 || !out)
    return fail(ctx, TCI_EINVAL, std::string(kWho) + ": null argument");
  tci_modesearch_options o;
  tci_modesearch_defaults(&o);
  if (opt) o = *opt;
  int rc = search_check(ctx, o, pop0, ld, cell_id, n_sel, n_pop, lower, upper, prior_mu, prior_sig, s2);
  if (rc != TCI_OK) return rc;

  const size_t n = (size_t)n_sel, L = (size_t)ld, B = n * (size_t)n_pop, G = (size_t)o.n_gen;
  std::vector<int32_t> row_cell;
  std::vector<int64_t> keys;
  std::vector<double> best_vals;
  try {
    row_cell.resize(B);
    keys.resize(n);
    best_vals.resize(3 * n);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(kWho) + ": host allocation failed");
  }
  for (size_t b = 0; b < B; ++b) row_cell[b] = cell_id[b / (size_t)n_pop];
  for (size_t k = 0; k < n; ++k) keys[k] = o.keys ? o.keys[k] : (int64_t)k;

  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  auto dalloc = [&](size_t count) { return e == hipSuccess ? A.alloc<double>(count, &e) : nullptr; };
  double* d_pop = dalloc(B * L);
  double* d_trial = dalloc(B * L);
  double* d_row = dalloc(5 * B);  // f, ss, pri of the population, then ss and pri of the trials
  double* d_cellv = dalloc(4 * n * L);  // lower, upper, mu, sig
  double* d_s2 = dalloc(n);
  double* d_trace = dalloc((G + 1) * n);
  double* d_bvals = dalloc(3 * n);
  double* d_tb = dalloc(n * L);
  int32_t* d_cell = e == hipSuccess ? A.alloc<int32_t>(n, &e) : nullptr;
  int32_t* d_rowcell = e == hipSuccess ? A.alloc<int32_t>(B, &e) : nullptr;
  int32_t* d_best = e == hipSuccess ? A.alloc<int32_t>(n, &e) : nullptr;
  int32_t* d_nacc = e == hipSuccess ? A.alloc<int32_t>(G * n, &e) : nullptr;
  int64_t* d_keys = e == hipSuccess ? A.alloc<int64_t>(n, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(kWho) + ": the populations (" + std::to_string(2 * B * L * sizeof(double)) +
                                     " bytes) do not fit the device");
  }
  double *d_f = d_row, *d_ss = d_row + B, *d_pri = d_row + 2 * B, *d_ss_t = d_row + 3 * B, *d_pri_t = d_row + 4 * B;
  double *d_lo = d_cellv, *d_up = d_cellv + n * L, *d_mu = d_cellv + 2 * n * L, *d_sig = d_cellv + 3 * n * L;
  hipStream_t s = ctx->stream;
  const auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); };
  TCI_HIP(ctx, up(d_pop, pop0, B * L * sizeof(double)));
  TCI_HIP(ctx, up(d_lo, lower, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_up, upper, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_mu, prior_mu, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_sig, prior_sig, n * L * sizeof(double)));
  TCI_HIP(ctx, up(d_s2, s2, n * sizeof(double)));
  TCI_HIP(ctx, up(d_cell, cell_id, n * sizeof(int32_t)));
  TCI_HIP(ctx, up(d_rowcell, row_cell.data(), B * sizeof(int32_t)));
  TCI_HIP(ctx, up(d_keys, keys.data(), n * sizeof(int64_t)));

  auto launch = [&]() -> int {
    int rc = TCI_OK;
    for (int64_t g = 0; g <= o.n_gen && rc == TCI_OK; ++g) {
      const bool init = g == 0;
      // generation 0 evaluates the population itself; a later one its trials
      rc = tci::launch_modesearch_trial(ctx->kp, d_cell, d_keys, d_pop, d_lo, d_up, d_mu, d_sig, n_sel, n_pop, ld, g, o.seed,
                                        o.F, o.CR, d_trial, init ? d_pri : d_pri_t, (void*)s);
      if (rc == TCI_OK)
        rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, init ? d_pop : d_trial, ld, d_rowcell, nullptr, (int64_t)B,
                         init ? d_ss : d_ss_t, nullptr, 0, (void*)s);
      if (rc == TCI_OK)
        rc = tci::launch_modesearch_select(ctx->kp, d_cell, d_s2, d_trial, d_ss_t, d_pri_t, n_sel, n_pop, ld, g, g == o.n_gen,
                                           d_pop, d_f, d_ss, d_pri, d_trace + (size_t)g * n,
                                           init ? nullptr : d_nacc + (size_t)(g - 1) * n, d_best, d_bvals, d_tb, (void*)s);
    }
    return rc;
  };
  float ms = 0.f;
  rc = timed_launch(ctx, kWho, {"mode search kernel launch", "mode search kernels", "mode search copy",
                     "a launch refused sizes the checks had passed (n_sel, n_pop, ld or the generation)"}, launch,
                    {{out->pop, d_pop, B * L * sizeof(double)},
                     {out->f, d_f, B * sizeof(double)},
                     {out->ss, d_ss, B * sizeof(double)},
                     {out->best, d_best, n * sizeof(int32_t)},
                     {out->theta_best, d_tb, n * L * sizeof(double)},
                     {best_vals.data(), d_bvals, 3 * n * sizeof(double)},
                     {out->f_trace, d_trace, (G + 1) * n * sizeof(double)},
                     {G ? (void*)out->n_accepted : nullptr, d_nacc, G * n * sizeof(int32_t)}},
                    &ms);
  if (rc != TCI_OK) return rc;
  double* dst[3] = {out->f_best, out->ss_best, out->pri_best};
  for (int q = 0; q < 3; ++q)
    if (dst[q]) std::memcpy(dst[q], best_vals.data() + (size_t)q * n, n * sizeof(double));
  out->n_evals = (int64_t)B * (o.n_gen + 1);
  out->kernel_ms = ms;
  return TCI_OK;
}

}  // extern "C"
