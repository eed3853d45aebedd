// tci_api_chain.cpp -- C ABI (include/tci.h): the reductions of a stored chain. The chain*_device helpers run one
// reduction on a chain that is on the device already (the sampler's kept rows, tci_api_dram.cpp, or a host chain the
// stand-alone tci_chain* entry points below upload first).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "tci_api_internal.h"

namespace tci_api {

// The statistics kernels on a device chain (launch_chainstats), timed with HIP events, and their results
// scattered into the caller's host buffers (d_npar null: ld columns for every chain).
int chainstats_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                      int64_t n_chains, int64_t ld, const int32_t* d_npar, int64_t max_lag, tci_chainstats_outputs* out) {
  const size_t ldc = (size_t)ld + 1, plane = (size_t)n_chains * ldc;
  DevAllocs A;
  hipError_t e = hipSuccess;
  double* d_stats = A.alloc<double>(5 * plane, &e);
  if (e != hipSuccess) return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the statistics failed");
  int32_t* d_win = A.alloc<int32_t>(plane, &e);
  if (e != hipSuccess) return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the statistics failed");
  std::vector<double> hs;
  std::vector<int32_t> hw;
  try {
    hs.resize(4 * plane);
    hw.resize(plane);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  float ms = 0.f;
  const int rc = timed_launch(
      ctx, who, {"chain statistics kernel launch", "chain statistics kernels", "chain statistics copy"},
      [&] {
        return tci::launch_chainstats(d_chain, d_s2, n_rows, n_chains, ld, d_npar, max_lag, d_stats, d_win,
                                      (void*)ctx->stream);
      },
      {{hs.data(), d_stats, 4 * plane * sizeof(double)}, {hw.data(), d_win, plane * sizeof(int32_t)}}, &ms);
  if (rc != TCI_OK) return rc;
  double* dst[4] = {out->mcerr, out->tau, out->geweke_z, out->geweke_p};
  double* dst2[4] = {out->s2_mcerr, out->s2_tau, out->s2_geweke_z, out->s2_geweke_p};
  for (int64_t c = 0; c < n_chains; ++c) {
    const size_t o = (size_t)c * ldc;
    for (int k = 0; k < 4; ++k) {
      if (dst[k]) std::memcpy(dst[k] + (size_t)c * (size_t)ld, hs.data() + (size_t)k * plane + o, (size_t)ld * sizeof(double));
      if (dst2[k]) dst2[k][c] = hs[(size_t)k * plane + o + (size_t)ld];
    }
    if (out->tau_window) std::memcpy(out->tau_window + (size_t)c * (size_t)ld, hw.data() + o, (size_t)ld * sizeof(int32_t));
    if (out->s2_tau_window) out->s2_tau_window[c] = hw[o + (size_t)ld];
  }
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  return TCI_OK;
}

// Checks of tci_chaincov_options against ld, before any device work: the chains per group through the scratch.
int chaincov_group(tci_ctx* ctx, const char* who, const tci_chaincov_options* copt, int64_t n_chains, int64_t ld,
                   int64_t* group) {
  const int64_t sb = copt ? copt->scratch_bytes : 0;
  if (sb < 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": scratch_bytes must be >= 0");
  if (ld > ((int64_t)1 << 24)) return fail(ctx, TCI_ERANGE, std::string(who) + ": ld above 2^24");
  const int64_t cap = sb > 0 ? sb : (int64_t)1 << 30;
  const int64_t per_chain = 2 * ld * ld * (int64_t)sizeof(double);  // <= 2^52
  if (per_chain > cap)
    return fail(ctx, TCI_EINVAL, std::string(who) + ": one chain needs " + std::to_string(per_chain) +
                                     " bytes of scratch (2 x ld x ld doubles), scratch_bytes allows " +
                                     std::to_string(cap));
  *group = std::min(std::min(cap / per_chain, tci::chaincov_max_chains(ld)), n_chains);
  return TCI_OK;
}

// The covariance kernels on a device chain (launch_chaincov), `group` chains at a time through the context's
// scratch, timed with HIP events; every group's matrices are copied straight into the caller's host buffers.
int chaincov_device(tci_ctx* ctx, const char* who, const double* d_chain, int64_t n_rows, int64_t n_chains, int64_t ld,
                    const int32_t* d_npar, int64_t group, tci_chaincov_outputs* out) {
  const size_t L = (size_t)ld, L2 = L * L;
  int rc = ensure(ctx, &ctx->d_cov, &ctx->cap_cov, 2 * (size_t)group * L2);
  if (rc != TCI_OK) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the matrices failed");
  }
  DevAllocs A;
  hipError_t e = hipSuccess;
  double* d_mean = A.alloc<double>((size_t)n_chains * L, &e);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the means failed");
  }
  hipStream_t s = ctx->stream;
  EventTimer timer;
  const char* what_create = nullptr;
  if ((e = timer.create(&what_create)) != hipSuccess) return hip_fail(ctx, e, what_create);
  double total_ms = 0.0;
  hipError_t e1 = hipSuccess;
  rc = TCI_OK;
  for (int64_t c0 = 0; c0 < n_chains && rc == TCI_OK && e1 == hipSuccess; c0 += group) {
    const int64_t nc = std::min(group, n_chains - c0);
    double* d_cv = ctx->d_cov;
    double* d_cr = ctx->d_cov + (size_t)nc * L2;
    e1 = timer.start(s);
    if (e1 != hipSuccess) break;
    rc = tci::launch_chaincov(d_chain, n_rows, n_chains, ld, d_npar, c0, nc, d_mean, d_cv, d_cr, (void*)s);
    e1 = timer.stop(s);
    const size_t o = (size_t)c0 * L2, nb = (size_t)nc * L2 * sizeof(double);
    if (rc == TCI_OK && e1 == hipSuccess && out->cov) e1 = hipMemcpyAsync(out->cov + o, d_cv, nb, hipMemcpyDeviceToHost, s);
    if (rc == TCI_OK && e1 == hipSuccess && out->corr) e1 = hipMemcpyAsync(out->corr + o, d_cr, nb, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // the scratch is reused by the next group
    if (e1 == hipSuccess) e1 = e2;
    float ms = 0.f;
    if (rc == TCI_OK && e1 == hipSuccess) e1 = timer.elapsed_ms(&ms);
    total_ms += ms;
  }
  if (rc == TCI_OK && e1 == hipSuccess && out->mean)
    e1 = hipMemcpy(out->mean, d_mean, (size_t)n_chains * L * sizeof(double), hipMemcpyDeviceToHost);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain covariance kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain covariance kernels");
  out->n_rows = n_rows;
  out->kernel_ms = total_ms;
  return TCI_OK;
}

// Checks of tci_chainquant_options before any device work; *probs, *nq: the probs to use (the defaults for null).
int chainquant_probs(tci_ctx* ctx, const char* who, const tci_chainquant_options* qopt, int64_t n_chains, int64_t ld,
                     const double** probs, int32_t* nq) {
  static const double def[3] = {0.025, 0.5, 0.975};
  *probs = qopt ? qopt->probs : def;
  *nq = qopt ? qopt->nq : 3;
  if (*nq < 1 || *nq > 16) return fail(ctx, TCI_EINVAL, std::string(who) + ": nq must be in [1, 16]");
  for (int32_t q = 0; q < *nq; ++q)
    if (!((*probs)[q] >= 0.0 && (*probs)[q] <= 1.0))
      return fail(ctx, TCI_EINVAL, std::string(who) + ": probs[" + std::to_string(q) + "] is not in [0, 1]");
  if (ld > ((int64_t)1 << 24) || n_chains > ((int64_t)1 << 30) / ((ld + 64) / 64))
    return fail(ctx, TCI_ERANGE, std::string(who) + ": ld above 2^24, or n_chains x ceil((ld + 1) / 64) above 2^30");
  return TCI_OK;
}

// The selection kernel on a device chain (launch_chainquant), timed with HIP events, and its results scattered
// into the caller's host buffers (d_npar null: ld columns for every chain; d_s2 null: s2_q is NaN).
int chainquant_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                      int64_t n_chains, int64_t ld, const int32_t* d_npar, const double* probs, int32_t nq,
                      tci_chainquant_outputs* out) {
  const size_t ldc = (size_t)ld + 1, total = (size_t)n_chains * (size_t)nq * ldc;
  DevAllocs A;
  hipError_t e = hipSuccess;
  double* d_q = A.alloc<double>(total, &e);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the quantiles failed");
  }
  std::vector<double> hq;
  try {
    hq.resize(total);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  float ms = 0.f;
  const int rc = timed_launch(
      ctx, who, {"chain quantile kernel launch", "chain quantile kernel", "chain quantile copy"},
      [&] {
        return tci::launch_chainquant(d_chain, d_s2, n_rows, n_chains, ld, d_npar, probs, nq, d_q, (void*)ctx->stream);
      },
      {{hq.data(), d_q, total * sizeof(double)}}, &ms);
  if (rc != TCI_OK) return rc;
  for (size_t cq = 0; cq < (size_t)n_chains * (size_t)nq; ++cq) {
    if (out->q) std::memcpy(out->q + cq * (size_t)ld, hq.data() + cq * ldc, (size_t)ld * sizeof(double));
    if (out->s2_q) out->s2_q[cq] = hq[cq * ldc + (size_t)ld];
  }
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  return TCI_OK;
}

// Checks of tci_chaindens_options and of the sizes before any device work; *G, *B, *bw_scale: the options to use (the
// defaults for null), *scratch: the bytes launch_chaindens needs.
int chaindens_opts(tci_ctx* ctx, const char* who, const tci_chaindens_options* dopt, int64_t n_rows, int64_t n_chains,
                   int64_t ld, int32_t* G, int32_t* B, double* bw_scale, size_t* scratch) {
  *G = dopt ? dopt->n_grid : 100;
  *B = dopt ? dopt->n_bins : 20;
  *bw_scale = dopt ? dopt->bw_scale : 1.0;
  if (*G < 2 || *G > 256) return fail(ctx, TCI_EINVAL, std::string(who) + ": n_grid must be in [2, 256]");
  if (*B < 1 || *B > 256) return fail(ctx, TCI_EINVAL, std::string(who) + ": n_bins must be in [1, 256]");
  if (!(*bw_scale > 0.0) || !std::isfinite(*bw_scale))
    return fail(ctx, TCI_EINVAL, std::string(who) + ": bw_scale must be finite and > 0");
  if (n_rows < 2) return fail(ctx, TCI_EINVAL, std::string(who) + ": fewer than 2 rows (n_rows < 2)");
  if (n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30) || ld > ((int64_t)1 << 24))
    return fail(ctx, TCI_ERANGE, std::string(who) + ": n_rows or n_chains above 2^30, or ld above 2^24");
  const int rc = tci::chaindens_scratch_bytes(n_rows, n_chains, ld, *G, *B, scratch);
  if (rc == TCI_ENOMEM)
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": the per-segment partial sums are larger than any device memory");
  if (rc != TCI_OK)
    return fail(ctx, TCI_ERANGE, std::string(who) + ": rows x chains x ld too large for one launch (2^31 workgroups)");
  return TCI_OK;
}

// The density kernels on a device chain (launch_chaindens), timed with HIP events, and their results scattered
// into the caller's host buffers (d_npar null: ld columns for every chain; d_s2 null: the s2 twins are NaN / -1).
int chaindens_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, int32_t G, int32_t B, double bw_scale,
                     size_t scratch, tci_chaindens_outputs* out) {
  const size_t ldc = (size_t)ld + 1, n = (size_t)n_chains, L = (size_t)ld;
  const size_t nd = n * (size_t)(G + 3) * ldc, nc = n * (size_t)B * ldc;
  DevAllocs A;
  hipError_t e = hipSuccess;
  void* d_scratch = A.alloc<uint8_t>(scratch, &e);
  double* d_d = e == hipSuccess ? A.alloc<double>(nd, &e) : nullptr;
  int32_t* d_c = e == hipSuccess ? A.alloc<int32_t>(nc, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the densities (" +
                                     std::to_string(scratch + nd * sizeof(double) + nc * sizeof(int32_t)) + " bytes) failed");
  }
  std::vector<double> hd;
  std::vector<int32_t> hc;
  try {
    hd.resize(nd);
    hc.resize(nc);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  float ms = 0.f;
  const int rc = timed_launch(
      ctx, who, {"chain density kernel launch", "chain density kernels", "chain density copy"},
      [&] {
        return tci::launch_chaindens(d_chain, d_s2, n_rows, n_chains, ld, d_npar, G, B, bw_scale,
                                     std::pow((double)n_rows, -0.2), d_scratch, d_d, d_c, (void*)ctx->stream);
      },
      {{hd.data(), d_d, nd * sizeof(double)}, {hc.data(), d_c, nc * sizeof(int32_t)}}, &ms);
  if (rc != TCI_OK) return rc;
  const size_t g = (size_t)G, b = (size_t)B;
  for (size_t c = 0; c < n; ++c) {
    const double* src = hd.data() + c * (g + 3) * ldc;  // G density rows, xmin, xmax, bw
    for (size_t k = 0; k < g; ++k) {
      if (out->dens) std::memcpy(out->dens + (c * g + k) * L, src + k * ldc, L * sizeof(double));
      if (out->s2_dens) out->s2_dens[c * g + k] = src[k * ldc + L];
    }
    for (size_t k = 0; k < 2; ++k) {
      if (out->range) std::memcpy(out->range + (c * 2 + k) * L, src + (g + k) * ldc, L * sizeof(double));
      if (out->s2_range) out->s2_range[c * 2 + k] = src[(g + k) * ldc + L];
    }
    if (out->bw) std::memcpy(out->bw + c * L, src + (g + 2) * ldc, L * sizeof(double));
    if (out->s2_bw) out->s2_bw[c] = src[(g + 2) * ldc + L];
    for (size_t k = 0; k < b; ++k) {
      if (out->counts) std::memcpy(out->counts + (c * b + k) * L, hc.data() + (c * b + k) * ldc, L * sizeof(int32_t));
      if (out->s2_counts) out->s2_counts[c * b + k] = hc[(c * b + k) * ldc + L];
    }
  }
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  return TCI_OK;
}

// Checks of a tci_chainlp call before any device work (the cell ids and ld are check_rows'): the options, the sizes
// and the priors of every chain's P = 7 + N entries.
int chainlp_check(tci_ctx* ctx, const char* who, const tci_chainlp_options* lopt, int64_t n_rows, int64_t n_chains,
                  int64_t ld, const int32_t* cell_id, const double* prior_mu, const double* prior_sig, size_t* scratch) {
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, std::string(who) + ": n_rows must be >= 1");
  if (lopt && lopt->flags != 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": flags is reserved and must be 0");
  int rc = check_rows(ctx, ld, cell_id, n_chains);
  if (rc != TCI_OK) return rc;
  rc = tci::chainlp_scratch_bytes(n_rows, n_chains, ld, scratch);
  if (rc != TCI_OK)
    return fail(ctx, rc, std::string(who) + ": n_rows * n_chains must stay below 2^31 (n_rows and n_chains at most 2^30, ld 2^24)");
  for (int64_t c = 0; c < n_chains; ++c) {
    const int64_t P = 7 + ctx->meta[(size_t)cell_id[c]].n;
    for (int64_t j = 0; j < P; ++j) {
      const double m = prior_mu[c * ld + j], s = prior_sig[c * ld + j];
      if (!std::isfinite(m))
        return fail(ctx, TCI_EINVAL, std::string(who) + ": prior_mu of chain " + std::to_string(c) + ", index " +
                                         std::to_string(j) + " is not finite");
      if (!(s > 0))
        return fail(ctx, TCI_EINVAL, std::string(who) + ": prior_sig of chain " + std::to_string(c) + ", index " +
                                         std::to_string(j) + " is NaN or <= 0");
    }
  }
  return TCI_OK;
}

// The log-posterior kernels on a device chain (tci_chainlp.hip) with the two likelihood launches between them, timed
// with HIP events, and their results copied into the caller's host buffers. d_cell, d_npar (= 7 + N), d_mu and d_sig
// are the chains' (device); scratch: chainlp_check's.
int chainlp_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                   int64_t n_chains, int64_t ld, const int32_t* d_cell, const int32_t* d_npar, const double* d_mu,
                   const double* d_sig, size_t scratch, tci_chainlp_outputs* out) {
  const size_t n = (size_t)n_chains, L = (size_t)ld, B = (size_t)n_rows * n;
  const int K = tci::kChainlpScalars;
  DevAllocs A;
  hipError_t e = hipSuccess;
  int32_t* d_rowcell = A.alloc<int32_t>(B, &e);
  double* d_tr = e == hipSuccess ? A.alloc<double>(4 * B, &e) : nullptr;  // ss, pri, dev, lp
  double* d_scal = e == hipSuccess ? A.alloc<double>((size_t)K * n, &e) : nullptr;
  int64_t* d_best = e == hipSuccess ? A.alloc<int64_t>(n, &e) : nullptr;
  double* d_tb = e == hipSuccess ? A.alloc<double>(n * L, &e) : nullptr;
  double* d_tm = e == hipSuccess ? A.alloc<double>(n * L, &e) : nullptr;
  char* d_scr = e == hipSuccess ? A.alloc<char>(scratch, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the traces failed");
  }
  std::vector<double> hs;
  try {
    hs.resize((size_t)K * n);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  double *d_ss = d_tr, *d_pri = d_tr + B, *d_dev = d_tr + 2 * B, *d_lp = d_tr + 3 * B;
  hipStream_t s = ctx->stream;
  auto launch = [&]() -> int {
    // the SS of every kept row: one launch of the batched likelihood kernel straight on the chain
    int rc = tci::launch_chainlp_ids(d_cell, n_rows, n_chains, d_rowcell, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, d_chain, ld, d_rowcell, nullptr, (int64_t)B, d_ss, nullptr, 0, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch_chainlp_rows(ctx->kp, d_chain, d_s2, d_ss, d_cell, d_mu, d_sig, n_rows, n_chains, ld, d_pri, d_dev,
                                    d_lp, (void*)s);
    // the means through tci_chaincov's mean kernel (s2: a chain of one column), then the SS of the mean rows
    if (rc == TCI_OK) rc = tci::launch_chain_mean(d_chain, n_rows, n_chains, ld, d_npar, d_tm, (void*)s);
    if (rc == TCI_OK) rc = tci::launch_chain_mean(d_s2, n_rows, n_chains, 1, nullptr, d_scal + 7 * n, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, d_tm, ld, d_cell, nullptr, n_chains, d_scal + 8 * n, nullptr, 0, (void*)s);
    if (rc == TCI_OK)
      rc = tci::launch_chainlp_reduce(ctx->kp, d_chain, d_s2, d_ss, d_pri, d_dev, d_lp, d_cell, n_rows, n_chains, ld, d_scr,
                                      d_scal, d_best, d_tb, d_tm, (void*)s);
    return rc;
  };
  float ms = 0.f;
  const int rc = timed_launch(ctx, who, {"log-posterior kernel launch", "log-posterior kernels", "log-posterior copy"}, launch,
                              {{out->ss, d_ss, B * sizeof(double)},  // a trace the caller does not ask for is not copied
                               {out->pri, d_pri, B * sizeof(double)},
                               {out->dev, d_dev, B * sizeof(double)},
                               {out->lp, d_lp, B * sizeof(double)},
                               {hs.data(), d_scal, (size_t)K * n * sizeof(double)},
                               {out->best_row, d_best, n * sizeof(int64_t)},
                               {out->theta_best, d_tb, n * L * sizeof(double)},
                               {out->theta_mean, d_tm, n * L * sizeof(double)}},
                              &ms);
  if (rc != TCI_OK) return rc;
  double* dst[tci::kChainlpScalars] = {out->ss_min,  out->ss_mean, out->dev_mean, out->dev_var, out->lp_best,
                                       out->ss_best, out->s2_best, out->s2_mean,  out->ss_hat,  out->d_hat,
                                       out->p_d,     out->p_v,     out->dic};
  for (int k = 0; k < K; ++k)
    if (dst[k]) std::memcpy(dst[k], hs.data() + (size_t)k * n, n * sizeof(double));
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  return TCI_OK;
}

int chainrhat_groups(tci_ctx* ctx, const char* who, const tci_chainrhat_options* ropt, int64_t n_rows, int64_t n_chains,
                     int64_t ld, const int32_t* npar, const int32_t* group, int64_t n_groups, RhatGroups* G) {
  if (ropt && ropt->flags != 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": flags is reserved and must be 0");
  if (n_groups < 1) return fail(ctx, TCI_EINVAL, std::string(who) + ": n_groups must be >= 1");
  if (n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30) || ld > ((int64_t)1 << 24))
    return fail(ctx, TCI_ERANGE, std::string(who) + ": n_rows or n_chains above 2^30, or ld above 2^24");
  if (group)
    for (int64_t c = 0; c < n_chains; ++c)
      if (group[c] < -1 || group[c] >= n_groups)
        return fail(ctx, TCI_ERANGE, std::string(who) + ": group[" + std::to_string(c) + "] = " +
                                         std::to_string(group[c]) + " outside [-1, n_groups)");
  try {
    G->group.assign((size_t)n_chains, 0);
    if (group) std::copy(group, group + n_chains, G->group.begin());
    G->off.assign((size_t)n_groups + 1, 0);
    for (int64_t c = 0; c < n_chains; ++c)
      if (G->group[(size_t)c] >= 0) ++G->off[(size_t)G->group[(size_t)c] + 1];
    for (int64_t g = 0; g < n_groups; ++g) G->off[(size_t)g + 1] += G->off[(size_t)g];
    G->list.assign((size_t)std::max<int32_t>(G->off[(size_t)n_groups], 1), 0);
    std::vector<int32_t> fill(G->off.begin(), G->off.end() - 1);
    for (int64_t c = 0; c < n_chains; ++c)
      if (G->group[(size_t)c] >= 0) G->list[(size_t)fill[(size_t)G->group[(size_t)c]]++] = (int32_t)c;
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  if (npar)
    for (int64_t g = 0; g < n_groups; ++g)
      for (int32_t k = G->off[(size_t)g] + 1; k < G->off[(size_t)g + 1]; ++k)
        if (npar[G->list[(size_t)k]] != npar[G->list[(size_t)G->off[(size_t)g]]])
          return fail(ctx, TCI_EINVAL, std::string(who) + ": group " + std::to_string(g) + " has chains of different npar (" +
                                           std::to_string(npar[G->list[(size_t)G->off[(size_t)g]]]) + " and " +
                                           std::to_string(npar[G->list[(size_t)k]]) + ")");
  const int rc = tci::chainrhat_scratch_bytes(n_rows, n_chains, ld, n_groups, &G->scratch);
  if (rc == TCI_ENOMEM)
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": the per-segment partial sums are larger than any device memory");
  if (rc != TCI_OK)
    return fail(ctx, TCI_ERANGE, std::string(who) + ": rows x chains x ld too large for one launch (2^31 workgroups)");
  return TCI_OK;
}

namespace {

// tci_chainess's cap = (m L) log10(m L) of every group: cap[g] classic (m = M, L = n), cap[n_groups + g] split
// (m = 2 M, L = h).
void ess_caps(const RhatGroups& G, int64_t n_rows, double* cap) {
  const size_t ng = G.off.size() - 1;
  const int64_t h = n_rows / 2;
  for (size_t g = 0; g < ng; ++g) {
    const int64_t M = G.off[g + 1] - G.off[g];
    const double tc = (double)(M * n_rows), ts = (double)(2 * M * h);
    cap[g] = tc > 0 ? tc * std::log10(tc) : 0.0;
    cap[ng + g] = ts > 0 ? ts * std::log10(ts) : 0.0;
  }
}

// The three vectors of G onto the device, asynchronously: G outlives the stream's next synchronisation.
hipError_t upload_groups(const RhatGroups& G, int32_t* d_group, int32_t* d_off, int32_t* d_list, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(d_group, G.group.data(), G.group.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, G.off.data(), G.off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_list, G.list.data(), G.list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  return e;
}

}  // namespace

// The group kernels on a device chain (launch_chainrhat), timed with HIP events, and their results scattered into
// the caller's host buffers (d_npar null: ld columns for every chain; d_s2 null: the s2 twins are NaN).
int chainrhat_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, const RhatGroups& G, int64_t n_groups,
                     tci_chainrhat_outputs* out, int64_t max_lag, tci_chainess_outputs* eout) {
  const size_t ldc = (size_t)ld + 1, L = (size_t)ld, ng = (size_t)n_groups, plane = ng * ldc;
  DevAllocs A;
  hipError_t e = hipSuccess;
  void* d_scratch = A.alloc<uint8_t>(G.scratch, &e);
  // the effective sample size (eout): five more planes of doubles, two of windows and the groups' caps
  double* d_ed = e == hipSuccess && eout ? A.alloc<double>(5 * plane, &e) : nullptr;
  int32_t* d_ew = e == hipSuccess && eout ? A.alloc<int32_t>(2 * plane, &e) : nullptr;
  double* d_cap = e == hipSuccess && eout ? A.alloc<double>(2 * ng, &e) : nullptr;
  double* d_o = e == hipSuccess ? A.alloc<double>(4 * plane, &e) : nullptr;
  int32_t* d_group = e == hipSuccess ? A.alloc<int32_t>(G.group.size(), &e) : nullptr;
  int32_t* d_off = e == hipSuccess ? A.alloc<int32_t>(G.off.size(), &e) : nullptr;
  int32_t* d_list = e == hipSuccess ? A.alloc<int32_t>(G.list.size(), &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the group reduction (" +
                                     std::to_string(G.scratch + 4 * plane * sizeof(double)) + " bytes) failed");
  }
  std::vector<double> ho, he, hcap;
  std::vector<int32_t> hw;
  try {
    ho.resize(4 * plane);
    if (eout) {
      he.resize(5 * plane);
      hw.resize(2 * plane);
      hcap.assign(2 * ng, 0.0);
      ess_caps(G, n_rows, hcap.data());
    }
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  hipStream_t s = ctx->stream;
  EventTimer timer;
  const char* what_create = nullptr;
  if ((e = timer.create(&what_create)) != hipSuccess) return hip_fail(ctx, e, what_create);
  // from here every path reaches the hipStreamSynchronize below: G's vectors outlive their uploads
  e = upload_groups(G, d_group, d_off, d_list, s);
  if (e == hipSuccess && eout) e = hipMemcpyAsync(d_cap, hcap.data(), hcap.size() * sizeof(double), hipMemcpyHostToDevice, s);
  hipError_t e1 = e == hipSuccess ? timer.start(s) : e;
  const int rc = e != hipSuccess ? TCI_OK
                 : eout ? tci::launch_chainess(d_chain, d_s2, n_rows, n_chains, ld, d_npar, d_group, n_groups, d_off,
                                               d_list, max_lag, d_cap, d_scratch, d_o, d_ed, d_ew, (void*)s)
                        : tci::launch_chainrhat(d_chain, d_s2, n_rows, n_chains, ld, d_npar, d_group, n_groups,
                                                d_off, d_list, d_scratch, d_o, (void*)s);
  if (e1 == hipSuccess) e1 = timer.stop(s);
  if (rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(ho.data(), d_o, 4 * plane * sizeof(double), hipMemcpyDeviceToHost, s);
  if (rc == TCI_OK && e1 == hipSuccess && eout) e1 = hipMemcpyAsync(he.data(), d_ed, 5 * plane * sizeof(double), hipMemcpyDeviceToHost, s);
  if (rc == TCI_OK && e1 == hipSuccess && eout) e1 = hipMemcpyAsync(hw.data(), d_ew, 2 * plane * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = timer.elapsed_ms(&ms);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain R-hat kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "chain R-hat kernels");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain R-hat copy");
  if (out) {
    double* const dst[4] = {out->rhat, out->rhat_split, out->pooled_mean, out->pooled_std};
    double* const dst2[4] = {out->s2_rhat, out->s2_rhat_split, out->s2_pooled_mean, out->s2_pooled_std};
    for (size_t t = 0; t < 4; ++t)
      for (size_t g = 0; g < ng; ++g) {
        const double* src = ho.data() + (t * ng + g) * ldc;
        if (dst[t]) std::memcpy(dst[t] + g * L, src, L * sizeof(double));
        if (dst2[t]) dst2[t][g] = src[L];
      }
    out->n_rows = n_rows;
    out->kernel_ms = ms;
  }
  if (eout) {
    double* const dst[5] = {eout->ess, eout->ess_split, eout->tau, eout->tau_split, eout->mcse};
    double* const dst2[5] = {eout->s2_ess, eout->s2_ess_split, eout->s2_tau, eout->s2_tau_split, eout->s2_mcse};
    int32_t* const wdst[2] = {eout->window, eout->window_split};
    int32_t* const wdst2[2] = {eout->s2_window, eout->s2_window_split};
    for (size_t g = 0; g < ng; ++g) {
      for (size_t t = 0; t < 5; ++t) {
        const double* src = he.data() + (t * ng + g) * ldc;
        if (dst[t]) std::memcpy(dst[t] + g * L, src, L * sizeof(double));
        if (dst2[t]) dst2[t][g] = src[L];
      }
      for (size_t t = 0; t < 2; ++t) {
        const int32_t* src = hw.data() + (t * ng + g) * ldc;
        if (wdst[t]) std::memcpy(wdst[t] + g * L, src, L * sizeof(int32_t));
        if (wdst2[t]) wdst2[t][g] = src[L];
      }
    }
    eout->n_rows = n_rows;
    eout->kernel_ms = ms;
  }
  return TCI_OK;
}

// Checks of tci_chainrank_options before any device work; *o: the options to use (the defaults for null).
int chainrank_opts(tci_ctx* ctx, const char* who, const tci_chainrank_options* kopt, tci_chainrank_options* o) {
  tci_chainrank_defaults(o);
  if (kopt) *o = *kopt;
  if (o->nq < 1 || o->nq > 16) return fail(ctx, TCI_EINVAL, std::string(who) + ": nq must be in [1, 16]");
  for (int32_t q = 0; q < o->nq; ++q)
    if (!(o->probs[q] >= 0.0 && o->probs[q] <= 1.0))
      return fail(ctx, TCI_EINVAL, std::string(who) + ": probs[" + std::to_string(q) + "] is not in [0, 1]");
  if (!(o->tail_lo > 0.0 && o->tail_lo < o->tail_hi && o->tail_hi < 1.0))
    return fail(ctx, TCI_EINVAL, std::string(who) + ": the tails must satisfy 0 < tail_lo < tail_hi < 1");
  if (o->max_lag < 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": max_lag must be >= 0");
  if (o->flags != 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": flags is reserved and must be 0");
  return TCI_OK;
}

// The rank diagnostics on a device chain: four passes through one transformed chain (z, z_folded, I_lo, I_hi), each
// launch_chainrank followed by launch_chainess (launch_chainrhat for the folded scores), timed with HIP events, and
// their results scattered into the caller's host buffers.
int chainrank_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, const RhatGroups& G, int64_t n_groups,
                     const tci_chainrank_options& o, tci_chainrank_outputs* out) {
  const size_t ldc = (size_t)ld + 1, L = (size_t)ld, ng = (size_t)n_groups, plane = ng * ldc;
  const size_t nqq = (size_t)o.nq + 3, nch = (size_t)n_rows * (size_t)n_chains * L, ns2 = (size_t)n_rows * (size_t)n_chains;
  int64_t stride = 0;
  size_t keys = 0;
  int rc = tci::chainrank_scratch_keys(n_rows, ld, n_groups, G.off.data(), &stride, &keys);
  if (rc == TCI_ENOMEM) return fail(ctx, TCI_ENOMEM, std::string(who) + ": the sort's keys are larger than any device memory");
  if (rc != TCI_OK)
    return fail(ctx, TCI_ERANGE, std::string(who) + ": a group of 2^31 values or more, or a launch of 2^31 workgroups");
  DevAllocs A;
  hipError_t e = hipSuccess;
  void* d_scratch = A.alloc<uint8_t>(G.scratch, &e);
  double* d_z = e == hipSuccess ? A.alloc<double>(nch, &e) : nullptr;
  double* d_zs2 = e == hipSuccess && d_s2 ? A.alloc<double>(ns2, &e) : nullptr;
  uint64_t* d_gk = e == hipSuccess && keys ? A.alloc<uint64_t>(keys, &e) : nullptr;
  double* d_q = e == hipSuccess ? A.alloc<double>(nqq * plane, &e) : nullptr;
  double* d_o = e == hipSuccess ? A.alloc<double>(16 * plane, &e) : nullptr;   // launch_chainrhat's out of every pass
  double* d_ed = e == hipSuccess ? A.alloc<double>(15 * plane, &e) : nullptr;  // launch_chainess's: z, I_lo, I_hi
  int32_t* d_ew = e == hipSuccess ? A.alloc<int32_t>(6 * plane, &e) : nullptr;
  double* d_cap = e == hipSuccess ? A.alloc<double>(2 * ng, &e) : nullptr;
  int32_t* d_group = e == hipSuccess ? A.alloc<int32_t>(G.group.size(), &e) : nullptr;
  int32_t* d_off = e == hipSuccess ? A.alloc<int32_t>(G.off.size(), &e) : nullptr;
  int32_t* d_list = e == hipSuccess ? A.alloc<int32_t>(G.list.size(), &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": device allocation of the transformed chain and the sort's keys (" +
                                     std::to_string(G.scratch + (nch + (d_s2 ? ns2 : 0) + keys + (nqq + 31) * plane + 2 * ng) *
                                                                    sizeof(double) +
                                                    (6 * plane + G.group.size() + G.off.size() + G.list.size()) *
                                                        sizeof(int32_t)) +
                                     " bytes) failed");
  }
  std::vector<double> ho, he, hq, hcap;
  std::vector<int32_t> hw;
  try {
    ho.resize(16 * plane);
    he.resize(15 * plane);
    hw.resize(6 * plane);
    hq.resize(nqq * plane);
    hcap.assign(2 * ng, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  ess_caps(G, n_rows, hcap.data());
  hipStream_t s = ctx->stream;
  EventTimer whole, pass[4];
  const char* what_create = nullptr;
  if ((e = whole.create(&what_create)) != hipSuccess) return hip_fail(ctx, e, what_create);
  for (EventTimer& t : pass)
    if ((e = t.create(&what_create)) != hipSuccess) return hip_fail(ctx, e, what_create);
  // from here every path reaches the hipStreamSynchronize below: G's vectors outlive their uploads
  e = upload_groups(G, d_group, d_off, d_list, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cap, hcap.data(), hcap.size() * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = whole.start(s);
  // NaN: what padding, the chains of no group and the quantiles of unused columns keep
  rc = e != hipSuccess ? TCI_OK : tci::launch_chainrank_fill(d_z, nch, (void*)s);
  if (rc == TCI_OK && e == hipSuccess && d_zs2) rc = tci::launch_chainrank_fill(d_zs2, ns2, (void*)s);
  if (rc == TCI_OK && e == hipSuccess) rc = tci::launch_chainrank_fill(d_q, nqq * plane, (void*)s);
  double* const zdst[2] = {out->z, out->z_folded};
  double* const zdst2[2] = {out->s2_z, out->s2_z_folded};
  for (int m = 0; m < 4 && rc == TCI_OK && e == hipSuccess; ++m) {
    e = pass[m].start(s);
    rc = tci::launch_chainrank(d_chain, d_s2, n_rows, n_chains, ld, d_npar, n_groups, G.off.data(), d_off, d_list, m,
                               o.probs, o.nq, o.tail_lo, o.tail_hi, d_q, d_gk, d_z, d_zs2, (void*)s);
    if (e == hipSuccess) e = pass[m].stop(s);
    if (rc != TCI_OK || e != hipSuccess) break;
    const int k = m == 0 ? 0 : m - 1;  // the pass's slot of d_ed / d_ew
    rc = m == 1 ? tci::launch_chainrhat(d_z, d_zs2, n_rows, n_chains, ld, d_npar, d_group, n_groups, d_off, d_list,
                                        d_scratch, d_o + (size_t)m * 4 * plane, (void*)s)
                : tci::launch_chainess(d_z, d_zs2, n_rows, n_chains, ld, d_npar, d_group, n_groups, d_off, d_list,
                                       o.max_lag, d_cap, d_scratch, d_o + (size_t)m * 4 * plane,
                                       d_ed + (size_t)k * 5 * plane, d_ew + (size_t)k * 2 * plane, (void*)s);
    if (rc == TCI_OK && m < 2 && zdst[m]) e = hipMemcpyAsync(zdst[m], d_z, nch * sizeof(double), hipMemcpyDeviceToHost, s);
    if (rc == TCI_OK && e == hipSuccess && m < 2 && zdst2[m] && d_zs2)
      e = hipMemcpyAsync(zdst2[m], d_zs2, ns2 * sizeof(double), hipMemcpyDeviceToHost, s);
  }
  hipError_t e1 = e;
  if (e1 == hipSuccess) e1 = whole.stop(s);
  const bool ok = rc == TCI_OK && e1 == hipSuccess;
  if (ok) e1 = hipMemcpyAsync(ho.data(), d_o, ho.size() * sizeof(double), hipMemcpyDeviceToHost, s);
  if (ok && e1 == hipSuccess) e1 = hipMemcpyAsync(he.data(), d_ed, he.size() * sizeof(double), hipMemcpyDeviceToHost, s);
  if (ok && e1 == hipSuccess) e1 = hipMemcpyAsync(hw.data(), d_ew, hw.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (ok && e1 == hipSuccess) e1 = hipMemcpyAsync(hq.data(), d_q, hq.size() * sizeof(double), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f, rank_ms = 0.f;
  if (ok && e1 == hipSuccess && e2 == hipSuccess) e1 = whole.elapsed_ms(&ms);
  for (EventTimer& t : pass) {
    float pm = 0.f;
    if (ok && e1 == hipSuccess && e2 == hipSuccess) e1 = t.elapsed_ms(&pm);
    rank_ms += pm;
  }
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain rank kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "chain rank kernels");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain rank copy");
  if (!d_s2) {  // no s2 chain: its z twins are NaN
    for (int m = 0; m < 2; ++m)
      if (zdst2[m]) std::fill(zdst2[m], zdst2[m] + ns2, std::nan(""));
  }
  // rhat_split is plane 1 of a pass's launch_chainrhat out; ess_split, tau_split planes 1 and 3 of launch_chainess's
  // doubles and window_split plane 1 of its windows
  const auto rh = [&](int m, size_t g) { return ho.data() + (((size_t)m * 4 + 1) * ng + g) * ldc; };
  const auto ed = [&](int k, int t, size_t g) { return he.data() + (((size_t)k * 5 + (size_t)t) * ng + g) * ldc; };
  const auto ew = [&](int k, size_t g) { return hw.data() + (((size_t)k * 2 + 1) * ng + g) * ldc; };
  const auto put = [&](double* dst, double* dst2, size_t g, const double* src) {
    if (dst) std::memcpy(dst + g * L, src, L * sizeof(double));
    if (dst2) dst2[g] = src[L];
  };
  const auto putw = [&](int32_t* dst, int32_t* dst2, size_t g, const int32_t* src) {
    if (dst) std::memcpy(dst + g * L, src, L * sizeof(int32_t));
    if (dst2) dst2[g] = src[L];
  };
  std::vector<double> both(ldc);
  for (size_t g = 0; g < ng; ++g) {
    for (size_t q = 0; q < nqq; ++q) {
      const double* src = hq.data() + (g * nqq + q) * ldc;
      if (q < (size_t)o.nq) {
        if (out->q) std::memcpy(out->q + (g * (size_t)o.nq + q) * L, src, L * sizeof(double));
        if (out->s2_q) out->s2_q[g * (size_t)o.nq + q] = src[L];
      } else if (q > (size_t)o.nq) {
        const size_t t = q - (size_t)o.nq - 1;
        if (out->q_tail) std::memcpy(out->q_tail + (g * 2 + t) * L, src, L * sizeof(double));
        if (out->s2_q_tail) out->s2_q_tail[g * 2 + t] = src[L];
      }
    }
    put(out->rhat_bulk, out->s2_rhat_bulk, g, rh(0, g));
    put(out->rhat_folded, out->s2_rhat_folded, g, rh(1, g));
    for (size_t j = 0; j < ldc; ++j) {  // the larger, NaN if either is NaN
      const double a = rh(0, g)[j], b = rh(1, g)[j];
      both[j] = a != a || b != b ? std::nan("") : (a > b ? a : b);
    }
    put(out->rhat_rank, out->s2_rhat_rank, g, both.data());
    put(out->ess_bulk, out->s2_ess_bulk, g, ed(0, 1, g));
    put(out->tau_bulk, out->s2_tau_bulk, g, ed(0, 3, g));
    put(out->ess_tail_lo, out->s2_ess_tail_lo, g, ed(1, 1, g));
    put(out->ess_tail_hi, out->s2_ess_tail_hi, g, ed(2, 1, g));
    for (size_t j = 0; j < ldc; ++j) {  // the smaller, NaN if either is NaN
      const double a = ed(1, 1, g)[j], b = ed(2, 1, g)[j];
      both[j] = a != a || b != b ? std::nan("") : (a < b ? a : b);
    }
    put(out->ess_tail, out->s2_ess_tail, g, both.data());
    putw(out->window_bulk, out->s2_window_bulk, g, ew(0, g));
    putw(out->window_tail_lo, out->s2_window_tail_lo, g, ew(1, g));
    putw(out->window_tail_hi, out->s2_window_tail_hi, g, ew(2, g));
  }
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  out->rank_ms = rank_ms;
  return TCI_OK;
}

}  // namespace tci_api

using namespace tci_api;

namespace {

// A host chain's npar (null: ld for every chain): every entry in [0, ld].
int check_npar(tci_ctx* ctx, const char* who, const int32_t* npar, int64_t n_chains, int64_t ld) {
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, std::string(who) + ": npar[" + std::to_string(c) + "] outside [0, ld]");
  return TCI_OK;
}

// A host chain [n_rows][n_chains][ld] on the device, with its s2 chain and npar where the caller has them (null
// stays null), freed with this object. upload: the size check, the allocations and the copies on the context's stream.
struct DeviceChain {
  DevAllocs A;
  double *d_chain = nullptr, *d_s2 = nullptr;
  int32_t* d_npar = nullptr;
  int upload(tci_ctx* ctx, const char* who, const double* chain, const double* s2chain, int64_t n_rows,
             int64_t n_chains, int64_t ld, const int32_t* npar) {
    const size_t per_row = (size_t)n_chains * (size_t)ld;
    if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
      return fail(ctx, TCI_ENOMEM, std::string(who) + ": the chain is larger than any device memory");
    TCI_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
    d_chain = A.alloc<double>(nch, &e);
    d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
    d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, TCI_ENOMEM, std::string(who) + ": the chain (" + std::to_string(nch * sizeof(double)) +
                                       " bytes) does not fit the device");
    }
    hipStream_t s = ctx->stream;
    TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
    if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
    if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return TCI_OK;
  }
};

}  // namespace

extern "C" {

int tci_chainquant_defaults(tci_chainquant_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->nq = 3;
  o->probs[0] = 0.025;
  o->probs[1] = 0.5;
  o->probs[2] = 0.975;
  return TCI_OK;
}

int tci_chainquant(tci_ctx* ctx, const tci_chainquant_options* opt, const double* chain, const double* s2chain,
                   int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chainquant_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chainquant: null argument");
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, "tci_chainquant: n_rows must be >= 1");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainquant: n_chains and ld must be >= 1");
  if (n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30))
    return fail(ctx, TCI_ERANGE, "tci_chainquant: n_rows or n_chains above 2^30");
  const double* probs = nullptr;
  int32_t nq = 0;
  int rc = chainquant_probs(ctx, "tci_chainquant", opt, n_chains, ld, &probs, &nq);
  if (rc != TCI_OK) return rc;
  if ((rc = check_npar(ctx, "tci_chainquant", npar, n_chains, ld)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chainquant", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chainquant_device(ctx, "tci_chainquant", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, probs, nq, out);
}

int tci_chaindens_defaults(tci_chaindens_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->n_grid = 100;  // linspace's default in density.m
  o->n_bins = 20;
  o->bw_scale = 1.0;
  return TCI_OK;
}

int tci_chaindens(tci_ctx* ctx, const tci_chaindens_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chaindens_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chaindens: null argument");
  if (n_rows < 2) return fail(ctx, TCI_EINVAL, "tci_chaindens: n_rows must be >= 2");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chaindens: n_chains and ld must be >= 1");
  int32_t G = 0, B = 0;
  double bws = 0.0;
  size_t scratch = 0;
  int rc = chaindens_opts(ctx, "tci_chaindens", opt, n_rows, n_chains, ld, &G, &B, &bws, &scratch);
  if (rc != TCI_OK) return rc;
  if ((rc = check_npar(ctx, "tci_chaindens", npar, n_chains, ld)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chaindens", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chaindens_device(ctx, "tci_chaindens", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, G, B, bws, scratch, out);
}

int tci_chainess_defaults(tci_chainess_options* o) {
  if (!o) return TCI_EINVAL;
  o->max_lag = 0;  // L - 1: the pairs are summed until Geyer's sequence stops
  o->flags = 0;
  return TCI_OK;
}

int tci_chainess(tci_ctx* ctx, const tci_chainess_options* opt, const double* chain, const double* s2chain,
                 int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                 int64_t n_groups, tci_chainess_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chainess: null argument");
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, "tci_chainess: n_rows must be >= 1");
  if (opt && opt->max_lag < 0) return fail(ctx, TCI_EINVAL, "tci_chainess: max_lag must be >= 0");
  if (opt && opt->flags != 0) return fail(ctx, TCI_EINVAL, "tci_chainess: flags is reserved and must be 0");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainess: n_chains and ld must be >= 1");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_chainess: n_groups must be in [1, n_chains]");
  int rc = check_npar(ctx, "tci_chainess", npar, n_chains, ld);
  if (rc != TCI_OK) return rc;
  RhatGroups G;
  if ((rc = chainrhat_groups(ctx, "tci_chainess", nullptr, n_rows, n_chains, ld, npar, group, n_groups, &G)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chainess", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chainrhat_device(ctx, "tci_chainess", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, G, n_groups, nullptr,
                          opt ? opt->max_lag : 0, out);
}

int tci_chainrank_defaults(tci_chainrank_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->nq = 3;
  o->probs[0] = 0.025;
  o->probs[1] = 0.5;
  o->probs[2] = 0.975;
  o->tail_lo = 0.05;
  o->tail_hi = 0.95;
  return TCI_OK;
}

int64_t tci_chainrank_lds_cap(void) { return tci::kRankLdsCap; }

int tci_chainrank(tci_ctx* ctx, const tci_chainrank_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                  int64_t n_groups, tci_chainrank_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chainrank: null argument");
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, "tci_chainrank: n_rows must be >= 1");
  tci_chainrank_options o;
  int rc = chainrank_opts(ctx, "tci_chainrank", opt, &o);
  if (rc != TCI_OK) return rc;
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainrank: n_chains and ld must be >= 1");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_chainrank: n_groups must be in [1, n_chains]");
  if ((rc = check_npar(ctx, "tci_chainrank", npar, n_chains, ld)) != TCI_OK) return rc;
  RhatGroups G;
  if ((rc = chainrhat_groups(ctx, "tci_chainrank", nullptr, n_rows, n_chains, ld, npar, group, n_groups, &G)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chainrank", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chainrank_device(ctx, "tci_chainrank", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, G, n_groups, o, out);
}

int tci_chainlp_defaults(tci_chainlp_options* o) {
  if (!o) return TCI_EINVAL;
  o->flags = 0;
  return TCI_OK;
}

int tci_chainlp(tci_ctx* ctx, const tci_chainlp_options* opt, const double* chain, const double* s2chain,
                int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* cell_id, const double* prior_mu,
                const double* prior_sig, tci_chainlp_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !s2chain || !cell_id || !prior_mu || !prior_sig || !out)
    return fail(ctx, TCI_EINVAL, "tci_chainlp: null argument");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainlp: n_chains and ld must be >= 1");
  size_t scratch = 0;
  const int rc = chainlp_check(ctx, "tci_chainlp", opt, n_rows, n_chains, ld, cell_id, prior_mu, prior_sig, &scratch);
  if (rc != TCI_OK) return rc;
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t n = (size_t)n_chains, L = (size_t)ld;
  const size_t nch = (size_t)n_rows * n * L, ns2 = (size_t)n_rows * n;  // n_rows * n_chains < 2^31, ld <= 2^24
  std::vector<int32_t> npar(n);
  for (size_t c = 0; c < n; ++c) npar[c] = 7 + ctx->meta[(size_t)cell_id[c]].n;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_cell = e == hipSuccess ? A.alloc<int32_t>(n, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess ? A.alloc<int32_t>(n, &e) : nullptr;
  double* d_mu = e == hipSuccess ? A.alloc<double>(n * L, &e) : nullptr;
  double* d_sig = e == hipSuccess ? A.alloc<double>(n * L, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chainlp: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  TCI_HIP(ctx, hipMemcpyAsync(d_cell, cell_id, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  TCI_HIP(ctx, hipMemcpyAsync(d_mu, prior_mu, n * L * sizeof(double), hipMemcpyHostToDevice, s));
  TCI_HIP(ctx, hipMemcpyAsync(d_sig, prior_sig, n * L * sizeof(double), hipMemcpyHostToDevice, s));
  return chainlp_device(ctx, "tci_chainlp", d_chain, d_s2, n_rows, n_chains, ld, d_cell, d_npar, d_mu, d_sig, scratch, out);
}

int tci_chainrhat_defaults(tci_chainrhat_options* o) {
  if (!o) return TCI_EINVAL;
  o->flags = 0;
  return TCI_OK;
}

int tci_chainrhat(tci_ctx* ctx, const tci_chainrhat_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                  int64_t n_groups, tci_chainrhat_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chainrhat: null argument");
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, "tci_chainrhat: n_rows must be >= 1");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainrhat: n_chains and ld must be >= 1");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_chainrhat: n_groups must be in [1, n_chains]");
  int rc = check_npar(ctx, "tci_chainrhat", npar, n_chains, ld);
  if (rc != TCI_OK) return rc;
  RhatGroups G;
  if ((rc = chainrhat_groups(ctx, "tci_chainrhat", opt, n_rows, n_chains, ld, npar, group, n_groups, &G)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chainrhat", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chainrhat_device(ctx, "tci_chainrhat", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, G, n_groups, out);
}

int tci_chaincov_defaults(tci_chaincov_options* o) {
  if (!o) return TCI_EINVAL;
  o->scratch_bytes = 0;  // 1 GiB
  return TCI_OK;
}

int tci_chaincov(tci_ctx* ctx, const tci_chaincov_options* opt, const double* chain, int64_t n_rows, int64_t n_chains,
                 int64_t ld, const int32_t* npar, tci_chaincov_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chaincov: null argument");
  if (n_rows < 2) return fail(ctx, TCI_EINVAL, "tci_chaincov: n_rows must be >= 2");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chaincov: n_chains and ld must be >= 1");
  if (n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30))
    return fail(ctx, TCI_ERANGE, "tci_chaincov: n_rows or n_chains above 2^30");
  int rc = check_npar(ctx, "tci_chaincov", npar, n_chains, ld);
  if (rc != TCI_OK) return rc;
  int64_t group = 0;
  if ((rc = chaincov_group(ctx, "tci_chaincov", opt, n_chains, ld, &group)) != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chaincov", chain, nullptr, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chaincov_device(ctx, "tci_chaincov", d.d_chain, n_rows, n_chains, ld, d.d_npar, group, out);
}

int tci_chainstats_defaults(tci_chainstats_options* o) {
  if (!o) return TCI_EINVAL;
  o->max_lag = 0;  // n: mcmcstat's iact sums until Sokal's window closes
  return TCI_OK;
}

int tci_chainstats(tci_ctx* ctx, const tci_chainstats_options* opt, const double* chain, const double* s2chain,
                   int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chainstats_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  const int64_t max_lag = opt ? opt->max_lag : 0;
  if (!chain || !out) return fail(ctx, TCI_EINVAL, "tci_chainstats: null argument");
  if (n_rows < 1) return fail(ctx, TCI_EINVAL, "tci_chainstats: n_rows must be >= 1");
  if (max_lag < 0) return fail(ctx, TCI_EINVAL, "tci_chainstats: max_lag must be >= 0");
  if (n_chains < 1 || ld < 1) return fail(ctx, TCI_EINVAL, "tci_chainstats: n_chains and ld must be >= 1");
  if (ld > ((int64_t)1 << 24) || n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30))
    return fail(ctx, TCI_ERANGE, "tci_chainstats: ld above 2^24, or n_rows or n_chains above 2^30");
  int rc = check_npar(ctx, "tci_chainstats", npar, n_chains, ld);
  if (rc != TCI_OK) return rc;
  DeviceChain d;
  if ((rc = d.upload(ctx, "tci_chainstats", chain, s2chain, n_rows, n_chains, ld, npar)) != TCI_OK) return rc;
  return chainstats_device(ctx, "tci_chainstats", d.d_chain, d.d_s2, n_rows, n_chains, ld, d.d_npar, max_lag, out);
}

}  // extern "C"
