// tci_api_dram.cpp -- C ABI (include/tci.h): the GPU-resident DRAM sampler, tci_dram_run and the entry points that add
// reductions of the kept rows, a group reduction, the log-posterior trace or tempering to it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "tci_api_internal.h"

using namespace tci_api;

namespace {

// What tci_dram_run_rhat adds to a run: the groups of its chains and where the group reduction goes.
struct RhatAsk {
  const tci_chainrhat_options* ropt;
  const int32_t* group;
  int64_t n_groups;
  tci_chainrhat_outputs* rout;
  const char* who = "tci_dram_run_rhat";
  const tci_chainess_options* eopt = nullptr;  // tci_dram_run_ess: the effective sample size too (rout may be null)
  tci_chainess_outputs* eout = nullptr;
  const tci_chainrank_options* kopt = nullptr;  // tci_dram_run_rank: the rank diagnostics too (rout, eout may be null)
  tci_chainrank_outputs* kout = nullptr;
};

// One DRAM step: propose -> ssfun -> accept/propose stage 2 -> ssfun -> accept, sigma2, log the row
// -> [window records] -> [adapt] -> step + 1.
int enqueue_step(tci_ctx* ctx, const tci::DramState& st, const tci::DramParams& p, hipStream_t s, bool with_stats,
                 bool with_adapt, const tci::SwapArgs* swap = nullptr) {
  int rc;
  if ((rc = tci::dram_launch_propose1(st, p, s)) != TCI_OK) return rc;
  if ((rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, st.prop1, st.ld, st.cell, st.act1, st.n_chains, st.ss1,
                        nullptr, 0, s)) != TCI_OK)
    return rc;
  if ((rc = tci::dram_launch_accept1(st, p, s)) != TCI_OK) return rc;
  if (p.ntry >= 2 && (rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, st.prop2, st.ld, st.cell, st.act2,
                                       st.n_chains, st.ss2, nullptr, 0, s)) != TCI_OK)
    return rc;
  if ((rc = tci::dram_launch_accept2(st, p, s)) != TCI_OK) return rc;
  if (with_stats && (rc = tci::dram_launch_stats(st, p, s)) != TCI_OK) return rc;
  if (with_adapt && (rc = tci::dram_launch_adapt(st, p, s)) != TCI_OK) return rc;  // no-op unless step % adaptint == 0
  // a window's end (with_stats): the ladders' swap, which reads the row from *st.step as the adaptation does
  if (swap && with_stats && (rc = tci::dram_launch_swap(st, p, *swap, s)) != TCI_OK) return rc;
  return tci::dram_launch_step_incr(st, s);
}

// The batched engine's captured window of steps and its executable, destroyed with their owner.
struct StepGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  StepGraph() = default;
  StepGraph(const StepGraph&) = delete;
  StepGraph& operator=(const StepGraph&) = delete;
  ~StepGraph() { reset(); }
  void reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
  }
};

// One run. The entry points fill the arguments and the request; go() runs the phases in order, each a method that
// reads what the earlier ones left in the members below: check and plan (no device work), alloc, upload, run_steps
// (fused_steps or batched_steps), read_outputs, reduce. It owns a self-referring state (swp = &sw): not copyable.
struct DramRun {
  // ---- tci_dram_run's arguments
  tci_ctx* ctx;
  const tci_dram_options* opt;
  int64_t n_chains;
  const int32_t* cell_id;
  const double *theta0, *lower, *upper, *prior_mu, *prior_sig, *qcov_diag, *sigma2_0;
  int64_t ld;
  tci_dram_outputs* out;
  // ---- the request: what an entry point adds. All reductions read the same kept rows.
  tci_dram_reductions red{};                  // of every chain: statistics, matrices, quantiles, densities
  const RhatAsk* rhat = nullptr;              // across the chains of every group
  const tci_chainlp_options* lopt = nullptr;  // the log-posterior trace (lout: asked for)
  tci_chainlp_outputs* lout = nullptr;
  const tci_temper_options* topt = nullptr;  // tci_dram_run_tempered: the ladders and where the swap records go
  tci_temper_outputs* tout = nullptr;
  // ---- check: the kept rows k (chain row 1 + k * thin) from the first one at or past stats_from, every reduction's
  // checked options, each chain's P = 7 + N and observation count 2 N
  size_t n = 0, L = 0, d_scratch = 0, l_scratch = 0;  // n_chains, ld; the densities' and the trace's scratch bytes
  int64_t keep_k0 = 0, keep_rows = 0, max_lag = 0, cov_group = 0;
  const double* q_probs = nullptr;
  int32_t q_nq = 0, d_G = 0, d_B = 0;
  double d_bws = 0.0;
  std::vector<int32_t> npar, nobs;
  // ---- plan: the ladders (each chain's Gibbs shape and stored sigma2, the pairs of neighbouring rungs), the groups,
  // the P the adaptation kernel is picked for, and the run's windows
  std::vector<double> gshape, s20, beta;
  std::vector<int32_t> pair_a, pair_b, pair_r;
  int64_t swap_every = 0, p_max_all = 0;
  RhatGroups r_groups;
  tci_chainrank_options k_opt{};
  int64_t ai = 0, DW = 0, win = 0, chunk = 0, n_keep = 0;
  // ---- alloc, upload: the device side
  DevAllocs A;
  tci::DramState st{};
  tci::DramParams p{};
  int32_t *d_cell = nullptr, *d_npar = nullptr, *d_nobs = nullptr;
  int64_t* d_key = nullptr;
  double *d_gshape = nullptr, *d_lower = nullptr, *d_upper = nullptr, *d_pmu = nullptr, *d_psig = nullptr,
         *d_qdiag = nullptr, *d_s20 = nullptr;
  tci::SwapArgs sw{};
  const tci::SwapArgs* swp = nullptr;
  int64_t n_events = 0, log_rows = 0;
  // ---- run_steps
  hipStream_t s = nullptr;
  int n_cu = 0;
  bool fused = false;
  int rc = TCI_OK;           // the last TCI_* code; after the step loop, its first failed launch
  hipError_t e = hipSuccess;  // the last allocation's status; after the step loop, its first failed graph replay

  DramRun(const DramRun&) = delete;  // C++17: still an aggregate (TCI_RUN_ARGS); C++20 would need a constructor
  DramRun& operator=(const DramRun&) = delete;

  // ---- phase: the arguments and the options of the run and of every reduction asked for.
  int check() {
    if (!opt || !out || n_chains <= 0 || !cell_id || !theta0 || !lower || !upper || !prior_mu || !prior_sig ||
        !qcov_diag || !sigma2_0)
      return fail(ctx, TCI_EINVAL, "tci_dram_run: null argument or no chains");
    if (opt->n_steps < 1 || opt->ntry < 1 || opt->ntry > 2 || opt->adaptint < 0 || !(opt->drscale > 0) ||
        opt->engine < TCI_DRAM_AUTO || opt->engine > TCI_DRAM_WALK || opt->max_chunk < 0 || opt->adapt_pmax < 0 ||
        opt->adapt_pmax > TCI_MAX_POINTS + 7)
      return fail(ctx, TCI_EINVAL,
                  "tci_dram_run: bad options (n_steps >= 1, ntry in {1,2}, adaptint >= 0, engine in {0,1,2,3}, "
                  "max_chunk >= 0, 0 <= adapt_pmax <= 2055)");
    n = (size_t)n_chains;
    L = (size_t)ld;
    // the reductions, in this order: each needs the kept rows, enough of them in the window, then its own options
    const bool kept = opt->thin > 0;
    if (kept) {
      keep_k0 = (std::max<int64_t>(opt->stats_from, 1) - 1 + opt->thin - 1) / opt->thin;
      keep_rows = (opt->n_steps + opt->thin - 1) / opt->thin - keep_k0;
    }
    max_lag = red.sopt ? red.sopt->max_lag : 0;
    if (red.sout) {
      if (!kept) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: the statistics need the kept rows (thin >= 1)");
      if (max_lag < 0) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: max_lag must be >= 0");
      if (keep_rows < 1) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: no kept row at or past stats_from (n_rows < 1)");
    }
    if (red.cout) {
      if (!kept) return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: the matrices need the kept rows (thin >= 1)");
      if (keep_rows < 2)
        return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: fewer than 2 kept rows at or past stats_from (n_rows < 2)");
      if ((rc = chaincov_group(ctx, "tci_dram_run_cov", red.copt, n_chains, ld, &cov_group)) != TCI_OK) return rc;
    }
    if (red.qout) {
      if (!kept) return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: the quantiles need the kept rows (thin >= 1)");
      if (keep_rows < 1)
        return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: no kept row at or past stats_from (n_rows < 1)");
      if ((rc = chainquant_probs(ctx, "tci_dram_run_reduced", red.qopt, n_chains, ld, &q_probs, &q_nq)) != TCI_OK) return rc;
    }
    if (red.dout) {
      if (!kept) return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: the densities need the kept rows (thin >= 1)");
      if (keep_rows < 2)
        return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: fewer than 2 kept rows at or past stats_from (n_rows < 2)");
      rc = chaindens_opts(ctx, "tci_dram_run_reduced", red.dopt, keep_rows, n_chains, ld, &d_G, &d_B, &d_bws, &d_scratch);
      if (rc != TCI_OK) return rc;
    }
    if (lout) {
      if (!kept) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: the log-posterior trace needs the kept rows (thin >= 1)");
      if (keep_rows < 1) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: no kept row at or past stats_from (n_rows < 1)");
    }
    if (rhat) {
      if (!kept)
        return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": the group reduction needs the kept rows (thin >= 1)");
      if (keep_rows < 2)
        return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": fewer than 2 kept rows at or past stats_from (n_rows < 2)");
      if (rhat->eout && rhat->eopt && rhat->eopt->max_lag < 0)
        return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": max_lag must be >= 0");
      if (rhat->eout && rhat->eopt && rhat->eopt->flags != 0)
        return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": flags is reserved and must be 0");
      if (rhat->kout && (rc = chainrank_opts(ctx, rhat->who, rhat->kopt, &k_opt)) != TCI_OK) return rc;
    }
    if ((rc = check_rows(ctx, ld, cell_id, n_chains)) != TCI_OK) return rc;
    if (ld > TCI_MAX_POINTS + 7) return fail(ctx, TCI_ERANGE, "tci_dram_run: ld too large");
    if (lout) {
      rc = chainlp_check(ctx, "tci_dram_run_lp", lopt, keep_rows, n_chains, ld, cell_id, prior_mu, prior_sig, &l_scratch);
      if (rc != TCI_OK) return rc;
    }
    npar.resize(n);
    nobs.resize(n);
    for (size_t c = 0; c < n; ++c) {
      const int32_t N = ctx->meta[(size_t)cell_id[c]].n;
      npar[c] = 7 + N;
      nobs[c] = 2 * N;  // model.N = length(data.ydata) (:260), NaNs included
      for (int32_t j = 0; j < npar[c]; ++j) {
        const double x = theta0[c * L + j];
        if (!(x >= lower[c * L + j] && x <= upper[c * L + j]))
          return fail(ctx, TCI_EINVAL, "tci_dram_run: chain " + std::to_string(c) + " starts outside its bounds");
        if (!(qcov_diag[c * L + j] > 0)) return fail(ctx, TCI_EINVAL, "tci_dram_run: qcov_diag must be > 0");
      }
    }
    return TCI_OK;
  }

  // ---- phase: the ladder plan (from opt, the temper options and the chains' inputs), then the checks that need every
  // chain's P (the groups, the adaptation window's limits) and the run's windows. No device work.
  int plan() {
    gshape.resize(n);
    s20.assign(sigma2_0, sigma2_0 + n);
    beta.assign(n, 1.0);
    for (size_t c = 0; c < n; ++c) gshape[c] = 0.5 * (double)nobs[c];
    if (topt) {
      const tci_temper_options* t = topt;
      const char* who = "tci_dram_run_tempered";
      if (t->flags != 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": flags is reserved and must be 0");
      if (t->swap_every < 0) return fail(ctx, TCI_EINVAL, std::string(who) + ": swap_every must be >= 0");
      if (t->n_ladders < 0 || t->n_ladders > n_chains)
        return fail(ctx, TCI_EINVAL, std::string(who) + ": n_ladders must be in [0, n_chains]");
      swap_every = t->swap_every;
      for (size_t c = 0; c < n; ++c) {
        const double b = t->beta ? t->beta[c] : 1.0;
        const int32_t l = t->ladder ? t->ladder[c] : -1;
        const std::string where = " (chain " + std::to_string(c) + ", ladder " + std::to_string(l) + ")";
        if (l < -1 || l >= t->n_ladders)
          return fail(ctx, TCI_EINVAL, std::string(who) + ": ladder values must be in [-1, n_ladders)" + where);
        if (!std::isfinite(b) || !(b > 0.0) || !(b <= 1.0))
          return fail(ctx, TCI_EINVAL, std::string(who) + ": beta must be finite and in (0, 1]" + where);
        beta[c] = b;
        if (b != 1.0) {  // beta = 1 keeps the plain run's bits: no arithmetic on its values
          gshape[c] = b * (0.5 * (double)nobs[c]);
          s20[c] = sigma2_0[c] / b;
        }
        if (opt->updatesigma && !(gshape[c] >= 1.0))  // the Gibbs draw's shape; no draw, no limit
          return fail(ctx, TCI_EINVAL, std::string(who) + ": beta * N / 2 must be >= 1 for the sigma2 draw" + where);
      }
      std::vector<int64_t> last((size_t)t->n_ladders, -1);
      std::vector<int32_t> rung((size_t)t->n_ladders, 0);
      for (size_t c = 0; c < n && t->ladder; ++c) {
        const int32_t l = t->ladder[c];
        if (l < 0) continue;
        const int64_t a = last[(size_t)l];
        if (a >= 0) {
          const std::string where = " (ladder " + std::to_string(l) + ", chains " + std::to_string(a) + " and " +
                                    std::to_string(c) + ")";
          if (!(beta[c] < beta[(size_t)a]))
            return fail(ctx, TCI_EINVAL, std::string(who) + ": beta must be strictly decreasing along a ladder" + where);
          if (cell_id[c] != cell_id[a])
            return fail(ctx, TCI_EINVAL, std::string(who) + ": the rungs of a ladder must share the cell" + where);
          for (int32_t j = 0; j < npar[c]; ++j) {
            const size_t x = c * L + j, y = (size_t)a * L + j;
            const bool same_sig = prior_sig[x] == prior_sig[y] || (prior_sig[x] != prior_sig[x] && prior_sig[y] != prior_sig[y]);
            if (lower[x] != lower[y] || upper[x] != upper[y] || prior_mu[x] != prior_mu[y] || !same_sig)
              return fail(ctx, TCI_EINVAL, std::string(who) + ": the rungs of a ladder must share lower, upper, prior_mu "
                                                             "and prior_sig" + where);
          }
          if (!opt->updatesigma && sigma2_0[c] != sigma2_0[a])
            return fail(ctx, TCI_EINVAL, std::string(who) + ": with updatesigma = 0 the rungs of a ladder must share "
                                                           "sigma2_0" + where);
          pair_a.push_back((int32_t)a);
          pair_b.push_back((int32_t)c);
          pair_r.push_back(rung[(size_t)l] - 1);
        }
        last[(size_t)l] = (int64_t)c;
        ++rung[(size_t)l];
      }
    }
    if (rhat) {
      rc = chainrhat_groups(ctx, rhat->who, rhat->ropt, keep_rows, n_chains, ld, npar.data(), rhat->group, rhat->n_groups,
                            &r_groups);
      if (rc != TCI_OK) return rc;
    }
    // the P the adaptation kernel is picked for (> 208: k_adapt_gt and its tile grid): this run's largest,
    // or the whole fit's when this run is a shard of it (adapt_pmax)
    p_max_all = std::max<int64_t>(*std::max_element(npar.begin(), npar.end()), opt->adapt_pmax);
    // limits of the adaptation window, checked before anything is allocated or launched: the
    // adaptation kernel's LDS (the window's run table grows with adaptint) and the chain kernels'
    // 32-bit window-log offsets (adaptint * ld)
    if (opt->adaptint > 0 && tci::dram_adapt_lds_bytes(p_max_all, opt->adaptint) > 160 * 1024)
      return fail(ctx, TCI_ERANGE, "tci_dram_run: adaptint " + std::to_string(opt->adaptint) +
                                       " needs more LDS than a CU has for the adaptation at P = " +
                                       std::to_string(p_max_all));
    if ((opt->adaptint > 0 ? opt->adaptint : 100) * ld >= (int64_t)INT32_MAX)
      return fail(ctx, TCI_ERANGE, "tci_dram_run: adaptint * ld must be < 2^31");
    // Chunk of chain rows per fused-engine pass (its draws buffer holds one chunk; at most the next
    // adaptation row) and the window slots per chain: the covupd window (adaptint rows), which is also
    // every engine's per-row log.
    ai = opt->adaptint;
    DW = tci::draw_stride(ld);
    const int64_t chunk_cap =
        std::max<int64_t>(32, (int64_t)(((size_t)tci::kDrawsGiB << 30) / (n * (size_t)DW * sizeof(double))));
    // Without adaptation the window is 100 rows: the records' merge partition (the same for every engine)
    // and the batched engine's graph block stay small (a 1,000-row window made the batched engine run up
    // to 1,000 steps as plain launches before its first graph replay).
    win = ai > 0 ? ai : 100;
    chunk = std::min<int64_t>(win, chunk_cap);
    if (opt->max_chunk > 0) chunk = std::min<int64_t>(chunk, opt->max_chunk);
    n_keep = opt->thin > 0 ? (opt->n_steps + opt->thin - 1) / opt->thin : 0;
    return TCI_OK;
  }

  // ---- phase: every device array of the run.
  int alloc() {
    TCI_HIP(ctx, hipSetDevice(ctx->device));
    s = ctx->stream;
    st.n_chains = n_chains;
    st.ld = ld;
#define TCI_ALLOC(field, T, count)                                  \
    do {                                                              \
      st.field = A.alloc<T>((count), &e);                             \
      if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram " #field ")"); \
    } while (0)
    d_cell = A.alloc<int32_t>(n, &e);
    d_key = A.alloc<int64_t>(n, &e);
    d_npar = A.alloc<int32_t>(n, &e);
    d_nobs = A.alloc<int32_t>(n, &e);
    d_gshape = A.alloc<double>(n, &e);
    d_lower = A.alloc<double>(n * L, &e);
    d_upper = A.alloc<double>(n * L, &e);
    d_pmu = A.alloc<double>(n * L, &e);
    d_psig = A.alloc<double>(n * L, &e);
    d_qdiag = A.alloc<double>(n * L, &e);
    d_s20 = A.alloc<double>(n, &e);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram inputs)");
    st.cell = d_cell;
    st.key = d_key;
    st.npar = d_npar;
    st.nobs = d_nobs;
    st.gshape = d_gshape;
    st.lower = d_lower;
    st.upper = d_upper;
    st.pmu = d_pmu;
    st.psig = d_psig;
    TCI_ALLOC(theta, double, n * L);
    TCI_ALLOC(ss, double, n);
    TCI_ALLOC(prior, double, n);
    TCI_ALLOC(sigma2, double, n);
    TCI_ALLOC(Rd, double, n * tci::dram_tri_stride(L));
    TCI_ALLOC(cov, double, n * tci::dram_cov_stride(L));
    TCI_ALLOC(work, double, p_max_all > tci::kAdaptGtFrom ? n * (size_t)((L + 15) / 16 * 16) * ((L + 15) / 16 * 16) : 1);
    TCI_ALLOC(cmean, double, n * L);
    TCI_ALLOC(wsum, double, n);
    TCI_ALLOC(window, double, n * (size_t)win * L);
    TCI_ALLOC(wsumv, double, n * L);
    TCI_ALLOC(wacc1, double, n * L);
    TCI_ALLOC(wacc2, double, n * L);
    TCI_ALLOC(s2acc, double, n * 3);
    TCI_ALLOC(s2log, double, n * (size_t)win);
    TCI_ALLOC(runf, uint8_t, n * (size_t)win);
    TCI_ALLOC(prop1, double, n * L);
    TCI_ALLOC(prop2, double, n * L);
    TCI_ALLOC(act1, uint8_t, n);
    TCI_ALLOC(act2, uint8_t, n);
    TCI_ALLOC(acc1, uint8_t, n);
    TCI_ALLOC(ss1, double, n);
    TCI_ALLOC(ss2, double, n);
    TCI_ALLOC(prior1, double, n);
    TCI_ALLOC(a12, double, n);
    TCI_ALLOC(naccept, int32_t, n);
    TCI_ALLOC(nrej_win, int32_t, n);
    TCI_ALLOC(nevals, int64_t, n);
    TCI_ALLOC(smean, double, n * L);
    TCI_ALLOC(sm2, double, n * L);
    TCI_ALLOC(s2sum, double, n);
    TCI_ALLOC(sq_mean, double, n);
    TCI_ALLOC(sq_m2, double, n);
    TCI_ALLOC(step, int64_t, 1);
#if TCI_CHAIN_PROFILE || TCI_ADAPT_PROFILE
    TCI_ALLOC(prof, int64_t, 32);
    TCI_HIP(ctx, hipMemsetAsync(st.prof, 0, 32 * sizeof(int64_t), ctx->stream));
#endif
    if (n_keep > 0 && (red.sout || red.cout || red.qout || red.dout || lout || rhat) && !(out->chain || out->s2chain)) {
      // the chain is kept on the device for the statistics alone: running out of memory is the caller's to handle
      st.chain_out = A.alloc<double>((size_t)n_keep * n * L, &e);
      if (e == hipSuccess) st.s2_out = A.alloc<double>((size_t)n_keep * n, &e);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, TCI_ENOMEM, std::string(red.sout ? "tci_dram_run_stats" : red.cout ? "tci_dram_run_cov" : rhat ? rhat->who : "tci_dram_run_reduced") +
                                         ": the device chain (" +
                                         std::to_string((size_t)n_keep * n * L * sizeof(double)) + " bytes) does not fit");
      }
      TCI_HIP(ctx, hipMemsetAsync(st.chain_out, 0, (size_t)n_keep * n * L * sizeof(double), ctx->stream));
    } else if (n_keep > 0 && (out->chain || out->s2chain)) {
      TCI_ALLOC(chain_out, double, (size_t)n_keep * n * L);
      TCI_ALLOC(s2_out, double, (size_t)n_keep * n);
      // entries past a chain's P are never written: zero them so outputs are deterministic
      TCI_HIP(ctx, hipMemsetAsync(st.chain_out, 0, (size_t)n_keep * n * L * sizeof(double), ctx->stream));
    }
#undef TCI_ALLOC
    return TCI_OK;
  }

  // ---- phase: the inputs onto the device, the kernels' parameters, the ladders' swaps, and every chain's first row.
  int upload() {
    TCI_HIP(ctx, hipMemcpyAsync(d_cell, cell_id, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    std::vector<int64_t> keys(n);
    for (size_t c = 0; c < n; ++c) keys[c] = opt->chain_keys ? opt->chain_keys[c] : (int64_t)c;
    TCI_HIP(ctx, hipMemcpyAsync(d_key, keys.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_nobs, nobs.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_lower, lower, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_upper, upper, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_pmu, prior_mu, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_psig, prior_sig, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_qdiag, qcov_diag, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_s20, s20.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(d_gshape, gshape.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemcpyAsync(st.theta, theta0, n * L * sizeof(double), hipMemcpyHostToDevice, s));
    TCI_HIP(ctx, hipMemsetAsync(st.wsum, 0, n * sizeof(double), s));
    TCI_HIP(ctx, hipMemsetAsync(st.act2, 0, n, s));
    p.seed = opt->seed;
    p.ntry = opt->ntry;
    p.updatesigma = opt->updatesigma;
    p.drscale = opt->drscale;
    p.adascale = opt->adascale;
    p.qcovadj = opt->qcovadj;
    p.burnin_scale = opt->burnin_scale;
    p.adaptint = opt->adaptint;
    p.burnintime = opt->burnintime;
    p.stats_from = std::max<int64_t>(opt->stats_from, 1);
    p.thin = opt->thin;
    p.n_keep = n_keep;
    p.win = win;
    // the ladders' swap: one event after every swap_every-th window that is not the run's last row
    n_events = swap_every > 0 ? (opt->n_steps - 1) / win / swap_every : 0;
    log_rows = topt && tout && (tout->swap_logr || tout->swap_acc)
                                 ? std::min<int64_t>(n_events, std::max<int64_t>(tout->swap_log_rows, 0))
                                 : 0;
    if (topt && !pair_a.empty() && n_events > 0) {
      const size_t np = pair_a.size();
      int32_t* d_pa = A.alloc<int32_t>(np, &e);
      int32_t* d_pb = A.alloc<int32_t>(np, &e);
      int32_t* d_pr = A.alloc<int32_t>(np, &e);
      double* d_beta = A.alloc<double>(n, &e);
      sw.tried = A.alloc<int32_t>(n, &e);
      sw.accepted = A.alloc<int32_t>(n, &e);
      if (log_rows > 0) {
        sw.logr = A.alloc<double>((size_t)log_rows * n, &e);
        sw.acc = A.alloc<uint8_t>((size_t)log_rows * n, &e);
      }
      if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram swap)");
      TCI_HIP(ctx, hipMemcpyAsync(d_pa, pair_a.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, s));
      TCI_HIP(ctx, hipMemcpyAsync(d_pb, pair_b.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, s));
      TCI_HIP(ctx, hipMemcpyAsync(d_pr, pair_r.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, s));
      TCI_HIP(ctx, hipMemcpyAsync(d_beta, beta.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
      TCI_HIP(ctx, hipMemsetAsync(sw.tried, 0, n * sizeof(int32_t), s));
      TCI_HIP(ctx, hipMemsetAsync(sw.accepted, 0, n * sizeof(int32_t), s));
      if (log_rows > 0) {
        TCI_HIP(ctx, hipMemsetAsync(sw.logr, 0xFF, (size_t)log_rows * n * sizeof(double), s));  // all ones: a NaN
        TCI_HIP(ctx, hipMemsetAsync(sw.acc, 0, (size_t)log_rows * n, s));
      }
      sw.pair_a = d_pa;
      sw.pair_b = d_pb;
      sw.pair_r = d_pr;
      sw.n_pairs = (int64_t)np;
      sw.beta = d_beta;
      sw.swap_every = swap_every;
      sw.n_steps = opt->n_steps;
      sw.n_events = log_rows;
      swp = &sw;
    }
    // initial state: R = chol(J0), prior, sigma2, the initial ssfun call, chain row 1
    if ((rc = tci::dram_launch_init(st, d_qdiag, d_s20, s)) != TCI_OK) return fail(ctx, rc, "dram init launch");
    if ((rc = tci::launch(ctx->kp, ctx->rpl, tci::MODE_SS, st.theta, ld, d_cell, nullptr, n_chains, st.ss, nullptr, 0,
                          s)) != TCI_OK)
      return fail(ctx, rc, "initial ssfun launch");
    if ((rc = tci::dram_launch_init_stats(st, p, s)) != TCI_OK) return fail(ctx, rc, "dram stats launch");
    if (win == 1) {  // one-row windows: row 1 is a window of its own
      const int64_t one = 1;
      TCI_HIP(ctx, hipMemcpyAsync(st.step, &one, sizeof(int64_t), hipMemcpyHostToDevice, s));
      if ((rc = tci::dram_launch_stats(st, p, s)) != TCI_OK) return fail(ctx, rc, "dram stats launch");
    }
    const int64_t two = 2;
    TCI_HIP(ctx, hipMemcpyAsync(st.step, &two, sizeof(int64_t), hipMemcpyHostToDevice, s));
    return TCI_OK;
  }

  // ---- phase: the fused engines (FUSED: one workgroup per chain, WALK: one wavefront): steps 2 .. n_steps.
  int fused_steps(tci::LaunchTimer* tm) {
    // Chunks of chain rows up to the next adaptation row (and at most p.chunk rows: the draws
    // buffer holds one chunk); k_chain leaves *st.step at the chunk end. Per chunk: the draws pass
    // and the walk (dram_launch_chain, which also keeps a completed window's records), and at an
    // adaptation row the adaptation.
    p.chunk = chunk;
    st.draws = A.alloc<double>(n * (size_t)p.chunk * DW, &e);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram draws)");
    std::vector<std::pair<int64_t, int64_t>> chunks;
    for (int64_t next = 2; next <= opt->n_steps;) {
      int64_t end = std::min<int64_t>(opt->n_steps, next + p.chunk - 1);
      end = std::min<int64_t>(end, ((next + win - 1) / win) * win);  // chunks never cross a window
      chunks.emplace_back(next, end);
      next = end + 1;
    }
    // k_chain's engine splits the draws (DramParams::split; TCI_DRAWS_SPLIT=0 keeps them in one
    // launch): chunk i + 1's normals and scalar draws go into the other of two draws buffers, drawn by
    // extra workgroups of chunk i's k_chain launch in the CU slots its chains leave free; k_draws then
    // only multiplies by the adapted R. The first chunk's: one k_draws_rng launch.
    // Only while the chains leave slots free (at most two chain workgroups per CU, AUTO's FUSED range):
    // past that the extra workgroups would wait behind the chains. And only while the units' dynamic LDS
    // fits a CU beside k_chain's static __shared__ (k_chain<8>: 103,712 B, so up to ld = 468); longer
    // rows keep the one-launch draws pass -- the same bits.
    const char* split_env = getenv("TCI_DRAWS_SPLIT");
    p.split = !p.walk && n_chains < 2 * (int64_t)std::max(n_cu, 1) && !(split_env && split_env[0] == '0') ? 1 : 0;
    if (p.split) {
      const int64_t chain_static = tci::dram_chain_static_lds_bytes(ctx->rpl, ctx->kp.n_seg);
      if (chain_static < 0 || chain_static + tci::dram_draws_rng_lds_bytes(ld) > 160 * 1024) p.split = 0;
    }
    double* dbuf[2] = {st.draws, st.draws};
    int rng_wgs = 0;
    if (p.split && !chunks.empty()) {
      dbuf[1] = A.alloc<double>(n * (size_t)p.chunk * DW, &e);
      if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram draws, second buffer)");
      // the workgroup slots the chains leave (two per CU), at least a quarter of the CUs
      const char* w_env = getenv("TCI_RNG_WGS");
      rng_wgs = w_env && atoi(w_env) > 0 ? atoi(w_env)
                                         : (int)std::max<int64_t>(2 * (int64_t)n_cu - n_chains, n_cu / 4);
      if ((rc = tci::dram_launch_draws_rng(st, p, chunks[0].first, chunks[0].second, 4 * std::max(n_cu, 1), s, tm)) !=
          TCI_OK)
        return fail(ctx, rc, "dram draws launch");
    }
    for (size_t i = 0; i < chunks.size() && rc == TCI_OK; ++i) {
      const int64_t next = chunks[i].first, end = chunks[i].second;
      const int rec = end % win == 0 || end == opt->n_steps;  // the records kept in the chain kernel
      tci::DramState sc = st;
      sc.draws = dbuf[i & 1];
      // the next chunk's buffer was last read by chunk i - 1's walk, which ended before this launch
      tci::ChainNext nx{dbuf[(i + 1) & 1], 0, -1, rng_wgs};
      if (i + 1 < chunks.size()) {
        nx.s_begin = chunks[i + 1].first;
        nx.s_end = chunks[i + 1].second;
      }
      rc = tci::dram_launch_chain(sc, p, ctx->kp, ctx->rpl, next, end, rec, s, tm,
                                  p.split && i + 1 < chunks.size() ? &nx : nullptr);
      if (rc == TCI_OK && ai > 0 && end % ai == 0) rc = tci::dram_launch_adapt(sc, p, s, tm);
      if (rc == TCI_OK && swp && end % win == 0 && end < opt->n_steps) rc = tci::dram_launch_swap(sc, p, sw, s);
    }
    return TCI_OK;
  }

  // ---- phase: the batched engine, one launch per kernel and step.
  // The step loop. Steps 2 .. n_steps; adaptation after steps that are multiples of adaptint.
  // Blocks of adaptint steps (aligned so that each ends on an adaptation step) are captured once
  // as a hipGraph and replayed; the head (steps 2..adaptint) and the tail run as plain launches.
  int batched_steps(StepGraph* g) {
    int64_t next = 2;  // next step number to enqueue
    auto plain = [&](int64_t upto) {  // steps next .. upto
      for (; next <= upto && rc == TCI_OK; ++next)
        rc = enqueue_step(ctx, st, p, s, next % win == 0, ai > 0 && next % ai == 0, swp);
    };
    const int64_t G = win;  // graph blocks of one window (win = adaptint when adapting)
    plain(std::min<int64_t>(win, opt->n_steps));  // head: up to the first window's end
    const int64_t blocks = (opt->n_steps - next + 1) / G;
    if (rc == TCI_OK && blocks > 0) {
      TCI_HIP(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      int crc = TCI_OK;
      for (int64_t k = 0; k < G && crc == TCI_OK; ++k) crc = enqueue_step(ctx, st, p, s, k == G - 1, ai > 0 && k == G - 1, swp);
      hipError_t ce = hipStreamEndCapture(s, &g->graph);
      if (crc != TCI_OK || ce != hipSuccess) return fail(ctx, TCI_EHIP, "DRAM step graph capture failed");
      e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
      if (e != hipSuccess) return hip_fail(ctx, e, "hipGraphInstantiate");
      for (int64_t b = 0; b < blocks && e == hipSuccess; ++b) e = hipGraphLaunch(g->exec, s);
      next += blocks * G;
    }
    if (e == hipSuccess) plain(opt->n_steps);  // tail
    return TCI_OK;
  }

  // ---- phase: the step loop between its two events, on the engine the options and the sizes pick.
  int run_steps() {
    EventTimer events;
    hipEvent_t &ev0 = events.ev[0], &ev1 = events.ev[1];
    TCI_HIP(ctx, hipEventCreate(&ev0));
    TCI_HIP(ctx, hipEventCreate(&ev1));
    TCI_HIP(ctx, hipEventRecord(ev0, s));
    p.pmax = p_max_all;
    // the fused engine's draws pass keeps a chain's R (packed fp32) and a tile of normals and products
    // in LDS: it must fit a CU (160 KB). AUTO picks it whenever it fits: measured on config 4 (10,000
    // chains x 200 points, 39 per CU) its chain walk + draws pass take 209 us per step against 1950 us
    // for the batched engine's per-step kernels, which stage every chain's R once per stage.
    const int64_t fused_lds = tci::dram_chain_lds_bytes(ld, ctx->rpl);
    const bool fused_fits = ctx->rpl > 0 && fused_lds <= 160 * 1024;  // long cells: the batched engine
    StepGraph graph;
    // WALK (one wavefront per chain) once k_chain's one-workgroup-per-chain layout would need more
    // than one round of resident workgroups (two chains per CU).
    n_cu = 0;
    TCI_HIP(ctx, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    fused = opt->engine == TCI_DRAM_FUSED || opt->engine == TCI_DRAM_WALK;
    p.walk = opt->engine == TCI_DRAM_WALK ? 1 : 0;
    if (opt->engine == TCI_DRAM_AUTO) {
      fused = fused_fits;
      p.walk = n_chains > 2 * (int64_t)std::max(n_cu, 1) ? 1 : 0;
    }
    if (fused && !fused_fits) return fail(ctx, TCI_ERANGE, "tci_dram_run: rows too long for the fused engine");
    for (int k = 0; k < 4; ++k) {
      out->kernel_ms[k] = 0.0;
      out->kernel_launches[k] = 0;
    }
    tci::LaunchTimer timer;
    tci::LaunchTimer* tm = opt->kernel_times && fused ? &timer : nullptr;
    const int started = fused ? fused_steps(tm) : batched_steps(&graph);
    if (started != TCI_OK) return started;
    // the last, partial window's records (the fused engines: kept by the last chunk's kernel)
    if (e == hipSuccess && rc == TCI_OK && opt->n_steps % win != 0 && !(fused && opt->n_steps >= 2)) {
      const int64_t last = opt->n_steps;
      rc = hipMemcpyAsync(st.step, &last, sizeof(int64_t), hipMemcpyHostToDevice, s) == hipSuccess ? TCI_OK : TCI_EHIP;
      if (rc == TCI_OK) rc = tci::dram_launch_stats(st, p, s);
    }
    const hipError_t ge = e;
    TCI_HIP(ctx, hipEventRecord(ev1, s));
    TCI_HIP(ctx, hipStreamSynchronize(s));
    graph.reset();
#if TCI_CHAIN_PROFILE || TCI_ADAPT_PROFILE
    {
      int64_t ph[32];
      TCI_HIP(ctx, hipMemcpy(ph, st.prof, sizeof(ph), hipMemcpyDeviceToHost));
      // TCI_CHAIN_PROFILE=1: slots 0-6 are wave 0's cycles per phase; slot 5 also counts the rounds
      // in its bits 40+ (decoded here). =2: per-wave barrier waits (0-3) and pre-barrier work (4-7).
      // TCI_ADAPT_PROFILE: thread 0's cycles per adaptation phase. All summed over the chains.
      double rounds = 0.0;
      int nslots = 8;
#if TCI_CHAIN_PROFILE == 1 || TCI_CHAIN_PROFILE == 3
      // =3: slots 8 w + k, wave w's cycles per phase (slot 8 w + 5 also counts the rounds)
      nslots = TCI_CHAIN_PROFILE == 3 ? 32 : 8;
      rounds = (double)((uint64_t)ph[5] >> 40) / (double)n;
      for (int w = 0; w < nslots / 8; ++w) ph[8 * w + 5] = (int64_t)((uint64_t)ph[8 * w + 5] & ((1ull << 40) - 1));
#endif
      std::fprintf(stderr, "{\"cycles_per_chain\": [");
      for (int k = 0; k < nslots; ++k) std::fprintf(stderr, "%s%.1f", k ? ", " : "", (double)ph[k] / (double)n);
      std::fprintf(stderr, "], \"rounds_per_chain\": %.1f}\n", rounds);
    }
#endif
    if (ge != hipSuccess) return hip_fail(ctx, ge, "DRAM step replay");
    if (rc != TCI_OK) return fail(ctx, rc, "DRAM step launch");
    if (tm) tm->collect(out->kernel_ms, out->kernel_launches);
    float ms = 0.f;
    TCI_HIP(ctx, hipEventElapsedTime(&ms, ev0, ev1));
    out->elapsed_ms = ms;
    return TCI_OK;
  }

  // ---- phase: the run's outputs to the host.
  int read_outputs() {
    const size_t L2 = L * L;
    std::vector<double> smean(n * L), sm2(n * L), s2sum(n), sqm(n), sqm2(n);
    std::vector<int32_t> nacc(n);
    std::vector<int64_t> nev(n);
    TCI_HIP(ctx, hipMemcpy(smean.data(), st.smean, n * L * sizeof(double), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(sm2.data(), st.sm2, n * L * sizeof(double), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(s2sum.data(), st.s2sum, n * sizeof(double), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(sqm.data(), st.sq_mean, n * sizeof(double), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(sqm2.data(), st.sq_m2, n * sizeof(double), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(nacc.data(), st.naccept, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    TCI_HIP(ctx, hipMemcpy(nev.data(), st.nevals, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    const double nrow_stats = (double)std::max<int64_t>(opt->n_steps - p.stats_from + 1, 0);
    for (size_t c = 0; c < n; ++c) {
      for (size_t j = 0; j < L; ++j) {
        if (out->mean) out->mean[c * L + j] = (int64_t)j < npar[c] && nrow_stats > 0 ? smean[c * L + j] : NAN;
        if (out->std)
          out->std[c * L + j] = (int64_t)j < npar[c] && nrow_stats > 0 ? std::sqrt(sm2[c * L + j] / nrow_stats) : NAN;
      }
      if (out->sigma_mean) out->sigma_mean[c] = std::sqrt(s2sum[c] / (double)opt->n_steps);
      if (out->sigma_std) out->sigma_std[c] = std::sqrt(sqm2[c] / (double)opt->n_steps);
      if (out->accept_rate) out->accept_rate[c] = opt->n_steps > 1 ? nacc[c] / (double)(opt->n_steps - 1) : 0.0;
      if (out->n_evals) out->n_evals[c] = nev[c];
    }
    if (topt && tout) {
      tci_temper_outputs* to = tout;
      to->n_events = n_events;
      if (to->swap_tried) {
        if (swp) TCI_HIP(ctx, hipMemcpy(to->swap_tried, sw.tried, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        else std::fill(to->swap_tried, to->swap_tried + n, 0);
      }
      if (to->swap_accepted) {
        if (swp) TCI_HIP(ctx, hipMemcpy(to->swap_accepted, sw.accepted, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        else std::fill(to->swap_accepted, to->swap_accepted + n, 0);
      }
      if (to->swap_logr && log_rows > 0) {
        if (swp) TCI_HIP(ctx, hipMemcpy(to->swap_logr, sw.logr, (size_t)log_rows * n * sizeof(double), hipMemcpyDeviceToHost));
        else std::fill(to->swap_logr, to->swap_logr + (size_t)log_rows * n, (double)NAN);
      }
      if (to->swap_acc && log_rows > 0) {
        if (swp) TCI_HIP(ctx, hipMemcpy(to->swap_acc, sw.acc, (size_t)log_rows * n, hipMemcpyDeviceToHost));
        else std::fill(to->swap_acc, to->swap_acc + (size_t)log_rows * n, (uint8_t)0);
      }
    }
    if (out->final_theta) TCI_HIP(ctx, hipMemcpy(out->final_theta, st.theta, n * L * sizeof(double), hipMemcpyDeviceToHost));
    if (st.chain_out && out->chain)
      TCI_HIP(ctx, hipMemcpy(out->chain, st.chain_out, (size_t)n_keep * n * L * sizeof(double), hipMemcpyDeviceToHost));
    if (out->qcov_R) {  // the device keeps R as packed FP64 upper triangles
      const int64_t ts = tci::dram_tri_stride((int64_t)L);
      std::vector<double> rd((size_t)n * ts);
      TCI_HIP(ctx, hipMemcpy(rd.data(), st.Rd, rd.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t c = 0; c < n; ++c) {
        double* R = out->qcov_R + c * L2;
        std::fill(R, R + L2, 0.0);
        const int64_t P = npar[c];
        const double* src = rd.data() + c * ts;
        for (int64_t i = 0, e = 0; i < P; ++i)
          for (int64_t j = i; j < P; ++j, ++e) R[i * L + j] = src[e];
      }
    }
    if (st.s2_out && out->s2chain)
      TCI_HIP(ctx, hipMemcpy(out->s2chain, st.s2_out, (size_t)n_keep * n * sizeof(double), hipMemcpyDeviceToHost));
    return TCI_OK;
  }

  // ---- phase: the reductions asked for, each on the device chain's rows from the first one in the window.
  int reduce() {
    if (!(red.sout || red.cout || red.qout || red.dout || lout || rhat)) return TCI_OK;  // no device chain, perhaps
    const double* chain = st.chain_out + (size_t)keep_k0 * n * L;
    const double* s2 = st.s2_out + (size_t)keep_k0 * n;
    if (red.sout && (rc = chainstats_device(ctx, "tci_dram_run_stats", chain, s2, keep_rows, n_chains, ld, st.npar, max_lag,
                                            red.sout)) != TCI_OK)
      return rc;
    if (red.cout && (rc = chaincov_device(ctx, "tci_dram_run_cov", chain, keep_rows, n_chains, ld, st.npar, cov_group,
                                          red.cout)) != TCI_OK)
      return rc;
    if (red.qout && (rc = chainquant_device(ctx, "tci_dram_run_reduced", chain, s2, keep_rows, n_chains, ld, st.npar, q_probs,
                                            q_nq, red.qout)) != TCI_OK)
      return rc;
    if (red.dout && (rc = chaindens_device(ctx, "tci_dram_run_reduced", chain, s2, keep_rows, n_chains, ld, st.npar, d_G, d_B,
                                           d_bws, d_scratch, red.dout)) != TCI_OK)
      return rc;
    if (lout && (rc = chainlp_device(ctx, "tci_dram_run_lp", chain, s2, keep_rows, n_chains, ld, st.cell, st.npar, st.pmu,
                                     st.psig, l_scratch, lout)) != TCI_OK)
      return rc;
    if (rhat && (rhat->rout || rhat->eout) &&
        (rc = chainrhat_device(ctx, rhat->who, chain, s2, keep_rows, n_chains, ld, st.npar, r_groups, rhat->n_groups,
                               rhat->rout, rhat->eout && rhat->eopt ? rhat->eopt->max_lag : 0, rhat->eout)) != TCI_OK)
      return rc;
    if (rhat && rhat->kout)
      return chainrank_device(ctx, rhat->who, chain, s2, keep_rows, n_chains, ld, st.npar, r_groups, rhat->n_groups, k_opt,
                              rhat->kout);
    return TCI_OK;
  }

  int go() {
    if (!ctx) return TCI_EINVAL;
    int r;
    if ((r = check()) != TCI_OK || (r = plan()) != TCI_OK || (r = alloc()) != TCI_OK || (r = upload()) != TCI_OK ||
        (r = run_steps()) != TCI_OK || (r = read_outputs()) != TCI_OK)
      return r;
    return reduce();
  }
};

// the arguments every tci_dram_run* entry point takes, in DramRun's order
#define TCI_RUN_ARGS ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld, out

}  // namespace

extern "C" {

int tci_dram_defaults(tci_dram_options* o) {
  if (!o) return TCI_EINVAL;
  o->n_steps = 20000;     // TranscriptionCycleMCMC.m:40
  o->burnintime = 10000;  // :39, :267
  o->adaptint = 100;      // :268
  o->ntry = 2;            // 'dram' (:269)
  o->updatesigma = 1;     // :265
  o->drscale = 5.0;
  o->adascale = 0.0;
  o->qcovadj = 1e-5;
  o->burnin_scale = 10.0;
  o->stats_from = 10000;  // chain(n_burn:end, :) (:276)
  o->thin = 0;
  o->seed = 20201028;
  o->engine = TCI_DRAM_AUTO;
  o->max_chunk = 0;
  o->chain_keys = nullptr;
  o->adapt_pmax = 0;
  o->kernel_times = 0;
  return TCI_OK;
}

int tci_dram_run(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                 const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                 const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                 tci_dram_outputs* out) {
  return DramRun{TCI_RUN_ARGS}.go();
}

int tci_dram_run_stats(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                       const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                       const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                       tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout) {
  if (!ctx) return TCI_EINVAL;
  if (!sout) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: null statistics outputs");
  DramRun r{TCI_RUN_ARGS};
  r.red.sopt = sopt;
  r.red.sout = sout;
  return r.go();
}

int tci_dram_run_cov(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                     const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                     const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                     tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout,
                     const tci_chaincov_options* copt, tci_chaincov_outputs* cvout) {
  if (!ctx) return TCI_EINVAL;
  if (!cvout) return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: null covariance outputs");
  DramRun r{TCI_RUN_ARGS};
  r.red.sopt = sopt;
  r.red.sout = sout;
  r.red.copt = copt;
  r.red.cout = cvout;
  return r.go();
}

int tci_dram_run_reduced(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                         const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                         const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                         tci_dram_outputs* out, const tci_dram_reductions* red) {
  if (!ctx) return TCI_EINVAL;
  if (!red) return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: null reductions");
  DramRun r{TCI_RUN_ARGS};
  r.red = *red;
  return r.go();
}

int tci_dram_run_rhat(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                      const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                      const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                      tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                      const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout) {
  if (!ctx) return TCI_EINVAL;
  if (!rout) return fail(ctx, TCI_EINVAL, "tci_dram_run_rhat: null group reduction outputs");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_rhat: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout};
  DramRun r{TCI_RUN_ARGS};
  if (red) r.red = *red;
  r.rhat = &ask;
  return r.go();
}

int tci_dram_run_ess(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                     const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                     const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                     tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                     const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                     tci_chainess_outputs* eout) {
  if (!ctx) return TCI_EINVAL;
  if (!eout) return fail(ctx, TCI_EINVAL, "tci_dram_run_ess: null effective sample size outputs");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_ess: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_ess", eopt, eout};
  DramRun r{TCI_RUN_ARGS};
  if (red) r.red = *red;
  r.rhat = &ask;
  return r.go();
}

int tci_dram_run_rank(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                      const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                      const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                      tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                      const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                      tci_chainess_outputs* eout, const tci_chainrank_options* kopt, tci_chainrank_outputs* kout) {
  if (!ctx) return TCI_EINVAL;
  if (!kout) return fail(ctx, TCI_EINVAL, "tci_dram_run_rank: null rank diagnostics outputs");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_rank: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_rank", eopt, eout, kopt, kout};
  DramRun r{TCI_RUN_ARGS};
  if (red) r.red = *red;
  r.rhat = &ask;
  return r.go();
}

int tci_dram_run_lp(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                    const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                    const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                    tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                    const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                    tci_chainess_outputs* eout, const tci_chainlp_options* lopt, tci_chainlp_outputs* lout) {
  if (!ctx) return TCI_EINVAL;
  if (!lout) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: null log-posterior outputs");
  DramRun r{TCI_RUN_ARGS};
  if (red) r.red = *red;
  r.lopt = lopt;
  r.lout = lout;
  if (!group) return r.go();
  if (!rout && !eout) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: group without group reduction outputs");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_lp", eopt, eout};
  r.rhat = &ask;
  return r.go();
}

int tci_temper_defaults(tci_temper_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->swap_every = 1;
  return TCI_OK;
}

int tci_dram_run_tempered(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                          const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                          const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                          tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                          const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_temper_options* topt,
                          tci_temper_outputs* tout) {
  if (!ctx) return TCI_EINVAL;
  tci_temper_options def;
  tci_temper_defaults(&def);
  DramRun r{TCI_RUN_ARGS};
  if (red) r.red = *red;
  r.topt = topt ? topt : &def;
  r.tout = tout;
  if (!rout) return r.go();
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_tempered: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_tempered"};
  r.rhat = &ask;
  return r.go();
}

}  // extern "C"
