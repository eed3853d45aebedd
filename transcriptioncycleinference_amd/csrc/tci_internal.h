// tci_internal.h -- shared host/device definitions of the MI355X likelihood path.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tci.h"

namespace tci {

// Resident cell table. Every cell owns a fixed-stride block of `cell_stride` records in each
// record array, so a wave can address all of its cell's data from the cell id alone and issue
// every load of an evaluation at once (no dependent meta -> data round trip).
struct CellMeta {
  int32_t n;     // acquisition points N (= grid points M, checked at create)
  int32_t pad;
  double d;      // grid increment of t(1):d:t(end) (SumofSquares...m:29)
  double delta;  // max_j |(t_interp(j+1) - t_interp(j)) - d| over the grid (a few ulps)
  double eps_v;  // fast-path position bound per unit v (tci_kernels.hip): eps = v * eps_v
};

// Per grid step g: the step length and the step's start time (ConstantElongationSim.m:43-45,57).
struct StepRec {
  double dt;
  double t;
};

// Per acquisition point j: interp1 interval k and weight w (SumofSquares...m:55-56) and the
// data (NaN = missing). A point outside the grid has w = NaN and k = 0, so its interpolated
// value is NaN exactly as interp1 returns; padding records (j >= N) are all-NaN.
struct PointRec {
  double w;
  double y1;  // MS2
  double y2;  // PP7
  int32_t k;
  int32_t pad;
};

// One stem-loop segment of one dye (GetFluorFromPolPos.m:21-27,48-52,60-64).
struct SegParams {
  double a;    // loop start (kb)
  double e;    // loop end (kb)
  double phi;  // loopn / 24
  double k;    // phi / (e - a): fractional-occupancy slope
  double ka;   // k * a (the ramp's offset term of the fast-path row sums, theta-independent)
};

// Kernel arguments: device pointers of the resident cell table + the construct.
struct KParams {
  const CellMeta* cells;
  const StepRec* steps;      // uniform grid t_interp (SumofSquares...m:30) and its steps
  const StepRec* steps_raw;  // raw times t and raw steps (forward on raw t, TranscriptionCycleMCMC.m:307)
  const PointRec* points;
  const double* thr;         // 64 per-lane thresholds of the distance cuts (tci_eval.h distance_cuts): lane
                             // 1 + 4k .. 4 + 4k = MS2 a, MS2 e, PP7 a, PP7 e of segment k; 0 elsewhere
  int64_t n_cells;
  int64_t cell_stride;       // records per cell in steps/steps_raw/points (64*(rows_per_lane+1); long cells: N_max
                             // rounded up to 64)
  int64_t max_n;             // longest cell (points): sizes the long-cell kernel's LDS
  double L0;            // gene length before tau*v (GetFluorFromPolPos.m:19)
  double emax;          // max loop end over all segments and dyes
  int32_t n_seg;
  int32_t force_exact;  // test hook: bit 0 = always run the exact sequential counter scan,
                        //            bit 1 = always run the exact per-(row, cohort) position sweep
  SegParams ms2[TCI_MAX_SEG];
  SegParams pp7[TCI_MAX_SEG];
};

enum Mode : int { MODE_SS = 0, MODE_FWD_INTERP = 1, MODE_FWD_RAW = 2 };

// Allow `func` up to `bytes` of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize). The
// attribute is set once per kernel and process, raised only when a larger size is asked for: the
// DRAM engines launch the same kernels every chunk, and the host call costs a driver round trip.
// Returns TCI_OK or TCI_EHIP. Thread-safe.
int ensure_dyn_lds(const void* func, size_t bytes);

// Launch the batched kernel (device pointers). rpl = rows per lane (1,2,4,8); 0 = the long-cell
// kernel (tci_tile_kernel, any N up to TCI_MAX_POINTS).
// out0/out1: MODE_SS -> out0 = ss[B]; forward modes -> MS2/PP7 rows of ld_out.
int launch(const KParams& kp, int rpl, int mode, const double* theta, int64_t ld_theta,
           const int32_t* cell_id, const uint8_t* active, int64_t B, double* out0, double* out1,
           int64_t ld_out, void* stream);

// Quantiles over samples (tci_predict.hip, k_quantile). sim0/sim1: the forward launch's MS2/PP7 rows,
// S consecutive rows of ld_out per selected cell; row_cell: the forward launch's cell id per row;
// out0/out1: [n_sel * nq][ld_out], entries past a cell's N are NaN. probs are host values in [0, 1].
// TCI_EINVAL when the launch would not fit (grid or LDS), TCI_EHIP on a HIP error.
int launch_quantile(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1, int64_t n_sel,
                    int64_t S, int64_t ld_out, const double* probs, int32_t nq, double* out0, double* out1,
                    void* stream);
// The most selected cells one forward + quantile launch pair takes (grid limits).
int quantile_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells);

// Fit checks over samples (tci_fitcheck.hip, k_fitcheck). sim0/sim1 and row_cell as for launch_quantile; sd, lg
// (device): [n_sel * S], sqrt(s2) and log(2 pi s2) of every row; logS = log((double)S). out (device):
// [n_sel][2][6][ld_out] = per dye lppd, p_waic, pit, resid, zbar, z2; unscored points and entries past a cell's N are
// NaN. The data are kp.points. TCI_EINVAL when the launch would not fit (grid or LDS), TCI_EHIP on a HIP error.
int launch_fitcheck(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1,
                    const double* sd, const double* lg, int64_t n_sel, int64_t S, int64_t ld_out, double logS,
                    double* out, void* stream);
// The most selected cells one forward + fitcheck launch pair takes (grid limits).
int fitcheck_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells);

// PSIS-LOO over samples (tci_loocheck.hip, k_loocheck). Arguments as for launch_fitcheck; 32 <= S <= 4096. out
// (device): [n_sel][2][4][ld_out] = per dye elpd_loo, lppd, p_loo, khat; unscored points and entries past a cell's N
// are NaN. TCI_EINVAL when the launch would not fit (grid or LDS), TCI_EHIP on a HIP error.
constexpr int kLcMaxM = 192;  // the tail length M at S = 4096
constexpr int kLcMaxG = 43;   // 30 + floor(sqrt(kLcMaxM)): points of the profile likelihood
int launch_loocheck(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1,
                    const double* sd, const double* lg, int64_t n_sel, int64_t S, int64_t ld_out, double logS,
                    double* out, void* stream);
// The most selected chains one forward + loocheck launch pair takes (grid limits).
int loocheck_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells);
// The tail length M and the profile's point count G for S samples (include/tci.h); TCI_EINVAL outside [32, 4096].
int loocheck_tail(int64_t S, int32_t* M, int32_t* G);

// Chain diagnostics (tci_chainstats.hip) of a device chain [n_rows][n_chains][ld] and, when s2 is not null,
// of s2 [n_rows][n_chains] as column ld of every chain. npar (device, may be null = ld): columns j >= npar[c]
// are padding. stats (device): [5][n_chains * (ld + 1)] doubles = mcerr, tau, Geweke z, Geweke p and the
// column means; win (device): [n_chains * (ld + 1)] windows. Padding and non-finite columns: NaN and -1.
// max_lag 0 = n_rows. Asynchronous on `stream`. TCI_EINVAL on a size the grid cannot take, TCI_EHIP on a HIP error.
int launch_chainstats(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                      const int32_t* npar, int64_t max_lag, double* stats, int32_t* win, void* stream);

// Mean, covariance and correlation (tci_chaincov.hip) of the chains c0 .. c0 + nc - 1 of a device chain
// [n_rows][n_chains][ld], n_rows >= 2. npar (device, may be null = ld): columns j >= npar[c] are padding.
// mean (device): [n_chains][ld], written for the launch's chains; cov, corr (device): [nc][ld][ld], indexed by
// c - c0. Padding and non-finite columns: NaN. Asynchronous on `stream`. TCI_EINVAL on a size the grid cannot
// take (nc above chaincov_max_chains(ld)), TCI_EHIP on a HIP error.
int launch_chaincov(const double* chain, int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, int64_t c0,
                    int64_t nc, double* mean, double* cov, double* corr, void* stream);
// The most chains one launch_chaincov takes (grid limits).
int64_t chaincov_max_chains(int64_t ld);
// launch_chaincov's mean alone (its k_cc_mean, the same bits) for every chain, n_rows >= 1. mean (device):
// [n_chains][ld]. A chain's s2 [n_rows][n_chains] goes through as a chain of ld = 1 with npar null.
int launch_chain_mean(const double* chain, int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar,
                      double* mean, void* stream);

// Exact quantiles (tci_chainquant.hip) of every column of a device chain [n_rows][n_chains][ld] and, when s2 is
// not null, of s2 [n_rows][n_chains] as column ld of every chain. npar (device, may be null = ld): columns
// j >= npar[c] are padding. probs: nq host values in [0, 1], 1 <= nq <= 16. out (device): [n_chains][nq][ld + 1];
// padding, non-finite columns and column ld without s2 are NaN. Asynchronous on `stream`. TCI_EINVAL on a size
// the grid cannot take or a bad prob, TCI_EHIP on a HIP error.
int launch_chainquant(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                      const int32_t* npar, const double* probs, int32_t nq, double* out, void* stream);

// Densities and histograms (tci_chaindens.hip) of every column of a device chain, laid out and padded as for
// launch_chainquant; n_rows >= 2, 2 <= G <= 256, 1 <= B <= 256, npow = n_rows^(-1/5). scratch (device):
// chaindens_scratch_bytes() bytes, 8-byte aligned. out_d (device): [n_chains][G + 3][ld + 1] doubles, per chain the
// G density rows, then xmin, xmax and bw; out_c (device): [n_chains][B][ld + 1] counts. Padding, non-finite
// columns and column ld without s2 are NaN / -1. Asynchronous on `stream`; launches launch_chainquant for the
// quartiles. TCI_EINVAL on a bad size, TCI_ERANGE on a grid above 2^31 - 1 workgroups, TCI_EHIP on a HIP error.
int launch_chaindens(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, int32_t G, int32_t B, double bw_scale, double npow, void* scratch,
                     double* out_d, int32_t* out_c, void* stream);
// The scratch launch_chaindens needs; TCI_ERANGE when the sizes do not fit the launch grid, TCI_ENOMEM above 2^46 bytes.
int chaindens_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, int32_t G, int32_t B, size_t* bytes);

// Classic and split R-hat, pooled mean and pooled standard deviation (tci_chainrhat.hip) of every group of chains of
// a device chain, laid out and padded as for launch_chainquant; n_rows >= 1. group (device): [n_chains], the group
// of every chain, < 0 = none; g_off (device): [n_groups + 1] and g_list (device): the chains of group g, ascending,
// at g_list[g_off[g] .. g_off[g + 1]) (the CSR form of `group`, built by the host); the chains of a group have one
// npar. scratch (device): chainrhat_scratch_bytes() bytes, 8-byte aligned. out (device): [4][n_groups][ld + 1] =
// rhat, rhat_split, pooled_mean, pooled_std; padding, non-finite columns, column ld without s2 and empty groups are
// NaN. Asynchronous on `stream`. TCI_EINVAL on a bad size, TCI_ERANGE on a grid above 2^31 - 1 workgroups, TCI_EHIP
// on a HIP error.
int launch_chainrhat(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, const int32_t* group, int64_t n_groups, const int32_t* g_off,
                     const int32_t* g_list, void* scratch, double* out, void* stream);
// The scratch launch_chainrhat needs; TCI_ERANGE when the sizes do not fit the launch grid, TCI_ENOMEM above 2^46 bytes.
int chainrhat_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, int64_t n_groups, size_t* bytes);
// Where launch_chainrhat left the per-sequence moments in its scratch: mu, var [3][n_chains * (ld + 1)] (whole chain,
// half A, half B) and state [n_chains * (ld + 1)] (tci_chainrhat_dev.h). Same codes as chainrhat_scratch_bytes.
int chainrhat_scratch_moments(void* scratch, int64_t n_rows, int64_t n_chains, int64_t ld, int64_t n_groups,
                              const double** mu, const double** var, const int32_t** state);

// Multi-chain effective sample size (tci_chainess.hip) of every group of chains of a device chain; arguments as for
// launch_chainrhat, which it launches first for the moments (scratch: chainrhat_scratch_bytes() bytes; rhat_out
// (device): launch_chainrhat's out, its pooled_std feeds mcse). max_lag >= 0 (0 = no cap); cap (device):
// [2][n_groups] = (m L) log10(m L) of the classic and of the split statistic of every group. out_d (device):
// [5][n_groups][ld + 1] = ess, ess_split, tau, tau_split, mcse; out_w (device): [2][n_groups][ld + 1] = window,
// window_split. Padding, non-finite columns, column ld without s2 and empty groups are NaN / -1. Asynchronous on
// `stream`. TCI_EINVAL on a bad size, TCI_ERANGE on a grid above 2^31 - 1 workgroups, TCI_EHIP on a HIP error.
int launch_chainess(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                    const int32_t* npar, const int32_t* group, int64_t n_groups, const int32_t* g_off,
                    const int32_t* g_list, int64_t max_lag, const double* cap, void* scratch, double* rhat_out,
                    double* out_d, int32_t* out_w, void* stream);

// The pooled sort of every (group, column) of a device chain and the chains that follow from it (tci_chainrank.hip;
// include/tci.h has the definition); the chain, npar and the groups (g_off, g_list device; g_off_host the same
// offsets on the host) as for launch_chainrhat. One launch per mode, in this order on one stream:
//   0  the pooled quantiles into qbuf (device): [n_groups][nq + 3][ld + 1] = the quantiles at probs (nq host values),
//      then at 0.5, tail_lo and tail_hi; and the rank scores z of x into zc / zs2;
//   1  the rank scores of |x - med| into zc / zs2, med read from qbuf;
//   2  the indicator x <= q(tail_lo) into zc / zs2;  3  the same for tail_hi (both read qbuf, neither sorts).
// zc (device): [n_rows][n_chains][ld]; zs2 (device): [n_rows][n_chains], required with s2. Only the entries of a
// group's real columns are written: the caller fills both with NaN once, which is what padding and the chains of no
// group keep (launch_chainrank_fill). A column with a non-finite entry gets NaN in qbuf and in every entry of zc / zs2.
// A group of N = M n_rows <= kRankLdsCap keys is sorted in LDS; a larger one in its slab of gkeys (device):
// chainrank_scratch_keys() keys of 8 bytes (0: no group is that large and gkeys may be null). Asynchronous on
// `stream`. TCI_EINVAL on a bad size, TCI_ERANGE for a group of 2^31 values or more or a grid above 2^31 - 1
// workgroups, TCI_ENOMEM above 2^46 bytes of keys, TCI_EHIP on a HIP error.
// kRankLdsCap: 8,192 keys = 64 KiB of LDS, two workgroups per CU's 160 KiB; it holds the shapes the samplers make
// (4 replicates x 1,000 rows; 64 members x 101 rows).
constexpr int kRankLdsCap = 8192;
int launch_chainrank(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, int64_t n_groups, const int32_t* g_off_host, const int32_t* g_off,
                     const int32_t* g_list, int mode, const double* probs, int32_t nq, double tail_lo, double tail_hi,
                     double* qbuf, void* gkeys, double* zc, double* zs2, void* stream);
// n entries of p (device) set to the quiet NaN the reductions write. Asynchronous on `stream`.
int launch_chainrank_fill(double* p, size_t n, void* stream);
int chainrank_scratch_keys(int64_t n_rows, int64_t ld, int64_t n_groups, const int32_t* g_off, int64_t* stride,
                           size_t* keys);

// Log-posterior trace, best sample and DIC of every chain (tci_chainlp.hip) of a device chain [n_rows][n_chains][ld]
// with its s2 [n_rows][n_chains]; the traces are laid out as s2 is. cell (device): [n_chains], valid ids of cells
// with 7 + N <= ld (the host checks). n_rows * n_chains must stay below 2^31 (TCI_ERANGE), the likelihood launch's
// grid. All asynchronous on `stream`; TCI_EINVAL on a bad size or a null pointer, TCI_EHIP on a HIP error.
//   launch_chainlp_ids     row_cell (device): [n_rows * n_chains], the cell of every (row, chain): the id vector of the
//                          likelihood launch on the chain.
//   launch_chainlp_rows    ss: the likelihood launch's output; mu, sig (device): [n_chains][ld] priors. Writes pri, dev, lp.
//   launch_chainlp_reduce  scal (device): [kChainlpScalars][n_chains] = ss_min, ss_mean, dev_mean, dev_var, lp_best,
//                          ss_best, s2_best, s2_mean, ss_hat, d_hat, p_d, p_v, dic; on entry plane 7 holds the s2 mean
//                          (launch_chain_mean) and plane 8 the SS of theta_mean. theta_mean (device): [n_chains][ld], on
//                          entry launch_chain_mean's; a chain with a non-finite ss, pri or dev gets NaN there, in every
//                          plane of scal and in theta_best, and best_row -1. scratch (device): chainlp_scratch_bytes()
//                          bytes, 8-byte aligned.
constexpr int kChainlpScalars = 13;
int launch_chainlp_ids(const int32_t* cell, int64_t n_rows, int64_t n_chains, int32_t* row_cell, void* stream);
int launch_chainlp_rows(const KParams& kp, const double* chain, const double* s2, const double* ss, const int32_t* cell,
                        const double* mu, const double* sig, int64_t n_rows, int64_t n_chains, int64_t ld, double* pri,
                        double* dev, double* lp, void* stream);
int launch_chainlp_reduce(const KParams& kp, const double* chain, const double* s2, const double* ss, const double* pri,
                          const double* dev, const double* lp, const int32_t* cell, int64_t n_rows, int64_t n_chains,
                          int64_t ld, void* scratch, double* scal, int64_t* best_row, double* theta_best,
                          double* theta_mean, void* stream);
int chainlp_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, size_t* bytes);

// One generation of the mode search (tci_modesearch.hip) on a device population [n_sel][n_pop][ld]; f, ss and pri are
// [n_sel * n_pop], laid out as the rows are. cell_id, s2, keys (device): [n_sel], valid ids of cells with 7 + N <= ld
// (the host checks); lower, upper, mu, sig (device): [n_sel][ld]. 4 <= n_pop <= 4096 and n_sel * n_pop below 2^31
// (TCI_ERANGE). Asynchronous on `stream`; TCI_EINVAL on a bad size or a null pointer, TCI_EHIP on a HIP error.
//   launch_modesearch_trial   gen == 0: pri of every member of pop (keys, lower, upper and trial are not read). gen >= 1:
//                             the trial of every member into trial [n_sel * n_pop][ld] and the trial's prior into pri.
//                             The caller then launches the likelihood kernel on the rows it wrote.
//   launch_modesearch_select  gen == 0: f = ss / s2 + pri of every member (trial, ss_t, pri_t, n_acc are not read). gen >= 1:
//                             an accepted trial replaces its parent in pop, f, ss, pri; n_acc [n_sel] counts them. Both:
//                             best [n_sel] and f_trace [n_sel] (this generation's row); with final_gen also theta_best
//                             [n_sel][ld] and best_vals [3][n_sel] = f, ss, pri of the best member.
int launch_modesearch_trial(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                            const double* lower, const double* upper, const double* mu, const double* sig, int64_t n_sel,
                            int64_t n_pop, int64_t ld, int64_t gen, uint64_t seed, double F, double CR, double* trial,
                            double* pri, void* stream);
int launch_modesearch_select(const KParams& kp, const int32_t* cell_id, const double* s2, const double* trial,
                             const double* ss_t, const double* pri_t, int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen,
                             bool final_gen, double* pop, double* f, double* ss, double* pri, double* f_trace,
                             int32_t* n_acc, int32_t* best, double* best_vals, double* theta_best, void* stream);

// One half-sweep of the DE-MC sampler (tci_demc.hip) on a device population [n_sel][n_pop][ld]; ss, pri, s2, n_acc and
// n_oob are [n_sel * n_pop], laid out as the rows are. In half-sweep h (0 or 1) the n_mov = (n_pop - h + 1) / 2 members
// with i mod 2 == h move; trial [n_sel * n_mov][ld], ss_t, pri_t and active [n_sel * n_mov] hold the moving members
// alone, row t = k * n_mov + (i >> 1). cell_id, keys, sigma2_0 (device): [n_sel], valid ids of cells with 7 + N <= ld
// (the host checks); lower, upper, mu, sig, jitter (device): [n_sel][ld]. 4 <= n_pop <= 4096 and n_sel * n_pop below
// 2^31 (TCI_ERANGE). Asynchronous on `stream`; TCI_EINVAL on a bad size or a null pointer, TCI_EHIP on a HIP error.
//   launch_demc_propose  gen == 0: pri of every member of pop ([n_sel * n_pop]; nothing else is read). gen >= 1: the trial
//                        of every moving member, its prior into pri and its active byte (0: a crossing entry is NaN or
//                        out of bounds, pri is NaN). The caller then launches the likelihood kernel on trial under active.
//   launch_demc_decide   gen == 0: s2 = sigma2_0 and zero counters for every member. gen >= 1: the decision and the
//                        sigma2 draw of every moving member; an accepted trial replaces its parent in pop, ss, pri.
//                        log_row >= 0: logr, acc_log and oob_log (each may be null) [.][n_sel * n_pop] get the moving
//                        members' entries of that row. keep_row >= 0: after the decisions, row keep_row of chain
//                        [.][n_sel * n_pop][ld], s2chain, sschain and prichain [.][n_sel * n_pop] gets every member.
int launch_demc_propose(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                        const double* lower, const double* upper, const double* mu, const double* sig,
                        const double* jitter, int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen, int h, bool jump,
                        uint64_t seed, double gamma0, double CR, double* trial, double* pri, uint8_t* active,
                        void* stream);
int launch_demc_decide(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                       const double* trial, const double* ss_t, const double* pri_t, const uint8_t* active,
                       int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen, int h, uint64_t seed, bool updatesigma,
                       int64_t keep_row, int64_t log_row, double* pop, double* ss, double* pri, double* s2,
                       int32_t* n_acc, int32_t* n_oob, double* chain, double* s2chain, double* sschain,
                       double* prichain, double* logr, uint8_t* acc_log, uint8_t* oob_log, void* stream);

// One generation of the DE-MC(zs) sampler (tci_demczs.hip) on device chains [n_sel][n_pop][ld] and a device archive
// [n_sel][M_cap][ld] of which generation gen reads the first M_g rows (3 <= M_g <= M_cap < 2^24). ss, pri, s2, the
// counters, trial [n_sel * n_pop][ld] and ss_t, pri_t, ljac, move, active [n_sel * n_pop] are laid out as the rows are:
// every chain moves. cell_id, keys, sigma2_0 (device): [n_sel]; lower, upper, mu, sig, jitter (device): [n_sel][ld].
// 1 <= n_pop <= 4096 and n_sel * n_pop below 2^31 (TCI_ERANGE). Asynchronous on `stream`; TCI_EINVAL on a bad size or a
// null pointer, TCI_EHIP on a HIP error.
//   launch_zs_propose  gen == 0: pri of every chain's start (nothing else is read). gen >= 1: the trial of every chain,
//                      its prior, ljac, move (0 parallel, 1 snooker, 2 a null snooker move) and active byte (0: null, or
//                      an entry is NaN or out of bounds; pri is NaN). The caller then launches the likelihood kernel.
//   launch_zs_decide   gen == 0: s2 = sigma2_0 and zero counters. gen >= 1: the decision and the sigma2 draw of every
//                      chain; an accepted trial replaces its parent. log_row >= 0: the five logs (each may be null) get
//                      that row. app_row >= 0: after the decisions chain i's row goes to archive row app_row + i of its
//                      cell. keep_row >= 0: row keep_row of chain, s2chain, sschain and prichain gets every chain.
// The bounds variants (tci_demczs_run_bounds): with bx given, generation gen >= 1 runs the kBounds instantiations of
// k_zs_propose / k_zs_decide (tci_demczs_bounds.hip, a code object of its own), which take the struct as one more
// kernel argument; with bx null the launches are the instantiations without the flag (tci_demczs.hip), whose arguments
// are the ones listed here and nothing else. All pointers are device buffers laid out as the rows are.
struct ZsBounds {
  int reflect;                          // 1: TCI_BOUNDS_REFLECT
  int32_t *n_cross, *oob_lo, *oob_hi;   // [n_sel * n_pop][ld], all three or none (census off)
  const uint8_t* orient;                // [n_sel * n_pop][ld]: the chains' orientation bits; required with reflect
  uint8_t* orient_t;                    // [n_sel * n_pop][ld]: the trials'; required with reflect
  int32_t *n_left_t, *n_refl_t;         // [n_sel * n_pop], required: the two counts of this generation's proposals
};
struct ZsDecideBounds {
  const int32_t *n_left_t, *n_refl_t;   // as k_zs_propose's kBounds instantiation wrote them
  const uint8_t* orient_t;
  uint8_t* orient;                      // null: no orientation rows (reject mode)
  int32_t *n_left_log, *n_refl_log;     // [log_rows][n_sel * n_pop], each may be null
  int32_t* n_reflected;                 // [n_sel * n_pop], required
};
int launch_zs_propose(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                      const double* arch, const double* lower, const double* upper, const double* mu, const double* sig,
                      const double* jitter, int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld,
                      int64_t gen, bool jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial,
                      double* pri, double* ljac, uint8_t* move, uint8_t* active, void* stream, const ZsBounds* bx = nullptr);
int launch_zs_decide(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                     const double* trial, const double* ss_t, const double* pri_t, const double* ljac, const uint8_t* move,
                     const uint8_t* active, int64_t n_sel, int64_t n_pop, int64_t M_cap, int64_t ld, int64_t gen,
                     uint64_t seed, bool updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop,
                     double* arch, double* ss, double* pri, double* s2, int32_t* n_acc, int32_t* n_oob, int32_t* n_null,
                     double* chain, double* s2chain, double* sschain, double* prichain, double* logr, uint8_t* acc_log,
                     uint8_t* oob_log, double* ljac_log, uint8_t* snk_log, void* stream,
                     const ZsDecideBounds* bx = nullptr);
// The launches of the kBounds instantiations (tci_demczs_bounds.hip), which the two above hand a call with bx to.
int launch_zs_propose_bounds(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                      const double* arch, const double* lower, const double* upper, const double* mu, const double* sig,
                      const double* jitter, int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld,
                      int64_t gen, bool jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial,
                      double* pri, double* ljac, uint8_t* move, uint8_t* active, void* stream, const ZsBounds& bx);
int launch_zs_decide_bounds(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                     const double* trial, const double* ss_t, const double* pri_t, const double* ljac, const uint8_t* move,
                     const uint8_t* active, int64_t n_sel, int64_t n_pop, int64_t M_cap, int64_t ld, int64_t gen,
                     uint64_t seed, bool updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop,
                     double* arch, double* ss, double* pri, double* s2, int32_t* n_acc, int32_t* n_oob, int32_t* n_null,
                     double* chain, double* s2chain, double* sschain, double* prichain, double* logr, uint8_t* acc_log,
                     uint8_t* oob_log, double* ljac_log, uint8_t* snk_log, void* stream, const ZsDecideBounds& bx);

}  // namespace tci
