/*
 * tci.h -- C ABI of the MI355X-native TranscriptionCycleInference likelihood path.
 *
 * Drop-in boundary: mcmcstat's model.ssfun handle, ss = ssfun(theta, data), set at
 *   /root/reference/src/TranscriptionCycleMCMC.m:186 (closure over `construct`) and :258,
 *   called by mcmcrun at :273. The handle wraps
 *   SumofSquaresFunction_TranscriptionCycleMCMC(construct,data,x)
 *   (/root/reference/src/SumofSquaresFunction_TranscriptionCycleMCMC.m:1-64), which runs
 *   ConstantElongationSim (src/dependencies/ConstantElongationSim.m:1-67) and
 *   GetFluorFromPolPos (src/GetFluorFromPolPos.m:1-71).
 *
 * The reference's FFI for this path would be a MATLAB MEX gateway; its source is
 * matlab/tci_mex.cpp and the binding is shown in INTEGRATION.md.
 *
 * Conventions: every entry point returns int status (TCI_OK = 0, negative = error) and
 * never throws; tci_last_error(ctx) gives the message. Plain pointers and sizes only.
 * A context is bound to one device and is NOT thread-safe (one context per host thread).
 * Theta layout (TranscriptionCycleMCMC.m:210, SumofSquares...m:35-42):
 *   theta = [v, tau, ton, MS2_basal, PP7_basal, A, R, dR_1 .. dR_N]   (P = 7 + N doubles)
 */
#ifndef TCI_H_
#define TCI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCI_OK 0
#define TCI_EINVAL (-1)  /* bad argument (null pointer, size, construct table) */
#define TCI_EHIP (-2)    /* HIP runtime error */
#define TCI_ENOMEM (-3)  /* host or device allocation failed */
#define TCI_EDIM (-4)    /* grid length != data length: the reference errors at
                            ConstantElongationSim.m:47 ("Matrix dimensions must agree") */
#define TCI_ERANGE (-5)  /* cell id out of range, or ld_theta < 7 + N of that cell */

#define TCI_MAX_SEG 4    /* stem-loop segments per dye (GetFluorFromPolPos.m:47 loop) */
#define TCI_MAX_POINTS 2048 /* acquisition points per cell: <= 513 run the register-resident kernels,
                               longer cells the long-cell kernel (its tables in LDS, 64 B per point) */

typedef struct tci_ctx tci_ctx;

/* Ragged struct-of-arrays cell table: cell c owns t/ms2/pp7[offsets[c] .. offsets[c+1]).
 * Replaces the per-cell data struct {xdata = time, ydata = [MS2, PP7]} built at
 * TranscriptionCycleMCMC.m:163-181 (schema README.md:11-16). NaN = missing sample.
 * Borrowed for the duration of tci_create only (copied to the device). */
typedef struct {
  int64_t n_cells;
  const int64_t* offsets; /* [n_cells + 1] */
  const double* t;
  const double* ms2;
  const double* pp7;
} tci_cells;

/* Reporter construct (GetFluorFromPolPos.m:18-30): gene length L = L0 + tau*v (kb) and,
 * per segment s, the MS2 and PP7 stem-loop start/end (kb) and loop count (fluorval =
 * loopn/24). Requirements (checked): 1 <= n_seg <= TCI_MAX_SEG, 0 <= start < end. */
typedef struct {
  double L0;
  int32_t n_seg;
  const double* ms2_start;
  const double* ms2_end;
  const double* ms2_loopn;
  const double* pp7_start;
  const double* pp7_end;
  const double* pp7_loopn;
} tci_construct;

typedef struct {
  int32_t device;
  int32_t rows_per_lane;   /* kernel variant selected from the longest cell (0: the long-cell kernel) */
  int64_t n_cells;
  int64_t max_points;
  int64_t device_bytes;    /* resident cell-table bytes in HBM */
} tci_info;

/* Fill *out with the construct named by `name`; pointers refer to static storage.
 * Only "P2P-MS2v5-LacZ-PP7v4" is built in (GetFluorFromPolPos.m:18); any other name
 * returns TCI_EINVAL, as the reference errors on an undefined construct. */
int tci_construct_by_name(const char* name, tci_construct* out);

/* Create a context on HIP device `device`: validates the cells, builds each cell's
 * uniform grid t(1):mean(diff(t)):t(end) (SumofSquares...m:29-30, MATLAB colon rule),
 * interpolation indices/weights and time steps, and uploads everything to HBM. */
int tci_create(const tci_cells* cells, const tci_construct* construct, int device, tci_ctx** out);
int tci_destroy(tci_ctx* ctx);
const char* tci_last_error(const tci_ctx* ctx);
int tci_get_info(const tci_ctx* ctx, tci_info* out);

/* Test hook. flags bit 0: run the exact sequential loading-counter scan in every evaluation
 * (normally only when the parallel scan cannot prove floor() exact); bit 1: run the exact
 * per-(row, cohort) position sweep (normally only when the uniform-grid distance table cannot
 * prove every stem-loop/gene-end comparison). 0 restores the default. */
int tci_set_force_exact_scan(tci_ctx* ctx, int flags);

/* Batched likelihood, HOST pointers, synchronous: for b in [0,B)
 *   ss_out[b] = SumofSquaresFunction_TranscriptionCycleMCMC(construct, cell[cell_id[b]], theta[b,:])
 * theta is B rows of ld_theta doubles (ld_theta >= 7 + N of the row's cell).
 * active (may be NULL = all active): rows with active[b] == 0 are skipped (mcmcstat
 * rejects out-of-bounds proposals without calling ssfun) and get ss_out[b] = +Inf.
 * Non-finite theta entries give ss_out[b] = NaN (mcmcstat treats it as a rejection). */
int tci_ss_batch(tci_ctx* ctx, const double* theta, int64_t ld_theta, const int32_t* cell_id,
                 const uint8_t* active, int64_t B, double* ss_out);

/* Same on DEVICE pointers, asynchronous on `stream` (a hipStream_t; NULL = the HIP default
 * stream, as in every HIP API). Inputs stay resident in HBM; nothing is copied or
 * synchronised. Rows whose cell id is out of range or whose ld_theta is too short get NaN. */
int tci_ss_batch_async(tci_ctx* ctx, const double* d_theta, int64_t ld_theta, const int32_t* d_cell_id,
                       const uint8_t* d_active, int64_t B, double* d_ss_out, void* stream);

/* One evaluation: the literal ssfun(theta, data) call for one cell (host pointers).
 * P must be >= 7 + N of the cell. */
int tci_ssfun(tci_ctx* ctx, int32_t cell, const double* theta, int64_t P, double* ss_out);

#define TCI_GRID_INTERP 0 /* through the uniform grid + interp1, as inside the SS
                             (SumofSquares...m:28-56) */
#define TCI_GRID_RAW 1    /* on the raw acquisition times, as the plot/summary call
                             TranscriptionCycleMCMC.m:307-309 (no grid, no interp1) */

/* Batched forward model, HOST pointers, synchronous: simulated MS2 (already x A) and
 * PP7 at the acquisition times of each row's cell. Row b writes N(cell) values at
 * ms2_out[b*ld_out] and pp7_out[b*ld_out] (ld_out >= N of the cell); NaN where the
 * grid does not cover a time (interp1 out of range). The entries from N to ld_out of a
 * row are set to NaN. */
int tci_forward(tci_ctx* ctx, const double* theta, int64_t ld_theta, const int32_t* cell_id, int64_t B,
                int grid_mode, double* ms2_out, double* pp7_out, int64_t ld_out);

/* Number of HIP devices visible to this process (*n_out = 0 when there is none; never an error
 * for that). Lets a caller spread contexts over a node's GPUs, e.g. the reference's parfor worker k
 * (TranscriptionCycleMCMC.m:161) on device (k - 1) mod n (matlab/tci_ssfun.m). */
int tci_device_count(int* n_out);

/* Number of acquisition points of a cell, and the grid the SS uses for it (M points). */
int tci_cell_points(const tci_ctx* ctx, int32_t cell, int64_t* n_out);
int tci_cell_grid(const tci_ctx* ctx, int32_t cell, double* t_interp_out, int64_t cap, int64_t* m_out);

/* ---- GPU-resident batched DRAM: the caller of ssfun ----------------
 * mcmcrun(model, data, params, options) for many independent chains at once, one chain per
 * row (TranscriptionCycleMCMC.m:161-273): proposals, bounds rejection, delayed rejection,
 * adaptive covariance, Gaussian priors and the sigma^2 Gibbs update all run on the device; every
 * ssfun call is the batched likelihood kernel. mcmcstat is restated from its published algorithm
 * (version unpinned); MATLAB's RNG is not reproducible, so parity is statistical. */
typedef struct {
  int64_t n_steps;      /* nsimu: chain rows including the initial state (:264) */
  int64_t burnintime;   /* options.burnintime (:267): steps before covariance adaptation starts */
  int64_t adaptint;     /* options.adaptint (:268); 0 = no adaptation */
  int32_t ntry;         /* 2 = DRAM ('dram', :269), 1 = adaptive Metropolis only */
  int32_t updatesigma;  /* options.updatesigma (:265) */
  double drscale;       /* stage-2 proposal shrink (mcmcstat default 5) */
  double adascale;      /* adapted proposal scale; <= 0 = 2.4/sqrt(npar) */
  double qcovadj;       /* diagonal added before the Cholesky (1e-5) */
  double burnin_scale;  /* burn-in proposal scaling factor (10) */
  int64_t stats_from;   /* first chain row (1-based) of the posterior summaries (n_burn, :276) */
  int64_t thin;         /* keep every thin-th chain row in outputs.chain (0 = keep none) */
  uint64_t seed;
  int32_t engine;       /* TCI_DRAM_AUTO / _FUSED / _BATCHED / _WALK (below) */
  int32_t max_chunk;    /* FUSED/WALK: at most this many chain rows per draws pass + walk (0 = automatic:
                           adaptint, or the draws buffer's 2 GiB cap); same chains whatever it is */
  const int64_t* chain_keys; /* optional [n_chains]: chain c draws from RNG stream chain_keys[c]
                                (NULL: stream c). Keying chains by their global cell index makes a
                                shard of a run (its cells on one GPU) reproduce the unsharded chains.
                                A key is taken modulo 2^32: the generator's counter carries its low 32
                                bits only, and two chains whose keys agree there draw the same numbers */
  int64_t adapt_pmax;   /* 0, or the largest P = 7 + N over every chain of a larger fit that this run is one
                           shard of: the covariance adaptation kernel is picked by the largest P
                           (k_adapt_gt past 208), so a shard passing the whole fit's value adapts with the
                           same kernel, hence the same bits, as the unsharded fit (parallel.fit_sharded) */
  int64_t kernel_times; /* 1: time every kernel launch of the FUSED / WALK engines with HIP events on the
                           launch stream (tci_dram_outputs.kernel_ms); 0 (default): no events */
} tci_dram_options;

/* DRAM engines; all give identical chains for the same seed.
 *   FUSED:   per chunk of steps (up to the next adaptation) one wide launch draws every
 *            state-independent random quantity (proposal offsets z*R on MFMA, uniforms, Gamma
 *            variates), then one workgroup per chain walks the chunk with its ssfun evaluations in
 *            the loop (one workgroup barrier per step): latency-bound runs (few chains). The draws
 *            that do not need the adapted R (normals, uniforms, Gamma variates) are drawn one chunk
 *            ahead inside the previous chunk's walk launch (the first chunk's: one k_draws_rng launch).
 *   BATCHED: one launch per stage, every chain's ssfun in the batched likelihood kernel, replayed
 *            as a hipGraph per adaptation window: many chains, or cells too long for FUSED.
 *   WALK:    FUSED's draws pass, then ONE WAVEFRONT per chain walks the chunk (stage 2 evaluated
 *            only after a stage-1 rejection, no workgroup barriers): many chains (configs 4/5).
 *   AUTO:    FUSED whenever the cells are register-resident in the chain kernel and its draws pass
 *            fits a CU's LDS (cells of up to 513 points, P <= 520), as WALK beyond two chains per
 *            CU; BATCHED otherwise (longer cells, which FUSED and WALK refuse with TCI_ERANGE). */
#define TCI_DRAM_AUTO 0
#define TCI_DRAM_FUSED 1
#define TCI_DRAM_BATCHED 2
#define TCI_DRAM_WALK 3

/* Host buffers filled by tci_dram_run (any may be NULL). Per-chain vectors have stride ld.
 * Padding (entries j >= P = 7 + N of a chain whose row is shorter than ld): mean and std are NaN
 * (also every entry when no row is in the statistics range, stats_from > n_steps); final_theta keeps
 * theta0's padding unchanged; chain rows and qcov_R are 0 there. */
typedef struct {
  double* mean;         /* mean(chain(stats_from:end, :)) (:286-301) */
  double* std;          /* std(chain(stats_from:end, :), 1) */
  double* final_theta;  /* last chain row */
  double* sigma_mean;   /* sqrt(mean(s2chain)) over all rows (:302) */
  double* sigma_std;    /* std(sqrt(s2chain), 1) (:303) */
  double* accept_rate;  /* accepted moves / (n_steps - 1) */
  int64_t* n_evals;     /* ssfun calls: the initial one + every in-bounds proposal */
  double* chain;        /* [ceil(n_steps/thin)][n_chains][ld] thinned rows (rows 1, 1+thin, ...) */
  double* s2chain;      /* [ceil(n_steps/thin)][n_chains] */
  double* qcov_R;       /* [n_chains][ld][ld] final proposal factor R (upper): qcov = R'R (mcmcstat results.qcov) */
  double elapsed_ms;    /* device time of the step loop (HIP events) */
  double kernel_ms[4];  /* with opt.kernel_times (FUSED / WALK): device ms summed per kernel class -- [0] the
                           draws pass (k_draws), [1] the chain walk (k_chain / k_walk), [2] the covariance
                           adaptation (k_adapt_*), [3] FUSED's split draws: the normals and scalar draws
                           of the first chunk (k_draws_rng; later chunks' are drawn inside the k_chain launches, class 1) --
                           written by tci_dram_run, 0 otherwise */
  int64_t kernel_launches[4]; /* launches per class behind kernel_ms */
} tci_dram_outputs;

int tci_dram_defaults(tci_dram_options* opt);

/* Run n_chains chains; chain c evaluates cell cell_id[c] of the context. Inputs (host, n_chains x
 * ld row-major, ld >= 7 + N of every chain's cell): theta0 = x0 (:210), lower/upper = parameter
 * bounds (:242-255), prior_mu/prior_sig = Gaussian priors (sig = +Inf: none; dR: 0, 50, :254),
 * qcov_diag = the initial proposal covariance diagonal J0 (:230); sigma2_0 = model.sigma2 (:259,
 * per chain). The number of observations per chain is 2 N_c, NaNs included (:260). */
int tci_dram_run(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                 const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                 const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                 tci_dram_outputs* out);

/* ---- Posterior predictive envelopes (mcmcstat's mcmcpred / plims) ---------------------------
 * The forward model at S posterior samples per cell, reduced on the device to quantile bands of the
 * simulated signal at every acquisition time; only the bands come back to the host. */
typedef struct {
  int32_t grid_mode;      /* TCI_GRID_RAW (default) or TCI_GRID_INTERP */
  int64_t scratch_bytes;  /* cap on the device scratch for simulated rows; 0 = default (1 GiB) */
} tci_predict_options;
int tci_predict_defaults(tci_predict_options* opt);

/* For k in [0,n_sel): rows theta[(k*S + s)*ld_theta .. ], s in [0,S), are S posterior samples of cell
 * cell_id[k]. For each k, each dye and each acquisition time j < N(cell):
 *   x = sort(sim[k, 0..S-1, j])            (NaN last, as MATLAB's sort)
 *   h = (S-1)*probs[q]; lo = floor(h); f = h - lo
 *   out[(k*nq + q)*ld_out + j] = (lo + 1 < S) ? x[lo] + f*(x[lo+1] - x[lo]) : x[S-1]
 * i.e. mcmcstat's plims: interp1(sort(x), (n-1)*p+1). ms2 is already x A. Entries j >= N(cell) of an
 * output row are NaN. HOST pointers, synchronous. opt may be NULL (the defaults). 1 <= S <= 4096,
 * 1 <= nq <= 16, every prob finite and in [0, 1]; ld_theta >= 7 + N and ld_out >= N of every selected
 * cell (TCI_ERANGE). The simulated rows (2 * n_sel * S * ld_out doubles) live in a scratch buffer the
 * context owns; past opt->scratch_bytes whole cells are processed in chunks (same results), and
 * TCI_EINVAL is returned when one cell alone does not fit. */
int tci_predict(tci_ctx* ctx, const tci_predict_options* opt, const double* theta, int64_t ld_theta,
                const int32_t* cell_id, int64_t n_sel, int64_t S, const double* probs, int32_t nq,
                double* ms2_q, double* pp7_q, int64_t ld_out);

/* ---- Chain convergence diagnostics (mcmcstat's chainstats) -----------------------------------
 * Per column x[0..n) (one parameter of one chain over the n diagnostic rows; a chain's s2 is one more
 * column), all in FP64, reduced on the device so that only a few vectors per chain cross the bus:
 *   mcerr   b = max(10, floor(n/20)), nb = floor(n/b) batches from row 0 (the rows past nb*b left out),
 *           s = sqrt(b * sum_i (ybar_i - xbar)^2 / (nb - 1)) with xbar the mean of all n rows;
 *           mcerr = s / sqrt(n) (bmstd / sqrt(n)). NaN for n < 20.
 *   tau     Sokal's adaptive window (iact): y = x - xbar, c(k) = sum_t y[t] y[(t+k) mod n] (circular, what
 *           mcmcstat's FFT computes, here summed lag by lag with an early exit); c(0) == 0: tau = 0,
 *           window = 0; else S = -1/3 and for i = 1, 2, ..: S += c(i-1)/c(0) - 1/6, and at the first
 *           S < 0: tau = 2 (S + (i-1)/6), window = i. No crossing within max_lag lags: tau = +Inf,
 *           window = max_lag.
 *   geweke  segment A = the first floor(0.1 n) rows, B = the last floor(0.5 n);
 *           z = (mean_A - mean_B) / sqrt(s_A^2/n_A + s_B^2/n_B), s_A and s_B the batch-means s above of each
 *           segment (b from the segment's length), p = erfc(|z| / sqrt(2)). NaN when a segment has fewer
 *           than 20 rows (n < 200); a constant column gives 0/0 = NaN. mcmcstat estimates the same
 *           spectral density at zero with a Welch periodogram; batch means are used here because this
 *           variant is pinned by its formula alone.
 * A non-finite entry makes every statistic of its column NaN (its window -1). */
typedef struct {
  int64_t max_lag;  /* most lags iact may use; 0 = n (mcmcstat's rule). Bounds the O(n * window) work */
} tci_chainstats_options;

/* Host buffers (any may be NULL). Per-chain vectors have stride ld; padding (j >= npar of the chain) is
 * NaN, its window -1. */
typedef struct {
  double *mcerr, *tau, *geweke_z, *geweke_p;             /* [n_chains][ld] */
  int32_t* tau_window;
  double *s2_mcerr, *s2_tau, *s2_geweke_z, *s2_geweke_p; /* [n_chains]; NaN / -1 without an s2 chain */
  int32_t* s2_tau_window;
  int64_t n_rows;    /* written: rows the statistics used */
  double kernel_ms;  /* written: device time of the statistics kernels (HIP events) */
} tci_chainstats_outputs;

int tci_chainstats_defaults(tci_chainstats_options* opt);

/* The statistics of a chain already on the host (e.g. read back from a _RawChain file): chain is
 * [n_rows][n_chains][ld], s2chain [n_rows][n_chains] or NULL, npar [n_chains] (NULL: ld for every chain;
 * TCI_ERANGE outside [0, ld]). opt may be NULL (the defaults). TCI_EINVAL for n_rows < 1 or max_lag < 0,
 * TCI_ENOMEM when the chain does not fit the device. */
int tci_chainstats(tci_ctx* ctx, const tci_chainstats_options* opt, const double* chain, const double* s2chain,
                   int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chainstats_outputs* out);

/* tci_dram_run plus the statistics of the rows it kept, taken from the device chain before any copy:
 * the kept rows (1, 1 + thin, ..) whose 1-based chain row is >= stats_from, for theta and for s2. The
 * device chain exists for the statistics alone when out->chain is NULL (nothing of it is copied). sopt may
 * be NULL. TCI_EINVAL when opt->thin == 0, when no kept row is in the range, or for max_lag < 0. Every
 * engine gives the same chain bits, hence the same statistics bits. */
int tci_dram_run_stats(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                       const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                       const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                       tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout);

/* ---- Posterior mean, covariance and correlation of every chain (MATLAB's mean / cov / corrcoef) ----
 * Per chain c over its n = n_rows rows and its P = npar[c] columns (i, j < P), all in FP64, reduced on the device
 * so that the chain itself does not cross the bus:
 *   mean[i]     Neumaier-compensated sum of the column in row order, divided by n; a constant column's mean is
 *               its value.
 *   cov[i][j]   (sum_t (x_ti - mean_i) (x_tj - mean_j)) / (n - 1): cov(chain). Always two-pass and centred (a
 *               hierarchical fit holds v within 1e-5 of a value near 5, where a one-pass form cancels). The rows
 *               are summed in order, four per v_mfma_f64_16x16x4, by one wavefront per 16 x 16 tile; the tiles
 *               on and above the diagonal are computed, the lower triangle is their mirror (the same bits).
 *   corr[i][j]  cov_ij / (sqrt(cov_ii) * sqrt(cov_jj)), clamped to [-1, 1]; the diagonal is exactly 1.0 where
 *               cov_ii is finite and > 0. A constant column gives NaN in its whole row and column, diagonal
 *               included (0/0, as corrcoef gives).
 * A non-finite entry makes its column's mean, and its row and column of both matrices, NaN. Padding (i >= P or
 * j >= P) is NaN in all three outputs. An element's bits depend on its two columns, their indices and n alone:
 * not on n_chains, the chain's position, ld or scratch_bytes. */
typedef struct {
  int64_t scratch_bytes;  /* cap on the device buffer for the matrices (cov and corr, 2 x ld x ld doubles per
                             chain); 0 = 1 GiB. Past it the chains go through the buffer in groups */
} tci_chaincov_options;

/* Host buffers (any of the three may be NULL). */
typedef struct {
  double* mean;      /* [n_chains][ld] */
  double* cov;       /* [n_chains][ld][ld] */
  double* corr;      /* [n_chains][ld][ld] */
  int64_t n_rows;    /* written: rows the matrices used */
  double kernel_ms;  /* written: device time of the kernels (HIP events) */
} tci_chaincov_outputs;

int tci_chaincov_defaults(tci_chaincov_options* opt);

/* The matrices of a chain already on the host: chain is [n_rows][n_chains][ld], npar [n_chains] (NULL: ld for
 * every chain; TCI_ERANGE outside [0, ld]). opt may be NULL (the defaults). TCI_EINVAL for a null argument,
 * n_rows < 2, scratch_bytes < 0 or one chain's two ld x ld matrices above scratch_bytes; TCI_ENOMEM when the
 * chain does not fit the device. */
int tci_chaincov(tci_ctx* ctx, const tci_chaincov_options* opt, const double* chain, int64_t n_rows, int64_t n_chains,
                 int64_t ld, const int32_t* npar, tci_chaincov_outputs* out);

/* tci_dram_run_stats plus the matrices of the same rows (the kept rows whose 1-based chain row is >=
 * stats_from), taken from the device chain before any copy. sout may be NULL (no chain statistics); cout is
 * required; sopt and copt may be NULL. TCI_EINVAL when opt->thin == 0 or fewer than 2 kept rows are in the
 * range. */
int tci_dram_run_cov(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                     const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                     const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                     tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout,
                     const tci_chaincov_options* copt, tci_chaincov_outputs* cout);

/* ---- Posterior quantiles of every chain column (mcmcstat's plims: median and credible intervals) ----
 * Per column x[0..n) (one parameter of one chain over the n = n_rows rows; a chain's s2 is one more column), all
 * in FP64, selected on the device so that the chain itself does not cross the bus. For each p = probs[q]:
 *   key(x)  the 64-bit total order of tci_predict: the bits of x, all inverted for a negative x, the sign bit set
 *           otherwise; so -0 sorts before +0
 *   y = x sorted ascending by key
 *   h = (n-1)*p;  lo = floor(h);  f = h - lo
 *   out = (lo + 1 < n) ? y[lo] + f * (y[lo+1] - y[lo]) : y[n-1]
 * i.e. plims' interp1(sort(x), (n-1)*p+1), the formula of tci_predict: a multiply and an add as written, never
 * fused. Unlike tci_predict, which sorts NaN last, a non-finite entry (NaN or +-Inf) makes every quantile of its
 * column NaN, as tci_chainstats and tci_chaincov treat such a column. Padding (j >= npar[c]) is NaN.
 * The result is exact: y[lo] and y[lo+1] are the column's true order statistics (a radix selection on the keys;
 * no sketch, no sampling, no histogram approximation), so an output's bits depend on the column's values, n and p
 * alone: not on n_chains, the chain's position, ld or any tile size. */
typedef struct {
  int32_t nq;        /* 1 <= nq <= 16 */
  double probs[16];  /* each finite and in [0, 1]; defaults: nq = 3, {0.025, 0.5, 0.975} */
} tci_chainquant_options;

/* Host buffers (any may be NULL). */
typedef struct {
  double* q;         /* [n_chains][nq][ld] */
  double* s2_q;      /* [n_chains][nq]; NaN without an s2 chain */
  int64_t n_rows;    /* written: rows the quantiles used */
  double kernel_ms;  /* written: device time of the kernel (HIP events) */
} tci_chainquant_outputs;

int tci_chainquant_defaults(tci_chainquant_options* opt);

/* The quantiles of a chain already on the host: chain is [n_rows][n_chains][ld], s2chain [n_rows][n_chains] or
 * NULL, npar [n_chains] (NULL: ld for every chain; TCI_ERANGE outside [0, ld]). opt may be NULL (the defaults).
 * TCI_EINVAL for a null argument, n_rows < 1, nq outside [1, 16] or a prob that is not in [0, 1]; TCI_ENOMEM
 * when the chain does not fit the device. */
int tci_chainquant(tci_ctx* ctx, const tci_chainquant_options* opt, const double* chain, const double* s2chain,
                   int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chainquant_outputs* out);

/* ---- Marginal posterior density and histogram of every chain column (mcmcstat's density.m / mcmcplot's
 * 'denspanel' and 'hist') ----
 * Per column x[0..n) (one parameter of one chain over the n = n_rows >= 2 rows; a chain's s2 is one more column),
 * all in FP64, reduced on the device so that the chain itself does not cross the bus. With G = n_grid and
 * B = n_bins:
 *   xmin, xmax  the extremes in the key order of tci_chainquant (-0 sorts below +0); r = xmax - xmin.
 *               range = {xmin, xmax}.
 *   mean        the Neumaier-compensated sum of the column, divided by n; a constant column's mean is its value
 *               (xmin == xmax), as in tci_chaincov, so that its sd is exactly 0.
 *   sd          sqrt(sum_t (x_t - mean)^2 / (n - 1)), two-pass and centred.
 *   iqr         q(0.75) - q(0.25), q exactly tci_chainquant's quantile (plims) of the column.
 *   bw          ((bw_scale * 1.06) * s) * n^(-1/5), s = (iqr > 0 ? min(sd, iqr / 1.34) : sd); n^(-1/5) is
 *               pow((double)n, -0.2), computed once on the host.
 *   grid        lo = xmin - 0.08 * r;  hi = xmax + 0.08 * r;  step = (hi - lo) / (G - 1);  g_k = lo + k * step,
 *               k = 0 .. G - 1: every product, sum and quotient rounded once, as written, never fused. The grid's
 *               bits follow from xmin, xmax and G alone; it is not an output, a caller restates it from range.
 *   dens[k]     (1 / (n * bw)) * sum_t phi((g_k - x_t) / bw), phi(u) = exp(-u^2 / 2) / sqrt(2 pi): a Gaussian
 *               kernel estimate with the device library's exp (no fast-math variant).
 *   counts[b]   the rows of bin b of B equal-width bins over [xmin, xmax]: row t goes to bin
 *               min(B - 1, (int)floor((x_t - xmin) / r * B)) -- a subtraction, a division and a multiplication,
 *               in that order -- so a value equal to xmax lands in the last bin; r == 0: all n rows in bin 0.
 * range and counts are exact. bw is within (n + 16) * 2^-53 (relative) and dens within (4 n + 96) * 2^-53 *
 * peak, peak = 1 / (bw * sqrt(2 pi)), of the formulas evaluated without rounding (DESIGN.md has the derivation).
 * A constant column (sd == 0) has bw = 0 and every dens[k] NaN (0/0, as density.m gives); its range is the value
 * twice and its counts are as above. A non-finite entry (NaN or +-Inf) makes range, bw and dens of its column NaN
 * and its counts -1, as tci_chainquant and tci_chaincov treat such a column. Padding (j >= npar[c]) is NaN / -1.
 * An output's bits depend on the column's values, n and the options alone: not on n_chains, the chain's position,
 * ld or how many workgroups ran (the rows are reduced in segments whose boundaries follow from n alone).
 *
 * Two deliberate deviations from mcmcstat, whose version is not pinned (this definition is pinned by its formulas
 * alone, as tci_chainstats is):
 *   1. iqr uses the project's one quantile definition (plims, interpolating at (n - 1) p + 1); mcmcstat's iqrange
 *      interpolates at (n + 1) p.
 *   2. the grid is always density.m's rule for n > 200 (the data's range widened by 8 % each side); its n <= 200
 *      branch (mean +- 4 sd) is not restated: one rule keeps the grid bit-exact, and posterior chains are never
 *      that short. */
typedef struct {
  int32_t n_grid;   /* G, 2 .. 256; default 100 (linspace's default in density.m) */
  int32_t n_bins;   /* B, 1 .. 256; default 20 */
  double bw_scale;  /* finite and > 0; default 1.0 */
} tci_chaindens_options;

/* Host buffers (any pointer may be NULL). */
typedef struct {
  double* range;       /* [n_chains][2][ld]: xmin, xmax */
  double* bw;          /* [n_chains][ld] */
  double* dens;        /* [n_chains][n_grid][ld] */
  int32_t* counts;     /* [n_chains][n_bins][ld] */
  double* s2_range;    /* [n_chains][2]; the s2 twins are NaN / -1 without an s2 chain */
  double* s2_bw;       /* [n_chains] */
  double* s2_dens;     /* [n_chains][n_grid] */
  int32_t* s2_counts;  /* [n_chains][n_bins] */
  int64_t n_rows;      /* written: rows the estimate used */
  double kernel_ms;    /* written: device time of the kernels (HIP events) */
} tci_chaindens_outputs;

int tci_chaindens_defaults(tci_chaindens_options* opt);

/* The densities and histograms of a chain already on the host: chain is [n_rows][n_chains][ld], s2chain
 * [n_rows][n_chains] or NULL, npar [n_chains] (NULL: ld for every chain; TCI_ERANGE outside [0, ld]). opt may be
 * NULL (the defaults). TCI_EINVAL for a null argument, n_rows < 2 or an option out of range; TCI_ERANGE for
 * n_rows above 2^30 or a launch grid above 2^31 workgroups; TCI_ENOMEM when the chain or the per-segment partial
 * sums do not fit the device. */
int tci_chaindens(tci_ctx* ctx, const tci_chaindens_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, tci_chaindens_outputs* out);

/* The optional reductions of a run's device chain. Each *out that is NULL: that reduction is not run; each *opt
 * may be NULL (its defaults). A zero-initialised struct asks for none. */
typedef struct {
  const tci_chainstats_options* sopt;
  tci_chainstats_outputs* sout;
  const tci_chaincov_options* copt;
  tci_chaincov_outputs* cout;
  const tci_chainquant_options* qopt;
  tci_chainquant_outputs* qout;
  const tci_chaindens_options* dopt;
  tci_chaindens_outputs* dout;
} tci_dram_reductions;

/* tci_dram_run plus any of the four reductions, all over the same rows (the kept rows whose 1-based chain row is
 * >= stats_from), taken from the device chain before any copy; the device chain exists for them alone when
 * out->chain is NULL. tci_dram_run_stats and tci_dram_run_cov are this call with the fields they name.
 * TCI_EINVAL for a null red, and, when a reduction is asked for, when opt->thin == 0 or no kept row (covariance
 * and density: fewer than 2) is in the range. */
int tci_dram_run_reduced(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                         const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                         const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                         tci_dram_outputs* out, const tci_dram_reductions* red);

/* ---- Replicate chains compared: Gelman-Rubin's potential scale reduction factor (mcmcstat's psrf) ----
 * The one reduction ACROSS chains. A group is the set of chains c with the same group[c], taken in ascending chain
 * index; group[c] == -1: the chain belongs to no group. Per group and per column (the group's P = npar parameters;
 * the chains' s2 is one more column), over the n = n_rows rows, all in FP64, reduced on the device so that the
 * chains do not cross the bus. mcmcstat is not vendored: the formulas below (Gelman et al., Bayesian Data Analysis,
 * 3rd ed., section 11.4) are the definition.
 *   sequences   per chain of the group three: the whole chain, rows [0, n); half A, rows [0, h), h = floor(n / 2);
 *               half B, rows [n - h, n). For an odd n the middle row belongs to no half.
 *   mu, s2      per sequence of length L: mu = the Neumaier-compensated sum of its rows divided by L; a constant
 *               sequence's mean is its value (as in tci_chaincov, so that its s2 is exactly 0);
 *               s2 = sum_t (x_t - mu)^2 / (L - 1), two-pass and centred.
 *   classic     the m = M whole chains of the group, L = n.
 *   split       the m = 2 M halves, L = h, ordered A, B of the group's first chain, A, B of the next, and so on.
 *   W = (sum_j s2_j) / m;  mubar = (sum_j mu_j) / m;  T = sum_j (mu_j - mubar)^2 / (m - 1);
 *   rhat = sqrt((L - 1) / L + T / W)
 *   pooled_mean = mubar of the whole chains
 *   pooled_std  = sqrt(((n - 1) * sum_j s2_j + n * sum_j (mu_j - mubar)^2) / (M * n)) over the whole chains: the
 *               std(., 1) of all M n rows, the divisor the reference uses for its sigma_*.
 * Every sum over j runs in sequence order; every operation is rounded once, as written, never fused. One rule is
 * added to the formulas: when all mu_j are equal, mubar is that value (what the constant-sequence rule is to mu),
 * so that T is exactly 0. Consequences:
 *   m == 1 (classic with one chain): NaN.  L < 2 (split for n < 4): NaN.
 *   W == 0 and T == 0: NaN (0/0).  W == 0 and T > 0: +Inf.
 *   identical chains: classic rhat is exactly sqrt((n - 1) / n).
 * A non-finite entry (NaN or +-Inf) anywhere in a group's column makes all four outputs of that column NaN. Padding
 * (j >= npar) is NaN, and so is every output of a group id no chain carries. All chains of a group must have the
 * same npar (TCI_EINVAL, the group named in the message).
 * An output's bits depend on the group's columns in chain order and on n alone: not on n_chains, where the chains
 * sit, how groups interleave, ld or how many workgroups ran (the rows are reduced in 256-row segments whose
 * boundaries follow from n alone, inside a segment in a fixed order, and the segments are combined in order).
 * With u = 2^-53 and X = max|x| over the group's column, rhat is within
 *   (L + 2 m + 16) u rhat  +  8 u X sqrt(T) / (W rhat)  +  (m^2 + 32) (u X)^2 (rhat + 1 / rhat) / W
 * of the formulas evaluated without rounding: a relative term, the cancellation in mu_j - mubar (it grows when the
 * chains sit far from 0 relative to their spread, as a hierarchical fit's v does) and its second-order companion.
 * pooled_mean is within (m + 4) u X and pooled_std within (n + m + 10) u pooled_std + 8 u X (DESIGN.md section 7f has
 * the derivation).
 *
 * Deviations from mcmcstat's psrf.m, whose version is not pinned: psrf.m follows Brooks and Gelman (1998), whose
 * estimate carries a sampling-variability correction in m on the between-chain term; the BDA3 form above has none,
 * and the two agree as m grows. psrf.m has no split variant and no rule for non-finite or constant columns. */
typedef struct {
  int64_t flags;  /* reserved, must be 0 */
} tci_chainrhat_options;

/* Host buffers (any pointer may be NULL). Per-group vectors have stride ld. */
typedef struct {
  double *rhat, *rhat_split, *pooled_mean, *pooled_std;             /* [n_groups][ld] */
  double *s2_rhat, *s2_rhat_split, *s2_pooled_mean, *s2_pooled_std; /* [n_groups]; NaN without an s2 chain */
  int64_t n_rows;    /* written: rows the reduction used */
  double kernel_ms;  /* written: device time of the kernels (HIP events) */
} tci_chainrhat_outputs;

int tci_chainrhat_defaults(tci_chainrhat_options* opt);

/* The reduction of a chain already on the host: chain is [n_rows][n_chains][ld], s2chain [n_rows][n_chains] or
 * NULL, npar [n_chains] (NULL: ld for every chain; TCI_ERANGE outside [0, ld]), group [n_chains] with values in
 * [-1, n_groups) (NULL: every chain in group 0; TCI_ERANGE outside). opt may be NULL (the defaults). TCI_EINVAL for
 * a null argument, n_rows < 1, n_groups outside [1, n_chains], flags != 0 or a group of mixed npar; TCI_ENOMEM when the chain does not
 * fit the device. */
int tci_chainrhat(tci_ctx* ctx, const tci_chainrhat_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                  int64_t n_groups, tci_chainrhat_outputs* out);

/* tci_dram_run_reduced plus the group reduction over the same rows (the kept rows whose 1-based chain row is >=
 * stats_from), taken from the device chain before any copy. red may be NULL (no per-chain reduction); rout is
 * required; ropt may be NULL; group and n_groups as in tci_chainrhat (npar is the cells': 7 + N). TCI_EINVAL when
 * opt->thin == 0, fewer than 2 kept rows are in the range or n_groups is outside [1, n_chains]. For replicate chains
 * of one cell to be independent their chain_keys must differ modulo 2^32 (tci_dram_options). Every engine gives the same chain bits, hence the same
 * bits here. */
int tci_dram_run_rhat(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                      const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                      const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                      tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                      const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout);

/* ---- Replicate chains pooled: the multi-chain effective sample size (the n_eff of BDA3 section 11.5) ----
 * What the pooled posterior of a group of chains is worth in independent draws, with the between-chain variance
 * charged to the autocorrelation (Gelman et al., BDA3 section 11.5; Geyer 1992), and the pooled mean's Monte-Carlo
 * standard error. mcmcstat has no such function: the formulas below are the definition. The group, the column, the s2
 * column and the sequences are tci_chainrhat's: a group's chains in ascending chain index; the whole chain, rows
 * [0, n); half A, rows [0, h), and half B, rows [n - h, n), h = floor(n / 2); `classic` uses the m = M whole chains,
 * L = n; `split` the m = 2 M halves, L = h, ordered A, B per chain. All in FP64, every operation rounded once as
 * written, never fused, except the lag sums (below).
 *   mu_j, s2_j, W, mubar (with the equal-means rule) and T are exactly tci_chainrhat's (the same bits), but m == 1
 *   is allowed here (the single-chain estimate) with T = 0.
 *   vplus = ((L - 1) / L) * W + T
 *   y_j[t] = x_j[t] - mu_j
 *   c_j(k) = sum_{t = 0}^{L - 1 - k} y_j[t] * y_j[t + k]: linear, not circular as tci_chainstats' c(k) is. Summed
 *            in increasing t from 0.0, each product fused into the sum: acc = fma(y_j[t], y_j[t + k], acc). The order
 *            follows from L and k alone.
 *   a(k)   = (sum_j (c_j(k) / L)) / m: every c_j(k) divided by L, the quotients added in sequence order from 0.0, the
 *            sum divided by m.
 *   rho(0) = 1;  rho(k) = 1 - (W - a(k)) / vplus for k >= 1
 *   K      = L - 1 if max_lag == 0, else min(max_lag, L - 1)
 *   P_i    = rho(2 i) + rho(2 i + 1) for i = 0, 1, .. while 2 i + 1 <= K
 *   s      the least i >= 1 for which P_i > 0 is false (a NaN stops); if the pairs run out first, their count
 *   Q_0 = P_0;  Q_i = (P_i < Q_{i-1} ? P_i : Q_{i-1}): Geyer's initial monotone sequence (a NaN Q_0 stays)
 *   tau    = -1 + 2 * sum_{i < s} Q_i, summed in order from Q_0
 *   cap    = (m L) * log10(m L), log10 computed once per group on the host
 *   ess    = tau > 0 ? min((m L) / tau, cap) : cap; NaN when tau is NaN
 *   window = 2 s, the lags summed
 *   mcse   = pooled_std / sqrt(ess), pooled_std tci_chainrhat's; classic only
 * Consequences:
 *   L < 2: tau, ess and mcse are NaN and window is 0. So split is NaN for n < 4; n = 2 and n = 3 have P_0 only.
 *   No pair stopped and K < L - 1 (max_lag ended it): tau = +Inf, ess = 0, window = 2 s: tci_chainstats' convention.
 *     Running out of lags at K = L - 1 is a finite result.
 *   vplus == 0 (W = T = 0, a constant column): tau, ess and mcse are NaN (0/0); window = 2 s as the NaN stops it.
 *   W == 0 < T (each chain constant, at different values): every a(k) is 0 and every rho is 1 by the formula; nothing
 *     is special-cased: no pair stops.
 *   A non-finite entry (NaN or +-Inf) anywhere in a group's column: every output of that column is NaN and its
 *     windows are -1, as in tci_chainrhat; such a column is flagged before the lag loop and never enters it.
 *   Padding (j >= npar) and every output of a group id no chain carries: NaN / -1. All chains of a group must have
 *     the same npar (TCI_EINVAL, the group named in the message).
 *   Every device loop over lags is bounded by K; none ends on a floating comparison alone. The stop is a
 *     discontinuous decision: the device takes it on its own FP64 values, with no tolerance.
 * Bits. An output's bits depend on the group's columns in chain order, on n and on max_lag alone: not on n_chains,
 * where the chains sit, how groups interleave, ld or how many workgroups ran (the moments are tci_chainrhat's; one
 * lane sums a lag in the order above whatever the tiles are).
 * Error bound. With u = 2^-53, X = max|x| over the group's column, lambda = L / (L - 1), and for the same stop s:
 *   E_a  = 8 u X sqrt(W) + (L + m + 6) u W + 36 (u X)^2                       |a(k) - exact|
 *   E_Wa = E_a + (L + m + 5) u W + 32 (u X)^2                                 |(W - a(k)) - exact|
 *   E_v  = (L + 2 m + 10) u vplus + 12 u X sqrt(T) + (2 m^2 + 96) (u X)^2     |vplus - exact|
 *   E_rho = (E_Wa + 2 lambda E_v) / vplus + (4 lambda + 1) u
 *   E_P  = 2 E_rho + (2 + 4 lambda) u
 *   |tau - exact| <= E_tau = 2 s E_P + (s + 2) u (|tau| + 1)
 *   |ess - exact| <= 4 u cap + 1.01 ess E_tau / |tau|   (the second term where (m L) / tau <= 2 cap)
 *   |mcse - exact| <= mcse (E_std / pooled_std + 0.505 E_ess / ess + 3 u), E_std tci_chainrhat's bound
 * of the formulas evaluated without rounding: the roundings of the L - k products and their sum, the cancellation in
 * y = x - mu_j (the 8 u X sqrt(W) term), in W - a(k) and in mu_j - mubar (12 u X sqrt(T)), and the sum of s pairs
 * (DESIGN.md section 7g and tests/chainess_oracle.py have the derivation). */
typedef struct {
  int64_t max_lag;  /* cap on the lags; 0 = none (L - 1) */
  int64_t flags;    /* reserved, must be 0 */
} tci_chainess_options;

/* Host buffers (any pointer may be NULL). Per-group vectors have stride ld. */
typedef struct {
  double *ess, *ess_split, *tau, *tau_split, *mcse;                /* [n_groups][ld] */
  int32_t *window, *window_split;                                  /* [n_groups][ld] */
  double *s2_ess, *s2_ess_split, *s2_tau, *s2_tau_split, *s2_mcse; /* [n_groups]; NaN without an s2 chain */
  int32_t *s2_window, *s2_window_split;                            /* [n_groups]; -1 without an s2 chain */
  int64_t n_rows;    /* written: rows the reduction used */
  double kernel_ms;  /* written: device time of the kernels (HIP events), the moments' kernels included */
} tci_chainess_outputs;

int tci_chainess_defaults(tci_chainess_options* opt);

/* The reduction of a chain already on the host; arguments, rules and error codes as for tci_chainrhat, plus
 * TCI_EINVAL for max_lag < 0. */
int tci_chainess(tci_ctx* ctx, const tci_chainess_options* opt, const double* chain, const double* s2chain,
                 int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                 int64_t n_groups, tci_chainess_outputs* out);

/* tci_dram_run_rhat plus the effective sample size of the same groups over the same rows, both taken from the device
 * chain before any copy. rout may be NULL here (no R-hat outputs); eout is required; ropt and eopt may be NULL. */
int tci_dram_run_ess(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                     const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                     const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                     tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                     const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                     tci_chainess_outputs* eout);

/* ---- Replicate chains ranked: rank-normalised split R-hat, bulk and tail ESS, pooled quantiles ----
 * The diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization, folding, and localization:
 * an improved R-hat for assessing convergence of MCMC", Bayesian Analysis 16 (2021), and the pooled quantiles of a
 * group, all resting on one pooled sort of the group's column on the device. The group, the column, the s2 column,
 * padding, group ids no chain carries and the mixed-npar error are tci_chainrhat's. A non-finite entry (NaN or +-Inf)
 * anywhere in a group's column makes every output of that column NaN and every window -1. For a finite column of one
 * group, N = M n: the group's M chains in ascending chain index, rows [0, n) of each. All in FP64, every operation
 * rounded once as written, never fused.
 *   1. pooled order   key(x) is tci_chainquant's 64-bit total order (-0 sorts below +0; they do not tie); y is the N
 *                     values sorted ascending by key.
 *   2. q              for each p = probs[k]: tci_chainquant's plims rule on y with n := N: h = (N - 1) * p,
 *                     lo = floor(h), f = h - lo, q = y[lo] + f * (y[lo + 1] - y[lo]), and y[N - 1] where lo + 1 == N.
 *                     Exact: bit for bit the sorted-column definition.
 *   3. rank scores    for an element with key k: lt = the number of keys below k, eq = the number equal to k,
 *                     R2 = 2 lt + eq + 1 (twice the average rank, an integer),
 *                     p = ((double)R2 - 0.75) / ((double)(2 N) + 0.5): Blom's (r - 3/8) / (N + 1/4) with one division,
 *                     z = PPND16(p), Wichura's algorithm AS241 written as CPython's statistics.NormalDist().inv_cdf
 *                     writes it (the same expression and coefficients, every Horner step a multiplication, then an
 *                     addition). Where |p - 0.5| <= 0.425 the expression has no transcendental: z is the library's bit
 *                     for bit. Elsewhere r = sqrt(-log(min(p, 1 - p))) goes through the device's log, and z lies
 *                     within 72 ulp of the expression evaluated with any log that is good to 1 ulp (DESIGN.md
 *                     section 7n and tests/chainrank_oracle.py have the derivation; the largest difference seen is
 *                     recorded there).
 *   4. bulk           rhat_bulk = tci_chainrhat's SPLIT rhat of the z chain; ess_bulk, tau_bulk, window_bulk =
 *                     tci_chainess's SPLIT outputs on the z chain with max_lag.
 *   5. folded         med = the pooled quantile at p = 0.5 (rule 2); zeta = fabs(x - med), one subtraction; z_folded =
 *                     the rank scores (rule 3) of zeta; rhat_folded = its split rhat;
 *                     rhat_rank = max(rhat_bulk, rhat_folded), NaN if either is NaN.
 *   6. tail           q_tail = the pooled quantiles at tail_lo and tail_hi; the indicator chains
 *                     I_lo = (x <= q_tail[0]) ? 1.0 : 0.0 and I_hi = (x <= q_tail[1]) ? 1.0 : 0.0; ess_tail_lo and
 *                     ess_tail_hi = their split ESS with max_lag (window_tail_lo, window_tail_hi the lags summed);
 *                     ess_tail = min of the two, NaN if either is NaN. A constant indicator column gives NaN by
 *                     tci_chainess's vplus == 0 rule; nothing is special-cased.
 *   7. z, z_folded    optional: the rank-score chains themselves, laid out as the chain (what rank plots draw). Padding
 *                     columns, chains of no group and columns with a non-finite entry are NaN there.
 * Consequences: n < 4 has no split sequence of two rows: every rhat and ess output is NaN and the windows are 0, as
 * tci_chainrhat / tci_chainess give; q, q_tail, z and z_folded are defined for every n >= 1. M = 1 is allowed: the
 * two halves of the one chain are compared. A constant column has every R2 = N + 1, p = 0.5 exactly and z = 0: rhat
 * NaN (0/0), ess NaN.
 * Deviations from Vehtari et al.: (a) they split each chain before ranking, which changes nothing for an even n (the
 * pooled set is the same); for an odd n the middle row is ranked here and belongs to no half, as in tci_chainrhat.
 * (b) Their ESS truncates Geyer's sequence as Stan does (initial positive, then monotone, with a tail correction
 * term); bulk and tail ESS here are tci_chainess's estimator on the transformed chains. (c) Their tail-ESS indicator
 * quantiles are taken per call of the quantile function of the pooled draws with R's type 7 rule, which is plims.
 * Bits. An output's bits depend on the group's columns in chain order, on n and on the options alone: not on n_chains,
 * where the chains sit, how groups interleave, ld, or which sort path ran (up to tci_chainrank_lds_cap() values of a
 * group are sorted in LDS, more in global memory; the sorted keys are one sequence either way).
 * Device memory beyond the chain: one transformed chain (the size of chain and s2chain), reused by the four passes
 * (z, z_folded, I_lo, I_hi); for groups above the cap, 8 N_max bytes per (group, column); and tci_chainess's scratch. */
typedef struct {
  int32_t nq;         /* 1 .. 16; default 3 */
  double probs[16];   /* each in [0, 1]; default 0.025, 0.5, 0.975 */
  double tail_lo;     /* 0 < tail_lo < tail_hi < 1; defaults 0.05, 0.95 */
  double tail_hi;
  int64_t max_lag;    /* as tci_chainess_options; default 0 */
  int64_t flags;      /* reserved, must be 0 */
} tci_chainrank_options;

/* Host buffers (any pointer may be NULL). Per-group vectors have stride ld. */
typedef struct {
  double* q;                                                /* [n_groups][nq][ld] */
  double* q_tail;                                           /* [n_groups][2][ld] */
  double *rhat_bulk, *rhat_folded, *rhat_rank;              /* [n_groups][ld] */
  double *ess_bulk, *tau_bulk;                              /* [n_groups][ld] */
  double *ess_tail_lo, *ess_tail_hi, *ess_tail;             /* [n_groups][ld] */
  int32_t *window_bulk, *window_tail_lo, *window_tail_hi;   /* [n_groups][ld] */
  double* s2_q;                                             /* [n_groups][nq]; the s2 twins are NaN / -1 without s2 */
  double* s2_q_tail;                                        /* [n_groups][2] */
  double *s2_rhat_bulk, *s2_rhat_folded, *s2_rhat_rank;     /* [n_groups] */
  double *s2_ess_bulk, *s2_tau_bulk;
  double *s2_ess_tail_lo, *s2_ess_tail_hi, *s2_ess_tail;
  int32_t *s2_window_bulk, *s2_window_tail_lo, *s2_window_tail_hi;
  double *z, *z_folded;                                     /* [n_rows][n_chains][ld] */
  double *s2_z, *s2_z_folded;                               /* [n_rows][n_chains] */
  int64_t n_rows;    /* written: rows the reduction used */
  double kernel_ms;  /* written: device time of the whole reduction (HIP events); with z / z_folded given, their
                        device-to-host copies between the passes lie inside it */
  double rank_ms;    /* written: device time of the sort, rank and indicator kernels alone */
} tci_chainrank_outputs;

int tci_chainrank_defaults(tci_chainrank_options* opt);

/* The most values of one group (M * n_rows) the pooled sort holds in LDS; larger groups are sorted in global memory. */
int64_t tci_chainrank_lds_cap(void);

/* The reduction of a chain already on the host; arguments, rules, error codes and their order as for tci_chainrhat,
 * plus TCI_EINVAL for nq outside [1, 16], a prob that is not in [0, 1], tail_lo / tail_hi that do not satisfy
 * 0 < tail_lo < tail_hi < 1, max_lag < 0 and flags != 0 (checked after n_rows and before n_chains, as tci_chainess
 * checks its options), and TCI_ERANGE for a group of 2^31 values or more. TCI_ENOMEM, with the byte count in the
 * message, when the transformed chain and the sort's keys do not fit the device. */
int tci_chainrank(tci_ctx* ctx, const tci_chainrank_options* opt, const double* chain, const double* s2chain,
                  int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, const int32_t* group,
                  int64_t n_groups, tci_chainrank_outputs* out);

/* tci_dram_run_ess plus the rank diagnostics of the same groups over the same rows, all taken from the device chain
 * before any copy. rout and eout may be NULL here; kout is required; ropt, eopt and kopt may be NULL. */
int tci_dram_run_rank(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                      const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                      const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                      tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                      const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                      tci_chainess_outputs* eout, const tci_chainrank_options* kopt, tci_chainrank_outputs* kout);

/* ---- Posterior predictive fit checks per cell (WAIC, PIT, coverage, reduced chi^2, Durbin-Watson) ----
 * Does the fitted model describe a cell's data? Every observed MS2 and PP7 value is scored under the Gaussian-mixture
 * posterior predictive distribution that S posterior samples (theta_s, sigma2_s) define: (1 / S) sum_s
 * N(f_s, sigma2_s), f_s the simulated signal. Nothing is drawn: the mixture's density and CDF are evaluated in closed
 * form, so everything is deterministic. The simulated rows stay in the device scratch, as in tci_predict; only the
 * pointwise vectors come back. mcmcstat has no such function: the formulas below are the definition (WAIC: Gelman et
 * al., BDA3 section 7.2, the variance form of the penalty).
 * Inputs. For k in [0, n_sel): theta[(k*S + s)*ld_theta ..] holds the S posterior samples of cell cell_id[k], as for
 *   tci_predict; s2[k*S + s] is the sigma2 of the same chain row.
 * Forward model. Always TCI_GRID_INTERP: the signal the SS compares with the data (SumofSquares...m:49-61), MS2
 *   already x A. There is no grid option.
 * Data. The y1 / y2 (MS2 / PP7) of the cell as given to tci_create.
 * Host, once per sample row, with the C library's sqrt and log:
 *   sd_s = sqrt(s2_s);  lg_s = log(6.283185307179586 * s2_s);  logS = log((double)S), computed once.
 * Scored points. A point (dye d, index j < N) is scored when its datum y is finite and every f_s, s in [0, S), is
 *   finite. For a scored point, every operation rounded once, as written, never fused; exp, log and erfc are the
 *   device library's (no fast-math variants):
 *     r_s  = y - f_s;   z_s = r_s / sd_s;   ll_s = -0.5 * (lg_s + z_s * z_s)
 *     m    = max_s ll_s
 *     lppd = (m + log(SUM_s exp(ll_s - m))) - logS
 *     lbar = (SUM_s ll_s) / S
 *     p_waic = (SUM_s (ll_s - lbar)^2) / (S - 1)          NaN for S == 1 (0 / 0)
 *     pit  = (SUM_s 0.5 * erfc(-z_s * 0.7071067811865476)) / S
 *     resid = (SUM_s r_s) / S;   zbar = (SUM_s z_s) / S;   z2 = (SUM_s z_s * z_s) / S
 *   Order of every SUM_s: the samples are taken in segments of 64 consecutive s (the boundaries follow from S alone);
 *   inside a segment the terms are added in ascending s from 0.0; the segment partials are then added in ascending
 *   order from 0.0. Nothing is special-cased: an overflowing z * z makes ll = -Inf and the formulas carry it.
 * Unscored points and padding (j from N to ld_out): all six pointwise outputs are NaN.
 * Per cell, computed on the host from the pointwise vectors; the points are visited in the order dye 0 ascending j,
 *   then dye 1 ascending j, over scored points, sums from 0.0:
 *     n_obs       the number of scored points
 *     lppd        sum_i lppd_i;   p_waic = sum_i p_waic_i;   elpd_waic = lppd - p_waic (WAIC is -2 x this)
 *     chi2        (sum_i z2_i) / n_obs: the reduced chi^2 (near 1 by construction when sigma2 is sampled)
 *     coverage[l] #{i : lo_l <= pit_i <= hi_l} / n_obs, lo_l = (1 - level_l) / 2, hi_l = 1 - lo_l: the share of the
 *                 data inside the central predictive interval of that level
 *     dw[d]       per dye, (sum (zbar_j - zbar_{j-1})^2 over the pairs with j - 1 and j both scored) / (sum zbar_j^2
 *                 over scored j): the Durbin-Watson statistic of the standardised residuals (2: uncorrelated; towards
 *                 0: a systematic misfit)
 *   n_obs == 0: every per-cell value is NaN and n_obs is 0.
 * Bits. A cell's outputs depend on its samples in order, its data, S and the levels alone: not on n_sel, the cell's
 * position, ld_theta, ld_out, scratch_bytes, the tile shape or how many workgroups ran.
 * Error bound. resid, zbar and z2 use +, -, x and / in the stated order: a float64 restatement in that order gives
 * the same bits. For the rest, against the formulas evaluated without rounding on the same f_s, sd_s and lg_s, with
 * u = 2^-53, Z2 = max_s z_s^2, L = max_s |lg_s|, g = min(S, 64) + ceil(S / 64) (the terms one sum's value passes
 * through), and the device functions within K_exp = 3, K_log = 3 and K_erfc = 16 ulp (1 ulp = 2 u):
 *   E = u (4 Z2 + L)                                                            |ll_s - exact|
 *   |lppd - exact|   <= 1.01 u (4 Z2 + L + 2 K_exp + g + (2 K_log + 4) log S + 2 |lppd|)
 *   A = (L + Z2) / 2;   D = 2 E + (g + 3) u A                                   |(ll_s - lbar) - exact|
 *   |p_waic - exact| <= 1.01 (2 D sqrt(S p_waic / (S - 1)) + S D^2 / (S - 1) + (g + 4) u p_waic)
 *   |pit - exact|    <= 1.01 u (2 K_erfc + g + 4)
 * The ROCm device-library documentation states no accuracy for these functions; K_exp, K_log and K_erfc are the
 * limits of OpenCL's double-precision profile, which that library implements, and the largest deviation measured on
 * the test inputs stays inside the bounds they give (DESIGN.md section 7h has the derivation and the measurement;
 * tests/fitcheck_oracle.py restates the bound). */
typedef struct {
  int64_t scratch_bytes;  /* cap on the device scratch for simulated rows; 0 = default (1 GiB) */
  int32_t n_levels;       /* 1 .. 8; default 2 */
  double levels[8];       /* each strictly inside (0, 1); defaults {0.5, 0.95} */
} tci_fitcheck_options;

/* Host buffers (any pointer may be NULL). */
typedef struct {
  double *lppd_i, *p_waic_i, *pit, *resid, *zbar, *z2;  /* pointwise, each [n_sel][2][ld_out]: dye 0 = MS2, 1 = PP7 */
  int32_t* n_obs;                                       /* [n_sel] */
  double *lppd, *p_waic, *elpd_waic, *chi2;             /* [n_sel] */
  double* coverage;                                     /* [n_sel][n_levels] */
  double* dw;                                           /* [n_sel][2] */
  double kernel_ms;   /* written: device time of the fit-check kernel (HIP events), summed over the chunks */
  double forward_ms;  /* written: device time of the forward launches that fill the scratch */
} tci_fitcheck_outputs;

int tci_fitcheck_defaults(tci_fitcheck_options* opt);

/* HOST pointers, synchronous. opt may be NULL (the defaults); out is required. 1 <= S <= 4096; ld_theta >= 7 + N and
 * ld_out >= N of every selected cell (TCI_ERANGE). TCI_EINVAL, naming the index, for an s2 entry that is not finite
 * and > 0 or a level that is not inside (0, 1); for n_levels outside [1, 8] or scratch_bytes < 0. The simulated rows
 * (2 * n_sel * S * ld_out doubles) live in the scratch buffer the context owns; past opt->scratch_bytes whole cells
 * are processed in chunks (the same bits), and TCI_EINVAL is returned when one cell alone does not fit. Every check
 * comes before any device work. */
int tci_fitcheck(tci_ctx* ctx, const tci_fitcheck_options* opt, const double* theta, int64_t ld_theta, const double* s2,
                 const int32_t* cell_id, int64_t n_sel, int64_t S, int64_t ld_out, tci_fitcheck_outputs* out);

/* ---- PSIS-LOO per chain and stacking weights across the chains of a cell (loocheck) ----
 * How well does a chain predict the data it was not fitted to, and how should replicate chains that do not mix be
 * weighted? Per selected chain and per scored datum: the Pareto-smoothed importance-sampling leave-one-out log
 * predictive density (Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024), its Pareto k diagnostic, and per group of
 * chains of one cell the simplex weights that maximise the stacked LOO density (Yao, Vehtari, Gelman 2022). The
 * formulas below are the definition.
 * Inputs, forward model, data, host values sd_s, lg_s, logS, the rule for scored points and r_s, z_s, ll_s: exactly
 *   those of tci_fitcheck; "selected cell k" there is "selected chain k" here. 32 <= S <= 4096.
 * For a scored point, every operation rounded once, as written, never fused; exp, log, log1p and expm1 are the device
 * library's (no fast-math variants); every SUM runs in ascending index from 0.0 unless stated.
 * Tail selection.
 *   lr_s = -ll_s;   mx = max_s lr_s;   lr_s = lr_s - mx
 *   M = min(floor(S / 5), ceil(3 * sqrt(S)))                      6 <= M <= 192
 *   Total order on the samples: by lr_s as tci_chainquant orders doubles (-0 < +0, NaN above +Inf), ties by ascending
 *   s (among equal values the larger s is the larger). The tail is the M largest; cut = the largest lr_s not in the
 *   tail; tail_1 <= ... <= tail_M the tail in that order. Membership and order are exact.
 * Generalised-Pareto fit (Zhang and Stephens 2009 with the weak prior of Vehtari et al.).
 *   ec = exp(cut);   x_j = exp(tail_j) - ec, j = 1 .. M
 *   degenerate when x_M <= 0, x_M is not finite or x_1 < 0: khat = +Inf and the tail stays as it is. Otherwise
 *   G = 30 + floor(sqrt(M));   xq = x_{floor(M / 4 + 0.5)};   c_g = 1 - sqrt(G / (g - 0.5)), the host's, g = 1 .. G
 *   b_g = 1 / x_M + c_g / (3 * xq)
 *   k_g = (SUM_j log1p(-b_g * x_j)) / M
 *   L_g = M * ((log(-b_g / k_g) + (-k_g)) - 1)
 *   w_g = 1 / SUM_h exp(L_h - L_g);   b = SUM_g b_g * w_g
 *   k = (SUM_j log1p(-b * x_j)) / M;   sigma = -k / b;   khat = (k * M + 5.0) / (M + 10)
 *   khat or sigma not finite: degenerate as above.
 * Smoothing (not degenerate).   p_j = (j - 0.5) / M;   q_j = (sigma * expm1(-khat * log1p(-p_j))) / khat
 *   (the generalised-Pareto quantile sigma ((1 - p)^(-khat) - 1) / khat at the regularised khat)
 *   tail_j = min(log(q_j + ec), 0.0), a NaN kept
 *   lw_s: lr_s with the tail entries replaced by rank.
 * Outputs per point.
 *   lse(v) = mv + log(SUM_s exp(v_s - mv)), mv = max_s v_s, SUM_s in tci_fitcheck's order (segments of 64 samples)
 *   elpd_loo_i = lse(lw + ll) - lse(lw);   lppd_i: tci_fitcheck's, the same bits;   p_loo_i = lppd_i - elpd_loo_i
 *   khat_i
 *   Unscored points and padding (j from N to ld_out): NaN in all four.
 * Per selected chain, on the host from the pointwise vectors (dye 0 ascending j, then dye 1, scored points, sums from
 *   0.0): n_obs; elpd_loo, p_loo, lppd (sums); khat_max; n_khat_bad = #{i : khat_i > khat_threshold}. n_obs == 0: NaN.
 * Per group. group[k] in [0, n_groups) puts chain k into a group, -1 (or group == NULL) into none. All chains of a
 *   group select one cell (TCI_EINVAL). Over the n points scored in every chain c = 1 .. C of the group (in the order
 *   given) with finite e_ic = elpd_loo_i of chain c, from w_c = 1 / C, with the C library's exp and log:
 *     m_i = max_c e_ic;   a_ic = w_c * exp(e_ic - m_i);   w_c <- (SUM_i (a_ic / SUM_c' a_ic')) / n
 *   until max_iter iterations are done or max_c |new w_c - w_c| <= tol (n_iter counts the iterations done). Every step
 *   raises SUM_i log SUM_c w_c exp(e_ic), whose maximiser is the stacking weight vector.
 *     weight[k]      w_c of chain k in its group; NaN for a chain in no group
 *     elpd_stack[g]  SUM_i (m_i + log SUM_c w_c * exp(e_ic - m_i)) at the final weights
 *     n_points[g]    n;   n_iter[g]
 *   One chain: weight 1, n_iter 0. n == 0 or an empty group: NaN weights and elpd_stack, n_iter 0.
 * Bits. A chain's pointwise and per-chain outputs depend on its samples in order, its data, S and khat_threshold
 * alone: not on n_sel, the chain's position, ld_theta, ld_out, scratch_bytes, the tile shape or how many workgroups
 * ran. A group's outputs depend on its chains' pointwise outputs in order.
 * Error. Tail membership, order and cut are exact; lppd_i has tci_fitcheck's bound. khat passes through a profile
 * likelihood over G <= 43 points; no useful a-priori bound came out, and the tests compare with a float64 restatement
 * within 8 x the largest difference between that restatement and its long-double twin on the test inputs
 * (profiles/loocheck/tolerance.json). */
typedef struct {
  int64_t scratch_bytes;   /* cap on the device scratch for simulated rows; 0 = default (1 GiB) */
  int64_t n_groups;        /* length of the per-group outputs; group ids lie in [-1, n_groups); default 0 */
  double khat_threshold;   /* 0 = default: min(1 - 1 / log10(S), 0.7); else finite and > 0 */
  int64_t max_iter;        /* stacking iterations, >= 1; default 5000 */
  double tol;              /* >= 0; default 1e-12 */
} tci_loocheck_options;

/* Host buffers (any pointer may be NULL). */
typedef struct {
  double *elpd_loo_i, *lppd_i, *p_loo_i, *khat_i;  /* pointwise, each [n_sel][2][ld_out]: dye 0 = MS2, 1 = PP7 */
  int32_t* n_obs;                                  /* [n_sel] */
  double *elpd_loo, *p_loo, *lppd, *khat_max;      /* [n_sel] */
  int32_t* n_khat_bad;                             /* [n_sel] */
  double* weight;                                  /* [n_sel] */
  double* elpd_stack;                              /* [n_groups] */
  int32_t *n_points, *n_iter;                      /* [n_groups] */
  double khat_threshold;  /* written: the threshold used */
  double kernel_ms;       /* written: device time of the loocheck kernel (HIP events), summed over the chunks */
  double forward_ms;      /* written: device time of the forward launches that fill the scratch */
} tci_loocheck_outputs;

int tci_loocheck_defaults(tci_loocheck_options* opt);

/* HOST pointers, synchronous. opt may be NULL (the defaults); out is required; group may be NULL. 32 <= S <= 4096
 * (TCI_EINVAL); ld_theta >= 7 + N and ld_out >= N of every selected cell (TCI_ERANGE). TCI_EINVAL, naming the index,
 * for an s2 entry that is not finite and > 0 and for a group whose chains select different cells; TCI_ERANGE for a
 * group id outside [-1, n_groups); TCI_EINVAL for scratch_bytes < 0, n_groups < 0, max_iter < 1, tol < 0 or not
 * finite, khat_threshold < 0 or not finite. Scratch and chunking as for tci_fitcheck. Every check comes before any
 * device work. */
int tci_loocheck(tci_ctx* ctx, const tci_loocheck_options* opt, const double* theta, int64_t ld_theta, const double* s2,
                 const int32_t* cell_id, const int32_t* group, int64_t n_sel, int64_t S, int64_t ld_out,
                 tci_loocheck_outputs* out);

/* ---- Log-posterior trace, best sample and DIC of every chain (mcmcstat's sschain, mcmcrun's fourth output) ----
 * mcmcrun returns [results, chain, s2chain, sschain]; the sampler here keeps no SS. The kept rows are re-evaluated
 * instead: the engines are bitwise identical to the batched likelihood kernel, so the recomputed SS is the SS the
 * sampler saw. Everything is per chain c over its n = n_rows rows; P = 7 + N is the parameter count of cell
 * cell_id[c] and nobs = 2 N the sampler's observation count, NaNs included (the count the sigma2 update uses). All in
 * FP64, every operation rounded once as written, never fused; log is the device library's (no fast-math variant).
 * Per row t:
 *   ss_t   the batched likelihood kernel's SS of chain[t][c][0..P): the bits of tci_ss_batch_async on that row;
 *          mcmcstat's sschain.
 *   pri_t  SUM_{j < P} ((theta_tj - mu_j) / sig_j)^2: a subtraction, a division and a multiplication per term. Order:
 *          64 partial sums; partial l adds the terms j = l, l + 64, .. in ascending j from 0.0; the partials are then
 *          added in ascending l from 0.0. A term with sig_j = +Inf is exactly 0 and is not special-cased. Entries
 *          j >= P (of the row, of mu and of sig) are never read.
 *   dev_t  ss_t / s2_t + nobs * log(6.283185307179586 * s2_t): -2 log likelihood at (theta_t, sigma2_t).
 *   lp_t   -0.5 * (dev_t + pri_t): the log of likelihood x theta-prior at the sampled point, up to a constant.
 * Nothing is special-cased: a non-finite theta gives the kernel's NaN, s2_t <= 0 what the formulas give, and the
 * traces carry it.
 * Per chain, from the four traces. Every sum over rows runs in segments of 256 consecutive rows (the boundaries
 * follow from n alone, as in tci_chainrhat); inside a segment the terms are added in ascending t from 0.0, the
 * segment sums are then added in ascending order from 0.0:
 *   ss_min     the least ss_t;   ss_mean = (SUM ss_t) / n
 *   dev_mean   (SUM dev_t) / n
 *   dev_var    (SUM (dev_t - dev_mean)^2) / (n - 1); NaN for n = 1 (0 / 0)
 *   best_row   the least t whose lp_t equals the largest lp_t of the chain, compared on the device's own values;
 *              0-based among the n reduced rows
 *   lp_best, ss_best, s2_best   the values of that row;   theta_best[0..P) that chain row's bits
 *   theta_mean[j]   exactly tci_chaincov's mean (Neumaier sum, constant-column rule; the same bits);
 *   s2_mean    the same rule on the s2 column
 *   ss_hat     the likelihood kernel's SS of theta_mean
 *   d_hat      ss_hat / s2_mean + nobs * log(6.283185307179586 * s2_mean)
 *   p_d = dev_mean - d_hat;   p_v = 0.5 * dev_var;   dic = dev_mean + p_d
 * A non-finite ss_t, pri_t or dev_t anywhere in a chain: every reduced output of that chain is NaN (theta_mean,
 * s2_mean and ss_hat included), best_row is -1 and theta_best is NaN; the traces keep what the formulas gave.
 * Padding of theta_best and theta_mean (j >= P) is NaN.
 * Bits. An output depends on the chain's rows in order, its s2, the cell, mu, sig and n alone: not on n_chains, the
 * chain's position, ld or how many workgroups ran.
 * Error bound. ss, pri, best_row, theta_best, theta_mean and ss_hat are exact: a float64 restatement in the stated
 * order gives the same bits, and so does it for every reduced value when applied to the returned traces. dev, lp
 * and d_hat go through log. With u = 2^-53, the device log within K_log = 3 ulp (1 ulp = 2 u; the figure of
 * tci_fitcheck), L = log(6.283185307179586 * s2) and the formulas evaluated without rounding on the same ss, s2, pri:
 *   |dev - exact|   <= E_dev = 1.01 u (|ss / s2| + nobs (1 + (2 K_log + 1) |L|) + |dev|)
 *   |lp - exact|    <= 0.5 E_dev + 1.01 u |lp|
 *   |d_hat - exact| <= E_dev at (ss_hat, s2_mean)
 * (DESIGN.md section 7i has the derivation; tests/chainlp_oracle.py restates the bound). */
typedef struct {
  int64_t flags;  /* reserved, must be 0 */
} tci_chainlp_options;

/* Host buffers (any pointer may be NULL). */
typedef struct {
  double *ss, *pri, *dev, *lp;                           /* traces, each [n_rows][n_chains] */
  double *ss_min, *ss_mean, *dev_mean, *dev_var;         /* [n_chains] */
  double *lp_best, *ss_best, *s2_best;                   /* [n_chains] */
  double *s2_mean, *ss_hat, *d_hat, *p_d, *p_v, *dic;    /* [n_chains] */
  int64_t* best_row;                                     /* [n_chains]; -1: a non-finite trace value */
  double *theta_best, *theta_mean;                       /* [n_chains][ld] */
  int64_t n_rows;    /* written: rows the reduction used */
  double kernel_ms;  /* written: device time of the kernels (HIP events), the two likelihood launches included */
} tci_chainlp_outputs;

int tci_chainlp_defaults(tci_chainlp_options* opt);

/* The reduction of a chain already on the host (e.g. read back from a _RawChain file): chain is
 * [n_rows][n_chains][ld], s2chain [n_rows][n_chains] (required), cell_id [n_chains], prior_mu and prior_sig
 * [n_chains][ld] as for tci_dram_run. opt may be NULL (the defaults). Checked in this order, all before any device
 * work: TCI_EINVAL for a null argument, n_rows < 1, n_chains < 1 or flags != 0; TCI_ERANGE for a cell id out of
 * range, ld < 7 + N of a chain's cell or n_rows * n_chains at or above 2^31; TCI_EINVAL, naming the chain and the
 * index, for a prior_mu entry with j < P that is not finite or a prior_sig entry with j < P that is NaN or <= 0;
 * TCI_ENOMEM when the chain does not fit the device. */
int tci_chainlp(tci_ctx* ctx, const tci_chainlp_options* opt, const double* chain, const double* s2chain,
                int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* cell_id, const double* prior_mu,
                const double* prior_sig, tci_chainlp_outputs* out);

/* tci_dram_run_ess plus tci_chainlp's outputs of the same rows (the kept rows whose 1-based chain row is >=
 * stats_from), taken from the device chain before any copy, with the priors and cell ids the run already has on the
 * device. lout is required; lopt may be NULL. red may be NULL (no per-chain reduction). group == NULL: no group
 * reduction (n_groups, ropt, rout, eopt and eout are ignored); else group, n_groups, ropt, rout, eopt and eout as in
 * tci_dram_run_ess, where either of rout and eout may be NULL but not both. tci_dram_reductions keeps its eight
 * fields: a caller-allocated struct cannot grow without breaking the callers built against it, so this reduction is
 * asked for here, as the group reductions are. TCI_EINVAL when opt->thin == 0 or no kept row is in the range, for
 * lopt->flags != 0 and for a prior tci_chainlp refuses. Every engine gives the same chain bits, hence the same bits
 * here. */
int tci_dram_run_lp(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                    const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                    const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                    tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                    const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                    tci_chainess_outputs* eout, const tci_chainlp_options* lopt, tci_chainlp_outputs* lout);

/* ---- Parallel tempering: a ladder of chains per cell that exchange states on the device ----
 * Replica exchange (Swendsen and Wang 1986; Geyer 1991) for chains that do not mix. A ladder is a set of chains of one
 * cell, its rungs in ascending chain index, at inverse temperatures 1 >= beta_0 > beta_1 > ... . A rung with inverse
 * temperature beta samples the posterior with the likelihood alone tempered,
 *   pi_beta(theta, sigma2) ~ [ (2 pi sigma2)^(-N/2) exp(-ss(theta) / (2 sigma2)) ]^beta * (1 / sigma2) * prior(theta),
 * N = 2 N_c the chain's observation count; the theta prior and the implicit 1 / sigma2 prior are not tempered. Its
 * theta-conditional is the plain acceptance rule with 1 / sigma2 replaced by beta / sigma2 and its sigma2-conditional
 * 1 / sigma2 ~ Gamma(beta N / 2, scale 2 / (beta ss)). The sampler holds s2t = sigma2 / beta for such a rung: every
 * acceptance is then the plain sampler's, and the Gibbs draw is 1 / s2t ~ Gamma(beta N / 2, scale 2 / ss).
 *   UNITS. sigma2_0 is passed physical and stored as sigma2_0 / beta. Every s2 OUTPUT of a rung with beta < 1 is in
 *   s2t = sigma2 / beta: s2chain, sigma_mean, sigma_std and the s2 columns of every reduction. The cold rung (beta = 1)
 *   is physical, and it is the posterior sample.
 * Swaps. The chain rows are cut into windows of `win` rows (adaptint, or 100 without adaptation). After the row
 * s = w * win that ends window w has been logged and adapted, and only when s < n_steps (never after the run's last
 * row), neighbouring rungs exchange states when w % swap_every == 0: event e = w / swap_every - 1 tries the pairs
 * (r, r + 1) of every ladder with r congruent to w / swap_every modulo 2, so a ladder with an odd rung count leaves one
 * rung idle each time. For a = rung r and b = rung r + 1, with the physical sigma2_x = beta_x * s2t_x and
 *   dev_x = ss_x / sigma2_x + nobs * log(6.283185307179586 * sigma2_x)     (tci_chainlp's dev, the same operations)
 *   logr  = (0.5 * (beta_a - beta_b)) * (dev_a - dev_b)
 * the swap is accepted iff u < exp(logr), u the uniform of stream (seed, chain_keys[a], row s, purpose 6); a logr that
 * is not finite is rejected. On accept theta, ss and the prior SS change places; with updatesigma = 1 the physical
 * sigma2 does too (s2t_a = (beta_b * s2t_b) / beta_a, s2t_b = (beta_a * s2t_a_old) / beta_b); with updatesigma = 0
 * sigma2 is a constant of the model and stays. The adaptation state (covariance, mean, proposal factor, window,
 * counters: accept_rate and n_evals) stays with the rung. Every engine gives the same bits.
 * A call whose beta are all 1 and that never swaps, and any chain with ladder = -1 and beta = 1, has tci_dram_run's bits.
 * Checked before any device work (TCI_EINVAL, the ladder or chain named in the message): beta finite and in (0, 1];
 * with updatesigma = 1, beta * N / 2 >= 1 (the Gamma sampler's range); ladder values in [-1, n_ladders); beta strictly decreasing along a
 * ladder; all rungs of a ladder with the same cell, lower, upper, prior_mu and prior_sig; with updatesigma = 0 the same
 * sigma2_0; swap_every >= 0 (0: never swap); flags == 0. */
typedef struct {
  const double* beta;    /* [n_chains]; NULL: 1 for every chain */
  const int32_t* ladder; /* [n_chains], -1: in no ladder; NULL: -1 for every chain */
  int64_t n_ladders;
  int64_t swap_every;
  int64_t flags;         /* reserved, must be 0 */
} tci_temper_options;

/* Host buffers (any pointer may be NULL). swap_tried / swap_accepted count at the lower rung of a pair (0 elsewhere).
 * The logs have one row per swap event, at most swap_log_rows of them are written (events past it are counted only):
 * swap_logr is logr at the lower rung of every pair tried and NaN elsewhere, swap_acc 1 where the swap was accepted. */
typedef struct {
  int32_t *swap_tried, *swap_accepted; /* [n_chains] */
  double* swap_logr;                   /* [swap_log_rows][n_chains] */
  uint8_t* swap_acc;                   /* [swap_log_rows][n_chains] */
  int64_t swap_log_rows;               /* rows the two logs hold (the caller's) */
  int64_t n_events;                    /* written: swap events of the run */
} tci_temper_outputs;

int tci_temper_defaults(tci_temper_options* opt); /* no ladders, swap_every = 1 */

/* tci_dram_run_rhat with the ladder added: red, group, ropt and rout as there, but rout may be NULL (then group,
 * n_groups and ropt are ignored and no group reduction runs). topt NULL is tci_temper_defaults; tout may be NULL. */
int tci_dram_run_tempered(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                          const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                          const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                          tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                          const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_temper_options* topt,
                          tci_temper_outputs* tout);

/* ---- Population mode search per cell before sampling (differential evolution, Storn and Price 1997) ----
 * Replicate chains of a cell settle in separate modes, and every chain starts from one draw of the reference's x0
 * distribution (TranscriptionCycleMCMC.m:200-210). This looks for a good mode first. The SS is discontinuous in theta
 * (floor and strict masks), so the search uses SS values alone: DE/rand/1/bin on the batched likelihood kernel.
 * For each selected cell k in [0, n_sel), P = 7 + N of cell cell_id[k], a population of n_pop members (theta rows of ld
 * doubles) runs n_gen generations. All in FP64, every operation rounded once as written, never fused.
 * Objective. f = ss / s2[k] + pri: ss the bits of tci_ss_batch_async on the row, pri exactly tci_chainlp's pri_t (the
 *   same 64-partial order, the same sig = +Inf rule, the same device code), s2[k] a per-cell input (the reference's
 *   model.sigma2 is 1).
 * Generation 0 evaluates f of every member of pop0.
 * Generation g = 1 .. n_gen, member i. All members read the population as it stood after generation g - 1
 * (synchronous DE). rng(seed, key, step, purpose, idx) is the sampler's Philox4x32-10 stream with the counter
 * (key, step, purpose, idx); purposes 1-6 are the sampler's. m(w, n) = (uint32)(((uint64)w * n) >> 32).
 *   Index draw. w = rng(seed, key[k], g, 7, i):
 *     r1 = m(w.x, n_pop - 1), then + 1 if >= i;
 *     r2 = m(w.y, n_pop - 2), then, over {i, r1} sorted ascending, + 1 for each excluded value it has reached, tested
 *          in ascending order;
 *     r3 = m(w.z, n_pop - 3), the same over {i, r1, r2};
 *     jrand = m(w.w, P).
 *   Crossover uniform of coordinate j. c = rng(seed, key[k], g, 8, i * 2048 + (j >> 1)); u_j = u01(c.x, c.y) for even
 *     j, u01(c.z, c.w) for odd j, u01(a, b) = ((double)((((uint64)a << 32) | b) >> 11) + 0.5) * 2^-53 as in the sampler.
 *     P <= 7 + TCI_MAX_POINTS = 2055, so j >> 1 < 2048 and no two members of a cell share a counter.
 *   Mutant.  v_j = x[r1][j] + F * (x[r2][j] - x[r3][j]): a subtraction, a multiplication, an addition.
 *   Trial.   t_j = v_j when (u_j < CR || j == jrand) and v_j >= lower_j && v_j <= upper_j; else t_j = x[i][j]: a NaN or
 *     out-of-bounds mutant coordinate keeps the parent's, so a trial is always in bounds and always evaluated. Entries
 *     j >= P are copied from the parent.
 *   Selection. The trial replaces the parent iff f_trial <= f_parent; a NaN f_trial never replaces.
 * best[k] is the member that comes first when the members are ordered by (f is NaN, f, index): the least index whose f
 * is the least, compared on the device's own values, a NaN f after every number.
 * Bits. A cell's outputs depend on its population, data, bounds, priors, s2, key, seed and options alone: not on n_sel,
 * the cell's position, ld, the launch shapes or how many generations share a launch. ss is the likelihood kernel's and
 * pri tci_chainlp's; everything else is exact in the stated order, so a float64 restatement that takes ss from the
 * kernel gives every output's bits (tests/modesearch_oracle.py). */
typedef struct {
  int64_t n_gen;       /* generations, >= 0; default 500 */
  double F;            /* differential weight, finite and in (0, 2]; default 0.5 */
  double CR;           /* crossover rate in [0, 1]; default 0.9 */
  uint64_t seed;
  const int64_t* keys; /* optional [n_sel]: cell k draws from RNG stream keys[k] (NULL: stream k), taken modulo 2^32 as
                          tci_dram_options.chain_keys is. Keying by the dataset-wide cell index makes a shard of a
                          search reproduce the unsharded one */
  int64_t flags;       /* reserved, must be 0 */
} tci_modesearch_options;

/* Host buffers (any pointer may be NULL). */
typedef struct {
  double *pop;                            /* [n_sel][n_pop][ld]: the final population */
  double *f, *ss;                         /* [n_sel][n_pop]: of the final population */
  int32_t* best;                          /* [n_sel] */
  double* theta_best;                     /* [n_sel][ld]; padding (j >= P) is NaN */
  double *f_best, *ss_best, *pri_best;    /* [n_sel] */
  double* f_trace;                        /* [n_gen + 1][n_sel]: the least f after each generation (row 0: pop0's) */
  int32_t* n_accepted;                    /* [n_gen][n_sel]: trials that replaced their parent */
  int64_t n_evals;   /* written: SS evaluations, n_sel * n_pop * (n_gen + 1) */
  double kernel_ms;  /* written: device time of the search (HIP events), the likelihood launches included */
} tci_modesearch_outputs;

int tci_modesearch_defaults(tci_modesearch_options* opt);

/* HOST pointers, synchronous. pop0 is [n_sel][n_pop][ld]; lower, upper, prior_mu and prior_sig are [n_sel][ld] as for
 * tci_dram_run; s2 is [n_sel]. opt may be NULL (the defaults); out is required. Checked in this order, all before any
 * device work: TCI_EINVAL for a null argument, n_sel < 1, flags != 0, n_gen < 0, F not finite or outside (0, 2], CR
 * outside [0, 1] or NaN, n_pop outside [4, 4096] or n_sel * n_pop at or above 2^31; TCI_ERANGE for ld outside
 * [1, 2^24]; TCI_EINVAL for (n_gen + 1) * n_sel at or above 2^31 (the traces); TCI_ERANGE for a cell id out of
 * range or ld < 7 + N of a selected cell; TCI_EINVAL, naming the cell and the index, for a prior tci_chainlp refuses
 * and an s2 entry that is not finite and > 0; TCI_EINVAL, naming cell, member and index, for a pop0 entry with j < P
 * that is not finite or lies outside [lower_j, upper_j]. TCI_ENOMEM when the populations do not fit the device. */
int tci_modesearch(tci_ctx* ctx, const tci_modesearch_options* opt, const double* pop0, int64_t ld,
                   const int32_t* cell_id, int64_t n_sel, int64_t n_pop, const double* lower, const double* upper,
                   const double* prior_mu, const double* prior_sig, const double* s2, tci_modesearch_outputs* out);

/* ---- DE-MC population sampler per cell (differential-evolution Markov chain, ter Braak 2006) ----
 * A sampler beside DRAM. A population of states of one cell already encodes the posterior's scale and correlations:
 * a member is proposed along the difference of two other members, so no covariance is adapted, and with gamma = 1 a
 * member jumps between modes that two others occupy. mcmcstat has no such sampler: the text below is the definition.
 * For each selected cell k in [0, n_sel), P = 7 + N of cell cell_id[k], a population of n_pop members runs n_gen
 * generations. A member is a theta row of ld doubles plus its own sigma2. All in FP64, every operation rounded once as
 * written, never fused. Member i of cell k is chain b = k * n_pop + i in every output (n_chains = n_sel * n_pop).
 * State per member: theta; ss, the bits of tci_ss_batch_async on the row; pri, exactly tci_chainlp's pri_t (the same
 *   device code); s2, starting at sigma2_0[k].
 * Generation 0 evaluates ss and pri of pop0.
 * Generation g = 1 .. n_gen is two half-sweeps, h = 0 then h = 1. In half-sweep h the members with i mod 2 == h move
 *   and the others rest; a moving member takes its pair from the resting half as it stands now (after half-sweep 0 of
 *   the same generation for h = 1). Updating all members at once from the old population is not reversible; the
 *   two-set update is (the standard parallel form of ensemble moves). n_pop >= 4, so either half has 2 members.
 * rng(seed, key, step, purpose, idx), m(w, n) and u01(a, b) are tci_modesearch's; step = 2 g + h; purposes 9-12.
 *   Index draw. w = rng(seed, key[k], step, 9, i). R = the resting members ascending, n_R of them:
 *     a = m(w.x, n_R); c = m(w.y, n_R - 1), then + 1 if >= a; r1 = R[a], r2 = R[c]; jrand = m(w.z, P).
 *   Coordinate j < P. q = rng(seed, key[k], step, 10, i * 4096 + j): u_j = u01(q.x, q.y), v_j = u01(q.z, q.w).
 *     j < 2055 and i < 4096, so no two (member, coordinate) pairs share a counter.
 *   Jump generation (jump_every > 0 and g mod jump_every == 0): every j < P crosses and gamma = 1.
 *   Other generations: j crosses iff u_j < CR or j == jrand; d' = the number of crossing coordinates (>= 1);
 *     gamma = gamma0 / sqrt((double)(2 d')), sqrt and division correctly rounded. gamma0 <= 0 means 2.38.
 *   Trial. For a crossing j: t_j = (x_i[j] + gamma * (x_r1[j] - x_r2[j])) + jitter[k][j] * (2 * v_j - 1): the
 *     subtraction, the product, the addition; then 2 * v_j, minus 1, times jitter, and the last addition. A
 *     non-crossing j, and j >= P, keep the parent's bits. The jitter is uniform, not Gaussian, on purpose: it is
 *     symmetric, so detailed balance holds; with jitter_j > 0 it has positive width in every coordinate, so the chain
 *     is irreducible on a connected support; and it is exact arithmetic, so a restatement reproduces the bits.
 *   Bounds. If any crossing t_j is NaN or outside [lower_j, upper_j] the proposal is rejected without evaluation
 *     (mcmcstat's rule): the row reaches the likelihood launch inactive, counts in n_oob, and its logr is NaN.
 *   Acceptance. f_old = ss_i / s2_i + pri_i, formed afresh because s2 moves; f_new = ss_t / s2_i + pri_t;
 *     logr = -0.5 * (f_new - f_old). Accept iff logr >= 0, or u < exp(logr) with u = u01 of the x and y words of
 *     rng(seed, key[k], step, 11, i); a NaN logr rejects. exp is the device library's.
 *   sigma2. After the decision, with updatesigma: 1 / s2_i ~ Gamma(nobs / 2, scale 2 / ss_i), nobs = 2 N, as
 *     s2_i = 1 / (G * (2 / ss_i)), G the sampler's own Marsaglia-Tsang unit variate on stream (seed, key[k], step, 12):
 *     its try `it` (< 1024) reads the calls (i << 16) | it and (i << 16) | it | 2^31, and i < 4096 keeps i << 16 below
 *     2^28, so no two members share a call. Without updatesigma s2 never changes.
 * Kept rows: the states after generations g = 0, thin, 2 thin, ..: n_keep = n_gen / thin + 1 rows (thin = 0: none).
 *   sschain and prichain are the values the sampler held (mcmcstat's sschain), not re-evaluated.
 * Bits. A cell's outputs depend on its population, data, bounds, priors, jitter, sigma2_0, key, seed and options
 * alone: not on n_sel, the cell's position, ld or the launch shapes. Everything but ss, exp and the Gamma variate's
 * log, cos and sqrt is exact in the stated order, so a float64 restatement that takes ss from the kernel reproduces
 * every decision it can decide (tests/demc_oracle.py). */
typedef struct {
  int64_t n_gen;       /* generations, >= 0; default 1000 */
  int64_t thin;        /* keep every thin-th generation, >= 0 (0: no kept rows); default 1 */
  int64_t jump_every;  /* every jump_every-th generation is a jump generation, >= 0 (0: never); default 10 */
  int64_t stats_from;  /* the reductions use the kept rows of generations >= stats_from; default 0 */
  int64_t updatesigma; /* 0 or 1; default 1 */
  double CR;           /* crossover rate in [0, 1]; default 0.2 */
  double gamma0;       /* finite; <= 0 means 2.38; default 0 */
  uint64_t seed;
  const int64_t* keys; /* optional [n_sel], as tci_modesearch_options.keys */
  int64_t flags;       /* reserved, must be 0 */
} tci_demc_options;

/* Host buffers (any pointer may be NULL). n_chains = n_sel * n_pop. The logs hold generation g = 1 .. min(n_gen,
 * log_rows) in row g - 1: every member moves once per generation. */
typedef struct {
  double *chain;                          /* [n_keep][n_chains][ld] */
  double *s2chain, *sschain, *prichain;   /* [n_keep][n_chains] */
  double *pop;                            /* [n_chains][ld]: the final population */
  double *s2, *ss;                        /* [n_chains]: of the final population */
  double* accept_rate;                    /* [n_chains]: accepted proposals / n_gen (NaN for n_gen = 0) */
  int32_t* n_oob;                         /* [n_chains]: proposals rejected at the bounds */
  int64_t* n_evals;                       /* [n_chains]: SS evaluations, 1 + n_gen - n_oob */
  double* logr;                           /* [log_rows][n_chains]; NaN for a proposal rejected at the bounds */
  uint8_t *accepted, *trial_oob;          /* [log_rows][n_chains] */
  int64_t log_rows;                       /* rows the three logs hold (the caller's) */
  int64_t n_keep;    /* written: kept rows */
  double kernel_ms;  /* written: device time of the run (HIP events), the likelihood launches included */
} tci_demc_outputs;

int tci_demc_defaults(tci_demc_options* opt);

/* HOST pointers, synchronous. pop0 is [n_sel][n_pop][ld]; lower, upper, prior_mu, prior_sig and jitter are
 * [n_sel][ld]; sigma2_0 is [n_sel]. opt may be NULL (the defaults); out is required. rout and eout may be NULL: when
 * given, tci_chainrhat / tci_chainess (ropt, eopt may be NULL) of the kept rows of generations >= stats_from are taken
 * from the device chain before any copy, with the members of cell k as group k and npar = P; the device chain exists
 * for them alone when out->chain is NULL. Checked in this order, all before any device work: TCI_EINVAL for a null
 * argument, n_sel < 1, flags != 0, n_gen, thin, jump_every or stats_from < 0, updatesigma outside {0, 1}, CR outside
 * [0, 1] or NaN, gamma0 not finite, log_rows < 0, n_pop outside [4, 4096], n_sel * n_pop or n_gen at or above 2^31;
 * TCI_ERANGE for ld outside [1, 2^24], a cell id out of range or ld < 7 + N of a selected cell; TCI_EINVAL, naming the
 * cell (and the index), for a prior tci_chainlp refuses, a jitter entry with j < P that is not finite or < 0, a
 * sigma2_0 that is not finite and > 0, nobs / 2 < 1 with updatesigma; TCI_EINVAL, naming cell, member and index, for a
 * pop0 entry with j < P that is not finite or lies outside [lower_j, upper_j]; TCI_EINVAL for a reduction without kept
 * rows (thin = 0), with fewer than 2 kept rows at or past stats_from, with max_lag < 0 or reduction flags != 0.
 * TCI_ENOMEM, with the byte count in the message, when the population and the chain do not fit the device. */
int tci_demc_run(tci_ctx* ctx, const tci_demc_options* opt, const double* pop0, int64_t ld, const int32_t* cell_id,
                 int64_t n_sel, int64_t n_pop, const double* lower, const double* upper, const double* prior_mu,
                 const double* prior_sig, const double* jitter, const double* sigma2_0, tci_demc_outputs* out,
                 const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                 tci_chainess_outputs* eout);

/* tci_demc_run plus tci_chainrank (kopt may be NULL) of the same groups over the same kept rows, from the device chain
 * before any copy; kout NULL: exactly tci_demc_run. The options of kopt are checked with the other reductions'. */
int tci_demc_run_rank(tci_ctx* ctx, const tci_demc_options* opt, const double* pop0, int64_t ld, const int32_t* cell_id,
                      int64_t n_sel, int64_t n_pop, const double* lower, const double* upper, const double* prior_mu,
                      const double* prior_sig, const double* jitter, const double* sigma2_0, tci_demc_outputs* out,
                      const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                      tci_chainess_outputs* eout, const tci_chainrank_options* kopt, tci_chainrank_outputs* kout);

/* ---- DE-MC(zs) sampler per cell (ter Braak & Vrugt 2008, Statistics and Computing 18:435) ----
 * A third sampler beside DRAM and DE-MC. A few chains per cell take their difference vectors from an archive Z of past
 * states instead of from the current population: Z starts with m0 >> P rows and grows while the run goes on, so the
 * differences span the whole space from the first generation and shrink as the chains contract; a share of the moves
 * are snooker updates along the line through the current state and an archive point; and the archive does not depend
 * on the other chains' current states, so every chain moves in every generation: one likelihood launch per generation
 * where tci_demc_run has two half-sweeps. All in FP64, every operation rounded once as written, never fused. Names not
 * defined here (rng, m, u01, the bounds rule, f_old / f_new, the sigma2 draw, kept rows, keys) are tci_demc_run's.
 * For each selected cell k, P = 7 + N of cell cell_id[k]: n_pop chains, 1 <= n_pop <= 4096, start at pop0[k]; the
 *   archive of M rows of ld doubles starts as z0[k], m0 rows, 3 <= m0, each checked like a pop0 row. Chain i of cell k
 *   is chain b = k * n_pop + i in every output (n_chains = n_sel * n_pop).
 * Generation 0 evaluates ss and pri of pop0.
 * Generation g = 1 .. n_gen: all chains move, from the states and the archive as they stood after generation g - 1. The
 *   step is g. M_g = m0 + n_pop * floor((g - 1) / append_every) rows of the archive are read. After the decisions of a
 *   generation with g mod append_every == 0 the n_pop current states are appended to the archive in ascending i.
 *   Draws. Purposes 13 (index), 14 (coordinate), 15 (accept), 16 (sigma2). w = rng(seed, key[k], g, 13, i) and
 *     q = rng(seed, key[k], g, 13, 4096 + i). a = m(w.x, M_g); c = m(w.y, M_g - 1), then + 1 if >= a;
 *     e = m(w.w, M_g - 2), then + 1 if >= min(a, c), then + 1 if >= max(a, c): a, c, e distinct, each uniform given
 *     the ones before. jrand = m(w.z, P). The move is a snooker move iff u01(q.x, q.y) < p_snooker;
 *     gamma_s = 1.2 + u01(q.z, q.w).
 *   Parallel move: exactly tci_demc_run's trial with x_r1 = Z[a], x_r2 = Z[c]: the coordinate uniforms are those of
 *     rng(seed, key[k], g, 14, i * 4096 + j); crossover by CR and jrand, gamma = gamma0 / sqrt((double)(2 d')); a jump
 *     generation (jump_every > 0 and g mod jump_every == 0) crosses every coordinate with gamma = 1; the uniform jitter
 *     is tci_demc_run's. ljac = 0.
 *   Snooker move: no crossover, no jitter, no coordinate draws, unaffected by jump generations. z = Z[e], z1 = Z[a],
 *     z2 = Z[c]. For j < P: d_j = x_i[j] - z[j]; D = SUM d_j * d_j; A = SUM (z1[j] - z2[j]) * d_j (the subtraction,
 *     the product, the sum). If D == 0 or D is not finite the move is a NULL MOVE: rejected without evaluation, counted
 *     in n_null, logged with trial_oob = 2, logr and ljac NaN. It happens whenever a chain that has not moved since it
 *     was archived draws its own copy, so it is no corner case. Otherwise r = A / D, s = gamma_s * r and
 *     t_j = x_i[j] + s * d_j (the product, the addition) for every j < P; entries j >= P keep the parent's bits. The
 *     bounds rule applies over all j < P (an out-of-bounds snooker trial has ljac NaN). D' = SUM (t_j - z[j])^2;
 *     ljac = (0.5 * (double)(P - 1)) * (log(D') - log(D)), log the device library's. D' = 0 gives -Inf and rejects.
 *   The three sums have one order: lane l of 64 sums its terms j = l, l + 64, .. ascending from 0.0, and the 64
 *     partials combine by the xor butterfly p <- p + p[lane ^ d] for d = 32, 16, 8, 4, 2, 1. Addition commutes bitwise,
 *     so every lane holds the same value, and a restatement replays it with six pairwise folds. The prior stays in
 *     tci_chainlp's order, so prichain keeps equalling tci_chainlp's bits.
 *   Acceptance. logr = -0.5 * (f_new - f_old) + ljac, the last addition written as such. Accept iff logr >= 0, or
 *     u < exp(logr) with u = u01 of the x and y words of rng(seed, key[k], g, 15, i); a NaN logr rejects.
 *   sigma2: tci_demc_run's draw on stream (seed, key[k], g, 16), calls (i << 16) | it.
 * Validity. The chain is not Markov with a fixed kernel: the proposal depends on the archive, which grows. ter Braak &
 *   Vrugt show ergodicity by diminishing adaptation as M grows. Rows kept while the archive is young are burn-in, and
 *   stats_from is the caller's to set.
 * Bits. As tci_demc_run's, with z0 among what a cell's outputs depend on. ss, exp, the two logs of a snooker move and
 * the Gamma variate are the inexact steps; a float64 restatement that takes ss and ljac from the device reproduces
 * every decision it can decide (tests/demczs_oracle.py). */
typedef struct {
  int64_t n_gen, thin, jump_every, stats_from, updatesigma; /* as tci_demc_options */
  double CR, gamma0;                                        /* as tci_demc_options */
  uint64_t seed;
  const int64_t* keys;  /* optional [n_sel], as tci_demc_options.keys */
  int64_t flags;        /* reserved, must be 0 */
  int64_t append_every; /* the chains' states join the archive after every append_every-th generation, >= 1; default 10 */
  double p_snooker;     /* share of snooker moves, in [0, 1]; default 0.1 */
} tci_demczs_options;

/* Host buffers (any pointer may be NULL). The first sixteen fields are tci_demc_outputs'. */
typedef struct {
  double *chain;                          /* [n_keep][n_chains][ld] */
  double *s2chain, *sschain, *prichain;   /* [n_keep][n_chains] */
  double *pop;                            /* [n_chains][ld]: the chains' final states */
  double *s2, *ss;                        /* [n_chains]: of the final states */
  double* accept_rate;                    /* [n_chains]: accepted proposals / n_gen (NaN for n_gen = 0) */
  int32_t* n_oob;                         /* [n_chains]: proposals rejected at the bounds */
  int64_t* n_evals;                       /* [n_chains]: SS evaluations, 1 + n_gen - n_oob - n_null */
  double* logr;                           /* [log_rows][n_chains]; NaN for a proposal that was not evaluated */
  uint8_t *accepted, *trial_oob;          /* [log_rows][n_chains]; trial_oob: 0, 1 out of bounds, 2 a null move */
  int64_t log_rows;                       /* rows the five logs hold (the caller's) */
  int64_t n_keep;    /* written: kept rows */
  double kernel_ms;  /* written: device time of the run (HIP events), the likelihood launches included */
  int32_t* n_null;   /* [n_chains]: null snooker moves */
  double* ljac;      /* [log_rows][n_chains]: 0 for a parallel move, NaN for a null or out-of-bounds snooker move */
  uint8_t* snooker;  /* [log_rows][n_chains]: 1 for a snooker move */
  double* archive;   /* [n_sel][n_archive][ld]: z0 and the appended states, n_archive = m0 + n_pop * (n_gen / append_every) */
  int64_t n_archive; /* written: the final rows of a cell's archive */
} tci_demczs_outputs;

int tci_demczs_defaults(tci_demczs_options* opt);

/* HOST pointers, synchronous. pop0 is [n_sel][n_pop][ld], z0 [n_sel][m0][ld]; everything else is tci_demc_run's, the
 * reductions with the chains of cell k as group k included. Checked in tci_demc_run's order and wording, with these
 * differences: n_pop outside [1, 4096]; after gamma0, TCI_EINVAL for append_every < 1 and for p_snooker outside [0, 1]
 * or NaN; after n_pop, TCI_EINVAL for m0 < 3 and for an archive of 2^24 rows or more (m0 + n_pop * (n_gen /
 * append_every)); after the pop0 entries, TCI_EINVAL naming cell, row and index for a z0 entry with j < P that is not
 * finite or lies outside [lower_j, upper_j]. TCI_ENOMEM, with the byte count of every device buffer of the call in the
 * message, when the populations, the archive and the chain do not fit the device. */
int tci_demczs_run(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                   const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                   const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                   const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                   tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout);

/* tci_demczs_run plus tci_chainrank of the same groups over the same kept rows, as tci_demc_run_rank. */
int tci_demczs_run_rank(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                        const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                        const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                        const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                        tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout,
                        const tci_chainrank_options* kopt, tci_chainrank_outputs* kout);

/* ---- DE-MC(zs): per-coordinate bounds census and oriented reflection ----
 * tci_demczs_run_rank with two optional additions; everything not said here is tci_demczs_run's, bit for bit.
 * Census (census = 1, in either mode). For every generation g >= 1, chain b and coordinate j < P that CROSSES,
 *   n_cross[b][j] += 1; with t_j the RAW trial coordinate (before any reflection), oob_lo[b][j] += 1 if t_j < lower_j
 *   and oob_hi[b][j] += 1 if t_j > upper_j. A NaN counts in neither (the row's n_oob still catches it). In a parallel
 *   move the crossing coordinates are those of the crossover mask (all of them in a jump generation); in a snooker move
 *   every j < P crosses. n_left[g - 1][b] is the proposal's count of such coordinates, -1 for a null move; a null move
 *   touches no counter. Hence SUM_j (oob_lo + oob_hi)[b][j] = SUM_g n_left[g - 1][b] over the non-null moves when the
 *   log holds every generation, and in reject mode with NaN-free inputs n_left > 0 iff trial_oob == 1.
 * Reflect mode (mode = TCI_BOUNDS_REFLECT). Plain reflection of a leaving coordinate is NOT valid here: the difference
 *   of two archive rows is symmetric under d -> -d only, not under negating some coordinates. The valid form remembers
 *   its orientation. Unfold every coordinate onto a circle of circumference 2 w (the box and its mirror image), run the
 *   unchanged proposal there and store the state as the box coordinate plus one orientation bit per coordinate: an
 *   increment is applied with the sign of the bit and a reflection flips it. That is Metropolis on the unfolded torus
 *   with a translation-invariant proposal, which needs the d -> -d symmetry alone, and its marginal on the box is the
 *   target. Each chain carries orient[b][j] in {0, 1}, all 0 at the start (entries j >= P stay 0).
 *   Parallel move, crossing j, with tci_demc_run's s = gamma * d and zz = jitter_j * f: s' = orient ? -s : s,
 *     zz' = orient ? -zz : zz (negation is exact), y = x_j + s', t = y + zz', every other operation as in reject mode:
 *     with every bit 0 the raw trial has reject mode's bits. Then at most one reflection: if t < lower, e = lower - t
 *     and t' = lower + e; if t > upper, e = t - upper and t' = upper - e (a subtraction, then an addition or a
 *     subtraction, as written). The trial's bit is orient ^ 1 for a reflected coordinate, orient otherwise. If t' is
 *     NaN or still outside [lower, upper] (the overshoot exceeds the width) the proposal is rejected at the bounds as
 *     in reject mode: a second reflection is needed exactly when the unfolded segment crosses two wall points, and the
 *     reverse move crosses the same two, so the reject set is symmetric and the rule stays valid. n_refl[g - 1][b]
 *     counts the coordinates a reflection was applied to, whether or not the proposal then stayed inside; n_reflected[b]
 *     counts the evaluated proposals with n_refl > 0. An accepted trial's orientation row replaces the chain's.
 *   Snooker move: reject mode's rule in both modes, orient unchanged (a valid move on x alone), n_refl = 0.
 *   The archive, the kept rows, sschain, prichain, the reductions and the prior are in box coordinates, as always.
 * Census outputs: n_cross, oob_lo, oob_hi, n_left. Reflection outputs: n_refl, n_reflected, orient. */
#define TCI_BOUNDS_REJECT 0  /* tci_demczs_run's rule */
#define TCI_BOUNDS_REFLECT 1
typedef struct {
  int32_t mode;   /* TCI_BOUNDS_REJECT (default) or TCI_BOUNDS_REFLECT */
  int32_t census; /* 0 (default) or 1 */
  int64_t flags;  /* reserved, must be 0 */
} tci_bounds_options;

/* Host buffers (any pointer may be NULL); log_rows is tci_demczs_outputs'. */
typedef struct {
  int32_t *n_cross, *oob_lo, *oob_hi; /* [n_chains][ld]; padding j >= P is -1 */
  int32_t* n_left;      /* [log_rows][n_chains]: coordinates of the raw trial outside; -1 for a null move */
  int32_t* n_refl;      /* [log_rows][n_chains]: coordinates reflected (0 in reject mode and for snooker moves) */
  int32_t* n_reflected; /* [n_chains]: evaluated proposals with at least one reflection */
  uint8_t* orient;      /* [n_chains][ld]: the final orientation bits */
} tci_bounds_outputs;

int tci_bounds_defaults(tci_bounds_options* opt);

/* bopt and bout both NULL: exactly tci_demczs_run_rank. bopt NULL means the defaults. After tci_demczs_run_rank's
 * checks and before any device work, TCI_EINVAL naming the field for mode outside {0, 1}, census outside {0, 1},
 * flags != 0, a census output given with census = 0, a reflection output given in reject mode. With mode 0 and
 * census 0 the call makes tci_demczs_run_rank's device allocations, launches and copies and nothing else. */
int tci_demczs_run_bounds(tci_ctx* ctx, const tci_demczs_options* opt, const double* pop0, const double* z0, int64_t ld,
                          const int32_t* cell_id, int64_t n_sel, int64_t n_pop, int64_t m0, const double* lower,
                          const double* upper, const double* prior_mu, const double* prior_sig, const double* jitter,
                          const double* sigma2_0, tci_demczs_outputs* out, const tci_chainrhat_options* ropt,
                          tci_chainrhat_outputs* rout, const tci_chainess_options* eopt, tci_chainess_outputs* eout,
                          const tci_chainrank_options* kopt, tci_chainrank_outputs* kout, const tci_bounds_options* bopt,
                          tci_bounds_outputs* bout);

const char* tci_version(void);

#ifdef __cplusplus
}
#endif

#endif /* TCI_H_ */
