// tci_api.cpp -- C ABI (include/tci.h): context, resident cell table, validation, launches.
//
// The context replaces the per-call work the reference repeats inside every ssfun call
// (SumofSquaresFunction_TranscriptionCycleMCMC.m:28-30: the grid, which is theta-independent)
// with a one-time build at tci_create, and keeps the cell table resident in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <utility>
#include <string>
#include <vector>

#include "tci_diag.h"
#include "tci_dram_internal.h"
#include "tci_internal.h"

using tci::CellMeta;
using tci::KParams;

struct tci_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int rpl = 1;
  int64_t stride = 0;               // records per cell in the resident tables
  int64_t n_cells = 0;
  int64_t max_points = 0;
  int64_t device_bytes = 0;
  std::vector<CellMeta> meta;       // host copy
  std::vector<double> grid;         // host copy of t_interp (cell c at c * stride)
  KParams kp{};
  void* dbuf = nullptr;             // one allocation for the whole resident cell table
  // staging buffers for the host-pointer entry points
  double* d_theta = nullptr;
  int32_t* d_cell = nullptr;
  uint8_t* d_active = nullptr;
  double* d_out0 = nullptr;
  double* d_out1 = nullptr;
  size_t cap_theta = 0, cap_cell = 0, cap_active = 0, cap_out0 = 0, cap_out1 = 0;
  double* d_sim = nullptr;          // tci_predict: the simulated rows of one chunk of cells (MS2 rows, then PP7 rows)
  size_t cap_sim = 0;
  double* d_cov = nullptr;          // tci_chaincov: cov then corr of one group of chains
  size_t cap_cov = 0;
  // small batches of the host-pointer entry points: one pinned, device-mapped buffer the kernel
  // reads and writes in place (no copy launches; tci_ss_batch)
  char* h_io = nullptr;
  char* d_io = nullptr;
  size_t cap_io = 0;
  std::string err;
};

namespace {

const char kVersion[] = "tci-mi355x 0.1.0 (gfx950)";

int fail(tci_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

int hip_fail(tci_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, TCI_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define TCI_HIP(ctx, call)                                  \
  do {                                                      \
    hipError_t e_ = (call);                                 \
    if (e_ != hipSuccess) return hip_fail((ctx), e_, #call); \
  } while (0)

double round_half_away(double x) { return x >= 0 ? std::floor(x + 0.5) : -std::floor(-x + 0.5); }

// MATLAB a:d:b by the documented colon algorithm (colonop): n from round((b-a)/d) with a
// 2*eps*max(|a|,|b|) tolerance, right end snapped to b, and the vector built symmetrically
// from both ends. Used for t_interp = t(1):dt:t(end) (SumofSquares...m:30).
std::vector<double> colon(double a, double d, double b) {
  if (!std::isfinite(a) || !std::isfinite(d) || !std::isfinite(b)) return {NAN};
  if (d == 0 || (a < b && d < 0) || (b < a && d > 0)) return {};
  const double tol = 2.0 * 2.220446049250313e-16 * std::max(std::fabs(a), std::fabs(b));
  const double sig = d > 0 ? 1.0 : -1.0;
  double n;
  if (a == std::floor(a) && d == 1) {
    n = std::floor(b) - a;
  } else if (a == std::floor(a) && d == std::floor(d)) {
    const double q = std::floor(a / d);
    const double r = a - q * d;
    n = std::floor((b - r) / d) - q;
  } else {
    n = round_half_away((b - a) / d);
    if (sig * (a + n * d - b) > tol) n = n - 1;
  }
  if (!(n >= 0) || n > 1e7) return {};
  const int64_t ni = (int64_t)n;
  double c = a + n * d;
  if (sig * (c - b) > -tol) c = b;
  std::vector<double> v((size_t)ni + 1);
  for (int64_t k = 0; k <= ni / 2; ++k) {
    const double kd = (double)k;
    v[(size_t)k] = a + kd * d;
    v[(size_t)(ni - k)] = c - kd * d;
  }
  if (ni % 2 == 0) v[(size_t)(ni / 2)] = (a + c) / 2;
  return v;
}

// dt = mean(t(2:end)-t(1:end-1)) (sequential sum / count), then the colon grid.
std::vector<double> interp_grid(const double* t, int64_t n, double* d_out) {
  double s = 0.0;
  for (int64_t i = 0; i + 1 < n; ++i) s = s + (t[i + 1] - t[i]);
  const double d = s / (double)(n - 1);
  if (d_out) *d_out = d;
  return colon(t[0], d, t[n - 1]);
}

template <typename T>
int ensure(tci_ctx* ctx, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return TCI_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  size_t n = std::max(need, (size_t)1024);
  TCI_HIP(ctx, hipMalloc((void**)p, n * sizeof(T)));
  *cap = n;
  return TCI_OK;
}

// Bytes of theta + ids + flags + SS per call up to which tci_ss_batch works in place in pinned host
// memory (TCI_ZERO_COPY_MAX overrides; 0 disables).
size_t zero_copy_max() {
  static const size_t v = [] {
    const char* e = std::getenv("TCI_ZERO_COPY_MAX");
    return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)1024 * 1024;
  }();
  return v;
}

int ensure_io(tci_ctx* ctx, size_t need) {
  if (need <= ctx->cap_io) return TCI_OK;
  if (ctx->h_io) (void)hipHostFree(ctx->h_io);
  ctx->h_io = ctx->d_io = nullptr;
  ctx->cap_io = 0;
  const size_t n = std::max(need, (size_t)64 * 1024);
  TCI_HIP(ctx, hipHostMalloc((void**)&ctx->h_io, n, hipHostMallocMapped | hipHostMallocCoherent));
  TCI_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->d_io, ctx->h_io, 0));
  ctx->cap_io = n;
  return TCI_OK;
}

int check_construct(tci_ctx* ctx, const tci_construct* cs) {
  if (!cs) return fail(ctx, TCI_EINVAL, "construct is NULL");
  if (cs->n_seg < 1 || cs->n_seg > TCI_MAX_SEG)
    return fail(ctx, TCI_EINVAL, "construct n_seg must be in [1, " + std::to_string(TCI_MAX_SEG) + "]");
  if (!cs->ms2_start || !cs->ms2_end || !cs->ms2_loopn || !cs->pp7_start || !cs->pp7_end || !cs->pp7_loopn)
    return fail(ctx, TCI_EINVAL, "construct segment arrays must not be NULL");
  if (!std::isfinite(cs->L0)) return fail(ctx, TCI_EINVAL, "construct L0 must be finite");
  for (int s = 0; s < cs->n_seg; ++s) {
    const double vals[6] = {cs->ms2_start[s], cs->ms2_end[s], cs->ms2_loopn[s],
                            cs->pp7_start[s], cs->pp7_end[s], cs->pp7_loopn[s]};
    for (double x : vals)
      if (!std::isfinite(x)) return fail(ctx, TCI_EINVAL, "construct values must be finite");
    if (!(cs->ms2_start[s] >= 0 && cs->ms2_start[s] < cs->ms2_end[s] && cs->pp7_start[s] >= 0 &&
          cs->pp7_start[s] < cs->pp7_end[s]))
      return fail(ctx, TCI_EINVAL, "construct segment " + std::to_string(s) + " needs 0 <= start < end");
  }
  return TCI_OK;
}

void fill_segments(KParams* kp, const tci_construct* cs) {
  kp->L0 = cs->L0;
  kp->n_seg = cs->n_seg;
  double emax = 0.0;
  for (int s = 0; s < cs->n_seg; ++s) {
    tci::SegParams m, p;
    m.a = cs->ms2_start[s];
    m.e = cs->ms2_end[s];
    m.phi = cs->ms2_loopn[s] / 24;  // GetFluorFromPolPos.m:48
    m.k = m.phi / (m.e - m.a);
    m.ka = m.k * m.a;
    p.a = cs->pp7_start[s];
    p.e = cs->pp7_end[s];
    p.phi = cs->pp7_loopn[s] / 24;  // GetFluorFromPolPos.m:60
    p.k = p.phi / (p.e - p.a);
    p.ka = p.k * p.a;
    kp->ms2[s] = m;
    kp->pp7[s] = p;
    emax = std::max(emax, std::max(m.e, p.e));
  }
  kp->emax = emax;
}

// Rows per lane of the register-resident kernel, or 0 for the long-cell kernel (N > 513).
int pick_rpl(int64_t max_points) {
  const int64_t steps = max_points - 1;
  for (int r : {1, 2, 4, 8})
    if (64 * r >= steps) return r;
  return 0;
}

int run(tci_ctx* ctx, int mode, const double* theta, int64_t ld, const int32_t* cell, const uint8_t* active,
        int64_t B, double* out0, double* out1, int64_t ld_out, void* stream) {
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  // every cell has >= 2 points, so a row needs >= 9 entries; the kernels read theta[0..6] of a row
  // before they know its cell (tci_kernels.hip)
  if (B > 0 && ld < 9) return fail(ctx, TCI_ERANGE, "ld_theta=" + std::to_string(ld) + " < 9 (7 + at least 2 rates)");
  const int rc = tci::launch(ctx->kp, ctx->rpl, mode, theta, ld, cell, active, B, out0, out1, ld_out, stream);
  if (rc != TCI_OK) {
    if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "kernel launch");
    return fail(ctx, rc, "kernel launch rejected");
  }
  return TCI_OK;
}

// Host-side validation of a host-pointer batch (cell ids and row lengths).
int check_rows(tci_ctx* ctx, int64_t ld, const int32_t* cell, int64_t B) {
  for (int64_t b = 0; b < B; ++b) {
    const int32_t c = cell[b];
    if (c < 0 || c >= ctx->n_cells)
      return fail(ctx, TCI_ERANGE, "row " + std::to_string(b) + ": cell id " + std::to_string(c) + " out of range");
    if (ld < 7 + ctx->meta[(size_t)c].n)
      return fail(ctx, TCI_ERANGE, "row " + std::to_string(b) + ": theta needs " +
                                       std::to_string(7 + ctx->meta[(size_t)c].n) + " entries (ld_theta=" +
                                       std::to_string(ld) + ")");
  }
  return TCI_OK;
}

const double kP2P_ms2_start[1] = {0.024};
const double kP2P_ms2_end[1] = {1.299};
const double kP2P_ms2_loopn[1] = {24};
const double kP2P_pp7_start[1] = {4.292};
const double kP2P_pp7_end[1] = {5.758};
const double kP2P_pp7_loopn[1] = {24};

}  // namespace

namespace tci {

int ensure_dyn_lds(const void* func, size_t bytes) {
  if (bytes <= 48 * 1024) return TCI_OK;  // within the default limit
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TCI_EHIP;
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> set;  // per device and kernel
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = set[{dev, func}];
  if (bytes <= have) return TCI_OK;
  if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return TCI_EHIP;
  have = bytes;
  return TCI_OK;
}

}  // namespace tci

extern "C" {

const char* tci_version(void) { return kVersion; }

int tci_construct_by_name(const char* name, tci_construct* out) {
  if (!name || !out) return TCI_EINVAL;
  // GetFluorFromPolPos.m:18-28
  if (std::strcmp(name, "P2P-MS2v5-LacZ-PP7v4") == 0) {
    out->L0 = 6.626;
    out->n_seg = 1;
    out->ms2_start = kP2P_ms2_start;
    out->ms2_end = kP2P_ms2_end;
    out->ms2_loopn = kP2P_ms2_loopn;
    out->pp7_start = kP2P_pp7_start;
    out->pp7_end = kP2P_pp7_end;
    out->pp7_loopn = kP2P_pp7_loopn;
    return TCI_OK;
  }
  return TCI_EINVAL;
}

const char* tci_last_error(const tci_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int tci_create(const tci_cells* cells, const tci_construct* construct, int device, tci_ctx** out) {
  if (!out) return TCI_EINVAL;
  *out = nullptr;
  tci_ctx* ctx = new (std::nothrow) tci_ctx();
  if (!ctx) return TCI_ENOMEM;
  auto bail = [&](int rc) {
    *out = ctx;  // hand back the context so the caller can read tci_last_error, then destroy it
    return rc;
  };
  if (!cells || !cells->offsets || !cells->t || !cells->ms2 || !cells->pp7 || cells->n_cells <= 0)
    return bail(fail(ctx, TCI_EINVAL, "cells table is empty or has NULL arrays"));
  int rc = check_construct(ctx, construct);
  if (rc != TCI_OK) return bail(rc);
  ctx->device = device;
  ctx->n_cells = cells->n_cells;

  // ---- host precompute of the theta-independent per-cell tables
  const int64_t C = cells->n_cells;
  ctx->meta.resize((size_t)C);
  for (int64_t c = 0; c < C; ++c) {
    const int64_t n = cells->offsets[c + 1] - cells->offsets[c];
    if (n < 2) return bail(fail(ctx, TCI_EINVAL, "cell " + std::to_string(c) + " has fewer than 2 points"));
    if (n > TCI_MAX_POINTS)
      return bail(fail(ctx, TCI_EINVAL, "cell " + std::to_string(c) + " has " + std::to_string(n) +
                                            " points (max " + std::to_string(TCI_MAX_POINTS) + ")"));
    ctx->meta[(size_t)c] = CellMeta{(int32_t)n, 0, 0.0, 0.0, 0.0};
    ctx->max_points = std::max(ctx->max_points, n);
  }
  ctx->rpl = pick_rpl(ctx->max_points);
  // records per cell: every slot/point index a wave touches (the long-cell kernel reads < N)
  const int64_t stride = ctx->rpl > 0 ? 64 * (ctx->rpl + 1) : (ctx->max_points + 63) / 64 * 64;
  ctx->stride = stride;
  const size_t total = (size_t)C * (size_t)stride;
  // slots past a cell's last step: dt = 0 and t = -Inf, so every kernel skips them as steps before ton
  // (ConstantElongationSim.m:57-60) without a bounds test
  std::vector<tci::StepRec> steps(total, tci::StepRec{0.0, -INFINITY}), steps_raw(total, tci::StepRec{0.0, -INFINITY});
  std::vector<tci::PointRec> points(total, tci::PointRec{NAN, NAN, NAN, 0, 0});
  ctx->grid.assign(total, 0.0);
  for (int64_t c = 0; c < C; ++c) {
    const int64_t o = cells->offsets[c], n = ctx->meta[(size_t)c].n, base = c * stride;
    const double* t = cells->t + o;
    for (int64_t j = 0; j < n; ++j) {
      if (!std::isfinite(t[j]))
        return bail(fail(ctx, TCI_EINVAL, "cell " + std::to_string(c) + ": non-finite time"));
      if (j > 0 && !(t[j] > t[j - 1]))
        return bail(fail(ctx, TCI_EINVAL, "cell " + std::to_string(c) + ": times must be strictly increasing"));
    }
    double dgrid = 0.0;
    std::vector<double> g = interp_grid(t, n, &dgrid);  // SumofSquares...m:29-30
    if ((int64_t)g.size() != n)
      return bail(fail(ctx, TCI_EDIM, "cell " + std::to_string(c) + ": grid t(1):mean(diff(t)):t(end) has " +
                                          std::to_string(g.size()) + " points, data has " + std::to_string(n) +
                                          " (the reference errors: ConstantElongationSim.m:47)"));
    double delta = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      ctx->grid[(size_t)(base + i)] = g[(size_t)i];
      if (i + 1 < n) {
        const double dti = g[(size_t)i + 1] - g[(size_t)i];  // ConstantElongationSim.m:43-45
        steps[(size_t)(base + i)] = tci::StepRec{dti, g[(size_t)i]};
        steps_raw[(size_t)(base + i)] = tci::StepRec{t[i + 1] - t[i], t[i]};
        delta = std::max(delta, std::fabs(dti - dgrid));
      }
    }
    ctx->meta[(size_t)c].d = dgrid;
    ctx->meta[(size_t)c].delta = delta;
    // |p(r, r-m) - m*(v*d)| <= v * (m*delta + (m+4)*u*m*(d+delta)) for every distance m <= n-1
    // (tci_kernels.hip, fast path); doubled, plus 2^-40 relative for the rounding of v * eps_v.
    const double mx = (double)(n - 1);
    ctx->meta[(size_t)c].eps_v =
        2.0 * (mx * delta + (mx + 4.0) * 0x1p-53 * mx * (dgrid + delta)) * (1.0 + 0x1p-40);
    // interp1(t_interp, y, t): interval k = last grid point <= t_j (clamped to n-2);
    // outside [t_interp(1), t_interp(end)] -> NaN (w = NaN, k = 0).
    for (int64_t j = 0; j < n; ++j) {
      tci::PointRec& pr = points[(size_t)(base + j)];
      pr.y1 = cells->ms2[o + j];
      pr.y2 = cells->pp7[o + j];
      const double q = t[j];
      if (!(q >= g[0] && q <= g[(size_t)n - 1])) continue;
      int64_t k = (int64_t)(std::upper_bound(g.begin(), g.end(), q) - g.begin()) - 1;
      k = std::min(std::max(k, (int64_t)0), n - 2);
      pr.k = (int32_t)k;
      pr.w = (q - g[(size_t)k]) / (g[(size_t)k + 1] - g[(size_t)k]);
    }
  }

  // ---- upload: one resident allocation, 256-byte aligned sub-arrays
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t szM = al((size_t)C * sizeof(CellMeta)), szS = al(total * sizeof(tci::StepRec)),
               szP = al(total * sizeof(tci::PointRec));
  const size_t szT = al(64 * sizeof(double));
  const size_t bytes = szM + 2 * szS + szP + szT;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(hip_fail(ctx, e, "hipSetDevice"));
  e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return bail(hip_fail(ctx, e, "hipStreamCreate"));
  e = hipMalloc(&ctx->dbuf, bytes);
  if (e != hipSuccess) return bail(hip_fail(ctx, e, "hipMalloc(cell table)"));
  ctx->device_bytes = (int64_t)bytes;
  char* p = (char*)ctx->dbuf;
  auto put = [&](const void* src, size_t n, size_t span) -> void* {
    void* dst = p;
    p += span;
    if (hipMemcpy(dst, src, n, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return dst;
  };
  KParams& kp = ctx->kp;
  kp.cells = (const CellMeta*)put(ctx->meta.data(), (size_t)C * sizeof(CellMeta), szM);
  kp.steps = (const tci::StepRec*)put(steps.data(), total * sizeof(tci::StepRec), szS);
  kp.steps_raw = (const tci::StepRec*)put(steps_raw.data(), total * sizeof(tci::StepRec), szS);
  kp.points = (const tci::PointRec*)put(points.data(), total * sizeof(tci::PointRec), szP);
  double thr[64] = {0.0};
  for (int k = 0; k < construct->n_seg; ++k) {
    thr[1 + 4 * k] = construct->ms2_start[k];
    thr[2 + 4 * k] = construct->ms2_end[k];
    thr[3 + 4 * k] = construct->pp7_start[k];
    thr[4 + 4 * k] = construct->pp7_end[k];
  }
  kp.thr = (const double*)put(thr, sizeof(thr), szT);
  if (!kp.cells || !kp.steps || !kp.steps_raw || !kp.points || !kp.thr)
    return bail(fail(ctx, TCI_EHIP, "hipMemcpy(cell table) failed"));
  kp.cell_stride = stride;
  kp.max_n = ctx->max_points;
  kp.n_cells = C;
  kp.force_exact = 0;
  fill_segments(&kp, construct);
  *out = ctx;
  return TCI_OK;
}

int tci_destroy(tci_ctx* ctx) {
  if (!ctx) return TCI_EINVAL;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (void* q : {(void*)ctx->dbuf, (void*)ctx->d_theta, (void*)ctx->d_cell, (void*)ctx->d_active,
                  (void*)ctx->d_out0, (void*)ctx->d_out1, (void*)ctx->d_sim, (void*)ctx->d_cov})
    if (q) (void)hipFree(q);
  if (ctx->h_io) (void)hipHostFree(ctx->h_io);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return TCI_OK;
}

int tci_get_info(const tci_ctx* ctx, tci_info* out) {
  if (!ctx || !out) return TCI_EINVAL;
  out->device = ctx->device;
  out->rows_per_lane = ctx->rpl;
  out->n_cells = ctx->n_cells;
  out->max_points = ctx->max_points;
  out->device_bytes = ctx->device_bytes;
  return TCI_OK;
}

int tci_set_force_exact_scan(tci_ctx* ctx, int flags) {
  if (!ctx || flags < 0 || flags > 3) return TCI_EINVAL;
  ctx->kp.force_exact = flags;
  return TCI_OK;
}

int tci_ss_batch_async(tci_ctx* ctx, const double* d_theta, int64_t ld_theta, const int32_t* d_cell_id,
                       const uint8_t* d_active, int64_t B, double* d_ss_out, void* stream) {
  if (!ctx) return TCI_EINVAL;
  if (B < 0 || (B > 0 && (!d_theta || !d_cell_id || !d_ss_out)))
    return fail(ctx, TCI_EINVAL, "null device pointer or negative batch");
  return run(ctx, tci::MODE_SS, d_theta, ld_theta, d_cell_id, d_active, B, d_ss_out, nullptr, 0, stream);
}

int tci_ss_batch(tci_ctx* ctx, const double* theta, int64_t ld_theta, const int32_t* cell_id,
                 const uint8_t* active, int64_t B, double* ss_out) {
  if (!ctx) return TCI_EINVAL;
  if (B < 0 || (B > 0 && (!theta || !cell_id || !ss_out)))
    return fail(ctx, TCI_EINVAL, "null pointer or negative batch");
  if (B == 0) return TCI_OK;
  int rc = check_rows(ctx, ld_theta, cell_id, B);
  if (rc != TCI_OK) return rc;
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nth = (size_t)B * (size_t)ld_theta;
  // layout of the zero-copy buffer: theta | SS | cell ids | active flags (8-byte aligned blocks)
  const size_t o_ss = nth * 8, o_cell = o_ss + (size_t)B * 8, o_act = o_cell + ((size_t)B * 4 + 7) / 8 * 8;
  if (o_act + (size_t)B <= zero_copy_max()) {
    // a small batch (the drop-in tci_ssfun is B = 1): the kernel reads theta/ids/flags from pinned
    // host memory and writes the SS there; one launch and one synchronisation per call
    if ((rc = ensure_io(ctx, o_act + (size_t)B)) != TCI_OK) return rc;
    std::memcpy(ctx->h_io, theta, nth * 8);
    std::memcpy(ctx->h_io + o_cell, cell_id, (size_t)B * 4);
    if (active) std::memcpy(ctx->h_io + o_act, active, (size_t)B);
    rc = run(ctx, tci::MODE_SS, (const double*)ctx->d_io, ld_theta, (const int32_t*)(ctx->d_io + o_cell),
             active ? (const uint8_t*)(ctx->d_io + o_act) : nullptr, B, (double*)(ctx->d_io + o_ss), nullptr, 0,
             (void*)ctx->stream);
    if (rc != TCI_OK) return rc;
    TCI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(ss_out, ctx->h_io + o_ss, (size_t)B * 8);
    return TCI_OK;
  }
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, nth)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, (size_t)B)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_active, &ctx->cap_active, (size_t)B)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, (size_t)B)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(ctx->d_theta, theta, nth * sizeof(double), hipMemcpyHostToDevice, st));
  TCI_HIP(ctx, hipMemcpyAsync(ctx->d_cell, cell_id, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (active)
    TCI_HIP(ctx, hipMemcpyAsync(ctx->d_active, active, (size_t)B, hipMemcpyHostToDevice, st));
  rc = run(ctx, tci::MODE_SS, ctx->d_theta, ld_theta, ctx->d_cell, active ? ctx->d_active : nullptr, B, ctx->d_out0,
           nullptr, 0, (void*)st);
  if (rc != TCI_OK) return rc;
  TCI_HIP(ctx, hipMemcpyAsync(ss_out, ctx->d_out0, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  TCI_HIP(ctx, hipStreamSynchronize(st));
  return TCI_OK;
}

int tci_ssfun(tci_ctx* ctx, int32_t cell, const double* theta, int64_t P, double* ss_out) {
  if (!ctx) return TCI_EINVAL;
  return tci_ss_batch(ctx, theta, P, &cell, nullptr, 1, ss_out);
}

int tci_forward(tci_ctx* ctx, const double* theta, int64_t ld_theta, const int32_t* cell_id, int64_t B,
                int grid_mode, double* ms2_out, double* pp7_out, int64_t ld_out) {
  if (!ctx) return TCI_EINVAL;
  if (grid_mode != TCI_GRID_INTERP && grid_mode != TCI_GRID_RAW)
    return fail(ctx, TCI_EINVAL, "grid_mode must be TCI_GRID_INTERP or TCI_GRID_RAW");
  if (B < 0 || (B > 0 && (!theta || !cell_id || !ms2_out || !pp7_out)))
    return fail(ctx, TCI_EINVAL, "null pointer or negative batch");
  if (B == 0) return TCI_OK;
  int rc = check_rows(ctx, ld_theta, cell_id, B);
  if (rc != TCI_OK) return rc;
  for (int64_t b = 0; b < B; ++b)
    if (ld_out < ctx->meta[(size_t)cell_id[b]].n) return fail(ctx, TCI_ERANGE, "ld_out shorter than a cell");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nth = (size_t)B * (size_t)ld_theta, nout = (size_t)B * (size_t)ld_out;
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, nth)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, (size_t)B)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, nout)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out1, &ctx->cap_out1, nout)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(ctx->d_theta, theta, nth * sizeof(double), hipMemcpyHostToDevice, st));
  TCI_HIP(ctx, hipMemcpyAsync(ctx->d_cell, cell_id, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  // a row's kernel writes its N values only and whole rows are copied back: without this the entries
  // past N came back as whatever the scratch buffers held (earlier rows, SS values). All-ones is a NaN.
  TCI_HIP(ctx, hipMemsetAsync(ctx->d_out0, 0xFF, nout * sizeof(double), st));
  TCI_HIP(ctx, hipMemsetAsync(ctx->d_out1, 0xFF, nout * sizeof(double), st));
  rc = run(ctx, grid_mode == TCI_GRID_RAW ? tci::MODE_FWD_RAW : tci::MODE_FWD_INTERP, ctx->d_theta, ld_theta,
           ctx->d_cell, nullptr, B, ctx->d_out0, ctx->d_out1, ld_out, (void*)st);
  if (rc != TCI_OK) return rc;
  TCI_HIP(ctx, hipMemcpyAsync(ms2_out, ctx->d_out0, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  TCI_HIP(ctx, hipMemcpyAsync(pp7_out, ctx->d_out1, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  TCI_HIP(ctx, hipStreamSynchronize(st));
  return TCI_OK;
}

int tci_predict_defaults(tci_predict_options* o) {
  if (!o) return TCI_EINVAL;
  o->grid_mode = TCI_GRID_RAW;  // the plot call's grid (TranscriptionCycleMCMC.m:307-309)
  o->scratch_bytes = 0;
  return TCI_OK;
}

int tci_predict(tci_ctx* ctx, const tci_predict_options* opt, const double* theta, int64_t ld_theta,
                const int32_t* cell_id, int64_t n_sel, int64_t S, const double* probs, int32_t nq, double* ms2_q,
                double* pp7_q, int64_t ld_out) {
  if (!ctx) return TCI_EINVAL;
  tci_predict_options o;
  tci_predict_defaults(&o);
  if (opt) o = *opt;
  // ---- every check comes before any device work
  if (o.grid_mode != TCI_GRID_INTERP && o.grid_mode != TCI_GRID_RAW)
    return fail(ctx, TCI_EINVAL, "tci_predict: grid_mode must be TCI_GRID_INTERP or TCI_GRID_RAW");
  if (o.scratch_bytes < 0) return fail(ctx, TCI_EINVAL, "tci_predict: scratch_bytes must be >= 0");
  if (S < 1 || S > 4096) return fail(ctx, TCI_EINVAL, "tci_predict: S=" + std::to_string(S) + " must be in [1, 4096]");
  if (nq < 1 || nq > 16) return fail(ctx, TCI_EINVAL, "tci_predict: nq=" + std::to_string(nq) + " must be in [1, 16]");
  if (!probs) return fail(ctx, TCI_EINVAL, "tci_predict: probs is NULL");
  for (int32_t q = 0; q < nq; ++q)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
      return fail(ctx, TCI_EINVAL, "tci_predict: probs[" + std::to_string(q) + "] must be finite and in [0, 1]");
  if (n_sel < 0 || (n_sel > 0 && (!theta || !cell_id || !ms2_q || !pp7_q)))
    return fail(ctx, TCI_EINVAL, "tci_predict: null pointer or negative n_sel");
  if (n_sel == 0) return TCI_OK;
  int rc = check_rows(ctx, ld_theta, cell_id, n_sel);
  if (rc != TCI_OK) return rc;
  for (int64_t k = 0; k < n_sel; ++k)
    if (ld_out < ctx->meta[(size_t)cell_id[k]].n) return fail(ctx, TCI_ERANGE, "tci_predict: ld_out shorter than a cell");
  if (ld_theta > ((int64_t)1 << 24) || ld_out > ((int64_t)1 << 24))
    return fail(ctx, TCI_ERANGE, "tci_predict: ld_theta / ld_out above 2^24");
  const int64_t cap = o.scratch_bytes > 0 ? o.scratch_bytes : (int64_t)1 << 30;
  const int64_t per_cell = 2 * S * ld_out * (int64_t)sizeof(double);  // <= 2^41
  if (per_cell > cap)
    return fail(ctx, TCI_EINVAL, "tci_predict: one cell needs " + std::to_string(per_cell) +
                                     " bytes of scratch (2 x S x ld_out doubles), scratch_bytes allows " +
                                     std::to_string(cap));
  int64_t chunk = 0;
  if (tci::quantile_max_cells(S, ld_out, &chunk) != TCI_OK)
    return fail(ctx, TCI_EINVAL, "tci_predict: S x ld_out too large for one launch");
  chunk = std::min(std::min(chunk, cap / per_cell), n_sel);  // whole cells per chunk, at least one
  std::vector<int32_t> row_cell;
  try {
    row_cell.resize((size_t)(chunk * S));
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_predict: host allocation failed");
  }

  // ---- device work: per chunk, the forward launch into the scratch, then the quantile reduction
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  const size_t rows_max = (size_t)(chunk * S), nsim = rows_max * (size_t)ld_out;
  const size_t nqo_max = (size_t)chunk * (size_t)nq * (size_t)ld_out;
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, rows_max * (size_t)ld_theta)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, rows_max)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_sim, &ctx->cap_sim, 2 * nsim)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, nqo_max)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out1, &ctx->cap_out1, nqo_max)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  const int mode = o.grid_mode == TCI_GRID_RAW ? tci::MODE_FWD_RAW : tci::MODE_FWD_INTERP;
  for (int64_t k0 = 0; k0 < n_sel; k0 += chunk) {
    const int64_t nc = std::min(chunk, n_sel - k0), B = nc * S;
    for (int64_t k = 0; k < nc; ++k) std::fill_n(row_cell.begin() + k * S, S, cell_id[k0 + k]);
    const size_t nqo = (size_t)nc * (size_t)nq * (size_t)ld_out;
    double* sim0 = ctx->d_sim;
    double* sim1 = ctx->d_sim + (size_t)B * (size_t)ld_out;
    TCI_HIP(ctx, hipMemcpyAsync(ctx->d_theta, theta + (size_t)k0 * (size_t)S * (size_t)ld_theta,
                                (size_t)B * (size_t)ld_theta * sizeof(double), hipMemcpyHostToDevice, st));
    TCI_HIP(ctx, hipMemcpyAsync(ctx->d_cell, row_cell.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = run(ctx, mode, ctx->d_theta, ld_theta, ctx->d_cell, nullptr, B, sim0, sim1, ld_out, (void*)st)) != TCI_OK)
      return rc;
    rc = tci::launch_quantile(ctx->kp, ctx->d_cell, sim0, sim1, nc, S, ld_out, probs, nq, ctx->d_out0, ctx->d_out1,
                              (void*)st);
    if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "tci_predict: quantile kernel launch");
    if (rc != TCI_OK) return fail(ctx, rc, "tci_predict: the quantile kernel's tile does not fit a CU's LDS or the grid");
    const size_t oo = (size_t)k0 * (size_t)nq * (size_t)ld_out;
    TCI_HIP(ctx, hipMemcpyAsync(ms2_q + oo, ctx->d_out0, nqo * sizeof(double), hipMemcpyDeviceToHost, st));
    TCI_HIP(ctx, hipMemcpyAsync(pp7_q + oo, ctx->d_out1, nqo * sizeof(double), hipMemcpyDeviceToHost, st));
    TCI_HIP(ctx, hipStreamSynchronize(st));  // row_cell and the staging buffers are reused by the next chunk
  }
  return TCI_OK;
}

int tci_fitcheck_defaults(tci_fitcheck_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->scratch_bytes = 0;
  o->n_levels = 2;
  o->levels[0] = 0.5;
  o->levels[1] = 0.95;
  return TCI_OK;
}

namespace {

// The per-cell values of one cell from its pointwise vectors pt = [2][6][ld_out] (include/tci.h: dye 0 ascending j,
// then dye 1, over scored points; an unscored point is NaN in all six).
void fitcheck_cell(const double* pt, int64_t ld_out, const tci_fitcheck_options& o, int64_t k, tci_fitcheck_outputs* out) {
  const double nan = std::nan("");
  int32_t n_obs = 0;
  int32_t inside[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double lppd = 0.0, pw = 0.0, z2 = 0.0, dw[2];
  for (int d = 0; d < 2; ++d) {
    const double* v = pt + (size_t)d * 6 * (size_t)ld_out;
    const double *v_lppd = v, *v_pw = v + ld_out, *v_pit = v + 2 * ld_out, *v_zbar = v + 4 * ld_out, *v_z2 = v + 5 * ld_out;
    double num = 0.0, den = 0.0;
    bool prev = false;
    for (int64_t j = 0; j < ld_out; ++j) {
      const bool scored = !std::isnan(v_pit[j]);  // pit of a scored point is a sum of values in [0, 1]
      if (scored) {
        ++n_obs;
        lppd = lppd + v_lppd[j];
        pw = pw + v_pw[j];
        z2 = z2 + v_z2[j];
        for (int32_t l = 0; l < o.n_levels; ++l) {
          const double lo = (1.0 - o.levels[l]) / 2.0, hi = 1.0 - lo;
          if (lo <= v_pit[j] && v_pit[j] <= hi) ++inside[l];
        }
        if (prev) {
          const double dz = v_zbar[j] - v_zbar[j - 1];
          num = num + dz * dz;
        }
        den = den + v_zbar[j] * v_zbar[j];
      }
      prev = scored;
    }
    dw[d] = num / den;
  }
  const bool any = n_obs > 0;
  if (out->n_obs) out->n_obs[k] = n_obs;
  if (out->lppd) out->lppd[k] = any ? lppd : nan;
  if (out->p_waic) out->p_waic[k] = any ? pw : nan;
  if (out->elpd_waic) out->elpd_waic[k] = any ? lppd - pw : nan;
  if (out->chi2) out->chi2[k] = any ? z2 / (double)n_obs : nan;
  if (out->coverage)
    for (int32_t l = 0; l < o.n_levels; ++l)
      out->coverage[(size_t)k * (size_t)o.n_levels + l] = any ? (double)inside[l] / (double)n_obs : nan;
  if (out->dw)
    for (int d = 0; d < 2; ++d) out->dw[2 * k + d] = any ? dw[d] : nan;
}

}  // namespace

int tci_fitcheck(tci_ctx* ctx, const tci_fitcheck_options* opt, const double* theta, int64_t ld_theta, const double* s2,
                 const int32_t* cell_id, int64_t n_sel, int64_t S, int64_t ld_out, tci_fitcheck_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  tci_fitcheck_options o;
  tci_fitcheck_defaults(&o);
  if (opt) o = *opt;
  // ---- every check comes before any device work
  if (!out) return fail(ctx, TCI_EINVAL, "tci_fitcheck: out is NULL");
  if (o.scratch_bytes < 0) return fail(ctx, TCI_EINVAL, "tci_fitcheck: scratch_bytes must be >= 0");
  if (o.n_levels < 1 || o.n_levels > 8)
    return fail(ctx, TCI_EINVAL, "tci_fitcheck: n_levels=" + std::to_string(o.n_levels) + " must be in [1, 8]");
  for (int32_t l = 0; l < o.n_levels; ++l)
    if (!(o.levels[l] > 0.0 && o.levels[l] < 1.0))
      return fail(ctx, TCI_EINVAL, "tci_fitcheck: levels[" + std::to_string(l) + "] must be strictly inside (0, 1)");
  if (S < 1 || S > 4096) return fail(ctx, TCI_EINVAL, "tci_fitcheck: S=" + std::to_string(S) + " must be in [1, 4096]");
  if (n_sel < 0 || (n_sel > 0 && (!theta || !s2 || !cell_id)))
    return fail(ctx, TCI_EINVAL, "tci_fitcheck: null pointer or negative n_sel");
  out->kernel_ms = 0.0;
  out->forward_ms = 0.0;
  if (n_sel == 0) return TCI_OK;
  int rc = check_rows(ctx, ld_theta, cell_id, n_sel);
  if (rc != TCI_OK) return rc;
  for (int64_t k = 0; k < n_sel; ++k)
    if (ld_out < ctx->meta[(size_t)cell_id[k]].n) return fail(ctx, TCI_ERANGE, "tci_fitcheck: ld_out shorter than a cell");
  if (ld_theta > ((int64_t)1 << 24) || ld_out > ((int64_t)1 << 24))
    return fail(ctx, TCI_ERANGE, "tci_fitcheck: ld_theta / ld_out above 2^24");
  if (n_sel > ((int64_t)1 << 40) / S) return fail(ctx, TCI_ERANGE, "tci_fitcheck: n_sel x S above 2^40");
  for (int64_t i = 0; i < n_sel * S; ++i)
    if (!(std::isfinite(s2[i]) && s2[i] > 0.0))
      return fail(ctx, TCI_EINVAL, "tci_fitcheck: s2[" + std::to_string(i) + "] must be finite and > 0");
  const int64_t cap = o.scratch_bytes > 0 ? o.scratch_bytes : (int64_t)1 << 30;
  const int64_t per_cell = 2 * S * ld_out * (int64_t)sizeof(double);  // <= 2^41
  if (per_cell > cap)
    return fail(ctx, TCI_EINVAL, "tci_fitcheck: one cell needs " + std::to_string(per_cell) +
                                     " bytes of scratch (2 x S x ld_out doubles), scratch_bytes allows " +
                                     std::to_string(cap));
  int64_t chunk = 0;
  if (tci::fitcheck_max_cells(S, ld_out, &chunk) != TCI_OK)
    return fail(ctx, TCI_EINVAL, "tci_fitcheck: S x ld_out too large for one launch");
  chunk = std::min(std::min(chunk, cap / per_cell), n_sel);  // whole cells per chunk, at least one
  const size_t rows_max = (size_t)(chunk * S), cell_out = (size_t)12 * (size_t)ld_out;
  std::vector<int32_t> row_cell;
  std::vector<double> sdlg, pt;
  try {
    row_cell.resize(rows_max);
    sdlg.resize(2 * rows_max);
    pt.resize((size_t)chunk * cell_out);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_fitcheck: host allocation failed");
  }
  const double logS = std::log((double)S);

  // ---- device work: per chunk, the forward launch into the scratch, then the reduction over the samples
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, rows_max * (size_t)ld_theta)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, rows_max)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_sim, &ctx->cap_sim, 2 * rows_max * (size_t)ld_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, (size_t)chunk * cell_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out1, &ctx->cap_out1, 2 * rows_max)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) {
    const hipError_t e = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return hip_fail(ctx, e, "tci_fitcheck: hipEventCreate");
  }
  auto body = [&]() -> int {
    for (int64_t k0 = 0; k0 < n_sel; k0 += chunk) {
      const int64_t nc = std::min(chunk, n_sel - k0), B = nc * S;
      for (int64_t k = 0; k < nc; ++k) std::fill_n(row_cell.begin() + k * S, S, cell_id[k0 + k]);
      for (int64_t i = 0; i < B; ++i) {
        const double v = s2[k0 * S + i];
        sdlg[(size_t)i] = std::sqrt(v);
        sdlg[(size_t)(B + i)] = std::log(6.283185307179586 * v);
      }
      double* sim0 = ctx->d_sim;
      double* sim1 = ctx->d_sim + (size_t)B * (size_t)ld_out;
      double* d_sd = ctx->d_out1;
      double* d_lg = ctx->d_out1 + B;
      TCI_HIP(ctx, hipMemcpyAsync(ctx->d_theta, theta + (size_t)k0 * (size_t)S * (size_t)ld_theta,
                                  (size_t)B * (size_t)ld_theta * sizeof(double), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipMemcpyAsync(ctx->d_cell, row_cell.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipMemcpyAsync(d_sd, sdlg.data(), 2 * (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipEventRecord(e0, st));
      int r = run(ctx, tci::MODE_FWD_INTERP, ctx->d_theta, ld_theta, ctx->d_cell, nullptr, B, sim0, sim1, ld_out, (void*)st);
      if (r != TCI_OK) return r;
      TCI_HIP(ctx, hipEventRecord(e1, st));
      r = tci::launch_fitcheck(ctx->kp, ctx->d_cell, sim0, sim1, d_sd, d_lg, nc, S, ld_out, logS, ctx->d_out0, (void*)st);
      if (r == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "tci_fitcheck: kernel launch");
      if (r != TCI_OK) return fail(ctx, r, "tci_fitcheck: the kernel does not fit a CU's LDS or the grid");
      TCI_HIP(ctx, hipEventRecord(e2, st));
      TCI_HIP(ctx, hipMemcpyAsync(pt.data(), ctx->d_out0, (size_t)nc * cell_out * sizeof(double), hipMemcpyDeviceToHost, st));
      TCI_HIP(ctx, hipStreamSynchronize(st));  // the host vectors and the staging buffers are reused by the next chunk
      float ms = 0.f;
      TCI_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
      out->forward_ms += (double)ms;
      TCI_HIP(ctx, hipEventElapsedTime(&ms, e1, e2));
      out->kernel_ms += (double)ms;
      for (int64_t k = 0; k < nc; ++k) {
        const double* p = pt.data() + (size_t)k * cell_out;
        double* const dst[6] = {out->lppd_i, out->p_waic_i, out->pit, out->resid, out->zbar, out->z2};
        for (int q = 0; q < 6; ++q)
          if (dst[q])
            for (int d = 0; d < 2; ++d)
              std::memcpy(dst[q] + ((size_t)(k0 + k) * 2 + d) * (size_t)ld_out, p + ((size_t)d * 6 + q) * (size_t)ld_out,
                          (size_t)ld_out * sizeof(double));
        fitcheck_cell(p, ld_out, o, k0 + k, out);
      }
    }
    return TCI_OK;
  };
  rc = body();
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  return rc;
}

int tci_loocheck_defaults(tci_loocheck_options* o) {
  if (!o) return TCI_EINVAL;
  std::memset(o, 0, sizeof(*o));
  o->scratch_bytes = 0;
  o->n_groups = 0;
  o->khat_threshold = 0.0;
  o->max_iter = 5000;
  o->tol = 1e-12;
  return TCI_OK;
}

namespace {

// The per-chain values of one chain from its pointwise vectors pt = [2][4][ld_out] = per dye elpd_loo, lppd, p_loo,
// khat (include/tci.h: dye 0 ascending j, then dye 1, over scored points; an unscored point is NaN in all four).
void loocheck_chain(const double* pt, int64_t ld_out, double thr, int64_t k, tci_loocheck_outputs* out) {
  const double nan = std::nan("");
  int32_t n_obs = 0, n_bad = 0;
  double elpd = 0.0, ploo = 0.0, lppd = 0.0, kmax = -INFINITY;
  for (int d = 0; d < 2; ++d) {
    const double* v = pt + (size_t)d * 4 * (size_t)ld_out;
    for (int64_t j = 0; j < ld_out; ++j) {
      if (std::isnan(v[3 * ld_out + j])) continue;  // khat of a scored point is a number or +Inf
      ++n_obs;
      elpd = elpd + v[j];
      lppd = lppd + v[ld_out + j];
      ploo = ploo + v[2 * ld_out + j];
      const double kh = v[3 * ld_out + j];
      kmax = kh > kmax ? kh : kmax;
      if (kh > thr) ++n_bad;
    }
  }
  const bool any = n_obs > 0;
  if (out->n_obs) out->n_obs[k] = n_obs;
  if (out->elpd_loo) out->elpd_loo[k] = any ? elpd : nan;
  if (out->p_loo) out->p_loo[k] = any ? ploo : nan;
  if (out->lppd) out->lppd[k] = any ? lppd : nan;
  if (out->khat_max) out->khat_max[k] = any ? kmax : nan;
  if (out->n_khat_bad) out->n_khat_bad[k] = n_bad;
}

// The stacking weights of one group (include/tci.h): e[c] = the chain's pointwise elpd_loo, len values each.
void loocheck_stack(const std::vector<const double*>& e, size_t len, int64_t max_iter, double tol, std::vector<double>* w,
                    double* elpd_stack, int32_t* n_points, int32_t* n_iter) {
  const size_t C = e.size();
  const double nan = std::nan("");
  std::vector<double> E, mi;  // exp(e_ic - m_i), [n][C], and m_i
  for (size_t i = 0; i < len; ++i) {
    bool all = true;
    double m = -INFINITY;
    for (size_t c = 0; c < C; ++c) {
      all = all && std::isfinite(e[c][i]);
      m = e[c][i] > m ? e[c][i] : m;
    }
    if (!all) continue;
    mi.push_back(m);
    for (size_t c = 0; c < C; ++c) E.push_back(std::exp(e[c][i] - m));
  }
  const size_t n = mi.size();
  *n_points = (int32_t)n;
  *n_iter = 0;
  w->assign(C, nan);
  *elpd_stack = nan;
  if (C == 0 || n == 0) return;
  const double dn = (double)n;
  std::vector<double> a(C), num(C);
  std::fill(w->begin(), w->end(), 1.0 / (double)C);
  if (C == 1) (*w)[0] = 1.0;
  for (int64_t it = 1; C > 1 && it <= max_iter; ++it) {
    std::fill(num.begin(), num.end(), 0.0);
    for (size_t i = 0; i < n; ++i) {
      double den = 0.0;
      for (size_t c = 0; c < C; ++c) {
        a[c] = (*w)[c] * E[i * C + c];
        den = den + a[c];
      }
      for (size_t c = 0; c < C; ++c) num[c] = num[c] + a[c] / den;
    }
    double delta = 0.0;
    for (size_t c = 0; c < C; ++c) {
      const double wn = num[c] / dn, dw = std::fabs(wn - (*w)[c]);
      delta = dw > delta ? dw : delta;
      (*w)[c] = wn;
    }
    *n_iter = (int32_t)it;
    if (delta <= tol) break;
  }
  double tot = 0.0;
  for (size_t i = 0; i < n; ++i) {
    double den = 0.0;
    for (size_t c = 0; c < C; ++c) den = den + (*w)[c] * E[i * C + c];
    tot = tot + (mi[i] + std::log(den));
  }
  *elpd_stack = tot;
}

}  // namespace

int tci_loocheck(tci_ctx* ctx, const tci_loocheck_options* opt, const double* theta, int64_t ld_theta, const double* s2,
                 const int32_t* cell_id, const int32_t* group, int64_t n_sel, int64_t S, int64_t ld_out,
                 tci_loocheck_outputs* out) {
  if (!ctx) return TCI_EINVAL;
  tci_loocheck_options o;
  tci_loocheck_defaults(&o);
  if (opt) o = *opt;
  // ---- every check comes before any device work
  if (!out) return fail(ctx, TCI_EINVAL, "tci_loocheck: out is NULL");
  if (o.scratch_bytes < 0) return fail(ctx, TCI_EINVAL, "tci_loocheck: scratch_bytes must be >= 0");
  if (o.n_groups < 0 || o.n_groups > ((int64_t)1 << 31) - 1)
    return fail(ctx, TCI_EINVAL, "tci_loocheck: n_groups must be in [0, 2^31)");
  if (o.max_iter < 1) return fail(ctx, TCI_EINVAL, "tci_loocheck: max_iter must be >= 1");
  if (!(std::isfinite(o.tol) && o.tol >= 0.0)) return fail(ctx, TCI_EINVAL, "tci_loocheck: tol must be finite and >= 0");
  if (!(std::isfinite(o.khat_threshold) && o.khat_threshold >= 0.0))
    return fail(ctx, TCI_EINVAL, "tci_loocheck: khat_threshold must be finite and >= 0 (0 = the default)");
  if (S < 32 || S > 4096) return fail(ctx, TCI_EINVAL, "tci_loocheck: S=" + std::to_string(S) + " must be in [32, 4096]");
  if (n_sel < 0 || (n_sel > 0 && (!theta || !s2 || !cell_id)))
    return fail(ctx, TCI_EINVAL, "tci_loocheck: null pointer or negative n_sel");
  const double thr = o.khat_threshold > 0.0 ? o.khat_threshold : std::min(1.0 - 1.0 / std::log10((double)S), 0.7);
  int rc = TCI_OK;
  if (n_sel > 0) {
    rc = check_rows(ctx, ld_theta, cell_id, n_sel);
    if (rc != TCI_OK) return rc;
    for (int64_t k = 0; k < n_sel; ++k)
      if (ld_out < ctx->meta[(size_t)cell_id[k]].n) return fail(ctx, TCI_ERANGE, "tci_loocheck: ld_out shorter than a cell");
    if (ld_theta > ((int64_t)1 << 24) || ld_out > ((int64_t)1 << 24))
      return fail(ctx, TCI_ERANGE, "tci_loocheck: ld_theta / ld_out above 2^24");
    if (n_sel > ((int64_t)1 << 40) / S) return fail(ctx, TCI_ERANGE, "tci_loocheck: n_sel x S above 2^40");
    for (int64_t i = 0; i < n_sel * S; ++i)
      if (!(std::isfinite(s2[i]) && s2[i] > 0.0))
        return fail(ctx, TCI_EINVAL, "tci_loocheck: s2[" + std::to_string(i) + "] must be finite and > 0");
  }
  // the chains of every group, in the order given
  std::vector<std::vector<int64_t>> members;
  bool grouped = false;
  try {
    members.resize((size_t)o.n_groups);
    for (int64_t k = 0; group && k < n_sel; ++k) {
      if (group[k] < -1 || group[k] >= o.n_groups)
        return fail(ctx, TCI_ERANGE, "tci_loocheck: group[" + std::to_string(k) + "] = " + std::to_string(group[k]) +
                                         " outside [-1, n_groups)");
      if (group[k] < 0) continue;
      std::vector<int64_t>& mem = members[(size_t)group[k]];
      if (!mem.empty() && cell_id[mem[0]] != cell_id[k])
        return fail(ctx, TCI_EINVAL, "tci_loocheck: group " + std::to_string(group[k]) + " selects cells " +
                                         std::to_string(cell_id[mem[0]]) + " and " + std::to_string(cell_id[k]) +
                                         " (chain " + std::to_string(k) + "): the chains of a group select one cell");
      mem.push_back(k);
      grouped = true;
    }
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_loocheck: host allocation failed");
  }
  const int64_t cap = o.scratch_bytes > 0 ? o.scratch_bytes : (int64_t)1 << 30;
  const int64_t per_cell = 2 * S * ld_out * (int64_t)sizeof(double);  // <= 2^41
  if (n_sel > 0 && per_cell > cap)
    return fail(ctx, TCI_EINVAL, "tci_loocheck: one chain needs " + std::to_string(per_cell) +
                                     " bytes of scratch (2 x S x ld_out doubles), scratch_bytes allows " +
                                     std::to_string(cap));
  // the last check is passed: from here on out is written
  out->khat_threshold = thr;
  out->kernel_ms = 0.0;
  out->forward_ms = 0.0;
  const double nan = std::nan("");
  for (int64_t k = 0; out->weight && k < n_sel; ++k) out->weight[k] = nan;
  for (int64_t g = 0; g < o.n_groups; ++g) {
    if (out->elpd_stack) out->elpd_stack[g] = nan;
    if (out->n_points) out->n_points[g] = 0;
    if (out->n_iter) out->n_iter[g] = 0;
  }
  if (n_sel == 0) return TCI_OK;
  int64_t chunk = 0;
  if (tci::loocheck_max_cells(S, ld_out, &chunk) != TCI_OK)
    return fail(ctx, TCI_EINVAL, "tci_loocheck: S x ld_out too large for one launch");
  chunk = std::min(std::min(chunk, cap / per_cell), n_sel);  // whole chains per chunk, at least one
  const size_t rows_max = (size_t)(chunk * S), cell_out = (size_t)8 * (size_t)ld_out, len = 2 * (size_t)ld_out;
  std::vector<int32_t> row_cell;
  std::vector<double> sdlg, pt, elpd_all;
  try {
    row_cell.resize(rows_max);
    sdlg.resize(2 * rows_max);
    pt.resize((size_t)chunk * cell_out);
    if (grouped) elpd_all.resize((size_t)n_sel * len);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_loocheck: host allocation failed");
  }
  const double logS = std::log((double)S);

  // ---- device work: per chunk, the forward launch into the scratch, then the reduction over the samples
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, rows_max * (size_t)ld_theta)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, rows_max)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_sim, &ctx->cap_sim, 2 * rows_max * (size_t)ld_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, (size_t)chunk * cell_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out1, &ctx->cap_out1, 2 * rows_max)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) {
    const hipError_t e = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return hip_fail(ctx, e, "tci_loocheck: hipEventCreate");
  }
  auto body = [&]() -> int {
    for (int64_t k0 = 0; k0 < n_sel; k0 += chunk) {
      const int64_t nc = std::min(chunk, n_sel - k0), B = nc * S;
      for (int64_t k = 0; k < nc; ++k) std::fill_n(row_cell.begin() + k * S, S, cell_id[k0 + k]);
      for (int64_t i = 0; i < B; ++i) {
        const double v = s2[k0 * S + i];
        sdlg[(size_t)i] = std::sqrt(v);
        sdlg[(size_t)(B + i)] = std::log(6.283185307179586 * v);
      }
      double* sim0 = ctx->d_sim;
      double* sim1 = ctx->d_sim + (size_t)B * (size_t)ld_out;
      double* d_sd = ctx->d_out1;
      double* d_lg = ctx->d_out1 + B;
      TCI_HIP(ctx, hipMemcpyAsync(ctx->d_theta, theta + (size_t)k0 * (size_t)S * (size_t)ld_theta,
                                  (size_t)B * (size_t)ld_theta * sizeof(double), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipMemcpyAsync(ctx->d_cell, row_cell.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipMemcpyAsync(d_sd, sdlg.data(), 2 * (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
      TCI_HIP(ctx, hipEventRecord(e0, st));
      int r = run(ctx, tci::MODE_FWD_INTERP, ctx->d_theta, ld_theta, ctx->d_cell, nullptr, B, sim0, sim1, ld_out, (void*)st);
      if (r != TCI_OK) return r;
      TCI_HIP(ctx, hipEventRecord(e1, st));
      r = tci::launch_loocheck(ctx->kp, ctx->d_cell, sim0, sim1, d_sd, d_lg, nc, S, ld_out, logS, ctx->d_out0, (void*)st);
      if (r == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "tci_loocheck: kernel launch");
      if (r != TCI_OK) return fail(ctx, r, "tci_loocheck: the kernel does not fit a CU's LDS or the grid");
      TCI_HIP(ctx, hipEventRecord(e2, st));
      TCI_HIP(ctx, hipMemcpyAsync(pt.data(), ctx->d_out0, (size_t)nc * cell_out * sizeof(double), hipMemcpyDeviceToHost, st));
      TCI_HIP(ctx, hipStreamSynchronize(st));  // the host vectors and the staging buffers are reused by the next chunk
      float ms = 0.f;
      TCI_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
      out->forward_ms += (double)ms;
      TCI_HIP(ctx, hipEventElapsedTime(&ms, e1, e2));
      out->kernel_ms += (double)ms;
      for (int64_t k = 0; k < nc; ++k) {
        const double* p = pt.data() + (size_t)k * cell_out;
        double* const dst[4] = {out->elpd_loo_i, out->lppd_i, out->p_loo_i, out->khat_i};
        for (int q = 0; q < 4; ++q)
          if (dst[q])
            for (int d = 0; d < 2; ++d)
              std::memcpy(dst[q] + ((size_t)(k0 + k) * 2 + d) * (size_t)ld_out, p + ((size_t)d * 4 + q) * (size_t)ld_out,
                          (size_t)ld_out * sizeof(double));
        if (grouped)
          for (int d = 0; d < 2; ++d)
            std::memcpy(elpd_all.data() + ((size_t)(k0 + k) * 2 + d) * (size_t)ld_out, p + (size_t)d * 4 * (size_t)ld_out,
                        (size_t)ld_out * sizeof(double));
        loocheck_chain(p, ld_out, thr, k0 + k, out);
      }
    }
    return TCI_OK;
  };
  rc = body();
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  if (rc != TCI_OK) return rc;
  try {
    std::vector<const double*> e;
    std::vector<double> w;
    for (int64_t g = 0; g < o.n_groups; ++g) {
      const std::vector<int64_t>& mem = members[(size_t)g];
      if (mem.empty()) continue;
      e.clear();
      for (int64_t k : mem) e.push_back(elpd_all.data() + (size_t)k * len);
      double es = nan;
      int32_t np = 0, ni = 0;
      loocheck_stack(e, len, o.max_iter, o.tol, &w, &es, &np, &ni);
      for (size_t c = 0; out->weight && c < mem.size(); ++c) out->weight[mem[c]] = w[c];
      if (out->elpd_stack) out->elpd_stack[g] = es;
      if (out->n_points) out->n_points[g] = np;
      if (out->n_iter) out->n_iter[g] = ni;
    }
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_loocheck: host allocation failed");
  }
  return TCI_OK;
}

int tci_device_count(int* n_out) {
  if (!n_out) return TCI_EINVAL;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;  // hipErrorNoDevice: none visible
  *n_out = n;
  return TCI_OK;
}

int tci_cell_points(const tci_ctx* ctx, int32_t cell, int64_t* n_out) {
  if (!ctx || !n_out || cell < 0 || cell >= ctx->n_cells) return TCI_EINVAL;
  *n_out = ctx->meta[(size_t)cell].n;
  return TCI_OK;
}

int tci_cell_grid(const tci_ctx* ctx, int32_t cell, double* t_interp_out, int64_t cap, int64_t* m_out) {
  if (!ctx || cell < 0 || cell >= ctx->n_cells) return TCI_EINVAL;
  const CellMeta& m = ctx->meta[(size_t)cell];
  if (m_out) *m_out = m.n;
  if (!t_interp_out) return TCI_OK;
  if (cap < m.n) return TCI_ERANGE;
  std::memcpy(t_interp_out, ctx->grid.data() + (size_t)cell * (size_t)ctx->stride, (size_t)m.n * sizeof(double));
  return TCI_OK;
}

}  // extern "C"

namespace {

// Device allocations of one DRAM run, freed together.
struct DevAllocs {
  std::vector<void*> ptrs;
  ~DevAllocs() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* alloc(size_t n, hipError_t* err) {
    void* p = nullptr;
    *err = hipMalloc(&p, std::max(n, (size_t)1) * sizeof(T));
    if (*err == hipSuccess) ptrs.push_back(p);
    return (T*)p;
  }
};

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
  hipStream_t s = ctx->stream;
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  TCI_HIP(ctx, hipEventCreate(&ev1));
  TCI_HIP(ctx, hipEventRecord(ev0, s));
  const int rc = tci::launch_chainstats(d_chain, d_s2, n_rows, n_chains, ld, d_npar, max_lag, d_stats, d_win, (void*)s);
  hipError_t e1 = hipEventRecord(ev1, s);
  if (e1 == hipSuccess) e1 = hipMemcpyAsync(hs.data(), d_stats, 4 * plane * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess) e1 = hipMemcpyAsync(hw.data(), d_win, plane * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain statistics kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "chain statistics kernels");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain statistics copy");
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
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  e = hipEventCreate(&ev1);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return hip_fail(ctx, e, "hipEventCreate");
  }
  double total_ms = 0.0;
  hipError_t e1 = hipSuccess;
  rc = TCI_OK;
  for (int64_t c0 = 0; c0 < n_chains && rc == TCI_OK && e1 == hipSuccess; c0 += group) {
    const int64_t nc = std::min(group, n_chains - c0);
    double* d_cv = ctx->d_cov;
    double* d_cr = ctx->d_cov + (size_t)nc * L2;
    e1 = hipEventRecord(ev0, s);
    if (e1 != hipSuccess) break;
    rc = tci::launch_chaincov(d_chain, n_rows, n_chains, ld, d_npar, c0, nc, d_mean, d_cv, d_cr, (void*)s);
    e1 = hipEventRecord(ev1, s);
    const size_t o = (size_t)c0 * L2, nb = (size_t)nc * L2 * sizeof(double);
    if (rc == TCI_OK && e1 == hipSuccess && out->cov) e1 = hipMemcpyAsync(out->cov + o, d_cv, nb, hipMemcpyDeviceToHost, s);
    if (rc == TCI_OK && e1 == hipSuccess && out->corr) e1 = hipMemcpyAsync(out->corr + o, d_cr, nb, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // the scratch is reused by the next group
    if (e1 == hipSuccess) e1 = e2;
    float ms = 0.f;
    if (rc == TCI_OK && e1 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
    total_ms += ms;
  }
  if (rc == TCI_OK && e1 == hipSuccess && out->mean)
    e1 = hipMemcpy(out->mean, d_mean, (size_t)n_chains * L * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
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
  hipStream_t s = ctx->stream;
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  e = hipEventCreate(&ev1);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return hip_fail(ctx, e, "hipEventCreate");
  }
  hipError_t e1 = hipEventRecord(ev0, s);
  const int rc = tci::launch_chainquant(d_chain, d_s2, n_rows, n_chains, ld, d_npar, probs, nq, d_q, (void*)s);
  if (e1 == hipSuccess) e1 = hipEventRecord(ev1, s);
  if (rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(hq.data(), d_q, total * sizeof(double), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain quantile kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "chain quantile kernel");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain quantile copy");
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
  hipStream_t s = ctx->stream;
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  e = hipEventCreate(&ev1);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return hip_fail(ctx, e, "hipEventCreate");
  }
  hipError_t e1 = hipEventRecord(ev0, s);
  const int rc = tci::launch_chaindens(d_chain, d_s2, n_rows, n_chains, ld, d_npar, G, B, bw_scale,
                                       std::pow((double)n_rows, -0.2), d_scratch, d_d, d_c, (void*)s);
  if (e1 == hipSuccess) e1 = hipEventRecord(ev1, s);
  if (rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(hd.data(), d_d, nd * sizeof(double), hipMemcpyDeviceToHost, s);
  if (rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(hc.data(), d_c, nc * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "chain density kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "chain density kernels");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "chain density copy");
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
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  e = hipEventCreate(&ev1);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return hip_fail(ctx, e, "hipEventCreate");
  }
  hipError_t e1 = hipEventRecord(ev0, s);
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
  if (e1 == hipSuccess) e1 = hipEventRecord(ev1, s);
  auto copy = [&](void* dst, const void* src, size_t bytes) {
    if (dst && rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
  };
  copy(out->ss, d_ss, B * sizeof(double));
  copy(out->pri, d_pri, B * sizeof(double));
  copy(out->dev, d_dev, B * sizeof(double));
  copy(out->lp, d_lp, B * sizeof(double));
  copy(hs.data(), d_scal, (size_t)K * n * sizeof(double));
  copy(out->best_row, d_best, n * sizeof(int64_t));
  copy(out->theta_best, d_tb, n * L * sizeof(double));
  copy(out->theta_mean, d_tm, n * L * sizeof(double));
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), "log-posterior kernel launch");
  if (rc != TCI_OK) return fail(ctx, rc, std::string(who) + ": rows x chains x ld too large for one launch");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "log-posterior kernels");
  if (e1 != hipSuccess) return hip_fail(ctx, e1, "log-posterior copy");
  double* dst[tci::kChainlpScalars] = {out->ss_min,  out->ss_mean, out->dev_mean, out->dev_var, out->lp_best,
                                       out->ss_best, out->s2_best, out->s2_mean,  out->ss_hat,  out->d_hat,
                                       out->p_d,     out->p_v,     out->dic};
  for (int k = 0; k < K; ++k)
    if (dst[k]) std::memcpy(dst[k], hs.data() + (size_t)k * n, n * sizeof(double));
  out->n_rows = n_rows;
  out->kernel_ms = ms;
  return TCI_OK;
}

// The groups of a tci_chainrhat call, checked before any device work: group (null: every chain in group 0) as the
// per-chain vector the kernels skip by, and its CSR form (the chains of a group ascending). npar (host, may be null =
// ld): the chains of a group must have one npar.
struct RhatGroups {
  std::vector<int32_t> group, off, list;
  size_t scratch = 0;
};
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

// The group kernels on a device chain (launch_chainrhat), timed with HIP events, and their results scattered into
// the caller's host buffers (d_npar null: ld columns for every chain; d_s2 null: the s2 twins are NaN).
int chainrhat_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, const RhatGroups& G, int64_t n_groups,
                     tci_chainrhat_outputs* out, int64_t max_lag = 0, tci_chainess_outputs* eout = nullptr) {
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
      const int64_t h = n_rows / 2;
      for (size_t g = 0; g < ng; ++g) {  // cap = (m L) log10(m L): classic m = M, L = n; split m = 2 M, L = h
        const int64_t M = G.off[g + 1] - G.off[g];
        const double tc = (double)(M * n_rows), ts = (double)(2 * M * h);
        hcap[g] = tc > 0 ? tc * std::log10(tc) : 0.0;
        hcap[ng + g] = ts > 0 ? ts * std::log10(ts) : 0.0;
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, std::string(who) + ": host allocation failed");
  }
  hipStream_t s = ctx->stream;
  hipEvent_t ev0, ev1;
  TCI_HIP(ctx, hipEventCreate(&ev0));
  e = hipEventCreate(&ev1);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return hip_fail(ctx, e, "hipEventCreate");
  }
  // from here every path reaches the hipStreamSynchronize below: G's vectors outlive their uploads
  e = hipMemcpyAsync(d_group, G.group.data(), G.group.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, G.off.data(), G.off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_list, G.list.data(), G.list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && eout) e = hipMemcpyAsync(d_cap, hcap.data(), hcap.size() * sizeof(double), hipMemcpyHostToDevice, s);
  hipError_t e1 = e == hipSuccess ? hipEventRecord(ev0, s) : e;
  const int rc = e != hipSuccess ? TCI_OK
                 : eout ? tci::launch_chainess(d_chain, d_s2, n_rows, n_chains, ld, d_npar, d_group, n_groups, d_off,
                                               d_list, max_lag, d_cap, d_scratch, d_o, d_ed, d_ew, (void*)s)
                        : tci::launch_chainrhat(d_chain, d_s2, n_rows, n_chains, ld, d_npar, d_group, n_groups,
                                                d_off, d_list, d_scratch, d_o, (void*)s);
  if (e1 == hipSuccess) e1 = hipEventRecord(ev1, s);
  if (rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(ho.data(), d_o, 4 * plane * sizeof(double), hipMemcpyDeviceToHost, s);
  if (rc == TCI_OK && e1 == hipSuccess && eout) e1 = hipMemcpyAsync(he.data(), d_ed, 5 * plane * sizeof(double), hipMemcpyDeviceToHost, s);
  if (rc == TCI_OK && e1 == hipSuccess && eout) e1 = hipMemcpyAsync(hw.data(), d_ew, 2 * plane * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  float ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
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

// What tci_dram_run_rhat adds to a run: the groups of its chains and where the group reduction goes.
struct RhatAsk {
  const tci_chainrhat_options* ropt;
  const int32_t* group;
  int64_t n_groups;
  tci_chainrhat_outputs* rout;
  const char* who = "tci_dram_run_rhat";
  const tci_chainess_options* eopt = nullptr;  // tci_dram_run_ess: the effective sample size too (rout may be null)
  tci_chainess_outputs* eout = nullptr;
};

// One DRAM step: propose -> ssfun -> accept/propose stage 2 -> ssfun -> accept, sigma2, log the row
// -> [window records] -> [adapt] -> step + 1.
// What tci_dram_run_tempered adds to a run: the ladders and where the swap records go.
struct TemperAsk {
  const tci_temper_options* topt;
  tci_temper_outputs* tout;
};

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

}  // extern "C"

namespace {

// tci_dram_run, with the reductions of the kept rows that `red` asks for: red.sout the chain statistics
// (tci_dram_run_stats), red.cout their mean, covariance and correlation (tci_dram_run_cov), red.qout their
// quantiles and red.dout their densities and histograms (tci_dram_run_reduced); rhat: the reduction across the
// chains of every group over the same rows (tci_dram_run_rhat); lout: the log-posterior trace of the same rows
// (tci_dram_run_lp).
int dram_run_impl(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                  const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                  const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                  tci_dram_outputs* out, const tci_dram_reductions& red, const RhatAsk* rhat = nullptr,
                  const tci_chainlp_options* lopt = nullptr, tci_chainlp_outputs* lout = nullptr,
                  const TemperAsk* temper = nullptr) {
  if (!ctx) return TCI_EINVAL;
  const tci_chainstats_options* sopt = red.sopt;
  tci_chainstats_outputs* sout = red.sout;
  const tci_chaincov_options* copt = red.copt;
  tci_chaincov_outputs* cvout = red.cout;
  tci_chainquant_outputs* qout = red.qout;
  tci_chaindens_outputs* dout = red.dout;
  if (!opt || !out || n_chains <= 0 || !cell_id || !theta0 || !lower || !upper || !prior_mu || !prior_sig ||
      !qcov_diag || !sigma2_0)
    return fail(ctx, TCI_EINVAL, "tci_dram_run: null argument or no chains");
  if (opt->n_steps < 1 || opt->ntry < 1 || opt->ntry > 2 || opt->adaptint < 0 || !(opt->drscale > 0) ||
      opt->engine < TCI_DRAM_AUTO || opt->engine > TCI_DRAM_WALK || opt->max_chunk < 0 || opt->adapt_pmax < 0 ||
      opt->adapt_pmax > TCI_MAX_POINTS + 7)
    return fail(ctx, TCI_EINVAL,
                "tci_dram_run: bad options (n_steps >= 1, ntry in {1,2}, adaptint >= 0, engine in {0,1,2,3}, "
                "max_chunk >= 0, 0 <= adapt_pmax <= 2055)");
  // the statistics' rows: the kept rows k (chain row 1 + k * thin) from the first one at or past stats_from
  const int64_t max_lag = sopt ? sopt->max_lag : 0;
  int64_t stats_k0 = 0, stats_rows = 0;
  if (sout) {
    if (opt->thin <= 0)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: the statistics need the kept rows (thin >= 1)");
    if (max_lag < 0) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: max_lag must be >= 0");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    stats_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    stats_rows = (opt->n_steps + opt->thin - 1) / opt->thin - stats_k0;
    if (stats_rows < 1) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: no kept row at or past stats_from (n_rows < 1)");
  }
  int64_t cov_k0 = 0, cov_rows = 0, cov_group = 0;  // the matrices use the statistics' rows
  if (cvout) {
    if (opt->thin <= 0) return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: the matrices need the kept rows (thin >= 1)");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    cov_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    cov_rows = (opt->n_steps + opt->thin - 1) / opt->thin - cov_k0;
    if (cov_rows < 2)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: fewer than 2 kept rows at or past stats_from (n_rows < 2)");
    const int rcg = chaincov_group(ctx, "tci_dram_run_cov", copt, n_chains, ld, &cov_group);
    if (rcg != TCI_OK) return rcg;
  }
  int64_t q_k0 = 0, q_rows = 0;  // the quantiles use the statistics' rows too
  const double* q_probs = nullptr;
  int32_t q_nq = 0;
  if (qout) {
    if (opt->thin <= 0)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: the quantiles need the kept rows (thin >= 1)");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    q_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    q_rows = (opt->n_steps + opt->thin - 1) / opt->thin - q_k0;
    if (q_rows < 1)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: no kept row at or past stats_from (n_rows < 1)");
    const int rcq = chainquant_probs(ctx, "tci_dram_run_reduced", red.qopt, n_chains, ld, &q_probs, &q_nq);
    if (rcq != TCI_OK) return rcq;
  }
  int64_t d_k0 = 0, d_rows = 0;  // and so do the densities
  int32_t d_G = 0, d_B = 0;
  double d_bws = 0.0;
  size_t d_scratch = 0;
  if (dout) {
    if (opt->thin <= 0)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: the densities need the kept rows (thin >= 1)");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    d_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    d_rows = (opt->n_steps + opt->thin - 1) / opt->thin - d_k0;
    if (d_rows < 2)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: fewer than 2 kept rows at or past stats_from (n_rows < 2)");
    const int rcd = chaindens_opts(ctx, "tci_dram_run_reduced", red.dopt, d_rows, n_chains, ld, &d_G, &d_B, &d_bws, &d_scratch);
    if (rcd != TCI_OK) return rcd;
  }
  int64_t l_k0 = 0, l_rows = 0;  // and so does the log-posterior trace
  if (lout) {
    if (opt->thin <= 0)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: the log-posterior trace needs the kept rows (thin >= 1)");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    l_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    l_rows = (opt->n_steps + opt->thin - 1) / opt->thin - l_k0;
    if (l_rows < 1)
      return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: no kept row at or past stats_from (n_rows < 1)");
  }
  int64_t r_k0 = 0, r_rows = 0;  // and so does the group reduction
  if (rhat) {
    if (opt->thin <= 0)
      return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": the group reduction needs the kept rows (thin >= 1)");
    const int64_t from = std::max<int64_t>(opt->stats_from, 1);
    r_k0 = (from - 1 + opt->thin - 1) / opt->thin;
    r_rows = (opt->n_steps + opt->thin - 1) / opt->thin - r_k0;
    if (r_rows < 2)
      return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": fewer than 2 kept rows at or past stats_from (n_rows < 2)");
    if (rhat->eout && rhat->eopt && rhat->eopt->max_lag < 0)
      return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": max_lag must be >= 0");
    if (rhat->eout && rhat->eopt && rhat->eopt->flags != 0)
      return fail(ctx, TCI_EINVAL, std::string(rhat->who) + ": flags is reserved and must be 0");
  }
  int rc = check_rows(ctx, ld, cell_id, n_chains);
  if (rc != TCI_OK) return rc;
  if (ld > TCI_MAX_POINTS + 7) return fail(ctx, TCI_ERANGE, "tci_dram_run: ld too large");
  size_t l_scratch = 0;
  if (lout) {
    rc = chainlp_check(ctx, "tci_dram_run_lp", lopt, l_rows, n_chains, ld, cell_id, prior_mu, prior_sig, &l_scratch);
    if (rc != TCI_OK) return rc;
  }
  const size_t n = (size_t)n_chains, L = (size_t)ld, L2 = L * L;
  std::vector<int32_t> npar(n), nobs(n);
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
  // the ladders (tci_dram_run_tempered): each chain's Gibbs shape and stored sigma2, and the pairs of neighbouring rungs
  std::vector<double> gshape(n), s20(sigma2_0, sigma2_0 + n), beta(n, 1.0);
  for (size_t c = 0; c < n; ++c) gshape[c] = 0.5 * (double)nobs[c];
  std::vector<int32_t> pair_a, pair_b, pair_r;
  int64_t swap_every = 0;
  if (temper) {
    const tci_temper_options* t = temper->topt;
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
  RhatGroups r_groups;
  if (rhat) {
    rc = chainrhat_groups(ctx, rhat->who, rhat->ropt, r_rows, n_chains, ld, npar.data(), rhat->group,
                          rhat->n_groups, &r_groups);
    if (rc != TCI_OK) return rc;
  }
  // the P the adaptation kernel is picked for (> 208: k_adapt_gt and its tile grid): this run's largest,
  // or the whole fit's when this run is a shard of it (adapt_pmax)
  const int64_t p_max_all = std::max<int64_t>(*std::max_element(npar.begin(), npar.end()), opt->adapt_pmax);
  // limits of the adaptation window, checked before anything is allocated or launched: the
  // adaptation kernel's LDS (the window's run table grows with adaptint) and the chain kernels'
  // 32-bit window-log offsets (adaptint * ld)
  if (opt->adaptint > 0 && tci::dram_adapt_lds_bytes(p_max_all, opt->adaptint) > 160 * 1024)
    return fail(ctx, TCI_ERANGE, "tci_dram_run: adaptint " + std::to_string(opt->adaptint) +
                                     " needs more LDS than a CU has for the adaptation at P = " +
                                     std::to_string(p_max_all));
  if ((opt->adaptint > 0 ? opt->adaptint : 100) * ld >= (int64_t)INT32_MAX)
    return fail(ctx, TCI_ERANGE, "tci_dram_run: adaptint * ld must be < 2^31");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  tci::DramState st{};
  tci::DramParams p{};
  // Chunk of chain rows per fused-engine pass (its draws buffer holds one chunk; at most the next
  // adaptation row) and the window slots per chain: the covupd window (adaptint rows), which is also
  // every engine's per-row log.
  const int64_t ai = opt->adaptint;
  const int64_t DW = tci::draw_stride(ld);
  const int64_t chunk_cap =
      std::max<int64_t>(32, (int64_t)(((size_t)tci::kDrawsGiB << 30) / (n * (size_t)DW * sizeof(double))));
  // Without adaptation the window is 100 rows: the records' merge partition (the same for every engine)
  // and the batched engine's graph block stay small (a 1,000-row window made the batched engine run up
  // to 1,000 steps as plain launches before its first graph replay).
  const int64_t win = ai > 0 ? ai : 100;
  int64_t chunk = std::min<int64_t>(win, chunk_cap);
  if (opt->max_chunk > 0) chunk = std::min<int64_t>(chunk, opt->max_chunk);
  const int64_t n_keep = opt->thin > 0 ? (opt->n_steps + opt->thin - 1) / opt->thin : 0;
  st.n_chains = n_chains;
  st.ld = ld;
#define TCI_ALLOC(field, T, count)                                  \
  do {                                                              \
    st.field = A.alloc<T>((count), &e);                             \
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(dram " #field ")"); \
  } while (0)
  int32_t *d_cell, *d_npar, *d_nobs;
  double *d_lower, *d_upper, *d_pmu, *d_psig, *d_qdiag, *d_s20;
  d_cell = A.alloc<int32_t>(n, &e);
  int64_t* d_key = A.alloc<int64_t>(n, &e);
  d_npar = A.alloc<int32_t>(n, &e);
  d_nobs = A.alloc<int32_t>(n, &e);
  double* d_gshape = A.alloc<double>(n, &e);
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
  if (n_keep > 0 && (sout || cvout || qout || dout || lout || rhat) && !(out->chain || out->s2chain)) {
    // the chain is kept on the device for the statistics alone: running out of memory is the caller's to handle
    st.chain_out = A.alloc<double>((size_t)n_keep * n * L, &e);
    if (e == hipSuccess) st.s2_out = A.alloc<double>((size_t)n_keep * n, &e);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, TCI_ENOMEM, std::string(sout ? "tci_dram_run_stats" : cvout ? "tci_dram_run_cov" : rhat ? rhat->who : "tci_dram_run_reduced") +
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
  hipStream_t s = ctx->stream;
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
  tci::SwapArgs sw{};
  const tci::SwapArgs* swp = nullptr;
  const int64_t n_events = swap_every > 0 ? (opt->n_steps - 1) / win / swap_every : 0;
  const int64_t log_rows = temper && temper->tout && (temper->tout->swap_logr || temper->tout->swap_acc)
                               ? std::min<int64_t>(n_events, std::max<int64_t>(temper->tout->swap_log_rows, 0))
                               : 0;
  if (temper && !pair_a.empty() && n_events > 0) {
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
  hipEvent_t ev0, ev1;
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
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // WALK (one wavefront per chain) once k_chain's one-workgroup-per-chain layout would need more
  // than one round of resident workgroups (two chains per CU).
  int n_cu = 0;
  TCI_HIP(ctx, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  bool fused = opt->engine == TCI_DRAM_FUSED || opt->engine == TCI_DRAM_WALK;
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
  if (fused) {
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
    e = hipSuccess;
  } else {
  // The step loop. Steps 2 .. n_steps; adaptation after steps that are multiples of adaptint.
  // Blocks of adaptint steps (aligned so that each ends on an adaptation step) are captured once
  // as a hipGraph and replayed; the head (steps 2..adaptint) and the tail run as plain launches.
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
    hipError_t ce = hipStreamEndCapture(s, &graph);
    if (crc != TCI_OK || ce != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      return fail(ctx, TCI_EHIP, "DRAM step graph capture failed");
    }
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      (void)hipGraphDestroy(graph);
      return hip_fail(ctx, e, "hipGraphInstantiate");
    }
    for (int64_t b = 0; b < blocks && e == hipSuccess; ++b) e = hipGraphLaunch(exec, s);
    next += blocks * G;
  }
  if (e == hipSuccess) plain(opt->n_steps);  // tail
  }
  // the last, partial window's records (the fused engines: kept by the last chunk's kernel)
  if (e == hipSuccess && rc == TCI_OK && opt->n_steps % win != 0 && !(fused && opt->n_steps >= 2)) {
    const int64_t last = opt->n_steps;
    rc = hipMemcpyAsync(st.step, &last, sizeof(int64_t), hipMemcpyHostToDevice, s) == hipSuccess ? TCI_OK : TCI_EHIP;
    if (rc == TCI_OK) rc = tci::dram_launch_stats(st, p, s);
  }
  const hipError_t ge = e;
  TCI_HIP(ctx, hipEventRecord(ev1, s));
  TCI_HIP(ctx, hipStreamSynchronize(s));
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
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
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  out->elapsed_ms = ms;
  // ---- outputs
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
  if (temper && temper->tout) {
    tci_temper_outputs* to = temper->tout;
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
  if (sout) {  // the device chain's rows from the first one in the statistics range
    rc = chainstats_device(ctx, "tci_dram_run_stats", st.chain_out + (size_t)stats_k0 * n * L,
                           st.s2_out + (size_t)stats_k0 * n, stats_rows, n_chains, ld, st.npar, max_lag, sout);
    if (rc != TCI_OK) return rc;
  }
  if (cvout) {
    rc = chaincov_device(ctx, "tci_dram_run_cov", st.chain_out + (size_t)cov_k0 * n * L, cov_rows, n_chains, ld, st.npar,
                         cov_group, cvout);
    if (rc != TCI_OK) return rc;
  }
  if (qout) {
    rc = chainquant_device(ctx, "tci_dram_run_reduced", st.chain_out + (size_t)q_k0 * n * L,
                           st.s2_out + (size_t)q_k0 * n, q_rows, n_chains, ld, st.npar, q_probs, q_nq, qout);
    if (rc != TCI_OK) return rc;
  }
  if (dout) {
    rc = chaindens_device(ctx, "tci_dram_run_reduced", st.chain_out + (size_t)d_k0 * n * L,
                          st.s2_out + (size_t)d_k0 * n, d_rows, n_chains, ld, st.npar, d_G, d_B, d_bws, d_scratch, dout);
    if (rc != TCI_OK) return rc;
  }
  if (lout) {
    rc = chainlp_device(ctx, "tci_dram_run_lp", st.chain_out + (size_t)l_k0 * n * L, st.s2_out + (size_t)l_k0 * n,
                        l_rows, n_chains, ld, st.cell, st.npar, st.pmu, st.psig, l_scratch, lout);
    if (rc != TCI_OK) return rc;
  }
  if (rhat)
    return chainrhat_device(ctx, rhat->who, st.chain_out + (size_t)r_k0 * n * L,
                            st.s2_out + (size_t)r_k0 * n, r_rows, n_chains, ld, st.npar, r_groups, rhat->n_groups,
                            rhat->rout, rhat->eout && rhat->eopt ? rhat->eopt->max_lag : 0, rhat->eout);
  return TCI_OK;
}

}  // namespace

extern "C" {

int tci_dram_run(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                 const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                 const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                 tci_dram_outputs* out) {
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, tci_dram_reductions{});
}

int tci_dram_run_stats(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                       const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                       const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                       tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout) {
  if (!ctx) return TCI_EINVAL;
  if (!sout) return fail(ctx, TCI_EINVAL, "tci_dram_run_stats: null statistics outputs");
  tci_dram_reductions red{};
  red.sopt = sopt;
  red.sout = sout;
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red);
}

int tci_dram_run_cov(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                     const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                     const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                     tci_dram_outputs* out, const tci_chainstats_options* sopt, tci_chainstats_outputs* sout,
                     const tci_chaincov_options* copt, tci_chaincov_outputs* cvout) {
  if (!ctx) return TCI_EINVAL;
  if (!cvout) return fail(ctx, TCI_EINVAL, "tci_dram_run_cov: null covariance outputs");
  tci_dram_reductions red{};
  red.sopt = sopt;
  red.sout = sout;
  red.copt = copt;
  red.cout = cvout;
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red);
}

int tci_dram_run_reduced(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                         const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                         const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                         tci_dram_outputs* out, const tci_dram_reductions* red) {
  if (!ctx) return TCI_EINVAL;
  if (!red) return fail(ctx, TCI_EINVAL, "tci_dram_run_reduced: null reductions");
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, *red);
}

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
  const int rc = chainquant_probs(ctx, "tci_chainquant", opt, n_chains, ld, &probs, &nq);
  if (rc != TCI_OK) return rc;
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chainquant: npar[" + std::to_string(c) + "] outside [0, ld]");
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chainquant: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chainquant: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chainquant_device(ctx, "tci_chainquant", d_chain, d_s2, n_rows, n_chains, ld, d_npar, probs, nq, out);
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
  const int rc = chaindens_opts(ctx, "tci_chaindens", opt, n_rows, n_chains, ld, &G, &B, &bws, &scratch);
  if (rc != TCI_OK) return rc;
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chaindens: npar[" + std::to_string(c) + "] outside [0, ld]");
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chaindens: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chaindens: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chaindens_device(ctx, "tci_chaindens", d_chain, d_s2, n_rows, n_chains, ld, d_npar, G, B, bws, scratch, out);
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
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red ? *red : tci_dram_reductions{}, &ask);
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
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red ? *red : tci_dram_reductions{}, &ask);
}

int tci_dram_run_lp(tci_ctx* ctx, const tci_dram_options* opt, int64_t n_chains, const int32_t* cell_id,
                    const double* theta0, const double* lower, const double* upper, const double* prior_mu,
                    const double* prior_sig, const double* qcov_diag, const double* sigma2_0, int64_t ld,
                    tci_dram_outputs* out, const tci_dram_reductions* red, const int32_t* group, int64_t n_groups,
                    const tci_chainrhat_options* ropt, tci_chainrhat_outputs* rout, const tci_chainess_options* eopt,
                    tci_chainess_outputs* eout, const tci_chainlp_options* lopt, tci_chainlp_outputs* lout) {
  if (!ctx) return TCI_EINVAL;
  if (!lout) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: null log-posterior outputs");
  const tci_dram_reductions none{};
  if (!group)
    return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                         out, red ? *red : none, nullptr, lopt, lout);
  if (!rout && !eout) return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: group without group reduction outputs");
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_lp: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_lp", eopt, eout};
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red ? *red : none, &ask, lopt, lout);
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
  const TemperAsk task{topt ? topt : &def, tout};
  const tci_dram_reductions none{};
  if (!rout)
    return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                         out, red ? *red : none, nullptr, nullptr, nullptr, &task);
  if (n_groups < 1 || n_groups > n_chains)
    return fail(ctx, TCI_EINVAL, "tci_dram_run_tempered: n_groups must be in [1, n_chains]");
  const RhatAsk ask{ropt, group, n_groups, rout, "tci_dram_run_tempered"};
  return dram_run_impl(ctx, opt, n_chains, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0, ld,
                       out, red ? *red : none, &ask, nullptr, nullptr, &task);
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
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chainess: npar[" + std::to_string(c) + "] outside [0, ld]");
  RhatGroups G;
  const int rc = chainrhat_groups(ctx, "tci_chainess", nullptr, n_rows, n_chains, ld, npar, group, n_groups, &G);
  if (rc != TCI_OK) return rc;
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chainess: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chainess: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chainrhat_device(ctx, "tci_chainess", d_chain, d_s2, n_rows, n_chains, ld, d_npar, G, n_groups, nullptr,
                          opt ? opt->max_lag : 0, out);
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
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chainrhat: npar[" + std::to_string(c) + "] outside [0, ld]");
  RhatGroups G;
  const int rc = chainrhat_groups(ctx, "tci_chainrhat", opt, n_rows, n_chains, ld, npar, group, n_groups, &G);
  if (rc != TCI_OK) return rc;
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chainrhat: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chainrhat: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chainrhat_device(ctx, "tci_chainrhat", d_chain, d_s2, n_rows, n_chains, ld, d_npar, G, n_groups, out);
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
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chaincov: npar[" + std::to_string(c) + "] outside [0, ld]");
  int64_t group = 0;
  const int rc = chaincov_group(ctx, "tci_chaincov", opt, n_chains, ld, &group);
  if (rc != TCI_OK) return rc;
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chaincov: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row;
  double* d_chain = A.alloc<double>(nch, &e);
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chaincov: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chaincov_device(ctx, "tci_chaincov", d_chain, n_rows, n_chains, ld, d_npar, group, out);
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
  if (npar)
    for (int64_t c = 0; c < n_chains; ++c)
      if (npar[c] < 0 || npar[c] > ld)
        return fail(ctx, TCI_ERANGE, "tci_chainstats: npar[" + std::to_string(c) + "] outside [0, ld]");
  const size_t per_row = (size_t)n_chains * (size_t)ld;
  if (per_row > (((size_t)1 << 46) / sizeof(double)) / (size_t)n_rows)
    return fail(ctx, TCI_ENOMEM, "tci_chainstats: the chain is larger than any device memory");
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  DevAllocs A;
  hipError_t e = hipSuccess;
  const size_t nch = (size_t)n_rows * per_row, ns2 = (size_t)n_rows * (size_t)n_chains;
  double* d_chain = A.alloc<double>(nch, &e);
  double* d_s2 = e == hipSuccess && s2chain ? A.alloc<double>(ns2, &e) : nullptr;
  int32_t* d_npar = e == hipSuccess && npar ? A.alloc<int32_t>((size_t)n_chains, &e) : nullptr;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, TCI_ENOMEM, "tci_chainstats: the chain (" + std::to_string(nch * sizeof(double)) +
                                     " bytes) does not fit the device");
  }
  hipStream_t s = ctx->stream;
  TCI_HIP(ctx, hipMemcpyAsync(d_chain, chain, nch * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_s2) TCI_HIP(ctx, hipMemcpyAsync(d_s2, s2chain, ns2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (d_npar) TCI_HIP(ctx, hipMemcpyAsync(d_npar, npar, (size_t)n_chains * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return chainstats_device(ctx, "tci_chainstats", d_chain, d_s2, n_rows, n_chains, ld, d_npar, max_lag, out);
}

}  // extern "C"
