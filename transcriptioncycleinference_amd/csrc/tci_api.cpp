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

#include "tci_api_internal.h"
#include "tci_diag.h"

using tci::CellMeta;
using tci::KParams;
using namespace tci_api;

namespace {

const char kVersion[] = "tci-mi355x 0.1.0 (gfx950)";

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

// Bytes of theta + ids + flags + SS per call up to which tci_ss_batch works in place in pinned host
// memory (TCI_ZERO_COPY_MAX overrides; 0 disables).
size_t zero_copy_max() {
  static const size_t v = [] {
    const char* e = std::getenv("TCI_ZERO_COPY_MAX");
    return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)1024 * 1024;
  }();
  return v;
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

}  // namespace

// Host-side validation of a host-pointer batch (cell ids and row lengths).
int tci_api::check_rows(tci_ctx* ctx, int64_t ld, const int32_t* cell, int64_t B) {
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

namespace {

const double kP2P_ms2_start[1] = {0.024};
const double kP2P_ms2_end[1] = {1.299};
const double kP2P_ms2_loopn[1] = {24};
const double kP2P_pp7_start[1] = {4.292};
const double kP2P_pp7_end[1] = {5.758};
const double kP2P_pp7_loopn[1] = {24};

// The device work tci_fitcheck and tci_loocheck share. Per chunk of whole cells: the rows' uploads, the forward launch
// into the scratch, then `launch` (the reduction over the S samples: cell_out doubles per cell), the two timed apart;
// each(p, k) then reads cell k's values at p.
template <typename Each>
int score_chunks(tci_ctx* ctx, const char* who_, decltype(tci::launch_fitcheck)* launch, const double* theta, int64_t ld_theta,
                 const double* s2, const int32_t* cell_id, int64_t n_sel, int64_t S, int64_t ld_out, int64_t chunk,
                 size_t cell_out, double* forward_ms, double* kernel_ms, Each each) {
  const std::string who = who_;
  const size_t rows_max = (size_t)(chunk * S);
  std::vector<int32_t> row_cell;
  std::vector<double> sdlg, pt;
  try {
    row_cell.resize(rows_max);
    sdlg.resize(2 * rows_max);
    pt.resize((size_t)chunk * cell_out);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, who + ": host allocation failed");
  }
  const double logS = std::log((double)S);
  int rc;
  TCI_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure(ctx, &ctx->d_theta, &ctx->cap_theta, rows_max * (size_t)ld_theta)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_cell, &ctx->cap_cell, rows_max)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_sim, &ctx->cap_sim, 2 * rows_max * (size_t)ld_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out0, &ctx->cap_out0, (size_t)chunk * cell_out)) != TCI_OK) return rc;
  if ((rc = ensure(ctx, &ctx->d_out1, &ctx->cap_out1, 2 * rows_max)) != TCI_OK) return rc;
  hipStream_t st = ctx->stream;
  EventTimer events(3);
  const char* what = nullptr;
  const hipError_t ee = events.create(&what);
  if (ee != hipSuccess) return hip_fail(ctx, ee, (who + ": hipEventCreate").c_str());
  const hipEvent_t e0 = events.ev[0], e1 = events.ev[1], e2 = events.ev[2];
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
    rc = run(ctx, tci::MODE_FWD_INTERP, ctx->d_theta, ld_theta, ctx->d_cell, nullptr, B, sim0, sim1, ld_out, (void*)st);
    if (rc != TCI_OK) return rc;
    TCI_HIP(ctx, hipEventRecord(e1, st));
    rc = launch(ctx->kp, ctx->d_cell, sim0, sim1, d_sd, d_lg, nc, S, ld_out, logS, ctx->d_out0, (void*)st);
    if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), (who + ": kernel launch").c_str());
    if (rc != TCI_OK) return fail(ctx, rc, who + ": the kernel does not fit a CU's LDS or the grid");
    TCI_HIP(ctx, hipEventRecord(e2, st));
    TCI_HIP(ctx, hipMemcpyAsync(pt.data(), ctx->d_out0, (size_t)nc * cell_out * sizeof(double), hipMemcpyDeviceToHost, st));
    TCI_HIP(ctx, hipStreamSynchronize(st));  // the host vectors and the staging buffers are reused by the next chunk
    float ms = 0.f;
    TCI_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *forward_ms += (double)ms;
    TCI_HIP(ctx, hipEventElapsedTime(&ms, e1, e2));
    *kernel_ms += (double)ms;
    for (int64_t k = 0; k < nc; ++k) each(pt.data() + (size_t)k * cell_out, k0 + k);
  }
  return TCI_OK;
}

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
  return score_chunks(ctx, "tci_fitcheck", tci::launch_fitcheck, theta, ld_theta, s2, cell_id, n_sel, S, ld_out, chunk,
                      (size_t)12 * (size_t)ld_out, &out->forward_ms, &out->kernel_ms, [&](const double* p, int64_t k) {
                        double* const dst[6] = {out->lppd_i, out->p_waic_i, out->pit, out->resid, out->zbar, out->z2};
                        for (int q = 0; q < 6; ++q)
                          if (dst[q])
                            for (int d = 0; d < 2; ++d)
                              std::memcpy(dst[q] + ((size_t)k * 2 + d) * (size_t)ld_out, p + ((size_t)d * 6 + q) * (size_t)ld_out,
                                          (size_t)ld_out * sizeof(double));
                        fitcheck_cell(p, ld_out, o, k, out);
                      });
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
  const size_t len = 2 * (size_t)ld_out;
  std::vector<double> elpd_all;
  try {
    if (grouped) elpd_all.resize((size_t)n_sel * len);
  } catch (const std::bad_alloc&) {
    return fail(ctx, TCI_ENOMEM, "tci_loocheck: host allocation failed");
  }
  rc = score_chunks(ctx, "tci_loocheck", tci::launch_loocheck, theta, ld_theta, s2, cell_id, n_sel, S, ld_out, chunk,
                    (size_t)8 * (size_t)ld_out, &out->forward_ms, &out->kernel_ms, [&](const double* p, int64_t k) {
                      double* const dst[4] = {out->elpd_loo_i, out->lppd_i, out->p_loo_i, out->khat_i};
                      for (int q = 0; q < 4; ++q)
                        if (dst[q])
                          for (int d = 0; d < 2; ++d)
                            std::memcpy(dst[q] + ((size_t)k * 2 + d) * (size_t)ld_out, p + ((size_t)d * 4 + q) * (size_t)ld_out,
                                        (size_t)ld_out * sizeof(double));
                      if (grouped)
                        for (int d = 0; d < 2; ++d)
                          std::memcpy(elpd_all.data() + ((size_t)k * 2 + d) * (size_t)ld_out, p + (size_t)d * 4 * (size_t)ld_out,
                                      (size_t)ld_out * sizeof(double));
                      loocheck_chain(p, ld_out, thr, k, out);
                    });
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
