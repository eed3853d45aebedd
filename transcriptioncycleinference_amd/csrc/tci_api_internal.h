// tci_api_internal.h -- what the host translation units of the C ABI share (tci_api.cpp: context and likelihood,
// tci_api_chain.cpp: the reductions of a stored chain, tci_api_dram.cpp: the sampler, tci_api_search.cpp: the mode
// search). No .hip file includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "tci_dram_internal.h"
#include "tci_internal.h"

struct tci_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int rpl = 1;
  int64_t stride = 0;               // records per cell in the resident tables
  int64_t n_cells = 0;
  int64_t max_points = 0;
  int64_t device_bytes = 0;
  std::vector<tci::CellMeta> meta;  // host copy
  std::vector<double> grid;         // host copy of t_interp (cell c at c * stride)
  tci::KParams kp{};
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

namespace tci_api {

inline int fail(tci_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

inline int hip_fail(tci_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, TCI_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define TCI_HIP(ctx, call)                                  \
  do {                                                      \
    hipError_t e_ = (call);                                 \
    if (e_ != hipSuccess) return hip_fail((ctx), e_, #call); \
  } while (0)

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

inline int ensure_io(tci_ctx* ctx, size_t need) {
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

// Host-side validation of a host-pointer batch (cell ids and row lengths); tci_api.cpp.
int check_rows(tci_ctx* ctx, int64_t ld, const int32_t* cell, int64_t B);

// Device allocations of one call, freed together.
struct DevAllocs {
  std::vector<void*> ptrs;
  DevAllocs() = default;
  DevAllocs(const DevAllocs&) = delete;
  DevAllocs& operator=(const DevAllocs&) = delete;
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

// Two HIP events around a stretch of a stream's work (three for a caller that times two stretches), created
// together or not at all and destroyed with their owner. create: *what names the failed call as tci_last_error does.
struct EventTimer {
  hipEvent_t ev[3] = {};
  const int n;
  explicit EventTimer(int n_events = 2) : n(n_events) {}
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  ~EventTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(const char** what) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < n && e == hipSuccess; ++k) {
      *what = k == 0 ? "hipEventCreate(&ev0)" : "hipEventCreate";
      if ((e = hipEventCreate(&ev[k])) != hipSuccess) ev[k] = nullptr;
    }
    return e;
  }
  hipError_t start(hipStream_t s) { return hipEventRecord(ev[0], s); }
  hipError_t stop(hipStream_t s) { return hipEventRecord(ev[1], s); }
  hipError_t elapsed_ms(float* ms) { return hipEventElapsedTime(ms, ev[0], ev[1]); }
};

// One timed launch on the context's stream and the copies of its results to the host: the events around `launch` (a
// callable that returns a TCI_* code), then every copy with a destination, then the synchronisation. *ms: the device
// time between the events. `what`: the nouns of the three HIP failures, the launch's, the kernels' and the copies'.
struct LaunchNouns {
  const char *launch, *kernel, *copy;
  const char* refused = nullptr;  // what a launch wrapper's own refusal means (null: the chain reductions' size limit)
};
struct CopyBack {
  void* dst;
  const void* src;
  size_t bytes;
};
template <typename Launch>
int timed_launch(tci_ctx* ctx, const char* who, const LaunchNouns& what, Launch&& launch,
                 std::initializer_list<CopyBack> copies, float* ms) {
  hipStream_t s = ctx->stream;
  EventTimer timer;
  const char* what_create = nullptr;
  hipError_t e1 = timer.create(&what_create);
  if (e1 != hipSuccess) return hip_fail(ctx, e1, what_create);
  e1 = timer.start(s);
  const int rc = launch();
  if (e1 == hipSuccess) e1 = timer.stop(s);
  for (const CopyBack& c : copies)
    if (c.dst && rc == TCI_OK && e1 == hipSuccess) e1 = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  *ms = 0.f;
  if (rc == TCI_OK && e1 == hipSuccess && e2 == hipSuccess) e1 = timer.elapsed_ms(ms);
  if (rc == TCI_EHIP) return hip_fail(ctx, hipGetLastError(), what.launch);
  if (rc != TCI_OK)
    return fail(ctx, rc, std::string(who) + ": " + (what.refused ? what.refused : "rows x chains x ld too large for one launch"));
  if (e2 != hipSuccess) return hip_fail(ctx, e2, what.kernel);
  if (e1 != hipSuccess) return hip_fail(ctx, e1, what.copy);
  return TCI_OK;
}

// ---- the reductions of a chain on the device (tci_api_chain.cpp), shared by the stand-alone tci_chain* entry points
// and the sampler's reductions of its kept rows: each one's option checks (before any device work), then its kernels,
// timed, with the results scattered into the caller's host buffers. d_npar null: ld columns for every chain; d_s2
// null: the s2 twins are NaN / -1.
int chainstats_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                      int64_t n_chains, int64_t ld, const int32_t* d_npar, int64_t max_lag, tci_chainstats_outputs* out);
int chaincov_group(tci_ctx* ctx, const char* who, const tci_chaincov_options* copt, int64_t n_chains, int64_t ld,
                   int64_t* group);
int chaincov_device(tci_ctx* ctx, const char* who, const double* d_chain, int64_t n_rows, int64_t n_chains, int64_t ld,
                    const int32_t* d_npar, int64_t group, tci_chaincov_outputs* out);
int chainquant_probs(tci_ctx* ctx, const char* who, const tci_chainquant_options* qopt, int64_t n_chains, int64_t ld,
                     const double** probs, int32_t* nq);
int chainquant_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                      int64_t n_chains, int64_t ld, const int32_t* d_npar, const double* probs, int32_t nq,
                      tci_chainquant_outputs* out);
int chaindens_opts(tci_ctx* ctx, const char* who, const tci_chaindens_options* dopt, int64_t n_rows, int64_t n_chains,
                   int64_t ld, int32_t* G, int32_t* B, double* bw_scale, size_t* scratch);
int chaindens_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, int32_t G, int32_t B, double bw_scale,
                     size_t scratch, tci_chaindens_outputs* out);
int chainlp_check(tci_ctx* ctx, const char* who, const tci_chainlp_options* lopt, int64_t n_rows, int64_t n_chains,
                  int64_t ld, const int32_t* cell_id, const double* prior_mu, const double* prior_sig, size_t* scratch);
int chainlp_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                   int64_t n_chains, int64_t ld, const int32_t* d_cell, const int32_t* d_npar, const double* d_mu,
                   const double* d_sig, size_t scratch, tci_chainlp_outputs* out);
// The groups of a group reduction, checked before any device work: group (null: every chain in group 0) as the
// per-chain vector the kernels skip by, and its CSR form (the chains of a group ascending). npar (host, may be null =
// ld): the chains of a group must have one npar.
struct RhatGroups {
  std::vector<int32_t> group, off, list;
  size_t scratch = 0;
};
int chainrhat_groups(tci_ctx* ctx, const char* who, const tci_chainrhat_options* ropt, int64_t n_rows, int64_t n_chains,
                     int64_t ld, const int32_t* npar, const int32_t* group, int64_t n_groups, RhatGroups* G);
int chainrhat_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, const RhatGroups& G, int64_t n_groups,
                     tci_chainrhat_outputs* out, int64_t max_lag = 0, tci_chainess_outputs* eout = nullptr);
// tci_chainrank's option checks (*o: the options to use, the defaults for null) and its four passes over the groups
// chainrhat_groups made.
int chainrank_opts(tci_ctx* ctx, const char* who, const tci_chainrank_options* kopt, tci_chainrank_options* o);
int chainrank_device(tci_ctx* ctx, const char* who, const double* d_chain, const double* d_s2, int64_t n_rows,
                     int64_t n_chains, int64_t ld, const int32_t* d_npar, const RhatGroups& G, int64_t n_groups,
                     const tci_chainrank_options& o, tci_chainrank_outputs* out);

}  // namespace tci_api
