// tci_predict.hip -- posterior predictive envelopes: quantiles over S simulated rows per time point.
//
// mcmcstat's mcmcpred samples the chain, runs the model at every sample and takes plims() of the
// simulated signal at every time point: interp1(sort(x), (n-1)*p+1). The forward kernel leaves the S
// rows of a cell in HBM (tci_predict, tci_api.cpp); k_quantile reduces them over the sample axis.
//
// One workgroup per (selected cell, dye, tile of T time points):
//   1. the S x T tile is read coalesced along time and stored transposed in LDS, one column per time
//      point; the column stride is Spad + 1 doubles (odd), so the 16 lanes of a ds_write_b64 group,
//      which walk 16 columns at one sample index, land on 16 different even banks;
//   2. every value becomes a 64-bit key in a total order: NaNs canonicalised to one positive quiet NaN,
//      then the sign-flip map (negative: all bits inverted; else: sign bit set), so
//      -Inf < ... < -0 < +0 < ... < +Inf < NaN as MATLAB's sort puts them; columns are padded to
//      Spad = the next power of two with the all-ones key, which sorts after everything;
//   3. a bitonic network sorts every column: compare distances below 64 run in registers, one key per
//      lane and a 64-key chunk per wavefront, with cross-lane moves (DPP quad_perm / row_ror for
//      distances 1, 2, 8, ds_bpermute for 4, 16, 32); distances of 64 and more pair keys through LDS;
//   4. keys are mapped back and lanes write the nq values x[lo] + f * (x[lo + 1] - x[lo]): a multiply
//      and an add as written, never fused (plims' interp1).
#include <hip/hip_runtime.h>

#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_key.h"

namespace tci {

namespace {

constexpr int kQThreads = 256;
constexpr int64_t kQTileKeys = 8192;  // keys per workgroup: 64 KiB of LDS + padding, two workgroups per CU

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, true);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// The key of lane (lane ^ J).
template <int J>
__device__ __forceinline__ uint64_t lane_xor(uint64_t v) {
  if (J == 1) return dpp_u64<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  if (J == 2) return dpp_u64<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  if (J == 8) return dpp_u64<0x128>(v);  // row_ror:8 (a rotation by half a 16-lane row)
  return (uint64_t)__shfl_xor((unsigned long long)v, J, 64);
}

// One compare-exchange stage at distance J < 64 between lanes; asc: this lane's pair sorts ascending.
template <int J>
__device__ __forceinline__ void lane_stage(uint64_t& v, int lane, bool asc) {
  const uint64_t p = lane_xor<J>(v);
  const bool keep_min = ((lane & J) == 0) == asc;
  const uint64_t mn = p < v ? p : v, mx = p < v ? v : p;
  v = keep_min ? mn : mx;
}

// Stages J = JMAX, JMAX / 2, .., 1 of merge size k (keys at column index i; ascending where (i & k) == 0).
template <int JMAX>
__device__ __forceinline__ void lane_stages(uint64_t& v, int lane, bool asc) {
  if (JMAX >= 32) lane_stage<32>(v, lane, asc);
  if (JMAX >= 16) lane_stage<16>(v, lane, asc);
  if (JMAX >= 8) lane_stage<8>(v, lane, asc);
  if (JMAX >= 4) lane_stage<4>(v, lane, asc);
  if (JMAX >= 2) lane_stage<2>(v, lane, asc);
  lane_stage<1>(v, lane, asc);
}

struct QuantileArgs {
  int32_t nq;
  int32_t lo[16];
  double f[16];
};

// sim: [n_sel * S][ld_out] rows of one dye per pointer; out: [n_sel * nq][ld_out].
// T (time points per tile) and Spad are powers of two with T * Spad a multiple of 64.
__global__ __launch_bounds__(kQThreads) void k_quantile(const CellMeta* __restrict__ cells,
                                                        const int32_t* __restrict__ row_cell,
                                                        const double* __restrict__ sim0,
                                                        const double* __restrict__ sim1, int S, int lg_spad, int lg_t,
                                                        int64_t ld_out, int tiles, QuantileArgs qa,
                                                        double* __restrict__ out0, double* __restrict__ out1) {
  extern __shared__ __align__(16) uint64_t keys[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int spad = 1 << lg_spad, T = 1 << lg_t, stride = spad + 1;
  const int64_t bid = blockIdx.x;
  const int tile = (int)(bid % tiles);
  const int64_t rest = bid / tiles;
  const int dye = (int)(rest & 1);
  const int64_t k = rest >> 1;
  const double* sim = dye ? sim1 : sim0;
  double* out = dye ? out1 : out0;
  const int N = cells[row_cell[k * S]].n;
  const int j0 = tile << lg_t;

  // 1 + 2: coalesced along time, transposed into LDS as keys; points past N and samples past S pad
  for (int idx = tid; idx < (spad << lg_t); idx += kQThreads) {
    const int s = idx >> lg_t, jj = idx & (T - 1), j = j0 + jj;
    uint64_t key = ~0ull;
    if (s < S && j < N) key = to_key(sim[(k * S + s) * ld_out + j]);
    keys[jj * stride + s] = key;
  }
  __syncthreads();

  // 3: bitonic sort of every column. Flat key index e = column * Spad + i; a wavefront holds 64
  // consecutive e (Spad < 64: several whole columns), so lane ^ J pairs i ^ J for every J < min(64, Spad).
  const int chunks = (spad << lg_t) >> 6;
  for (int ch = wave; ch < chunks; ch += kQThreads / 64) {
    const int e = (ch << 6) + lane, i = e & (spad - 1), a = (e >> lg_spad) * stride + i;
    uint64_t v = keys[a];
    if (spad >= 2) lane_stages<1>(v, lane, (i & 2) == 0);
    if (spad >= 4) lane_stages<2>(v, lane, (i & 4) == 0);
    if (spad >= 8) lane_stages<4>(v, lane, (i & 8) == 0);
    if (spad >= 16) lane_stages<8>(v, lane, (i & 16) == 0);
    if (spad >= 32) lane_stages<16>(v, lane, (i & 32) == 0);
    if (spad >= 64) lane_stages<32>(v, lane, (i & 64) == 0);
    keys[a] = v;
  }
  __syncthreads();
  for (int lg_k = 7; lg_k <= lg_spad; ++lg_k) {
    const int kk = 1 << lg_k;
    for (int lg_j = lg_k - 1; lg_j >= 6; --lg_j) {  // distances >= 64: pairs (i, i | j) through LDS
      const int jd = 1 << lg_j;
      for (int t = tid; t < (spad << lg_t) >> 1; t += kQThreads) {
        const int c = t >> (lg_spad - 1), r = t & ((spad >> 1) - 1);
        const int i = ((r & ~(jd - 1)) << 1) | (r & (jd - 1));
        const int a = c * stride + i;
        const uint64_t x = keys[a], y = keys[a + jd];
        if ((x > y) == ((i & kk) == 0)) {
          keys[a] = y;
          keys[a + jd] = x;
        }
      }
      __syncthreads();
    }
    for (int ch = wave; ch < chunks; ch += kQThreads / 64) {  // distances 32 .. 1 in registers
      const int e = (ch << 6) + lane, i = e & (spad - 1), a = (e >> lg_spad) * stride + i;
      uint64_t v = keys[a];
      lane_stages<32>(v, lane, (i & kk) == 0);
      keys[a] = v;
    }
    __syncthreads();
  }

  // 4: plims: x[lo] + f * (x[lo + 1] - x[lo]), or x[S - 1] at the upper end; NaN past the cell's N
  for (int idx = tid; idx < (qa.nq << lg_t); idx += kQThreads) {
    const int q = idx >> lg_t, jj = idx & (T - 1), j = j0 + jj;
    if (j >= ld_out) continue;
    double r = qnan();
    if (j < N) {
      const uint64_t* col = keys + jj * stride;
      const int lo = qa.lo[q];
      if (lo + 1 < S) {
        const double x0 = from_key(col[lo]), x1 = from_key(col[lo + 1]);
        r = __dadd_rn(x0, __dmul_rn(qa.f[q], __dsub_rn(x1, x0)));
      } else {
        r = from_key(col[S - 1]);
      }
    }
    out[(k * qa.nq + q) * ld_out + j] = r;
  }
}

int lg2_ceil(int64_t x) {
  int l = 0;
  while (((int64_t)1 << l) < x) ++l;
  return l;
}

// Tile shape for S samples: Spad = 2^lg_spad >= S, T = 2^lg_t time points with T * Spad <= kQTileKeys
// (at least 2 columns, at most 64), and the dynamic LDS of one workgroup.
void quantile_shape(int64_t S, int* lg_spad, int* lg_t, size_t* lds) {
  *lg_spad = lg2_ceil(S);
  const int64_t spad = (int64_t)1 << *lg_spad;
  int64_t T = kQTileKeys / spad;
  T = T < 2 ? 2 : (T > 64 ? 64 : T);
  *lg_t = lg2_ceil(T);
  *lds = (size_t)T * (size_t)(spad + 1) * sizeof(uint64_t);
}

}  // namespace

int quantile_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells) {
  int lg_spad, lg_t;
  size_t lds;
  quantile_shape(S, &lg_spad, &lg_t, &lds);
  const int64_t tiles = (ld_out + ((int64_t)1 << lg_t) - 1) >> lg_t;
  // one launch: 2 * cells * tiles workgroups in grid.x, and cells * S rows in the forward launch's grid.x
  const int64_t by_grid = ((int64_t)1 << 30) / (2 * tiles), by_rows = ((int64_t)1 << 30) / S;
  *max_cells = by_grid < by_rows ? by_grid : by_rows;
  return *max_cells >= 1 ? TCI_OK : TCI_EINVAL;
}

int launch_quantile(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1, int64_t n_sel,
                    int64_t S, int64_t ld_out, const double* probs, int32_t nq, double* out0, double* out1,
                    void* stream) {
  if (n_sel <= 0) return TCI_OK;
  if (S < 1 || S > 4096 || nq < 1 || nq > 16 || ld_out < 1) return TCI_EINVAL;
  int lg_spad, lg_t;
  size_t dyn;
  quantile_shape(S, &lg_spad, &lg_t, &dyn);
  const int64_t tiles = (ld_out + ((int64_t)1 << lg_t) - 1) >> lg_t;
  if (tiles > ((int64_t)1 << 30) || 2 * n_sel > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  // static + dynamic LDS as the code object has it: a launch that cannot fit a CU's 160 KiB is refused here
  hipFuncAttributes a{};
  if (hipFuncGetAttributes(&a, (const void*)k_quantile) != hipSuccess) return TCI_EHIP;
  if ((size_t)a.sharedSizeBytes + dyn > (size_t)160 * 1024) return TCI_EINVAL;
  if (ensure_dyn_lds((const void*)k_quantile, dyn) != TCI_OK) return TCI_EHIP;
  QuantileArgs qa{};
  qa.nq = nq;
  for (int q = 0; q < nq; ++q) {
    const double h = (double)(S - 1) * probs[q];
    const double lo = floor(h);
    qa.lo[q] = (int32_t)lo;
    qa.f[q] = h - lo;
  }
  hipLaunchKernelGGL(k_quantile, dim3((unsigned)(2 * n_sel * tiles)), dim3(kQThreads), dyn, (hipStream_t)stream,
                     kp.cells, row_cell, sim0, sim1, (int)S, lg_spad, lg_t, ld_out, (int)tiles, qa, out0, out1);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
