// tci_fitcheck.hip -- posterior predictive fit checks: every datum scored under the Gaussian mixture that S
// posterior samples (theta_s, sigma2_s) define; the definition is in include/tci.h.
//
// The forward kernel leaves the S simulated rows of a cell in HBM (tci_fitcheck, tci_api.cpp); k_fitcheck reduces
// them over the sample axis into six values per (cell, dye, time point): lppd, p_waic, pit, resid, zbar, z2.
//
// One workgroup (4 wavefronts) per (selected cell, dye, tile of 64 time points). Lane l of every wavefront is time
// point 64 * tile + l, so a row read is one 512 B segment. The sample axis is cut into the contract's segments of 64
// consecutive samples; the wavefronts take them in rounds (round r: wavefront w takes segment 4 r + w), each lane adds
// its segment's terms in ascending s from 0.0, and after every round all four wavefronts read the round's partials
// from LDS and add them to their totals in segment order: every wavefront holds the same totals, and their bits follow
// from S alone. The partials are double-buffered by the round's parity, so a round costs one barrier.
//
// Two passes over the rows. The first gives max ll, sum ll, the PIT sum and the residual sums; the second needs the
// maximum and the mean of the first: sum exp(ll - m) and sum (ll - lbar)^2. The second pass reads the rows again and
// restates ll (a subtraction, a division, two multiplies and an add: the same operations, the same bits) instead of
// keeping ll or the rows in LDS: at the cap S = 4096 a 64-point tile is 2 MiB, a CU's 160 KiB would hold no more than
// two time points of it, and lanes along the sample axis would break the coalesced row reads. A tile's rows (S x 512 B,
// 250 KiB at S = 500) are still in the XCD's L2 when the second pass comes. What LDS holds is 2 x 4 x 5 x 64 partials
// (20 KiB) and the wavefronts' maxima and flags.
#include <hip/hip_runtime.h>

#include "tci_fp.h"
#include "tci_internal.h"

namespace tci {

namespace {

constexpr int kFcLanes = 64;   // time points per tile: one per lane
constexpr int kFcWaves = 4;    // wavefronts per workgroup, each a segment of the round
constexpr int kFcSeg = 64;     // samples per segment (include/tci.h: the order of every SUM_s)
constexpr int kFcSums = 5;     // partial sums of the first pass: ll, pit, r, z, z * z
constexpr int kFcU = 8;        // rows a wavefront loads together

struct FcTerm {
  double r, z, zz, ll;
};

// r = y - f; z = r / sd; ll = -0.5 * (lg + z * z): every operation rounded once (the build has -ffp-contract=off)
__device__ __forceinline__ FcTerm fc_term(double y, double f, double sd, double lg) {
  FcTerm t;
  t.r = y - f;
  t.z = t.r / sd;
  t.zz = t.z * t.z;
  t.ll = -0.5 * (lg + t.zz);
  return t;
}

// sim: [n_sel * S][ld_out] rows of one dye per pointer; sd, lg: [n_sel * S]; out: [n_sel][2][6][ld_out].
__global__ __launch_bounds__(kFcLanes * kFcWaves) void k_fitcheck(const CellMeta* __restrict__ cells,
                                                                   const PointRec* __restrict__ points,
                                                                   int64_t cell_stride,
                                                                   const int32_t* __restrict__ row_cell,
                                                                   const double* __restrict__ sim0,
                                                                   const double* __restrict__ sim1,
                                                                   const double* __restrict__ sd,
                                                                   const double* __restrict__ lg, int S, int64_t ld_out,
                                                                   int tiles, double logS, double* __restrict__ out) {
  __shared__ double part[2][kFcWaves][kFcSums][kFcLanes];
  __shared__ double red_m[kFcWaves][kFcLanes];
  __shared__ uint32_t red_bad[kFcWaves][kFcLanes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t bid = blockIdx.x;
  const int tile = (int)(bid % tiles);
  const int64_t rest = bid / tiles;
  const int dye = (int)(rest & 1);
  const int64_t k = rest >> 1;
  const int32_t cell = row_cell[k * S];
  const int N = cells[cell].n;
  const int64_t j = (int64_t)tile * kFcLanes + lane;
  double* o = out + (k * 2 + dye) * 6 * ld_out + j;
  if ((int64_t)tile * kFcLanes >= N) {  // a tile of padding only (the same for the whole workgroup)
    if (wave == 0 && j < ld_out)
      for (int q = 0; q < 6; ++q) o[q * ld_out] = qnan();
    return;
  }
  const bool live = j < N;  // the forward launch wrote sim[.., j] for j < N only
  const double* col = (dye ? sim1 : sim0) + k * S * ld_out + j;
  const double* sdk = sd + k * S;
  const double* lgk = lg + k * S;
  double y = 0.0;
  if (live) {
    const PointRec& p = points[(int64_t)cell * cell_stride + j];
    y = dye ? p.y2 : p.y1;
  }
  const int nseg = (S + kFcSeg - 1) / kFcSeg, rounds = (nseg + kFcWaves - 1) / kFcWaves;

  // ---- pass 1: max ll, and the sums of ll, the PIT terms, r, z and z * z
  double m = -INFINITY;
  bool bad = false;
  double tot[kFcSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < rounds; ++r) {
    const int seg = r * kFcWaves + wave;
    double acc[kFcSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (seg < nseg) {
      const int s1 = min(S, (seg + 1) * kFcSeg);
      for (int s0 = seg * kFcSeg; s0 < s1; s0 += kFcU) {
        double f[kFcU];
#pragma unroll
        for (int u = 0; u < kFcU; ++u) f[u] = (live && s0 + u < s1) ? col[(int64_t)(s0 + u) * ld_out] : 0.0;
#pragma unroll
        for (int u = 0; u < kFcU; ++u) {
          if (s0 + u < s1) {
            bad |= !is_finite(f[u]);
            const FcTerm t = fc_term(y, f[u], sdk[s0 + u], lgk[s0 + u]);
            m = t.ll > m ? t.ll : m;
            acc[0] = acc[0] + t.ll;
            acc[1] = acc[1] + 0.5 * erfc(-t.z * 0.7071067811865476);
            acc[2] = acc[2] + t.r;
            acc[3] = acc[3] + t.z;
            acc[4] = acc[4] + t.zz;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kFcSums; ++q) part[r & 1][wave][q][lane] = acc[q];
    __syncthreads();
    for (int w = 0; w < kFcWaves; ++w)
      if (r * kFcWaves + w < nseg) {
#pragma unroll
        for (int q = 0; q < kFcSums; ++q) tot[q] = tot[q] + part[r & 1][w][q][lane];
      }
  }
  red_m[wave][lane] = m;
  red_bad[wave][lane] = bad ? 1u : 0u;
  __syncthreads();  // also: every read of the first pass's partials is over
  uint32_t anybad = 0;
#pragma unroll
  for (int w = 0; w < kFcWaves; ++w) {
    const double mw = red_m[w][lane];
    m = mw > m ? mw : m;
    anybad |= red_bad[w][lane];
  }
  const double dS = (double)S;
  const double lbar = tot[0] / dS;

  // ---- pass 2: sum exp(ll - m) and sum (ll - lbar)^2, ll restated from the rows (the same bits)
  double tot2[2] = {0.0, 0.0};
  for (int r = 0; r < rounds; ++r) {
    const int seg = r * kFcWaves + wave;
    double acc[2] = {0.0, 0.0};
    if (seg < nseg) {
      const int s1 = min(S, (seg + 1) * kFcSeg);
      for (int s0 = seg * kFcSeg; s0 < s1; s0 += kFcU) {
        double f[kFcU];
#pragma unroll
        for (int u = 0; u < kFcU; ++u) f[u] = (live && s0 + u < s1) ? col[(int64_t)(s0 + u) * ld_out] : 0.0;
#pragma unroll
        for (int u = 0; u < kFcU; ++u) {
          if (s0 + u < s1) {
            const FcTerm t = fc_term(y, f[u], sdk[s0 + u], lgk[s0 + u]);
            const double d = t.ll - lbar;
            acc[0] = acc[0] + exp(t.ll - m);
            acc[1] = acc[1] + d * d;
          }
        }
      }
    }
    part[r & 1][wave][0][lane] = acc[0];
    part[r & 1][wave][1][lane] = acc[1];
    __syncthreads();
    for (int w = 0; w < kFcWaves; ++w)
      if (r * kFcWaves + w < nseg) {
        tot2[0] = tot2[0] + part[r & 1][w][0][lane];
        tot2[1] = tot2[1] + part[r & 1][w][1][lane];
      }
  }

  if (wave == 0 && j < ld_out) {
    const bool scored = live && is_finite(y) && anybad == 0;
    double v[6];
    v[0] = (m + log(tot2[0])) - logS;
    v[1] = tot2[1] / (double)(S - 1);
    v[2] = tot[1] / dS;
    v[3] = tot[2] / dS;
    v[4] = tot[3] / dS;
    v[5] = tot[4] / dS;
#pragma unroll
    for (int q = 0; q < 6; ++q) o[q * ld_out] = scored ? v[q] : qnan();
  }
}

int64_t fc_tiles(int64_t ld_out) { return (ld_out + kFcLanes - 1) / kFcLanes; }

}  // namespace

int fitcheck_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells) {
  // one launch: 2 * cells * tiles workgroups in grid.x, and cells * S rows in the forward launch's grid.x
  const int64_t by_grid = ((int64_t)1 << 30) / (2 * fc_tiles(ld_out)), by_rows = ((int64_t)1 << 30) / S;
  *max_cells = by_grid < by_rows ? by_grid : by_rows;
  return *max_cells >= 1 ? TCI_OK : TCI_EINVAL;
}

int launch_fitcheck(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1,
                    const double* sd, const double* lg, int64_t n_sel, int64_t S, int64_t ld_out, double logS,
                    double* out, void* stream) {
  if (n_sel <= 0) return TCI_OK;
  if (S < 1 || S > 4096 || ld_out < 1) return TCI_EINVAL;
  const int64_t tiles = fc_tiles(ld_out);
  if (tiles > ((int64_t)1 << 30) || 2 * n_sel > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  // the LDS is static (the partials do not grow with S); as the code object has it, it must fit a CU's 160 KiB
  hipFuncAttributes a{};
  if (hipFuncGetAttributes(&a, (const void*)k_fitcheck) != hipSuccess) return TCI_EHIP;
  if ((size_t)a.sharedSizeBytes > (size_t)160 * 1024) return TCI_EINVAL;
  hipLaunchKernelGGL(k_fitcheck, dim3((unsigned)(2 * n_sel * tiles)), dim3(kFcLanes * kFcWaves), 0, (hipStream_t)stream,
                     kp.cells, kp.points, kp.cell_stride, row_cell, sim0, sim1, sd, lg, (int)S, ld_out, (int)tiles, logS,
                     out);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
