// PSVM on gfx950, all fp64: the pivoted incomplete Cholesky factorisation of the
// Gaussian kernel with its state on the device, the weighted symmetric product
// C = A^T diag(w) A of the interior-point Newton system on
// v_mfma_f64_16x16x4_f64, the two thin products of its solves, and the decision
// function of the fitted model with the kernel values kept in registers.
//
//   icf_init_kernel     diag = 1, first pivot candidate (row 0), empty record
//   icf_pivot_kernel    one workgroup: arg-max of the block partials (ties to the
//                       lower row), stop test, copy of the pivot row's x and H
//   icf_step_kernel     column k of H for a block of rows, new diag, block arg-max
//   wsyrk_kernel        one 64 x 64 block of C over one slab of rows
//   wsyrk_fold_kernel   slabs added in slab order, both triangles written
//   tall_tv_kernel      A^T diag(s) V, r <= 4 columns, slab partials
//   tall_fold_kernel    slabs added in slab order
//   tall_v_kernel       diag(s) A T, r <= 4 columns
//   rbf_sqnorm_kernel   fp64 squared row norms of an fp32 matrix
//   rbf_decision_kernel sum_j coef_j exp(-gamma |x_i - s_j|^2) for 64 rows over one
//                       slab of support vectors
//   rbf_decision_fold_kernel  slabs added in slab order
//
// Nothing here uses a floating-point atomic or waits for another workgroup;
// every sum has a fixed order, so results are bit-identical between calls.
//
// Units.  icf_step_kernel and tall_v_kernel give every row a unit of U adjacent
// lanes (U a power of two, 1 .. 64, chosen by the host from the row length):
// lane c reads columns c, c + U, ..., so one wave instruction reads 64 / U
// contiguous row segments, and the unit's sum is a butterfly over its lanes.
//
// wsyrk.  A workgroup of four waves stages chunks of 16 rows of the two
// 64-column panels of A in LDS (left panel times w), double buffered: the next
// chunk's global loads are issued before the matrix instructions of the current
// one and written to the other buffer after them, one barrier per chunk.  An LDS
// row is 80 doubles: an operand read takes 16 lanes across columns and 4 rows,
// and 80 * 2 = 32 (mod 64) banks puts rows r and r + 1 on the two halves of the
// banks.  Wave w owns the 2 x 2 set of 16 x 16 tiles at tile row 2 (w / 2), tile
// column 2 (w % 2): two left and two right operand reads feed four instructions.
// A diagonal block reads its panel from global memory once and writes the
// weighted and the plain copy; its wave below the diagonal only stages.  Columns
// past k and rows past the slab are zero in the stage.
//
// rbf_decision.  A workgroup of four waves owns 64 scored rows and walks one slab
// of support vectors in tiles of 64.  The cross term C = S_tile X_block^T runs on
// the matrix units with the wsyrk wave layout (C rows are SVs, C columns scored
// rows), so a lane owns the scored rows lane % 16 of its two column tiles and four
// SVs per accumulator.  The fp32 inputs are widened to fp64 on their way into LDS,
// which is exact: every product is exact and only the additions round.  The
// features are walked in chunks of 16; the stage is [feature][point], 80 doubles a
// row as above, and a thread stages four adjacent features of one point (lanes
// along points, so the transposed LDS writes are consecutive).  Up to kRbfResD
// features the X block is staged once and stays in LDS for the whole slab
// (kResident); above, its chunks are staged again for every SV tile next to those
// of S.  The SV chunks are double buffered over the flattened (tile, chunk)
// sequence: global loads of the next step before the matrix instructions of this
// one, LDS writes after, one barrier per step.  A tile's |s_j|^2 and coef_j travel
// with its first chunk into a stage of their own, alternating by tile.  After a
// tile's last chunk the epilogue stays in registers: d2 = |x_i|^2 + |s_j|^2 - 2 c
// clamped at 0, exp, times coef_j, added into one running sum per lane and column
// tile in a fixed order.  At the slab's end the four lane groups are added by
// cross-lane moves and the two waves that share rows through LDS.  Ragged rows,
// SVs and features are zeros in the stage, padded SVs carry coef = 0.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxD = 1024;          // ICF: features
constexpr int kMaxP = 4096;          // ICF: rank
constexpr int kIcfUnitRows = 16;     // rows per unit of the step kernel
constexpr int kBlk = 64;             // wsyrk block of C
constexpr int kChunk = 16;           // wsyrk rows per stage
constexpr int kLd = 80;              // wsyrk LDS row, doubles
constexpr int kTChunk = 1024;        // tall_v: rows of T per LDS stage
constexpr int kTvUnitRows = 4;       // tall_v: rows per unit
constexpr int kMaxR = 4;             // thin products: right-hand sides
constexpr int kRbfResD = 32;         // rbf_decision: features of the resident X block

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool better(double v, int64_t i, double bv, int64_t bi) {
  return v > bv || (v == bv && i < bi);
}

// arg-max over the workgroup's candidates, result in bv[0] / bi[0]
__device__ __forceinline__ void block_argmax(double* bv, int64_t* bi, int tid) {
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (tid < off && better(bv[tid + off], bi[tid + off], bv[tid], bi[tid])) {
      bv[tid] = bv[tid + off];
      bi[tid] = bi[tid + off];
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------ ICF

// rec_i: pivot row, stop flag, columns written, then the pivot row of every
// column.  rec_v: pivot value, xp . xp.
__global__ void icf_init_kernel(double* __restrict__ diag, int64_t n, int64_t* __restrict__ rec_i,
                                double* __restrict__ rec_v, double* __restrict__ part_v,
                                int64_t* __restrict__ part_i) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) diag[i] = 1.0;   // K(x, x) of the Gaussian kernel
  if (i == 0) {
    rec_i[0] = 0; rec_i[1] = 0; rec_i[2] = 0;
    rec_v[0] = 0.0; rec_v[1] = 0.0;
    part_v[0] = 1.0;
    part_i[0] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void icf_pivot_kernel(
    const double* __restrict__ X, const double* __restrict__ H, int d, int p, int k, int nparts, double thresh,
    const double* __restrict__ part_v, const int64_t* __restrict__ part_i, int64_t* __restrict__ rec_i,
    double* __restrict__ rec_v, double* __restrict__ xp, double* __restrict__ hp) {
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  if (rec_i[1]) return;
  double v = -1.0;
  int64_t row = INT64_MAX;
  for (int j = tid; j < nparts; j += kThreads)
    if (better(part_v[j], part_i[j], v, row)) { v = part_v[j]; row = part_i[j]; }
  bv[tid] = v;
  bi[tid] = row;
  block_argmax(bv, bi, tid);
  v = bv[0];
  row = bi[0];
  if (v < thresh) {
    if (tid == 0) rec_i[1] = 1;
    return;
  }
  double s = 0.0;
  for (int j = tid; j < d; j += kThreads) {
    const double x = X[row * d + j];
    xp[j] = x;
    s += x * x;
  }
  for (int j = tid; j < k; j += kThreads) hp[j] = H[row * p + j];
  __syncthreads();
  bv[tid] = s;
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (tid < off) bv[tid] += bv[tid + off];
  }
  if (tid == 0) {
    rec_i[0] = row;
    rec_i[2] = k + 1;
    rec_i[3 + k] = row;
    rec_v[0] = v;
    rec_v[1] = bv[0];
  }
}

__global__ __launch_bounds__(kThreads) void icf_step_kernel(
    const double* __restrict__ X, const double* __restrict__ xsq, double* H, double* __restrict__ diag, int64_t n,
    int d, int p, int k, int U, double gamma, const double* __restrict__ xp_g, const double* __restrict__ hp_g,
    const int64_t* __restrict__ rec_i, const double* __restrict__ rec_v, double* __restrict__ part_v,
    int64_t* __restrict__ part_i) {
  __shared__ double xp[kMaxD];
  __shared__ double hp[kMaxP];
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  if (rec_i[1]) return;
  for (int j = tid; j < d; j += kThreads) xp[j] = xp_g[j];
  for (int j = tid; j < k; j += kThreads) hp[j] = hp_g[j];
  __syncthreads();
  const int64_t prow = rec_i[0];
  const double piv = sqrt(rec_v[0]), xpp = rec_v[1];
  const int c = tid & (U - 1), u = tid / U, NU = kThreads / U;
  const int64_t b0 = (int64_t)blockIdx.x * NU * kIcfUnitRows;
  double best = -1.0;
  int64_t besti = INT64_MAX;
  for (int q = 0; q < kIcfUnitRows; ++q) {
    const int64_t i = b0 + (int64_t)q * NU + u;   // ascending within the unit
    const bool live = i < n;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
      const double* xr = X + i * d;
      for (int j = c; j < d; j += U) s1 += xr[j] * xp[j];
      const double* hr = H + i * p;
      for (int j = c; j < k; j += U) s2 += hr[j] * hp[j];
    }
    for (int off = U >> 1; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off, kWave);
      s2 += __shfl_xor(s2, off, kWave);
    }
    if (live && c == 0) {
      double d2 = xsq[i] - 2.0 * s1 + xpp;
      d2 = d2 > 0.0 ? d2 : 0.0;
      double h = (exp(-gamma * d2) - s2) / piv;
      double nd = diag[i] - h * h;
      nd = nd > 0.0 ? nd : 0.0;
      if (i == prow) { h = piv; nd = 0.0; }
      H[i * p + k] = h;
      diag[i] = nd;
      if (nd > best) { best = nd; besti = i; }
    }
  }
  bv[tid] = best;
  bi[tid] = besti;
  block_argmax(bv, bi, tid);
  if (tid == 0) {
    part_v[blockIdx.x] = bv[0];
    part_i[blockIdx.x] = bi[0];
  }
}

// ---------------------------------------------------------------------- wsyrk

// block pair (bi <= bj) of a linear index, row by row over the upper triangle
__device__ __forceinline__ void block_pair(int idx, int nbc, int& bi, int& bj) {
  bi = 0;
  while (idx >= nbc - bi) { idx -= nbc - bi; ++bi; }
  bj = bi + idx;
}

__global__ __launch_bounds__(kThreads) void wsyrk_kernel(const double* __restrict__ A, const double* __restrict__ w,
                                                         int64_t n, int k, int64_t slab_rows, int nbc,
                                                         double* __restrict__ part) {
  __shared__ double sL[2][kChunk * kLd];
  __shared__ double sR[2][kChunk * kLd];
  int bi, bj;
  block_pair(blockIdx.x, nbc, bi, bj);
  const bool dg = bi == bj;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tr = (wave >> 1) * 2, tc = (wave & 1) * 2;
  const bool active = !(dg && wave == 2);
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  const int sc = tid & (kBlk - 1), sr = tid / kBlk;   // stage: column, first row
  const int colL = bi * kBlk + sc, colR = bj * kBlk + sc;
  const bool okL = colL < k, okR = colR < k;
  double gl[4], gr[4];
  auto load = [&](int64_t t0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = t0 + sr + 4 * q;
      const bool v = row < r1;
      const double wv = v ? w[row] : 0.0;
      const double a = (v && okL) ? A[row * k + colL] : 0.0;
      gr[q] = dg ? a : ((v && okR) ? A[row * k + colR] : 0.0);
      gl[q] = wv * a;
    }
  };
  auto store = [&](int b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sL[b][(sr + 4 * q) * kLd + sc] = gl[q];
      sR[b][(sr + 4 * q) * kLd + sc] = gr[q];
    }
  };
  d4 c00 = {0, 0, 0, 0}, c01 = c00, c10 = c00, c11 = c00;
  load(r0);
  store(0);
  __syncthreads();
  int b = 0;
  const int oa = tr * 16 + (lane & 15), ob = tc * 16 + (lane & 15);
  for (int64_t t0 = r0; t0 < r1; t0 += kChunk) {
    const bool more = t0 + kChunk < r1;
    if (more) load(t0 + kChunk);
    if (active) {
#pragma unroll
      for (int kk = 0; kk < kChunk / 4; ++kk) {
        const int ro = (4 * kk + (lane >> 4)) * kLd;
        const double a0 = sL[b][ro + oa], a1 = sL[b][ro + oa + 16];
        const double b0 = sR[b][ro + ob], b1 = sR[b][ro + ob + 16];
        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);
      }
    }
    if (more) store(b ^ 1);
    __syncthreads();
    b ^= 1;
  }
  if (!active) return;
  // register v of a tile holds C[4 v + lane / 16][lane % 16]
  double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kBlk * kBlk);
  const int j = tc * 16 + (lane & 15);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int i = tr * 16 + 4 * v + (lane >> 4);
    out[i * kBlk + j] = c00[v];
    out[i * kBlk + j + 16] = c01[v];
    out[(i + 16) * kBlk + j] = c10[v];
    out[(i + 16) * kBlk + j + 16] = c11[v];
  }
}

// one thread per element on or above the diagonal: the slabs in order
__global__ __launch_bounds__(kThreads) void wsyrk_fold_kernel(const double* __restrict__ part, int slabs, int pairs,
                                                              int nbc, int k, double* __restrict__ C) {
  int bi, bj;
  block_pair(blockIdx.x, nbc, bi, bj);
  const int e = blockIdx.y * kThreads + threadIdx.x;
  const int i = e / kBlk, j = e % kBlk;
  const int gi = bi * kBlk + i, gj = bj * kBlk + j;
  if (gi >= k || gj >= k || gi > gj) return;
  double s = 0.0;
  for (int q = 0; q < slabs; ++q) s += part[((int64_t)q * pairs + blockIdx.x) * (kBlk * kBlk) + e];
  C[(int64_t)gi * k + gj] = s;
  C[(int64_t)gj * k + gi] = s;
}

// -------------------------------------------------------------- thin products

// part[slab][k][r] = sum over the slab's rows of s_i A[i][col] V[i][:].  A
// workgroup is CW column lanes by 256 / CW row groups; group g takes rows
// g, g + G, ... of the slab and the groups are added in group order.
__global__ __launch_bounds__(kThreads) void tall_tv_kernel(const double* __restrict__ A, const double* __restrict__ s,
                                                           const double* __restrict__ V, int64_t n, int k, int r,
                                                           int CW, int64_t slab_rows, double* __restrict__ part) {
  __shared__ double red[kMaxR][kThreads];
  const int tid = threadIdx.x;
  const int c = tid & (CW - 1), g = tid / CW, G = kThreads / CW;
  const int col = blockIdx.x * CW + c;
  const bool ok = col < k;
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  double acc[kMaxR] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int64_t i = r0 + g; i < r1; i += G) {
    double a = ok ? A[i * k + col] : 0.0;
    if (s) a *= s[i];
#pragma unroll
    for (int q = 0; q < kMaxR; ++q)
      if (q < r) acc[q] += a * V[i * r + q];
  }
#pragma unroll
  for (int q = 0; q < kMaxR; ++q) red[q][tid] = acc[q];
  __syncthreads();
  if (g == 0 && ok) {
    for (int q = 0; q < r; ++q) {
      double t = 0.0;
      for (int gg = 0; gg < G; ++gg) t += red[q][gg * CW + c];
      part[((int64_t)blockIdx.y * k + col) * r + q] = t;
    }
  }
}

__global__ void tall_fold_kernel(const double* __restrict__ part, int slabs, int64_t len, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  double t = 0.0;
  for (int q = 0; q < slabs; ++q) t += part[(int64_t)q * len + e];
  out[e] = t;
}

// out[i][:] = s_i A[i][:] T, T [k][r] staged in LDS kTChunk rows at a time
__global__ __launch_bounds__(kThreads) void tall_v_kernel(const double* __restrict__ A, const double* __restrict__ s,
                                                          const double* __restrict__ T, int64_t n, int k, int r,
                                                          int U, double* __restrict__ out) {
  __shared__ double sT[kTChunk * kMaxR];
  const int tid = threadIdx.x;
  const int c = tid & (U - 1), u = tid / U, NU = kThreads / U;
  const int64_t b0 = (int64_t)blockIdx.x * NU * kTvUnitRows;
  double acc[kTvUnitRows][kMaxR] = {};
  for (int k0 = 0; k0 < k; k0 += kTChunk) {
    const int kc = k - k0 < kTChunk ? k - k0 : kTChunk;
    __syncthreads();
    for (int j = tid; j < kc * r; j += kThreads) sT[j] = T[(int64_t)k0 * r + j];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kTvUnitRows; ++q) {
      const int64_t i = b0 + (int64_t)q * NU + u;
      if (i < n) {
        const double* ar = A + i * k + k0;
        for (int j = c; j < kc; j += U) {
          const double a = ar[j];
#pragma unroll
          for (int m = 0; m < kMaxR; ++m)
            if (m < r) acc[q][m] += a * sT[j * r + m];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kTvUnitRows; ++q) {
    const int64_t i = b0 + (int64_t)q * NU + u;
#pragma unroll
    for (int m = 0; m < kMaxR; ++m) {
      double t = acc[q][m];
      for (int off = U >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
      if (i < n && c == 0 && m < r) out[i * r + m] = s ? s[i] * t : t;
    }
  }
}

// ------------------------------------------------------------- rbf decision

__global__ __launch_bounds__(kThreads) void rbf_sqnorm_kernel(const float* __restrict__ A, int64_t n, int d,
                                                              double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* a = A + i * d;
  double s = 0.0;
  for (int j = 0; j < d; ++j) s += (double)a[j] * (double)a[j];
  out[i] = s;
}

// dst[slab][n]; one slab: dst is the result
template <bool kResident>
__global__ __launch_bounds__(kThreads) void rbf_decision_kernel(
    const float* __restrict__ X, const float* __restrict__ S, const double* __restrict__ coef,
    const double* __restrict__ xsq, const double* __restrict__ ssq, int64_t n, int64_t nsv, int d, int64_t slab_svs,
    double gamma, double* __restrict__ dst) {
  __shared__ double sS[2][kChunk * kLd];
  __shared__ double sX[kResident ? kRbfResD / kChunk : 2][kChunk * kLd];
  __shared__ double sQ[2][kBlk], sCf[2][kBlk];   // |s_j|^2 and coef_j of a tile, by tile parity
  __shared__ double sF[4][32];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tr = (wave >> 1) * 2, tc = (wave & 1) * 2;
  const int64_t i0 = (int64_t)blockIdx.x * kBlk;
  const int64_t j0 = (int64_t)blockIdx.y * slab_svs;
  const int64_t j1 = j0 + slab_svs < nsv ? j0 + slab_svs : nsv;
  const int nch = (d + kChunk - 1) / kChunk;
  const int sp = tid & (kBlk - 1), sf = (tid / kBlk) * 4;   // stage: point, first feature of the chunk
  const bool okx = i0 + sp < n;
  const float* xrow = X + (i0 + sp) * d;
  float gs[4], gx[4];
  double gq = 0.0, gc = 0.0;
  auto load_x = [&](int c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = c * kChunk + sf + q;
      gx[q] = (okx && col < d) ? xrow[col] : 0.f;
    }
  };
  auto store_x = [&](double* sx) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sx[(sf + q) * kLd + sp] = (double)gx[q];
  };
  auto load_s = [&](int64_t t0, int c) {
    const int64_t j = t0 + sp;
    const bool ok = j < j1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = c * kChunk + sf + q;
      gs[q] = (ok && col < d) ? S[j * d + col] : 0.f;
    }
    if (c == 0 && tid < kBlk) {
      gq = ok ? ssq[j] : 0.0;
      gc = ok ? coef[j] : 0.0;
    }
  };
  auto store_s = [&](int b, int c, int par) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sS[b][(sf + q) * kLd + sp] = (double)gs[q];
    if (c == 0 && tid < kBlk) {
      sQ[par][tid] = gq;
      sCf[par][tid] = gc;
    }
  };
  if (kResident) {
    for (int c = 0; c < nch; ++c) {
      load_x(c);
      store_x(sX[c]);
    }
  } else {
    load_x(0);
    store_x(sX[0]);
  }
  load_s(j0, 0);
  store_s(0, 0, 0);
  const int64_t ra = i0 + tc * 16 + (lane & 15);
  const double xs0 = ra < n ? xsq[ra] : 0.0, xs1 = ra + 16 < n ? xsq[ra + 16] : 0.0;
  const double ng = -gamma;
  __syncthreads();
  d4 c00 = {0, 0, 0, 0}, c01 = c00, c10 = c00, c11 = c00;
  double f0 = 0.0, f1 = 0.0;
  const int oa = tr * 16 + (lane & 15), ob = tc * 16 + (lane & 15);
  int b = 0, c = 0, par = 0;
  int64_t t0 = j0;
  for (;;) {
    int cn = c + 1;
    int64_t tn = t0;
    if (cn == nch) { cn = 0; tn += kBlk; }
    const bool more = tn < j1;
    if (more) {
      load_s(tn, cn);
      if (!kResident) load_x(cn);
    }
    const double* sx = kResident ? sX[c] : sX[b];
    const int ks = (d - c * kChunk + 3) / 4;
#pragma unroll
    for (int kk = 0; kk < kChunk / 4; ++kk) {
      if (kk >= ks) break;
      const int ro = (4 * kk + (lane >> 4)) * kLd;
      const double a0 = sS[b][ro + oa], a1 = sS[b][ro + oa + 16];
      const double b0 = sx[ro + ob], b1 = sx[ro + ob + 16];
      c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);
    }
    if (c == nch - 1) {
      // register v of a tile holds C[4 v + lane / 16][lane % 16]: SV 4 v + lane / 16, scored row lane % 16
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int j = tr * 16 + 4 * v + (lane >> 4);
        const double q0 = sQ[par][j], q1 = sQ[par][j + 16];
        const double w0 = sCf[par][j], w1 = sCf[par][j + 16];
        double e;
        e = xs0 + q0 - 2.0 * c00[v]; f0 += w0 * exp(ng * (e > 0.0 ? e : 0.0));
        e = xs1 + q0 - 2.0 * c01[v]; f1 += w0 * exp(ng * (e > 0.0 ? e : 0.0));
        e = xs0 + q1 - 2.0 * c10[v]; f0 += w1 * exp(ng * (e > 0.0 ? e : 0.0));
        e = xs1 + q1 - 2.0 * c11[v]; f1 += w1 * exp(ng * (e > 0.0 ? e : 0.0));
      }
      c00 = d4{0, 0, 0, 0}; c01 = c00; c10 = c00; c11 = c00;
    }
    if (more) {
      store_s(b ^ 1, cn, par ^ 1);
      if (!kResident) store_x(sX[b ^ 1]);
    }
    __syncthreads();
    if (!more) break;
    b ^= 1;
    if (cn == 0) par ^= 1;
    c = cn;
    t0 = tn;
  }
  // the four lane groups, then the two waves that share the rows
  f0 += __shfl_xor(f0, 16, kWave);
  f1 += __shfl_xor(f1, 16, kWave);
  f0 += __shfl_xor(f0, 32, kWave);
  f1 += __shfl_xor(f1, 32, kWave);
  if (lane < 16) {
    sF[wave][lane] = f0;
    sF[wave][lane + 16] = f1;
  }
  __syncthreads();
  if (tid < kBlk && i0 + tid < n) {
    const int h = tid >> 5, r = tid & 31;
    dst[(int64_t)blockIdx.y * n + i0 + tid] = sF[h][r] + sF[h + 2][r];
  }
}

__global__ __launch_bounds__(kThreads) void rbf_decision_fold_kernel(const double* __restrict__ part, int slabs,
                                                                     int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double t = 0.0;
  for (int q = 0; q < slabs; ++q) t += part[(int64_t)q * n + i];
  out[i] = t;
}

int unit_lanes(int len) {   // power of two, 1 .. 64, covering len where it can
  int v = 1;
  while (v < len && v < kWave) v <<= 1;
  return v;
}

}  // namespace

// Pivoted incomplete Cholesky of exp(-gamma |x_i - x_j|^2) over the rows of X [n][d],
// up to p columns, into H [n][p]; stops at the first pivot below thresh.  After the
// call rec_i[2] holds the number of columns written and rec_i[3 ..] their pivot rows.
// xsq [n] = row norms squared.
// Work: diag [n], part_v / part_i [ceil(n / 64)], rec_i [3 + p], rec_v [2], xp [d], hp [p].
H2OMX_API int h2omx_svm_icf(const double* X, const double* xsq, int64_t n, int d, int p, double gamma,
                            double thresh, double* H, double* diag, double* part_v, int64_t* part_i,
                            int64_t* rec_i, double* rec_v, double* xp, double* hp, hipStream_t stream) {
  if (n < 1 || d < 1 || d > kMaxD || p < 1 || p > kMaxP) return kBadArg;
  icf_init_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(diag, n, rec_i, rec_v, part_v,
                                                                                      part_i);
  int nparts = 1;
  for (int k = 0; k < p; ++k) {
    icf_pivot_kernel<<<1, kThreads, 0, stream>>>(X, H, d, p, k, nparts, thresh, part_v, part_i, rec_i, rec_v, xp, hp);
    const int U = unit_lanes(k > d ? k : d);
    const int64_t rows = (int64_t)(kThreads / U) * kIcfUnitRows;
    nparts = (int)((n + rows - 1) / rows);
    icf_step_kernel<<<nparts, kThreads, 0, stream>>>(X, xsq, H, diag, n, d, p, k, U, gamma, xp, hp, rec_i, rec_v,
                                                     part_v, part_i);
  }
  return launch_status();
}

// C [k][k] = A^T diag(w) A for A [n][k] row-major, exactly symmetric.
// part: [slabs][pairs][64 * 64] doubles, slabs = ceil(n / slab_rows), pairs = nbc (nbc + 1) / 2,
// nbc = ceil(k / 64).
H2OMX_API int h2omx_svm_wsyrk(const double* A, const double* w, int64_t n, int k, int64_t slab_rows, double* part,
                              double* C, hipStream_t stream) {
  if (n < 1 || k < 1 || slab_rows < 1) return kBadArg;
  const int nbc = (k + kBlk - 1) / kBlk;
  const int pairs = nbc * (nbc + 1) / 2;
  const int64_t slabs = (n + slab_rows - 1) / slab_rows;
  if (slabs > 65535) return kBadArg;
  wsyrk_kernel<<<dim3(pairs, (unsigned)slabs), kThreads, 0, stream>>>(A, w, n, k, slab_rows, nbc, part);
  wsyrk_fold_kernel<<<dim3(pairs, kBlk * kBlk / kThreads), kThreads, 0, stream>>>(part, (int)slabs, pairs, nbc, k, C);
  return launch_status();
}

// out [k][r] = A^T diag(s) V, V [n][r], r <= 4; s null: ones.  part: [slabs][k][r].
H2OMX_API int h2omx_svm_tall_tv(const double* A, const double* s, const double* V, int64_t n, int k, int r,
                                int64_t slab_rows, double* part, double* out, hipStream_t stream) {
  if (n < 1 || k < 1 || r < 1 || r > kMaxR || slab_rows < 1) return kBadArg;
  const int64_t slabs = (n + slab_rows - 1) / slab_rows;
  if (slabs > 65535) return kBadArg;
  const int CW = unit_lanes(k);
  tall_tv_kernel<<<dim3((k + CW - 1) / CW, (unsigned)slabs), kThreads, 0, stream>>>(A, s, V, n, k, r, CW, slab_rows,
                                                                                    part);
  const int64_t len = (int64_t)k * r;
  tall_fold_kernel<<<(unsigned)((len + kThreads - 1) / kThreads), kThreads, 0, stream>>>(part, (int)slabs, len, out);
  return launch_status();
}

// out [n][r] = diag(s) A T, T [k][r], r <= 4; s null: ones.
H2OMX_API int h2omx_svm_tall_v(const double* A, const double* s, const double* T, int64_t n, int k, int r,
                               double* out, hipStream_t stream) {
  if (n < 1 || k < 1 || r < 1 || r > kMaxR) return kBadArg;
  const int U = unit_lanes(k);
  const int64_t rows = (int64_t)(kThreads / U) * kTvUnitRows;
  tall_v_kernel<<<(unsigned)((n + rows - 1) / rows), kThreads, 0, stream>>>(A, s, T, n, k, r, U, out);
  return launch_status();
}

// out [n] = sum_j coef_j exp(-gamma |x_i - s_j|^2) for X [n][d] and S [nsv][d] fp32, coef [nsv] fp64,
// gamma > 0.  Work: xsq [n], ssq [nsv]; part [slabs][n] with slabs = ceil(nsv / slab_svs), unused
// (may be null) with one slab.
H2OMX_API int h2omx_svm_rbf_decision(const float* X, const float* S, const double* coef, int64_t n, int64_t nsv, int d,
                                     double gamma, int64_t slab_svs, double* xsq, double* ssq, double* part,
                                     double* out, hipStream_t stream) {
  if (n < 1 || nsv < 1 || d < 1 || slab_svs < 1 || !(gamma > 0.0)) return kBadArg;
  const int64_t slabs = (nsv + slab_svs - 1) / slab_svs;
  const int64_t blocks = (n + kBlk - 1) / kBlk;
  if (slabs > 65535 || blocks > INT32_MAX) return kBadArg;
  rbf_sqnorm_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(X, n, d, xsq);
  rbf_sqnorm_kernel<<<(unsigned)((nsv + kThreads - 1) / kThreads), kThreads, 0, stream>>>(S, nsv, d, ssq);
  double* dst = slabs > 1 ? part : out;
  const dim3 grid((unsigned)blocks, (unsigned)slabs);
  if (d <= kRbfResD)
    rbf_decision_kernel<true><<<grid, kThreads, 0, stream>>>(X, S, coef, xsq, ssq, n, nsv, d, slab_svs, gamma, dst);
  else
    rbf_decision_kernel<false><<<grid, kThreads, 0, stream>>>(X, S, coef, xsq, ssq, n, nsv, d, slab_svs, gamma, dst);
  if (slabs > 1)
    rbf_decision_fold_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(part, (int)slabs, n,
                                                                                                 out);
  return launch_status();
}
