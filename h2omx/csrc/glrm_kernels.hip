// GLRM with missing entries on gfx950, all fp64: the per-row (X-step) and
// per-column (Y-step) normal equations of masked ALS as one product each on
// v_mfma_f64_16x16x4_f64, the row systems solved before they leave LDS.
//
//   glrm_xstep_kernel        G_i = sum_j m_ji y_j y_j^T + lam I, r_i = sum_j a_ji y_j
//                            and x_i = G_i^-1 r_i for a block of rows
//   glrm_bad_fold_kernel     the blocks' counts of failed pivots, added
//   glrm_yterms_kernel       [G_j | r_j] = sum_i m_ji x_i x_i^T | sum_i a_ji x_i for
//                            16 data columns over one slab of rows
//   glrm_yterms_fold_kernel  slabs added in slab order, both triangles written
//
// Nothing here uses a floating-point atomic or waits for another workgroup;
// every sum has a fixed order, so results are bit-identical between calls.
//
// The product.  With T = k (k + 1) / 2 pairs a <= b, the upper triangles of all
// G are (mask as 0 / 1)^T Z with Z[j][(a, b)] = Y[a][j] Y[b][j], and all r are
// A^T Y^T.  Z is never stored: the lane that supplies column (a, b) of the right
// operand multiplies two LDS values.  Both factors are fp32 widened to fp64, so
// the product is exact, as are the 0 / 1 mask and the widened A: only the
// additions round.  The pair columns are padded to whole 16-column tiles, so a
// tile's left operand is either the mask (pair tiles) or A (the tiles of r);
// the factor stage has a column of zeros (padding columns) and a column of ones
// (r = Y[a][j] * 1), which keeps one code path for every tile.
//
// X-step.  A workgroup of four waves owns 16 RT consecutive rows and walks p
// in chunks of 16 data columns, lanes along n, double buffered as wsyrk_kernel
// is: global loads of the next chunk before the matrix instructions of this
// one, LDS writes after, one barrier per chunk.  Column tile t belongs to wave
// t % 4; a wave keeps RT x CT accumulators.  The epilogue moves the
// accumulators to LDS E rows at a time ([row][Tc | 1] doubles, lam added on the
// diagonal) and solves every row with a unit of U lanes, U the power of two
// covering k: lane a owns row a of the Cholesky factor, which overwrites the
// row's upper triangle in place (L[a][m] where G[m][a] was).  Column c takes one
// dot product per lane against row c, read from LDS after the barrier that
// follows column c - 1; the pivot travels by a cross-lane move.  Forward
// substitution pushes z_c to the lanes below it, back substitution folds the
// unit's terms by a butterfly.  x goes to the row's r slot and from there to
// X[a][i] with lanes along i.
//
// Y-terms.  A workgroup owns 16 data columns over one slab of rows and stages
// 32 rows at a time: mask and A as [16][32], X as [32][k].  The left operand is
// the mask or A of (j, i), the right one X[a][i] X[b][i].
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 32;
constexpr int kZero = kMaxK;         // factor stage: column of zeros
constexpr int kOne = kMaxK + 1;      // factor stage: column of ones
constexpr int kLdF = kMaxK + 2;      // factor stage row, doubles
constexpr int kPC = 16;              // x-step: data columns per stage
constexpr int kNC = 32;              // y-terms: rows per stage
constexpr int kLdN = 36;             // y-terms: LDS row of mask / A, doubles
constexpr int kSmemX = 4 * kPC * 80 + 2 * kPC * kLdF;   // x-step LDS, doubles (stage at RT = 4)
constexpr int kSmemY = 4 * 16 * kLdN + 2 * kNC * kLdF;  // y-terms LDS, doubles

typedef double d4 __attribute__((ext_vector_type(4)));

// pair (a <= b) of a linear index, row by row over the upper triangle
__device__ __forceinline__ void pair_of(int t, int k, int& a, int& b) {
  a = 0;
  while (t >= k - a) { t -= k - a; ++a; }
  b = a + t;
}

// index of (m, a), m <= a, in the packed upper triangle, less a
__device__ __forceinline__ int packed_row(int m, int k) { return m * k - m * (m - 1) / 2 - m; }

// The columns of this lane in the wave's CT tiles: the two factor columns whose
// product is the right operand, and the column's place in a [Tc] row (-1: padding).
template <int CT>
__device__ __forceinline__ void tile_columns(int k, int T, int ntp, int nt, int wave, int lane, int (&ia)[CT],
                                             int (&ib)[CT], int (&off)[CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int tile = wave + 4 * ct, c = lane & 15;
    ia[ct] = ib[ct] = kZero;
    off[ct] = -1;
    if (tile < ntp) {
      const int t = tile * 16 + c;
      if (t < T) {
        pair_of(t, k, ia[ct], ib[ct]);
        off[ct] = t;
      }
    } else if (tile < nt) {
      const int a = (tile - ntp) * 16 + c;
      if (a < k) {
        ia[ct] = a;
        ib[ct] = kOne;
        off[ct] = T + a;
      }
    }
  }
}

// the constant columns of both buffers of a factor stage of `rows` rows
__device__ __forceinline__ void factor_constants(double* sF, int rows, int tid) {
  for (int e = tid; e < 2 * rows; e += kThreads) {
    sF[e * kLdF + kZero] = 0.0;
    sF[e * kLdF + kOne] = 1.0;
  }
}

// --------------------------------------------------------------------- X-step

template <int RT, int CT>
__global__ __launch_bounds__(kThreads) void glrm_xstep_kernel(const float* __restrict__ A,
                                                              const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ Y, int64_t n, int p, int k,
                                                              int U, int E, double lam, float* __restrict__ X,
                                                              int* __restrict__ bad_part) {
  constexpr int R = 16 * RT;                 // rows of the block
  constexpr int LD = RT == 1 ? 16 : R + 16;  // LDS row: 2 LD = 32 (mod 64) banks
  constexpr int STEP = kThreads / R;         // data columns staged per pass of the threads
  static_assert(kPC / STEP == RT && 4 * kPC * LD + 2 * kPC * kLdF <= kSmemX, "stage");
  __shared__ double smem[kSmemX];
  __shared__ int sbad[kThreads / kWave];
  double* const sL = smem;                       // [2][mask, A][kPC][LD]
  double* const sF = smem + 4 * kPC * LD;        // [2][kPC][kLdF]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int T = k * (k + 1) / 2, Tc = T + k, ntp = (T + 15) / 16, nt = ntp + (k + 15) / 16;
  const int64_t i0 = (int64_t)blockIdx.x * R;
  int ia[CT], ib[CT], off[CT];
  tile_columns<CT>(k, T, ntp, nt, wave, lane, ia, ib, off);

  const int sc = tid % R, sr = tid / R;          // stage: row, first data column
  const int ya = tid / kPC, yj = tid % kPC;      // stage of Y: factor, data column
  const bool iv = i0 + sc < n;
  double gm[RT], ga[RT], gy[2];
  auto load = [&](int j0) {
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int j = j0 + sr + q * STEP;
      const bool ok = iv && j < p;
      const int64_t idx = (int64_t)j * n + i0 + sc;
      const bool m = ok && mask[idx] != 0;
      gm[q] = m ? 1.0 : 0.0;
      ga[q] = m ? (double)A[idx] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int a = ya + 16 * q, j = j0 + yj;
      gy[q] = (a < k && j < p) ? (double)Y[(int64_t)a * p + j] : 0.0;
    }
  };
  auto store = [&](int b) {
    double* const m = sL + b * 2 * kPC * LD;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      m[(sr + q * STEP) * LD + sc] = gm[q];
      m[kPC * LD + (sr + q * STEP) * LD + sc] = ga[q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) sF[b * kPC * kLdF + yj * kLdF + ya + 16 * q] = gy[q];
  };

  d4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = d4{0, 0, 0, 0};
  factor_constants(sF, kPC, tid);
  load(0);
  store(0);
  __syncthreads();
  int b = 0;
  for (int j0 = 0; j0 < p; j0 += kPC) {
    const bool more = j0 + kPC < p;
    if (more) load(j0 + kPC);
    const double* const m = sL + b * 2 * kPC * LD;
    const double* const f = sF + b * kPC * kLdF;
#pragma unroll
    for (int kk = 0; kk < kPC / 4; ++kk) {
      const int jj = 4 * kk + (lane >> 4);
      double lm[RT], la[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        lm[rt] = m[jj * LD + rt * 16 + (lane & 15)];
        la[rt] = m[kPC * LD + jj * LD + rt * 16 + (lane & 15)];
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int tile = wave + 4 * ct;
        if (tile < nt) {
          const double rgt = f[jj * kLdF + ia[ct]] * f[jj * kLdF + ib[ct]];
          const bool pairs = tile < ntp;
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(pairs ? lm[rt] : la[rt], rgt, acc[rt][ct], 0, 0, 0);
        }
      }
    }
    if (more) store(b ^ 1);
    __syncthreads();
    b ^= 1;
  }

  // epilogue: E rows at a time through LDS, a unit of U lanes per row
  const int ldG = Tc | 1;
  const int a = tid & (U - 1), unit = tid / U, units = kThreads / U;
  const bool live = a < k;
  int nbad = 0;
  for (int e0 = 0; e0 < R; e0 += E) {
    const int ep = e0 + E < R ? E : R - e0;
    __syncthreads();
    // register v of a tile holds C[4 v + lane / 16][lane % 16]
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int grp = rt * 16 + 4 * v;
        if (grp >= e0 && grp < e0 + ep) {
          double* const g = smem + (grp - e0 + (lane >> 4)) * ldG;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            if (off[ct] >= 0) g[off[ct]] = acc[rt][ct][v] + (ia[ct] == ib[ct] ? lam : 0.0);
        }
      }
    __syncthreads();
    for (int r0 = 0; r0 < ep; r0 += units) {       // the same trips for every thread: barriers inside
      const int r = r0 + unit;
      const bool act = live && r < ep;
      double* const g = smem + (r < ep ? r : 0) * ldG;
      bool ok = true;
      double inv = 1.0;
      for (int c = 0; c < k; ++c) {
        double s = 0.0;
        if (act && a >= c) {
          s = g[packed_row(c, k) + a];
          int base = 0;
          for (int m = 0; m < c; ++m) {
            s -= g[base + a] * g[base + c];
            base += k - m - 1;
          }
        }
        double piv = __shfl(s, c, U);
        if (!(piv > 0.0 && piv < __builtin_huge_val())) {
          ok = false;
          piv = 1.0;
        }
        const double d = sqrt(piv);
        if (a == c) inv = 1.0 / d;
        if (act && a >= c) g[packed_row(c, k) + a] = a == c ? d : s / d;
        __syncthreads();
      }
      // L z = r, z_c pushed to the lanes below c; then L^T x = z, the unit's terms folded
      double z = act ? g[T + a] : 0.0;
      for (int c = 0; c < k; ++c) {
        const double zc = __shfl(z * inv, c, U);
        if (a == c) z = zc;
        if (act && a > c) z -= g[packed_row(c, k) + a] * zc;
      }
      double x = 0.0;
      for (int c = k - 1; c >= 0; --c) {
        double t = (act && a > c) ? g[packed_row(c, k) + a] * x : 0.0;
        for (int o = U >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, U);
        if (a == c) x = (z - t) * inv;
      }
      if (act) g[T + a] = x;
      if (a == 0 && r < ep && i0 + e0 + r < n && !ok) ++nbad;
    }
    __syncthreads();
    for (int e = tid; e < k * ep; e += kThreads) {
      const int xa = e / ep, r = e % ep;
      const int64_t i = i0 + e0 + r;
      if (i < n) X[(int64_t)xa * n + i] = (float)smem[r * ldG + T + xa];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, kWave);
  if (lane == 0) sbad[wave] = nbad;
  __syncthreads();
  if (tid == 0) bad_part[blockIdx.x] = sbad[0] + sbad[1] + sbad[2] + sbad[3];
}

__global__ __launch_bounds__(kThreads) void glrm_bad_fold_kernel(const int* __restrict__ bad_part, int64_t blocks,
                                                                 int* __restrict__ bad) {
  __shared__ int sbad[kThreads / kWave];
  int s = 0;
  for (int64_t e = threadIdx.x; e < blocks; e += kThreads) s += bad_part[e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) sbad[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) bad[0] = sbad[0] + sbad[1] + sbad[2] + sbad[3];
}

// -------------------------------------------------------------------- Y-terms

template <int CT>
__global__ __launch_bounds__(kThreads) void glrm_yterms_kernel(const float* __restrict__ A,
                                                               const uint8_t* __restrict__ mask,
                                                               const float* __restrict__ X, int64_t n, int p, int k,
                                                               int64_t slab_rows, double* __restrict__ part) {
  __shared__ double smem[kSmemY];
  double* const sL = smem;                       // [2][mask, A][16][kLdN]
  double* const sF = smem + 4 * 16 * kLdN;       // [2][kNC][kLdF]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int T = k * (k + 1) / 2, Tc = T + k, ntp = (T + 15) / 16, nt = ntp + (k + 15) / 16;
  const int j0 = blockIdx.x * 16;
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  int ia[CT], ib[CT], off[CT];
  tile_columns<CT>(k, T, ntp, nt, wave, lane, ia, ib, off);

  const int sn = tid % kNC, sj = tid / kNC;      // stage: row, first data column / factor
  double gm[2], ga[2], gx[4];
  auto load = [&](int64_t t0) {
    const int64_t row = t0 + sn;
    const bool rv = row < r1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = j0 + sj + 8 * q;
      const int64_t idx = (int64_t)j * n + row;
      const bool m = rv && j < p && mask[idx] != 0;
      gm[q] = m ? 1.0 : 0.0;
      ga[q] = m ? (double)A[idx] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = sj + 8 * q;
      gx[q] = (rv && a < k) ? (double)X[(int64_t)a * n + row] : 0.0;
    }
  };
  auto store = [&](int b) {
    double* const m = sL + b * 2 * 16 * kLdN;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      m[(sj + 8 * q) * kLdN + sn] = gm[q];
      m[16 * kLdN + (sj + 8 * q) * kLdN + sn] = ga[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) sF[b * kNC * kLdF + sn * kLdF + sj + 8 * q] = gx[q];
  };

  d4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = d4{0, 0, 0, 0};
  factor_constants(sF, kNC, tid);
  load(r0);
  store(0);
  __syncthreads();
  int b = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += kNC) {
    const bool more = t0 + kNC < r1;
    if (more) load(t0 + kNC);
    const double* const m = sL + b * 2 * 16 * kLdN;
    const double* const f = sF + b * kNC * kLdF;
#pragma unroll
    for (int kk = 0; kk < kNC / 4; ++kk) {
      const int nn = 4 * kk + (lane >> 4);
      const double lm = m[(lane & 15) * kLdN + nn], la = m[16 * kLdN + (lane & 15) * kLdN + nn];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int tile = wave + 4 * ct;
        if (tile < nt) {
          const double rgt = f[nn * kLdF + ia[ct]] * f[nn * kLdF + ib[ct]];
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(tile < ntp ? lm : la, rgt, acc[ct], 0, 0, 0);
        }
      }
    }
    if (more) store(b ^ 1);
    __syncthreads();
    b ^= 1;
  }
  // register v of a tile holds C[4 v + lane / 16][lane % 16]
  double* const out = part + (int64_t)blockIdx.y * p * Tc;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int j = j0 + 4 * v + (lane >> 4);
    if (j < p) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (off[ct] >= 0) out[(int64_t)j * Tc + off[ct]] = acc[ct][v];
    }
  }
}

// one thread per (data column, pair or r entry): the slabs in order, S[j] = [G_j | r_j]
__global__ __launch_bounds__(kThreads) void glrm_yterms_fold_kernel(const double* __restrict__ part, int slabs, int p,
                                                                    int k, double* __restrict__ S) {
  const int T = k * (k + 1) / 2, Tc = T + k;
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x, len = (int64_t)p * Tc;
  if (e >= len) return;
  const int64_t j = e / Tc;
  const int t = (int)(e % Tc);
  double s = 0.0;
  for (int q = 0; q < slabs; ++q) s += part[q * len + e];
  double* const out = S + j * k * (k + 1);
  if (t < T) {
    int a, b;
    pair_of(t, k, a, b);
    out[a * (k + 1) + b] = s;
    out[b * (k + 1) + a] = s;
  } else {
    out[(t - T) * (k + 1) + k] = s;
  }
}

// accumulator tiles per wave: pair tiles plus the tiles of r, dealt over four waves
int tiles_per_wave(int k) {
  const int T = k * (k + 1) / 2;
  return ((T + 15) / 16 + (k + 15) / 16 + 3) / 4;
}

int unit_lanes(int k) {   // power of two covering k
  int v = 1;
  while (v < k) v <<= 1;
  return v;
}

template <int RT, int CT>
void launch_x(const float* A, const uint8_t* mask, const float* Y, int64_t n, int p, int k, double lam, float* X,
              int* bad_part, int* bad, hipStream_t stream) {
  constexpr int R = 16 * RT;
  const int ldG = (k * (k + 1) / 2 + k) | 1;
  int E = (kSmemX / ldG) & ~3;    // rows of the epilogue stage, whole groups of 4
  if (E > R) E = R;
  const int64_t blocks = (n + R - 1) / R;
  glrm_xstep_kernel<RT, CT><<<(unsigned)blocks, kThreads, 0, stream>>>(A, mask, Y, n, p, k, unit_lanes(k), E, lam, X,
                                                                      bad_part);
  glrm_bad_fold_kernel<<<1, kThreads, 0, stream>>>(bad_part, blocks, bad);
}

}  // namespace

// X [k][n] fp32: x_i = (sum_j m_ji y_j y_j^T + lam I)^-1 sum_j a_ji y_j for every row i of the
// feature-major A [p][n] (fp32) with mask [p][n] (bytes, 0 = missing) and Y [k][p] (fp32),
// 1 <= k <= 32.  bad[0]: rows that met a pivot that was not positive and finite.
// Work: bad_part [ceil(n / 16)] int32.
H2OMX_API int h2omx_glrm_masked_x(const float* A, const uint8_t* mask, const float* Y, int64_t n, int p, int k,
                                  double lam, float* X, int* bad_part, int* bad, hipStream_t stream) {
  if (n < 1 || p < 1 || k < 1 || k > kMaxK || (n + 15) / 16 > 0x7fffffff) return kBadArg;
  // rows per block: 64 while 12 accumulators per wave cover the tiles, fewer above
  const int ct = tiles_per_wave(k);
  if (ct <= 1) launch_x<4, 1>(A, mask, Y, n, p, k, lam, X, bad_part, bad, stream);
  else if (ct <= 2) launch_x<4, 2>(A, mask, Y, n, p, k, lam, X, bad_part, bad, stream);
  else if (ct <= 3) launch_x<4, 3>(A, mask, Y, n, p, k, lam, X, bad_part, bad, stream);
  else if (ct <= 5) launch_x<2, 5>(A, mask, Y, n, p, k, lam, X, bad_part, bad, stream);
  else launch_x<1, 9>(A, mask, Y, n, p, k, lam, X, bad_part, bad, stream);
  return launch_status();
}

// S [p][k][k + 1] fp64, S[j] = [sum_i m_ji x_i x_i^T | sum_i a_ji x_i] for X [k][n] (fp32), every
// G_j exactly symmetric.  part: [slabs][p][k (k + 1) / 2 + k] doubles, slabs = ceil(n / slab_rows).
H2OMX_API int h2omx_glrm_masked_y_terms(const float* A, const uint8_t* mask, const float* X, int64_t n, int p, int k,
                                        int64_t slab_rows, double* part, double* S, hipStream_t stream) {
  if (n < 1 || p < 1 || k < 1 || k > kMaxK || slab_rows < 1) return kBadArg;
  const int64_t slabs = (n + slab_rows - 1) / slab_rows;
  if (slabs > 65535) return kBadArg;
  const dim3 grid((p + 15) / 16, (unsigned)slabs);
  const int ct = tiles_per_wave(k);
  if (ct <= 1) glrm_yterms_kernel<1><<<grid, kThreads, 0, stream>>>(A, mask, X, n, p, k, slab_rows, part);
  else if (ct <= 2) glrm_yterms_kernel<2><<<grid, kThreads, 0, stream>>>(A, mask, X, n, p, k, slab_rows, part);
  else if (ct <= 3) glrm_yterms_kernel<3><<<grid, kThreads, 0, stream>>>(A, mask, X, n, p, k, slab_rows, part);
  else if (ct <= 5) glrm_yterms_kernel<5><<<grid, kThreads, 0, stream>>>(A, mask, X, n, p, k, slab_rows, part);
  else glrm_yterms_kernel<9><<<grid, kThreads, 0, stream>>>(A, mask, X, n, p, k, slab_rows, part);
  const int64_t len = (int64_t)p * (k * (k + 1) / 2 + k);
  glrm_yterms_fold_kernel<<<(unsigned)((len + kThreads - 1) / kThreads), kThreads, 0, stream>>>(part, (int)slabs, p, k,
                                                                                               S);
  return launch_status();
}
