// GLRM with generalized losses on gfx950, all fp64: the two sampled products of
// alternating proximal gradient, u_ji = sum_a x_ai y_aj over the OBSERVED entries,
//
//   glrm_lossgrad_x_kernel     gradX[a][i] = sum_j y_aj m_ji L_j'(u_ji, a_ji)  and  sum m L
//   glrm_lossgrad_y_kernel     gradY[a][j] = sum_i x_ai m_ji L_j'(u_ji, a_ji)  and  sum m L,
//                              16 data columns over one slab of rows
//   glrm_lossgrad_fold_kernel  slab partials added in slab order, objective partials
//                              added in a fixed order into one device scalar
//
// Each gradient is product, elementwise derivative, product, on
// v_mfma_f64_16x16x4_f64; the middle never leaves the registers, so nothing of
// size n p is written.  The contract is that of glrm_kernels.hip: A [p][n] fp32
// feature-major with zeros where missing, a byte mask, fp32 factors widened to
// fp64 (their products are exact), k 1..32, no floating-point atomics, no
// workgroup waits for another, every sum in a fixed order.
//
// The layouts.  One matrix instruction takes A[row = lane % 16][kk = lane / 16]
// and B[kk = lane / 16][col = lane % 16]; register v of its result holds
// C[4 v + lane / 16][lane % 16].  Register v of a 16 x 16 result is therefore
// the B operand of step v of a following product whose K runs over the
// result's rows.  Both kernels arrange the first product so that its rows are
// the index the second product sums over (data columns j in the X kernel, rows
// i in the Y kernel): the derivatives are applied to the accumulators in place
// and fed straight back to the matrix unit, with no trip through LDS.
//
// Every data column carries an int32 loss code and a double parameter (Periodic:
// 2 pi / period), staged with the column chunk, so one launch serves any mix.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 32;
constexpr int kPC = 16;              // data columns per chunk (X kernel) and per workgroup (Y kernel)
constexpr int kXR = 64;              // X kernel: rows per workgroup, 16 per wave
constexpr int kNC = 32;              // Y kernel: rows per stage
constexpr int kLdF = 36;             // factor stage row, doubles: [column or row][a], a < 32, zeros from k on
constexpr int kLdA = kXR + 16;       // X kernel: stage row of A / mask, floats (4 rows apart: 16 banks apart)
constexpr int kLdN = 36;             // Y kernel: stage row of A / mask, floats (36 j mod 64 distinct, 4 apart)

enum Loss : int { kQuadratic = 0, kAbsolute = 1, kHuber = 2, kPoisson = 3, kHinge = 4, kLogistic = 5, kPeriodic = 6 };

typedef double d4 __attribute__((ext_vector_type(4)));

// L(u, a) and dL/du of one entry; an unknown code gives NaN (the host refuses it first)
__device__ __forceinline__ void loss_eval(int code, double par, double u, double a, double& L, double& g) {
  const double x = u - a;
  switch (code) {
    case kQuadratic:
      L = x * x;
      g = 2.0 * x;
      break;
    case kAbsolute:
      L = fabs(x);
      g = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
      break;
    case kHuber:
      L = fabs(x) <= 1.0 ? 0.5 * x * x : fabs(x) - 0.5;
      g = x > 1.0 ? 1.0 : (x < -1.0 ? -1.0 : x);
      break;
    case kPoisson: {
      const double e = exp(u);
      L = e - a * u + (a > 0.0 ? a * log(a) - a : 0.0);
      g = e - a;
      break;
    }
    case kHinge: {
      const double s = 2.0 * a - 1.0, t = 1.0 - s * u;
      L = t > 0.0 ? t : 0.0;
      g = t > 0.0 ? -s : 0.0;
      break;
    }
    case kLogistic: {
      // z = s u: log(1 + exp(-z)) = max(-z, 0) + log1p(exp(-|z|)), no overflow
      const double s = 2.0 * a - 1.0, z = s * u, e = exp(-fabs(z));
      L = (z < 0.0 ? -z : 0.0) + log1p(e);
      g = -s * (z < 0.0 ? 1.0 : e) / (1.0 + e);
      break;
    }
    case kPeriodic:
      L = 1.0 - cos(par * x);
      g = par * sin(par * x);
      break;
    default:
      L = g = __builtin_nan("");
  }
}

// the four waves' sums in wave order, by thread 0
__device__ __forceinline__ void block_objective(double lsum, double* sObj, int tid, double* out) {
  lsum = wave_sum(lsum);
  if ((tid & (kWave - 1)) == 0) sObj[tid / kWave] = lsum;
  __syncthreads();
  if (tid == 0) out[0] = ((sObj[0] + sObj[1]) + sObj[2]) + sObj[3];
}

// --------------------------------------------------------------------- gradX

// K4 = ceil(k / 4) steps of the first product; KT = ceil(k / 16) row tiles of gradX.
template <int K4>
__global__ __launch_bounds__(kThreads) void glrm_lossgrad_x_kernel(
    const float* __restrict__ A, const uint8_t* __restrict__ mask, const float* __restrict__ X,
    const float* __restrict__ Y, const int* __restrict__ codes, const double* __restrict__ pars, int64_t n, int p,
    int k, double* __restrict__ gradX, double* __restrict__ obj_part) {
  constexpr int KT = (K4 + 3) / 4;
  __shared__ double sY[2][kPC * kLdF];           // [data column][a]
  __shared__ float sA[2][kPC * kLdA], sM[2][kPC * kLdA];
  __shared__ double sPar[2][kPC];
  __shared__ int sCode[2][kPC];
  __shared__ double sObj[kThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * kXR;

  // X of the wave's 16 rows as the right operand of the first product: x[kk] = X[4 kk + lk][row]
  const int64_t row = i0 + 16 * wave + lr;
  double x[K4];
#pragma unroll
  for (int kk = 0; kk < K4; ++kk) {
    const int a = 4 * kk + lk;
    x[kk] = (a < k && row < n) ? (double)X[(int64_t)a * n + row] : 0.0;
  }

  const int sc = tid % kXR, sr = tid / kXR;      // stage of A: row, first data column
  const int ya = tid / kPC, yj = tid % kPC;      // stage of Y: factor, data column
  const bool iv = i0 + sc < n;
  float gm[4], ga[4];
  double gy[2], gp = 0.0;
  int gc = 0;
  auto load = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + sr + 4 * q;
      const int64_t idx = (int64_t)j * n + i0 + sc;
      const bool m = iv && j < p && mask[idx] != 0;
      gm[q] = m ? 1.0f : 0.0f;
      ga[q] = m ? A[idx] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int a = ya + 16 * q, j = j0 + yj;
      gy[q] = (a < k && j < p) ? (double)Y[(int64_t)a * p + j] : 0.0;
    }
    if (tid < kPC) {
      const bool ok = j0 + tid < p;
      gc = ok ? codes[j0 + tid] : 0;
      gp = ok ? pars[j0 + tid] : 0.0;
    }
  };
  auto store = [&](int b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sM[b][(sr + 4 * q) * kLdA + sc] = gm[q];
      sA[b][(sr + 4 * q) * kLdA + sc] = ga[q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) sY[b][yj * kLdF + ya + 16 * q] = gy[q];
    if (tid < kPC) {
      sCode[b][tid] = gc;
      sPar[b][tid] = gp;
    }
  };

  d4 acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = d4{0, 0, 0, 0};
  double lsum = 0.0;
  load(0);
  store(0);
  __syncthreads();
  int b = 0;
  for (int j0 = 0; j0 < p; j0 += kPC) {
    const bool more = j0 + kPC < p;
    if (more) load(j0 + kPC);
    const double* const y = sY[b];
    // U[j][i] = sum_a Y[a][j] X[a][i]: register v holds U[4 v + lk][lr]
    d4 u = d4{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < K4; ++kk)
      u = __builtin_amdgcn_mfma_f64_16x16x4f64(y[lr * kLdF + 4 * kk + lk], x[kk], u, 0, 0, 0);
    d4 g;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int jj = 4 * v + lk;
      const bool m = sM[b][jj * kLdA + 16 * wave + lr] != 0.0f;
      double L, d;
      loss_eval(sCode[b][jj], sPar[b][jj], u[v], (double)sA[b][jj * kLdA + 16 * wave + lr], L, d);
      g[v] = m ? d : 0.0;
      lsum += m ? L : 0.0;
    }
    // gradX[a][i] += sum_j Y[a][j] G[j][i]: g[v] is the right operand of step v
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[(4 * v + lk) * kLdF + 16 * t + lr], g[v], acc[t], 0, 0, 0);
    if (more) store(b ^ 1);
    __syncthreads();
    b ^= 1;
  }
  // register v of tile t holds gradX[16 t + 4 v + lk][row]: lanes along i
  if (row < n) {
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int a = 16 * t + 4 * v + lk;
        if (a < k) gradX[(int64_t)a * n + row] = acc[t][v];
      }
  }
  block_objective(lsum, sObj, tid, obj_part + blockIdx.x);
}

// --------------------------------------------------------------------- gradY

// Wave w takes the stage's row tile w % 2 and, of that tile's four K steps of the
// second product, steps 2 (w / 2) and 2 (w / 2) + 1: the first product is formed
// twice, the derivatives (the expensive part) once.
template <int K4>
__global__ __launch_bounds__(kThreads) void glrm_lossgrad_y_kernel(
    const float* __restrict__ A, const uint8_t* __restrict__ mask, const float* __restrict__ X,
    const float* __restrict__ Y, const int* __restrict__ codes, const double* __restrict__ pars, int64_t n, int p,
    int k, int64_t slab_rows, double* __restrict__ part, double* __restrict__ obj_part) {
  constexpr int KT = (K4 + 3) / 4;
  __shared__ double sX[2][kNC * kLdF];           // [row][a]; the epilogue's [wave][a][16] after the walk
  __shared__ float sA[2][kPC * kLdN], sM[2][kPC * kLdN];
  __shared__ double sObj[kThreads / kWave];
  static_assert(2 * kNC * kLdF >= 4 * kMaxK * 16, "epilogue stage");
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lr = lane & 15, lk = lane >> 4;
  const int it = wave & 1, half = wave >> 1;
  const int j0 = blockIdx.x * kPC;
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;

  // Y of the 16 data columns as the right operand of the first product, and the lane's column
  const int jl = j0 + lr;
  double y[K4];
#pragma unroll
  for (int kk = 0; kk < K4; ++kk) {
    const int a = 4 * kk + lk;
    y[kk] = (a < k && jl < p) ? (double)Y[(int64_t)a * p + jl] : 0.0;
  }
  const int code = jl < p ? codes[jl] : 0;
  const double par = jl < p ? pars[jl] : 0.0;

  const int sn = tid % kNC, sj = tid / kNC;      // stage: row, first data column / factor
  float gm[2], ga[2];
  double gx[4];
  auto load = [&](int64_t t0) {
    const int64_t row = t0 + sn;
    const bool rv = row < r1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = j0 + sj + 8 * q;
      const int64_t idx = (int64_t)j * n + row;
      const bool m = rv && j < p && mask[idx] != 0;
      gm[q] = m ? 1.0f : 0.0f;
      ga[q] = m ? A[idx] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = sj + 8 * q;
      gx[q] = (rv && a < k) ? (double)X[(int64_t)a * n + row] : 0.0;
    }
  };
  auto store = [&](int b) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      sM[b][(sj + 8 * q) * kLdN + sn] = gm[q];
      sA[b][(sj + 8 * q) * kLdN + sn] = ga[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) sX[b][sn * kLdF + sj + 8 * q] = gx[q];
  };

  d4 acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = d4{0, 0, 0, 0};
  double lsum = 0.0;
  load(r0);
  store(0);
  __syncthreads();
  int b = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += kNC) {
    const bool more = t0 + kNC < r1;
    if (more) load(t0 + kNC);
    const double* const x = sX[b];
    // U^T[i][j] = sum_a X[a][i] Y[a][j]: register v holds U^T[16 it + 4 v + lk][lr]
    d4 u = d4{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < K4; ++kk)
      u = __builtin_amdgcn_mfma_f64_16x16x4f64(x[(16 * it + lr) * kLdF + 4 * kk + lk], y[kk], u, 0, 0, 0);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ii = 16 * it + 4 * (2 * half + h) + lk;
      const bool m = sM[b][lr * kLdN + ii] != 0.0f;
      double L, d;
      loss_eval(code, par, half ? u[2 + h] : u[h], (double)sA[b][lr * kLdN + ii], L, d);
      const double g = m ? d : 0.0;
      lsum += m ? L : 0.0;
      // gradY[a][j] += sum_i X[a][i] G^T[i][j], this step's rows i = 16 it + 4 (2 half + h) + 0..3
#pragma unroll
      for (int t = 0; t < KT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ii * kLdF + 16 * t + lr], g, acc[t], 0, 0, 0);
    }
    if (more) store(b ^ 1);
    __syncthreads();
    b ^= 1;
  }
  // the four waves' tiles through LDS, added in wave order; register v of tile t is (16 t + 4 v + lk, lr)
  double* const sOut = &sX[0][0];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) sOut[(wave * kMaxK + 16 * t + 4 * v + lk) * 16 + lr] = acc[t][v];
  __syncthreads();
  double* const out = part + (int64_t)blockIdx.y * p * k;
  for (int e = tid; e < kPC * k; e += kThreads) {
    const int j = e / k, a = e % k;
    if (j0 + j < p)
      out[(int64_t)(j0 + j) * k + a] = ((sOut[a * 16 + j] + sOut[(kMaxK + a) * 16 + j]) +
                                        sOut[(2 * kMaxK + a) * 16 + j]) + sOut[(3 * kMaxK + a) * 16 + j];
  }
  block_objective(lsum, sObj, tid, obj_part + (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// ---------------------------------------------------------------------- fold

// Blocks 0 .. gridDim.x - 2: one thread per gradY[a][j], the slabs in order (none for the X
// kernel, whose gradient is final).  The last block: the objective partials, each thread its
// stride in index order, then the lanes by a butterfly and the waves in order.
__global__ __launch_bounds__(kThreads) void glrm_lossgrad_fold_kernel(const double* __restrict__ part, int slabs,
                                                                     int p, int k, double* __restrict__ gradY,
                                                                     const double* __restrict__ obj_part,
                                                                     int64_t nobj, double* __restrict__ obj) {
  __shared__ double sObj[kThreads / kWave];
  if (blockIdx.x == gridDim.x - 1) {
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < nobj; e += kThreads) s += obj_part[e];
    block_objective(s, sObj, threadIdx.x, obj);
    return;
  }
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x, len = (int64_t)p * k;
  if (e >= len) return;
  const int64_t a = e / p, j = e % p;
  double s = 0.0;
  for (int q = 0; q < slabs; ++q) s += part[q * len + j * k + a];
  gradY[e] = s;
}

#define H2OMX_K4_DISPATCH(KERNEL, ...)                    \
  switch ((k + 3) / 4) {                                  \
    case 1: KERNEL<1> __VA_ARGS__; break;                 \
    case 2: KERNEL<2> __VA_ARGS__; break;                 \
    case 3: KERNEL<3> __VA_ARGS__; break;                 \
    case 4: KERNEL<4> __VA_ARGS__; break;                 \
    case 5: KERNEL<5> __VA_ARGS__; break;                 \
    case 6: KERNEL<6> __VA_ARGS__; break;                 \
    case 7: KERNEL<7> __VA_ARGS__; break;                 \
    default: KERNEL<8> __VA_ARGS__; break;                \
  }

}  // namespace

// gradX [k][n] fp64, gradX[a][i] = sum_j Y[a][j] m_ji L_j'(u_ji, a_ji), and obj[0] = sum m L, for
// A [p][n] (fp32, feature-major), mask [p][n] (bytes, 0 = missing), X [k][n] and Y [k][p] (fp32),
// codes [p] (int32, the Loss enum) and pars [p] (double), 1 <= k <= 32.
// Work: obj_part [ceil(n / 64)] doubles.
H2OMX_API int h2omx_glrm_loss_grad_x(const float* A, const uint8_t* mask, const float* X, const float* Y,
                                     const int* codes, const double* pars, int64_t n, int p, int k, double* gradX,
                                     double* obj_part, double* obj, hipStream_t stream) {
  if (n < 1 || p < 1 || k < 1 || k > kMaxK || (n + kXR - 1) / kXR > 0x7fffffff) return kBadArg;
  const int64_t blocks = (n + kXR - 1) / kXR;
  H2OMX_K4_DISPATCH(glrm_lossgrad_x_kernel, <<<(unsigned)blocks, kThreads, 0, stream>>>(A, mask, X, Y, codes, pars, n,
                                                                                        p, k, gradX, obj_part));
  glrm_lossgrad_fold_kernel<<<1, kThreads, 0, stream>>>(nullptr, 0, p, k, nullptr, obj_part, blocks, obj);
  return launch_status();
}

// gradY [k][p] fp64, gradY[a][j] = sum_i X[a][i] m_ji L_j'(u_ji, a_ji), and obj[0] = sum m L.
// Work: part [slabs][p][k] and obj_part [slabs][ceil(p / 16)] doubles, slabs = ceil(n / slab_rows).
H2OMX_API int h2omx_glrm_loss_grad_y(const float* A, const uint8_t* mask, const float* X, const float* Y,
                                     const int* codes, const double* pars, int64_t n, int p, int k,
                                     int64_t slab_rows, double* part, double* obj_part, double* gradY, double* obj,
                                     hipStream_t stream) {
  if (n < 1 || p < 1 || k < 1 || k > kMaxK || slab_rows < 1) return kBadArg;
  const int64_t slabs = (n + slab_rows - 1) / slab_rows;
  if (slabs > 65535) return kBadArg;
  const dim3 grid((p + kPC - 1) / kPC, (unsigned)slabs);
  H2OMX_K4_DISPATCH(glrm_lossgrad_y_kernel, <<<grid, kThreads, 0, stream>>>(A, mask, X, Y, codes, pars, n, p, k,
                                                                            slab_rows, part, obj_part));
  const int64_t len = (int64_t)p * k;
  glrm_lossgrad_fold_kernel<<<(unsigned)((len + kThreads - 1) / kThreads) + 1, kThreads, 0, stream>>>(
      part, (int)slabs, p, k, gradY, obj_part, slabs * grid.x, obj);
  return launch_status();
}
