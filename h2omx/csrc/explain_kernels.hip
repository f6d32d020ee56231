// Model explanation kernels: path-dependent TreeSHAP contributions for tree
// ensembles (H2O predict_contributions for GBM / DRF / XGBoost).
//
// The host flattens every root-to-leaf path of the ensemble into a leaf
// record {first element, unique features m, leaf value} and m path elements
// {feature | na_ok << 30 | categorical << 29, zero fraction z, lo, hi}: a row
// "follows" the path on feature f (one fraction o = 1) when lo < x <= hi (NA:
// na_ok; categorical: level x in the path's level set sets[lo]), and z is
// the product of the cover ratios of the path's edges on f.  For the path
// polynomial P(t) = prod_j (z_j + o_j t) the Shapley contribution of
// element i is
//     phi_i += v (o_i - z_i) sum_k w(m, k) [t^k] P(t) / (z_i + o_i t),
// w(m, k) = k! (m - 1 - k)! / m!   (Lundberg et al. 2020, path form used by
// GPUTreeShap).  One thread per row walks the same leaf list, so leaf and
// element loads are wave-uniform (scalar / broadcast) and the per-feature
// accumulators are written coalesced: in LDS ([F][256] per workgroup) when
// they fit, else straight to the feature-major output.
//
// Precision.  Followed elements (o_i = 1) are taken out of P by synthetic
// division from the top coefficient, which carries the rounding error of the
// middle coefficients, eps C(m, m/2) when the z_j are near 1, down to the
// constant term.  In fp32 that stays below 1e-5 per unit leaf value up to
// m = 16 and reaches 1e-1 at m = 32 (measured against tests/shapref.py), so
// the MAXM = 32 instantiation keeps P and the division in fp64 (2^-53 C(32, 16)
// = 7e-8); the two narrower ones are fp32 throughout.
#include <type_traits>

#include "common.h"

namespace {

template <int MAXM, bool LDS>
__global__ __launch_bounds__(256) void tree_shap_kernel(const float* __restrict__ X, int64_t ld, int64_t n, int F,
                                                        const int4* __restrict__ leaves, int nleaves,
                                                        const float4* __restrict__ elems,
                                                        const float* __restrict__ wtab, float* __restrict__ out,
                                                        const uint32_t* __restrict__ sets) {
  // fp32 for MAXM <= 16; the 32-wide instantiation carries P and the division in fp64
  // (see the header).  z and o are kept as the float32 they were read as, which is exact.
  using T = typename std::conditional<(MAXM > 16), double, float>::type;
  extern __shared__ float acc[];
  __shared__ float w_s[(MAXM + 1) * (MAXM + 1)];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  const bool live = r < n;
  const int64_t rr = live ? r : 0;
  for (int j = tid; j < (MAXM + 1) * (MAXM + 1); j += 256) w_s[j] = wtab[j];
  if (LDS)
    for (int j = tid; j < F * 256; j += 256) acc[j] = 0.0f;
  __syncthreads();
  for (int L = 0; L < nleaves; ++L) {
    const int4 hd = leaves[L];
    const int m = hd.y;
    const float v = __int_as_float(hd.z);
    float z[MAXM], o[MAXM];
    int fe[MAXM];
    T P[MAXM + 1];
    P[0] = 1.0f;
#pragma unroll
    for (int k = 1; k <= MAXM; ++k) P[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXM; ++j) {
      z[j] = 1.0f; o[j] = 1.0f; fe[j] = 0;
      if (j < m) {
        const float4 e = elems[hd.x + j];
        const int fi = __float_as_int(e.x);
        const int f = fi & 0x1FFFFFFF;
        const float x = X[(int64_t)f * ld + rr];
        float oj;
        if (x != x) {
          oj = (float)((fi >> 30) & 1);
        } else if ((fi >> 29) & 1) {
          // categorical feature: the path's allowed level set (unseen levels: NA direction)
          const int b = (int)x;
          const uint32_t* st = sets + 8 * (int64_t)e.z;
          oj = (b < 0 || b > 255) ? (float)((fi >> 30) & 1) : (float)((st[b >> 5] >> (b & 31)) & 1u);
        } else {
          oj = (x > e.z && x <= e.w) ? 1.0f : 0.0f;
        }
        const T zj = e.y, ojt = oj;
        z[j] = e.y; o[j] = oj; fe[j] = f;
#pragma unroll
        for (int k = MAXM; k >= 1; --k)
          if (k <= j + 1) P[k] = zj * P[k] + ojt * P[k - 1];
        P[0] *= zj;
      }
    }
    const float* wm = w_s + m * (MAXM + 1);
#pragma unroll
    for (int i = 0; i < MAXM; ++i) {
      if (i < m) {
        const T zi = z[i], oi = o[i];
        T s = 0.0f;
        if (oi != 0.0f) {
          // P / (z_i + t) by synthetic division from the top coefficient
          T carry = 0.0f;
#pragma unroll
          for (int k = MAXM; k >= 1; --k) {
            if (k <= m) {
              const T q = P[k] - zi * carry;
              s += q * wm[k - 1];
              carry = q;
            }
          }
        } else if (zi > 0.0f) {
          const T inv = 1.0f / zi;
#pragma unroll
          for (int k = 0; k < MAXM; ++k)
            if (k < m) s += P[k] * inv * wm[k];
        }
        const float phi = (float)(v * (oi - zi) * s);
        if (LDS) acc[fe[i] * 256 + tid] += phi;
        else if (live) out[(int64_t)fe[i] * n + r] += phi;
      }
    }
  }
  if (LDS) {
    __syncthreads();
    if (live)
      for (int f = 0; f < F; ++f) out[(int64_t)f * n + r] = acc[f * 256 + tid];
  }
}

}  // namespace

H2OMX_API int h2omx_tree_shap(const float* X, int64_t ld, int64_t n, int F, const void* leaves, int nleaves,
                              const void* elems, const float* wtab, int maxm, float* out, const uint32_t* sets,
                              hipStream_t stream) {
  if (n <= 0) return kOk;
  if (F <= 0 || maxm < 1 || maxm > 32) return kBadArg;
  const int grid = (int)((n + 255) / 256);
  const bool lds = (size_t)F * 256 * sizeof(float) <= 64 * 1024;
  const size_t shm = lds ? (size_t)F * 256 * sizeof(float) : 0;
  const int4* lv = reinterpret_cast<const int4*>(leaves);
  const float4* el = reinterpret_cast<const float4*>(elems);
#define LAUNCH_SHAP(M)                                                                                           \
  do {                                                                                                          \
    if (lds)                                                                                                    \
      hipLaunchKernelGGL((tree_shap_kernel<M, true>), dim3(grid), dim3(256), shm, stream, X, ld, n, F, lv,      \
                         nleaves, el, wtab, out, sets);                                                         \
    else                                                                                                        \
      hipLaunchKernelGGL((tree_shap_kernel<M, false>), dim3(grid), dim3(256), 0, stream, X, ld, n, F, lv,       \
                         nleaves, el, wtab, out, sets);                                                         \
  } while (0)
  if (maxm <= 8) LAUNCH_SHAP(8);
  else if (maxm <= 16) LAUNCH_SHAP(16);
  else LAUNCH_SHAP(32);
#undef LAUNCH_SHAP
  return launch_status();
}

// ---------------------------------------------------------------------------
// Interventional (baseline) SHAP against a background set
// ---------------------------------------------------------------------------
// For a scored row x and a background row b the game value of a coalition T is
// the margin of the hybrid row (features in T from x, the rest from b).  Per
// flattened leaf with m unique-feature elements this is closed form: with
// ox_j / ob_j = "x / b satisfies element j" (the follow rule above), the leaf
// is dead when some element has neither; otherwise S = {ox && !ob}, a = |S|,
// B = {!ox && ob}, c = |B| and
//     phi_j += v (a-1)! c! / (a+c)!   for j in S,
//     phi_j -= v a! (c-1)! / (a+c)!   for j in B.
// Both weights come from one table T[a][c] = (a-1)! c! / (a+c)! (row 0 is
// zero): wS = T[a][c], wB = T[c][a].
//
// shap_bg_mask_kernel packs ob for every (leaf, background row) into a
// leaf-major word table [L][nb].  tree_shap_bg_kernel keeps one thread per
// scored row: per leaf it packs ox once, then walks a chunk of background rows
// whose ob words are wave-uniform scalar loads.  blockIdx.y is the background
// chunk; each chunk owns a slab out[chunk][F][n] (no float atomics), and
// shap_slab_mean_kernel adds the slabs in index order.
namespace {

constexpr int kBgW = 33;  // weight table is [33][33]: a, c <= 32

__device__ __forceinline__ uint32_t elem_follows(float x, const float4 e, const uint32_t* __restrict__ sets) {
  const int fi = __float_as_int(e.x);
  if (x != x) return (uint32_t)((fi >> 30) & 1);
  if ((fi >> 29) & 1) {
    // categorical feature: the path's allowed level set (unseen levels: NA direction)
    const int b = (int)x;
    const uint32_t* st = sets + 8 * (int64_t)e.z;
    return (b < 0 || b > 255) ? (uint32_t)((fi >> 30) & 1) : ((st[b >> 5] >> (b & 31)) & 1u);
  }
  return (x > e.z && x <= e.w) ? 1u : 0u;
}

// bit j of w spread over the word (0 or ~0).  Kept opaque: written as shifts the
// compiler turns the mask-and-or below back into and / compare / select chains.
__device__ __forceinline__ uint32_t bit_mask(uint32_t w, int j) {
  uint32_t r;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(r) : "v"(w), "i"(j));
  return r;
}

__global__ __launch_bounds__(256) void shap_bg_mask_kernel(const float* __restrict__ B, int64_t ldb, int nb,
                                                           const int4* __restrict__ leaves, int nleaves,
                                                           const float4* __restrict__ elems,
                                                           const uint32_t* __restrict__ sets,
                                                           uint32_t* __restrict__ bmask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nleaves * nb) return;
  const int L = (int)(i / nb);
  const int b = (int)(i - (int64_t)L * nb);
  const int4 hd = leaves[L];
  const int m = hd.y < 32 ? hd.y : 32;
  uint32_t mk = 0;
  for (int j = 0; j < m; ++j) {
    const float4 e = elems[hd.x + j];
    const int f = __float_as_int(e.x) & 0x1FFFFFFF;
    mk |= elem_follows(B[(int64_t)f * ldb + b], e, sets) << j;
  }
  bmask[i] = mk;
}

template <int MAXM, bool LDS>
__global__ __launch_bounds__(256) void tree_shap_bg_kernel(const float* __restrict__ X, int64_t ld, int64_t n, int F,
                                                           const int4* __restrict__ leaves, int nleaves,
                                                           const float4* __restrict__ elems,
                                                           const float* __restrict__ wtab,
                                                           const uint32_t* __restrict__ sets,
                                                           const uint32_t* __restrict__ bmask, int nb, int chunk,
                                                           float* __restrict__ slabs) {
  extern __shared__ float acc[];
  __shared__ float w_s[kBgW * kBgW];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  const bool live = r < n;
  const int64_t rr = live ? r : 0;
  const int b0 = (int)blockIdx.y * chunk;
  const int b1 = b0 + chunk < nb ? b0 + chunk : nb;
  float* __restrict__ out = slabs + (int64_t)blockIdx.y * F * n;
  for (int j = tid; j < kBgW * kBgW; j += 256) w_s[j] = wtab[j];
  if (LDS)
    for (int j = tid; j < F * 256; j += 256) acc[j] = 0.0f;
  __syncthreads();
  for (int L = 0; L < nleaves; ++L) {
    const int4 hd = leaves[L];
    const int m = hd.y;
    if (m == 0) continue;
    const float v = __int_as_float(hd.z);
    int fe[MAXM];
    float s[MAXM];
    uint32_t ox = 0;
#pragma unroll
    for (int j = 0; j < MAXM; ++j) {
      fe[j] = 0; s[j] = 0.0f;
      if (j < m) {
        const float4 e = elems[hd.x + j];
        const int f = __float_as_int(e.x) & 0x1FFFFFFF;
        ox |= elem_follows(X[(int64_t)f * ld + rr], e, sets) << j;
        fe[j] = f;
      }
    }
    const uint32_t mm = m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);
    // leaf L's background words: L, b and nb are uniform, so these are scalar loads
    const uint32_t* __restrict__ bm = bmask + (int64_t)L * nb;
    for (int b = b0; b < b1; ++b) {
      const uint32_t ob = bm[b];
      const uint32_t S = ox & ~ob, Bs = ob & ~ox;
      const bool dead = (~(ox | ob) & mm) != 0u;
      const int a = __popc(S), c = __popc(Bs);
      const uint32_t ws = __float_as_uint(w_s[dead ? 0 : a * kBgW + c]);
      const uint32_t nwb = __float_as_uint(w_s[dead ? 0 : c * kBgW + a]) ^ 0x80000000u;
#pragma unroll
      for (int g = 0; g < MAXM; g += 4) {
        if (g < m) {
#pragma unroll
          for (int j = g; j < g + 4; ++j) {
            // S and Bs are disjoint: bit j sign-extended selects +wS, -wB or 0 without a branch
            s[j] += __uint_as_float((bit_mask(S, j) & ws) | (bit_mask(Bs, j) & nwb));
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MAXM; ++j) {
      if (j < m) {
        const float phi = v * s[j];
        if (LDS) acc[fe[j] * 256 + tid] += phi;
        else if (live) out[(int64_t)fe[j] * n + r] += phi;
      }
    }
  }
  if (LDS) {
    __syncthreads();
    if (live)
      for (int f = 0; f < F; ++f) out[(int64_t)f * n + r] = acc[f * 256 + tid];
  }
}

__global__ __launch_bounds__(256) void shap_slab_mean_kernel(const float* __restrict__ slabs, int nslabs, int64_t len,
                                                             float div, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  float s = 0.0f;
  for (int c = 0; c < nslabs; ++c) s += slabs[(int64_t)c * len + i];
  out[i] = s / div;
}

}  // namespace

// Contributions of n scored rows against nb background rows.  bmask is
// [nleaves][nb] scratch, slabs is [ceil(nb / chunk)][F][n] and must be zeroed
// by the caller; chunk = 1 leaves phi(x, b) of pair (r, b) at slabs[b][f][r].
// With out != null the slabs are added in index order and divided by nb into
// out [F][n] (the averaged form).
H2OMX_API int h2omx_tree_shap_background(const float* X, int64_t ld, int64_t n, int F, const float* B, int64_t ldb,
                                         int nb, const void* leaves, int nleaves, const void* elems,
                                         const float* wtab, int maxm, const uint32_t* sets, uint32_t* bmask,
                                         int chunk, float* slabs, float* out, hipStream_t stream) {
  if (n <= 0) return kOk;
  if (F <= 0 || maxm < 1 || maxm > 32 || nb <= 0 || chunk <= 0 || nleaves < 0) return kBadArg;
  const int64_t gx = (n + 255) / 256;
  const int nchunks = (nb + chunk - 1) / chunk;
  const int64_t cells = (int64_t)nleaves * nb;
  if (gx > 0x7FFFFFFF || nchunks > 65535 || (cells + 255) / 256 > 0x7FFFFFFF) return kBadArg;
  const int4* lv = reinterpret_cast<const int4*>(leaves);
  const float4* el = reinterpret_cast<const float4*>(elems);
  if (cells > 0)
    hipLaunchKernelGGL(shap_bg_mask_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, B, ldb, nb,
                       lv, nleaves, el, sets, bmask);
  const bool lds = (size_t)F * 256 * sizeof(float) <= 64 * 1024;
  const size_t shm = lds ? (size_t)F * 256 * sizeof(float) : 0;
  const dim3 grid((unsigned)gx, (unsigned)nchunks);
#define LAUNCH_SHAP_BG(M)                                                                                        \
  do {                                                                                                          \
    if (lds)                                                                                                    \
      hipLaunchKernelGGL((tree_shap_bg_kernel<M, true>), grid, dim3(256), shm, stream, X, ld, n, F, lv,         \
                         nleaves, el, wtab, sets, bmask, nb, chunk, slabs);                                     \
    else                                                                                                        \
      hipLaunchKernelGGL((tree_shap_bg_kernel<M, false>), grid, dim3(256), 0, stream, X, ld, n, F, lv,          \
                         nleaves, el, wtab, sets, bmask, nb, chunk, slabs);                                     \
  } while (0)
  if (maxm <= 8) LAUNCH_SHAP_BG(8);
  else if (maxm <= 16) LAUNCH_SHAP_BG(16);
  else LAUNCH_SHAP_BG(32);
#undef LAUNCH_SHAP_BG
  if (out != nullptr) {
    const int64_t len = (int64_t)F * n;
    if ((len + 255) / 256 > 0x7FFFFFFF) return kBadArg;
    hipLaunchKernelGGL(shap_slab_mean_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, stream, slabs,
                       nchunks, len, (float)nb, out);
  }
  return launch_status();
}

// ---------------------------------------------------------------------------
// Friedman-Popescu H statistic: partial dependence of every variable subset
// ---------------------------------------------------------------------------
// The partial dependence of the model on a variable set S by the weighted tree
// traversal is a sum over the flattened leaves:
//     PD_S(x) = sum_l v_l prod_{e in l, feat(e) in S} [x follows e] prod_{e in l, feat(e) not in S} z_e.
// For k variables the host keeps the leaves whose path touches one of them and
// gives each a record: hdr [2k + 2] = {lo_0, hi_0, ..., lo_{k-1}, hi_{k-1},
// na_ok mask, untouched mask} and w [2^k] doubles, w[S] = v prod_{e not in S}
// z_e for the subset with bit mask S (w[0] pads; 0 where S holds no touched
// variable: that term is the same for every row and stays on the host).  One
// thread per row builds the k-bit follow mask of its row per leaf and adds
// w[S] for every S the mask covers, in fp64 registers: H is a difference of
// partial dependences that cancels to zero for variables that do not interact.
// The leaf record is wave-uniform (scalar loads).  blockIdx.y is a chunk of
// leaves; each chunk owns a slab Fd[chunk][2^k - 1][n] (no fp64 atomics), and
// h_slab_sum_kernel adds the slabs in index order.
namespace {

constexpr int kHMaxK = 6;
constexpr int kHGroup = 16;

struct HVars {
  int f[kHMaxK];
};

template <int K>
__global__ __launch_bounds__(256) void friedman_h_pd_kernel(const float* __restrict__ X, int64_t ld, int64_t n,
                                                            HVars vars, const float* __restrict__ hdr,
                                                            const double* __restrict__ w, int nleaves, int chunk,
                                                            double* __restrict__ Fd) {
  constexpr int NS = (1 << K) - 1, HW = 2 * K + 2;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < n;
  const int64_t rr = live ? r : 0;
  float x[K];
  uint32_t isna = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    x[j] = X[(int64_t)vars.f[j] * ld + rr];
    isna |= (x[j] != x[j] ? 1u : 0u) << j;
  }
  const int l0 = (int)blockIdx.y * chunk;
  const int l1 = l0 + chunk < nleaves ? l0 + chunk : nleaves;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (int L = l0; L < l1; ++L) {
    // L is uniform: the record arrives as scalar loads.  Every load is unconditional (a load under
    // the row's condition would become a branch around a scalar load and its wait).
    const float* __restrict__ h = hdr + (int64_t)L * HW;
    const double* __restrict__ wl = w + ((int64_t)L << K);
    float hv[HW];
#pragma unroll
    for (int j = 0; j < HW; ++j) hv[j] = h[j];
    uint32_t in = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) in |= ((uint32_t)(x[j] > hv[2 * j]) & (uint32_t)(x[j] <= hv[2 * j + 1])) << j;
    // a NaN compares false above and follows the path's NA direction
    const uint32_t mk = in | (isna & __float_as_uint(hv[2 * K])) | __float_as_uint(hv[2 * K + 1]);
    // weights in groups of 16 doubles (32 SGPRs); w[0] is padding.  The fence keeps the scheduler
    // from hoisting every group's loads to the top of the body, which runs out of SGPRs at K >= 5.
#pragma unroll
    for (int g = 0; g <= NS; g += kHGroup) {
      double wv[kHGroup];
#pragma unroll
      for (int i = 0; i < kHGroup; ++i) wv[i] = (g + i <= NS) ? wl[g + i] : 0.0;
#pragma unroll
      for (int i = 0; i < kHGroup; ++i) {
        const int S = g + i;
        // acc += w * (1.0 or 0.0): one select on the multiplier's high word, the weight stays scalar
        if (S >= 1 && S <= NS)
          acc[S - 1] = fma(wv[i], __hiloint2double(((mk & S) == S) ? 0x3FF00000 : 0, 0), acc[S - 1]);
      }
      if (NS >= kHGroup) __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (live) {
    double* __restrict__ out = Fd + (int64_t)blockIdx.y * NS * n + r;
#pragma unroll
    for (int s = 0; s < NS; ++s) out[(int64_t)s * n] = acc[s];
  }
}

__global__ __launch_bounds__(256) void h_slab_sum_kernel(const double* __restrict__ slabs, int nslabs, int64_t len,
                                                         double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  double s = 0.0;
  for (int c = 0; c < nslabs; ++c) s += slabs[(int64_t)c * len + i];
  out[i] = s;
}

}  // namespace

// Partial dependence of n rows on every non-empty subset of k variables (2 <= k
// <= 6, feature rows v0 .. v5 of X, the first k used).  hdr is [nleaves][2k + 2],
// w is [nleaves][2^k]; leaves are cut into chunks of `chunk`.  One chunk
// writes out [2^k - 1][n] directly; more write slabs [nchunks][2^k - 1][n], which
// are then added in index order into out.
H2OMX_API int h2omx_friedman_h_pd(const float* X, int64_t ld, int64_t n, int F, int k, int v0, int v1, int v2, int v3,
                                  int v4, int v5, const float* hdr, const double* w, int nleaves, int chunk,
                                  double* slabs, double* out, hipStream_t stream) {
  if (n <= 0 || nleaves <= 0) return kOk;
  if (k < 2 || k > kHMaxK || chunk <= 0 || ld < n) return kBadArg;
  const HVars vars = {{v0, v1, v2, v3, v4, v5}};
  for (int j = 0; j < k; ++j)
    if (vars.f[j] < 0 || vars.f[j] >= F) return kBadArg;
  const int64_t gx = (n + 255) / 256;
  const int nchunks = (nleaves + chunk - 1) / chunk;
  const int64_t len = (((int64_t)1 << k) - 1) * n;
  if (gx > 0x7FFFFFFF || nchunks > 65535 || (len + 255) / 256 > 0x7FFFFFFF) return kBadArg;
  double* Fd = nchunks == 1 ? out : slabs;
  const dim3 grid((unsigned)gx, (unsigned)nchunks);
#define LAUNCH_H(KK)                                                                                             \
  case KK:                                                                                                      \
    hipLaunchKernelGGL((friedman_h_pd_kernel<KK>), grid, dim3(256), 0, stream, X, ld, n, vars, hdr, w, nleaves, \
                       chunk, Fd);                                                                              \
    break
  switch (k) {
    LAUNCH_H(2);
    LAUNCH_H(3);
    LAUNCH_H(4);
    LAUNCH_H(5);
    LAUNCH_H(6);
  }
#undef LAUNCH_H
  if (nchunks > 1)
    hipLaunchKernelGGL(h_slab_sum_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, stream, slabs, nchunks,
                       len, out);
  return launch_status();
}

// ---------------------------------------------------------------------------
// Partial dependence: every grid cell of a swept feature in one ensemble walk
// ---------------------------------------------------------------------------
// out[y][c][cls][r] is the raw margin of row r with feature fs set to grid[c]
// (and, for ff >= 0, feature ff set to fixed[y]): what predict_raw_kernel
// (tree_kernels.hip) gives on the matrix with those rows overwritten, with the
// same fp32 additions in the same tree order, so the two are bit-identical.
// The caller initialises out as raw_margin does (init_f or zero).
//
// A row that reaches a leaf without meeting a split on fs reaches it for every
// cell, and a numeric split on fs cuts the ascending grid in two runs.  One
// thread per row walks each tree once per run: from the root for the first cell
// c0 of the run, lowering `next` (the first cell after c0 that would leave the
// path) at every split on fs where c0 goes left, to the upper bound of thr in
// the grid; cells that go right stay right for the rest of the grid.  The upper
// bound depends on the node and the grid alone, so the host gives it per node
// (ub, aligned with nodes).  The leaf value goes to cells [c0, next).  Cells
// [gn, G) hold NaN and are runs of their own, as is a cell at a categorical
// group split on fs; a walk that meets no split on fs ends the tree for every
// cell that is left, NaN cells included.  No stack, no scratch.
//
// The cell accumulators live in LDS as [cell][thread] (a lane keeps its bank),
// at most 64 cells (64 KiB) per window of sorted cells; a window starts its
// walk at its first cell and clips runs at its end.  blockIdx.z = window * K +
// class, blockIdx.y = y.
namespace {

constexpr int kPdWindow = 64;

struct PdNode {  // TreeNode of tree_kernels.hip (32 B)
  int feat, bin, left, na_left;
  float thr, value, gain, weight;
};

template <bool COUNT>
__global__ __launch_bounds__(256) void pd_sweep_kernel(const float* __restrict__ X, int64_t ld, int64_t n,
                                                       const PdNode* __restrict__ nodes,
                                                       const int* __restrict__ roots, int ntrees, int K,
                                                       const uint32_t* __restrict__ catbits, int fs,
                                                       const float* __restrict__ grid, const int* __restrict__ ub,
                                                       int G, int gn, int ff, const float* __restrict__ fixed,
                                                       float* __restrict__ out,
                                                       unsigned long long* __restrict__ walks) {
  extern __shared__ float acc[];  // [W][256]
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  if (r >= n) return;
  const int cls = (int)blockIdx.z % K;
  const int w0 = ((int)blockIdx.z / K) * kPdWindow;
  const int w1 = w0 + kPdWindow < G ? w0 + kPdWindow : G;
  const int W = w1 - w0;
  // cells [w0, wn) of the window are ascending numbers, [wn, w1) are NaN
  const int wn = gn < w0 ? w0 : (gn < w1 ? gn : w1);
  const float fy = ff >= 0 ? fixed[blockIdx.y] : 0.0f;
  float* __restrict__ o = out + (((int64_t)blockIdx.y * G + w0) * K + cls) * n + r;
  for (int c = 0; c < W; ++c) acc[c * 256 + tid] = o[(int64_t)c * K * n];
  unsigned cnt = 0;
  for (int t = cls; t < ntrees; t += K) {
    const int root = roots[t];
    const PdNode* __restrict__ tr = nodes + root;
    int c0 = w0;
    while (c0 < w1) {
      const float gv = grid[c0];
      int next = c0 < wn ? wn : c0 + 1;
      bool met = false;  // a split on fs on this walk's path
      int id = 0;
      for (int guard = 0; guard < 64; ++guard) {
        const PdNode nd = tr[id];
        if (nd.feat < 0) break;
        const bool swept = nd.feat == fs;
        met |= swept;
        const float v = swept ? gv : (nd.feat == ff ? fy : X[(int64_t)nd.feat * ld + r]);
        bool left;
        if (v != v) {
          left = (nd.na_left & 1) != 0;
        } else if (nd.na_left & 2) {
          const int b = (int)v;
          const uint32_t* __restrict__ bits = catbits + 8 * ((int64_t)root + id);
          left = (b < 0 || b > 255) ? (nd.na_left & 1) != 0 : ((bits[b >> 5] >> (b & 31)) & 1u) != 0;
          if (swept) next = c0 + 1;
        } else {
          left = v <= nd.thr;
          if (swept && left) {
            // grid[c0] <= thr, so the bound lies past c0; clamped all the same, a run never ends before c0 + 1
            int u = ub[root + id];
            u = u > c0 ? u : c0 + 1;
            next = u < next ? u : next;
          }
        }
        id = left ? nd.left : nd.left + 1;
      }
      const float val = tr[id].value;
      if (!met) next = w1;  // the path never asked for the swept value: every cell left ends here
      for (int c = c0; c < next; ++c) acc[(c - w0) * 256 + tid] += val;
      c0 = next;
      if (COUNT) ++cnt;
    }
  }
  for (int c = 0; c < W; ++c) o[(int64_t)c * K * n] = acc[c * 256 + tid];
  if (COUNT) atomicAdd(walks, (unsigned long long)cnt);
}

}  // namespace

// Margins of n rows for G cells of feature fs: grid [G] holds gn ascending
// numbers, then G - gn NaNs; ub [total nodes] is, for a node that splits on fs,
// the number of the gn cells that are <= its thr.  ff >= 0 pins feature ff to
// fixed[y] for each of the ny slices of out [ny][G][K][n] (ff < 0: ny = 1, fixed
// unused).  nodes, roots and catbits are those of h2omx_predict_raw.  walks
// (optional) receives the number of root-to-leaf walks made; it selects a
// separate instantiation, the kernel without it carries no counter.
H2OMX_API int h2omx_pd_sweep(const float* X, int64_t ld, int64_t n, int F, const void* nodes, const int* roots,
                             int ntrees, int K, const uint32_t* catbits, int fs, const float* grid, const int* ub,
                             int G, int gn, int ff, const float* fixed, int ny, float* out,
                             unsigned long long* walks, hipStream_t stream) {
  if (n <= 0 || G <= 0) return kOk;
  if (K < 1 || ntrees < 0 || fs < 0 || fs >= F || ff >= F || ff == fs || gn < 0 || gn > G || ny < 1 || ld < n)
    return kBadArg;
  if (ff >= 0 ? fixed == nullptr : ny != 1) return kBadArg;
  const int64_t gx = (n + 255) / 256;
  const int64_t gz = (int64_t)((G + kPdWindow - 1) / kPdWindow) * K;
  if (gx > 0x7FFFFFFF || ny > 65535 || gz > 65535) return kBadArg;
  const size_t shm = (size_t)(G < kPdWindow ? G : kPdWindow) * 256 * sizeof(float);
  const dim3 blocks((unsigned)gx, (unsigned)ny, (unsigned)gz);
  const PdNode* nd = reinterpret_cast<const PdNode*>(nodes);
  if (walks != nullptr)
    hipLaunchKernelGGL((pd_sweep_kernel<true>), blocks, dim3(256), shm, stream, X, ld, n, nd, roots, ntrees, K,
                       catbits, fs, grid, ub, G, gn, ff, fixed, out, walks);
  else
    hipLaunchKernelGGL((pd_sweep_kernel<false>), blocks, dim3(256), shm, stream, X, ld, n, nd, roots, ntrees, K,
                       catbits, fs, grid, ub, G, gn, ff, fixed, out, walks);
  return launch_status();
}

// ---------------------------------------------------------------------------
// Ranked contributions: the top / bottom features of every row (reason codes)
// ---------------------------------------------------------------------------
// phi [F][ld] holds a row's contributions down a column.  With key[f] = phi[f]
// (|phi[f]| for ABS) two total orders are defined, both breaking ties towards
// the lower feature index (-0.0 == +0.0 is a tie):
//     descending D: f before g iff key[f] > key[g] or (key[f] == key[g] and f < g),
//     ascending  A: f before g iff key[f] < key[g] or (key[f] == key[g] and f < g).
// The position of f in an order is the number of features before it, so one
// thread per row ranks by counting, with no sort:
//     rankD[f] = #{g < f : key[g] >= key[f]} + #{g > f : key[g] > key[f]},
//     rankA[f] = #{g < f : key[g] <= key[f]} + #{g > f : key[g] < key[f]}.
// Both ranks are bijections onto 0 .. F-1, so slot s of idx_out / val_out
// [kt + kb][n] (kt top slots, then kb bottom slots) is written exactly once:
// (f, phi[f]) goes to slot rankD[f] when rankD[f] < kt and to slot kt + rankA[f]
// when rankA[f] < kb.  Nothing depends on an order of execution and no float is
// computed, so results are bit-identical between calls.  Keys are finite (sums
// of leaf values); a NaN key compares false both ways and its slot is undefined.
//
// kRankC candidates are held in registers per sweep over the keys, so a key is
// read F / kRankC times.  The sweep has three parts, each with compile-time
// comparisons: features before the candidates (>=, <=), the candidates against
// each other (unrolled: the relation of two of them is their register index),
// and features after them (>, <).  For F <= 64 the keys are staged in LDS as
// [f][256] (a lane keeps its bank, every thread reads only its own column, so no
// barrier); above that they are re-read from the planes, which a workgroup keeps
// in cache (256 x F floats).
namespace {

constexpr int kRankC = 4;
constexpr int kRankLdsF = 64;  // F * 1 KiB of keys per workgroup within the file's 64 KiB budget

template <bool LDS, bool ABS>
__global__ __launch_bounds__(256) void contrib_rank_kernel(const float* __restrict__ phi, int64_t ld, int64_t n,
                                                           int F, int kt, int kb, int* __restrict__ idx_out,
                                                           float* __restrict__ val_out) {
  extern __shared__ float keys[];  // [F][256] when LDS
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  if (r >= n) return;
  const float* __restrict__ col = phi + r;
  auto plane = [&](int g) -> float {
    const float x = col[(int64_t)g * ld];
    return ABS ? fabsf(x) : x;
  };
  auto key = [&](int g) -> float { return LDS ? keys[g * 256 + tid] : plane(g); };
  if (LDS)
    for (int g = 0; g < F; ++g) keys[g * 256 + tid] = plane(g);
  for (int f0 = 0; f0 < F; f0 += kRankC) {
    float kf[kRankC];
    int rd[kRankC], ra[kRankC];
#pragma unroll
    for (int c = 0; c < kRankC; ++c) {
      // candidates past F repeat the last feature; they are counted and never written
      kf[c] = key(f0 + c < F ? f0 + c : F - 1);
      rd[c] = 0;
      ra[c] = 0;
    }
#pragma unroll 4
    for (int g = 0; g < f0; ++g) {
      const float kg = key(g);
#pragma unroll
      for (int c = 0; c < kRankC; ++c) {
        rd[c] += kg >= kf[c] ? 1 : 0;
        ra[c] += kg <= kf[c] ? 1 : 0;
      }
    }
#pragma unroll
    for (int j = 0; j < kRankC; ++j) {
      if (f0 + j < F) {
#pragma unroll
        for (int c = 0; c < kRankC; ++c) {
          if (j < c) {
            rd[c] += kf[j] >= kf[c] ? 1 : 0;
            ra[c] += kf[j] <= kf[c] ? 1 : 0;
          } else if (j > c) {
            rd[c] += kf[j] > kf[c] ? 1 : 0;
            ra[c] += kf[j] < kf[c] ? 1 : 0;
          }
        }
      }
    }
#pragma unroll 4
    for (int g = f0 + kRankC; g < F; ++g) {
      const float kg = key(g);
#pragma unroll
      for (int c = 0; c < kRankC; ++c) {
        rd[c] += kg > kf[c] ? 1 : 0;
        ra[c] += kg < kf[c] ? 1 : 0;
      }
    }
#pragma unroll
    for (int c = 0; c < kRankC; ++c) {
      const int f = f0 + c;
      if (f < F) {
        // the reported value keeps its sign (and the sign of a zero)
        const float v = ABS ? col[(int64_t)f * ld] : kf[c];
        if (rd[c] < kt) {
          idx_out[(int64_t)rd[c] * n + r] = f;
          val_out[(int64_t)rd[c] * n + r] = v;
        }
        if (ra[c] < kb) {
          idx_out[(int64_t)(kt + ra[c]) * n + r] = f;
          val_out[(int64_t)(kt + ra[c]) * n + r] = v;
        }
      }
    }
  }
}

}  // namespace

// The kt first features of every row in descending and the kb first in
// ascending order of the key (phi, or |phi| with compare_abs), ties to the
// lower feature index: phi is [F][ld] with ld >= n, idx_out (feature indices)
// and val_out (the signed phi) are [kt + kb][n], top slots first.
H2OMX_API int h2omx_contrib_rank(const float* phi, int64_t ld, int64_t n, int F, int kt, int kb, int compare_abs,
                                 int* idx_out, float* val_out, hipStream_t stream) {
  if (n <= 0) return kOk;
  if (F <= 0 || kt < 0 || kb < 0 || kt > F || kb > F || kt + kb == 0 || ld < n) return kBadArg;
  const int64_t gx = (n + 255) / 256;
  if (gx > 0x7FFFFFFF) return kBadArg;
  const bool lds = F <= kRankLdsF;
  const size_t shm = lds ? (size_t)F * 256 * sizeof(float) : 0;
#define LAUNCH_RANK(L, A)                                                                                        \
  hipLaunchKernelGGL((contrib_rank_kernel<L, A>), dim3((unsigned)gx), dim3(256), shm, stream, phi, ld, n, F, kt, \
                     kb, idx_out, val_out)
  if (lds) {
    if (compare_abs) LAUNCH_RANK(true, true);
    else LAUNCH_RANK(true, false);
  } else {
    if (compare_abs) LAUNCH_RANK(false, true);
    else LAUNCH_RANK(false, false);
  }
#undef LAUNCH_RANK
  return launch_status();
}

// ---------------------------------------------------------------------------
// DeepSHAP (DeepLIFT rescale rule) for the Deep Learning MLP
// ---------------------------------------------------------------------------
// A pair (scored row x, background row b) back-propagates multipliers through
// the net: with the hidden pre-activations a = zx[h], b = zb[h] of a layer and
// the multipliers G of its outputs, U = G * r(a, b) and the layer below gets
// G' = U W (the project's GEMM).  r is the secant slope (f(a) - f(b)) / (a - b)
// of the activation f, written so that nothing cancels (d = a - b):
//   Rectifier     1 if a, b > 0;  0 if a, b <= 0;  a / (a - b) if a > 0 >= b;
//                 b / (b - a) if b > 0 >= a (a tie lands in the first two).
//   Tanh          s(d) (1 - tanh a tanh b), s(d) = tanh(d) / d, s(0) = 1
//                 (tanh a - tanh b = tanh(a - b) (1 - tanh a tanh b)); at a tie
//                 this is the derivative 1 - tanh^2 a.
//   ExpRectifier  (ELU, alpha = 1)  1 if a, b > 0;
//                 e^max(a,b) (-expm1(-|d|)) / |d| if a, b <= 0, e^a at d = 0:
//                 the same number as e^min(a,b) expm1(|d|) / |d| with every
//                 factor in [0, 1], so a wide gap cannot give 0 * inf;
//                 (a - expm1(b)) / (a - b) if a > 0 >= b (both terms of the
//                 numerator are >= 0), mirrored for b > 0 >= a.
// Every branch is a quotient of same-signed finite terms or a product of
// bounded ones: no epsilon, and finite inputs give a finite r in [0, 1].
//
// deepshap_rescale_kernel is a pure stream over the [pairs][h] planes (pair =
// i * nb + j, x-major).  Lanes run along the unit axis, so a wave moves 256
// contiguous bytes of a row of G, U, Zx and Zb per instruction.  A workgroup
// (4 waves) owns 64 units of one scored row: every lane keeps its zx (and what
// depends on zx alone) in registers while wave w walks the background rows
// w, w + 4 gridDim.z, ... of the workgroup's share; Zb [nb][h] is re-read by
// every scored row and stays in L2.  For the top hidden layer G is the vector
// g_L [h] (VEC), held in a register as well, never a [pairs][h] plane.  U may
// be G: an element is read and written by the same lane.
namespace {

constexpr int kDsWaves = 4;  // waves (background rows in flight) per workgroup

template <int ACT>
struct DsRow;  // what depends on the scored row's pre-activation alone

template <>
struct DsRow<1> {
  float a;
  __device__ explicit DsRow(float a_) : a(a_) {}
  __device__ float r(float b) const {
    const bool pa = a > 0.0f, pb = b > 0.0f;
    if (pa == pb) return pa ? 1.0f : 0.0f;
    return pa ? a / (a - b) : b / (b - a);
  }
};

template <>
struct DsRow<2> {
  float a, ta;
  __device__ explicit DsRow(float a_) : a(a_), ta(tanhf(a_)) {}
  __device__ float r(float b) const {
    const float d = a - b;
    const float s = d == 0.0f ? 1.0f : tanhf(d) / d;
    return s * (1.0f - ta * tanhf(b));
  }
};

template <>
struct DsRow<4> {
  float a, ea, ema;  // e^a and expm1(a), used where a <= 0
  __device__ explicit DsRow(float a_) : a(a_), ea(expf(fminf(a_, 0.0f))), ema(expm1f(fminf(a_, 0.0f))) {}
  __device__ float r(float b) const {
    const bool pa = a > 0.0f, pb = b > 0.0f;
    if (pa && pb) return 1.0f;
    if (pa) return (a - expm1f(b)) / (a - b);
    if (pb) return (b - ema) / (b - a);
    const float ad = fabsf(a - b);
    const float top = a >= b ? ea : expf(b);
    return ad == 0.0f ? ea : top * (-expm1f(-ad)) / ad;
  }
};

template <int ACT, bool VEC>
__global__ __launch_bounds__(kDsWaves * kWave) void deepshap_rescale_kernel(const float* G,
                                                                           const float* __restrict__ Zx,
                                                                           const float* __restrict__ Zb, float* U,
                                                                           int nb, int h) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int c = blockIdx.y * kWave + lane;
  if (c >= h) return;
  const int64_t i = blockIdx.x;
  const DsRow<ACT> row(Zx[i * h + c]);
  const float gv = VEC ? G[c] : 0.0f;
  const int step = kDsWaves * (int)gridDim.z;
  const int64_t base = i * nb;
  int j = (int)blockIdx.z * kDsWaves + wave;
  // two background rows per trip: their loads are independent
  for (; j + step < nb; j += 2 * step) {
    const int64_t o0 = (base + j) * h + c, o1 = (base + j + step) * h + c;
    const float b0 = Zb[(int64_t)j * h + c], b1 = Zb[(int64_t)(j + step) * h + c];
    const float g0 = VEC ? gv : G[o0], g1 = VEC ? gv : G[o1];
    U[o0] = g0 * row.r(b0);
    U[o1] = g1 * row.r(b1);
  }
  if (j < nb) {
    const int64_t o0 = (base + j) * h + c;
    U[o0] = (VEC ? gv : G[o0]) * row.r(Zb[(int64_t)j * h + c]);
  }
}

// deepshap_fold_kernel: G0 [rows * nb][p] holds a pair's multipliers of the p
// design columns.  Design column f contributes scale G0[pair][f] (xs[i][f] -
// bs[j][f]); predictor c owns the columns col_start[c] .. col_start[c + 1] - 1,
// added in that order.  MEAN = false writes the pair's value to out[c][pair],
// MEAN = true the mean over the background to out[c][i]: one thread adds the
// pairs j = 0 .. nb - 1 of its (i, c) in index order and divides once, so the
// result does not depend on a schedule and is bit-identical between calls (no
// atomics).  Threads take (row, c) with c fastest, so a wave reads whole rows
// of G0; the tile is turned in LDS ([c][row], padded) and written with lanes
// along the row axis of the feature-major output.
constexpr int kFoldC = 64;  // predictors per LDS tile
// output rows per workgroup: pairs, or (MEAN) scored rows, few of them because each is a walk over nb pairs
constexpr int kFoldPairs = 64, kFoldMeanRows = 8;

template <bool MEAN>
__global__ __launch_bounds__(256) void deepshap_fold_kernel(const float* __restrict__ G0, const float* __restrict__ xs,
                                                            const float* __restrict__ bs,
                                                            const int* __restrict__ col_start, float scale,
                                                            int64_t rows, int nb, int p, int C, int64_t ldo,
                                                            float* __restrict__ out) {
  constexpr int TR = MEAN ? kFoldMeanRows : kFoldPairs;
  __shared__ float tile[kFoldC * (TR + 1)];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * TR;
  const int nr = (int)(rows - r0 < TR ? rows - r0 : TR);
  for (int c0 = 0; c0 < C; c0 += kFoldC) {
    const int cc = C - c0 < kFoldC ? C - c0 : kFoldC;
    for (int t = tid; t < nr * cc; t += 256) {
      const int rl = t / cc, cl = t - rl * cc;
      const int f0 = col_start[c0 + cl], f1 = col_start[c0 + cl + 1];
      const int64_t r = r0 + rl;
      float v;
      if (MEAN) {
        const float* __restrict__ x = xs + r * p;
        float acc = 0.0f;
#pragma unroll 4
        for (int j = 0; j < nb; ++j) {
          const float* __restrict__ g = G0 + (r * nb + j) * p;
          const float* __restrict__ b = bs + (int64_t)j * p;
          float s = 0.0f;
          for (int f = f0; f < f1; ++f) s += scale * g[f] * (x[f] - b[f]);
          acc += s;
        }
        v = acc / (float)nb;
      } else {
        const int64_t i = r / nb;
        const float* __restrict__ x = xs + i * p;
        const float* __restrict__ b = bs + (r - i * nb) * p;
        const float* __restrict__ g = G0 + r * p;
        v = 0.0f;
        for (int f = f0; f < f1; ++f) v += scale * g[f] * (x[f] - b[f]);
      }
      tile[cl * (TR + 1) + rl] = v;
    }
    __syncthreads();
    for (int t = tid; t < cc * TR; t += 256) {
      const int cl = t / TR, rl = t - cl * TR;
      if (rl < nr) out[(int64_t)(c0 + cl) * ldo + r0 + rl] = tile[cl * (TR + 1) + rl];
    }
    __syncthreads();
  }
}

}  // namespace

// U[(i nb + j)][c] = G[..] r(Zx[i][c], Zb[j][c]) over ni scored rows, nb
// background rows and h units; act = 1 Rectifier, 2 Tanh, 4 ExpRectifier.
// g_is_vector: G is the [h] vector every pair shares (top hidden layer), else
// the [ni nb][h] plane, which U may alias.
H2OMX_API int h2omx_deepshap_rescale(const float* G, int g_is_vector, const float* Zx, const float* Zb, float* U,
                                     int64_t ni, int nb, int h, int act, hipStream_t stream) {
  if (ni <= 0 || nb <= 0 || h <= 0 || (act != 1 && act != 2 && act != 4)) return kBadArg;
  const int64_t gy = (h + kWave - 1) / kWave;
  if (ni > 0x7FFFFFFF || gy > 65535) return kBadArg;
  // enough workgroups for a small block of scored rows, at most one wave per background row
  int64_t gz = 2048 / (ni * gy);
  const int64_t zmax = (nb + kDsWaves - 1) / kDsWaves;
  gz = gz < 1 ? 1 : (gz > zmax ? zmax : gz);
  if (gz > 65535) gz = 65535;
  const dim3 grid((unsigned)ni, (unsigned)gy, (unsigned)gz), blk(kDsWaves * kWave);
#define LAUNCH_DS(A)                                                                                             \
  if (g_is_vector)                                                                                               \
    hipLaunchKernelGGL((deepshap_rescale_kernel<A, true>), grid, blk, 0, stream, G, Zx, Zb, U, nb, h);           \
  else                                                                                                           \
    hipLaunchKernelGGL((deepshap_rescale_kernel<A, false>), grid, blk, 0, stream, G, Zx, Zb, U, nb, h)
  if (act == 1) { LAUNCH_DS(1); }
  else if (act == 2) { LAUNCH_DS(2); }
  else { LAUNCH_DS(4); }
#undef LAUNCH_DS
  return launch_status();
}

// G0 [ni nb][p], xs [ni][p], bs [nb][p], col_start [C + 1] (ascending, 0 .. p).
// mean = 0: out[c][ldo] gets the ni nb pairs (x-major) from column 0 on;
// mean = 1: it gets the ni background means.  The caller offsets ``out`` to
// the block's first row; ldo is the row length of the whole result.
H2OMX_API int h2omx_deepshap_fold(const float* G0, const float* xs, const float* bs, const int* col_start, float scale,
                                  int64_t ni, int nb, int p, int C, int mean, int64_t ldo, float* out,
                                  hipStream_t stream) {
  if (ni <= 0 || nb <= 0 || p <= 0 || C <= 0) return kBadArg;
  const int64_t rows = mean ? ni : ni * nb;
  if (ldo < rows) return kBadArg;
  const int tr = mean ? kFoldMeanRows : kFoldPairs;
  const int64_t gx = (rows + tr - 1) / tr;
  if (gx > 0x7FFFFFFF) return kBadArg;
  if (mean)
    hipLaunchKernelGGL((deepshap_fold_kernel<true>), dim3((unsigned)gx), dim3(256), 0, stream, G0, xs, bs, col_start,
                       scale, rows, nb, p, C, ldo, out);
  else
    hipLaunchKernelGGL((deepshap_fold_kernel<false>), dim3((unsigned)gx), dim3(256), 0, stream, G0, xs, bs, col_start,
                       scale, rows, nb, p, C, ldo, out);
  return launch_status();
}
