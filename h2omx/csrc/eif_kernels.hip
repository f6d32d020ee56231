// Extended Isolation Forest scoring on gfx950: every row walks every tree of the
// forest and only the hyperplane products on its own path are ever formed.
//
//   eif_walk_sparse_kernel<XLDS>  lane per row, packed non-zeros of the normals
//   eif_walk_dense_kernel<U>      unit of U lanes per row, dense normals
//   eif_fold_kernel               slab partials added in slab order, / T, fp32
//
// Arithmetic, both walks: x and the normal's entries are fp32 widened to fp64, so
// every product is exact and only the additions round; the branch is
// proj > (double) offs.  A NaN of the scored matrix becomes its column's training
// mean as it is loaded.  A leaf's value hval = depth + c(size) is an fp32 table
// entry (0, or a multiple of 2^-23 in [1, 64)), an inner node carries -1; a row's
// values are added over the trees in fp64, which is exact in any order for
// T <= 2^20, so the result depends neither on the slab split nor on the call.
// Nothing here uses a floating-point atomic or waits for another workgroup.
//
// Forest.  Heap-indexed trees of cap = 2^(limit + 1) - 1 nodes, children of node v
// at 2 v + 1 and 2 v + 2.  meta [T][cap] = {offs, hval}.  A walk takes at most
// limit steps, after which it stands on a node of index < cap; the host has
// checked that every node a walk can reach after limit steps is a leaf.
//
// Sparse.  ent [T][cap][K] = {dim, val}, dims ascending, K the largest number of
// non-zeros of any node; padded entries carry val = 0 and the node's first dim.  A
// workgroup of four waves owns 256 rows and one slab of trees.  With p <= 64
// (XLDS) its block of the feature-major matrix Xraw [p][n] is staged once as
// [p][256] fp32 in LDS by coalesced row reads; lane l only ever reads column l, so
// it stays on its bank.  Otherwise x comes from Xraw[dim][row] in global memory.
// All lanes are in the same tree at the same time: the top levels are wave-uniform
// reads, deeper levels gathers of 8 to 8 + 8 K bytes per lane.  A wave leaves a
// tree when all its lanes stand on leaves (wave vote, no barrier).
//
// Dense.  A row has a unit of U adjacent lanes, U the power of two covering p, at
// most 64; lane c keeps x[c], x[c + U], ... of its row in registers (at most four,
// p <= 256).  A workgroup owns 64 rows: they are staged once as [p][64] in LDS by
// coalesced reads (column r of feature f at r ^ (f & 63), so a unit's reads across
// features hit distinct banks), then walked 256 / U rows at a time, each pass over
// the whole slab.  Per step a unit reads its node's row of normals [T][cap][p],
// one contiguous segment, multiplies and folds by an xor butterfly in fp64: every
// lane of the unit holds the same sum and takes the same branch.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSparseRows = 256;     // rows of a sparse workgroup
constexpr int kDenseRows = 64;       // rows of a dense workgroup
constexpr int kXldsMaxP = 64;        // sparse: widest matrix staged in LDS (64 KB)
constexpr int kDenseMaxP = 256;      // dense: four values per lane at U = 64
constexpr int kDenseVals = 4;
constexpr int kMaxLimit = 24;

struct Ent {
  uint32_t dim;
  float val;
};

__device__ __forceinline__ float impute(float v, const float* __restrict__ means, int f) {
  return v != v ? means[f] : v;
}

// one row's result: the slab's partial, or with one slab the mean length itself
__device__ __forceinline__ void store_row(double acc, int64_t row, int64_t n, int T, double* __restrict__ part,
                                          float* __restrict__ out) {
  if (part != nullptr)
    part[(int64_t)blockIdx.y * n + row] = acc;
  else
    out[row] = (float)(acc / (double)T);
}

template <bool XLDS>
__global__ __launch_bounds__(kThreads) void eif_walk_sparse_kernel(
    const float* __restrict__ Xraw, const float* __restrict__ means, const float2* __restrict__ meta,
    const Ent* __restrict__ ent, int64_t n, int p, int T, int cap, int K, int limit, int slab_trees,
    double* __restrict__ part, float* __restrict__ out) {
  extern __shared__ float sx[];   // XLDS: [p][256]
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * kSparseRows + tid;
  const bool live = row < n;
  if (XLDS) {
    for (int f = 0; f < p; ++f) sx[f * kSparseRows + tid] = live ? impute(Xraw[(int64_t)f * n + row], means, f) : 0.0f;
    __syncthreads();
  }
  const int t0 = blockIdx.y * slab_trees;
  const int t1 = min(T, t0 + slab_trees);
  double acc = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int64_t base = (int64_t)t * cap;
    uint32_t node = 0;
    float hv;
    for (int step = 0;; ++step) {
      const float2 m = meta[base + node];
      hv = m.y;
      const bool inner = live && hv < 0.0f && step < limit;
      if (!__any(inner)) break;
      if (inner) {
        const Ent* __restrict__ e = ent + (base + node) * K;
        double proj = 0.0;
        for (int k = 0; k < K; ++k) {
          const Ent q = e[k];
          const float x = XLDS ? sx[q.dim * kSparseRows + tid] : impute(Xraw[(int64_t)q.dim * n + row], means, (int)q.dim);
          proj += (double)x * (double)q.val;
        }
        node = 2 * node + 1 + (proj > (double)m.x ? 1u : 0u);
      }
    }
    acc += (double)fmaxf(hv, 0.0f);
  }
  if (live) store_row(acc, row, n, T, part, out);
}

template <int U>
__global__ __launch_bounds__(kThreads) void eif_walk_dense_kernel(
    const float* __restrict__ Xraw, const float* __restrict__ means, const float2* __restrict__ meta,
    const float* __restrict__ normals, int64_t n, int p, int T, int cap, int limit, int slab_trees,
    double* __restrict__ part, float* __restrict__ out) {
  extern __shared__ float sx[];   // [p][64], column r of feature f at r ^ (f & 63)
  constexpr int kUnits = kThreads / U;                                  // units of the workgroup
  constexpr int kPassRows = kUnits < kDenseRows ? kUnits : kDenseRows;  // rows of a pass
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kDenseRows;
  for (int i = tid; i < p * kDenseRows; i += kThreads) {
    const int f = i / kDenseRows, r = i % kDenseRows;
    const int64_t row = row0 + r;
    sx[f * kDenseRows + (r ^ (f & 63))] = row < n ? impute(Xraw[(int64_t)f * n + row], means, f) : 0.0f;
  }
  __syncthreads();
  const int unit = tid / U, c = tid % U;
  const int t0 = blockIdx.y * slab_trees;
  const int t1 = min(T, t0 + slab_trees);
  for (int r = unit; r < kDenseRows; r += kPassRows) {   // U < 4: the waves of the units past row 64 idle
    const int64_t row = row0 + r;
    const bool live = row < n;
    float x[kDenseVals];
#pragma unroll
    for (int j = 0; j < kDenseVals; ++j) {
      const int f = c + j * U;
      x[j] = f < p ? sx[f * kDenseRows + (r ^ (f & 63))] : 0.0f;
    }
    double acc = 0.0;
    for (int t = t0; t < t1; ++t) {
      const int64_t base = (int64_t)t * cap;
      uint32_t node = 0;
      float hv;
      for (int step = 0;; ++step) {
        const float2 m = meta[base + node];
        hv = m.y;
        const bool inner = live && hv < 0.0f && step < limit;   // the same in every lane of a unit
        if (!__any(inner)) break;
        const float* __restrict__ nr = normals + (base + node) * p;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kDenseVals; ++j) {
          const int f = c + j * U;
          if (inner && f < p) s += (double)x[j] * (double)nr[f];
        }
#pragma unroll
        for (int off = U / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        if (inner) node = 2 * node + 1 + (s > (double)m.x ? 1u : 0u);
      }
      acc += (double)fmaxf(hv, 0.0f);
    }
    if (live && c == 0) store_row(acc, row, n, T, part, out);
  }
}

__global__ __launch_bounds__(kThreads) void eif_fold_kernel(const double* __restrict__ part, int slabs, int64_t n, int T,
                                                            float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double t = 0.0;
  for (int q = 0; q < slabs; ++q) t += part[(int64_t)q * n + i];
  out[i] = (float)(t / (double)T);
}

template <int U>
void launch_dense(dim3 grid, hipStream_t stream, const float* Xraw, const float* means, const float2* meta,
                  const float* normals, int64_t n, int p, int T, int cap, int limit, int slab_trees, double* part,
                  float* out) {
  eif_walk_dense_kernel<U><<<grid, kThreads, (size_t)p * kDenseRows * sizeof(float), stream>>>(
      Xraw, means, meta, normals, n, p, T, cap, limit, slab_trees, part, out);
}

}  // namespace

// out [n] fp32 = mean over the T trees of the path value of every column of Xraw [p][n] (feature-major, NaN ->
// means [p]).  meta [T][cap] {offs, hval}; dense == 0: ent [T][cap][K] {dim, val}; dense != 0: normals [T][cap][p],
// p <= 256.  cap = 2^(limit + 1) - 1, limit <= 24, T <= 2^20.
// Work: part [slabs][n] doubles with slabs = ceil(T / slab_trees), unused (may be null) with one slab.
H2OMX_API int h2omx_eif_mean_length(const float* Xraw, const float* means, const void* meta, const void* ent,
                                    const float* normals, int64_t n, int p, int T, int cap, int K, int limit,
                                    int slab_trees, int dense, double* part, float* out, hipStream_t stream) {
  if (n < 1 || p < 1 || T < 1 || T > (1 << 20) || limit < 0 || limit > kMaxLimit || cap != (2 << limit) - 1 ||
      slab_trees < 1)
    return kBadArg;
  if (dense ? (normals == nullptr || p > kDenseMaxP) : (ent == nullptr || K < 1)) return kBadArg;
  const int slabs = (T + slab_trees - 1) / slab_trees;
  const int64_t blocks = (n + (dense ? kDenseRows : kSparseRows) - 1) / (dense ? kDenseRows : kSparseRows);
  if (slabs > 65535 || blocks > INT32_MAX || (slabs > 1 && part == nullptr)) return kBadArg;
  double* dst = slabs > 1 ? part : nullptr;
  const dim3 grid((unsigned)blocks, (unsigned)slabs);
  const float2* mt = (const float2*)meta;
  if (!dense) {
    if (p <= kXldsMaxP)
      eif_walk_sparse_kernel<true><<<grid, kThreads, (size_t)p * kSparseRows * sizeof(float), stream>>>(
          Xraw, means, mt, (const Ent*)ent, n, p, T, cap, K, limit, slab_trees, dst, out);
    else
      eif_walk_sparse_kernel<false><<<grid, kThreads, 0, stream>>>(Xraw, means, mt, (const Ent*)ent, n, p, T, cap, K,
                                                                    limit, slab_trees, dst, out);
  } else {
#define EIF_DENSE(U_) launch_dense<U_>(grid, stream, Xraw, means, mt, normals, n, p, T, cap, limit, slab_trees, dst, out)
    if (p <= 1) EIF_DENSE(1);
    else if (p <= 2) EIF_DENSE(2);
    else if (p <= 4) EIF_DENSE(4);
    else if (p <= 8) EIF_DENSE(8);
    else if (p <= 16) EIF_DENSE(16);
    else if (p <= 32) EIF_DENSE(32);
    else EIF_DENSE(64);
#undef EIF_DENSE
  }
  if (slabs > 1)
    eif_fold_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(part, slabs, n, T, out);
  return launch_status();
}
