// Tree introspection on gfx950: every row walks every tree of a packed ensemble
// once and leaves what the three public tree outputs need.
//
//   walk_kernel<kLeaf, XLDS>    ids [T][n] int32 (tree-local node index), reached [T][cap] bytes
//   walk_kernel<kStaged, XLDS>  out [nt][K][n] fp32, the margin after every iteration
//   walk_kernel<kCounts, XLDS>  cnt [F][n] fp32, how often a row's paths test each feature
//   walk_fold_kernel            int32 count partials added in slab order, to fp32
//
// Walk rule (TreeWalker.go_left, pd_sweep_kernel): every decision is an exact fp32
// comparison.  NaN goes by flag bit 0; a node with flag bit 1 is a categorical
// group split and tests bit (int) v of its 8-word bitset, codes outside 0 .. 255
// go by flag bit 0; otherwise v <= thr goes left.  At most 64 steps per tree.
//
// Packed ensemble.  A node is 16 bytes {feat, thr, left << 2 | flags, value}, a leaf
// has feat < 0.  Tree t owns the slots roots[t] .. roots[t] + cap - 1; the host has
// checked that the children of every reachable inner node lie behind it and inside
// those slots, so a walk stays in bounds and ends.
//
// Work split.  A workgroup of four waves owns 256 rows, one lane per row, and a
// slab of trees (leaf ids, counts) or every tree of one class in order (staged
// margins, whose fp64 running sum lives in the lane).  All lanes are in the same
// tree at the same time: the top levels are wave-uniform reads, deeper levels
// gathers of 16 bytes per lane.  A wave leaves a tree when all its lanes stand on
// leaves (wave vote); the kernel has no barrier at all.
//
// LDS.  With F <= 32 the [F][256] block of the feature-major matrix is staged once
// by coalesced reads; lane l only ever reads column l, so it keeps its bank and
// needs no barrier.  The counts mode keeps int32 counters [F][256] the same way.
// Tree records are read from global memory.  A double-buffered LDS stage for trees
// of up to 1024 nodes was built and measured here and lost at every shape
// (docs/ROADMAP.md, Round 24), so it is not in the kernel.
//
// No floating-point atomics, no workgroup waits for another, no host
// synchronisation; results are bit-identical between calls.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 256;           // rows of a workgroup
constexpr int kXldsMaxF = 32;        // widest matrix (and counter block) staged in LDS
constexpr int kMaxSteps = 64;
constexpr int kLeaf = 0, kStaged = 1, kCounts = 2;

struct alignas(16) WNode {
  int feat;
  float thr;
  int lf;       // left << 2 | categorical << 1 | na_left
  float value;
};
static_assert(sizeof(WNode) == 16, "a node is one 16-byte load");

struct WalkArgs {
  const float* X;            // [F][ld]
  int64_t ld, n;
  int F;
  const WNode* nodes;
  const int* roots;          // [T]
  const uint32_t* catbits;   // [T][cap][8] or null
  int T, cap, K;
  int slab_trees;            // leaf, counts
  int average;               // staged
  const double* init_f;      // staged, [K]
  int* ids;                  // leaf
  uint8_t* reached;          // leaf, optional
  float* out;                // staged; counts with LDS counters and one slab
  int* part;                 // counts: [slabs][F][n]
};

template <int MODE, bool XLDS>
__global__ __launch_bounds__(kThreads) void walk_kernel(const WalkArgs a) {
  extern __shared__ float smem[];
  constexpr bool CLDS = MODE == kCounts && XLDS;
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * kRows + tid;
  const bool live = row < a.n;
  float* __restrict__ sx = smem;                                                      // XLDS: [F][256]
  int* __restrict__ sc = reinterpret_cast<int*>(smem) + (XLDS ? a.F * kRows : 0);     // CLDS: [F][256]
  if (XLDS)
    for (int f = 0; f < a.F; ++f) sx[f * kRows + tid] = live ? a.X[(int64_t)f * a.ld + row] : 0.0f;
  if (CLDS)
    for (int f = 0; f < a.F; ++f) sc[f * kRows + tid] = 0;

  // the trees of this workgroup: tb, tb + ts, ... (cnt of them)
  int tb, ts, cnt;
  if (MODE == kStaged) {
    tb = blockIdx.y;
    ts = a.K;
    cnt = a.T / a.K;
  } else {
    tb = blockIdx.y * a.slab_trees;
    ts = 1;
    cnt = min(a.T, tb + a.slab_trees) - tb;
  }
  double acc = 0.0;
  if (MODE == kStaged && !a.average) acc = a.init_f[blockIdx.y];
  int* __restrict__ gc = MODE == kCounts && !CLDS ? a.part + (int64_t)blockIdx.y * a.F * a.n + row : nullptr;

  for (int i = 0; i < cnt; ++i) {
    const int t = tb + i * ts;
    const int root = a.roots[t];
    const WNode* __restrict__ tr = a.nodes + root;
    int node = 0, step = 0;
    float val = 0.0f;
    for (; step < kMaxSteps; ++step) {
      const WNode nd = tr[node];
      val = nd.value;
      const bool inner = live && nd.feat >= 0;
      if (!__any(inner)) break;
      if (inner) {
        const float v = XLDS ? sx[nd.feat * kRows + tid] : a.X[(int64_t)nd.feat * a.ld + row];
        bool left;
        if (v != v) {
          left = (nd.lf & 1) != 0;
        } else if (nd.lf & 2) {
          const int b = (int)v;
          const uint32_t* __restrict__ bits = a.catbits + 8 * ((int64_t)root + node);
          left = (b < 0 || b > 255) ? (nd.lf & 1) != 0 : ((bits[b >> 5] >> (b & 31)) & 1u) != 0;
        } else {
          left = v <= nd.thr;
        }
        if (MODE == kCounts) {
          if (CLDS)
            sc[nd.feat * kRows + tid] += 1;
          else
            gc[(int64_t)nd.feat * a.n] += 1;
        }
        node = (nd.lf >> 2) + (left ? 0 : 1);
      }
    }
    if (MODE == kStaged && step == kMaxSteps) val = tr[node].value;   // the walk was cut on an inner node
    if (live) {
      if (MODE == kLeaf) {
        a.ids[(int64_t)t * a.n + row] = node;
        if (a.reached != nullptr) a.reached[(int64_t)t * a.cap + node] = 1;
      }
      if (MODE == kStaged) {
        acc += (double)val;
        a.out[(int64_t)t * a.n + row] = a.average ? (float)(acc / (double)(i + 1)) : (float)acc;
      }
    }
  }
  if (CLDS && live) {
    if (gridDim.y == 1)
      for (int f = 0; f < a.F; ++f) a.out[(int64_t)f * a.n + row] = (float)sc[f * kRows + tid];
    else
      for (int f = 0; f < a.F; ++f) a.part[((int64_t)blockIdx.y * a.F + f) * a.n + row] = sc[f * kRows + tid];
  }
}

__global__ __launch_bounds__(kThreads) void walk_fold_kernel(const int* __restrict__ part, int slabs, int64_t len,
                                                             float* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= len) return;
  int s = 0;
  for (int q = 0; q < slabs; ++q) s += part[(int64_t)q * len + i];
  cnt[i] = (float)s;
}

template <int MODE>
int launch(const WalkArgs& a, unsigned gy, hipStream_t stream) {
  const int64_t gx = (a.n + kRows - 1) / kRows;
  if (gx > INT32_MAX || gy < 1 || gy > 65535) return kBadArg;
  const dim3 grid((unsigned)gx, gy);
  if (a.F <= kXldsMaxF)
    walk_kernel<MODE, true><<<grid, kThreads, (size_t)a.F * kRows * 4 * (MODE == kCounts ? 2 : 1), stream>>>(a);
  else
    walk_kernel<MODE, false><<<grid, kThreads, 0, stream>>>(a);
  return launch_status();
}

WalkArgs common(const float* X, int64_t ld, int64_t n, int F, const void* nodes, const int* roots,
                const uint32_t* catbits, int T, int cap) {
  WalkArgs a{};
  a.X = X, a.ld = ld, a.n = n, a.F = F, a.nodes = (const WNode*)nodes, a.roots = roots, a.catbits = catbits;
  a.T = T, a.cap = cap, a.K = 1, a.slab_trees = T;
  return a;
}

bool bad_common(const WalkArgs& a) {
  return a.X == nullptr || a.nodes == nullptr || a.roots == nullptr || a.n < 1 || a.ld < a.n || a.F < 1 || a.T < 1 ||
         a.cap < 1;
}

}  // namespace

// The limits the launch code and the tests follow: widest matrix staged in LDS (also the widest counter block),
// rows of a workgroup.
H2OMX_API int h2omx_walk_limits(int* out) {
  out[0] = kXldsMaxF;
  out[1] = kRows;
  return kOk;
}

// ids [T][n] = the node every column of X [F][ld] (feature-major, n columns) ends on in every tree; reached
// [T][cap] (optional, zeroed by the caller) gets a 1 at every such node.  Slab s of slab_trees trees is one
// grid row.
H2OMX_API int h2omx_walk_leaf(const float* X, int64_t ld, int64_t n, int F, const void* nodes, const int* roots,
                              const uint32_t* catbits, int T, int cap, int slab_trees, int* ids, uint8_t* reached,
                              hipStream_t stream) {
  WalkArgs a = common(X, ld, n, F, nodes, roots, catbits, T, cap);
  if (bad_common(a) || slab_trees < 1 || ids == nullptr) return kBadArg;
  a.slab_trees = slab_trees < T ? slab_trees : T;
  a.ids = ids, a.reached = reached;
  return launch<kLeaf>(a, (unsigned)((T + a.slab_trees - 1) / a.slab_trees), stream);
}

// out [nt][K][n] fp32: the fp64 running sum over iterations of the leaf values of class k's trees (tree i K + k),
// from init_f [K] (average == 0) or from 0 and divided by the iteration count (average != 0), rounded to fp32.
H2OMX_API int h2omx_walk_staged(const float* X, int64_t ld, int64_t n, int F, const void* nodes, const int* roots,
                                const uint32_t* catbits, int nt, int K, int cap, const double* init_f, int average,
                                float* out, hipStream_t stream) {
  if (K < 1 || nt < 1 || nt > INT32_MAX / K) return kBadArg;
  WalkArgs a = common(X, ld, n, F, nodes, roots, catbits, nt * K, cap);
  if (bad_common(a) || out == nullptr || (!average && init_f == nullptr)) return kBadArg;
  a.K = K, a.average = average != 0, a.init_f = init_f, a.out = out;
  return launch<kStaged>(a, (unsigned)K, stream);
}

// cnt [F][n] fp32 = the number of tests of feature f on the paths of column r, over all trees.  part
// [slabs][F][n] int32 with slabs = ceil(T / slab_trees): needed (zeroed by the caller) when F > 32, where the
// counters live there, and with more than one slab; may be null otherwise.
H2OMX_API int h2omx_walk_counts(const float* X, int64_t ld, int64_t n, int F, const void* nodes, const int* roots,
                                const uint32_t* catbits, int T, int cap, int slab_trees, int* part, float* cnt,
                                hipStream_t stream) {
  WalkArgs a = common(X, ld, n, F, nodes, roots, catbits, T, cap);
  if (bad_common(a) || slab_trees < 1 || cnt == nullptr) return kBadArg;
  a.slab_trees = slab_trees < T ? slab_trees : T;
  const int slabs = (T + a.slab_trees - 1) / a.slab_trees;
  const bool fold = slabs > 1 || F > kXldsMaxF;
  if (fold && part == nullptr) return kBadArg;
  a.out = cnt, a.part = part;
  const int rc = launch<kCounts>(a, (unsigned)slabs, stream);
  if (rc != kOk || !fold) return rc;
  const int64_t len = (int64_t)F * n;
  const int64_t blocks = (len + kThreads - 1) / kThreads;
  if (blocks > INT32_MAX) return kBadArg;
  walk_fold_kernel<<<(unsigned)blocks, kThreads, 0, stream>>>(part, slabs, len, cnt);
  return launch_status();
}
