// Uplift DRF on gfx950: the four passes of a level-wise uplift tree over the uint8
// binned matrix codes [F][ld] (feature-major, ld a multiple of 4, NA code nbt - 1).
//
//   uplift_hist_kernel<LDS>   category counts [S][F][nbt][4] of one level
//   uplift_split_kernel       best (na_left, feature, bin) of every node
//   uplift_route_kernel       rows to their children, next level's histogram keys
//   uplift_score_kernel<XLDS> every row through every tree, (p_t, p_c) sums
//
// A row belongs to one of four categories, cat = 2 (1 - treated) + y, and every
// statistic of the model is a count of categories: nt = c0 + c1, yt = c1,
// nc = c2 + c3, yc = c3.  The histogram and everything derived from it up to the
// divergences are therefore int32, added with integer atomics whose order cannot
// matter, and prefix-summed exactly.  Nothing here uses a floating-point atomic or
// waits for another workgroup, and every result is bit-identical between calls.
//
// Histogram.  key [n] = slot * 4 + cat, or -1 for a row that is out of bag or not in
// a built child.  A workgroup of four waves owns one feature and one slab of rows; a
// lane reads four consecutive codes as one dword and the four matching keys as one
// 16-byte load.  LDS = true: the counts go to an LDS histogram [S][nbt][4] by LDS
// adds without a return value, and the workgroup's non-zero cells are added to the
// zeroed result at the end.  LDS = false (more slots than the LDS budget holds; the
// rows are then spread over hundreds of nodes): the lanes add straight into the
// result.
//
// Split scan.  One workgroup per node, its waves take the features in turn, the
// lanes of a wave lie along the bins with B = ceil((nbt - 1) / 64) <= 4 adjacent bins
// each.  The four channels are summed over the lane's bins and scanned across the
// wave as integers (Hillis-Steele over cross-lane moves), which gives every lane the
// exact cumulative counts of its bins.  For both NA directions the lane forms the
// validity test and the gain in fp64 with the operations, and their order, of the
// tensor expressions this replaces (the library is built with floating-point
// contraction off): ratios y / n with the node's p, q as fallbacks, the 1e-6 clamps,
// (nL dL + nR dR) / ntot - d_node.  Arg-max per lane, per wave by an xor butterfly,
// per workgroup through LDS; among equal gains the lowest (na_left, feature, bin)
// wins, for which the three are packed into one ascending integer.  No valid
// candidate: gain -inf, split (0, 0, 0).  The winner's left counts are then summed
// again by wave 0.
//
// Route.  A lane per row: level-local node k -> 2 remap[k] + right or -1, and the
// next key, slot * 4 + cat with slot = remap[k] where the row went to the child that
// is built (the smaller one), else -1.  It reads the one code byte it needs.
//
// Score.  nodes [T][M] of 8 bytes {feat int16 (-1 leaf), bin uint8, na_left uint8,
// left int32}, leaves [T][M] {pt, pc} fp64.  A lane owns a row, a workgroup of four
// waves 256 rows, and walks all trees in tree order, adding the leaf pairs to two
// fp64 registers in that order: the sums round as a loop over the trees does.  With
// F <= 256 (XLDS) the workgroup's [F][256] block of codes is staged once in LDS by
// coalesced dword reads; otherwise codes[feat][row] comes from global memory.  A wave
// leaves a tree when a wave vote finds all its lanes on leaves.  The host has checked
// that every inner node's children lie behind it and inside the tree, so a walk ends
// and stays in bounds.
#include "common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kHistRows = kThreads * 4;   // rows of one step of a histogram workgroup
constexpr int kScoreRows = 256;
constexpr int kXldsMaxF = 256;            // widest frame staged in LDS (64 KB)
constexpr int kMaxNbt = 256;
constexpr int kMaxF = 32767;
constexpr double kEps = 1e-6;

enum Metric : int { kKL = 0, kEuclidean = 1, kChiSquared = 2 };

// one split record, 64 bytes (the host reads it as 16 int32)
struct SplitRec {
  double gain;
  int feat, bin, na_left, pad0;
  int left[4];   // nt, yt, nc, yc of the left child
  int node[4];   // ... of the node
  int pad1[2];
};

struct alignas(8) Node {
  int16_t feat;
  uint8_t bin, na_left;
  int32_t left;
};

// ---------------------------------------------------------------- histogram

template <bool LDS>
__device__ __forceinline__ void hist_add(int* __restrict__ cells, int key, uint32_t code, int S, int nbt, int F, int f) {
  if (key < 0 || key >= 4 * S || code >= (uint32_t)nbt) return;
  const int slot = key >> 2, cat = key & 3;
  if (LDS)
    atomicAdd(&cells[(slot * nbt + (int)code) * 4 + cat], 1);
  else
    atomicAdd(&cells[(((int64_t)slot * F + f) * nbt + (int)code) * 4 + cat], 1);
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void uplift_hist_kernel(const uint8_t* __restrict__ codes, int64_t ld,
                                                               const int* __restrict__ key, int64_t n, int F, int nbt,
                                                               int S, int64_t slab_rows, int* __restrict__ H) {
  extern __shared__ int sh[];   // LDS: [S][nbt][4]
  const int tid = threadIdx.x;
  const int f = blockIdx.y;
  const int cells = S * nbt * 4;
  if (LDS) {
    for (int i = tid; i < cells; i += kThreads) sh[i] = 0;
    __syncthreads();
  }
  int* __restrict__ dst = LDS ? sh : H;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = min(n, r0 + slab_rows);
  const uint8_t* __restrict__ cf = codes + (int64_t)f * ld;
  for (int64_t row = r0 + 4 * tid; row < r1; row += kHistRows) {
    const uint32_t c4 = *reinterpret_cast<const uint32_t*>(cf + row);   // row % 4 == 0, row + 3 < ld
    if (row + 3 < n) {
      const int4 k4 = *reinterpret_cast<const int4*>(key + row);
      hist_add<LDS>(dst, k4.x, c4 & 255u, S, nbt, F, f);
      hist_add<LDS>(dst, k4.y, (c4 >> 8) & 255u, S, nbt, F, f);
      hist_add<LDS>(dst, k4.z, (c4 >> 16) & 255u, S, nbt, F, f);
      hist_add<LDS>(dst, k4.w, c4 >> 24, S, nbt, F, f);
    } else {
      for (int j = 0; row + j < n; ++j) hist_add<LDS>(dst, key[row + j], (c4 >> (8 * j)) & 255u, S, nbt, F, f);
    }
  }
  if (LDS) {
    __syncthreads();
    const int per = nbt * 4;
    for (int i = tid; i < cells; i += kThreads) {
      const int v = sh[i];
      if (v != 0) atomicAdd(&H[((int64_t)(i / per) * F + f) * per + i % per], v);
    }
  }
}

// ---------------------------------------------------------------- split scan

__device__ __forceinline__ double ratio(int y, int n, double fallback) {
  return n > 0 ? (double)y / (double)n : fallback;
}

__device__ __forceinline__ double clamp_eps(double v) {
  return fmin(fmax(v, kEps), 1.0 - kEps);
}

__device__ __forceinline__ double divergence(double p, double q, int metric) {
  if (metric == kKL) {
    const double p_ = clamp_eps(p), q_ = clamp_eps(q);
    const double a = p_ * log(p_ / q_);
    const double b = (1.0 - p_) * log((1.0 - p_) / (1.0 - q_));
    return a + b;
  }
  const double d = p - q;
  const double d2 = d * d;
  if (metric == kEuclidean) return 2.0 * d2;
  const double q_ = clamp_eps(q);
  const double a = d2 / q_;
  const double b = d2 / (1.0 - q_);
  return a + b;
}

// (gain, code) better than (g, c): greater gain, or the same gain at a lower code
__device__ __forceinline__ bool better(double gain, int code, double g, int c) {
  return gain > g || (gain == g && code < c);
}

__device__ __forceinline__ int4 stats_of(int4 c) {
  return make_int4(c.x + c.y, c.y, c.z + c.w, c.w);   // nt, yt, nc, yc
}

__device__ __forceinline__ int4 add4(int4 a, int4 b) {
  return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ int4 shfl_xor4(int4 v, int off) {
  return make_int4(__shfl_xor(v.x, off, kWave), __shfl_xor(v.y, off, kWave), __shfl_xor(v.z, off, kWave),
                   __shfl_xor(v.w, off, kWave));
}

__device__ __forceinline__ int4 shfl_up4(int4 v, int off) {
  return make_int4(__shfl_up(v.x, off, kWave), __shfl_up(v.y, off, kWave), __shfl_up(v.z, off, kWave),
                   __shfl_up(v.w, off, kWave));
}

__global__ __launch_bounds__(kThreads) void uplift_split_kernel(const int4* __restrict__ H,
                                                                const uint8_t* __restrict__ fmask,
                                                                const int* __restrict__ nvb, int F, int nbt, int metric,
                                                                double min_rows, SplitRec* __restrict__ out) {
  __shared__ double s_gain[kWaves];
  __shared__ int s_code[kWaves];
  const int k = blockIdx.x;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int nb = nbt - 1;              // value bins; bin nb holds the NA rows
  const int B = (nb + kWave - 1) / kWave;
  const int4* __restrict__ Hk = H + (int64_t)k * F * nbt;

  // the node's totals: all bins of feature 0 (every wave forms them for itself)
  int4 T = make_int4(0, 0, 0, 0);
  for (int b = lane; b < nbt; b += kWave) T = add4(T, stats_of(Hk[b]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) T = add4(T, shfl_xor4(T, off));
  const double pn = ratio(T.y, T.x, 0.0), qn = ratio(T.w, T.z, 0.0);
  const double d_node = divergence(pn, qn, metric);
  const double ntot = fmax((double)(T.x + T.z), 1e-300);

  double best_gain = -INFINITY;
  int best_code = INT32_MAX;           // na_left << 24 | feat << 8 | bin
  for (int f = wave; f < F; f += kWaves) {
    if (!fmask[(int64_t)k * F + f]) continue;
    const int4* __restrict__ Hf = Hk + (int64_t)f * nbt;
    const int nok = min(max(nvb[f] - 1, 0), nb);   // bins below this one are split points
    int4 c[4];
    int4 run = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * B + j;
      if (j < B && b < nb) run = add4(run, stats_of(Hf[b]));
      c[j] = run;                      // inclusive over the lane's own bins
    }
    int4 incl = run;                   // inclusive scan of the lanes' sums
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int4 v = shfl_up4(incl, off);
      if (lane >= off) incl = add4(incl, v);
    }
    const int4 before = make_int4(incl.x - run.x, incl.y - run.y, incl.z - run.z, incl.w - run.w);
    const int4 na = stats_of(Hf[nb]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * B + j;
      if (j >= B || b >= nok) continue;
      const int4 cum = add4(before, c[j]);
#pragma unroll
      for (int na_left = 0; na_left < 2; ++na_left) {
        const int4 L = na_left ? add4(cum, na) : cum;
        const int4 R = make_int4(T.x - L.x, T.y - L.y, T.z - L.z, T.w - L.w);
        const double nL = (double)(L.x + L.z), nR = (double)(R.x + R.z);
        if (!(nL >= min_rows && nR >= min_rows && L.x > 0 && L.z > 0 && R.x > 0 && R.z > 0)) continue;
        const double dL = divergence(ratio(L.y, L.x, pn), ratio(L.w, L.z, qn), metric);
        const double dR = divergence(ratio(R.y, R.x, pn), ratio(R.w, R.z, qn), metric);
        const double wl = nL * dL;
        const double wr = nR * dR;
        const double gain = (wl + wr) / ntot - d_node;
        const int code = na_left << 24 | f << 8 | b;
        if (better(gain, code, best_gain, best_code)) {
          best_gain = gain;
          best_code = code;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double g = __shfl_xor(best_gain, off, kWave);
    const int cd = __shfl_xor(best_code, off, kWave);
    if (better(g, cd, best_gain, best_code)) {
      best_gain = g;
      best_code = cd;
    }
  }
  if (lane == 0) {
    s_gain[wave] = best_gain;
    s_code[wave] = best_code;
  }
  __syncthreads();
  if (wave != 0) return;
  best_gain = s_gain[0];
  best_code = s_code[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (better(s_gain[w], s_code[w], best_gain, best_code)) {
      best_gain = s_gain[w];
      best_code = s_code[w];
    }
  const bool found = best_code != INT32_MAX;
  const int na_left = found ? best_code >> 24 : 0;
  const int feat = found ? (best_code >> 8) & 0xffff : 0;
  const int bin = found ? best_code & 255 : 0;
  // left counts of the reported split: bins 0 .. bin of feat, plus the NA bin where it goes left
  const int4* __restrict__ Hf = Hk + (int64_t)feat * nbt;
  int4 L = make_int4(0, 0, 0, 0);
  for (int b = lane; b <= bin; b += kWave) L = add4(L, stats_of(Hf[b]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) L = add4(L, shfl_xor4(L, off));
  if (na_left) L = add4(L, stats_of(Hf[nb]));
  if (lane == 0) {
    SplitRec r;
    r.gain = best_gain;
    r.feat = feat;
    r.bin = bin;
    r.na_left = na_left;
    r.pad0 = 0;
    r.left[0] = L.x, r.left[1] = L.y, r.left[2] = L.z, r.left[3] = L.w;
    r.node[0] = T.x, r.node[1] = T.y, r.node[2] = T.z, r.node[3] = T.w;
    r.pad1[0] = r.pad1[1] = 0;
    out[k] = r;
  }
}

// ---------------------------------------------------------------- route

__global__ __launch_bounds__(kThreads) void uplift_route_kernel(const uint8_t* __restrict__ codes, int64_t ld, int64_t n,
                                                                int* __restrict__ nid, const int* __restrict__ cat,
                                                                const SplitRec* __restrict__ rec,
                                                                const int* __restrict__ remap,
                                                                const int* __restrict__ built_right, int K, int P, int F,
                                                                int nbt, int* __restrict__ key) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= n) return;
  const int k = nid[row];
  int next = -1, slot_key = -1;
  if (k >= 0 && k < K) {
    const int rk = remap[k];
    const int feat = rec[k].feat;
    if (rk >= 0 && rk < P && feat >= 0 && feat < F) {
      const int c = codes[(int64_t)feat * ld + row];
      const int right = c == nbt - 1 ? (rec[k].na_left == 0) : (c > rec[k].bin);
      next = 2 * rk + right;
      const int ct = cat[row];
      if (right == built_right[rk] && ct >= 0) slot_key = rk * 4 + (ct & 3);
    }
  }
  nid[row] = next;
  key[row] = slot_key;
}

// ---------------------------------------------------------------- score

template <bool XLDS>
__global__ __launch_bounds__(kThreads) void uplift_score_kernel(const uint8_t* __restrict__ codes, int64_t ld, int64_t n,
                                                                int F, const Node* __restrict__ nodes,
                                                                const double2* __restrict__ leaves, int T, int M,
                                                                int nbt, double* __restrict__ pt,
                                                                double* __restrict__ pc) {
  extern __shared__ uint8_t sc[];   // XLDS: [F][256]
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kScoreRows;
  const int64_t row = row0 + tid;
  const bool live = row < n;
  if (XLDS) {
    // wave w takes features w, w + 4, ...; its lanes read one row of 256 codes as 64 dwords
    uint32_t* __restrict__ sw = reinterpret_cast<uint32_t*>(sc);
    const int lane = tid % kWave;
    const int64_t r = row0 + 4 * lane;
    for (int f = tid / kWave; f < F; f += kWaves)
      sw[f * (kScoreRows / 4) + lane] = r < ld ? *reinterpret_cast<const uint32_t*>(codes + (int64_t)f * ld + r) : 0u;
    __syncthreads();
  }
  double at = 0.0, ac = 0.0;
  for (int t = 0; t < T; ++t) {
    const Node* __restrict__ nt = nodes + (int64_t)t * M;
    int node = 0;
    for (int step = 0; step < M; ++step) {
      const Node q = nt[node];
      const bool inner = live && q.feat >= 0;
      if (!__any(inner)) break;
      if (inner) {
        const int c = XLDS ? sc[q.feat * kScoreRows + tid] : codes[(int64_t)q.feat * ld + row];
        const int right = c == nbt - 1 ? (q.na_left == 0) : (c > q.bin);
        node = q.left + right;
      }
    }
    const double2 v = leaves[(int64_t)t * M + node];
    at += v.x;
    ac += v.y;
  }
  if (live) {
    pt[row] = at;
    pc[row] = ac;
  }
}

}  // namespace

// H [S][F][nbt][4] int32 (zeroed by the caller) += category counts of the rows with key >= 0.  codes [F][ld] uint8,
// 4-byte aligned, ld % 4 == 0 and ld >= n rounded up to 4; key [n] int32, 16-byte aligned.  slab_rows a positive
// multiple of 1024.  lds != 0: S * nbt * 16 bytes of LDS per workgroup (at most 64 KB).
H2OMX_API int h2omx_uplift_hist(const uint8_t* codes, int64_t ld, const int* key, int64_t n, int F, int nbt, int S,
                                int64_t slab_rows, int lds, int* H, hipStream_t stream) {
  if (n < 1 || n > INT32_MAX || F < 1 || F > kMaxF || nbt < 2 || nbt > kMaxNbt || S < 1 || ld % 4 != 0 ||
      ld < (n + 3) / 4 * 4 || slab_rows < kHistRows || slab_rows % kHistRows != 0 || (int64_t)S * 4 > INT32_MAX ||
      ((uintptr_t)codes & 3) != 0 || ((uintptr_t)key & 15) != 0)
    return kBadArg;
  const int64_t slabs = (n + slab_rows - 1) / slab_rows;
  const size_t bytes = (size_t)S * nbt * 4 * sizeof(int);
  if (slabs > INT32_MAX || (lds && bytes > 65536)) return kBadArg;
  const dim3 grid((unsigned)slabs, (unsigned)F);
  if (lds)
    uplift_hist_kernel<true><<<grid, kThreads, bytes, stream>>>(codes, ld, key, n, F, nbt, S, slab_rows, H);
  else
    uplift_hist_kernel<false><<<grid, kThreads, 0, stream>>>(codes, ld, key, n, F, nbt, S, slab_rows, H);
  return launch_status();
}

// out [K] 64-byte records = best split of every node of H [K][F][nbt][4] int32 (16-byte aligned) over the features of
// fmask [K][F] (bytes) and the bins below nvb [F] - 1.  metric: 0 KL, 1 Euclidean, 2 ChiSquared.
H2OMX_API int h2omx_uplift_splits(const int* H, const uint8_t* fmask, const int* nvb, int K, int F, int nbt, int metric,
                                  double min_rows, void* out, hipStream_t stream) {
  if (K < 1 || F < 1 || F > kMaxF || nbt < 2 || nbt > kMaxNbt || metric < kKL || metric > kChiSquared ||
      ((uintptr_t)H & 15) != 0 || ((uintptr_t)out & 7) != 0)
    return kBadArg;
  uplift_split_kernel<<<(unsigned)K, kThreads, 0, stream>>>((const int4*)H, fmask, nvb, F, nbt, metric, min_rows,
                                                           (SplitRec*)out);
  return launch_status();
}

// nid [n] (level-local node, -1 done) -> 2 remap[nid] + right or -1, in place; key [n] = remap[nid] * 4 + cat where the
// row went to the child built_right [P] names, else -1.  rec [K]: the records of h2omx_uplift_splits; remap [K] in
// [-1, P).
H2OMX_API int h2omx_uplift_route(const uint8_t* codes, int64_t ld, int64_t n, int* nid, const int* cat, const void* rec,
                                 const int* remap, const int* built_right, int K, int P, int F, int nbt, int* key,
                                 hipStream_t stream) {
  if (n < 1 || n > INT32_MAX || ld < n || K < 1 || P < 1 || F < 1 || F > kMaxF || nbt < 2 || nbt > kMaxNbt)
    return kBadArg;
  uplift_route_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(
      codes, ld, n, nid, cat, (const SplitRec*)rec, remap, built_right, K, P, F, nbt, key);
  return launch_status();
}

// pt, pc [n] fp64 = sums over the T trees, in tree order, of the leaf pairs the rows of codes [F][ld] reach.  nodes
// [T][M] 8-byte records, leaves [T][M] {pt, pc}; every feat < F, every inner node's children behind it and < M (the
// caller has checked both).
H2OMX_API int h2omx_uplift_score(const uint8_t* codes, int64_t ld, int64_t n, int F, const void* nodes,
                                 const void* leaves, int T, int M, int nbt, double* pt, double* pc, hipStream_t stream) {
  if (n < 1 || n > INT32_MAX || ld % 4 != 0 || ld < (n + 3) / 4 * 4 || F < 1 || F > kMaxF || T < 1 || M < 1 || nbt < 2 ||
      nbt > kMaxNbt || ((uintptr_t)codes & 3) != 0 || ((uintptr_t)leaves & 15) != 0)
    return kBadArg;
  const unsigned blocks = (unsigned)((n + kScoreRows - 1) / kScoreRows);
  if (F <= kXldsMaxF)
    uplift_score_kernel<true><<<blocks, kThreads, (size_t)F * kScoreRows, stream>>>(
        codes, ld, n, F, (const Node*)nodes, (const double2*)leaves, T, M, nbt, pt, pc);
  else
    uplift_score_kernel<false><<<blocks, kThreads, 0, stream>>>(codes, ld, n, F, (const Node*)nodes,
                                                                (const double2*)leaves, T, M, nbt, pt, pc);
  return launch_status();
}
