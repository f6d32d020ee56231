// Cox proportional hazards: one Newton pass (partial log-likelihood, gradient,
// Hessian) and Harrell's concordance for gfx950, all fp64, O(n p) memory.
//
// The rows are sorted once per fit by (stratum, stop time descending) and the
// distinct event times of a stratum are numbered in the same order (buckets;
// every stratum ends with one bucket without events that takes the rows below
// its last event time, so a bucket index is never "none").  Row i carries
// b(i), the first bucket whose time is <= stop_i, and with start times b'(i),
// the same for start_i; it is in the risk set of bucket u iff b(i) <= u < b'(i).
//
//   cox_row_sums_kernel   stream over the rows in bucket order: eta, r = w e^eta,
//                         per-bucket sums of r, r x and, over the event rows,
//                         r, r x, count, w, w eta
//   cox_fold_kernel       adds the carry records of the row pass in unit order
//   cox_scan_*            per-stratum prefix sums over the buckets (reduce,
//                         offsets, scan), the six Efron / Breslow scalars per
//                         bucket, ll and grad partials, the suffix sums of c_u
//   cox_row_weight_kernel omega_i = r_i (Csuf[b] - Csuf[b'] - event_i g_b)
//   cox_wxty_kernel       C = sum_i omega_i y_i z_i^T on v_mfma_f64_16x16x4_f64
//   cox_concord_kernel    tiled pair counts in 64-bit integers
//
// Nothing here uses a floating-point atomic or waits for another workgroup;
// every sum has a fixed order, so results are bit-identical between calls.
//
// Split of the row pass.  A unit is P2 = pow2 >= p adjacent lanes (64 / P2
// units per wave, one wave per workgroup) and owns `unit_rows` consecutive
// rows; lane c of the unit reads column c, so a unit reads its row as one
// contiguous segment, four rows in flight.  eta is a butterfly over the unit's
// lanes, after which every lane holds r.  The segmented reduction on the bucket
// key lives in registers: a lane keeps the running sums of its column (and,
// redundantly, of the scalar channels), and when the key changes it writes the
// finished bucket.  A bucket that starts and ends inside the unit is written
// straight to the bucket tables, once; the unit's first and last bucket go out
// as carry records, which cox_fold_kernel adds per bucket in unit order.
#include "common.h"

namespace {

constexpr int kFoldThreads = 192;   // >= 2 * 64 + 5 record channels
constexpr int kScanThreads = 128;   // >= 64 + 2 channels
constexpr int kMaxChunk = 1024;     // buckets per scan workgroup (LDS arrays)
constexpr int kSmallTies = 8;       // Efron terms up to here: one lane per bucket
constexpr int kConcTile = 256;

typedef double d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- row pass

// Record layout (MAIN: 2p + 5 channels, else p + 1): B1[p] B0 | A1[p] A0 m dw we
template <bool MAIN>
struct RowAcc {
  double b1 = 0, b0 = 0, a1 = 0, a0 = 0, m = 0, dw = 0, we = 0;
  __device__ void record(double* rec, int p, int c) const {
    if (c < p) rec[c] = b1;
    if (c == 0) rec[p] = b0;
    if (MAIN) {
      if (c < p) rec[p + 1 + c] = a1;
      if (c == 0) { rec[2 * p + 1] = a0; rec[2 * p + 2] = m; rec[2 * p + 3] = dw; rec[2 * p + 4] = we; }
    }
  }
  __device__ void direct(int64_t u, int64_t nb, int p, int c, double* B1, double* A1, double* sc) const {
    if (c < p) B1[u * p + c] = b1;
    if (c == 0) sc[u] = b0;
    if (MAIN) {
      if (c < p) A1[u * p + c] = a1;
      if (c == 0) { sc[nb + u] = a0; sc[2 * nb + u] = m; sc[3 * nb + u] = dw; sc[4 * nb + u] = we; }
    }
  }
};

template <bool MAIN>
__global__ __launch_bounds__(kWave) void cox_row_sums_kernel(
    const double* __restrict__ X, int64_t n, int p, int P2, int unit_rows, const int* __restrict__ perm,
    const int* __restrict__ key, const double* __restrict__ beta, const double* __restrict__ w,
    const double* __restrict__ ev, double* __restrict__ eta_out, double* __restrict__ r_io,
    double* __restrict__ B1, double* __restrict__ A1, double* __restrict__ sc, int64_t nb,
    int* __restrict__ rec_key, double* __restrict__ rec) {
  const int lane = threadIdx.x;
  const int c = lane & (P2 - 1);
  const int64_t unit = (int64_t)blockIdx.x * (kWave / P2) + lane / P2;
  const int64_t r0 = unit * unit_rows;
  const int64_t r1 = r0 + unit_rows < n ? r0 + unit_rows : n;   // r1 <= r0: the unit has no rows
  const bool col = c < p;
  const int RC = MAIN ? 2 * p + 5 : p + 1;
  const double bc = (MAIN && col) ? beta[c] : 0.0;
  RowAcc<MAIN> acc;
  int cur = r0 < n ? key[r0] : -1;
  bool first = true;
  for (int64_t t0 = r0; t0 < r0 + unit_rows; t0 += 4) {   // same trip count in every lane (shuffles below)
    int kk[4];
    double x[4], ww[4], ee[4], rr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t row = t0 + u;
      const bool v = row < r1;
      const int64_t src = v ? (MAIN ? row : (int64_t)perm[row]) : 0;
      kk[u] = v ? key[row] : -1;
      x[u] = (v && col) ? X[src * p + c] : 0.0;
      if (MAIN) {
        ww[u] = v ? w[src] : 0.0;
        ee[u] = v ? ev[src] : 0.0;
      } else {
        rr[u] = v ? r_io[src] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double eta = 0.0, r;
      if (MAIN) {
        eta = x[u] * bc;
        for (int off = P2 >> 1; off > 0; off >>= 1) eta += __shfl_xor(eta, off, kWave);
        r = ww[u] * exp(eta);
        if (kk[u] >= 0 && c == 0) { eta_out[t0 + u] = eta; r_io[t0 + u] = r; }
      } else {
        r = rr[u];
      }
      if (kk[u] < 0) continue;
      if (kk[u] != cur) {
        if (first) {
          acc.record(rec + (2 * unit) * RC, p, c);
          if (c == 0) rec_key[2 * unit] = cur;
          first = false;
        } else {
          acc.direct(cur, nb, p, c, B1, A1, sc);
        }
        acc = RowAcc<MAIN>();
        cur = kk[u];
      }
      acc.b1 += r * x[u];
      acc.b0 += r;
      if (MAIN) {
        const double er = ee[u] * r, ew = ee[u] * ww[u];
        acc.a1 += er * x[u];
        acc.a0 += er;
        acc.m += ee[u];
        acc.dw += ew;
        acc.we += ew * eta;
      }
    }
  }
  if (r0 >= n) return;
  // a unit inside one bucket: that bucket is its first record, the second is a zero of the same key
  acc.record(rec + (2 * unit + (first ? 0 : 1)) * RC, p, c);
  if (first) RowAcc<MAIN>().record(rec + (2 * unit + 1) * RC, p, c);
  if (c == 0) {
    if (first) rec_key[2 * unit] = cur;
    rec_key[2 * unit + 1] = cur;
  }
}

// One workgroup per record, one thread per channel; the first record of a run of
// equal keys (they are adjacent: keys do not decrease along the units) adds the run.
__global__ __launch_bounds__(kFoldThreads) void cox_fold_kernel(
    const int* __restrict__ rec_key, const double* __restrict__ rec, int64_t nrec, int p, int main_pass,
    double* __restrict__ B1, double* __restrict__ A1, double* __restrict__ sc, int64_t nb) {
  const int64_t j = blockIdx.x;
  const int ch = threadIdx.x;
  const int RC = main_pass ? 2 * p + 5 : p + 1;
  if (ch >= RC) return;
  const int u = rec_key[j];
  if (j > 0 && rec_key[j - 1] == u) return;
  double s = 0.0;
  for (int64_t jj = j; jj < nrec && rec_key[jj] == u; ++jj) s += rec[jj * RC + ch];
  if (ch < p) B1[(int64_t)u * p + ch] = s;
  else if (ch == p) sc[u] = s;
  else if (ch <= 2 * p) A1[(int64_t)u * p + ch - p - 1] = s;
  else sc[(int64_t)(ch - 2 * p) * nb + u] = s;
}

// ------------------------------------------------------------- bucket stage

struct BucketArgs {
  const double *B1, *sc;          // main pass: [nb][p], [5][nb] = B0 A0 m dw we
  const double *Bp1, *Bp0;        // start-time pass (null without start times)
  const double* A1;
  const int *sstart, *send;       // first / last bucket of each bucket's stratum
  int64_t nb;
  int p, chunk, efron;
  double *agg, *off;              // [chunks][p + 1]
  double *S1;                     // out [nb][p]
  double *scal;                   // out [7][nb] = L c g c2 d2 e2 Csuf
  double *gpart, *llpart, *cpart, *coff;   // [chunks][p], [chunks] x 3
  const double* gw;               // sum over events of w x
  double *ll, *grad;
};

__device__ __forceinline__ double bucket_delta(const BucketArgs& a, int64_t u, int c) {
  if (c < a.p) return a.B1[u * a.p + c] - (a.Bp1 ? a.Bp1[u * a.p + c] : 0.0);
  return a.sc[u] - (a.Bp0 ? a.Bp0[u] : 0.0);
}

__global__ __launch_bounds__(kScanThreads) void cox_scan_reduce_kernel(BucketArgs a) {
  const int c = threadIdx.x;
  if (c > a.p) return;
  const int64_t u0 = (int64_t)blockIdx.x * a.chunk;
  const int64_t u1 = u0 + a.chunk < a.nb ? u0 + a.chunk : a.nb;
  double acc = 0.0;
  for (int64_t u = u0; u < u1; ++u) {
    if (a.sstart[u] == u) acc = 0.0;
    acc += bucket_delta(a, u, c);
  }
  a.agg[(int64_t)blockIdx.x * (a.p + 1) + c] = acc;
}

__global__ __launch_bounds__(kScanThreads) void cox_scan_offsets_kernel(BucketArgs a, int chunks) {
  const int c = threadIdx.x;
  if (c > a.p) return;
  double run = 0.0;
  for (int k = 0; k < chunks; ++k) {
    a.off[(int64_t)k * (a.p + 1) + c] = run;
    const int64_t u0 = (int64_t)k * a.chunk;
    const int64_t ul = (u0 + a.chunk < a.nb ? u0 + a.chunk : a.nb) - 1;
    if (a.sstart[ul] >= u0) run = 0.0;   // a stratum starts in this chunk
    run += a.agg[(int64_t)k * (a.p + 1) + c];
  }
}

// six sums over the Efron terms k0, k0 + step, ... < m of one bucket
__device__ __forceinline__ void efron_terms(double S0, double A0, double m, double s, int k0, int step, int mi,
                                            double* t) {
  for (int k = k0; k < mi; k += step) {
    const double f = k / m, phi = S0 - f * A0, q = s / phi, q2 = q / phi;
    t[0] += s * log(phi);
    t[1] += q;
    t[2] += q * f;
    t[3] += q2;
    t[4] += q2 * f;
    t[5] += q2 * f * f;
  }
}

__global__ __launch_bounds__(kScanThreads) void cox_bucket_scalars_kernel(BucketArgs a) {
  __shared__ double sS0[kMaxChunk], sL[kMaxChunk], sC[kMaxChunk], sG[kMaxChunk];
  __shared__ double sred[kScanThreads / kWave][6];
  const int tid = threadIdx.x;
  const int p = a.p;
  const int64_t nb = a.nb;
  const int64_t u0 = (int64_t)blockIdx.x * a.chunk;
  const int cnt = (int)((u0 + a.chunk < nb ? u0 + a.chunk : nb) - u0);
  // 1. per-stratum prefix sums of the bucket sums, one thread per channel
  if (tid <= p) {
    double acc = a.off[(int64_t)blockIdx.x * (p + 1) + tid];
    for (int j = 0; j < cnt; ++j) {
      const int64_t u = u0 + j;
      if (a.sstart[u] == u) acc = 0.0;
      acc += bucket_delta(a, u, tid);
      if (tid < p) a.S1[u * p + tid] = acc;
      else sS0[j] = acc;
    }
  }
  __syncthreads();
  // 2. tie scalars: lanes along the buckets for few terms, along the terms for many
  for (int j = tid; j < cnt; j += kScanThreads) {
    const int64_t u = u0 + j;
    const double m = a.sc[2 * nb + u], dw = a.sc[3 * nb + u];
    double t[6] = {0, 0, 0, 0, 0, 0};
    if (m > 0 && dw > 0) {
      if (!a.efron) efron_terms(sS0[j], 0.0, 1.0, dw, 0, 1, 1, t);
      else if (m <= kSmallTies) efron_terms(sS0[j], a.sc[nb + u], m, dw / m, 0, 1, (int)m, t);
    }
    sL[j] = t[0]; sC[j] = t[1]; sG[j] = t[2];
    a.scal[3 * nb + u] = t[3]; a.scal[4 * nb + u] = t[4]; a.scal[5 * nb + u] = t[5];
  }
  __syncthreads();
  if (a.efron) {
    for (int j = 0; j < cnt; ++j) {
      const int64_t u = u0 + j;
      const double m = a.sc[2 * nb + u], dw = a.sc[3 * nb + u];
      if (!(m > kSmallTies && dw > 0)) continue;   // the same in every thread
      double t[6] = {0, 0, 0, 0, 0, 0};
      efron_terms(sS0[j], a.sc[nb + u], m, dw / m, tid, kScanThreads, (int)m, t);
#pragma unroll
      for (int q = 0; q < 6; ++q) t[q] = wave_sum(t[q]);
      if ((tid & (kWave - 1)) == 0)
        for (int q = 0; q < 6; ++q) sred[tid / kWave][q] = t[q];
      __syncthreads();
      if (tid == 0) {
        for (int q = 0; q < 6; ++q) {
          double s = sred[0][q];
          for (int wv = 1; wv < kScanThreads / kWave; ++wv) s += sred[wv][q];
          t[q] = s;
        }
        sL[j] = t[0]; sC[j] = t[1]; sG[j] = t[2];
        a.scal[3 * nb + u] = t[3]; a.scal[4 * nb + u] = t[4]; a.scal[5 * nb + u] = t[5];
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < cnt; j += kScanThreads) {
    a.scal[u0 + j] = sL[j]; a.scal[nb + u0 + j] = sC[j]; a.scal[2 * nb + u0 + j] = sG[j];
  }
  // 3. this chunk's share of grad and ll, and of the suffix sums of c
  if (tid < p) {
    double g = 0.0;
    for (int j = 0; j < cnt; ++j) g += sC[j] * a.S1[(u0 + j) * p + tid] - sG[j] * a.A1[(u0 + j) * p + tid];
    a.gpart[(int64_t)blockIdx.x * p + tid] = g;
  } else if (tid == p) {
    double l = 0.0;
    for (int j = 0; j < cnt; ++j) l += a.sc[4 * nb + u0 + j] - sL[j];
    a.llpart[blockIdx.x] = l;
  } else if (tid == p + 1) {
    double s = 0.0;   // what this chunk hands to the one before it: c from its start to the first stratum end
    for (int j = 0; j < cnt; ++j) {
      s += sC[j];
      if (a.send[u0 + j] == u0 + j) break;
    }
    a.cpart[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kScanThreads) void cox_finalize_kernel(BucketArgs a, int chunks) {
  const int tid = threadIdx.x;
  if (tid < a.p) {
    double g = 0.0;
    for (int k = 0; k < chunks; ++k) g += a.gpart[(int64_t)k * a.p + tid];
    a.grad[tid] = a.gw[tid] - g;
  } else if (tid == a.p) {
    double l = 0.0;
    for (int k = 0; k < chunks; ++k) l += a.llpart[k];
    a.ll[0] = l;
  } else if (tid == a.p + 1) {
    double run = 0.0;
    for (int k = chunks - 1; k >= 0; --k) {
      a.coff[k] = run;
      const int64_t u0 = (int64_t)k * a.chunk;
      const int64_t ul = (u0 + a.chunk < a.nb ? u0 + a.chunk : a.nb) - 1;
      if (a.send[u0] <= ul) run = 0.0;   // a stratum ends in this chunk
      run += a.cpart[k];
    }
  }
}

// one thread per chunk: Csuf[u] = c_u + (u ends its stratum ? 0 : Csuf[u + 1])
__global__ void cox_csuf_kernel(BucketArgs a, int chunks) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= chunks) return;
  const int64_t u0 = (int64_t)k * a.chunk;
  const int64_t u1 = u0 + a.chunk < a.nb ? u0 + a.chunk : a.nb;
  double run = a.coff[k];
  for (int64_t u = u1 - 1; u >= u0; --u) {
    if (a.send[u] == u) run = 0.0;
    run += a.scal[a.nb + u];
    a.scal[6 * a.nb + u] = run;
  }
}

__global__ void cox_row_weight_kernel(const double* __restrict__ r, const double* __restrict__ ev,
                                      const int* __restrict__ b, const int* __restrict__ bp,
                                      const double* __restrict__ scal, int64_t nb, int64_t n,
                                      double* __restrict__ omega) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int u = b[i];
  double s = scal[6 * nb + u] - ev[i] * scal[2 * nb + u];
  if (bp) s -= scal[6 * nb + bp[i]];
  omega[i] = r[i] * s;
}

// ---------------------------------------------------------- weighted product

// Workgroup = one slab of rows, wave = one 16x16 tile of C.  Per issue the
// instruction reduces 4 rows: lane l feeds A[a = l % 16][row l / 16] = om y and
// B[row l / 16][b = l % 16] = z, each 16 lanes reading one 128-byte row segment;
// the result sits as C[4 v + l / 16][l % 16] in register v.  The tiles of a slab
// share their row segments through the cache.
__global__ void cox_wxty_kernel(const double* __restrict__ Y, const double* __restrict__ Z,
                                const double* __restrict__ om, int64_t n, int p, int64_t slab_rows, int sym,
                                double* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int T = (p + 15) / 16;
  int ta = 0, tb = wave;
  if (sym) {   // tiles on or above the diagonal, row by row
    int rem = wave;
    while (rem >= T - ta) { rem -= T - ta; ++ta; }
    tb = ta + rem;
  } else {
    ta = wave / T;
    tb = wave % T;
  }
  const int ca = ta * 16 + (lane & 15), cb = tb * 16 + (lane & 15);
  const bool va = ca < p, vb = cb < p;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  d4 acc = {0, 0, 0, 0};
  for (int64_t t0 = r0; t0 < r1; t0 += 16) {   // 4 issues in flight
    double av[4], bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = t0 + 4 * q + (lane >> 4);
      const bool v = row < r1;
      av[q] = (v && va) ? om[row] * Y[row * p + ca] : 0.0;
      bv[q] = (v && vb) ? Z[row * p + cb] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
  }
  double* out = part + ((int64_t)blockIdx.x * (blockDim.x / kWave) + wave) * 256;
#pragma unroll
  for (int v = 0; v < 4; ++v) out[(4 * v + (lane >> 4)) * 16 + (lane & 15)] = acc[v];
}

// one thread per element of a tile: the slabs in order
__global__ void cox_wxty_fold_kernel(const double* __restrict__ part, int slabs, int tiles, int p, int sym,
                                     double* __restrict__ C) {
  const int tile = blockIdx.x, e = threadIdx.x;
  const int T = (p + 15) / 16;
  int ta = 0, tb = tile;
  if (sym) {
    int rem = tile;
    while (rem >= T - ta) { rem -= T - ta; ++ta; }
    tb = ta + rem;
  } else {
    ta = tile / T;
    tb = tile % T;
  }
  const int i = ta * 16 + e / 16, j = tb * 16 + e % 16;
  if (i >= p || j >= p) return;
  double s = 0.0;
  for (int k = 0; k < slabs; ++k) s += part[((int64_t)k * tiles + tile) * 256 + e];
  C[i * p + j] = s;
  if (sym && ta != tb) C[j * p + i] = s;
}

// -------------------------------------------------------------- concordance

// thread = one event row, the rows j of this workgroup's share pass through LDS
__global__ __launch_bounds__(kConcTile) void cox_concord_kernel(
    const double* __restrict__ te, const double* __restrict__ lpe, int64_t ne, const double* __restrict__ t,
    const double* __restrict__ lp, int64_t n, int64_t share, unsigned long long* __restrict__ part) {
  __shared__ double st[kConcTile], sl[kConcTile];
  __shared__ unsigned long long sred[kConcTile / kWave][3];
  const int tid = threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * kConcTile + tid;
  const bool live = e < ne;
  const double t_e = live ? te[e] : 0.0, lp_e = live ? lpe[e] : 0.0;
  const int64_t j0 = (int64_t)blockIdx.y * share;
  const int64_t j1 = j0 + share < n ? j0 + share : n;
  unsigned long long gt = 0, eq = 0, tot = 0;
  for (int64_t b = j0; b < j1; b += kConcTile) {
    const int cnt = (int)(j1 - b < kConcTile ? j1 - b : kConcTile);
    __syncthreads();
    if (tid < cnt) { st[tid] = t[b + tid]; sl[tid] = lp[b + tid]; }
    __syncthreads();
    if (live) {
      unsigned g = 0, q = 0, c = 0;
      for (int j = 0; j < cnt; ++j) {
        const bool comp = st[j] > t_e;
        c += comp;
        g += comp && lp_e > sl[j];
        q += comp && lp_e == sl[j];
      }
      gt += g; eq += q; tot += c;
    }
  }
  unsigned long long v[3] = {gt, eq, tot};
#pragma unroll
  for (int q = 0; q < 3; ++q)
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, kWave);
  if ((tid & (kWave - 1)) == 0)
    for (int q = 0; q < 3; ++q) sred[tid / kWave][q] = v[q];
  __syncthreads();
  if (tid < 3) {
    unsigned long long s = 0;
    for (int wv = 0; wv < kConcTile / kWave; ++wv) s += sred[wv][tid];
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + tid] = s;
  }
}

__global__ void cox_concord_fold_kernel(const unsigned long long* __restrict__ part, int64_t blocks,
                                        unsigned long long* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= 3) return;
  unsigned long long s = 0;
  for (int64_t k = 0; k < blocks; ++k) s += part[k * 3 + q];
  out[q] = s;
}

int pow2_at_least(int p) {
  int v = 1;
  while (v < p) v <<= 1;
  return v;
}

}  // namespace

// Row pass over n rows walked in bucket-key order.  Main pass (perm == null):
// computes eta and r from X, beta, w and fills B1 A1 sc[5][nb]; start-time pass
// (perm != null): reads r, walks X[perm[i]] with key[i], fills B1 and sc[1][nb].
// The bucket tables must be zero on entry.  rec_key [2 units], rec [2 units][2p + 5].
H2OMX_API int h2omx_cox_row_sums(const double* X, int64_t n, int p, int unit_rows, const int* perm, const int* key,
                                 const double* beta, const double* w, const double* ev, double* eta, double* r,
                                 double* B1, double* A1, double* sc, int64_t nb, int* rec_key, double* rec,
                                 hipStream_t stream) {
  if (n < 1 || p < 1 || p > 64 || unit_rows < 4 || unit_rows % 4 || nb < 1) return kBadArg;
  const int P2 = pow2_at_least(p);
  const int64_t units = (n + unit_rows - 1) / unit_rows;
  const int64_t per_wave = kWave / P2;
  const unsigned grid = (unsigned)((units + per_wave - 1) / per_wave);
  if (perm == nullptr) {
    cox_row_sums_kernel<true><<<grid, kWave, 0, stream>>>(X, n, p, P2, unit_rows, perm, key, beta, w, ev, eta, r, B1,
                                                          A1, sc, nb, rec_key, rec);
  } else {
    cox_row_sums_kernel<false><<<grid, kWave, 0, stream>>>(X, n, p, P2, unit_rows, perm, key, beta, w, ev, eta, r,
                                                           B1, A1, sc, nb, rec_key, rec);
  }
  cox_fold_kernel<<<(unsigned)(2 * units), kFoldThreads, 0, stream>>>(rec_key, rec, 2 * units, p, perm == nullptr,
                                                                      B1, A1, sc, nb);
  return launch_status();
}

// Prefix sums, tie scalars, ll, grad and Csuf.  work: [chunks][3 (p + 1) + 3] doubles
// with chunks = ceil(nb / chunk).  scal [7][nb] = L c g c2 d2 e2 Csuf, S1 [nb][p].
H2OMX_API int h2omx_cox_bucket_stage(const double* B1, const double* sc, const double* Bp1, const double* Bp0,
                                     const double* A1, const int* sstart, const int* send, int64_t nb, int p,
                                     int chunk, int efron, const double* gw, double* work, double* S1, double* scal,
                                     double* ll, double* grad, hipStream_t stream) {
  if (nb < 1 || p < 1 || p > 64 || chunk < 1 || chunk > kMaxChunk) return kBadArg;
  const int chunks = (int)((nb + chunk - 1) / chunk);
  BucketArgs a;
  a.B1 = B1; a.sc = sc; a.Bp1 = Bp1; a.Bp0 = Bp0; a.A1 = A1; a.sstart = sstart; a.send = send;
  a.nb = nb; a.p = p; a.chunk = chunk; a.efron = efron;
  a.agg = work;
  a.off = a.agg + (int64_t)chunks * (p + 1);
  a.gpart = a.off + (int64_t)chunks * (p + 1);
  a.llpart = a.gpart + (int64_t)chunks * p;
  a.cpart = a.llpart + chunks;
  a.coff = a.cpart + chunks;
  a.S1 = S1; a.scal = scal; a.gw = gw; a.ll = ll; a.grad = grad;
  cox_scan_reduce_kernel<<<chunks, kScanThreads, 0, stream>>>(a);
  cox_scan_offsets_kernel<<<1, kScanThreads, 0, stream>>>(a, chunks);
  cox_bucket_scalars_kernel<<<chunks, kScanThreads, 0, stream>>>(a);
  cox_finalize_kernel<<<1, kScanThreads, 0, stream>>>(a, chunks);
  cox_csuf_kernel<<<(chunks + 63) / 64, 64, 0, stream>>>(a, chunks);
  return launch_status();
}

H2OMX_API int h2omx_cox_row_weight(const double* r, const double* ev, const int* b, const int* bp,
                                   const double* scal, int64_t nb, int64_t n, double* omega, hipStream_t stream) {
  if (n < 1) return kBadArg;
  cox_row_weight_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(r, ev, b, bp, scal, nb, n, omega);
  return launch_status();
}

// C[p][p] = sum_i om_i y_i z_i^T; Y == Z computes the upper tiles and mirrors them.
// part: [slabs][tiles][256] doubles, slabs = ceil(n / slab_rows), tiles = T (T + 1) / 2 or T T.
H2OMX_API int h2omx_cox_wxty(const double* Y, const double* Z, const double* om, int64_t n, int p,
                             int64_t slab_rows, double* part, double* C, hipStream_t stream) {
  if (n < 1 || p < 1 || p > 64 || slab_rows < 16 || slab_rows % 16) return kBadArg;
  const int T = (p + 15) / 16;
  const int sym = Y == Z;
  const int tiles = sym ? T * (T + 1) / 2 : T * T;
  const int slabs = (int)((n + slab_rows - 1) / slab_rows);
  cox_wxty_kernel<<<slabs, tiles * kWave, 0, stream>>>(Y, Z, om, n, p, slab_rows, sym, part);
  cox_wxty_fold_kernel<<<tiles, 256, 0, stream>>>(part, slabs, tiles, p, sym, C);
  return launch_status();
}

// counts[3] = pairs (event e, row j with t_j > t_e) with lp_e > lp_j, with lp_e == lp_j, all.
// part: [ysplit][ceil(ne / 256)][3] 64-bit counts.
H2OMX_API int h2omx_cox_concordance(const double* te, const double* lpe, int64_t ne, const double* t,
                                    const double* lp, int64_t n, int ysplit, unsigned long long* part,
                                    unsigned long long* counts, hipStream_t stream) {
  if (ne < 1 || n < 1 || ysplit < 1 || ysplit > 65535) return kBadArg;
  const int64_t eb = (ne + kConcTile - 1) / kConcTile;
  const int64_t share = ((n + ysplit - 1) / ysplit + kConcTile - 1) / kConcTile * kConcTile;
  cox_concord_kernel<<<dim3((unsigned)eb, (unsigned)ysplit), kConcTile, 0, stream>>>(te, lpe, ne, t, lp, n, share,
                                                                                     part);
  cox_concord_fold_kernel<<<1, 64, 0, stream>>>(part, eb * ysplit, counts);
  return launch_status();
}
