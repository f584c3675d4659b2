// whals.hip — solver='whals': whals_step_kernel, whals_loss_kernel and the cnmf_whals_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// Weighted / masked coordinate descent: hals.hip's Gauss-Seidel sweep for the objective
// ½ Σ m_if (x_if − Σ_j w_ij h_jf)² (+ sklearn's l1 / l2 terms), M >= 0 elementwise (spec:
// tests/whals_ref.py).  The weights couple the features, so the Gram matrix is per sample in the
// W-sweep (G_i = H·diag(m_i)·Hᵀ) and per feature in the H-sweep (G_f = W'ᵀ·diag(m_:f)·W').  One
// iteration is ONE launch with hals_step_kernel's structure:
//   gate   every workgroup reads the control block's STOPPED word and returns without a write when
//          it is set;
//   table  per feature the row [h_0 .. h_KP-1 | h_a·h_b, a <= b] in LDS, from the fp64 Hᵀ;
//   pass   per workgroup, its rows in tiles of X and M staged in LDS (16-byte loads): per sample
//          c_i = Σ_f (m·x)·h_j − l1_W (k sums) and the upper triangle of G_i = Σ_f m·(h_a·h_b)
//          (k(k+1)/2 sums, one FMA per term against the table) in fp64, the k-step sweep in fp64,
//          w' rounded once to W's type, stored, and the rounded value (and its products w'_a·w'_b)
//          accumulated per feature into the fp64 partial row
//          [A = W'ᵀ(M∘X) (k·F) | S = upper triangle of W'ᵀdiag(m_:f)W' (k(k+1)/2 · F) | Σ|pg| | pad],
//          written in full;
//   tail   the last-arriving workgroup (hals.hip's ticket and hand-off) sums the rows in row order,
//          runs the H-sweep with a lane per feature (c_f = A[:,f] − l1_H, G_f = S[:,f] with l2_H on
//          the diagonal), writes H64 / Ht and applies sklearn's rule on the control block
//          (cnmf_hals_slots, as hals_step_kernel's).
// Nothing in the launch waits for another workgroup and every sum has a fixed order, so the same
// inputs give the same bits.  A weight of zero makes x_if drop out of every sum (0·x is ±0), and a
// fully masked row or column has G[t,t] == 0: it keeps its factor row and adds no violation.
// The staging, ticket and row sums are hals.hip's, duplicated under namespace whals.
// ------------------------------------------------------------------------------------------------
namespace whals {
constexpr int MAX_BLOCKS = 256;   // partial rows of a launch, at most (one tail workgroup sums them)
constexpr int ROW_ALIGN = 64;     // rows per workgroup: a multiple (tiles then start 16-byte aligned)
constexpr int TILE_BYTES = 32 * 1024;  // of X, and as much of M, per team
constexpr int MISC = 256;         // bytes at the start of LDS: red[16] doubles, flags
constexpr int KMAX = 8;
constexpr int FMAX4 = 512, FMAX8 = 192;  // widest row for k <= 4 and for 5 <= k <= 8

__host__ __device__ constexpr int tri(int k) { return k * (k + 1) / 2; }
// index of (a, b), a <= b, in the row-major upper triangle of a K x K matrix
__host__ __device__ constexpr int tix(int a, int b, int K) { return a * K - a * (a - 1) / 2 + (b - a); }

__host__ __device__ inline int64_t rows_per_block(int64_t n_rows) {
  int64_t rpb = (n_rows + MAX_BLOCKS - 1) / MAX_BLOCKS;
  return (rpb + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
}
__host__ __device__ inline int64_t blocks(int64_t n_rows) {
  const int64_t rpb = rows_per_block(n_rows);
  return (n_rows + rpb - 1) / rpb;
}
__host__ __device__ inline int row_doubles(int F, int k) { return (k * F + tri(k) * F + 1 + 1) & ~1; }
__host__ __device__ inline bool served(int F, int k) { return k <= 4 ? F <= FMAX4 : (k <= KMAX && F <= FMAX8); }
// rows of a staged tile: 64, 32, 16 or 8 so that the tile (in X's type) fits TILE_BYTES
__host__ __device__ inline int tile_rows(int F, int xbytes) {
  int tr = 64;
  while (tr > 8 && tr * F * xbytes > TILE_BYTES) tr >>= 1;
  return tr;
}
__host__ __device__ inline int tile_bytes(int F, int xbytes) { return (tile_rows(F, xbytes) * F * xbytes + 15) & ~15; }
// feature lanes of the accumulation phase: 64, 128 or 256; a lane owns features fl + s·lanes, s < NF
__host__ __device__ inline int feat_lanes(int F, int nf) { return F <= 64 * nf ? 64 : (F <= 128 * nf ? 128 : 256); }

struct Args {
  const void* X;
  const void* M;
  void* W;
  double* H64;
  double* Ht;
  double* partials;
  uint32_t* counter;
  double* ctl;
  int64_t n_rows;
  int F, k;
  double l1W, l2W, l1H, l2H;
  int flags;  // CNMF_HALS_UPDATE_H
};

// deterministic workgroup sum (fixed shuffle tree, the waves in order); every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < nw; ++w) s += red[w];
  return s;
}

// One Gauss-Seidel sweep of a row r[0..k) (tests/hals_ref.py `sweep`, one row): g is the upper
// triangle of the row's own KP x KP Gram matrix, zero beyond k and with the l2 term on its
// diagonal, c has the l1 term subtracted; r is zero beyond k.  Returns the row's Σ|pg|.
template <int KP>
__device__ __forceinline__ double sweep_tri(const double (&g)[tri(KP)], const double (&c)[KP], double (&r)[KP], int k) {
  double viol = 0.0;
#pragma unroll
  for (int t = 0; t < KP; ++t) {
    if (t < k) {
      double grad = -c[t];
#pragma unroll
      for (int m = 0; m < KP; ++m) grad = fma(g[m < t ? tix(m, t, KP) : tix(t, m, KP)], r[m], grad);
      const double pg = r[t] == 0.0 ? fmin(0.0, grad) : grad;
      viol += fabs(pg);
      const double hess = g[tix(t, t, KP)];
      if (hess != 0.0) r[t] = fmax(r[t] - grad / hess, 0.0);
    }
  }
  return viol;
}

// the ticket: true in every thread of the last-arriving workgroup (which leaves the counter zero)
__device__ __forceinline__ bool last_arriver(uint32_t* counter, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = old == gridDim.x - 1;
    if (flag[0]) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return flag[0] != 0;
}

__device__ __forceinline__ double ld_agent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// column sums of partials[G][RL] in row order into S (LDS): a thread owns columns tid, tid + NTB, ...
__device__ __forceinline__ void sum_rows(const double* partials, int G, int RL, double* S) {
  for (int c = threadIdx.x; c < RL; c += blockDim.x) {
    double s = 0.0;
    for (int b0 = 0; b0 < G; b0 += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = b0 + u < G ? ld_agent(partials + (size_t)(b0 + u) * RL + c) : 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    S[c] = s;
  }
  __syncthreads();
}

// The W-sweep of this workgroup's rows [r0, r1), tile by tile, the tiles round-robin over the
// TEAMS teams; accumulates the partial row of the rounded w' into the caller's registers:
// acc[s][0..KP) is A[:, f], acc[s][KP + tix(a, b, KP)] is S[(a, b), f] for the lane's feature s.
template <typename TX, int KP, int NF, int TEAMS>
__device__ __forceinline__ void pass(const Args& a, unsigned char* smem, int64_t r0, int64_t r1,
                                     double (&acc)[NF][KP + tri(KP)], double& viol) {
  constexpr int TP = tri(KP), VL = KP + TP;
  const int team = threadIdx.x / NT, t = threadIdx.x - team * NT;
  const int F = a.F, k = a.k;
  const int TR = tile_rows(F, (int)sizeof(TX));
  const int TPR = NT / TR;      // sweep phase: lanes per row, 4, 8, 16 or 32
  const int FL = feat_lanes(F, NF);
  const int RG = NT / FL;
  const int TB = tile_bytes(F, (int)sizeof(TX));
  double* sT = reinterpret_cast<double*>(smem + MISC);  // [F][VL]: h_j | h_a·h_b, zero beyond k
  double* sW = sT + (size_t)F * VL + (size_t)team * TR * VL;  // per team [TR][VL]: the rounded w' | w'_a·w'_b
  unsigned char* tiles = reinterpret_cast<unsigned char*>(sT + (size_t)F * VL + (size_t)TEAMS * TR * VL);
  TX* tX = reinterpret_cast<TX*>(tiles + (size_t)team * 2 * TB);  // per team [TR][F] of X, then of M
  TX* tM = reinterpret_cast<TX*>(tiles + (size_t)team * 2 * TB + TB);
  const TX* X = static_cast<const TX*>(a.X);
  const TX* M = static_cast<const TX*>(a.M);
  TX* W = static_cast<TX*>(a.W);

  for (int f = threadIdx.x; f < F; f += NT * TEAMS) {  // the table: a thread per feature
    double h[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) h[j] = j < k ? a.Ht[(size_t)f * KP + j] : 0.0;
    double* row = sT + (size_t)f * VL;
#pragma unroll
    for (int j = 0; j < KP; ++j) row[j] = h[j];
#pragma unroll
    for (int p = 0; p < KP; ++p) {
#pragma unroll
      for (int q = p; q < KP; ++q) row[KP + tix(p, q, KP)] = h[p] * h[q];
    }
  }

  const int ur = t / TPR, uq = t - ur * TPR;  // sweep phase: row of the tile, lane of the row
  const int rg = t / FL, fl = t - rg * FL;    // accumulation phase: row group, feature lane
  const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
  for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {  // the same trip count in every team (barriers)
    const int64_t ti = i * TEAMS + team;
    const int64_t rt = r0 + ti * TR;
    const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
    __syncthreads();  // the previous tile's readers are done (and the table is written)
    {  // the tile's rows are contiguous and start 16-byte aligned in X and in M: whole chunks, then the tail
      const int64_t n_el = (int64_t)nr * F;
      const TX* srcX = X + rt * F;
      const TX* srcM = M + rt * F;
      constexpr int PER = 16 / (int)sizeof(TX);
      const int n16 = (int)(n_el / PER);
      const u32x4* sx16 = reinterpret_cast<const u32x4*>(srcX);
      const u32x4* sm16 = reinterpret_cast<const u32x4*>(srcM);
      u32x4* dx16 = reinterpret_cast<u32x4*>(tX);
      u32x4* dm16 = reinterpret_cast<u32x4*>(tM);
      for (int c0 = t; c0 < n16; c0 += 4 * NT) {  // 4 + 4 loads in flight per thread, then their LDS stores
        u32x4 vx[4], vm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c0 + u * NT < n16) {
            vx[u] = sx16[c0 + u * NT];
            vm[u] = sm16[c0 + u * NT];
          }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c0 + u * NT < n16) {
            dx16[c0 + u * NT] = vx[u];
            dm16[c0 + u * NT] = vm[u];
          }
      }
      for (int e = n16 * PER + t; e < n_el; e += NT) {
        tX[e] = srcX[e];
        tM[e] = srcM[e];
      }
    }
    const bool live = ur < nr;
    const int64_t row = rt + ur;
    double w[KP];  // the row of W: loaded ahead of the sums that its sweep waits for
#pragma unroll
    for (int j = 0; j < KP; ++j) w[j] = (live && j < k) ? (double)W[row * k + j] : 0.0;
    __syncthreads();
    {  // the TPR lanes of row ur sum their features, combine by shuffle (every lane then holds the
       // sums) and sweep; lane 0 of the row stores
      double num[VL];
#pragma unroll
      for (int j = 0; j < VL; ++j) num[j] = 0.0;
      const TX* xr = tX + (size_t)(live ? ur : 0) * F;
      const TX* mr = tM + (size_t)(live ? ur : 0) * F;
      for (int f = uq; f < F; f += TPR) {
        const double m = (double)mr[f];
        const double xm = m * (double)xr[f];
        const double* tv = sT + (size_t)f * VL;
#pragma unroll
        for (int j = 0; j < KP; ++j)
          if (j < k) num[j] = fma(xm, tv[j], num[j]);
#pragma unroll
        for (int p = 0; p < KP; ++p) {
#pragma unroll
          for (int q = p; q < KP; ++q)
            if (q < k) num[KP + tix(p, q, KP)] = fma(m, tv[KP + tix(p, q, KP)], num[KP + tix(p, q, KP)]);
        }
      }
      for (int off = TPR >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < KP; ++j)
          if (j < k) num[j] += __shfl_xor(num[j], off);
#pragma unroll
        for (int p = 0; p < KP; ++p) {
#pragma unroll
          for (int q = p; q < KP; ++q)
            if (q < k) num[KP + tix(p, q, KP)] += __shfl_xor(num[KP + tix(p, q, KP)], off);
        }
      }
      double c[KP], g[TP];
#pragma unroll
      for (int j = 0; j < KP; ++j) c[j] = num[j] - a.l1W;
#pragma unroll
      for (int j = 0; j < TP; ++j) g[j] = num[KP + j];
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) g[tix(j, j, KP)] += a.l2W;
      const double v = sweep_tri<KP>(g, c, w, k);
      if (live && uq == 0) {
        viol += v;
        double wq[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          wq[j] = 0.0;
          if (j < k) {
            const TX q = (TX)w[j];
            W[row * k + j] = q;
            wq[j] = (double)q;
          }
        }
        double* wrow = sW + (size_t)ur * VL;
#pragma unroll
        for (int j = 0; j < KP; ++j) wrow[j] = wq[j];
#pragma unroll
        for (int p = 0; p < KP; ++p) {
#pragma unroll
          for (int q = p; q < KP; ++q) wrow[KP + tix(p, q, KP)] = wq[p] * wq[q];
        }
      }
    }
    __syncthreads();
    // accumulation: thread (rg, fl) owns features fl + s·FL for rows rg, rg + RG, ...
    for (int r = rg; r < nr; r += RG) {
      const double* wv = sW + (size_t)r * VL;
#pragma unroll
      for (int s = 0; s < NF; ++s) {
        const int f = fl + s * FL;
        if (f >= F) continue;
        const double m = (double)tM[(size_t)r * F + f];
        const double xm = m * (double)tX[(size_t)r * F + f];
#pragma unroll
        for (int j = 0; j < KP; ++j)
          if (j < k) acc[s][j] = fma(wv[j], xm, acc[s][j]);
#pragma unroll
        for (int p = 0; p < KP; ++p) {
#pragma unroll
          for (int q = p; q < KP; ++q)
            if (q < k) acc[s][KP + tix(p, q, KP)] = fma(wv[KP + tix(p, q, KP)], m, acc[s][KP + tix(p, q, KP)]);
        }
      }
    }
  }
}

}  // namespace whals

template <typename TX, int KP, int NF, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void whals_step_kernel(whals::Args a) {
  using namespace whals;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_HALS_STOPPED) != 0.0) return;  // the gate
  constexpr int NTB = NT * TEAMS;
  constexpr int TP = tri(KP), VL = KP + TP;
  double* red = reinterpret_cast<double*>(smem);           // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* un = reinterpret_cast<double*>(smem + MISC);     // the union region
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int F = a.F, k = a.k;
  const int kF = k * F, SL = kF + tri(k) * F;  // A | S
  const int RL = row_doubles(F, k);
  const int FL = feat_lanes(F, NF), RG = NT / FL;
  const int rg = t / FL, fl = t - rg * FL;
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;

  double acc[NF][VL], viol = 0.0;
#pragma unroll
  for (int s = 0; s < NF; ++s) {
#pragma unroll
    for (int j = 0; j < VL; ++j) acc[s][j] = 0.0;
  }
  pass<TX, KP, NF, TEAMS>(a, smem, r0, r1, acc, viol);

  // the (team, row group) accumulators through LDS (over the pass's buffers), summed in order
  const int NG = TEAMS * RG;
  __syncthreads();
  {
    double* mine = un + (size_t)(team * RG + rg) * SL;
#pragma unroll
    for (int s = 0; s < NF; ++s) {
      const int f = fl + s * FL;
      if (f >= F) continue;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) mine[j * F + f] = acc[s][j];
#pragma unroll
      for (int p = 0; p < KP; ++p) {
#pragma unroll
        for (int q = p; q < KP; ++q)
          if (q < k) mine[kF + tix(p, q, k) * F + f] = acc[s][KP + tix(p, q, KP)];
      }
    }
  }
  const double bviol = block_sum(viol, red);  // its barriers also publish the scratch
  double* prow = a.partials + (size_t)blockIdx.x * RL;
  for (int e = tid; e < SL; e += NTB) {
    double s = 0.0;
    for (int g = 0; g < NG; ++g) s += un[(size_t)g * SL + e];
    st_agent(prow + e, s);
  }
  if (tid == 0) {
    st_agent(prow + SL, bviol);
    for (int e = SL + 1; e < RL; ++e) st_agent(prow + e, 0.0);
  }
  if (!last_arriver(a.counter, flag)) return;

  // ---- tail: the whole iteration's sums, the H-sweep, the stopping rule
  double* S = un;        // [RL]: A | S | Σ|pg| of the W-sweep
  double* Hn = un + RL;  // [k][F] the new H
  sum_rows(a.partials, (int)gridDim.x, RL, S);
  const bool update_h = a.flags & CNMF_HALS_UPDATE_H;
  double vh = 0.0;
  if (update_h) {
    for (int f = tid; f < F; f += NTB) {  // a lane per feature: the row f of Hᵀ against its own G_f
      double c[KP], h[KP], g[TP];
#pragma unroll
      for (int j = 0; j < TP; ++j) g[j] = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        c[j] = j < k ? S[j * F + f] - a.l1H : 0.0;
        h[j] = j < k ? a.H64[j * F + f] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < KP; ++p) {
#pragma unroll
        for (int q = p; q < KP; ++q)
          if (q < k) g[tix(p, q, KP)] = S[kF + tix(p, q, k) * F + f] + (p == q ? a.l2H : 0.0);
      }
      vh += sweep_tri<KP>(g, c, h, k);
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) Hn[j * F + f] = h[j];
    }
    vh = block_sum(vh, red);  // its barriers: every read of the old H64 is done, Hn is written
    for (int e = tid; e < kF; e += NTB) a.H64[e] = Hn[e];
    for (int e = tid; e < F * KP; e += NTB) {
      const int f = e / KP, j = e - f * KP;
      a.Ht[e] = j < k ? Hn[j * F + f] : 0.0;
    }
  }
  if (tid != 0) return;
  double* c = a.ctl;
  const double violation = S[SL] + vh;  // the sum over both sweeps
  const double it = c[CNMF_HALS_ITERS_DONE] + 1.0;
  c[CNMF_HALS_ITERS_DONE] = it;
  if (it == 1.0) c[CNMF_HALS_VIOL_INIT] = violation;
  const double init = c[CNMF_HALS_VIOL_INIT];
  c[CNMF_HALS_VIOL_LAST] = violation;
  const int64_t cap = (int64_t)c[CNMF_HALS_LOG_CAP], n = (int64_t)c[CNMF_HALS_NLOG];
  if (n < cap) {
    c[CNMF_HALS_LOG + n] = violation;
    c[CNMF_HALS_NLOG] = (double)(n + 1);
  }
  if (init == 0.0 || violation / init <= c[CNMF_HALS_TOL]) st_agent(c + CNMF_HALS_STOPPED, 1.0);
}

// Σ m (x − w·h)² in fp64 from the fp64 H (hals_loss_kernel with the weight): the workgroups and
// their rows as the step's, a wave per row and a lane per feature, H staged in LDS; one double per
// workgroup, the last arriver sums them in row order into out[0].
template <typename TX>
__global__ __launch_bounds__(NT) void whals_loss_kernel(const TX* X, const TX* M, const TX* W, const double* H64,
                                                        double* partials, uint32_t* counter, double* out,
                                                        int64_t n_rows, int F, int k) {
  using namespace whals;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);        // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* sH = reinterpret_cast<double*>(smem + MISC);  // [k][F]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < k * F; e += NT) sH[e] = H64[e];
  __syncthreads();
  const int64_t rpb = rows_per_block(n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  double acc = 0.0;
  for (int64_t r = r0 + wave; r < r1; r += NWAVE) {
    const TX* x = X + r * F;
    const TX* m = M + r * F;
    const TX* w = W + r * k;
    for (int f = lane; f < F; f += 64) {
      double d = (double)x[f];
      for (int j = 0; j < k; ++j) d = fma(-(double)w[j], sH[j * F + f], d);
      acc = fma((double)m[f] * d, d, acc);
    }
  }
  acc = block_sum(acc, red);
  if (tid == 0) st_agent(partials + blockIdx.x, acc);
  if (!last_arriver(counter, flag)) return;
  if (tid != 0) return;
  double s = 0.0;
  for (int b = 0; b < (int)gridDim.x; ++b) s += ld_agent(partials + b);
  out[0] = s;
}

}  // namespace cnmf

using namespace cnmf;

namespace {

size_t whals_lds(int F, int k, int KP, int nf, int xbytes, int teams) {
  using namespace cnmf::whals;
  const int VL = KP + tri(KP), SL = k * F + tri(k) * F;
  const size_t pass = ((size_t)F * VL + (size_t)teams * tile_rows(F, xbytes) * VL) * 8 +
                      (size_t)teams * 2 * tile_bytes(F, xbytes);
  const size_t scratch = (size_t)teams * (NT / feat_lanes(F, nf)) * SL * 8;
  const size_t tail = ((size_t)row_doubles(F, k) + (size_t)k * F) * 8;
  return MISC + std::max(pass, std::max(scratch, tail));
}

template <typename TX, int KP, int NF, int TEAMS>
int whals_launch_t(const whals::Args& a, hipStream_t hs) {
  const size_t lds = whals_lds(a.F, a.k, KP, NF, (int)sizeof(TX), TEAMS);
  if (lds > kMaxLds) return set_err(CNMF_ERR_UNSUPPORTED, "whals step needs %zu bytes of LDS (k=%d, n_features=%d)", lds, a.k, a.F);
  const void* fn = reinterpret_cast<const void*>(&whals_step_kernel<TX, KP, NF, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)whals::blocks(a.n_rows)), block(NT * TEAMS);
  hipLaunchKernelGGL((whals_step_kernel<TX, KP, NF, TEAMS>), grid, block, lds, hs, a);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

// k <= 4: two features per lane and two teams where the workgroup has the tiles and the LDS for
// them; 5 <= k <= 8: one feature per lane (44 accumulators each), one team
template <typename TX>
int whals_launch_k(const whals::Args& a, hipStream_t hs) {
  if (a.k > 4) return whals_launch_t<TX, 8, 1, 1>(a, hs);
  const int tr = whals::tile_rows(a.F, (int)sizeof(TX));
  const int64_t tiles = (whals::rows_per_block(a.n_rows) + tr - 1) / tr;
  if (tiles >= 2 && whals_lds(a.F, a.k, 4, 2, (int)sizeof(TX), 2) <= kMaxLds) return whals_launch_t<TX, 4, 2, 2>(a, hs);
  return whals_launch_t<TX, 4, 2, 1>(a, hs);
}

// the checks the launches share, after their null-pointer checks
int whals_check(const void* X, const void* M, int x_dtype, const void* W, int64_t n_parts, int64_t n_rows,
                int n_features, int k) {
  if (n_rows < 1 || n_features < 1 || k < 1)
    return set_err(CNMF_ERR_SHAPE, "invalid shape: n_rows=%lld F=%d k=%d", (long long)n_rows, n_features, k);
  if (!whals::served(n_features, k))
    return set_err(CNMF_ERR_UNSUPPORTED, "whals: k=%d (1..%d), n_features=%d (1..%d for k <= 4, 1..%d for k <= %d)", k,
                   whals::KMAX, n_features, whals::FMAX4, whals::FMAX8, whals::KMAX);
  if (x_dtype == CNMF_BF16) return set_err(CNMF_ERR_ARG, "whals: bf16 X is not served (fp32 or fp64)");
  if (x_dtype != CNMF_F32 && x_dtype != CNMF_F64) return set_err(CNMF_ERR_ARG, "whals: x_dtype %d (fp32 or fp64)", x_dtype);
  if (const int st = check_xw_aligned(X, W)) return st;
  if (reinterpret_cast<uintptr_t>(M) & 15) return set_err(CNMF_ERR_ALIGN, "M must be 16-byte aligned");
  if (whals::blocks(n_rows) > n_parts)
    return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the launch needs %lld", (long long)n_parts, (long long)whals::blocks(n_rows));
  return CNMF_OK;
}

template <typename TX>
int whals_loss_t(const void* X, const void* M, const void* W, const double* H64, double* partials, uint32_t* counter,
                 double* out, int64_t n_rows, int F, int k, hipStream_t hs) {
  const size_t lds = whals::MISC + (size_t)k * F * 8;
  hipLaunchKernelGGL((whals_loss_kernel<TX>), dim3((unsigned)whals::blocks(n_rows)), dim3(NT), lds, hs,
                     static_cast<const TX*>(X), static_cast<const TX*>(M), static_cast<const TX*>(W), H64, partials,
                     counter, out, n_rows, F, k);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

}  // namespace

extern "C" {

int64_t cnmf_whals_rows(int64_t n_rows) { return n_rows < 1 ? 0 : whals::blocks(n_rows); }

int64_t cnmf_whals_row_doubles(int n_features, int k) {
  if (n_features < 1 || k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: F=%d k=%d", n_features, k);
  if (!whals::served(n_features, k))
    return set_err(CNMF_ERR_UNSUPPORTED, "whals: k=%d (1..%d), n_features=%d (1..%d for k <= 4, 1..%d for k <= %d)", k,
                   whals::KMAX, n_features, whals::FMAX4, whals::FMAX8, whals::KMAX);
  return whals::row_doubles(n_features, k);
}

int cnmf_whals_step(const void* X, const void* M, int x_dtype, void* W, double* H64, double* Ht, double* partials,
                    int64_t n_parts, uint32_t* counter, double* ctl, int64_t n_rows, int n_features, int k,
                    double l1_W, double l2_W, double l1_H, double l2_H, int flags, void* stream) {
  if (!X || !M || !W || !H64 || !Ht || !partials || !counter || !ctl)
    return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (flags & ~CNMF_HALS_UPDATE_H) return set_err(CNMF_ERR_ARG, "flags %d", flags);
  if (const int st = whals_check(X, M, x_dtype, W, n_parts, n_rows, n_features, k)) return st;
  const whals::Args a{X, M, W, H64, Ht, partials, counter, ctl, n_rows, n_features, k, l1_W, l2_W, l1_H, l2_H, flags};
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? whals_launch_k<float>(a, hs) : whals_launch_k<double>(a, hs);
}

int cnmf_whals_loss(const void* X, const void* M, int x_dtype, const void* W, const double* H64, double* partials,
                    int64_t n_parts, uint32_t* counter, double* out, int64_t n_rows, int n_features, int k,
                    void* stream) {
  if (!X || !M || !W || !H64 || !partials || !counter || !out) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = whals_check(X, M, x_dtype, W, n_parts, n_rows, n_features, k)) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? whals_loss_t<float>(X, M, W, H64, partials, counter, out, n_rows, n_features, k, hs)
                             : whals_loss_t<double>(X, M, W, H64, partials, counter, out, n_rows, n_features, k, hs);
}

}  // extern "C"
