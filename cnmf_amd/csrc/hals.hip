// hals.hip — solver='hals': hals_step_kernel, its sharded form (hals_shard_step_kernel, hals_basis_kernel),
// hals_loss_kernel and the cnmf_hals_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// scikit-learn 1.7.2's coordinate-descent NMF solver with shuffle=False (SKCD =
// `_fit_coordinate_descent`, sklearn/decomposition/_nmf.py:376-523, and `_update_cdnmf_fast`,
// _cdnmf_fast.pyx — the "Fast HALS" sweep of Cichocki & Phan) on the device.  One SKCD iteration —
// the W-sweep of every sample, the H-sweep of every feature and the stopping rule — is ONE launch:
//   gate   every workgroup reads the control block's STOPPED word (agent-scope atomic load) and
//          returns without a write when it is set: the host enqueues a stretch of iterations and a
//          stop on the device turns the rest into no-ops;
//   pass   per workgroup, its rows in tiles staged in LDS: c = x·Hᵀ − l1_W in fp64 from the fp64 Hᵀ,
//          the k-step Gauss-Seidel sweep of the sample's row of W against G = HHᵀ (+ l2_W on the
//          diagonal) in fp64, w' rounded once to W's type, stored, and the rounded value used for
//          the fp64 partial row [W'ᵀX (k·F) | W'ᵀW' (k·k) | Σ|pg| | pad], written in full;
//   tail   the last-arriving workgroup (ticket and hand-off as mb_step_kernel: agent-scope relaxed
//          atomic stores of the row, s_waitcnt vmcnt(0), barrier, one fetch_add, agent-scope atomic
//          loads by the last arriver) sums the rows in row order, runs the H-sweep with a lane per
//          feature (C[f,:] = A[:,f] − l1_H, G = B with l2_H on the diagonal), refreshes H64 / Ht /
//          HHt, adds the two violations and applies SKCD's rule: stop when violation_init == 0 or
//          violation / violation_init <= tol, every iteration, also for tol = 0.
// Nothing in the launch waits for another workgroup.  Every sum has a fixed order, so the same
// inputs give the same bits.  The tile arithmetic is mb_step_kernel's (minibatch.hip), duplicated:
// a workgroup is TEAMS teams of 256 threads, each staging and processing its own tiles.
// General tile (1 <= F <= 512, 1 <= k <= 16, fp32 / fp64 X): not tuned per shape.
// Row shards (one rank per GPU) split the launch where the sum over all rows is needed: the last
// arriver of hals_shard_step_kernel writes the summed row to acc and stops there, the host
// all-reduces acc over the ranks, and hals_basis_kernel (one workgroup) runs the tail from it.
// ------------------------------------------------------------------------------------------------
namespace hals {
constexpr int MAX_BLOCKS = 256;   // partial rows of a launch, at most (one tail workgroup sums them)
constexpr int ROW_ALIGN = 64;     // rows per workgroup: a multiple (tiles then start 16-byte aligned)
constexpr int TILE_BYTES = 64 * 1024;
constexpr int MISC = 256;         // bytes at the start of LDS: red[16] doubles, flags
constexpr int FMAX = 512, KMAX = 16;

__host__ __device__ inline int64_t rows_per_block(int64_t n_rows) {
  int64_t rpb = (n_rows + MAX_BLOCKS - 1) / MAX_BLOCKS;
  return (rpb + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
}
__host__ __device__ inline int64_t blocks(int64_t n_rows) {
  const int64_t rpb = rows_per_block(n_rows);
  return (n_rows + rpb - 1) / rpb;
}
__host__ __device__ inline int row_doubles(int F, int k) { return (k * F + k * k + 1 + 1) & ~1; }
// rows of a staged tile: 64, 32 or 16 so that the tile (in X's type) fits TILE_BYTES
__host__ __device__ inline int tile_rows(int F, int xbytes) {
  int tr = 64;
  while (tr > 16 && tr * F * xbytes > TILE_BYTES) tr >>= 1;
  return tr;
}
__host__ __device__ inline int tile_bytes(int F, int xbytes) { return (tile_rows(F, xbytes) * F * xbytes + 15) & ~15; }
// feature lanes of the accumulation phase: 64, 128 or 256; a lane owns features fl and fl + lanes
__host__ __device__ inline int feat_lanes(int F) { return F <= 128 ? 64 : (F <= 256 ? 128 : 256); }

struct Args {
  const void* X;
  void* W;
  double* H64;
  double* Ht;
  double* HHt;
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

// One Gauss-Seidel sweep of a row r[0..k) (`_update_cdnmf_fast`, the identity permutation): G is
// KP x KP in LDS, zero beyond k and with the l2 term on its diagonal, c has the l1 term subtracted;
// r is zero beyond k.  Returns the row's Σ|projected gradient|.
template <int KP>
__device__ __forceinline__ double sweep_row(const double* G, const double (&c)[KP], double (&r)[KP], int k) {
  double viol = 0.0;
#pragma unroll
  for (int t = 0; t < KP; ++t) {
    if (t < k) {
      double grad = -c[t];
#pragma unroll
      for (int m = 0; m < KP; ++m) grad = fma(G[t * KP + m], r[m], grad);
      const double pg = r[t] == 0.0 ? fmin(0.0, grad) : grad;
      viol += fabs(pg);
      const double hess = G[t * KP + t];
      if (hess != 0.0) r[t] = fmax(r[t] - grad / hess, 0.0);
    }
  }
  return viol;
}

// The W-sweep of this workgroup's rows [r0, r1), tile by tile, the tiles round-robin over the
// TEAMS teams; accumulates the partial row of the rounded w' into the caller's registers.
template <typename TX, int KP, int TEAMS>
__device__ __forceinline__ void pass(const Args& a, unsigned char* smem, int64_t r0, int64_t r1,
                                     double (&acc)[2][KP], double (&bacc)[KP], double& viol) {
  const int team = threadIdx.x / NT, t = threadIdx.x - team * NT;
  const int F = a.F, k = a.k;
  const int TR = tile_rows(F, (int)sizeof(TX));
  const int HR = TR / 2;        // sweep phase: a thread works on rows ur and ur + HR of the tile
  const int TPR = NT / HR;      // lanes per row pair: 8, 16 or 32
  const int FL = feat_lanes(F);
  const int RG = NT / FL;
  double* sHt = reinterpret_cast<double*>(smem + MISC);  // [F][KP]
  double* sG = sHt + (size_t)F * KP;                     // [KP][KP]: HHᵀ, l2_W on the diagonal
  double* sW = sG + KP * KP + team * 64 * KP;            // per team [TR][KP]: the rounded w'
  TX* tile = reinterpret_cast<TX*>(reinterpret_cast<unsigned char*>(sG + KP * KP + TEAMS * 64 * KP) +
                                   (size_t)team * tile_bytes(F, (int)sizeof(TX)));  // per team [TR][F], 16-byte aligned
  const TX* X = static_cast<const TX*>(a.X);
  TX* W = static_cast<TX*>(a.W);

  for (int e = threadIdx.x; e < F * KP; e += NT * TEAMS) sHt[e] = a.Ht[e];
  for (int e = threadIdx.x; e < KP * KP; e += NT * TEAMS) {
    const int j = e / KP, m = e - j * KP;
    sG[e] = a.HHt[e] + ((j == m && j < k) ? a.l2W : 0.0);
  }

  const int ur = t / TPR, uq = t - ur * TPR;  // sweep phase: row of the tile, lane of the row
  const int rg = t / FL, fl = t - rg * FL;    // accumulation phase: row group, feature lane
  const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
  for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {  // the same trip count in every team (barriers)
    const int64_t ti = i * TEAMS + team;
    const int64_t rt = r0 + ti * TR;
    const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
    __syncthreads();  // the previous tile's readers are done (and sHt / sG are staged)
    {  // the tile's rows are contiguous and start 16-byte aligned: whole chunks, then the tail
      const int64_t n_el = (int64_t)nr * F;
      const TX* src = X + rt * F;
      constexpr int PER = 16 / (int)sizeof(TX);
      const int n16 = (int)(n_el / PER);
      const u32x4* src16 = reinterpret_cast<const u32x4*>(src);
      u32x4* dst16 = reinterpret_cast<u32x4*>(tile);
      for (int c0 = t; c0 < n16; c0 += 8 * NT) {  // 8 loads in flight per thread, then their LDS stores
        u32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (c0 + u * NT < n16) v[u] = src16[c0 + u * NT];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (c0 + u * NT < n16) dst16[c0 + u * NT] = v[u];
      }
      for (int e = n16 * PER + t; e < n_el; e += NT) tile[e] = src[e];
    }
    __syncthreads();
    {  // lane (ur, uq) sums its features of rows ur and ur + HR (one read of Hᵀ serves both), the
       // pair's lanes combine by shuffle (every lane then holds both sums), the even lanes sweep
       // row ur and the odd lanes row ur + HR; lanes 0 and 1 store
      const bool live[2] = {ur < nr, ur + HR < nr};
      double num[2][KP];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < KP; ++j) num[h][j] = 0.0;
      }
      const TX* x0 = tile + (size_t)(live[0] ? ur : 0) * F;
      const TX* x1 = tile + (size_t)(live[1] ? ur + HR : 0) * F;
      for (int f = uq; f < F; f += TPR) {
        const double xa = (double)x0[f], xb = (double)x1[f];
        const double* h = sHt + (size_t)f * KP;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          num[0][j] = fma(xa, h[j], num[0][j]);
          num[1][j] = fma(xb, h[j], num[1][j]);
        }
      }
      for (int off = TPR >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int j = 0; j < KP; ++j) num[h][j] += __shfl_xor(num[h][j], off);
        }
      }
      const int hh = uq & 1;
      const bool mine = hh ? live[1] : live[0];
      const int64_t row = rt + ur + hh * HR;
      double c[KP], w[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const double n0 = num[0][j], n1 = num[1][j];  // values, then a select: no indexed register array
        c[j] = (hh ? n1 : n0) - a.l1W;
        w[j] = (mine && j < k) ? (double)W[row * k + j] : 0.0;
      }
      const double v = sweep_row<KP>(sG, c, w, k);
      if (mine && uq < 2) {
        viol += v;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          if (j < k) {
            const TX wq = (TX)w[j];
            W[row * k + j] = wq;
            sW[(ur + hh * HR) * KP + j] = (double)wq;
          }
        }
      }
    }
    __syncthreads();
    // accumulation: thread (rg, fl) owns features fl and fl + FL for rows rg, rg + RG, ...;
    // lanes fl < k also own row fl of W'ᵀW'
    for (int r = rg; r < nr; r += RG) {
      double wr[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) wr[j] = j < k ? sW[r * KP + j] : 0.0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int f = fl + s * FL;
        if (f >= F) continue;
        const double x = (double)tile[(size_t)r * F + f];
#pragma unroll
        for (int j = 0; j < KP; ++j) acc[s][j] = fma(wr[j], x, acc[s][j]);
      }
      if (fl < k) {
        double wm = 0.0;
#pragma unroll
        for (int j = 0; j < KP; ++j) wm = j == fl ? wr[j] : wm;
#pragma unroll
        for (int j = 0; j < KP; ++j) bacc[j] = fma(wm, wr[j], bacc[j]);
      }
    }
  }
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

// front and tail: hals_step_kernel's body before and after its sum_rows, duplicated for the
// sharded form's two kernels (sharing them with hals_step_kernel changed its instances' code; as
// with the tile arithmetic, the copy keeps the shipped kernel as it was).  Keep them in step.
// front — after the gate: the W-sweep of this workgroup's rows, its partial row and the ticket.
// True in every thread of the last-arriving workgroup.
template <typename TX, int KP, int TEAMS>
__device__ __forceinline__ bool front(const Args& a, unsigned char* smem) {
  constexpr int NTB = NT * TEAMS;
  double* red = reinterpret_cast<double*>(smem);           // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* un = reinterpret_cast<double*>(smem + MISC);     // the union region
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int F = a.F, k = a.k;
  const int kF = k * F, kk = k * k;
  const int RL = row_doubles(F, k);
  const int FL = feat_lanes(F), RG = NT / FL;
  const int rg = t / FL, fl = t - rg * FL;
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;

  double acc[2][KP], bacc[KP], viol = 0.0;
#pragma unroll
  for (int j = 0; j < KP; ++j) acc[0][j] = acc[1][j] = bacc[j] = 0.0;
  pass<TX, KP, TEAMS>(a, smem, r0, r1, acc, bacc, viol);

  // the (team, row group) accumulators through LDS (over the pass's buffers), summed in order
  const int SL = kF + kk;  // per group: A | B
  const int NG = TEAMS * RG;
  __syncthreads();
  {
    double* mine = un + (size_t)(team * RG + rg) * SL;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int f = fl + s * FL;
      if (f >= F) continue;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) mine[j * F + f] = acc[s][j];
    }
    if (fl < k) {
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) mine[kF + fl * k + j] = bacc[j];
    }
  }
  const double bviol = block_sum(viol, red);  // its barriers also publish the scratch
  double* prow = a.partials + (size_t)blockIdx.x * RL;
  for (int e = tid; e < kF + kk; e += NTB) {
    double s = 0.0;
    for (int g = 0; g < NG; ++g) s += un[(size_t)g * SL + e];
    st_agent(prow + e, s);
  }
  if (tid == 0) {
    st_agent(prow + kF + kk, bviol);
    for (int e = kF + kk + 1; e < RL; ++e) st_agent(prow + e, 0.0);
  }
  return last_arriver(a.counter, flag);
}

// The tail of an iteration, run by one workgroup of NTB threads from the summed row S (LDS, [RL]:
// A | B | Σ|pg| of the W-sweep over all rows): with CNMF_HALS_UPDATE_H the H-sweep with a lane per
// feature into Hn (LDS, [k][F]; KP·KP doubles of scratch follow it) and H64 / Ht / HHt refreshed;
// always the control block's update and the stopping rule.  The H-sweep, H64, Ht and HHt do not
// depend on NTB; the H-sweep's violation is summed per thread (features tid, tid + NTB), then by
// block_sum, so its last bits depend on NTB only when F > NTB.
template <int KP, int NTB>
__device__ __forceinline__ void tail(const Args& a, double* S, double* Hn, double* red) {
  const int tid = threadIdx.x;
  const int F = a.F, k = a.k;
  const int kF = k * F, kk = k * k;
  const bool update_h = a.flags & CNMF_HALS_UPDATE_H;
  double vh = 0.0;
  if (update_h) {
    double* sG = Hn + kF;  // [KP][KP]: W'ᵀW', l2_H on the diagonal, zero beyond k
    for (int e = tid; e < KP * KP; e += NTB) {
      const int j = e / KP, m = e - j * KP;
      sG[e] = (j < k && m < k) ? S[kF + j * k + m] + (j == m ? a.l2H : 0.0) : 0.0;
    }
    __syncthreads();
    for (int f = tid; f < F; f += NTB) {  // a lane per feature: the row f of Hᵀ
      double c[KP], h[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        c[j] = j < k ? S[j * F + f] - a.l1H : 0.0;
        h[j] = j < k ? a.H64[j * F + f] : 0.0;
      }
      vh += sweep_row<KP>(sG, c, h, k);
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
    const int lane = tid & 63, wave = tid >> 6;
    for (int e = wave; e < KP * KP; e += NTB / 64) {
      const int j = e / KP, m = e - j * KP;
      double v = 0.0;
      if (j < k && m < k)
        for (int f = lane; f < F; f += 64) v = fma(Hn[j * F + f], Hn[m * F + f], v);
      v = wave_sum(v);
      if (lane == 0) a.HHt[e] = v;
    }
  }
  if (tid != 0) return;
  double* c = a.ctl;
  const double violation = S[kF + kk] + vh;  // SKCD: the sum over both sweeps
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

}  // namespace hals

template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void hals_step_kernel(hals::Args a) {
  using namespace hals;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_HALS_STOPPED) != 0.0) return;  // the gate
  constexpr int NTB = NT * TEAMS;
  double* red = reinterpret_cast<double*>(smem);           // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* un = reinterpret_cast<double*>(smem + MISC);     // the union region
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int F = a.F, k = a.k;
  const int kF = k * F, kk = k * k;
  const int RL = row_doubles(F, k);
  const int FL = feat_lanes(F), RG = NT / FL;
  const int rg = t / FL, fl = t - rg * FL;
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;

  double acc[2][KP], bacc[KP], viol = 0.0;
#pragma unroll
  for (int j = 0; j < KP; ++j) acc[0][j] = acc[1][j] = bacc[j] = 0.0;
  pass<TX, KP, TEAMS>(a, smem, r0, r1, acc, bacc, viol);

  // the (team, row group) accumulators through LDS (over the pass's buffers), summed in order
  const int SL = kF + kk;  // per group: A | B
  const int NG = TEAMS * RG;
  __syncthreads();
  {
    double* mine = un + (size_t)(team * RG + rg) * SL;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int f = fl + s * FL;
      if (f >= F) continue;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) mine[j * F + f] = acc[s][j];
    }
    if (fl < k) {
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < k) mine[kF + fl * k + j] = bacc[j];
    }
  }
  const double bviol = block_sum(viol, red);  // its barriers also publish the scratch
  double* prow = a.partials + (size_t)blockIdx.x * RL;
  for (int e = tid; e < kF + kk; e += NTB) {
    double s = 0.0;
    for (int g = 0; g < NG; ++g) s += un[(size_t)g * SL + e];
    st_agent(prow + e, s);
  }
  if (tid == 0) {
    st_agent(prow + kF + kk, bviol);
    for (int e = kF + kk + 1; e < RL; ++e) st_agent(prow + e, 0.0);
  }
  if (!last_arriver(a.counter, flag)) return;

  // ---- tail: the whole iteration's sums, the H-sweep, the stopping rule
  double* S = un;        // [RL]: A | B | Σ|pg| of the W-sweep
  double* Hn = un + RL;  // [k][F] the new H
  sum_rows(a.partials, (int)gridDim.x, RL, S);
  const bool update_h = a.flags & CNMF_HALS_UPDATE_H;
  double vh = 0.0;
  if (update_h) {
    double* sG = Hn + kF;  // [KP][KP]: W'ᵀW', l2_H on the diagonal, zero beyond k
    for (int e = tid; e < KP * KP; e += NTB) {
      const int j = e / KP, m = e - j * KP;
      sG[e] = (j < k && m < k) ? S[kF + j * k + m] + (j == m ? a.l2H : 0.0) : 0.0;
    }
    __syncthreads();
    for (int f = tid; f < F; f += NTB) {  // a lane per feature: the row f of Hᵀ
      double c[KP], h[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        c[j] = j < k ? S[j * F + f] - a.l1H : 0.0;
        h[j] = j < k ? a.H64[j * F + f] : 0.0;
      }
      vh += sweep_row<KP>(sG, c, h, k);
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
    const int lane = tid & 63, wave = tid >> 6;
    for (int e = wave; e < KP * KP; e += NTB / 64) {
      const int j = e / KP, m = e - j * KP;
      double v = 0.0;
      if (j < k && m < k)
        for (int f = lane; f < F; f += 64) v = fma(Hn[j * F + f], Hn[m * F + f], v);
      v = wave_sum(v);
      if (lane == 0) a.HHt[e] = v;
    }
  }
  if (tid != 0) return;
  double* c = a.ctl;
  const double violation = S[kF + kk] + vh;  // SKCD: the sum over both sweeps
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

// The sharded iteration's first launch (cnmf_hals_shard_step): hals_step_kernel up to the summed
// row, which the last arriver writes to acc for the all-reduce over the ranks.  No H-sweep, and no
// write to H64 / Ht / HHt / ctl (a.H64 is not read).
template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void hals_shard_step_kernel(hals::Args a, double* acc) {
  using namespace hals;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_HALS_STOPPED) != 0.0) return;  // the gate
  if (!front<TX, KP, TEAMS>(a, smem)) return;
  const int RL = row_doubles(a.F, a.k);
  double* S = reinterpret_cast<double*>(smem + MISC);
  sum_rows(a.partials, (int)gridDim.x, RL, S);
  for (int c = threadIdx.x; c < RL; c += NT * TEAMS) acc[c] = S[c];
}

// The sharded iteration's second launch (cnmf_hals_basis), one workgroup: the step's tail from the
// all-reduced row.  Every rank runs it on the same acc, H64 and ctl, so every rank gets the same H
// and takes the same decision.
template <int KP>
__global__ __launch_bounds__(NT) void hals_basis_kernel(const double* acc, double* H64, double* Ht, double* HHt,
                                                        double* ctl, int F, int k, double l1H, double l2H, int flags) {
  using namespace hals;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(ctl + CNMF_HALS_STOPPED) != 0.0) return;  // the gate
  const int RL = row_doubles(F, k);
  double* un = reinterpret_cast<double*>(smem + MISC);
  double* S = un;
  double* Hn = un + RL;
  for (int c = threadIdx.x; c < RL; c += NT) S[c] = acc[c];
  __syncthreads();
  const Args a{nullptr, nullptr, H64, Ht, HHt, nullptr, nullptr, ctl, 0, F, k, 0.0, 0.0, l1H, l2H, flags};
  tail<KP, NT>(a, S, Hn, reinterpret_cast<double*>(smem));
}

// ‖X − W·H‖² in fp64 from the fp64 H (SK:85-129 before the square root), for every shape the step
// serves: the workgroups and their rows as the step's, a wave per row and a lane per feature, H
// staged in LDS; one double per workgroup, the last arriver sums them in row order into out[0].
template <typename TX>
__global__ __launch_bounds__(NT) void hals_loss_kernel(const TX* X, const TX* W, const double* H64, double* partials,
                                                       uint32_t* counter, double* out, int64_t n_rows, int F, int k) {
  using namespace hals;
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
    const TX* w = W + r * k;
    for (int f = lane; f < F; f += 64) {
      double d = (double)x[f];
      for (int j = 0; j < k; ++j) d = fma(-(double)w[j], sH[j * F + f], d);
      acc = fma(d, d, acc);
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

size_t hals_lds(int F, int k, int KP, int xbytes, int teams) {
  using namespace cnmf::hals;
  const size_t pass = ((size_t)F * KP + KP * KP + (size_t)teams * 64 * KP) * 8 + (size_t)teams * tile_bytes(F, xbytes);
  const size_t scratch = (size_t)teams * (NT / feat_lanes(F)) * (k * F + k * k) * 8;
  const size_t tail = ((size_t)row_doubles(F, k) + (size_t)k * F + KP * KP) * 8;
  return MISC + std::max(pass, std::max(scratch, tail));
}

// acc null: the one-launch step; else the sharded iteration's first launch, which leaves the summed row in acc
template <typename TX, int KP, int TEAMS>
int hals_launch_t(const hals::Args& a, double* acc, hipStream_t hs) {
  const size_t lds = hals_lds(a.F, a.k, KP, (int)sizeof(TX), TEAMS);
  if (lds > kMaxLds) return set_err(CNMF_ERR_UNSUPPORTED, "hals step needs %zu bytes of LDS", lds);
  const void* fn = acc ? reinterpret_cast<const void*>(&hals_shard_step_kernel<TX, KP, TEAMS>)
                       : reinterpret_cast<const void*>(&hals_step_kernel<TX, KP, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)hals::blocks(a.n_rows)), block(NT * TEAMS);
  if (acc)
    hipLaunchKernelGGL((hals_shard_step_kernel<TX, KP, TEAMS>), grid, block, lds, hs, a, acc);
  else
    hipLaunchKernelGGL((hals_step_kernel<TX, KP, TEAMS>), grid, block, lds, hs, a);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

// teams per workgroup: as many as the registers of the instance (KP) and the LDS allow, and no
// more than the workgroup has tiles
template <typename TX>
int hals_launch_k(const hals::Args& a, double* acc, hipStream_t hs) {
  const int KP = a.k <= 4 ? 4 : (a.k <= 8 ? 8 : 16);
  const int64_t tiles = (hals::rows_per_block(a.n_rows) + hals::tile_rows(a.F, (int)sizeof(TX)) - 1) /
                        hals::tile_rows(a.F, (int)sizeof(TX));
  auto fits = [&](int teams) {
    return tiles >= teams && hals_lds(a.F, a.k, KP, (int)sizeof(TX), teams) <= kMaxLds;
  };
  if (KP == 4) {
    if (fits(4)) return hals_launch_t<TX, 4, 4>(a, acc, hs);
    if (fits(2)) return hals_launch_t<TX, 4, 2>(a, acc, hs);
    return hals_launch_t<TX, 4, 1>(a, acc, hs);
  }
  if (KP == 8) {
    if (fits(2)) return hals_launch_t<TX, 8, 2>(a, acc, hs);
    return hals_launch_t<TX, 8, 1>(a, acc, hs);
  }
  return hals_launch_t<TX, 16, 1>(a, acc, hs);
}

}  // namespace

extern "C" {

int64_t cnmf_hals_rows(int64_t n_rows) { return n_rows < 1 ? 0 : hals::blocks(n_rows); }

int64_t cnmf_hals_row_doubles(int n_features, int k) {
  if (n_features < 1 || k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: F=%d k=%d", n_features, k);
  if (k > hals::KMAX || n_features > hals::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "hals: k=%d (1..%d), n_features=%d (1..%d)", k, hals::KMAX, n_features, hals::FMAX);
  return hals::row_doubles(n_features, k);
}

int64_t cnmf_hals_ctl_doubles(int64_t log_cap) {
  if (log_cap < 0) return set_err(CNMF_ERR_ARG, "log_cap < 0");
  return CNMF_HALS_LOG + log_cap;
}

}  // extern "C"

namespace {

// the checks the launches over X share, after their null-pointer checks
int hals_check(const void* X, int x_dtype, const void* W, int64_t n_parts, int64_t n_rows, int n_features, int k) {
  if (n_rows < 1 || n_features < 1 || k < 1)
    return set_err(CNMF_ERR_SHAPE, "invalid shape: n_rows=%lld F=%d k=%d", (long long)n_rows, n_features, k);
  if (k > hals::KMAX || n_features > hals::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "hals: k=%d (1..%d), n_features=%d (1..%d)", k, hals::KMAX, n_features, hals::FMAX);
  if (x_dtype == CNMF_BF16) return set_err(CNMF_ERR_ARG, "hals: bf16 X is not served (fp32 or fp64)");
  if (x_dtype != CNMF_F32 && x_dtype != CNMF_F64) return set_err(CNMF_ERR_ARG, "hals: x_dtype %d (fp32 or fp64)", x_dtype);
  if (const int st = check_xw_aligned(X, W)) return st;
  if (hals::blocks(n_rows) > n_parts)
    return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the launch needs %lld", (long long)n_parts, (long long)hals::blocks(n_rows));
  return CNMF_OK;
}

template <typename TX>
int hals_loss_t(const void* X, const void* W, const double* H64, double* partials, uint32_t* counter, double* out,
                int64_t n_rows, int F, int k, hipStream_t hs) {
  const size_t lds = hals::MISC + (size_t)k * F * 8;
  const void* fn = reinterpret_cast<const void*>(&hals_loss_kernel<TX>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((hals_loss_kernel<TX>), dim3((unsigned)hals::blocks(n_rows)), dim3(NT), lds, hs,
                     static_cast<const TX*>(X), static_cast<const TX*>(W), H64, partials, counter, out, n_rows, F, k);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

// the tail's LDS (hals_lds's `tail` term): S, Hn and the H-sweep's G
template <int KP>
int hals_basis_t(const double* acc, double* H64, double* Ht, double* HHt, double* ctl, int F, int k, double l1H,
                 double l2H, int flags, hipStream_t hs) {
  const size_t lds = hals::MISC + ((size_t)hals::row_doubles(F, k) + (size_t)k * F + KP * KP) * 8;
  const void* fn = reinterpret_cast<const void*>(&hals_basis_kernel<KP>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((hals_basis_kernel<KP>), dim3(1), dim3(NT), lds, hs, acc, H64, Ht, HHt, ctl, F, k, l1H, l2H, flags);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

}  // namespace

extern "C" {

int cnmf_hals_step(const void* X, int x_dtype, void* W, double* H64, double* Ht, double* HHt, double* partials,
                   int64_t n_parts, uint32_t* counter, double* ctl, int64_t n_rows, int n_features, int k,
                   double l1_W, double l2_W, double l1_H, double l2_H, int flags, void* stream) {
  if (!X || !W || !H64 || !Ht || !HHt || !partials || !counter || !ctl)
    return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (flags & ~CNMF_HALS_UPDATE_H) return set_err(CNMF_ERR_ARG, "flags %d", flags);
  if (const int st = hals_check(X, x_dtype, W, n_parts, n_rows, n_features, k)) return st;
  const hals::Args a{X, W, H64, Ht, HHt, partials, counter, ctl, n_rows, n_features, k, l1_W, l2_W, l1_H, l2_H, flags};
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? hals_launch_k<float>(a, nullptr, hs) : hals_launch_k<double>(a, nullptr, hs);
}

int cnmf_hals_shard_step(const void* X, int x_dtype, void* W, const double* Ht, const double* HHt, double* partials,
                         int64_t n_parts, uint32_t* counter, const double* ctl, double* acc, int64_t n_rows,
                         int n_features, int k, double l1_W, double l2_W, void* stream) {
  if (!X || !W || !Ht || !HHt || !partials || !counter || !ctl || !acc)
    return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = hals_check(X, x_dtype, W, n_parts, n_rows, n_features, k)) return st;
  if (reinterpret_cast<uintptr_t>(acc) & 15) return set_err(CNMF_ERR_ALIGN, "acc must be 16-byte aligned");
  const hals::Args a{X, W, nullptr, const_cast<double*>(Ht), const_cast<double*>(HHt), partials, counter,
                     const_cast<double*>(ctl), n_rows, n_features, k, l1_W, l2_W, 0.0, 0.0, 0};
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? hals_launch_k<float>(a, acc, hs) : hals_launch_k<double>(a, acc, hs);
}

int cnmf_hals_basis(const double* acc, double* H64, double* Ht, double* HHt, double* ctl, int n_features, int k,
                    double l1_H, double l2_H, int flags, void* stream) {
  if (!acc || !H64 || !Ht || !HHt || !ctl) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (flags & ~CNMF_HALS_UPDATE_H) return set_err(CNMF_ERR_ARG, "flags %d", flags);
  if (n_features < 1 || k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: F=%d k=%d", n_features, k);
  if (k > hals::KMAX || n_features > hals::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "hals: k=%d (1..%d), n_features=%d (1..%d)", k, hals::KMAX, n_features, hals::FMAX);
  if (reinterpret_cast<uintptr_t>(acc) & 15) return set_err(CNMF_ERR_ALIGN, "acc must be 16-byte aligned");
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return k <= 4 ? hals_basis_t<4>(acc, H64, Ht, HHt, ctl, n_features, k, l1_H, l2_H, flags, hs)
       : k <= 8 ? hals_basis_t<8>(acc, H64, Ht, HHt, ctl, n_features, k, l1_H, l2_H, flags, hs)
                : hals_basis_t<16>(acc, H64, Ht, HHt, ctl, n_features, k, l1_H, l2_H, flags, hs);
}

int cnmf_hals_loss(const void* X, int x_dtype, const void* W, const double* H64, double* partials, int64_t n_parts,
                   uint32_t* counter, double* out, int64_t n_rows, int n_features, int k, void* stream) {
  if (!X || !W || !H64 || !partials || !counter || !out) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = hals_check(X, x_dtype, W, n_parts, n_rows, n_features, k)) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? hals_loss_t<float>(X, W, H64, partials, counter, out, n_rows, n_features, k, hs)
                             : hals_loss_t<double>(X, W, H64, partials, counter, out, n_rows, n_features, k, hs);
}

}  // extern "C"
