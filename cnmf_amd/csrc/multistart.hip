// multistart.hip — factorise_multistart: ms_step_kernel (one HALS iteration of a batch of starts in
// one launch, X staged once per tile), ms_loss_kernel and the cnmf_ms_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// R starts of solver='hals' (hals.hip: scikit-learn 1.7.2's coordinate-descent solver with
// shuffle=False, SKCD) share one launch per iteration.  The starts are independent fits of the same
// X: start s has its own W_s (n x k), H64_s, Ht_s, HHt_s and control words, laid out start-major.
//   gate   every workgroup reads the STOPPED word of every start of the batch (agent-scope atomic
//          loads) into a wave-uniform mask of the live starts; an empty mask returns without a
//          write, and a stopped start is skipped everywhere below: its W, partial row, H64 / Ht /
//          HHt and control words keep their bits;
//   pass   per workgroup, its rows in tiles staged in LDS ONCE; then for every live start the
//          arithmetic of hals_step_kernel's tile: c = x·Hᵀ_s − l1_W in fp64, the Gauss-Seidel sweep
//          against G_s = H_sH_sᵀ (+ l2_W), w' rounded once to W's type, stored, and the rounded
//          value accumulated into the start's [W'ᵀX | W'ᵀW' | Σ|pg|];
//   tail   the last-arriving workgroup, for every live start in turn: the partial rows summed in
//          row order, the H-sweep, H64_s / Ht_s / HHt_s, ITERS_DONE, VIOL_INIT, VIOL_LAST and STOPPED
//          under SKCD's rule (every iteration, also for tol = 0; violation_init == 0 stops).
// Where the accumulators live: hals_step_kernel keeps acc[2][KP] + bacc[KP] doubles per thread in
// registers across the workgroup's tiles; R copies do not fit (262 registers at KP = 16 for one).
// Here every start has an LDS region [Hᵀ | G | w' of the tile | Σ|pg| slots | accumulators], the
// accumulators with one slot per owner lane ((team, row group) x [A | B], the layout the final
// in-order sum reads): after a tile a lane loads its slots of start s into the registers of one
// start, runs the fma chain over the tile's rows and stores them back, so the register need is
// hals_step_kernel's whatever R is, and the chain of a slot is the same as in registers.
// Measured, this batched launch is slower than as many cnmf_hals_step launches: the
// workgroup's waves run the starts one after the other, and the LDS the slots take leaves fewer
// teams per workgroup.  So cnmf_ms_batch is 1 in the product library, where cnmf_ms_step hands its
// one start to cnmf_hals_step (the same control words, partial rows and gate) and ms_step_kernel is
// not compiled; the diagnostic library (-DCNMF_DIAG) holds it behind CNMF_MS_TEAMS, where its tests
// and tools/bench_multistart.py run it.  ms_loss_kernel is in both.
// Independence: start s reads and writes only its own region, its own global arrays and the shared
// read-only tile; TEAMS, the tile shape and every order of summation follow from (F, k, X's type)
// alone, never from R, the batch or the other starts' state.  So the bits of start s do not depend
// on what else is in the launch.  Nothing waits for another workgroup; every sum has a fixed order.
// The tile staging, the sweep, the ticket and sum_rows are hals.hip's, duplicated (sharing the
// bodies changed the instruction lists of the shipped step kernels).
// ------------------------------------------------------------------------------------------------
namespace ms {
constexpr int MAX_BLOCKS = 256;   // partial rows of a launch, at most (one tail workgroup sums them)
constexpr int ROW_ALIGN = 64;     // rows per workgroup: a multiple (tiles then start 16-byte aligned)
constexpr int TILE_BYTES = 64 * 1024;
constexpr int MISC = 256;         // bytes at the start of LDS: red[16] doubles, flags
constexpr int FMAX = 512, KMAX = 16;
constexpr int RBMAX = 8;          // starts of one launch, at most

__host__ __device__ inline int64_t rows_per_block(int64_t n_rows) {
  int64_t rpb = (n_rows + MAX_BLOCKS - 1) / MAX_BLOCKS;
  return (rpb + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
}
__host__ __device__ inline int64_t blocks(int64_t n_rows) {
  const int64_t rpb = rows_per_block(n_rows);
  return (n_rows + rpb - 1) / rpb;
}
__host__ __device__ inline int row_doubles(int F, int k) { return (k * F + k * k + 1 + 1) & ~1; }
__host__ __device__ inline int tile_rows(int F, int xbytes) {
  int tr = 64;
  while (tr > 16 && tr * F * xbytes > TILE_BYTES) tr >>= 1;
  return tr;
}
__host__ __device__ inline int tile_bytes(int F, int xbytes) { return (tile_rows(F, xbytes) * F * xbytes + 15) & ~15; }
// feature lanes of the accumulation phase: the fewest row groups (each has accumulator slots of
// its own in LDS) that keep a lane at two features at most
__host__ __device__ inline int feat_lanes(int F) { return F <= 64 ? 64 : (F <= 128 ? 128 : 256); }
// doubles of one start's LDS region: Hᵀ [F][KP] | G [KP][KP] | per team w' [64][KP] | per team Σ|pg|
// slots [64] | per (team, row group) [A (k·F) | B (k·k)]; even, so that the tiles stay 16-byte aligned
__host__ __device__ inline int start_doubles(int F, int k, int KP, int teams) {
  const int ng = teams * (NT / feat_lanes(F));
  return (F * KP + KP * KP + teams * 64 * KP + teams * 64 + ng * (k * F + k * k) + 1) & ~1;
}

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
  int F, k, R;
  double l1W, l2W, l1H, l2H;
  int flags;  // CNMF_MS_UPDATE_H
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

// One Gauss-Seidel sweep of a row r[0..k) (`_update_cdnmf_fast`, the identity permutation): see
// hals::sweep_row.  Returns the row's Σ|projected gradient|.
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

// column sums over the G workgroups' rows of one start (RL doubles each, `stride` doubles apart) in
// row order into S (LDS): a thread owns columns tid, tid + NTB, ...
__device__ __forceinline__ void sum_rows(const double* partials, int G, size_t stride, int RL, double* S) {
  for (int c = threadIdx.x; c < RL; c += blockDim.x) {
    double s = 0.0;
    for (int b0 = 0; b0 < G; b0 += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = b0 + u < G ? ld_agent(partials + (size_t)(b0 + u) * stride + c) : 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    S[c] = s;
  }
  __syncthreads();
}

// the wave-uniform mask of the batch's live starts
__device__ __forceinline__ uint32_t live_starts(const double* ctl, int R) {
  uint32_t live = 0;
  for (int s = 0; s < R; ++s)
    if (ld_agent(ctl + (size_t)s * CNMF_MS_STRIDE + CNMF_MS_STOPPED) == 0.0) live |= 1u << s;
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)live);
}

}  // namespace ms

#ifdef CNMF_DIAG
template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void ms_step_kernel(ms::Args a) {
  using namespace ms;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t live = live_starts(a.ctl, a.R);  // the gate
  if (live == 0) return;
  constexpr int NTB = NT * TEAMS;
  double* red = reinterpret_cast<double*>(smem);           // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* un = reinterpret_cast<double*>(smem + MISC);     // the starts' regions; the tail's union
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int F = a.F, k = a.k;
  const int R = a.R;
  const int kF = k * F, kk = k * k;
  const int RL = row_doubles(F, k);
  const int FL = feat_lanes(F), RG = NT / FL;
  const int rg = t / FL, fl = t - rg * FL;
  const int SL = kF + kk;  // per (team, row group): A | B
  const int NG = TEAMS * RG;
  const int PS = start_doubles(F, k, KP, TEAMS);
  // offsets within a start's region
  const int oG = F * KP, oW = oG + KP * KP, oV = oW + TEAMS * 64 * KP, oA = oV + TEAMS * 64;
  const int TR = tile_rows(F, (int)sizeof(TX));
  const int HR = TR / 2;        // sweep phase: a thread works on rows ur and ur + HR of the tile
  const int TPR = NT / HR;      // lanes per row pair: 8, 16 or 32
  const int ur = t / TPR, uq = t - ur * TPR;  // sweep phase: row of the tile, lane of the row
  TX* tile = reinterpret_cast<TX*>(reinterpret_cast<unsigned char*>(un + (size_t)R * PS) +
                                   (size_t)team * tile_bytes(F, (int)sizeof(TX)));  // per team [TR][F]
  const TX* X = static_cast<const TX*>(a.X);
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;

  for (int s = 0; s < R; ++s) {  // every live start's Hᵀ and G staged, its slots zeroed
    if (!((live >> s) & 1u)) continue;
    double* reg = un + (size_t)s * PS;
    const double* Ht = a.Ht + (size_t)s * F * KP;
    const double* HHt = a.HHt + (size_t)s * KP * KP;
    for (int e = tid; e < F * KP; e += NTB) reg[e] = Ht[e];
    for (int e = tid; e < KP * KP; e += NTB) {
      const int j = e / KP, m = e - j * KP;
      reg[oG + e] = HHt[e] + ((j == m && j < k) ? a.l2W : 0.0);
    }
    for (int e = oV + tid; e < PS; e += NTB) reg[e] = 0.0;
  }

  const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
  for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {  // the same trip count in every team (barriers)
    const int64_t ti = i * TEAMS + team;
    const int64_t rt = r0 + ti * TR;
    const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
    __syncthreads();  // the previous tile's readers are done (and the starts' regions are staged)
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
    // every live start's sums and sweep of the tile's rows (hals::pass, per start): lane (ur, uq)
    // sums its features of rows ur and ur + HR, the pair's lanes combine by shuffle, the even
    // lanes sweep row ur and the odd lanes row ur + HR; lanes 0 and 1 store
    for (int s = 0; s < R; ++s) {
      if (!((live >> s) & 1u)) continue;
      double* reg = un + (size_t)s * PS;
      const double* sHt = reg;
      const double* sG = reg + oG;
      double* sW = reg + oW + team * 64 * KP;
      double* sV = reg + oV + team * 64;
      TX* W = static_cast<TX*>(a.W) + (size_t)s * (size_t)a.n_rows * k;
      const bool lv[2] = {ur < nr, ur + HR < nr};
      double num[2][KP];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < KP; ++j) num[h][j] = 0.0;
      }
      const TX* x0 = tile + (size_t)(lv[0] ? ur : 0) * F;
      const TX* x1 = tile + (size_t)(lv[1] ? ur + HR : 0) * F;
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
      const bool mine = hh ? lv[1] : lv[0];
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
        sV[ur + hh * HR] += v;  // the slot of this lane alone, tile after tile
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
    // accumulation, per live start: thread (rg, fl) owns features fl and fl + FL for rows rg,
    // rg + RG, ...; lanes fl < k also own row fl of W'ᵀW'.  The owner's slots come into registers,
    // take the tile's rows and go back.
    for (int s = 0; s < R; ++s) {
      if (!((live >> s) & 1u)) continue;
      double* reg = un + (size_t)s * PS;
      const double* sW = reg + oW + team * 64 * KP;
      double* slot = reg + oA + (size_t)(team * RG + rg) * SL;
      double acc[2][KP], bacc[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int f = fl + q * FL;
          acc[q][j] = (j < k && f < F) ? slot[j * F + f] : 0.0;
        }
        bacc[j] = (j < k && fl < k) ? slot[kF + fl * k + j] : 0.0;
      }
      for (int r = rg; r < nr; r += RG) {
        double wr[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) wr[j] = j < k ? sW[r * KP + j] : 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int f = fl + q * FL;
          if (f >= F) continue;
          const double x = (double)tile[(size_t)r * F + f];
#pragma unroll
          for (int j = 0; j < KP; ++j) acc[q][j] = fma(wr[j], x, acc[q][j]);
        }
        if (fl < k) {
          double wm = 0.0;
#pragma unroll
          for (int j = 0; j < KP; ++j) wm = j == fl ? wr[j] : wm;
#pragma unroll
          for (int j = 0; j < KP; ++j) bacc[j] = fma(wm, wr[j], bacc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        if (j < k) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int f = fl + q * FL;
            if (f < F) slot[j * F + f] = acc[q][j];
          }
          if (fl < k) slot[kF + fl * k + j] = bacc[j];
        }
      }
    }
  }

  // every live start's partial row: the (team, row group) slots summed in order, Σ|pg| by block_sum
  __syncthreads();
  for (int s = 0; s < R; ++s) {
    if (!((live >> s) & 1u)) continue;
    const double* reg = un + (size_t)s * PS;
    const double* slots = reg + oA;
    const double viol = uq < 2 ? reg[oV + team * 64 + ur + (uq & 1) * HR] : 0.0;
    const double bviol = block_sum(viol, red);
    double* prow = a.partials + ((size_t)blockIdx.x * R + s) * RL;
    for (int e = tid; e < SL; e += NTB) {
      double sum = 0.0;
      for (int g = 0; g < NG; ++g) sum += slots[(size_t)g * SL + e];
      st_agent(prow + e, sum);
    }
    if (tid == 0) {
      st_agent(prow + SL, bviol);
      for (int e = SL + 1; e < RL; ++e) st_agent(prow + e, 0.0);
    }
  }
  if (!last_arriver(a.counter, flag)) return;

  // ---- tail, per live start: the whole iteration's sums, the H-sweep, the stopping rule
  double* S = un;        // [RL]: A | B | Σ|pg| of the W-sweep
  double* Hn = un + RL;  // [k][F] the new H
  double* tG = Hn + kF;  // [KP][KP]: W'ᵀW', l2_H on the diagonal, zero beyond k
  const bool update_h = a.flags & CNMF_MS_UPDATE_H;
  for (int s = 0; s < R; ++s) {
    if (!((live >> s) & 1u)) continue;
    __syncthreads();  // the previous start's readers of S and Hn are done
    double* H64 = a.H64 + (size_t)s * kF;
    double* Ht = a.Ht + (size_t)s * F * KP;
    double* HHt = a.HHt + (size_t)s * KP * KP;
    sum_rows(a.partials + (size_t)s * RL, (int)gridDim.x, (size_t)R * RL, RL, S);
    double vh = 0.0;
    if (update_h) {
      for (int e = tid; e < KP * KP; e += NTB) {
        const int j = e / KP, m = e - j * KP;
        tG[e] = (j < k && m < k) ? S[kF + j * k + m] + (j == m ? a.l2H : 0.0) : 0.0;
      }
      __syncthreads();
      for (int f = tid; f < F; f += NTB) {  // a lane per feature: the row f of Hᵀ
        double c[KP], h[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          c[j] = j < k ? S[j * F + f] - a.l1H : 0.0;
          h[j] = j < k ? H64[j * F + f] : 0.0;
        }
        vh += sweep_row<KP>(tG, c, h, k);
#pragma unroll
        for (int j = 0; j < KP; ++j)
          if (j < k) Hn[j * F + f] = h[j];
      }
      vh = block_sum(vh, red);  // its barriers: every read of the old H64 is done, Hn is written
      for (int e = tid; e < kF; e += NTB) H64[e] = Hn[e];
      for (int e = tid; e < F * KP; e += NTB) {
        const int f = e / KP, j = e - f * KP;
        Ht[e] = j < k ? Hn[j * F + f] : 0.0;
      }
      const int lane = tid & 63, wave = tid >> 6;
      for (int e = wave; e < KP * KP; e += NTB / 64) {
        const int j = e / KP, m = e - j * KP;
        double v = 0.0;
        if (j < k && m < k)
          for (int f = lane; f < F; f += 64) v = fma(Hn[j * F + f], Hn[m * F + f], v);
        v = wave_sum(v);
        if (lane == 0) HHt[e] = v;
      }
    }
    if (tid == 0) {
      double* c = a.ctl + (size_t)s * CNMF_MS_STRIDE;
      const double violation = S[kF + kk] + vh;  // SKCD: the sum over both sweeps
      const double it = c[CNMF_MS_ITERS_DONE] + 1.0;
      c[CNMF_MS_ITERS_DONE] = it;
      if (it == 1.0) c[CNMF_MS_VIOL_INIT] = violation;
      const double init = c[CNMF_MS_VIOL_INIT];
      c[CNMF_MS_VIOL_LAST] = violation;
      if (init == 0.0 || violation / init <= c[CNMF_MS_TOL]) st_agent(c + CNMF_MS_STOPPED, 1.0);
    }
  }
}

#endif  // CNMF_DIAG

// out[s] = ‖X − W_s·H_s‖² in fp64 for the R starts of a batch in ONE pass over X: per start the
// arithmetic of hals_loss_kernel (a wave per row, a lane per feature, the same chains and the same
// fixed-order sums), every start's H staged in LDS, x read once for all of them.
template <typename TX>
__global__ __launch_bounds__(NT) void ms_loss_kernel(const TX* X, const TX* W, const double* H64, double* partials,
                                                     uint32_t* counter, double* out, int64_t n_rows, int F, int k,
                                                     int R) {
  using namespace ms;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);        // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* sH = reinterpret_cast<double*>(smem + MISC);  // [R][k][F]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kF = k * F;
  for (int e = tid; e < R * kF; e += NT) sH[e] = H64[e];
  __syncthreads();
  const int64_t rpb = rows_per_block(n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  const size_t nk = (size_t)n_rows * k;
  double acc[RBMAX];
#pragma unroll
  for (int s = 0; s < RBMAX; ++s) acc[s] = 0.0;
  for (int64_t r = r0 + wave; r < r1; r += NWAVE) {
    const TX* x = X + r * F;
    const TX* w = W + r * k;
    for (int f = lane; f < F; f += 64) {
      const double xv = (double)x[f];
#pragma unroll
      for (int s = 0; s < RBMAX; ++s) {
        if (s < R) {
          double d = xv;
          for (int j = 0; j < k; ++j) d = fma(-(double)w[s * nk + j], sH[s * kF + j * F + f], d);
          acc[s] = fma(d, d, acc[s]);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < RBMAX; ++s) {
    if (s < R) {
      const double v = block_sum(acc[s], red);
      if (tid == 0) st_agent(partials + (size_t)blockIdx.x * R + s, v);
    }
  }
  if (!last_arriver(counter, flag)) return;
  if (tid >= R) return;
  double sum = 0.0;
  for (int b = 0; b < (int)gridDim.x; ++b) sum += ld_agent(partials + (size_t)b * R + tid);
  out[tid] = sum;
}

}  // namespace cnmf

using namespace cnmf;

namespace {

int ms_kp(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : 16); }

#ifdef CNMF_DIAG
size_t ms_lds(int F, int k, int xbytes, int teams, int R) {
  using namespace cnmf::ms;
  const int KP = ms_kp(k);
  const size_t pass = (size_t)R * start_doubles(F, k, KP, teams) * 8 + (size_t)teams * tile_bytes(F, xbytes);
  const size_t tail = ((size_t)row_doubles(F, k) + (size_t)k * F + KP * KP) * 8;
  return MISC + std::max(pass, tail);
}

// starts that fit one batched launch of `teams` teams (0: not even one)
int ms_fit(int F, int k, int xbytes, int teams) {
  int rb = 0;
  while (rb < cnmf::ms::RBMAX && ms_lds(F, k, xbytes, teams, rb + 1) <= kMaxLds) ++rb;
  return rb;
}

// CNMF_MS_TEAMS=1|2|4 (tools/bench_multistart.py, tests/test_gpu_multistart.py): the batched launch
// with that many teams per workgroup, where the registers of the instance allow them (4 / 2 / 1 at
// KP = 4 / 8 / 16) and LDS holds a start; else 0: the product's path.  From (F, k, X's type) alone,
// never from the number of starts, so that a start's arithmetic is the same in every batch.
int ms_teams(int F, int k, int xbytes) {
  const char* e = diag_env("CNMF_MS_TEAMS");
  const int v = e ? atoi(e) : 0, top = k <= 4 ? 4 : (k <= 8 ? 2 : 1);
  return ((v == 1 || v == 2 || v == 4) && v <= top && ms_fit(F, k, xbytes, v) >= 1) ? v : 0;
}

template <typename TX, int KP, int TEAMS>
int ms_launch_t(const ms::Args& a, hipStream_t hs) {
  const size_t lds = ms_lds(a.F, a.k, (int)sizeof(TX), TEAMS, a.R);
  if (lds > kMaxLds)
    return set_err(CNMF_ERR_UNSUPPORTED, "multistart step of %d starts needs %zu bytes of LDS", a.R, lds);
  const void* fn = reinterpret_cast<const void*>(&ms_step_kernel<TX, KP, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ms_step_kernel<TX, KP, TEAMS>), dim3((unsigned)ms::blocks(a.n_rows)), dim3(NT * TEAMS), lds, hs, a);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

template <typename TX>
int ms_launch_k(const ms::Args& a, int teams, hipStream_t hs) {
  if (a.k <= 4) {
    if (teams == 4) return ms_launch_t<TX, 4, 4>(a, hs);
    if (teams == 2) return ms_launch_t<TX, 4, 2>(a, hs);
    return ms_launch_t<TX, 4, 1>(a, hs);
  }
  if (a.k <= 8) {
    if (teams == 2) return ms_launch_t<TX, 8, 2>(a, hs);
    return ms_launch_t<TX, 8, 1>(a, hs);
  }
  return ms_launch_t<TX, 16, 1>(a, hs);
}
#endif  // CNMF_DIAG

// Starts per launch.  1 in the product library: the batched launch measured slower than as many
// cnmf_hals_step launches at every shape tried.
int ms_batch(int F, int k, int xbytes) {
#ifdef CNMF_DIAG
  if (const int t = ms_teams(F, k, xbytes)) return ms_fit(F, k, xbytes, t);
#endif
  (void)F, (void)k, (void)xbytes;
  return 1;
}

template <typename TX>
int ms_loss_t(const void* X, const void* W, const double* H64, double* partials, uint32_t* counter, double* out,
              int64_t n_rows, int F, int k, int R, hipStream_t hs) {
  const size_t lds = ms::MISC + (size_t)R * k * F * 8;
  const void* fn = reinterpret_cast<const void*>(&ms_loss_kernel<TX>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ms_loss_kernel<TX>), dim3((unsigned)ms::blocks(n_rows)), dim3(NT), lds, hs,
                     static_cast<const TX*>(X), static_cast<const TX*>(W), H64, partials, counter, out, n_rows, F, k, R);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

int ms_shape(int n_features, int k) {
  if (n_features < 1 || k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: F=%d k=%d", n_features, k);
  if (k > ms::KMAX || n_features > ms::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "multistart: k=%d (1..%d), n_features=%d (1..%d)", k, ms::KMAX, n_features,
                   ms::FMAX);
  return CNMF_OK;
}

int ms_dtype(int x_dtype) {
  if (x_dtype == CNMF_BF16) return set_err(CNMF_ERR_ARG, "multistart: bf16 X is not served (fp32 or fp64)");
  if (x_dtype != CNMF_F32 && x_dtype != CNMF_F64)
    return set_err(CNMF_ERR_ARG, "multistart: x_dtype %d (fp32 or fp64)", x_dtype);
  return CNMF_OK;
}

// the checks the launches over X share, after their null-pointer checks
int ms_check(const void* X, int x_dtype, const void* W, int64_t n_parts, int64_t n_rows, int n_features, int k,
             int n_starts) {
  if (n_rows < 1 || n_features < 1 || k < 1 || n_starts < 1)
    return set_err(CNMF_ERR_SHAPE, "invalid shape: n_rows=%lld F=%d k=%d n_starts=%d", (long long)n_rows, n_features, k,
                   n_starts);
  if (const int st = ms_shape(n_features, k)) return st;
  if (const int st = ms_dtype(x_dtype)) return st;
  const int rb = ms_batch(n_features, k, x_dtype == CNMF_F32 ? 4 : 8);
  if (n_starts > rb)
    return set_err(CNMF_ERR_UNSUPPORTED, "multistart: n_starts=%d, a launch takes %d at F=%d k=%d", n_starts, rb,
                   n_features, k);
  if (const int st = check_xw_aligned(X, W)) return st;
  if (ms::blocks(n_rows) > n_parts)
    return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the launch needs %lld", (long long)n_parts,
                   (long long)ms::blocks(n_rows));
  return CNMF_OK;
}

}  // namespace

extern "C" {

int cnmf_ms_batch(int n_features, int k, int x_dtype) {
  if (const int st = ms_shape(n_features, k)) return st;
  if (const int st = ms_dtype(x_dtype)) return st;
  return ms_batch(n_features, k, x_dtype == CNMF_F32 ? 4 : 8);
}

int64_t cnmf_ms_rows(int64_t n_rows) { return n_rows < 1 ? 0 : ms::blocks(n_rows); }

int64_t cnmf_ms_row_doubles(int n_features, int k, int n_starts) {
  if (n_starts < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: n_starts=%d", n_starts);
  if (const int st = ms_shape(n_features, k)) return st;
  if (n_starts > ms::RBMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "multistart: n_starts=%d (1..%d per launch)", n_starts, ms::RBMAX);
  return (int64_t)n_starts * ms::row_doubles(n_features, k);
}

int64_t cnmf_ms_ctl_doubles(int n_starts) {
  if (n_starts < 1) return set_err(CNMF_ERR_ARG, "n_starts < 1");
  return (int64_t)n_starts * CNMF_MS_STRIDE;
}

int cnmf_ms_step(const void* X, int x_dtype, void* W, double* H64, double* Ht, double* HHt, double* partials,
                 int64_t n_parts, uint32_t* counter, double* ctl, int64_t n_rows, int n_features, int k, int n_starts,
                 double l1_W, double l2_W, double l1_H, double l2_H, int flags, void* stream) {
  if (!X || !W || !H64 || !Ht || !HHt || !partials || !counter || !ctl)
    return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (flags & ~CNMF_MS_UPDATE_H) return set_err(CNMF_ERR_ARG, "flags %d", flags);
  if (const int st = ms_check(X, x_dtype, W, n_parts, n_rows, n_features, k, n_starts)) return st;
#ifdef CNMF_DIAG
  if (const int teams = ms_teams(n_features, k, x_dtype == CNMF_F32 ? 4 : 8)) {
    const ms::Args a{X, W, H64, Ht, HHt, partials, counter, ctl, n_rows, n_features, k, n_starts,
                     l1_W, l2_W, l1_H, l2_H, flags};
    hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    return x_dtype == CNMF_F32 ? ms_launch_k<float>(a, teams, hs) : ms_launch_k<double>(a, teams, hs);
  }
#endif
  // one start (ms_check): the iteration is cnmf_hals_step's.  The start's control words are
  // cnmf_hals_slots' (the log's LOG_CAP and NLOG stay zero within the stride), its partial rows and
  // the ticket are the step's, and so are the gate and every bit of the result.
  static_assert((int)CNMF_MS_STOPPED == (int)CNMF_HALS_STOPPED && (int)CNMF_MS_ITERS_DONE == (int)CNMF_HALS_ITERS_DONE &&
                (int)CNMF_MS_VIOL_INIT == (int)CNMF_HALS_VIOL_INIT && (int)CNMF_MS_VIOL_LAST == (int)CNMF_HALS_VIOL_LAST &&
                (int)CNMF_MS_TOL == (int)CNMF_HALS_TOL && (int)CNMF_HALS_NLOG < (int)CNMF_MS_STRIDE &&
                (int)CNMF_MS_UPDATE_H == (int)CNMF_HALS_UPDATE_H, "a start's control words are cnmf_hals_slots'");
  return cnmf_hals_step(X, x_dtype, W, H64, Ht, HHt, partials, n_parts, counter, ctl, n_rows, n_features, k, l1_W, l2_W,
                        l1_H, l2_H, flags, stream);
}

int cnmf_ms_loss(const void* X, int x_dtype, const void* W, const double* H64, double* partials, int64_t n_parts,
                 uint32_t* counter, double* out, int64_t n_rows, int n_features, int k, int n_starts, void* stream) {
  if (!X || !W || !H64 || !partials || !counter || !out) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = ms_check(X, x_dtype, W, n_parts, n_rows, n_features, k, n_starts)) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32
             ? ms_loss_t<float>(X, W, H64, partials, counter, out, n_rows, n_features, k, n_starts, hs)
             : ms_loss_t<double>(X, W, H64, partials, counter, out, n_rows, n_features, k, n_starts, hs);
}

}  // extern "C"
