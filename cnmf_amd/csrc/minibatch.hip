// minibatch.hip — online (minibatch) MU: mb_step_kernel, mb_solve_w_kernel and the cnmf_mb_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// scikit-learn 1.7.2's MiniBatchNMF (SKMB = sklearn/decomposition/_nmf.py, class MiniBatchNMF) on the
// device.  One minibatch step — SKMB _minibatch_step + _minibatch_convergence — is ONE launch over
// the batch's rows:
//   gate   every workgroup reads the control block's STOPPED word (agent-scope atomic load) and
//          returns without a write when it is set: the host can enqueue a whole epoch of steps and
//          a stop on the device turns the rest into no-ops;
//   pass   per workgroup, its rows in tiles staged in LDS: the W update (the rule of
//          cnmf_mu_sample_pass, evaluated in fp64) and one fp64 partial row
//          [W'ᵀX (k·F) | W'ᵀW' (k·k) | Σx² | Σw' | Σw'² | pad], written in full;
//   tail   the last-arriving workgroup (ticket and hand-off as reduce_kernel: agent-scope relaxed
//          atomic stores of the row, s_waitcnt vmcnt(0), barrier, one fetch_add, agent-scope atomic
//          loads by the last arriver) sums the rows in row order, takes the batch cost with the old
//          H, applies the online H-step on the running numerator / denominator, refreshes Ht / HHt
//          and evaluates both stopping rules.
// mb_solve_w_kernel is one iteration of SKMB _solve_W (H fixed) with the same gate; its tail tests
// ‖W' − W‖ / ‖W'‖ against tol.
// A workgroup is TEAMS teams of 256 threads; each team stages and processes its own tiles (the
// workgroup's tiles round-robin over the teams), so a compute unit holds 4·TEAMS waves while the
// launch still writes at most MAX_BLOCKS partial rows for the one tail workgroup to sum.
// General tile (1 <= F <= 512, 1 <= k <= 16, fp32 / fp64 X): not tuned per shape.
// ------------------------------------------------------------------------------------------------
namespace mb {
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
__host__ __device__ inline int row_doubles(int F, int k) { return (k * F + k * k + 3 + 1) & ~1; }
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
  double* Anum;
  double* Bden;
  double* partials;
  uint32_t* counter;
  double* ctl;
  int64_t n_rows;
  int F, k;
  double l1W, l2W, l1H, l2H;
  int flags;  // CNMF_MB_UPDATE_W | CNMF_MB_UPDATE_H
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

// The W update of this workgroup's rows [r0, r1), tile by tile, the tiles round-robin over the
// TEAMS teams.  SOLVE = false: accumulates the step's partial row into the caller's registers (see
// mb_step_kernel); SOLVE = true: Σ(w' − w)², Σw'².
template <typename TX, int KP, int TEAMS, bool SOLVE>
__device__ __forceinline__ void pass(const Args& a, unsigned char* smem, int64_t r0, int64_t r1,
                                     double (&acc)[2][KP], double (&bacc)[KP], double& sw, double& sx2,
                                     double& d2, double& w2) {
  using TC = TX;
  const int team = threadIdx.x / NT, t = threadIdx.x - team * NT;
  const int F = a.F, k = a.k;
  const int TR = tile_rows(F, (int)sizeof(TX));
  const int HR = TR / 2;        // update phase: a thread works on rows ur and ur + HR of the tile
  const int TPR = NT / HR;      // lanes per row pair: 8, 16 or 32
  const int FL = feat_lanes(F);
  const int RG = NT / FL;
  double* sHt = reinterpret_cast<double*>(smem + MISC);  // [F][KP]
  double* sHHt = sHt + (size_t)F * KP;                   // [KP][KP]
  double* sW = sHHt + KP * KP + team * 64 * KP;          // per team [TR][KP]: the new w, fp64
  TX* tile = reinterpret_cast<TX*>(reinterpret_cast<unsigned char*>(sHHt + KP * KP + TEAMS * 64 * KP) +
                                   (size_t)team * tile_bytes(F, (int)sizeof(TX)));  // per team [TR][F], 16-byte aligned
  const TX* X = static_cast<const TX*>(a.X);
  TC* W = static_cast<TC*>(a.W);
  const bool update_w = SOLVE || (a.flags & CNMF_MB_UPDATE_W);

  for (int e = threadIdx.x; e < F * KP; e += NT * TEAMS) sHt[e] = a.Ht[e];
  for (int e = threadIdx.x; e < KP * KP; e += NT * TEAMS) sHHt[e] = a.HHt[e];

  const int ur = t / TPR, uq = t - ur * TPR;  // update phase: row of the tile, lane of the row
  const int rg = t / FL, fl = t - rg * FL;    // accumulation phase: row group, feature lane
  const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
  for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {  // the same trip count in every team (barriers)
    const int64_t ti = i * TEAMS + team;
    const int64_t rt = r0 + ti * TR;
    const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
    __syncthreads();  // the previous tile's readers are done (and sHt / sHHt are staged)
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
    {  // W update: lane (ur, uq) sums its features of rows ur and ur + HR (one read of Hᵀ serves
       // both), the pair's lanes combine by shuffle, then each lane finishes its (row, component)s
      const bool live[2] = {ur < nr, ur + HR < nr};
      double num[2][KP], wv[2][KP];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          num[h][j] = 0.0;
          wv[h][j] = (live[h] && j < k) ? (double)W[(rt + ur + h * HR) * k + j] : 0.0;
        }
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
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          if (((h * KP + j) & (TPR - 1)) != uq || j >= k || !live[h]) continue;
          const int64_t row = rt + ur + h * HR;
          double wn = wv[h][j];
          if (update_w) {
            double den = 0.0;
#pragma unroll
            for (int m = 0; m < KP; ++m) den = fma(wv[h][m], sHHt[m * KP + j], den);  // SK:554
            if (a.l1W > 0.0) den += a.l1W;                                             // SK:616-617
            if (a.l2W > 0.0) den = den + a.l2W * wv[h][j];                             // SK:618-619
            if (den == 0.0) den = EPS32;                                               // SK:620
            wn = wv[h][j] * (num[h][j] / den);                                         // SK:622-629
            W[row * k + j] = (TC)wn;
          }
          if (SOLVE) {
            d2 = fma(wn - wv[h][j], wn - wv[h][j], d2);
            w2 = fma(wn, wn, w2);
          } else {
            sW[(ur + h * HR) * KP + j] = wn;
          }
        }
      }
    }
    if (SOLVE) continue;
    __syncthreads();
    // accumulation: thread (rg, fl) owns features fl and fl + FL for rows rg, rg + RG, ...;
    // lanes fl < k also own row fl of W'ᵀW' and Σw' of component fl
    for (int r = rg; r < nr; r += RG) {
      double wr[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) wr[j] = j < k ? sW[r * KP + j] : 0.0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int f = fl + s * FL;
        if (f >= F) continue;
        const double x = (double)tile[(size_t)r * F + f];
        sx2 = fma(x, x, sx2);
#pragma unroll
        for (int j = 0; j < KP; ++j) acc[s][j] = fma(wr[j], x, acc[s][j]);
      }
      if (fl < k) {
        double wm = 0.0;
#pragma unroll
        for (int j = 0; j < KP; ++j) wm = j == fl ? wr[j] : wm;
        sw += wm;
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

}  // namespace mb

template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void mb_step_kernel(mb::Args a) {
  using namespace mb;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_MB_STOPPED) != 0.0) return;  // the gate
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

  double acc[2][KP], bacc[KP], sw = 0.0, sx2 = 0.0, d2 = 0.0, w2 = 0.0;
#pragma unroll
  for (int j = 0; j < KP; ++j) acc[0][j] = acc[1][j] = bacc[j] = 0.0;
  pass<TX, KP, TEAMS, false>(a, smem, r0, r1, acc, bacc, sw, sx2, d2, w2);

  // the (team, row group) accumulators through LDS (over the pass's buffers), summed in order
  const int SL = kF + kk + k;  // per group: A | B | Σw' per component
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
      mine[kF + kk + fl] = sw;
    }
  }
  const double bx2 = block_sum(sx2, red);  // its barriers also publish the scratch
  double* prow = a.partials + (size_t)blockIdx.x * RL;
  for (int e = tid; e < kF + kk; e += NTB) {
    double s = 0.0;
    for (int g = 0; g < NG; ++g) s += un[(size_t)g * SL + e];
    st_agent(prow + e, s);
  }
  if (tid == 0) {
    double bsw = 0.0, bsw2 = 0.0;
    for (int j = 0; j < k; ++j)
      for (int g = 0; g < NG; ++g) {
        bsw += un[(size_t)g * SL + kF + kk + j];
        bsw2 += un[(size_t)g * SL + kF + j * k + j];
      }
    st_agent(prow + kF + kk, bx2);
    st_agent(prow + kF + kk + 1, bsw);
    st_agent(prow + kF + kk + 2, bsw2);
    for (int e = kF + kk + 3; e < RL; ++e) st_agent(prow + e, 0.0);
  }
  if (!last_arriver(a.counter, flag)) return;

  // ---- tail: the whole step's sums, the cost with the old H, the online H-step, the stop rules
  double* S = un;                 // [RL]: A | B | Σx² | Σw' | Σw'²
  double* Hn = un + RL;           // [k][F] the new H
  sum_rows(a.partials, (int)gridDim.x, RL, S);
  const bool update_h = a.flags & CNMF_MB_UPDATE_H;
  const double rho = a.ctl[CNMF_MB_RHO];
  double ah = 0.0, hs = 0.0, hs2 = 0.0;  // <A, H>, ΣH, ΣH²
  double dn = 0.0, nn = 0.0;             // ‖H_new − H_old‖², ‖H_new‖²
  for (int e = tid; e < kF; e += NTB) {
    const int j = e / F, f = e - j * F;
    const double h = a.H64[e];
    ah = fma(S[e], h, ah);
    hs += h;
    hs2 = fma(h, h, hs2);
    double hn = h;
    if (update_h) {
      const double num = S[e] * h;  // SK:712
      double den = 0.0;             // ((W'ᵀW')·H)[j][f], SK:640
      for (int m = 0; m < k; ++m) den = fma(S[kF + j * k + m], a.H64[m * F + f], den);
      if (a.l1H > 0.0) den += a.l1H;            // SK:702-703
      if (a.l2H > 0.0) den = den + a.l2H * h;   // SK:704-705
      if (den == 0.0) den = EPS32;              // SK:706
      const double An = rho * a.Anum[e] + num;  // SK:713-716
      const double Bn = rho * a.Bden[e] + den;
      hn = An / Bn;                             // SK:717
      a.Anum[e] = An;
      a.Bden[e] = Bn;
    }
    Hn[e] = hn;
    dn = fma(hn - h, hn - h, dn);
    nn = fma(hn, hn, nn);
  }
  double bh = 0.0;  // <B, HHᵀ> with the old H's HHᵀ
  for (int e = tid; e < kk; e += NTB) bh = fma(S[kF + e], a.HHt[(e / k) * KP + (e % k)], bh);
  ah = block_sum(ah, red);
  hs = block_sum(hs, red);
  hs2 = block_sum(hs2, red);
  dn = block_sum(dn, red);
  nn = block_sum(nn, red);
  bh = block_sum(bh, red);  // its barriers: every read of the old H64 / HHt is done, Hn is written
  if (update_h) {
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
  const double rows = (double)a.n_rows;
  const double cost = (0.5 * (S[kF + kk] - 2.0 * ah + bh) + a.l1W * S[kF + kk + 1] + a.l1H * hs +
                       a.l2W * S[kF + kk + 2] + a.l2H * hs2) / rows;  // SKMB _minibatch_step
  const double step = c[CNMF_MB_STEPS_DONE] + 1.0;
  const double hdiff = sqrt(dn) / sqrt(nn);
  c[CNMF_MB_STEPS_DONE] = step;
  c[CNMF_MB_LAST_COST] = cost;
  c[CNMF_MB_LAST_HDIFF] = hdiff;
  if (step >= 2.0 && update_h) {  // SKMB _minibatch_convergence
    if (c[CNMF_MB_HAVE_EWA] == 0.0) {
      c[CNMF_MB_EWA] = cost;
      c[CNMF_MB_HAVE_EWA] = 1.0;
    } else {
      double alpha = rows / (c[CNMF_MB_N_SAMPLES] + 1.0);
      alpha = alpha < 1.0 ? alpha : 1.0;
      c[CNMF_MB_EWA] = c[CNMF_MB_EWA] * (1.0 - alpha) + cost * alpha;
    }
    const double ewa = c[CNMF_MB_EWA], tol = c[CNMF_MB_TOL], mni = c[CNMF_MB_MAX_NO_IMPROVE];
    if (tol > 0.0 && hdiff <= tol) {
      c[CNMF_MB_REASON] = (double)CNMF_MB_STOP_H_CHANGE;
      st_agent(c + CNMF_MB_STOPPED, 1.0);
    } else {
      if (c[CNMF_MB_HAVE_MIN] == 0.0 || ewa < c[CNMF_MB_EWA_MIN]) {
        c[CNMF_MB_NO_IMPROVE] = 0.0;
        c[CNMF_MB_EWA_MIN] = ewa;
        c[CNMF_MB_HAVE_MIN] = 1.0;
      } else {
        c[CNMF_MB_NO_IMPROVE] += 1.0;
      }
      if (mni >= 0.0 && c[CNMF_MB_NO_IMPROVE] >= mni) {
        c[CNMF_MB_REASON] = (double)CNMF_MB_STOP_NO_IMPROVEMENT;
        st_agent(c + CNMF_MB_STOPPED, 1.0);
      }
    }
  }
  const int64_t cap = (int64_t)c[CNMF_MB_LOG_CAP], n = (int64_t)c[CNMF_MB_NLOG];
  if (n < cap) {
    double* lg = c + CNMF_MB_LOG + 3 * n;
    lg[0] = cost;
    lg[1] = hdiff;
    lg[2] = c[CNMF_MB_EWA];
    c[CNMF_MB_NLOG] = (double)(n + 1);
  }
}

template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void mb_solve_w_kernel(mb::Args a) {
  using namespace mb;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_MB_STOPPED) != 0.0) return;  // the gate
  double* red = reinterpret_cast<double*>(smem);
  int* flag = reinterpret_cast<int*>(smem + 128);
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;
  double acc[2][KP], bacc[KP], sw = 0.0, sx2 = 0.0, d2 = 0.0, w2 = 0.0;
  pass<TX, KP, TEAMS, true>(a, smem, r0, r1, acc, bacc, sw, sx2, d2, w2);
  d2 = block_sum(d2, red);
  w2 = block_sum(w2, red);
  if (threadIdx.x == 0) {
    st_agent(a.partials + (size_t)blockIdx.x * 2, d2);
    st_agent(a.partials + (size_t)blockIdx.x * 2 + 1, w2);
  }
  if (!last_arriver(a.counter, flag)) return;
  if (threadIdx.x != 0) return;
  double sd = 0.0, sn = 0.0;  // the rows in order
  for (int b = 0; b < (int)gridDim.x; ++b) {
    sd += ld_agent(a.partials + (size_t)b * 2);
    sn += ld_agent(a.partials + (size_t)b * 2 + 1);
  }
  double* c = a.ctl;
  const double wdiff = sqrt(sd) / sqrt(sn);  // SKMB _solve_W
  c[CNMF_MB_W_ITERS] += 1.0;
  c[CNMF_MB_W_DIFF] = wdiff;
  if (c[CNMF_MB_TOL] > 0.0 && wdiff <= c[CNMF_MB_TOL]) {
    c[CNMF_MB_REASON] = (double)CNMF_MB_STOP_W_CHANGE;
    st_agent(c + CNMF_MB_STOPPED, 1.0);
  }
}

}  // namespace cnmf

using namespace cnmf;

namespace {

size_t mb_lds(int F, int k, int KP, int xbytes, int teams, bool solve) {
  using namespace cnmf::mb;
  const size_t pass = ((size_t)F * KP + KP * KP + (size_t)teams * 64 * KP) * 8 + (size_t)teams * tile_bytes(F, xbytes);
  if (solve) return MISC + pass;
  const size_t scratch = (size_t)teams * (NT / feat_lanes(F)) * (k * F + k * k + k) * 8;
  const size_t tail = ((size_t)row_doubles(F, k) + (size_t)k * F) * 8;
  return MISC + std::max(pass, std::max(scratch, tail));
}

template <typename TX, int KP, int TEAMS>
int mb_launch_t(const mb::Args& a, bool solve, hipStream_t hs) {
  const size_t lds = mb_lds(a.F, a.k, KP, (int)sizeof(TX), TEAMS, solve);
  if (lds > kMaxLds) return set_err(CNMF_ERR_UNSUPPORTED, "minibatch step needs %zu bytes of LDS", lds);
  const void* fn = solve ? reinterpret_cast<const void*>(&mb_solve_w_kernel<TX, KP, TEAMS>)
                         : reinterpret_cast<const void*>(&mb_step_kernel<TX, KP, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)mb::blocks(a.n_rows)), block(NT * TEAMS);
  if (solve)
    hipLaunchKernelGGL((mb_solve_w_kernel<TX, KP, TEAMS>), grid, block, lds, hs, a);
  else
    hipLaunchKernelGGL((mb_step_kernel<TX, KP, TEAMS>), grid, block, lds, hs, a);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

// teams per workgroup: as many as the registers of the instance (KP) and the LDS allow, and no
// more than the workgroup has tiles
template <typename TX>
int mb_launch_k(const mb::Args& a, bool solve, hipStream_t hs) {
  const int KP = a.k <= 4 ? 4 : (a.k <= 8 ? 8 : 16);
  const int64_t tiles = (mb::rows_per_block(a.n_rows) + mb::tile_rows(a.F, (int)sizeof(TX)) - 1) /
                        mb::tile_rows(a.F, (int)sizeof(TX));
  auto fits = [&](int teams) {
    return tiles >= teams && mb_lds(a.F, a.k, KP, (int)sizeof(TX), teams, solve) <= kMaxLds;
  };
  if (KP == 4) {
    if (fits(4)) return mb_launch_t<TX, 4, 4>(a, solve, hs);
    if (fits(2)) return mb_launch_t<TX, 4, 2>(a, solve, hs);
    return mb_launch_t<TX, 4, 1>(a, solve, hs);
  }
  if (KP == 8) {
    if (fits(2)) return mb_launch_t<TX, 8, 2>(a, solve, hs);
    return mb_launch_t<TX, 8, 1>(a, solve, hs);
  }
  return mb_launch_t<TX, 16, 1>(a, solve, hs);
}

CNMF_LOCAL int mb_launch(const mb::Args& a, int x_dtype, bool solve, int64_t n_parts, void* stream) {
  if (a.n_rows < 1 || a.F < 1 || a.k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: n_rows=%lld F=%d k=%d", (long long)a.n_rows, a.F, a.k);
  if (a.k > mb::KMAX || a.F > mb::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "minibatch: k=%d (1..%d), n_features=%d (1..%d)", a.k, mb::KMAX, a.F, mb::FMAX);
  if (x_dtype != CNMF_F32 && x_dtype != CNMF_F64) return set_err(CNMF_ERR_ARG, "minibatch: x_dtype %d (fp32 or fp64)", x_dtype);
  if (const int st = check_xw_aligned(a.X, a.W)) return st;
  if (mb::blocks(a.n_rows) > n_parts)
    return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the launch needs %lld", (long long)n_parts, (long long)mb::blocks(a.n_rows));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? mb_launch_k<float>(a, solve, hs) : mb_launch_k<double>(a, solve, hs);
}

}  // namespace

extern "C" {

int64_t cnmf_mb_rows(int64_t n_rows) { return n_rows < 1 ? 0 : mb::blocks(n_rows); }

int64_t cnmf_mb_row_doubles(int n_features, int k) {
  if (n_features < 1 || k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: F=%d k=%d", n_features, k);
  if (k > mb::KMAX || n_features > mb::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "minibatch: k=%d (1..%d), n_features=%d (1..%d)", k, mb::KMAX, n_features, mb::FMAX);
  return mb::row_doubles(n_features, k);
}

int64_t cnmf_mb_ctl_doubles(int64_t log_cap) {
  if (log_cap < 0) return set_err(CNMF_ERR_ARG, "log_cap < 0");
  return CNMF_MB_LOG + 3 * log_cap;
}

int cnmf_mb_step(const void* X, int x_dtype, void* W, double* H64, double* Ht, double* HHt, double* Anum,
                 double* Bden, double* partials, int64_t n_parts, uint32_t* counter, double* ctl, int64_t n_rows,
                 int n_features, int k, double l1_W, double l2_W, double l1_H, double l2_H, int flags, void* stream) {
  if (!X || !W || !H64 || !Ht || !HHt || !Anum || !Bden || !partials || !counter || !ctl)
    return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (flags & ~(CNMF_MB_UPDATE_W | CNMF_MB_UPDATE_H)) return set_err(CNMF_ERR_ARG, "flags %d", flags);
  const mb::Args a{X, W, H64, Ht, HHt, Anum, Bden, partials, counter, ctl, n_rows, n_features, k,
                   l1_W, l2_W, l1_H, l2_H, flags};
  return mb_launch(a, x_dtype, false, n_parts, stream);
}

int cnmf_mb_solve_w(const void* X, int x_dtype, void* W, const double* Ht, const double* HHt, double* partials,
                    int64_t n_parts, uint32_t* counter, double* ctl, int64_t n_rows, int n_features, int k,
                    double l1_W, double l2_W, void* stream) {
  if (!X || !W || !Ht || !HHt || !partials || !counter || !ctl) return set_err(CNMF_ERR_ARG, "null pointer argument");
  const mb::Args a{X, W, nullptr, const_cast<double*>(Ht), const_cast<double*>(HHt), nullptr, nullptr, partials,
                   counter, ctl, n_rows, n_features, k, l1_W, l2_W, 0.0, 0.0, CNMF_MB_UPDATE_W};
  return mb_launch(a, x_dtype, true, n_parts, stream);
}

}  // extern "C"
