// spa.hip — init='spa': spa_step_kernel, spa_start_w_kernel and the cnmf_spa_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// The successive projection algorithm (SPA; Araújo et al. 2001, Gillis & Vavasis 2014) as a start
// for NMF: k rows of X, the "purest" spectra, chosen one per launch (tests/spa_ref.py is the spec).
// With y_i = s_i·x_i (s_i = 1/Σ_f x_if for the l1 scale, 0 for an all-zero row; 1 without a scale)
// step j picks the smallest row index p_j that attains max_i ‖r_i‖², r_i = y_i − Σ_{t<j} q_t (q_t·y_i),
// and q_j = r_{p_j}/‖r_{p_j}‖, orthogonalised once more against q_0 .. q_{j−1} (Gram-Schmidt twice).
// One step is ONE launch:
//   gate   every workgroup reads the control block's STOPPED word (agent-scope atomic load) and
//          returns without a write when it is set: the host enqueues the k steps back to back and a
//          rank stop on the device turns the rest into no-ops;
//   pass   per workgroup, its rows in tiles staged in LDS; per row, in fp64 from the fp64 Qᵀ in LDS:
//          the row sum, the j coefficients q_t·y, the residual formed explicitly and its squared
//          norm.  A row is always worked on by the same number of lanes, which take its features in
//          the same order and combine by the same shuffles, whatever its tile, team or workgroup:
//          identical rows give identical bits, so the smallest-index rule is exact;
//   part   [best score | its row | Σ of the workgroup's entries | pad], written in full with
//          agent-scope atomic stores; the ticket and hand-off are hals_step_kernel's, duplicated
//          (s_waitcnt vmcnt(0), barrier, one fetch_add, agent-scope atomic loads by the last arriver);
//   tail   the last-arriving workgroup takes the best of the partials in workgroup (= row) order,
//          the lower row on a tie, re-reads row p_j from X, computes q_j and writes Q[j], IDX[j],
//          RHO[j] = ‖r_{p_j}‖ / max_i ‖y_i‖ and STEPS_DONE; step 0 also writes SUM_X and YMAX.  When
//          RHO[j] <= RANK_TOL the rank of X is exhausted: STOPPED is set and nothing else written.
// Nothing in the launch waits for another workgroup.  Every sum has a fixed order, so the same
// inputs give the same bits.  General tile (1 <= F <= 512, 1 <= k <= 16, fp32 / fp64 X).
// ------------------------------------------------------------------------------------------------
namespace spa {
constexpr int MAX_BLOCKS = 256;   // partial rows of a launch, at most (one tail workgroup scans them)
constexpr int ROW_ALIGN = 64;     // rows per workgroup: a multiple (tiles then start 16-byte aligned)
constexpr int TILE_BYTES = 64 * 1024;
constexpr int MISC = 512;         // bytes at the start of LDS: red[16], flag, bs[16], bi[16], top[4]
constexpr int FMAX = 512, KMAX = 16;
constexpr int ROW_DOUBLES = 4;    // [best score | its row | Σ entries | pad]

__host__ __device__ inline int64_t rows_per_block(int64_t n_rows) {
  int64_t rpb = (n_rows + MAX_BLOCKS - 1) / MAX_BLOCKS;
  return (rpb + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
}
__host__ __device__ inline int64_t blocks(int64_t n_rows) {
  const int64_t rpb = rows_per_block(n_rows);
  return (n_rows + rpb - 1) / rpb;
}
// rows of a staged tile: 64, 32 or 16 so that the tile (in X's type) fits TILE_BYTES
__host__ __device__ inline int tile_rows(int F, int xbytes) {
  int tr = 64;
  while (tr > 16 && tr * F * xbytes > TILE_BYTES) tr >>= 1;
  return tr;
}
__host__ __device__ inline int tile_bytes(int F, int xbytes) { return (tile_rows(F, xbytes) * F * xbytes + 15) & ~15; }

struct Args {
  const void* X;
  double* Q;         // [k][F]: rows 0 .. j-1 read, row j written by the tail
  double* partials;
  uint32_t* counter;
  double* ctl;
  double* scores;    // optional [n_rows]: every row's score of this step (tests), else null
  int64_t n_rows;
  int F, k, j;
  int l1;            // the l1 row scale
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

// nr rows of F entries from src (16-byte aligned) into the team's tile: whole chunks, then the tail
template <typename TX>
__device__ __forceinline__ void stage_tile(TX* tile, const TX* src, int nr, int F, int t) {
  const int64_t n_el = (int64_t)nr * F;
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

// the sum over the TPR lanes of a row (adjacent lanes of one wave); every lane gets the same bits
__device__ __forceinline__ double row_sum(double v, int TPR) {
  for (int off = TPR >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the better of two (score, row) pairs: the higher score, on a tie the lower row
__device__ __forceinline__ void take_better(double& s, double& i, double s2, double i2) {
  if (s2 > s || (s2 == s && i2 < i)) {
    s = s2;
    i = i2;
  }
}

}  // namespace spa

template <typename TX, int JP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void spa_step_kernel(spa::Args a) {
  using namespace spa;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (ld_agent(a.ctl + CNMF_SPA_STOPPED) != 0.0) return;  // the gate
  constexpr int NTB = NT * TEAMS;
  double* red = reinterpret_cast<double*>(smem);         // [16]
  int* flag = reinterpret_cast<int*>(smem + 128);
  double* bs = reinterpret_cast<double*>(smem + 192);    // [16] per wave: best score
  double* bi = reinterpret_cast<double*>(smem + 320);    // [16] per wave: its row
  double* top = reinterpret_cast<double*>(smem + 448);   // [4] the tail's scan
  double* un = reinterpret_cast<double*>(smem + MISC);   // the union region
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int F = a.F, j = a.j;
  const int64_t rpb = rows_per_block(a.n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < a.n_rows ? r0 + rpb : a.n_rows;
  const TX* X = static_cast<const TX*>(a.X);

  // ---- pass: the scores of this workgroup's rows [r0, r1), the tiles round-robin over the teams
  double best = -1.0, besti = 0.0, esum = 0.0;
  {
    const int TR = tile_rows(F, (int)sizeof(TX));
    const int TPR = NT / TR;  // lanes per row: 4, 8 or 16
    double* sQt = un;         // [F][JP]: Qᵀ, zero beyond j
    TX* tile = reinterpret_cast<TX*>(reinterpret_cast<unsigned char*>(sQt + (size_t)F * JP) +
                                     (size_t)team * tile_bytes(F, (int)sizeof(TX)));  // per team [TR][F]
    for (int e = tid; e < F * JP; e += NTB) {
      const int f = e / JP, q = e - f * JP;
      sQt[e] = q < j ? a.Q[(size_t)q * F + f] : 0.0;
    }
    const int ur = t / TPR, uq = t - ur * TPR;  // row of the tile, lane of the row
    const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
    for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {  // the same trip count in every team (barriers)
      const int64_t ti = i * TEAMS + team;
      const int64_t rt = r0 + ti * TR;
      const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
      __syncthreads();  // the previous tile's readers are done (and sQt is staged)
      stage_tile<TX>(tile, X + rt * F, nr, F, t);
      __syncthreads();
      const bool live = ur < nr;
      const TX* x = tile + (size_t)(live ? ur : 0) * F;
      double sum = 0.0;
      for (int f = uq; f < F; f += TPR) sum += (double)x[f];
      sum = row_sum(sum, TPR);
      const double s = a.l1 ? (sum > 0.0 ? 1.0 / sum : 0.0) : 1.0;
      double c[JP];
#pragma unroll
      for (int q = 0; q < JP; ++q) c[q] = 0.0;
      for (int f = uq; f < F; f += TPR) {
        const double y = s * (double)x[f];
        const double* h = sQt + (size_t)f * JP;
#pragma unroll
        for (int q = 0; q < JP; ++q) c[q] = fma(y, h[q], c[q]);
      }
#pragma unroll
      for (int q = 0; q < JP; ++q) c[q] = row_sum(c[q], TPR);
      double sc = 0.0;
      for (int f = uq; f < F; f += TPR) {
        double r = s * (double)x[f];
        const double* h = sQt + (size_t)f * JP;
#pragma unroll
        for (int q = 0; q < JP; ++q) r = fma(-c[q], h[q], r);
        sc = fma(r, r, sc);
      }
      sc = row_sum(sc, TPR);
      if (live && uq == 0) {  // a thread's rows ascend: the strict test keeps the lowest
        const int64_t row = rt + ur;
        if (a.scores) a.scores[row] = sc;
        if (sc > best) {
          best = sc;
          besti = (double)row;
        }
        esum += sum;
      }
    }
  }

  // ---- the workgroup's partial row
  esum = block_sum(esum, red);
  for (int off = 32; off > 0; off >>= 1) take_better(best, besti, __shfl_xor(best, off), __shfl_xor(besti, off));
  if ((tid & 63) == 0) {
    bs[tid >> 6] = best;
    bi[tid >> 6] = besti;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NTB / 64; ++w) take_better(best, besti, bs[w], bi[w]);
    double* prow = a.partials + (size_t)blockIdx.x * ROW_DOUBLES;
    st_agent(prow + 0, best);
    st_agent(prow + 1, besti);
    st_agent(prow + 2, esum);
    st_agent(prow + 3, 0.0);
  }
  if (!last_arriver(a.counter, flag)) return;

  // ---- tail: the pick, its direction, the control block
  const int G = (int)gridDim.x;
  double* P = un;                              // [G][ROW_DOUBLES]
  double* y = un + MAX_BLOCKS * ROW_DOUBLES;   // [F]
  double* cc = y + FMAX;                       // [KMAX]
  for (int e = tid; e < G * ROW_DOUBLES; e += NTB) P[e] = ld_agent(a.partials + e);
  __syncthreads();
  if (tid == 0) {  // in workgroup order, which is row order: the strict test keeps the lower row
    double b = -1.0, brow = 0.0, sx = 0.0;
    for (int g = 0; g < G; ++g) {
      if (P[g * ROW_DOUBLES] > b) {
        b = P[g * ROW_DOUBLES];
        brow = P[g * ROW_DOUBLES + 1];
      }
      sx += P[g * ROW_DOUBLES + 2];
    }
    top[0] = b;
    top[1] = brow;
    top[2] = sx;
  }
  __syncthreads();
  const double nr = sqrt(top[0]);
  const int64_t p = (int64_t)top[1];
  const double ymax = j == 0 ? nr : a.ctl[CNMF_SPA_YMAX];
  if (j == 0 && tid == 0) {
    a.ctl[CNMF_SPA_SUM_X] = top[2];
    a.ctl[CNMF_SPA_YMAX] = ymax;
  }
  if (!(nr > a.ctl[CNMF_SPA_RANK_TOL] * ymax)) {  // the rank of X is exhausted (or X is zero)
    if (tid == 0) st_agent(a.ctl + CNMF_SPA_STOPPED, 1.0);
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  double v = 0.0;
  for (int f = tid; f < F; f += NTB) {
    y[f] = (double)X[p * F + f];
    v += y[f];
  }
  v = block_sum(v, red);
  const double s = a.l1 ? (v > 0.0 ? 1.0 / v : 0.0) : 1.0;
  double n2 = 0.0;
  for (int pass = 0; pass < 2; ++pass) {  // the residual of y, then of q once more; normalised
    for (int q = wave; q < j; q += NTB / 64) {
      double d = 0.0;
      for (int f = lane; f < F; f += 64) d = fma(a.Q[(size_t)q * F + f], pass ? y[f] : s * y[f], d);
      d = wave_sum(d);
      if (lane == 0) cc[q] = d;
    }
    __syncthreads();
    v = 0.0;
    for (int f = tid; f < F; f += NTB) {  // a feature belongs to one thread in every loop over f
      double r = pass ? y[f] : s * y[f];
      for (int q = 0; q < j; ++q) r = fma(-cc[q], a.Q[(size_t)q * F + f], r);
      y[f] = r;
      v = fma(r, r, v);
    }
    n2 = block_sum(v, red);  // its barriers: cc is read, y is written
    const double inv = 1.0 / sqrt(n2);
    for (int f = tid; f < F; f += NTB) y[f] *= inv;
    __syncthreads();
  }
  for (int f = tid; f < F; f += NTB) a.Q[(size_t)j * F + f] = y[f];
  if (tid != 0) return;
  a.ctl[CNMF_SPA_IDX + j] = (double)p;
  a.ctl[CNMF_SPA_RHO + j] = nr / ymax;
  a.ctl[CNMF_SPA_STEPS_DONE] = (double)(j + 1);
  if (j == a.k - 1) st_agent(a.ctl + CNMF_SPA_STOPPED, 1.0);
}

// W0 = max(X·M, floor) in one pass: M (F x k fp64, row-major) staged in LDS as [F][KP], the products
// in fp64 by the lanes of a row as in the step, rounded once to W's type.
template <typename TX, int KP, int TEAMS>
__global__ __launch_bounds__(NT * TEAMS) void spa_start_w_kernel(const TX* X, const double* M, void* W, int w64,
                                                                 double floor_, int64_t n_rows, int F, int k) {
  using namespace spa;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NTB = NT * TEAMS;
  const int tid = threadIdx.x;
  const int team = tid / NT, t = tid - team * NT;
  const int64_t rpb = rows_per_block(n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  const int TR = tile_rows(F, (int)sizeof(TX));
  const int TPR = NT / TR;
  double* sM = reinterpret_cast<double*>(smem + MISC);  // [F][KP], zero beyond k
  TX* tile = reinterpret_cast<TX*>(reinterpret_cast<unsigned char*>(sM + (size_t)F * KP) +
                                   (size_t)team * tile_bytes(F, (int)sizeof(TX)));
  for (int e = tid; e < F * KP; e += NTB) {
    const int f = e / KP, q = e - f * KP;
    sM[e] = q < k ? M[(size_t)f * k + q] : 0.0;
  }
  const int ur = t / TPR, uq = t - ur * TPR;
  const int64_t n_tiles = (r1 - r0 + TR - 1) / TR;
  for (int64_t i = 0; i * TEAMS < n_tiles; ++i) {
    const int64_t ti = i * TEAMS + team;
    const int64_t rt = r0 + ti * TR;
    const int nr = ti < n_tiles ? (int)(r1 - rt < TR ? r1 - rt : TR) : 0;
    __syncthreads();
    stage_tile<TX>(tile, X + rt * F, nr, F, t);
    __syncthreads();
    const bool live = ur < nr;
    const TX* x = tile + (size_t)(live ? ur : 0) * F;
    double c[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) c[q] = 0.0;
    for (int f = uq; f < F; f += TPR) {
      const double xv = (double)x[f];
      const double* h = sM + (size_t)f * KP;
#pragma unroll
      for (int q = 0; q < KP; ++q) c[q] = fma(xv, h[q], c[q]);
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) c[q] = row_sum(c[q], TPR);
    if (live && uq == 0) {
      const int64_t row = rt + ur;
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        if (q < k) {
          const double w = fmax(c[q], floor_);
          if (w64) static_cast<double*>(W)[row * k + q] = w;
          else static_cast<float*>(W)[row * k + q] = (float)w;
        }
      }
    }
  }
}

}  // namespace cnmf

using namespace cnmf;

namespace {

size_t spa_step_lds(int F, int JP, int xbytes, int teams) {
  using namespace cnmf::spa;
  const size_t pass = (size_t)F * JP * 8 + (size_t)teams * tile_bytes(F, xbytes);
  const size_t tail = ((size_t)MAX_BLOCKS * ROW_DOUBLES + FMAX + KMAX) * 8;
  return MISC + std::max(pass, tail);
}

size_t spa_w_lds(int F, int KP, int xbytes, int teams) {
  return spa::MISC + (size_t)F * KP * 8 + (size_t)teams * spa::tile_bytes(F, xbytes);
}

// teams per workgroup: as many as the LDS allows, and no more than the workgroup has tiles
int spa_teams(int64_t n_rows, int F, int P, int xbytes, bool step) {
  const int64_t tiles = (spa::rows_per_block(n_rows) + spa::tile_rows(F, xbytes) - 1) / spa::tile_rows(F, xbytes);
  for (int teams = 4; teams > 1; teams >>= 1) {
    const size_t lds = step ? spa_step_lds(F, P, xbytes, teams) : spa_w_lds(F, P, xbytes, teams);
    if (tiles >= teams && lds <= kMaxLds) return teams;
  }
  return 1;
}

template <typename TX, int JP, int TEAMS>
int spa_step_launch_t(const spa::Args& a, hipStream_t hs) {
  const size_t lds = spa_step_lds(a.F, JP, (int)sizeof(TX), TEAMS);
  if (lds > kMaxLds) return set_err(CNMF_ERR_UNSUPPORTED, "spa step needs %zu bytes of LDS", lds);
  const void* fn = reinterpret_cast<const void*>(&spa_step_kernel<TX, JP, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)spa::blocks(a.n_rows)), block(NT * TEAMS);
  hipLaunchKernelGGL((spa_step_kernel<TX, JP, TEAMS>), grid, block, lds, hs, a);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

template <typename TX, int JP>
int spa_step_launch_j(const spa::Args& a, hipStream_t hs) {
  switch (spa_teams(a.n_rows, a.F, JP, (int)sizeof(TX), true)) {
    case 4: return spa_step_launch_t<TX, JP, 4>(a, hs);
    case 2: return spa_step_launch_t<TX, JP, 2>(a, hs);
    default: return spa_step_launch_t<TX, JP, 1>(a, hs);
  }
}

template <typename TX>
int spa_step_launch(const spa::Args& a, hipStream_t hs) {
  if (a.j <= 4) return spa_step_launch_j<TX, 4>(a, hs);
  if (a.j <= 8) return spa_step_launch_j<TX, 8>(a, hs);
  return spa_step_launch_j<TX, 16>(a, hs);
}

template <typename TX, int KP, int TEAMS>
int spa_w_launch_t(const void* X, const double* M, void* W, int w64, double floor_, int64_t n_rows, int F, int k,
                   hipStream_t hs) {
  const size_t lds = spa_w_lds(F, KP, (int)sizeof(TX), TEAMS);
  if (lds > kMaxLds) return set_err(CNMF_ERR_UNSUPPORTED, "spa start needs %zu bytes of LDS", lds);
  const void* fn = reinterpret_cast<const void*>(&spa_start_w_kernel<TX, KP, TEAMS>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((spa_start_w_kernel<TX, KP, TEAMS>), dim3((unsigned)spa::blocks(n_rows)), dim3(NT * TEAMS), lds,
                     hs, static_cast<const TX*>(X), M, W, w64, floor_, n_rows, F, k);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

template <typename TX, int KP>
int spa_w_launch_k(const void* X, const double* M, void* W, int w64, double floor_, int64_t n_rows, int F, int k,
                   hipStream_t hs) {
  switch (spa_teams(n_rows, F, KP, (int)sizeof(TX), false)) {
    case 4: return spa_w_launch_t<TX, KP, 4>(X, M, W, w64, floor_, n_rows, F, k, hs);
    case 2: return spa_w_launch_t<TX, KP, 2>(X, M, W, w64, floor_, n_rows, F, k, hs);
    default: return spa_w_launch_t<TX, KP, 1>(X, M, W, w64, floor_, n_rows, F, k, hs);
  }
}

template <typename TX>
int spa_w_launch(const void* X, const double* M, void* W, int w64, double floor_, int64_t n_rows, int F, int k,
                 hipStream_t hs) {
  if (k <= 4) return spa_w_launch_k<TX, 4>(X, M, W, w64, floor_, n_rows, F, k, hs);
  if (k <= 8) return spa_w_launch_k<TX, 8>(X, M, W, w64, floor_, n_rows, F, k, hs);
  return spa_w_launch_k<TX, 16>(X, M, W, w64, floor_, n_rows, F, k, hs);
}

// the checks the two launches share, after their null-pointer checks
int spa_check(const void* X, int x_dtype, const void* W, int64_t n_rows, int n_features, int k) {
  if (n_rows < 1 || n_features < 1 || k < 1)
    return set_err(CNMF_ERR_SHAPE, "invalid shape: n_rows=%lld F=%d k=%d", (long long)n_rows, n_features, k);
  if (k > spa::KMAX || n_features > spa::FMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "spa: k=%d (1..%d), n_features=%d (1..%d)", k, spa::KMAX, n_features, spa::FMAX);
  if (x_dtype == CNMF_BF16) return set_err(CNMF_ERR_ARG, "spa: bf16 X is not served (fp32 or fp64)");
  if (x_dtype != CNMF_F32 && x_dtype != CNMF_F64) return set_err(CNMF_ERR_ARG, "spa: x_dtype %d (fp32 or fp64)", x_dtype);
  return check_xw_aligned(X, W);
}

}  // namespace

extern "C" {

int64_t cnmf_spa_rows(int64_t n_rows) { return n_rows < 1 ? 0 : spa::blocks(n_rows); }

int64_t cnmf_spa_row_doubles(void) { return spa::ROW_DOUBLES; }

int64_t cnmf_spa_ctl_doubles(int k) {
  if (k < 1) return set_err(CNMF_ERR_SHAPE, "invalid shape: k=%d", k);
  if (k > spa::KMAX) return set_err(CNMF_ERR_UNSUPPORTED, "spa: k=%d (1..%d)", k, spa::KMAX);
  return CNMF_SPA_RHO + k;
}

int cnmf_spa_step(const void* X, int x_dtype, double* Q, double* partials, int64_t n_parts, uint32_t* counter,
                  double* ctl, double* scores, int64_t n_rows, int n_features, int k, int j, int normalise,
                  void* stream) {
  if (!X || !Q || !partials || !counter || !ctl) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = spa_check(X, x_dtype, nullptr, n_rows, n_features, k)) return st;
  if (j < 0 || j >= k) return set_err(CNMF_ERR_ARG, "step j=%d (0..%d)", j, k - 1);
  if (normalise != CNMF_SPA_NORM_NONE && normalise != CNMF_SPA_NORM_L1) return set_err(CNMF_ERR_ARG, "normalise %d", normalise);
  if (spa::blocks(n_rows) > n_parts)
    return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the launch needs %lld", (long long)n_parts, (long long)spa::blocks(n_rows));
  const spa::Args a{X, Q, partials, counter, ctl, scores, n_rows, n_features, k, j, normalise == CNMF_SPA_NORM_L1};
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  return x_dtype == CNMF_F32 ? spa_step_launch<float>(a, hs) : spa_step_launch<double>(a, hs);
}

int cnmf_spa_start_w(const void* X, int x_dtype, const double* M, double floor, void* W, int w_dtype, int64_t n_rows,
                     int n_features, int k, void* stream) {
  if (!X || !M || !W) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (const int st = spa_check(X, x_dtype, W, n_rows, n_features, k)) return st;
  if (w_dtype != CNMF_F32 && w_dtype != CNMF_F64) return set_err(CNMF_ERR_ARG, "spa: w_dtype %d (fp32 or fp64)", w_dtype);
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const int w64 = w_dtype == CNMF_F64;
  return x_dtype == CNMF_F32 ? spa_w_launch<float>(X, M, W, w64, floor, n_rows, n_features, k, hs)
                             : spa_w_launch<double>(X, M, W, w64, floor, n_rows, n_features, k, hs);
}

}  // extern "C"
