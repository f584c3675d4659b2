// persist.hpp — what the persistent (multi-iteration) launches share: the counter map, the launch
// arguments, the tolerance and exchange control blocks, the write-through load / store helpers and
// the in-launch reduction and exchange.
#pragma once

#include "common.hpp"

namespace cnmf {

namespace sl {
constexpr int GROUP = 16;                               // workgroups per first-level group
constexpr int MAX_GROUPS = 64;
constexpr uint32_t XPOISON = 0xFFFFFFFFu;                // exchange flag of a failed rank
constexpr uint64_t SPIN_TIMEOUT = 200000000ull;         // 2 s of s_memrealtime (100 MHz)
}  // namespace sl

// counter words (uint32): [0] reduce_kernel's ticket; the persistent kernel's at 128-byte strides
static_assert(sl::MAX_GROUPS <= NSLICE, "group rows live in the reduction stage buffer");
constexpr int CNT_GROUP0 = 32;
constexpr int CNT_TOP = CNT_GROUP0 + 32 * sl::MAX_GROUPS;
constexpr int CNT_FLAG = CNT_TOP + 32;
constexpr int CNT_ERR = CNT_FLAG + 32;
constexpr int DYN_GRP = 8;                       // workgroups per floating-tile pool
constexpr int DYN_MAX_POOLS = sl::GROUP * sl::MAX_GROUPS / DYN_GRP;
constexpr int CNT_POOL = CNT_ERR + 32;           // floating-tile pools [parity][pool] (32-word stride)
constexpr int CNT_RCOL0 = CNT_POOL + 2 * DYN_MAX_POOLS * 32;          // reduce_kernel: one ticket per 64-column block
constexpr int CNT_UPD = CNT_POOL;  // basis_update_split_kernel's ticket (the pools serve layout 3 only)
// the wave-tile kernels' XCC table (round 6): word b = 1 + the XCC id workgroup b runs on (written at
// the launch's start, zeroed by the launch's last combiner), in the pools' words past CNT_UPD's line
constexpr int CNT_XCC0 = CNT_POOL + 32;
constexpr int RED_MAX_COLS = 512;
constexpr int CNT_WORDS = CNT_RCOL0 + RED_MAX_COLS;
static_assert(CNT_XCC0 + sl::GROUP * sl::MAX_GROUPS <= CNT_RCOL0, "the XCC table fits the pools' words");

struct PersistArgs {
  const float* X;
  float* W;
  double* H64;       // in: the basis; out: the final basis
  double* Ht;        // out [F][4]
  double* HHt;       // out [4][4]
  double* partials;  // [G][K*V] per-workgroup rows
  double* groups;    // [NG][K*V] group rows
  double* AB;        // [K*V]: in (apply_first) / out (the last iteration's reduced accumulators)
  uint32_t* cnt;     // CNT_WORDS counters
  int64_t n_tiles;
  int n_iter;
  int n_groups;
  int n_static;      // DYN: tiles per workgroup with W resident; tiles n_static*G.. float (the pool)
  double l1W, l2W, l1H, l2H;
  int apply_first;   // first apply the pending basis update from AB (multi-GPU: AB all-reduced)
  int apply_last;    // apply the last iteration's basis update in-launch (single GPU)
  // MULTI (one persistent launch per rank, the all-reduce in-launch): the exchange control block
  // (XC_* words, device memory), read only inside the exchange so that its values do not occupy
  // SGPRs through the streaming loop
  uint64_t* xctl;
  // TOL (the tolerance test on the device, SK:872-884): the control block of TC_* doubles
  double* tolctl;
  // the wave-tile kernel's first reduction level through the XCD's L2 (round 6):
  // a group's members (b ≡ g mod NG: one XCD under round-robin placement) store their partial rows
  // with plain stores, kept in the L2 their combiner reads with sc1 loads — from the second iteration
  // on, and only when the XCC table shows every member of the group on the combiner's XCC (placement
  // is never assumed: a group spread over XCDs keeps the write-through stores)
  int l2rows = 0;
  // mu_iter_wt_kernel: sixteenths of X loaded with the default cache policy, so that they stay in the
  // Infinity Cache from one iteration to the next; the rest streams through `nt` (0 = every load `nt`;
  // csrc/keep.hpp chooses it)
  int x_keep16 = 0;
};

// the arguments of a persistent launch of G workgroups (n_static = 0, l2rows = 0: the callers' own)
CNMF_LOCAL inline PersistArgs persist_args(const void* X, void* W, double* H64, double* Ht, double* HHt, double* partials,
                                double* stage, uint32_t* counter, double* AB, int64_t n_tiles, int n_iter,
                                int64_t G, double l1_W, double l2_W, double l1_H, double l2_H, int apply_first,
                                int apply_last, uint64_t* xctl, double* tolctl) {
  PersistArgs pa;
  pa.X = static_cast<const float*>(X);
  pa.W = static_cast<float*>(W);
  pa.H64 = H64;
  pa.Ht = Ht;
  pa.HHt = HHt;
  pa.partials = partials;
  pa.groups = stage;
  pa.AB = AB;
  pa.cnt = counter;
  pa.n_tiles = n_tiles;
  pa.n_iter = n_iter;
  pa.n_groups = (int)((G + sl::GROUP - 1) / sl::GROUP);
  pa.n_static = 0;
  pa.l1W = l1_W;
  pa.l2W = l2_W;
  pa.l1H = l1_H;
  pa.l2H = l2_H;
  pa.apply_first = apply_first;
  pa.apply_last = apply_last;
  pa.xctl = xctl;
  pa.tolctl = tolctl;
  return pa;
}

// tolerance control block (doubles; TC_WSNAP holds a pointer's bits): inputs tol, it0 (global index
// of the launch's first iteration), the capacity of the error list; in/out the error at init and the
// previous checked error; outputs the iterations done, whether the test stopped the fit, whether
// the stopped fit's W is in the snapshot buffer (streamed W) rather than in W itself, the count and
// list of the checked errors (index g / 10 for the state after g iterations)
constexpr int TC_TOL = 0, TC_IT0 = 1, TC_INIT = 2, TC_PREV = 3, TC_DONE = 4, TC_STOPPED = 5, TC_IN_SNAP = 6,
              TC_WSNAP = 7, TC_CAP = 8, TC_NERR = 9, TC_ERRS = 16;
static_assert(TC_TOL == CNMF_TC_TOL && TC_IT0 == CNMF_TC_IT0 && TC_INIT == CNMF_TC_INIT && TC_PREV == CNMF_TC_PREV &&
                  TC_DONE == CNMF_TC_DONE && TC_STOPPED == CNMF_TC_STOPPED && TC_IN_SNAP == CNMF_TC_IN_SNAP &&
                  TC_WSNAP == CNMF_TC_WSNAP && TC_CAP == CNMF_TC_CAP && TC_NERR == CNMF_TC_NERR && TC_ERRS == CNMF_TC_ERRS,
              "tolerance control block slots = include/cnmf_hip.h");
constexpr uint32_t FLAG_STOP = 1u << 30;  // the iteration flag of a launch the tolerance test stopped

// exchange control block words: rank, world, byte offset of the flags in an exchange buffer, the
// generation base (advanced by n_iter at the end of every launch, on the device), then the
// world exchange-buffer pointers (this rank's own at XC_PEERS + rank)
constexpr int XC_RANK = 0, XC_WORLD = 1, XC_FLAG_OFF = 2, XC_GEN = 3, XC_PEERS = 8;

__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// two doubles as one 16-byte sc1 store (p 16-byte aligned; the MI355X guide's table: a 16-B sc1
// store costs about a plain one, 8-B accesses 0.54-0.70x the rate)
__device__ __forceinline__ void st16_sc1(double* p, double v0, double v1) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  const d2v v = d2v{v0, v1};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// n / d for the W-updates of the wave-tile kernels: v_rcp_f64 + one Newton step (relative error
// ~2^-50, far below the fp32 rounding of the new w that follows) in place of the fp64 division's
// ~10-instruction IEEE sequence (round 5; d is a denominator >= EPS32, never denormal)
__device__ __forceinline__ double div_nr(double n, double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  return n * r;
}

#ifdef CNMF_STAMPS
// diagnostic timeline of the persistent kernel (s_memrealtime, 100 MHz): per iteration and
// workgroup [0] = rows published (arrival), [1] = next iteration's basis ready (resume); per
// iteration the top combiner's AB publish time.  Never in the product build.
constexpr int TL_IT = 64, TL_WG = 2048;
__device__ unsigned long long g_tl[TL_IT * TL_WG * 2];
__device__ unsigned long long g_tl_pub[TL_IT];
__device__ unsigned long long g_tl_x[TL_IT * 4];  // MULTI exchange: start, stored, flags seen, summed
__device__ unsigned long long g_tl_start[TL_WG];
__device__ unsigned int g_tl_hw[TL_WG * 2];  // HW_REG_HW_ID (cu / sh / se bits), HW_REG_XCC_ID
#define TL(it_, slot_)                                                                          \
  do {                                                                                          \
    if (t == 0 && (it_) < TL_IT && b < TL_WG) g_tl[((it_) * TL_WG + b) * 2 + (slot_)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define TL_PUB(it_) do { if (t == 0 && (it_) < TL_IT) g_tl_pub[it_] = __builtin_amdgcn_s_memrealtime(); } while (0)
// per-level stamps of the reduction tree (round 6): [it][g][0] group g's combiner's ticket returned,
// [1] its group row stored (vmcnt(0) + barrier); [it][TL_LVG][0] the top's ticket returned, [1] AB summed
// and stored; and [it][wg] each workgroup's time before its partial-row stores (g_tl_pre)
constexpr int TL_LVG = 64;
__device__ unsigned long long g_tl_lv[TL_IT * (TL_LVG + 1) * 2];
__device__ unsigned long long g_tl_pre[TL_IT * TL_WG];
__device__ unsigned long long g_tl_seen[TL_IT * TL_WG];  // flag seen (non-top workgroups)
__device__ unsigned long long g_tl_ab[TL_IT * TL_WG];    // AB in LDS (non-top workgroups)
__device__ unsigned long long g_tl_upd[TL_IT * TL_WG];   // basis update done (before load_basis)
#define TL_LV(it_, g_, slot_)                                                                   \
  do {                                                                                          \
    if (t == 0 && (it_) < TL_IT) g_tl_lv[((it_) * (TL_LVG + 1) + (g_)) * 2 + (slot_)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define TL_PRE(it_) do { if (t == 0 && (it_) < TL_IT && b < TL_WG) g_tl_pre[(it_) * TL_WG + b] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_SEEN(it_) do { if (t == 0 && (it_) < TL_IT && b < TL_WG) g_tl_seen[(it_) * TL_WG + b] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_AB(it_) do { if (t == 0 && (it_) < TL_IT && b < TL_WG) g_tl_ab[(it_) * TL_WG + b] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_UPD(it_) do { if (t == 0 && (it_) < TL_IT && b < TL_WG) g_tl_upd[(it_) * TL_WG + b] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_X(it_, slot_) do { if (t == 0 && (it_) < TL_IT) g_tl_x[(it_) * 4 + (slot_)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_START                                                                               \
  do {                                                                                         \
    if (t == 0 && b < TL_WG) {                                                                 \
      g_tl_start[b] = __builtin_amdgcn_s_memrealtime();                                        \
      unsigned hw_, xcc_;                                                                      \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                        \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                      \
      g_tl_hw[2 * b] = hw_;                                                                    \
      g_tl_hw[2 * b + 1] = xcc_;                                                               \
    }                                                                                          \
  } while (0)
#else
#define TL(it_, slot_) do {} while (0)
#define TL_PUB(it_) do {} while (0)
#define TL_X(it_, slot_) do {} while (0)
#define TL_START do {} while (0)
#define TL_LV(it_, g_, slot_) do {} while (0)
#define TL_PRE(it_) do {} while (0)
#define TL_SEEN(it_) do {} while (0)
#define TL_AB(it_) do {} while (0)
#define TL_UPD(it_) do {} while (0)
#endif

// sum of `cnt` rows (m0, m0 + step, ...) of NOUT doubles each, in row order, sc1 loads (the NOUT-
// generic form of sum_rows_sc1: up to three outputs per thread, their row batches in flight together)
template <int NOUT>
__device__ __forceinline__ void sum_rows_n(const double* rows, int m0, int step, int cnt, double* lds_out,
                                           double* g_out, int t) {
  constexpr int U = (NOUT + NT - 1) / NT;
  constexpr int RB = U == 1 ? 16 : (U == 2 ? 16 : 8);
  int o[U];
  double v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    o[u] = t + NT * u < NOUT ? t + NT * u : t;
    v[u] = 0.0;
  }
  for (int m = 0; m < cnt; m += RB) {
    double x[RB][U];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int row = m0 + min(m + r, cnt - 1) * step;
#pragma unroll
      for (int u = 0; u < U; ++u) x[r][u] = ld_sc1(rows + (size_t)row * NOUT + o[u]);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] += m + r < cnt ? x[r][u] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (t + NT * u < NOUT) {
      if (lds_out) lds_out[o[u]] = v[u];
      st_sc1(g_out + o[u], v[u]);
    }
}

// 16-byte agent-scope (sc1) loads and stores: the valid-forms table's first row allows 16-B sc1
// stores and loads on both sides of a hand-off (MI355X_MICROARCH.md); one instruction per two doubles
// where sum_rows_n moved 8 bytes per lane (round 6: the guide's 8-B accesses run at 0.54-0.70x the
// 16-B rate, and the tail's combines were latency-bound on those loads, profiles/r06/tree/)
__device__ __forceinline__ void ld16_sc1(u32x4& r, const double* p) {
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r) : "v"(p) : "memory");
}
__device__ __forceinline__ void st16_sc1v(double* p, double v0, double v1) {
  const u32x4 v = u32x4{(unsigned)__double2loint(v0), (unsigned)__double2hiint(v0), (unsigned)__double2loint(v1),
                        (unsigned)__double2hiint(v1)};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st16_plain(double* p, double v0, double v1) {
  const u32x4 v = u32x4{(unsigned)__double2loint(v0), (unsigned)__double2hiint(v0), (unsigned)__double2loint(v1),
                        (unsigned)__double2hiint(v1)};
  asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ double lo_d(const u32x4& r) { return __hiloint2double((int)r[1], (int)r[0]); }
__device__ __forceinline__ double hi_d(const u32x4& r) { return __hiloint2double((int)r[3], (int)r[2]); }
template <int N>
__device__ __forceinline__ void wait8(u32x4 (&x)[8]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
               : "n"(N) : "memory");
}
// sum_rows_n for an even NOUT with 16-byte sc1 loads: thread t owns the chunks (doubles 2c, 2c + 1)
// c = t (and c = t + NT when NOUT / 2 > NT: k = 8) of every row and adds the rows in row order
// (0.0 + r0 + r1 + ...: the same operations, the same bits as sum_rows_n); 16 loads in flight per
// batch (one chunk: 16 rows, two waits of 8 in issue order; two chunks: 8 rows each); the result
// goes to lds_out (optional) and, with 16-byte sc1 stores, to g_out
template <int NOUT>
__device__ __forceinline__ void sum_rows_v(const double* rows, int m0, int step, int cnt, double* lds_out,
                                           double* g_out, int t) {
  static_assert(NOUT % 2 == 0 && NOUT / 2 <= 2 * NT, "one or two 16-byte chunks per thread");
  constexpr int NCH = NOUT / 2, UC = NCH > NT ? 2 : 1;
  const int c0 = t < NCH ? t : NCH - 1;                    // threads past the row re-load its last chunk
  const int c1 = t + NT < NCH ? t + NT : NCH - 1;          // (never stored)
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  if constexpr (UC == 1) {
    for (int m = 0; m < cnt; m += 16) {
      u32x4 xa[8], xb[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) ld16_sc1(xa[r], rows + (size_t)(m0 + min(m + r, cnt - 1) * step) * NOUT + 2 * c0);
#pragma unroll
      for (int r = 0; r < 8; ++r) ld16_sc1(xb[r], rows + (size_t)(m0 + min(m + 8 + r, cnt - 1) * step) * NOUT + 2 * c0);
      wait8<8>(xa);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v0 += m + r < cnt ? lo_d(xa[r]) : 0.0;
        v1 += m + r < cnt ? hi_d(xa[r]) : 0.0;
      }
      wait8<0>(xb);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v0 += m + 8 + r < cnt ? lo_d(xb[r]) : 0.0;
        v1 += m + 8 + r < cnt ? hi_d(xb[r]) : 0.0;
      }
    }
  } else {
    for (int m = 0; m < cnt; m += 8) {
      u32x4 xa[8], xb[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const size_t row = (size_t)(m0 + min(m + r, cnt - 1) * step) * NOUT;
        ld16_sc1(xa[r], rows + row + 2 * c0);
        ld16_sc1(xb[r], rows + row + 2 * c1);
      }
      wait8<0>(xa);  // (both arrays' loads are interleaved: wait for all)
      wait8<0>(xb);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v0 += m + r < cnt ? lo_d(xa[r]) : 0.0;
        v1 += m + r < cnt ? hi_d(xa[r]) : 0.0;
        v2 += m + r < cnt ? lo_d(xb[r]) : 0.0;
        v3 += m + r < cnt ? hi_d(xb[r]) : 0.0;
      }
    }
  }
  if (t < NCH) {
    if (lds_out) {
      lds_out[2 * t] = v0;
      lds_out[2 * t + 1] = v1;
    }
    st16_sc1v(g_out + 2 * t, v0, v1);
  }
  if (UC == 2 && t + NT < NCH) {
    if (lds_out) {
      lds_out[2 * (t + NT)] = v2;
      lds_out[2 * (t + NT) + 1] = v3;
    }
    st16_sc1v(g_out + 2 * (t + NT), v2, v3);
  }
}

// the cross-rank all-reduce of AB inside a persistent launch (xchg_allreduce_ab's protocol,
// generic in the accumulator count NOUT; slot stride 2·NOUT words)
template <int NOUT>
__device__ __forceinline__ void xchg_allreduce_n(uint64_t* xctl, double* AB, double* sAB, uint32_t* err, int it, int t) {
  constexpr int U = (NOUT + NT - 1) / NT;
  const int xrank = (int)__hip_atomic_load(xctl + XC_RANK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int xworld = (int)__hip_atomic_load(xctl + XC_WORLD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t gen =
      (uint32_t)__hip_atomic_load(xctl + XC_GEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint32_t)it + 1u;
  auto peer = [&](int r) {
    return reinterpret_cast<uint64_t*>(__hip_atomic_load(xctl + XC_PEERS + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  };
  TL_X(it, 0);
  const size_t slot = 2 * (size_t)NOUT;
  const size_t par = (size_t)(gen & 1u) * xworld * slot;
  int o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) o[u] = t + NT * u < NOUT ? t + NT * u : t;
  {
    const bool bad = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    const uint64_t tag = (uint64_t)(bad ? sl::XPOISON : gen) << 32;
    for (int pr = 0; pr < xworld; ++pr) {
      uint64_t* dst = peer(pr) + par + (size_t)xrank * slot;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (t + NT * u < NOUT) {
          const uint64_t bv = (uint64_t)__double_as_longlong(sAB[o[u]]);
          __hip_atomic_store(dst + 2 * o[u], tag | (bv & 0xFFFFFFFFull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(dst + 2 * o[u] + 1, tag | (bv >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
  }
  TL_X(it, 1);
  const uint64_t* mine = peer(xrank) + par;
  double v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = 0.0;
  constexpr int QB = 4;  // ranks polled per round (their loads in flight together)
  for (int q0 = 0; q0 < xworld; q0 += QB) {
    uint64_t w[QB][2 * U];
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (true) {
      const uint32_t ev = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // same batch
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const uint64_t* src = mine + (size_t)min(q0 + j, xworld - 1) * slot;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          w[j][2 * u] = __hip_atomic_load(src + 2 * o[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          w[j][2 * u + 1] = __hip_atomic_load(src + 2 * o[u] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      bool ok = true, poison = false;
#pragma unroll
      for (int j = 0; j < QB; ++j)
#pragma unroll
        for (int m = 0; m < 2 * U; ++m) {
          const uint32_t tg = (uint32_t)(w[j][m] >> 32);
          ok = ok && tg == gen;
          poison = poison || tg == sl::XPOISON;
        }
      if (ok) break;
      if (poison) {
        __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (ev != 0u) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > sl::SPIN_TIMEOUT) {
        __hip_atomic_store(err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int j = 0; j < QB; ++j)
      if (q0 + j < xworld)  // rank order
#pragma unroll
        for (int u = 0; u < U; ++u)
          v[u] += __longlong_as_double((long long)((w[j][2 * u + 1] << 32) | (w[j][2 * u] & 0xFFFFFFFFull)));
  }
  TL_X(it, 2);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (t + NT * u < NOUT) {
      sAB[o[u]] = v[u];
      st_sc1(AB + o[u], v[u]);
    }
  TL_X(it, 3);
}


}  // namespace cnmf
