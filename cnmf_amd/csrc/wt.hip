// wt.hip — mu_iter_wt_kernel: n MU iterations as one persistent launch of barrier-free wave tiles
// (cfg2, cfg3), with wt_plan and launch_wt.
#include "wt.hpp"
#include "host.hpp"
#include "keep.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// mu_iter_wt_kernel<PD, MULTI> — the headline shape (fp32 X, F = 81, k = 4) as ONE persistent launch
// of barrier-free WAVE tiles.
//
// Why: the workgroup-tile kernel above (mu_iter_sl_kernel) is issue/latency-bound, not HBM-bound —
// with X served from L2 it runs at the same 67 µs per iteration (profiles/r02/probes/l2diag.log),
// its waves park 46 % of their cycles on two workgroup barriers per tile and on one-deep LDS reads
// of Hᵀ, while a plain streaming read of the same tile shape reaches 7.2 TB/s
// (profiles/r02/probes/stream_probe*.log).
//
// Layout: one 4-wave workgroup per CU, one wave per SIMD (up to 512 VGPRs); every wave owns its own
// 16-sample tiles gw + NW·i (gw = 4·blockIdx + wave, NW = 4·gridDim) and never waits for another
// wave inside an iteration.  Lane l = (sample s = l / 4, quarter q = l % 4); q owns features
// [21q, 21q + 21) (q = 3: 18 real features + 3 zero-Hᵀ pads).
//  * X: PD tiles (5184 B each) in flight per wave in registers (6 × 16 B per lane, the 6th for
//    lanes 0-3 only), staged to the wave's private LDS slot (in-order LDS: no barrier) and read
//    back per lane along its sample row (x kept in 21 VGPRs from phase 1 to phase 3).
//  * Hᵀ: the lane's 21 × 4 fp32 values and its HHᵀ row (fp64) live in VGPRs for the whole
//    iteration (reloaded after each basis update) — no Hᵀ read per tile.
//  * phase 1 (num = x·Hᵀ, SK:543): packed fp32 chains of 7 features folded into fp64 (the sl
//    arithmetic), then a DPP reduce-scatter inside the quad: lane q ends with num[s][q].
//  * phase 2 (SK:553-629): the fp64 update of w[s][q] against the LDS-resident W (each wave's tiles
//    stay in LDS for the whole launch), w' gathered back to the quad by DPP broadcasts.
//  * phase 3 (A += w'ᵀx, B += w'ᵀw', SK:639-640): packed fp32 accumulators per lane over the
//    iteration; at its end a DPP / permlane-swap butterfly over the 16 sample lanes of each q,
//    then the four waves' sums combined in fp64 in a fixed order -> the workgroup's partial row.
//  * the in-launch reduction (tickets, group / top combiners, flag), the basis update in every
//    workgroup and the optional cross-rank exchange are those of mu_iter_sl_kernel.
// ------------------------------------------------------------------------------------------------
template <int KK, bool WRES, int PD, bool MULTI = false, bool TOL = false>
__global__ __launch_bounds__(NT, 1) void mu_iter_wt_kernel(PersistArgs a) {
  using namespace wt;
  using G_ = Geo<KK>;
  constexpr int NL = G_::NL, TSW = G_::TSW, NQ = G_::NQ, V = G_::V, NOUT = G_::NOUT;
  constexpr int NOUTT = NOUT + (TOL ? 1 : 0);  // partial-row width: + the loss of the checked state
  // row stride of the partial / group rows and AB: even, so that every row is 16-byte chunks (round 6:
  // 16-byte sc1 hand-offs; TOL's odd NOUTT + a zero pad — cnmf_mu_fit_tol's rows of k(F+k) + 2)
  // k = 8 keeps the round-5 tail (8-byte hand-offs, the round-5 basis update; see wt_update_basis_r5)
  constexpr bool R6 = KK == 4;
  constexpr int RS = R6 ? (NOUTT + 1) & ~1 : NOUTT;
  constexpr int XBW = G_::XBW, XSTR = G_::XSTR, WBW = G_::WBW, NACC = G_::NACC;
  constexpr int PFW = G_::PFW, LASTL = G_::LASTL;
  constexpr int PFS = PFW + (WRES ? 0 : 1);  // loads per prefetch set (+ the W tile when streamed)
  // stores per body: W streamed — its W tile, and TOL's snapshot of the checked state's W (a resident
  // W keeps that snapshot in LDS: no store, so the counted waits are the plain kernel's)
  constexpr int NSTB = (WRES ? 0 : 1) + (TOL && !WRES ? 1 : 0);
  constexpr int KP = KK / 2;                 // component pairs
  // the PD prefetch sets live in AGPRs (4 per load) next to the kernel's own registers: past a
  // budget the allocator spills them to scratch right behind their loads, i.e. before the data has
  // landed, and the staged tiles are stale (k = 8 streamed W at PD = 6: 96 AGPRs, all-NaN W at 2.5x
  // the time).  tools/kcheck.py checks the built library for exactly that; the
  // depths measured clean are allowed here (k = 8: PD <= 5, 80 AGPRs; k = 4: PD <= 4, 96)
  static_assert(4 * PD * PFS <= (KK == 8 ? 80 : 96), "prefetch depth past the measured AGPR budget");
  static_assert(PFS * (PD - 1) + NSTB * PD <= 63, "the counted wait's vmcnt is a 6-bit field");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int s = l / NL, e = l % NL;
  const int b = blockIdx.x;
  const int G = gridDim.x;
  const int NW = NWV * G;
  const int gw = NWV * b + w;
  const int NG = a.n_groups;
  const int g = b % NG;
  const int gs = (G - g + NG - 1) / NG;
  const unsigned char* Xb = reinterpret_cast<const unsigned char*>(a.X);
  unsigned char* Wb = reinterpret_cast<unsigned char*>(a.W);
  const int nbt = (int)((a.n_tiles - gw + NW - 1) / NW);  // this wave's tiles per iteration
  const int nbt_max = (int)((a.n_tiles + NW - 1) / NW);
  unsigned char* stg = smem + G_::L_STG + w * XSTR;
  unsigned char* wstg = smem + G_::L_WSTG + w * WBW;  // streamed W: this wave's current tile
  // W streamed: its first nres tiles per wave resident all the same (the LDS the plan has left; round
  // 5): their W loads re-load an X chunk (the counted waits see the same loads) and their stores go
  // to the dummy word (the same stores), the rest streams
  const int nres = WRES ? 0 : __builtin_amdgcn_readfirstlane(a.n_static);
  const int xkeep = __builtin_amdgcn_readfirstlane(a.x_keep16);  // sixteenths of X kept in the cache
  float* wres = reinterpret_cast<float*>(smem + G_::L_WRES + (size_t)w * (WRES ? nbt_max : nres) * WBW);  // [i][TSW][K]
  float* red = reinterpret_cast<float*>(smem + G_::L_RED);
  double* sH = reinterpret_cast<double*>(smem + G_::L_H);
  double* sAB = reinterpret_cast<double*>(smem + G_::L_AB);
  int* sFlag = reinterpret_cast<int*>(smem + G_::L_FLAG);
  double* sLoss = reinterpret_cast<double*>(smem + G_::L_LOSS);
  // TOL: the launch's first global iteration, the snapshot buffer (streamed W)
  const int it0 = TOL ? (int)ld_sc1(a.tolctl + TC_IT0) : 0;
  // TOL: every workgroup tracks the test's error at init and previous error itself (sLoss[4], [5]),
  // so the decision of the iteration's top combiner reads no state another workgroup wrote
  const double tolv = TOL ? ld_sc1(a.tolctl + TC_TOL) : 0.0;
  if (TOL && t == 0) {
    sLoss[4] = ld_sc1(a.tolctl + TC_INIT);
    sLoss[5] = ld_sc1(a.tolctl + TC_PREV);
  }
  float* wsnap = (TOL && !WRES)
                     ? reinterpret_cast<float*>(__double_as_longlong(ld_sc1(a.tolctl + TC_WSNAP)))
                     : nullptr;
  // TOL with W resident: the W of the state a loss iteration checks, this wave's tiles [i][TSW][K],
  // after the four waves' resident W (the host sizes the LDS for both)
  float* wsnapl = (TOL && WRES) ? reinterpret_cast<float*>(smem + G_::L_WRES + (size_t)(NWV + w) * nbt_max * WBW)
                                : nullptr;
  double lossacc = 0.0;  // this lane's ‖x − w·H‖² over the iteration's tiles (loss iterations)
  uint32_t* cnt_group = a.cnt + CNT_GROUP0 + 32 * g;
  uint32_t* cnt_top = a.cnt + CNT_TOP;
  uint32_t* flag = a.cnt + CNT_FLAG;
  uint32_t* err = a.cnt + CNT_ERR;

  // ---- the basis for the first iteration, the staging pads, this wave's W tiles (W resident)
  const bool l2rows = R6 && a.l2rows != 0;
  if (t == 0) {  // the XCC this workgroup runs on, into the table (read once, after iteration 0)
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    sFlag[4] = 0;  // partial rows write-through until the group's placement has been checked
    sFlag[5] = (int)(xcc & 0xFu) + 1;
    if (l2rows) __hip_atomic_store(a.cnt + CNT_XCC0 + b, (xcc & 0xFu) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int i = t; i < KK * F; i += NT) sH[i] = a.H64[i];
  if (a.apply_first)
    for (int i = t; i < NOUT; i += NT) sAB[i] = a.AB[i];
  if (l < G_::PADB / 4) reinterpret_cast<float*>(stg + XBW)[l] = 0.f;
  {
    const int nw = WRES ? nbt : min(nres, nbt);
    for (int c = l; c < nw * (WBW / 16); c += 64) {
      const int i = c / (WBW / 16), ch = c - i * (WBW / 16);
      *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(wres) + i * WBW + 16 * ch) =
          *reinterpret_cast<const u32x4*>(Wb + (size_t)(gw + (int64_t)NW * i) * WBW + 16 * ch);
    }
  }
  __syncthreads();
  if (a.apply_first) {
    if constexpr (R6) wt_update_basis<KK>(smem, t, a.l1H, a.l2H);
    else wt_update_basis_r5<KK>(smem, t, a.l1H, a.l2H);
  } else {
    if constexpr (R6) wt_derive_basis<KK>(smem, t);
    else wt_derive_basis_r5<KK>(smem, t);
  }

  // the lane's Hᵀ (fp32 component pairs of each of its NQ features) and HHᵀ row e
  f2 hp[NQ][KP];
  double hh[KK];
  f2 hh32[KP];  // k = 8: the HHᵀ row in fp32 pairs for the denominator
  auto load_basis = [&]() {
    const float* sHt = reinterpret_cast<const float*>(smem + G_::L_HT);
    const double* sHHt = reinterpret_cast<const double*>(smem + G_::L_HHT);
#pragma unroll
    for (int c = 0; c < NQ; ++c)
#pragma unroll
      for (int p4 = 0; p4 < KK / 4; ++p4) {
        const float4 h = *reinterpret_cast<const float4*>(sHt + (NQ * e + c) * KK + 4 * p4);
        hp[c][2 * p4] = f2{h.x, h.y};
        hp[c][2 * p4 + 1] = f2{h.z, h.w};
      }
#pragma unroll
    for (int m = 0; m < KK; ++m) hh[m] = sHHt[e * KK + m];
#pragma unroll
    for (int q = 0; q < KP; ++q) hh32[q] = f2{(float)hh[2 * q], (float)hh[2 * q + 1]};
  };
  load_basis();

  f2 acc[NQ][KP], accB[KP];
  auto zero_acc = [&]() {
#pragma unroll
    for (int c = 0; c < NQ; ++c)
#pragma unroll
      for (int p = 0; p < KP; ++p) acc[c][p] = f2{0.f, 0.f};
#pragma unroll
    for (int p = 0; p < KP; ++p) accB[p] = f2{0.f, 0.f};
  };
  zero_acc();

  // the tile's 16-byte chunks of this lane: l + 64u (u < PFW - 1) and, for lanes < LASTL, the last
  // (other lanes re-load chunk l: never staged; every lane issues the same loads), then the W tile
  // when streamed (lanes < 16; others re-load chunk l)
  auto prefetch = [&](u32x4 (&pf)[PFS], int64_t tile, int ti) {
#ifdef CNMF_DIAG_L2
    const unsigned char* xs = Xb + (size_t)(tile & 255) * XBW + 16 * l;
#else
    const unsigned char* xs = Xb + (size_t)tile * XBW + 16 * l;
#endif
    // X kept in the Infinity Cache: tile position ti of this wave loads with the
    // default policy when ((ti + gw) & 15) < x_keep16 — the same addresses in every iteration, the
    // same share in every wave, the HBM-served positions spread over the chip at every moment
    ld_set<PFW>(pf, xs, l < LASTL ? xs + 1024 * (PFW - 1) : xs, (ti + gw) & 15, xkeep);
    if (!WRES) ld16(pf[PFW], (l < WBW / 16 && ti >= nres) ? Wb + (size_t)tile * WBW + 16 * l : xs);
  };
  auto stage = [&](const u32x4 (&pf)[PFS]) {
    const unsigned addr = (unsigned)(uintptr_t)(stg + 16 * l);
    stage_rec<0, PFW - 1>(addr, pf);
    if (l < LASTL) st16<1024 * (PFW - 1)>(addr, pf[PFW - 1]);
    if (!WRES && l < WBW / 16) st16<0>((unsigned)(uintptr_t)(wstg + 16 * l), pf[PFW]);
  };

  const int total = a.n_iter * nbt;
  u32x4 pf[PD][PFS];
  // W streamed: after each of the first PD sets one dummy store (to this workgroup's partial row,
  // rewritten at the iteration's end), so that every set — the first PD too — has exactly PD stores
  // younger than it when its step waits (set q < PD: PD - q dummies, then the W stores of bodies
  // 0..q-1).  Counting PD stores that were never issued would let the set's last loads (the W tile)
  // still be in flight when it is staged.
  float* dummy = reinterpret_cast<float*>(a.partials + (size_t)b * RS) + 64 * w + l;
#pragma unroll
  for (int k = 0; k < PD; ++k) {
    prefetch(pf[k], gw + (int64_t)NW * k, k);  // the host keeps nbt > PD
#pragma unroll
    for (int d = 0; d < NSTB; ++d) asm volatile("global_store_dword %0, %1, off" ::"v"(dummy), "v"(0) : "memory");
  }
  // W streamed: a tile's W store (body x) must have retired before its next load is issued (the
  // prefetch at step x + nbt - PD); the step waits retire every operation older than the set they
  // wait for, which covers that store when nbt >= 2·PD + 1 (the host guarantees it)
  TL_START;

  bool alive = true;
  // position counters (wave-uniform, incremental: no division per tile): the tile being processed
  // (iteration cur_it, index cur_i) and the next one to prefetch (nx_i).  Every step stages its
  // register set and re-issues it unconditionally (past the launch's last position: the wave's
  // first tile again, never used), so the count of younger loads is the same on every path.
  int cur_i = 0, cur_it = 0, nx_i = PD;
  auto step = [&](u32x4 (&pfk)[PFS]) {
    // younger than this set's loads: the PD-1 later sets and the stores of the PD bodies since
    // (for the launch's first PD sets the prologue's dummy stores): with W streamed its W store, and
    // TOL the snapshot store every body issues (a loss iteration's W, else a dummy)
    wait_set<PFS * (PD - 1) + NSTB * PD, PFS>(pfk);
    stage(pfk);
    prefetch(pfk, gw + (int64_t)NW * nx_i, nx_i);
    if (++nx_i == nbt) nx_i = 0;
  };
  auto body = [&]() {
    const int it = cur_it, i = cur_i;
    if (++cur_i == nbt) {
      cur_i = 0;
      ++cur_it;
    }
    const bool last_it = it + 1 == a.n_iter;
#ifdef CNMF_TOL_NOLOSS  // timing-only diagnostic: the TOL kernel without its loss iterations (never stops)
    const bool loss_it = false;
#else
    const bool loss_it = TOL && ((it0 + it) % 10 == 0);  // check the state after it0 + it iterations
#endif
    const int64_t tile = gw + (int64_t)NW * i;
    // phase 2 first where it does not need x: the sample's W row and den = w·HHᵀ[e] with its refined
    // reciprocal (div_nr's v_rcp_f64 + Newton step, so w·num·r is div_nr's arithmetic) — their loads
    // and their ~15-deep dependent chain then overlap phase 1 instead of following the reduce-scatter
    // (round 5).  SK:553-629
    const bool wr = WRES || i < nres;  // this tile's W resident
    float* wt_ = wr ? wres + i * (TSW * KK) : reinterpret_cast<float*>(wstg);
    float wv[KK];
#pragma unroll
    for (int m4 = 0; m4 < KK / 4; ++m4) {
      const float4 v4 = *reinterpret_cast<const float4*>(wt_ + s * KK + 4 * m4);
      wv[4 * m4] = v4.x;
      wv[4 * m4 + 1] = v4.y;
      wv[4 * m4 + 2] = v4.z;
      wv[4 * m4 + 3] = v4.w;
    }
    const float wold32 = wt_[s * KK + e];
    const double wold = (double)wold32;
    double den = 0.0;
    if constexpr (KK == 8) {
      // den = w·HHᵀ[e] in packed fp32 (8 positive terms: no cancellation, ≤ 8 roundings), the
      // update itself in fp64
      f2 d2 = f2{0.f, 0.f};
#pragma unroll
      for (int q = 0; q < KP; ++q) d2 = __builtin_elementwise_fma(f2{wv[2 * q], wv[2 * q + 1]}, hh32[q], d2);
      den = (double)(d2.x + d2.y);
    } else {
#pragma unroll
      for (int m = 0; m < KK; ++m) den = fma((double)wv[m], hh[m], den);
    }
    if (a.l1W > 0.0) den += a.l1W;              // SK:616-617
    if (a.l2W > 0.0) den = den + a.l2W * wold;  // SK:618-619
    if (den == 0.0) den = EPS32;                // SK:620
    double rden = __builtin_amdgcn_rcp(den);
    rden = fma(rden, fma(-den, rden, 1.0), rden);
    // phase 1: x along the lane's row, packed fp32 chains of 7 features folded into fp64
    const float* xr = reinterpret_cast<const float*>(stg) + s * F + NQ * e;
    float xv[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) xv[c] = xr[c];
    double num;
    if constexpr (KK == 8) {
      // k = 8: ONE fp32 chain over the lane's 11 features, then the reduce-scatter over the
      // sample's 8 lanes in fp32 (3 adds per value; a chain of 11 + 3 roundings, below the 7-term
      // chains' error budget of §4), one DPP move per 32-bit value: level 1 pairs lane e with 7 - e
      // (row_half_mirror: the other half of components), then e ^ 2 and e ^ 1 (quad_perm)
      f2 ch[KP];
#pragma unroll
      for (int q = 0; q < KP; ++q) ch[q] = f2{0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        const f2 xx = f2{xv[c], xv[c]};
#pragma unroll
        for (int q = 0; q < KP; ++q) ch[q] = __builtin_elementwise_fma(xx, hp[c][q], ch[q]);
      }
      const bool b4 = (e & 4) != 0, b2 = (e & 2) != 0, b1 = (e & 1) != 0;
      f2 r[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const f2 keep = b4 ? ch[2 + m] : ch[m], send = b4 ? ch[m] : ch[2 + m];
        r[m] = keep + f2{dppf<0x141>(send.x), dppf<0x141>(send.y)};  // row_half_mirror
      }
      const f2 keep2 = b2 ? r[1] : r[0], send2 = b2 ? r[0] : r[1];
      const f2 t2 = keep2 + f2{dppf<0x4E>(send2.x), dppf<0x4E>(send2.y)};  // quad_perm [2,3,0,1]
      const float keep1 = b1 ? t2.y : t2.x, send1 = b1 ? t2.x : t2.y;
      num = (double)(keep1 + dppf<0xB1>(send1));  // quad_perm [1,0,3,2]
    } else {
      // k = 4: packed fp32 chains of 7 features folded into fp64, fp64 reduce-scatter over the
      // sample's 4 lanes
      double p[KK];
#pragma unroll
      for (int c0 = 0; c0 < NQ; c0 += 7) {
        f2 ch[KP];
#pragma unroll
        for (int q = 0; q < KP; ++q) ch[q] = f2{0.f, 0.f};
#pragma unroll
        for (int c = c0; c < (c0 + 7 < NQ ? c0 + 7 : NQ); ++c) {
          const f2 xx = f2{xv[c], xv[c]};
#pragma unroll
          for (int q = 0; q < KP; ++q) ch[q] = __builtin_elementwise_fma(xx, hp[c][q], ch[q]);
        }
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          if (c0 == 0) {
            p[2 * q] = (double)ch[q].x;
            p[2 * q + 1] = (double)ch[q].y;
          } else {
            p[2 * q] += (double)ch[q].x;
            p[2 * q + 1] += (double)ch[q].y;
          }
        }
      }
      const bool b1 = (e & 1) != 0, b2 = (e & 2) != 0;
      double k2[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const double keep = b2 ? p[2 + m] : p[m], send = b2 ? p[m] : p[2 + m];
        k2[m] = keep + dpp64<0x4E>(send);  // quad_perm [2,3,0,1]
      }
      const double keep = b1 ? k2[1] : k2[0], send = b1 ? k2[0] : k2[1];
      num = keep + dpp64<0xB1>(send);  // quad_perm [1,0,3,2]
    }
    if constexpr (TOL && WRES) {
      // the W of the state a loss iteration checks, kept in LDS (written to HBM only on a stop)
      if (loss_it) wsnapl[i * (TSW * KK) + s * KK + e] = wold32;
    } else if constexpr (TOL) {
      // W streamed: the W of the checked state, ONE store per body in every iteration (the steps'
      // waits count it): a loss iteration stores the tile's W into the snapshot buffer, the others
      // the same value over the wave's first tile there, which the next loss iteration overwrites
      // (a stop happens only at the end of a loss iteration)
      const int64_t tsel = loss_it ? tile : (int64_t)gw;
      wsnap[(size_t)tsel * TSW * KK + l] = wold32;
    }
    if (loss_it) {
      // ‖x − w·H‖² of the state before this update, the lane's NQ features (the last lane's overrun
      // features past F belong to the next sample: masked)
      float l2 = 0.f;
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        f2 r2 = f2{0.f, 0.f};
#pragma unroll
        for (int q = 0; q < KP; ++q) r2 = __builtin_elementwise_fma(f2{wv[2 * q], wv[2 * q + 1]}, hp[c][q], r2);
        const float r = NQ * e + c < F ? xv[c] - (r2.x + r2.y) : 0.f;
        l2 = fmaf(r, r, l2);
      }
      lossacc += (double)l2;
    }
    const float wn = (float)(wold * (num * rden));  // SK:622-629 (div_nr's arithmetic)
    wt_[s * KK + e] = wn;
    if (!WRES) {  // lane l = (s, e); a resident tile's store goes to the dummy word
      if (!wr) reinterpret_cast<float*>(Wb)[(size_t)tile * TSW * KK + l] = wn;
      else asm volatile("global_store_dword %0, %1, off" ::"v"(dummy), "v"(0) : "memory");
    }
    // w'[s][·]: the sample's row back from LDS (this wave's writes above precede the reads)
    f2 wp[KP];
#pragma unroll
    for (int m4 = 0; m4 < KK / 4; ++m4) {
      const float4 v4 = *reinterpret_cast<const float4*>(wt_ + s * KK + 4 * m4);
      wp[2 * m4] = f2{v4.x, v4.y};
      wp[2 * m4 + 1] = f2{v4.z, v4.w};
    }
    // phase 3: A[·][f] += w'·x[f], B[e][·] += w'_e·w' (fp32 per lane over the iteration)
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      const f2 xx = f2{xv[c], xv[c]};
#pragma unroll
      for (int q = 0; q < KP; ++q) acc[c][q] = __builtin_elementwise_fma(xx, wp[q], acc[c][q]);
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) accB[q] = __builtin_elementwise_fma(f2{wn, wn}, wp[q], accB[q]);
    if (i + 1 != nbt) return;

    // ---- end of this wave's iteration: its sums over the sample lanes of each e -> LDS
    // (reduce-scatter, round 6: value j = c·KK + 2q + comp (A), NQ·KK + 2q + comp (B); row r of the
    // wave ends with the quarter of the values scatter_over_samples names, written by the row's
    // lanes of sample 0, in pairs of floats)
    {
      float vv[NACC];
#pragma unroll
      for (int c = 0; c < NQ; ++c)
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          vv[c * KK + 2 * q] = acc[c][q].x;
          vv[c * KK + 2 * q + 1] = acc[c][q].y;
        }
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        vv[NQ * KK + 2 * q] = accB[q].x;
        vv[NQ * KK + 2 * q + 1] = accB[q].y;
      }
      scatter_over_samples<NL>(vv);
      constexpr int NQT = NACC / 4;
      static_assert(NQT % 2 == 0, "the quarters are written in pairs of floats");
      const int r = l >> 4;
      float* rw = red + (w * NL + e) * NACC + (NACC / 2) * (r >> 1) + NQT * (r & 1);
      if ((l & 15) < NL)
#pragma unroll
        for (int j = 0; j < NQT; j += 2) *reinterpret_cast<float2*>(rw + j) = make_float2(vv[j], vv[j + 1]);
    }
    zero_acc();
    if (TOL) {  // the wave's loss sum (zero outside loss iterations), fixed xor tree
      const double v = wave_sum(lossacc);
      if (l == 0) sLoss[w] = v;
      lossacc = 0.0;
    }
    __syncthreads();
    TL_PRE(it);
    // the workgroup's fp64 row [K][V] (+ the loss): the four waves' sums in wave order (deterministic)
    {
      double* prow = a.partials + (size_t)b * RS;
      const bool plain = sFlag[4] != 0;  // the group's rows through the XCD's L2 (l2rows)
      auto row_val = [&](int o) {
        const int j = o / V;
        const int v = o - j * V;
        const int ee = v < F ? v / NQ : j;
        const int idx = v < F ? (v - NQ * ee) * KK + j : NQ * KK + (v - F);
        const float* rr = red + ee * NACC + idx;
        constexpr int WS = NL * NACC;  // wave stride
        return ((double)rr[0] + (double)rr[WS]) + ((double)rr[2 * WS] + (double)rr[3 * WS]);
      };
      // pairs of doubles, one 16-byte store each (round 6); TOL: the loss at NOUT, a zero pad after it
      auto val = [&](int o) {
        if (o < NOUT) return row_val(o);
        return (TOL && o == NOUT) ? (sLoss[0] + sLoss[1]) + (sLoss[2] + sLoss[3]) : 0.0;
      };
      if constexpr (R6) {
        for (int c = t; c < RS / 2; c += NT) {
          const double v0 = val(2 * c), v1 = val(2 * c + 1);
          if (plain) st16_plain(prow + 2 * c, v0, v1);
          else st16_sc1v(prow + 2 * c, v0, v1);
        }
      } else {
        for (int o = t; o < NOUTT; o += NT) __hip_atomic_store(prow + o, val(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave: its sc1 stores landed
    __syncthreads();
    TL(it, 0);
    if (t == 0) {
      const uint32_t old = __hip_atomic_fetch_add(cnt_group, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sFlag[0] = old == (uint32_t)((it + 1) * gs - 1);
      sFlag[1] = 0;
      sFlag[2] = 1;
      sFlag[3] = 0;
    }
    __syncthreads();
    // the last iteration of the launch waits for the flag too when it checks the tolerance (a stop
    // there must reach every workgroup before it writes W back)
    const bool must_wait = !last_it || loss_it;
    if (sFlag[0]) {  // group combiner
      TL_LV(it, g, 0);
      if constexpr (R6) sum_rows_v<RS>(a.partials, g, NG, gs, nullptr, a.groups + (size_t)g * RS, t);
      else sum_rows_n<RS>(a.partials, g, NG, gs, nullptr, a.groups + (size_t)g * RS, t);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      TL_LV(it, g, 1);
      if (t == 0) {
        const uint32_t old = __hip_atomic_fetch_add(cnt_top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sFlag[1] = old == (uint32_t)((it + 1) * NG - 1);
      }
      __syncthreads();
      if (sFlag[1]) {  // top combiner: AB
        TL_LV(it, TL_LVG, 0);
        if constexpr (R6) {
          sum_rows_v<RS>(a.groups, 0, 1, NG, sAB, a.AB, t);
          if (MULTI) __syncthreads();  // the exchange reads sAB in sum_rows_n's thread mapping
        } else {
          sum_rows_n<RS>(a.groups, 0, 1, NG, sAB, a.AB, t);
        }
        if (MULTI) xchg_allreduce_n<NOUTT>(a.xctl, a.AB, sAB, err, it, t);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        TL_LV(it, TL_LVG, 1);
        // (after the barrier: the summed loss sAB[NOUT] was written by another thread)
        if (TOL && loss_it && t == 0) {  // SK:872-884 on the state after it0 + it iterations
          const int gi = it0 + it;
          const double errv = sqrt(fmax(sAB[NOUT], 0.0));
          const int slot = gi / 10;
          if (slot < (int)ld_sc1(a.tolctl + TC_CAP)) st_sc1(a.tolctl + TC_ERRS + slot, errv);
          st_sc1(a.tolctl + TC_NERR, (double)(slot + 1));
          if (gi == 0) {
            sLoss[4] = sLoss[5] = errv;
            st_sc1(a.tolctl + TC_INIT, errv);
            st_sc1(a.tolctl + TC_PREV, errv);
          } else if ((sLoss[5] - errv) / sLoss[4] < tolv) {
            sFlag[3] = 1;
          } else {
            sLoss[5] = errv;
            st_sc1(a.tolctl + TC_PREV, errv);
          }
        }
        if (TOL && loss_it) __syncthreads();  // sFlag[3] (the decision) for the whole workgroup
        if (t == 0 && must_wait)
          __hip_atomic_store(flag, (uint32_t)(it + 1) | (sFlag[3] ? FLAG_STOP : 0u), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        TL_PUB(it);
      }
    }
    const bool top = sFlag[1] != 0;
    if (!top && must_wait) {
      if (t == 0) {
        const uint32_t want = (uint32_t)(it + 1);
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        uint32_t f;
        while (true) {  // the flag and the error word in one batch: one round trip per round
          const uint32_t ev = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          f = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((f & ~FLAG_STOP) >= want) break;
          if (ev != 0u) {
            sFlag[2] = 0;
            break;
          }
          if (__builtin_amdgcn_s_memrealtime() - t0 > sl::SPIN_TIMEOUT) {
            __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sFlag[2] = 0;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        if (TOL && (f & FLAG_STOP)) sFlag[3] = 1;
        TL_SEEN(it);
      }
      __syncthreads();
      if (!sFlag[2]) {  // a workgroup never arrived (not co-resident): give up, error word set
        alive = false;
        return;
      }
    }
    if (TOL && sFlag[3]) {
      // stopped by the tolerance test: the state after it0 + it iterations (W: the loss
      // iteration's LDS snapshot written back here, or the host copies the streamed-W snapshot
      // buffer; H = sH not updated); the host clears the flag word after the launch
      alive = false;
      if (WRES)
        for (int c = l; c < nbt * (WBW / 16); c += 64) {
          const int ii = c / (WBW / 16), ch = c - ii * (WBW / 16);
          *reinterpret_cast<u32x4*>(Wb + (size_t)(gw + (int64_t)NW * ii) * WBW + 16 * ch) =
              *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(wsnapl) + ii * WBW + 16 * ch);
        }
      if (!top) return;
      for (int o = t; o < KK * F; o += NT) a.H64[o] = sH[o];
      for (int o = t; o < F * KK; o += NT) {
        const int f = o / KK;
        const int j = o - f * KK;
        a.Ht[o] = sH[j * F + f];
      }
      if (t < KK * KK) a.HHt[t] = reinterpret_cast<const double*>(smem + G_::L_HHT)[t];
      if (t < NG) __hip_atomic_store(a.cnt + CNT_GROUP0 + 32 * t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (l2rows)
        for (int o = t; o < G; o += NT) __hip_atomic_store(a.cnt + CNT_XCC0 + o, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == 0) {
        __hip_atomic_store(cnt_top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st_sc1(a.tolctl + TC_DONE, (double)(it0 + it));
        st_sc1(a.tolctl + TC_STOPPED, 1.0);
        st_sc1(a.tolctl + TC_IN_SNAP, WRES ? 0.0 : 1.0);
        if (MULTI)
          __hip_atomic_fetch_add(a.xctl + XC_GEN, (uint64_t)(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    if (last_it) {
      alive = false;
      if (WRES || nres > 0)  // this wave's resident W back to HBM, once per launch
        for (int c = l; c < (WRES ? nbt : min(nres, nbt)) * (WBW / 16); c += 64) {
          const int ii = c / (WBW / 16), ch = c - ii * (WBW / 16);
          *reinterpret_cast<u32x4*>(Wb + (size_t)(gw + (int64_t)NW * ii) * WBW + 16 * ch) =
              *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(wres) + ii * WBW + 16 * ch);
        }
      if (!top) return;
      // the last combiner of the launch: every other workgroup has arrived for the last time
      if (a.apply_last) {
        if constexpr (R6) wt_update_basis<KK>(smem, t, a.l1H, a.l2H);
        else wt_update_basis_r5<KK>(smem, t, a.l1H, a.l2H);
      }
      for (int o = t; o < KK * F; o += NT) a.H64[o] = sH[o];
      for (int o = t; o < F * KK; o += NT) {
        const int f = o / KK;
        const int j = o - f * KK;
        a.Ht[o] = sH[j * F + f];
      }
      if (t < KK * KK) a.HHt[t] = reinterpret_cast<const double*>(smem + G_::L_HHT)[t];
      if (t < NG) __hip_atomic_store(a.cnt + CNT_GROUP0 + 32 * t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (l2rows)
        for (int o = t; o < G; o += NT) __hip_atomic_store(a.cnt + CNT_XCC0 + o, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == 0) {
        __hip_atomic_store(cnt_top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!must_wait)  // (else workgroups may still poll it: the host clears it after the launch)
          __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (TOL) {
          st_sc1(a.tolctl + TC_DONE, (double)(it0 + a.n_iter));
          st_sc1(a.tolctl + TC_STOPPED, 0.0);
        }
        if (MULTI)  // the next launch's generations follow this one's
          __hip_atomic_fetch_add(a.xctl + XC_GEN, (uint64_t)a.n_iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    if (!top) {
      if constexpr (!R6) {
        for (int o = t; o < NOUTT; o += NT) sAB[o] = ld_sc1(a.AB + o);
      } else {  // 16-byte sc1 loads, all in flight together (round 6)
        constexpr int NCH = RS / 2;
        const int c0 = t < NCH ? t : 0, c1 = t + NT < NCH ? t + NT : 0;
        u32x4 r0, r1;
        ld16_sc1(r0, a.AB + 2 * c0);
        if (NCH > NT) ld16_sc1(r1, a.AB + 2 * c1);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(r0), "+v"(r1) : : "memory");
        if (t < NCH) {
          sAB[2 * t] = lo_d(r0);
          sAB[2 * t + 1] = hi_d(r0);
        }
        if (t + NT < NCH) {
          sAB[2 * (t + NT)] = lo_d(r1);
          sAB[2 * (t + NT) + 1] = hi_d(r1);
        }
      }
      __syncthreads();
      TL_AB(it);
      if (TOL && loss_it && t == 0) {  // the top went on: prev <- this check's error
        const double errv = sqrt(fmax(sAB[NOUT], 0.0));
        if (it0 + it == 0) sLoss[4] = errv;
        sLoss[5] = errv;
      }
    }
    if (l2rows && it == 0 && w == 0) {
      // every member has written its XCC (at its start, before its first arrival): the group's rows
      // may go through the L2 when all of them share this workgroup's XCC (the same answer in every
      // member: they read the same table)
      const uint32_t xm = l < gs ? __hip_atomic_load(a.cnt + CNT_XCC0 + g + NG * l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : (uint32_t)sFlag[5];
      const bool same = __ballot(xm != (uint32_t)sFlag[5]) == 0;
      if (l == 0) sFlag[4] = same ? 1 : 0;
    }
    if constexpr (R6) wt_update_basis<KK>(smem, t, a.l1H, a.l2H);
    else wt_update_basis_r5<KK>(smem, t, a.l1H, a.l2H);
    TL_UPD(it);
    load_basis();
    TL(it, 1);
  };

  for (int p = 0; p < total && alive; p += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      step(pf[k]);
      if (p + k < total && alive) body();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no load outlives the workgroup
}


// ---- variant 4: barrier-free wave tiles (mu_iter_wt_kernel<K, WRES, PD, MULTI>: one 4-wave
// workgroup per CU, each wave on its own tiles; fp32 X, F = 81, k = 4 (16-sample tiles) or k = 8
// (8-sample tiles); W resident in LDS when the grid's share fits, else streamed with X).
// CNMF_WT_PD = prefetch depth 2..4 of the k = 4 W-resident single-GPU kernel, 3..5 of the k = 8
// streamed-W one (default 3).
int wt_pd(int k, bool wres, bool multi) {
  const char* v = diag_env("CNMF_WT_PD");
  const int pd = v ? atoi(v) : 3;
  if (k == 4 && wres && !multi && pd >= 2 && pd <= 4) return pd;
  if (k == 8 && !wres && !multi && pd >= 3 && pd <= 5) return pd;
  return 3;
}
template <int KK, bool WRES>
static PassFn wt_fn_k(int pd, bool multi, bool tol) {
  if (tol)  // the device tolerance test: PD = 3
    return multi ? reinterpret_cast<PassFn>(&mu_iter_wt_kernel<KK, WRES, 3, true, true>)
                 : reinterpret_cast<PassFn>(&mu_iter_wt_kernel<KK, WRES, 3, false, true>);
  if (multi) return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<KK, WRES, 3, true>);
#ifdef CNMF_DIAG  // the prefetch-depth sweeps (CNMF_WT_PD): diagnostic build only
  if (KK == 4 && WRES && pd == 2) return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<4, true, 2, false>);
  if (KK == 4 && WRES && pd == 4) return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<4, true, 4, false>);
  if (KK == 8 && !WRES && pd == 4) return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<8, false, 4, false>);
  if (KK == 8 && !WRES && pd == 5) return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<8, false, 5, false>);
#else
  (void)pd;
#endif
  return reinterpret_cast<PassFn>(&mu_iter_wt_kernel<KK, WRES, 3, false>);
}
static PassFn wt_fn(int k, bool wres, bool multi, bool tol = false) {
  const int pd = tol ? 3 : wt_pd(k, wres, multi);
  if (k == 4) return wres ? wt_fn_k<4, true>(pd, multi, tol) : wt_fn_k<4, false>(pd, multi, tol);
  return wres ? wt_fn_k<8, true>(pd, multi, tol) : wt_fn_k<8, false>(pd, multi, tol);
}
// the wave-tile launch for this shape, or false (not eligible: another kernel serves it).  k = 4
// follows the layout switch (variant 4, the default); k = 8 has no other persistent layout.
bool wt_plan(int64_t n_rows, int x_dtype, int F, int k, bool multi, int layout, WtLaunch* out, bool tol) {
  if (x_dtype != CNMF_F32 || F != wt::F || (k != 4 && k != 8) || n_rows <= 0) return false;
  if (k == 4 && layout != 4) return false;
  if (k == 8 && layout != 4 && layout != 5) return false;
  // k = 8, layout 4: the VALU wave tiles (8-sample tiles); layout 5 (rows a multiple of 16): the
  // matrix-core wave tiles (16-sample tiles; slower than layout 4 on the MI355X measured)
  const bool mf = k == 8 && layout == 5 && n_rows % 16 == 0;
  const int tsw = mf ? 16 : 64 / k, wbw = tsw * k * 4;
  if (n_rows % tsw != 0) return false;
  const size_t l_wres = mf ? (size_t)wt::GeoMF8::L_WRES
                           : (k == 4 ? (size_t)wt::Geo<4>::L_WRES : (size_t)wt::Geo<8>::L_WRES);
  const int ncu = device_cus();
  const int64_t n_tiles = n_rows / tsw;
  for (int wres = 1; wres >= 0; --wres) {
    const int pd = tol ? 3 : wt_pd(k, wres != 0, multi);
    // tiles per wave: > PD (the first prefetches), >= 2·PD + 1 when W is streamed (re-load hazard)
    const int min_nbt = wres ? pd + 1 : 2 * pd + 1;
    int64_t G = std::min<int64_t>({(int64_t)ncu, n_tiles / (wt::NWV * min_nbt), (int64_t)sl::GROUP * sl::MAX_GROUPS});
    if (const char* mg = diag_env("CNMF_WT_MAXG"))  // diagnostic: fewer, fuller waves (strong-scaling shards)
      if (atoi(mg) > 0) G = std::min<int64_t>(G, atoi(mg));
    if (G < 1) continue;
    const int64_t nbt_max = (n_tiles + wt::NWV * G - 1) / (wt::NWV * G);
    // W resident: the four waves' W tiles; TOL (the wave-tile kernel) a second copy: the snapshot of
    // the checked state
    size_t lds = l_wres + (wres ? (size_t)wt::NWV * nbt_max * wbw * (tol && !mf ? 2 : 1) : 0);
    if (lds > kMaxLds) continue;
    // W streamed (the VALU wave tiles): as many of each wave's tiles W-resident as the LDS holds —
    // their W neither read nor written through HBM in the iterations (cfg3's shard: ~78 % of its W
    // traffic).  CNMF_WT_NRES (diagnostic) caps it; 0 streams every tile.
    int nres = 0;
    if (!wres && !mf) {
      int64_t cap = (int64_t)((kMaxLds - lds) / ((size_t)wt::NWV * wbw));
      if (const char* nr = diag_env("CNMF_WT_NRES")) cap = std::min<int64_t>(cap, atoi(nr));
      nres = (int)std::max<int64_t>(0, std::min<int64_t>(cap, nbt_max));
      lds += (size_t)wt::NWV * nres * wbw;
    }
    const PassFn fn = mf ? mf8_fn(wres != 0, multi, tol) : wt_fn(k, wres != 0, multi, tol);
    if (max_resident(fn, lds) < G) continue;  // the whole grid co-resident (cached query)
    // the share of X kept in the Infinity Cache (the VALU wave tiles): W streams for the tiles past
    // every wave's nres resident ones, read and written once per iteration.  CNMF_WT_KEEP16
    // (diagnostic) overrides the rule.
    int keep16 = 0;
    if (!mf) {
      const int64_t w_tiles = wres ? 0 : std::max<int64_t>(0, n_tiles - (int64_t)nres * wt::NWV * G);
      keep16 = wt_keep16(n_rows * (int64_t)wt::F * 4, 2 * w_tiles * wbw);
      if (const char* kp = diag_env("CNMF_WT_KEEP16")) keep16 = std::min(16, std::max(0, atoi(kp)));
    }
    *out = WtLaunch{fn, G, n_tiles, lds, mf, nres, wres != 0, keep16};
    return true;
  }
  return false;
}
// the first reduction level through the XCD's L2 (PersistArgs::l2rows); CNMF_WT_L2ROWS in the
// diagnostic build overrides the default
static int wt_l2rows() {
  const char* v = diag_env("CNMF_WT_L2ROWS");
  return v ? (atoi(v) != 0) : 0;
}
int launch_wt(const WtLaunch& L, int n_iter, const void* X, void* W, double* H64, double* Ht, double* HHt,
              double* partials, double* stage, uint32_t* counter, double* AB, double l1_W, double l2_W,
              double l1_H, double l2_H, int apply_first, int apply_last, hipStream_t s, uint64_t* xctl,
              double* tolctl) {
  if (int st = check_xw_aligned(X, W)) return st;
  PersistArgs pa = persist_args(X, W, H64, Ht, HHt, partials, stage, counter, AB, L.n_tiles, n_iter, L.G, l1_W, l2_W,
                                l1_H, l2_H, apply_first, apply_last, xctl, tolctl);
  if (const char* gz = diag_env("CNMF_WT_GROUP"))  // diagnostic: workgroups per first-level group
    if (atoi(gz) > 0) pa.n_groups = (int)std::min<int64_t>((L.G + atoi(gz) - 1) / atoi(gz), sl::MAX_GROUPS);
  pa.n_static = L.nres;
  pa.l2rows = L.mf ? 0 : wt_l2rows();
  pa.x_keep16 = L.x_keep16;
  void* args[] = {&pa};
  HIP_CHECK(hipLaunchKernel(L.fn, dim3((unsigned)L.G), dim3(NT), args, L.lds, s));
  return CNMF_OK;
}

#ifdef CNMF_PD_PROBE
// diagnostic (tools/audit_wt_asm.py): the k = 8 streamed-W wave-tile kernel at a
// prefetch depth the product never launches, compiled only to inspect its ISA
template __global__ void mu_iter_wt_kernel<8, false, CNMF_PD_PROBE, false, false>(PersistArgs);
#endif

}  // namespace cnmf
