// wt.hpp — the wave-tile geometry and the device helpers shared by the wave-tile kernels
// (mu_iter_wt_kernel, mu_iter_mf8_kernel, wmu_iter_wt_kernel, als_iter_wt_kernel).
#pragma once

#include "persist.hpp"

namespace cnmf {

namespace wt {
constexpr int F = 81;
constexpr int NWV = 4;                  // waves per workgroup (one per SIMD)
typedef float f2 __attribute__((ext_vector_type(2)));

// geometry of the wave tile for k = KK components: NL = KK lanes per sample (lane l = NL·s + e),
// TSW = 64 / NL samples per tile, NQ features per lane (e owns [NQ·e, NQ·e + NQ); the lanes past F
// hold zero-Hᵀ pads)
template <int KK>
struct Geo {
  static constexpr int K = KK, NL = KK, TSW = 64 / KK, V = F + KK, NOUT = KK * V;
  static constexpr int NQ = (F + KK - 1) / KK;              // 21 (k = 4), 11 (k = 8)
  static constexpr int XBW = TSW * F * 4;                   // 5184 / 2592 B of X per tile
  static constexpr int NCHW = XBW / 16;                     // 324 / 162 chunks
  static constexpr int PFW = (NCHW + 63) / 64;              // 6 / 3 loads per lane
  static constexpr int LASTL = NCHW - 64 * (PFW - 1);       // lanes of the last load: 4 / 34
  // phase 1 reads NQ features from lane e's first one, so the last sample's last lane runs OVR
  // floats past the tile (features >= F, zero Hᵀ): they must be finite — zeros kept in the slot
  static constexpr int OVR = (TSW - 1) * F + NQ * NL - XBW / 4;  // 3 (k = 4), 7 (k = 8)
  static constexpr int PADB = (OVR * 4 + 15) / 16 * 16;          // 16 / 32 zero bytes
  static constexpr int XSTR = XBW + PADB;                        // staging stride
  static constexpr int WBW = TSW * KK * 4;                  // 256 B of W per tile
  static constexpr int NACC = NQ * KK + KK;                 // fp32 accumulators per lane
  // LDS carve (bytes)
  static constexpr int L_STG = 0;                                       // [NWV][XSTR]
  static constexpr int L_WSTG = L_STG + NWV * XSTR;                     // streamed W: [NWV][WBW]
  static constexpr int L_RED = (L_WSTG + NWV * WBW + 15) / 16 * 16;     // [NWV][NL][NACC] fp32
  static constexpr int L_H = (L_RED + NWV * NL * NACC * 4 + 15) / 16 * 16;  // H fp64 [K][F]
  static constexpr int L_AB = L_H + KK * F * 8;                         // AB fp64 [K][V] (+ the loss)
  static constexpr int L_HT = L_AB + (NOUT + 2) * 8;                    // Hᵀ fp32 [NL·NQ][K]
  static constexpr int L_HHT = L_HT + NL * NQ * KK * 4;                 // HHᵀ fp64 [K][K]
  static constexpr int L_FLAG = L_HHT + KK * KK * 8;                    // 8 ints
  static constexpr int L_LOSS = L_FLAG + 32;                            // [NWV] wave loss sums, init, prev
  static constexpr int L_WRES = (L_LOSS + 8 * 8 + 15) / 16 * 16;        // [NWV][nbt_max][WBW]
  static_assert(NCHW * 16 == XBW && XBW % 16 == 0, "tiles are whole 16-byte chunks");
  static_assert(OVR >= 0 && PADB / 4 <= 64, "one zero float per lane covers the overrun");
  static_assert(NOUT <= 3 * NT, "three accumulator outputs per thread at most");
  static_assert(NOUT * 8 >= NWV * 64 * 4, "the prologue's dummy stores stay inside the partial row");
};

template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  const long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xFFFFFFFFll), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// the value of lane l ^ 16 / l ^ 32 (v_permlane16/32_swap: lanes 32-63 of the first operand trade
// with lanes 0-31 of the second, resp. the odd 16-lane rows of the first with the even rows of the
// second; with both operands v, the first result holds l ^ 32 in the upper half / l ^ 16 in the odd
// rows, the second in the lower half / the even rows)
__device__ __forceinline__ double lane_xor16(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const bool odd = (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 16) != 0;
  return __hiloint2double(odd ? (int)b[0] : (int)b[1], odd ? (int)a[0] : (int)a[1]);
}
__device__ __forceinline__ double lane_xor32(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const bool up = (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 32) != 0;
  return __hiloint2double(up ? (int)b[0] : (int)b[1], up ? (int)a[0] : (int)a[1]);
}

// v summed over the lanes l' ≡ l (mod NL) of the wave (every lane gets its class's sum)
template <int NL>
__device__ __forceinline__ float sum_over_samples(float v) {
  if (NL == 4) v += dppf<0x124>(v);  // row_ror:4
  v += dppf<0x128>(v);               // row_ror:8
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);  // + lane ^ 16
  auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r2[0]) + __uint_as_float(r2[1]);  // + lane ^ 32
}

// Reduce-scatter of N per-lane floats over the lanes l' ≡ l (mod NL) (round 6): two permlane swap
// levels halve the values each (permlane32_swap(x, y): the lower half-wave ends with x's pair sum,
// the upper with y's; permlane16_swap likewise for even / odd 16-lane rows) — one swap and one add
// per PAIR of values, where the all-reduce form spends two of each per value — and the samples
// left inside a row are summed by DPP row rotations (ror 4 and 8 at NL = 4, ror 8 at NL = 8).
// On return v[0 .. N/4) of every lane of row r = l / 16 hold the totals of values
// j0 + [0, N/4) with j0 = (N/2)·(r >> 1) + (N/4)·(r & 1) (the same in the row's lanes of one class).
template <int NL, int N>
__device__ __forceinline__ void scatter_over_samples(float (&v)[N]) {
  static_assert(N % 4 == 0 && (NL == 4 || NL == 8), "four quarters of the values, 4 or 8 lanes per sample");
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[j]), __float_as_uint(v[j + N / 2]), false, false);
    v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[j]), __float_as_uint(v[j + N / 4]), false, false);
    v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
    if (NL == 4) v[j] += dppf<0x124>(v[j]);  // row_ror:4
    v[j] += dppf<0x128>(v[j]);               // row_ror:8
  }
}

// v summed over the 16 lanes of its row (every lane gets the row's sum)
__device__ __forceinline__ float sum_over_row16(float v) {
  v += dppf<0x128>(v);  // row_ror:8
  v += dppf<0x124>(v);  // row_ror:4
  v += dppf<0x122>(v);  // row_ror:2
  return v + dppf<0x121>(v);  // row_ror:1
}

// The X (and streamed W) prefetch lives in AGPRs and never touches a VGPR: inline-asm loads into
// AGPR tuples, an asm wait naming them "+a", and asm ds_write_b128 straight from the AGPRs into
// the staging slot (cdna_hip_programming.md §5.7 item 1, form ii).  Two reasons: (1) hipcc's own
// counted waits for compiler-issued loads degrade to vmcnt(0) at this loop's header (one tile in
// flight instead of PD), and (2) under this kernel's VGPR pressure hipcc parks VGPR-resident
// prefetch registers in AGPRs, copying them before the data has landed.  VMEM operations retire
// in issue order, so before staging set k, vmcnt(L·(PD-1)) (L loads per set) leaves exactly the
// PD-1 younger sets in flight; compiler-issued memory operations in between only make it stricter.
#ifdef CNMF_X_PLAIN
#define WT_LD "global_load_dwordx4 %0, %1, off"
#else
#define WT_LD "global_load_dwordx4 %0, %1, off nt"
#endif
__device__ __forceinline__ void ld16(u32x4& r, const unsigned char* p) {
  asm volatile(WT_LD : "=a"(r) : "v"(p) : "memory");
}
// The X loads of one prefetch set (mu_iter_wt_kernel): chunks p + 1024·u (u < C - 1) and plast, with
// the default cache policy when pos < keep (the tile belongs to the share of X kept in the Infinity
// Cache across iterations, PersistArgs::x_keep16), else WT_LD's `nt`.  ONE asm statement holding
// both forms behind a scalar branch: the two forms write the same AGPR tuples, so the compiler sees
// one definition per tuple and has nothing to merge with copies (a copy behind a load that has not
// landed is the stale-tile failure the counted waits exist to prevent).  Either path issues the same
// C loads in the same order; pos and keep are wave-uniform.  The 13-bit offset field ends at 4095:
// the chunk at 4096 takes its own address.
#ifdef CNMF_X_PLAIN
#define WT_LD_ST(d, a, o) "global_load_dwordx4 " d ", " a ", off offset:" o "\n\t"
#else
#define WT_LD_ST(d, a, o) "global_load_dwordx4 " d ", " a ", off offset:" o " nt\n\t"
#endif
#define WT_LD_KP(d, a, o) "global_load_dwordx4 " d ", " a ", off offset:" o "\n\t"
template <int C>
__device__ __forceinline__ void ld_set(u32x4* pf, const unsigned char* p, const unsigned char* plast, int pos,
                                       int keep) {
  if constexpr (C == 6) {
    const unsigned char* p4 = p + 4096;
    asm volatile(
        "s_cmp_lt_u32 %[pos], %[keep]\n\t"
        "s_cbranch_scc0 .Lwt_st%=\n\t"
        WT_LD_KP("%0", "%[p]", "0") WT_LD_KP("%1", "%[p]", "1024") WT_LD_KP("%2", "%[p]", "2048")
        WT_LD_KP("%3", "%[p]", "3072") WT_LD_KP("%4", "%[p4]", "0") WT_LD_KP("%5", "%[pl]", "0")
        "s_branch .Lwt_end%=\n"
        ".Lwt_st%=:\n\t"
        WT_LD_ST("%0", "%[p]", "0") WT_LD_ST("%1", "%[p]", "1024") WT_LD_ST("%2", "%[p]", "2048")
        WT_LD_ST("%3", "%[p]", "3072") WT_LD_ST("%4", "%[p4]", "0") WT_LD_ST("%5", "%[pl]", "0")
        "\n.Lwt_end%=:"
        : "=&a"(pf[0]), "=&a"(pf[1]), "=&a"(pf[2]), "=&a"(pf[3]), "=&a"(pf[4]), "=&a"(pf[5])
        : [p] "v"(p), [p4] "v"(p4), [pl] "v"(plast), [pos] "s"(pos), [keep] "s"(keep)
        : "memory", "scc");
  } else if constexpr (C == 3) {
    asm volatile(
        "s_cmp_lt_u32 %[pos], %[keep]\n\t"
        "s_cbranch_scc0 .Lwt_st%=\n\t"
        WT_LD_KP("%0", "%[p]", "0") WT_LD_KP("%1", "%[p]", "1024") WT_LD_KP("%2", "%[pl]", "0")
        "s_branch .Lwt_end%=\n"
        ".Lwt_st%=:\n\t"
        WT_LD_ST("%0", "%[p]", "0") WT_LD_ST("%1", "%[p]", "1024") WT_LD_ST("%2", "%[pl]", "0")
        "\n.Lwt_end%=:"
        : "=&a"(pf[0]), "=&a"(pf[1]), "=&a"(pf[2])
        : [p] "v"(p), [pl] "v"(plast), [pos] "s"(pos), [keep] "s"(keep)
        : "memory", "scc");
  } else {
    static_assert(C == 3 || C == 6, "X loads per prefetch set");
  }
}
template <int N>
__device__ __forceinline__ void wait_n() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N, int C>
__device__ __forceinline__ void wait_set(u32x4 (&pf)[C]) {
  static_assert(N >= 0 && N <= 63, "s_waitcnt vmcnt is a 6-bit field: a deeper prefetch cannot be counted");
  if constexpr (C == 7)
    asm volatile("s_waitcnt vmcnt(%7)"
                 : "+a"(pf[0]), "+a"(pf[1]), "+a"(pf[2]), "+a"(pf[3]), "+a"(pf[4]), "+a"(pf[5]), "+a"(pf[6])
                 : "n"(N) : "memory");
  else if constexpr (C == 6)
    asm volatile("s_waitcnt vmcnt(%6)"
                 : "+a"(pf[0]), "+a"(pf[1]), "+a"(pf[2]), "+a"(pf[3]), "+a"(pf[4]), "+a"(pf[5])
                 : "n"(N) : "memory");
  else if constexpr (C == 4)
    asm volatile("s_waitcnt vmcnt(%4)" : "+a"(pf[0]), "+a"(pf[1]), "+a"(pf[2]), "+a"(pf[3]) : "n"(N) : "memory");
  else if constexpr (C == 3)
    asm volatile("s_waitcnt vmcnt(%3)" : "+a"(pf[0]), "+a"(pf[1]), "+a"(pf[2]) : "n"(N) : "memory");
  else
    static_assert(C == 3 || C == 4 || C == 6 || C == 7, "prefetch set size");
}
template <int OFF>
__device__ __forceinline__ void st16(unsigned addr, const u32x4& v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "a"(v), "i"(OFF) : "memory");
}
template <int OFF, int U>
__device__ __forceinline__ void stage_rec(unsigned addr, const u32x4* pf) {
  st16<OFF>(addr, pf[0]);
  if constexpr (U > 1) stage_rec<OFF + 1024, U - 1>(addr, pf + 1);
}

// geometry of the k = 8 matrix-core wave tiles (mu_iter_mf8_kernel)
typedef float f4v __attribute__((ext_vector_type(4)));
struct GeoMF8 {
  static constexpr int K = 8, TSW = 16, V = F + 8, NOUT = 8 * V;
  static constexpr int NL = 8, NQ = 11;  // the sHt image wt_derive_basis<8> writes (Geo<8>'s)
  static constexpr int XBW = TSW * F * 4;                  // 5184 B of X per tile
  static constexpr int NCHW = XBW / 16;                    // 324 chunks
  static constexpr int PFW = (NCHW + 63) / 64;             // 6 loads per lane
  static constexpr int LASTL = NCHW - 64 * (PFW - 1);      // 4
  static constexpr int PADB = 16;                          // phase 1 reads 3 floats past the tile
  static constexpr int XSTR = XBW + PADB;
  static constexpr int WBW = TSW * 8 * 4;                  // 512 B of W per tile
  static constexpr int KS1 = 21, NCH1 = 7, NB3 = 6;
  static constexpr int L_STG = 0;                                       // [NWV][XSTR]
  static constexpr int L_WSTG = L_STG + NWV * XSTR;                     // streamed W: [NWV][WBW]
  static constexpr int L_WP = (L_WSTG + NWV * WBW + 15) / 16 * 16;      // W' operand [NWV][16][16] fp32
  static constexpr int L_RED = L_WP + NWV * 16 * 16 * 4;                // [NWV][8][V] fp64
  static constexpr int L_H = L_RED + NWV * 8 * V * 8;                   // H fp64 [8][F]
  static constexpr int L_AB = L_H + 8 * F * 8;                          // AB fp64 (+ the loss)
  static constexpr int L_HT = L_AB + (NOUT + 2) * 8;                    // (wt_derive_basis' Hᵀ image)
  static constexpr int L_HHT = L_HT + NL * NQ * 8 * 4;                  // HHᵀ fp64 [8][8]
  static constexpr int L_FLAG = L_HHT + 8 * 8 * 8;                      // 8 ints
  static constexpr int L_LOSS = L_FLAG + 32;                            // [NWV] wave loss sums, init, prev
  static constexpr int L_WRES = (L_LOSS + 8 * 8 + 15) / 16 * 16;        // [NWV][nbt_max][WBW]
  static_assert(NCHW * 16 == XBW && L_HT % 16 == 0 && L_RED % 16 == 0, "layout");
  static_assert(NOUT * 8 >= NWV * 64 * 4, "the prologue's dummy stores stay inside the partial row");
};
__device__ __forceinline__ f4v mfma4(float a, float b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
}  // namespace wt

// HHᵀ (fp64) from the fp64 H in LDS: NT / K² consecutive threads per entry (16 at k = 4: one DPP row;
// 4 at k = 8: a quad), each a strided part of the F products, then a fixed DPP butterfly over the
// group (xor 1, xor 2 by quad_perm; at 16 the half-row and row mirrors) — register moves where the
// round-5 xor tree went through the LDS crossbar (ds_bpermute, a dependent round trip per level).
// Every entry takes the same operations in the same order, and HHᵀ[j][m] / HHᵀ[m][j] are the same
// products, so it stays exactly symmetric.  Caller synchronises.
template <int KK, class G = wt::Geo<KK>>
__device__ __forceinline__ void wt_hht(unsigned char* smem, int t) {
  const double* sH = reinterpret_cast<const double*>(smem + G::L_H);
  double* sHHt = reinterpret_cast<double*>(smem + G::L_HHT);
  constexpr int NE = KK * KK, TPE = NT / NE;
  static_assert(TPE * NE == NT && (TPE == 4 || TPE == 16), "threads per HHᵀ entry: a quad or a DPP row");
  const int en = t / TPE, part = t - en * TPE;
  const int j = en / KK, m = en - (en / KK) * KK;
  // the strided products with a compile-time trip count: every LDS read of the row pair issued
  // before the first FMA (a runtime loop waited on each iteration's reads in turn)
  constexpr int NF = (wt::F + TPE - 1) / TPE;
  double hj[NF], hm[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int f = part + TPE * i < wt::F ? part + TPE * i : wt::F - 1;
    hj[i] = sH[j * wt::F + f];
    hm[i] = sH[m * wt::F + f];
  }
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < NF; ++i)
    if (part + TPE * i < wt::F) v = fma(hj[i], hm[i], v);
  v += wt::dpp64<0xB1>(v);  // quad_perm [1,0,3,2]
  v += wt::dpp64<0x4E>(v);  // quad_perm [2,3,0,1]
  if constexpr (TPE == 16) {
    v += wt::dpp64<0x141>(v);  // row_half_mirror: the other quad of the half-row
    v += wt::dpp64<0x140>(v);  // row_mirror: the other half-row
  }
  if (part == 0) sHHt[en] = v;
}
// Hᵀ (fp32, the lanes' feature blocks, rows >= F zero) and HHᵀ from the fp64 H in LDS — sl_derive_basis
// for k = KK
template <int KK, class G = wt::Geo<KK>>
__device__ __forceinline__ void wt_derive_basis(unsigned char* smem, int t) {
  const double* sH = reinterpret_cast<const double*>(smem + G::L_H);
  float* sHt = reinterpret_cast<float*>(smem + G::L_HT);
  for (int e = t; e < G::NL * G::NQ * KK; e += NT) {
    const int f = e / KK;
    const int j = e - f * KK;
    sHt[e] = f < wt::F ? (float)sH[j * wt::F + f] : 0.f;
  }
  wt_hht<KK, G>(smem, t);
  __syncthreads();
}
// H <- H·(WᵀX / ((WᵀW)·H (+l1)(+l2·H))) on the fp64 H in LDS from AB in LDS (SK:634-728) —
// sl_update_basis for k = KK.  Round 6: the quotient as div_nr (v_rcp_f64 + one Newton step, the
// W-update's arithmetic) and the new Hᵀ written with the new H (its pad rows stay zero), then HHᵀ
template <int KK, class G = wt::Geo<KK>>
__device__ __forceinline__ void wt_update_basis(unsigned char* smem, int t, double l1, double l2) {
  constexpr int KF = KK * wt::F;
  constexpr int U = (KF + NT - 1) / NT;
  double* sH = reinterpret_cast<double*>(smem + G::L_H);
  float* sHt = reinterpret_cast<float*>(smem + G::L_HT);
  const double* sAB = reinterpret_cast<const double*>(smem + G::L_AB);
  double hn[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = t + NT * u;
    hn[u] = 0.0;
    if (e < KF) {
      const int j = e / wt::F;
      const int f = e - j * wt::F;
      const double h = sH[e];
      const double num = sAB[j * G::V + f];                                      // (WᵀX)[j][f], SK:639
      double den = 0.0;                                                          // ((WᵀW)·H)[j][f], SK:640
      for (int m = 0; m < KK; ++m) den = fma(sAB[j * G::V + wt::F + m], sH[m * wt::F + f], den);
      if (l1 > 0.0) den += l1;                                                   // SK:702-703
      if (l2 > 0.0) den = den + l2 * h;                                          // SK:704-705
      if (den == 0.0) den = EPS32;                                               // SK:706
      hn[u] = h * div_nr(num, den);                                              // SK:722-726
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = t + NT * u;
    if (e < KF) {
      const int j = e / wt::F;
      const int f = e - j * wt::F;
      sH[e] = hn[u];
      sHt[f * KK + j] = (float)hn[u];
    }
  }
  // Hᵀ's pad rows (features >= F, read by the lanes past F): zero (a launch that starts with the
  // pending update, apply_first, has not run wt_derive_basis)
  for (int e = wt::F * KK + t; e < G::NL * G::NQ * KK; e += NT) sHt[e] = 0.f;
  __syncthreads();
  wt_hht<KK, G>(smem, t);
  __syncthreads();
}

// The round-5 forms of wt_derive_basis / wt_update_basis (xor-shuffle HHᵀ tree, IEEE division), kept
// for k = 8: the round-6 end of iteration measured 3.5 % slower on cfg3's k = 8 shard (the streaming
// body's schedule, not the tail; profiles/r06/tree/), so that kernel keeps the round-5 tail.
// Hᵀ (fp32, the lanes' feature blocks, rows >= F zero) and HHᵀ (fp64; lanes over f, fixed shuffle
// tree) from the fp64 H in LDS — sl_derive_basis for k = KK
template <int KK, class G = wt::Geo<KK>>
__device__ __forceinline__ void wt_derive_basis_r5(unsigned char* smem, int t) {
  const double* sH = reinterpret_cast<const double*>(smem + G::L_H);
  float* sHt = reinterpret_cast<float*>(smem + G::L_HT);
  double* sHHt = reinterpret_cast<double*>(smem + G::L_HHT);
  for (int e = t; e < G::NL * G::NQ * KK; e += NT) {
    const int f = e / KK;
    const int j = e - f * KK;
    sHt[e] = f < wt::F ? (float)sH[j * wt::F + f] : 0.f;
  }
  // HHᵀ: NT / K² consecutive threads per entry (16 at k = 4, 4 at k = 8), each a strided part of the
  // F products, then a fixed xor tree over the group (every entry in the same order; HHᵀ[j][m] and
  // HHᵀ[m][j] are the same products, so it stays exactly symmetric)
  constexpr int NE = KK * KK, TPE = NT / NE;
  static_assert(TPE * NE == NT && (TPE & (TPE - 1)) == 0, "threads per HHᵀ entry: a power of two");
  const int en = t / TPE, part = t - en * TPE;
  const int j = en / KK, m = en - (en / KK) * KK;
  double v = 0.0;
  for (int f = part; f < wt::F; f += TPE) v = fma(sH[j * wt::F + f], sH[m * wt::F + f], v);
#pragma unroll
  for (int o = TPE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (part == 0) sHHt[en] = v;
  __syncthreads();
}
// H <- H·(WᵀX / ((WᵀW)·H (+l1)(+l2·H))) on the fp64 H in LDS from AB in LDS (SK:634-728) —
// sl_update_basis for k = KK
template <int KK, class G = wt::Geo<KK>>
__device__ __forceinline__ void wt_update_basis_r5(unsigned char* smem, int t, double l1, double l2) {
  constexpr int KF = KK * wt::F;
  constexpr int U = (KF + NT - 1) / NT;
  double* sH = reinterpret_cast<double*>(smem + G::L_H);
  const double* sAB = reinterpret_cast<const double*>(smem + G::L_AB);
  double hn[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = t + NT * u;
    hn[u] = 0.0;
    if (e < KF) {
      const int j = e / wt::F;
      const int f = e - j * wt::F;
      const double h = sH[e];
      const double num = sAB[j * G::V + f];                                      // (WᵀX)[j][f], SK:639
      double den = 0.0;                                                          // ((WᵀW)·H)[j][f], SK:640
      for (int m = 0; m < KK; ++m) den = fma(sAB[j * G::V + wt::F + m], sH[m * wt::F + f], den);
      if (l1 > 0.0) den += l1;                                                   // SK:702-703
      if (l2 > 0.0) den = den + l2 * h;                                          // SK:704-705
      if (den == 0.0) den = EPS32;                                               // SK:706
      hn[u] = h * (num / den);                                                   // SK:722-726
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (t + NT * u < KF) sH[t + NT * u] = hn[u];
  __syncthreads();
  wt_derive_basis_r5<KK, G>(smem, t);
}

// TOL: the tolerance test of SK:872-884 on the device.  In iteration g + 1 (g = it0 + it, g % 10 ==
// 0) each lane also accumulates ‖x − w·H‖² of the state AFTER g iterations (x, the old w and H are
// all in registers then: fp32 residual per element, fp64 sums per tile), carried as one more
// column of the partial rows (NOUT + 1) and reduced / exchanged with [WᵀX | WᵀW]; the top combiner
// applies the relative-decrease test.  On a stop it publishes the flag with FLAG_STOP and every
// workgroup leaves with the state after g iterations: H (not updated), W as it was before this
// iteration's update — written to W itself in the loss iterations when W is resident in LDS, else to
// the snapshot buffer (TC_WSNAP; the host copies it) — so n_iter = g as in sklearn.

}  // namespace cnmf
