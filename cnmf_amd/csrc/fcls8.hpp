// fcls8.hpp — the constrained-ALS W-step for 5 <= k <= 8 (padded to 8): per sample the exact
//   w = argmin_{w >= 0} ½wᵀQw − cᵀw,  Q = HHᵀ + δ²11ᵀ,  c = Hx + δ²1      (oracle/als_ref.py fcls_w)
// by block principal pivoting on the Gram form (Kim & Park 2011; Júdice & Pires' backup rule), fp64.
// 2^k passive sets cannot be tabulated as for k <= 4 (als_table), so every sample runs its own
// active-set iteration.  Device code only; no kernel of its own (the pass kernel that
// inlines it is named in cnmf_hip.hip alone), so it can move into a persistent kernel unchanged.
//
// Layout: the four lanes of a quad share one sample (the quad of phase12: lane & 3 = qtr).  Lane qtr
// holds rows qtr and qtr + 4 of the 8x9 augmented system [Q_PP | c_P], rows and columns outside the
// passive set P held at the identity.  The solve is Gauss-Jordan over the full 8x8 without row
// exchanges (Q_PP is symmetric positive definite, so are its Schur complements: every pivot is the
// diagonal entry): every register index is a compile-time constant, the matrix never leaves the
// registers, and the pivot row reaches the quad by DPP quad_perm broadcasts.  One lane per sample
// with the whole 8x9 system would hold 72 fp64 registers where this holds 18 per lane.
#pragma once

#include "wt.hpp"

namespace cnmf {
namespace fcls8 {

constexpr int KP = 8;
// a pivot <= PIVOT_REL · (largest diagonal of Q_PP) pins its variable at zero for this sample (the
// validity threshold of the k <= 4 table): an all-zero basis row gives w_j = 0 at δ = 0, as scipy does
constexpr double PIVOT_REL = 1e-13;
// full exchanges allowed in a row without the infeasible count falling, before the backup rule
constexpr int FULL_BUDGET = 3;
// Trip bound of the exchange loop.  Termination: a full exchange is taken only while the infeasible
// count falls below its best so far (at most KP times) or FULL_BUDGET more times after each such
// fall; otherwise only the highest-index infeasible variable is exchanged — Murty's rule, which for a
// positive definite Q visits no passive set twice, so a run of single exchanges ends within 2^KP
// steps with a smaller count or none.  The loop therefore ends by itself in exact arithmetic; the
// bound (one run of 2^KP single exchanges plus every full exchange) makes it end in any case (a
// rounding-level tie between a tiny negative w_j and a tiny negative dual could otherwise swap one
// index for ever; the clamped result is then within rounding of the minimiser).  Mixtures with noise
// take 2-4 trips warm, one more from the empty set.
constexpr int MAX_TRIPS = (1 << KP) + (FULL_BUDGET + 1) * KP;

template <int I>
__device__ __forceinline__ double quad_bcast(double v) {  // lane I of the quad to its four lanes
  return wt::dpp64<I * 0x55>(v);
}
__device__ __forceinline__ double quad_max(double v) {
  v = fmax(v, wt::dpp64<0xB1>(v));  // quad_perm [1,0,3,2]
  return fmax(v, wt::dpp64<0x4E>(v));  // quad_perm [2,3,0,1]
}
__device__ __forceinline__ unsigned quad_or(unsigned v) {
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
  return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
}

// One Gauss-Jordan step on column C (its pivot row: slot C / 4 of lane C % 4).  A column outside P is
// an identity column: nothing to do.  A pivot at or under thr takes C out of P and out of `allowed`
// for this sample; rows and columns before C never used it, so the rest of the elimination is that of
// the system without C.
// The pivot row is left unscaled (its diagonal stays the pivot: the later steps clear column C in no
// other pivot row's favour), so the row's owner keeps 1 / pivot in ri[] for the final w = rhs / pivot.
template <int C>
__device__ __forceinline__ void gj_step(double (&a)[2][KP + 1], double (&ri)[2], int qtr, unsigned& P,
                                        unsigned& allowed, double thr) {
  constexpr int SL = C >> 2, OW = C & 3;
  const double piv = quad_bcast<OW>(a[SL][C]);
  const bool in_p = (P >> C & 1u) != 0u;
  const bool act = in_p && piv > thr;
  if (in_p && !act) {
    P &= ~(1u << C);
    allowed &= ~(1u << C);
  }
  // 1 / pivot: v_rcp_f64 refined by two Newton steps (full fp64 accuracy; the pivot is positive)
  double inv = __builtin_amdgcn_rcp(piv);
  inv = fma(inv, fma(-piv, inv, 1.0), inv);
  inv = fma(inv, fma(-piv, inv, 1.0), inv);
  inv = act ? inv : 0.0;
  const bool own = qtr == OW;
  ri[SL] = (act && own) ? inv : ri[SL];
  // the multipliers of this lane's two rows (0 for the pivot row itself and for an idle step)
  const double f0 = (own && SL == 0) ? 0.0 : a[0][C] * inv;
  const double f1 = (own && SL == 1) ? 0.0 : a[1][C] * inv;
#pragma unroll
  for (int e = C + 1; e <= KP; ++e) {
    const double pr = quad_bcast<OW>(a[SL][e]);  // the pivot row
    a[0][e] = fma(-f0, pr, a[0][e]);
    a[1][e] = fma(-f1, pr, a[1][e]);
  }
}

// The minimiser's components qtr and qtr + 4 of one sample (wm, not yet clamped).
//   cq[s]  c_j of row j = qtr + 4s (0 for j >= k)
//   sQ     Q in LDS, [8][8], zero rows / columns >= k
//   P0     the start set (any subset of the k components: the answer does not depend on it beyond
//          rounding; the old W's support is a warm start)
// Quad-uniform: P0, k; every lane of the wave must call it (DPP, one ballot per trip).
__device__ __forceinline__ void solve_quad(const double (&cq)[2], const double* __restrict__ sQ, unsigned P0,
                                           int k, int qtr, double (&wm)[2]) {
  unsigned allowed = (1u << k) - 1u;  // components k..7 of the padded system are never in P
  unsigned P = P0 & allowed;
  int alpha = FULL_BUDGET, beta = KP + 1;
  const int r0 = qtr, r1 = qtr + 4;
  wm[0] = 0.0;
  wm[1] = 0.0;
  // bound: MAX_TRIPS (compile time); ends earlier once no quad of the wave has an infeasible index —
  // the argument is at MAX_TRIPS above.  A finished quad repeats its last solve (same P, same bits).
#pragma unroll 1
  for (int trip = 0; trip < MAX_TRIPS; ++trip) {
    const bool in0 = (P >> r0 & 1u) != 0u, in1 = (P >> r1 & 1u) != 0u;
    double q[2][KP];
    double a[2][KP + 1];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      q[0][c] = sQ[r0 * KP + c];
      q[1][c] = sQ[r1 * KP + c];
      const bool inc = (P >> c & 1u) != 0u;
      a[0][c] = (in0 && inc) ? q[0][c] : (r0 == c ? 1.0 : 0.0);
      a[1][c] = (in1 && inc) ? q[1][c] : (r1 == c ? 1.0 : 0.0);
    }
    a[0][KP] = in0 ? cq[0] : 0.0;
    a[1][KP] = in1 ? cq[1] : 0.0;
    double ri[2] = {0.0, 0.0};
    const double thr = PIVOT_REL * quad_max(fmax(in0 ? sQ[r0 * KP + r0] : 0.0, in1 ? sQ[r1 * KP + r1] : 0.0));
    gj_step<0>(a, ri, qtr, P, allowed, thr);
    gj_step<1>(a, ri, qtr, P, allowed, thr);
    gj_step<2>(a, ri, qtr, P, allowed, thr);
    gj_step<3>(a, ri, qtr, P, allowed, thr);
    gj_step<4>(a, ri, qtr, P, allowed, thr);
    gj_step<5>(a, ri, qtr, P, allowed, thr);
    gj_step<6>(a, ri, qtr, P, allowed, thr);
    gj_step<7>(a, ri, qtr, P, allowed, thr);
    // w_P (a pinned variable has left P), zeros elsewhere; all eight to every lane for the duals
    const bool p0 = (P >> r0 & 1u) != 0u, p1 = (P >> r1 & 1u) != 0u;
    wm[0] = p0 ? a[0][KP] * ri[0] : 0.0;
    wm[1] = p1 ? a[1][KP] * ri[1] : 0.0;
    const double w8[KP] = {quad_bcast<0>(wm[0]), quad_bcast<1>(wm[0]), quad_bcast<2>(wm[0]), quad_bcast<3>(wm[0]),
                           quad_bcast<0>(wm[1]), quad_bcast<1>(wm[1]), quad_bcast<2>(wm[1]), quad_bcast<3>(wm[1])};
    // y_N = Q_NP w_P − c_N (w is zero off P)
    double y0 = -cq[0], y1 = -cq[1];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      y0 = fma(q[0][c], w8[c], y0);
      y1 = fma(q[1][c], w8[c], y1);
    }
    const bool bad0 = p0 ? wm[0] < 0.0 : ((allowed >> r0 & 1u) != 0u && y0 < 0.0);
    const bool bad1 = p1 ? wm[1] < 0.0 : ((allowed >> r1 & 1u) != 0u && y1 < 0.0);
    const unsigned bad = quad_or((bad0 ? 1u << r0 : 0u) | (bad1 ? 1u << r1 : 0u));
    const int ninf = __popc(bad);
    unsigned flip = bad;  // exchange every infeasible index
    if (ninf < beta) {
      beta = ninf;
      alpha = FULL_BUDGET;
    } else if (alpha >= 1) {
      --alpha;
    } else {
      flip = bad ? 1u << (31 - __clz((int)bad)) : 0u;  // the backup rule: the highest infeasible index alone
    }
    if (__ballot(ninf != 0) == 0ull) break;
    P ^= ninf != 0 ? flip : 0u;
  }
}

}  // namespace fcls8
}  // namespace cnmf
