// host.hpp — the host helpers one file of the library calls in another: the occupancy-derived
// residency, the wave-tile plan and launch, and the checks the entry points share.  A kernel is named
// (and so instantiated) only in its family's file; everything here passes kernels as PassFn.
#pragma once

#include "common.hpp"

namespace cnmf {

using PassFn = const void*;

constexpr size_t kMaxLds = 160 * 1024;

CNMF_LOCAL inline int check_xw_aligned(const void* X, const void* W) {
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(W) & 15))
    return set_err(CNMF_ERR_ALIGN, "X and W must be 16-byte aligned");
  return CNMF_OK;
}

// launch() between the optional event pair (events[0], events[1]) of a timed persistent launch
template <class Launch>
CNMF_LOCAL int with_events(void* const* events, int n_events, hipStream_t hs, Launch launch) {
  if (events && n_events >= 2) HIP_CHECK(hipEventRecord(reinterpret_cast<hipEvent_t>(events[0]), hs));
  if (const int st = launch()) return st;
  if (events && n_events >= 2) HIP_CHECK(hipEventRecord(reinterpret_cast<hipEvent_t>(events[1]), hs));
  return CNMF_OK;
}

// ---- cnmf_hip.hip
CNMF_LOCAL int64_t max_resident(PassFn fn, size_t lds);  // co-resident workgroups (cached), < 0 on error
CNMF_LOCAL int device_cus();                             // compute units of the current device
CNMF_LOCAL PassFn mf8_fn(bool wres, bool multi, bool tol);  // mu_iter_mf8_kernel (diagnostic build), else null

// ---- wt.hip
struct WtLaunch {
  PassFn fn;
  int64_t G, n_tiles;
  size_t lds;
  bool mf;       // k = 8 on the matrix cores (mu_iter_mf8_kernel)
  int nres = 0;  // W streamed: the first nres tiles of every wave resident in the LDS left over
  bool wres = false;  // W resident (every tile)
  int x_keep16 = 0;   // sixteenths of X kept in the Infinity Cache across iterations (csrc/keep.hpp)
};
CNMF_LOCAL int wt_pd(int k, bool wres, bool multi);
CNMF_LOCAL bool wt_plan(int64_t n_rows, int x_dtype, int F, int k, bool multi, int layout, WtLaunch* out,
                        bool tol = false);
CNMF_LOCAL int launch_wt(const WtLaunch& L, int n_iter, const void* X, void* W, double* H64, double* Ht, double* HHt,
                         double* partials, double* stage, uint32_t* counter, double* AB, double l1_W, double l2_W,
                         double l1_H, double l2_H, int apply_first, int apply_last, hipStream_t s, uint64_t* xctl,
                         double* tolctl = nullptr);

}  // namespace cnmf
