// common.hpp — what every family file of the kernel library shares: constants, error reporting,
// the diagnostic-environment switch, the element types and the diagnostic stamp macros.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "cnmf_hip.h"

// host helpers and state shared between the library's objects: not symbols of the shared library
#define CNMF_LOCAL __attribute__((visibility("hidden")))

namespace cnmf {

constexpr int TS = 64;       // samples per tile
constexpr int NT = 256;      // threads per workgroup
constexpr int NWAVE = NT / 64;
constexpr int PF = 8;        // 16-byte chunks per thread held in registers for the next tile
constexpr int NSLICE = 64;   // max slices of the deterministic cross-block reduction
constexpr int RED_NT = 256;  // threads of the reduce / update workgroups
constexpr double EPS32 = 1.1920928955078125e-07;  // np.finfo(np.float32).eps, SK:39
constexpr int ALS_TAB = 16 * 16 + 16;  // constrained-ALS passive-set table: 16 masks x 4x4 + valid

extern CNMF_LOCAL thread_local char g_err[512];  // one definition: cnmf_hip.hip

CNMF_LOCAL inline int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// Diagnostic switches (A/B timing and tools/ probes) are read from the environment only in the
// diagnostic build (-DCNMF_DIAG: python -m cnmf_amd.build --diag); the product library ignores the
// environment, so every plan's behaviour follows from its arguments alone.
CNMF_LOCAL inline const char* diag_env(const char* name) {
#ifdef CNMF_DIAG
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

#define HIP_CHECK(expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return set_err(CNMF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
  } while (0)

// ------------------------------------------------------------------------------------------------
// element conversions: X storage type -> compute type
// ------------------------------------------------------------------------------------------------
struct bf16_t {
  uint16_t bits;
};

// native 16-byte vector (HIP's uint4 class type defeats SROA: the prefetch array went to scratch)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float to_c(float v) { return v; }
__device__ __forceinline__ double to_c(double v) { return v; }
__device__ __forceinline__ float to_c(bf16_t v) { return __uint_as_float(((uint32_t)v.bits) << 16); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------------------------------------
// Diagnostic phase stamps (built only with -DCNMF_STAMPS into a separate .so; never in the real
// kernel): per wave, s_memtime deltas between the phase boundaries of every tile are summed in
// registers and added once per wave into g_stamps[slot] (MI355X guide §7 "In-kernel stamps").
// ------------------------------------------------------------------------------------------------
#ifdef CNMF_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long st_t0 = 0;
#define STAMP(slot)                                                                   \
  do {                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                \
    unsigned long long st_t;                                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t) :: "memory");    \
    __builtin_amdgcn_sched_barrier(0);                                                \
    if (slot > 0) st_acc[slot] += st_t - st_t0;                                       \
    st_t0 = st_t;                                                                     \
  } while (0)
#define STAMP_FLUSH                                                                   \
  do {                                                                                \
    if ((threadIdx.x & 63) == 0)                                                      \
      for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_stamps[i_], st_acc[i_]);           \
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_stamps[8], 1ull);                       \
  } while (0)
// the end of a persistent bfw iteration: thread 0 of every workgroup sums the phase durations
// (s_memtime) into g_eoi[slot]; g_eoi[15] counts the (workgroup, iteration) pairs
__device__ unsigned long long g_eoi[16];
// the persistent ALS resume path of workgroup 0: per slot the sum over iterations of the
// s_memrealtime stamp (differences of the sums = summed phase durations); g_ph[15] counts
__device__ unsigned long long g_ph[16];
#define PH(slot)                                                                        \
  do {                                                                                  \
    if (threadIdx.x == 0 && blockIdx.x == 0) {                                          \
      g_ph[slot] += __builtin_amdgcn_s_memrealtime();                                   \
      if (slot == 0) g_ph[15] += 1ull;                                                  \
    }                                                                                   \
  } while (0)
#define EOI_DECL unsigned long long eoi_t0 = 0;
#define EOI(slot)                                                                     \
  do {                                                                                \
    if (threadIdx.x == 0) {                                                           \
      unsigned long long st_t;                                                        \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t) :: "memory");  \
      if (slot > 0) atomicAdd(&g_eoi[slot], st_t - eoi_t0);                           \
      else atomicAdd(&g_eoi[15], 1ull);                                               \
      eoi_t0 = st_t;                                                                  \
    }                                                                                 \
  } while (0)
#else
#define STAMP_DECL
#define STAMP(slot) do {} while (0)
#define STAMP_FLUSH do {} while (0)
#define EOI_DECL
#define EOI(slot) do {} while (0)
#define PH(slot) do {} while (0)
#endif

}  // namespace cnmf
