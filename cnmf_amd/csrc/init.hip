// init.hip — GPU NNDSVD initialisation: the ig_* kernels and the cnmf_init_* entry points.
#include "common.hpp"
#include "host.hpp"

namespace cnmf {

// ------------------------------------------------------------------------------------------------
// GPU NNDSVD initialisation (sklearn's _initialize_nmf SK:317-373 over
// randomized_svd, extmath.py:530-604).  sklearn's range finder alternates Q <- lu(X·Q),
// Q <- lu(Xᵀ·Q): only span(Q) matters to the result (U, s, Vt are invariant under an orthonormal
// change of basis of the range; svd_flip fixes the signs), and span(Xᵀ·X·Q) needs only the F × F
// Gram matrix C = XᵀX.  So the device does the work that scales with N:
//   ig_gram_kernel    C = XᵀX and the column sums of X (fp64, per-workgroup partial rows, reduced by
//                     cnmf_reduce_partials) — one pass over X;
//   ig_xm_kernel      U = X·M (M = F × k from the small host algebra), fp64 — one pass over X;
//   ig_stats_kernel   per column of U: Σ max(u,0)², Σ min(u,0)², and the first entry of largest |u|
//                     (svd_flip's u-based sign) — per-workgroup rows;
//   ig_fill_kernel    W from U: sqrt(S0)|u| (j = 0) or lbd·part(sign·u)/‖part‖, < eps -> 0, and the
//                     nndsvda fill — in X's dtype;
// while the host does sklearn's F × r / r × r algebra in fp64 (cnmf_amd/gpu_init.py).
// ------------------------------------------------------------------------------------------------
namespace ig {
constexpr int FP = 96;   // features padded (F <= 96)
constexpr int GT = 64;   // rows per staged tile
constexpr int KMAX = 16;
}  // namespace ig

// C = XᵀX (F × F) and colsum (F) of this workgroup's rows [r0, r1): thread (a, c) owns C rows
// 3a..3a+2 × columns 12c..12c+11 (fp64 registers); the tile is staged in LDS as fp64 [GT][FP].
// Output row: [F·F | F].
template <typename TX>
__global__ __launch_bounds__(256) void ig_gram_kernel(const TX* __restrict__ X, int64_t n_rows, int F,
                                                      int64_t rows_per_block, double* __restrict__ partials) {
  using namespace ig;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* tile = reinterpret_cast<double*>(smem);  // [GT][FP]
  const int t = threadIdx.x;
  const int a = t >> 3, c = t & 7;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
  double acc[3][12], cs[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cs[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[i][j] = 0.0;
  }
  for (int64_t rt = r0; rt < r1; rt += GT) {
    const int nr = (int)(r1 - rt < GT ? r1 - rt : GT);
    __syncthreads();
    for (int e = t; e < GT * FP; e += 256) {
      const int r = e / FP, f = e - r * FP;
      tile[e] = (r < nr && f < F) ? (double)to_c(*(X + (rt + r) * F + f)) : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double* row = tile + r * FP;
      double xa[3], xb[12];
#pragma unroll
      for (int i = 0; i < 3; ++i) xa[i] = row[3 * a + i];
#pragma unroll
      for (int j = 0; j < 12; ++j) xb[j] = row[12 * c + j];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[i][j] = fma(xa[i], xb[j], acc[i][j]);
        cs[i] += xa[i];
      }
    }
  }
  double* prow = partials + (size_t)blockIdx.x * (F * F + F);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int fi = 3 * a + i;
    if (fi >= F) continue;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const int fj = 12 * c + j;
      if (fj < F) prow[fi * F + fj] = acc[i][j];
    }
    if (c == 0) prow[F * F + fi] = cs[i];
  }
}

// U[n][j] = Σ_f X[n][f]·M[f][j] (fp64), k <= 16: thread = (row of the tile, component group)
template <typename TX>
__global__ __launch_bounds__(256) void ig_xm_kernel(const TX* __restrict__ X, int64_t n_rows, int F, int k,
                                                    const double* __restrict__ M, double* __restrict__ U) {
  using namespace ig;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sM = reinterpret_cast<double*>(smem);  // [F][k]
  float* tile = reinterpret_cast<float*>(smem + (size_t)FP * KMAX * 8);  // [GT][F + 1] (fp32 copy; exact for f32/bf16)
  double* tile64 = reinterpret_cast<double*>(smem + (size_t)FP * KMAX * 8);  // f64 X: [GT][F + 1]
  const int t = threadIdx.x;
  for (int e = t; e < F * k; e += 256) sM[e] = M[e];
  const int r = t & (GT - 1), jg = t >> 6;  // 4 component groups: j = jg, jg + 4, ...
  const int64_t n_tiles = (n_rows + GT - 1) / GT;
  for (int64_t tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
    const int64_t row0 = tb * GT;
    const int nr = (int)(n_rows - row0 < GT ? n_rows - row0 : GT);
    __syncthreads();
    for (int e = t; e < nr * F; e += 256) {
      const int rr = e / F, f = e - rr * F;
      if (std::is_same<TX, double>::value)
        tile64[rr * (F + 1) + f] = (double)to_c(*(X + row0 * F + e));
      else
        tile[rr * (F + 1) + f] = (float)to_c(*(X + row0 * F + e));
    }
    __syncthreads();
    if (r < nr) {
      for (int j = jg; j < k; j += 4) {
        double u = 0.0;
        for (int f = 0; f < F; ++f) {
          const double x = std::is_same<TX, double>::value ? tile64[r * (F + 1) + f] : (double)tile[r * (F + 1) + f];
          u = fma(x, sM[f * k + j], u);
        }
        U[(row0 + r) * k + j] = u;
      }
    }
  }
}

// per column j of U (N × k fp64) over this workgroup's rows: [Σ max(u,0)², Σ min(u,0)², max|u|,
// the u at the first row attaining it, that row] — 5 doubles per column
__global__ __launch_bounds__(256) void ig_stats_kernel(const double* __restrict__ U, int64_t n_rows, int k,
                                                       int64_t rows_per_block, double* __restrict__ out) {
  __shared__ double red[256][5];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
  for (int j = 0; j < k; ++j) {
    double sp = 0.0, sn = 0.0, mx = -1.0, mv = 0.0, mi = 0.0;
    for (int64_t r = r0 + t; r < r1; r += 256) {  // rows ascending per thread: first max kept
      const double u = U[r * k + j];
      if (u > 0.0) sp = fma(u, u, sp);
      if (u < 0.0) sn = fma(u, u, sn);
      if (fabs(u) > mx) {
        mx = fabs(u);
        mv = u;
        mi = (double)r;
      }
    }
    red[t][0] = sp;
    red[t][1] = sn;
    red[t][2] = mx;
    red[t][3] = mv;
    red[t][4] = mi;
    __syncthreads();
    if (t == 0) {  // fixed order; ties on |u|: the lowest row (np.argmax's first occurrence)
      double a0 = 0.0, a1 = 0.0, bm = -1.0, bv = 0.0, bi = 0.0;
      for (int i = 0; i < 256; ++i) {
        a0 += red[i][0];
        a1 += red[i][1];
        if (red[i][2] > bm || (red[i][2] == bm && red[i][4] < bi)) {
          bm = red[i][2];
          bv = red[i][3];
          bi = red[i][4];
        }
      }
      double* o = out + ((size_t)blockIdx.x * k + j) * 5;
      o[0] = a0;
      o[1] = a1;
      o[2] = bm;
      o[3] = bv;
      o[4] = bi;
    }
    __syncthreads();
  }
}

// W[n][j] from U[n][j]: v = coef_j · part_j(sign_j · u) with part 0 = |u|, 1 = max(u,0), 2 = |min(u,0)|;
// v < eps -> 0; then v == 0 -> fill (nndsvda: X.mean(); nndsvd / nndsvdar: 0)
template <typename TW>
__global__ __launch_bounds__(256) void ig_fill_kernel(const double* __restrict__ U, int64_t n, int k,
                                                      const double* __restrict__ coef, const int* __restrict__ part,
                                                      const double* __restrict__ sgn, double eps, double fill,
                                                      TW* __restrict__ W) {
  const int64_t total = n * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % k);
    const double u = sgn[j] * U[e];
    const int pj = part[j];
    const double p = pj == 0 ? fabs(u) : (pj == 1 ? (u > 0.0 ? u : 0.0) : (u < 0.0 ? -u : 0.0));
    double v = pj == 0 ? coef[j] * p : p * coef[j];
    if (v < eps) v = 0.0;
    if (v == 0.0) v = fill;
    W[e] = (TW)v;
  }
}

}  // namespace cnmf

using namespace cnmf;

extern "C" {

// ---- GPU NNDSVD initialisation; see ig_gram_kernel
static int ig_blocks(int64_t n_rows) {
  const int ncu = device_cus();
  const int64_t want = (n_rows + 4095) / 4096;  // >= 4096 rows (64 tiles) per workgroup
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, 2 * (int64_t)std::max(ncu, 1)), 1024));
}
int64_t cnmf_init_gram_rows(int64_t n_rows) { return n_rows > 0 ? ig_blocks(n_rows) : 0; }

int cnmf_init_gram(const void* X, int x_dtype, int64_t n_rows, int n_features, double* partials,
                   int64_t n_parts, void* stream) {
  if (!X || !partials) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (n_rows < 1 || n_features < 1 || n_features > ig::FP)
    return set_err(CNMF_ERR_UNSUPPORTED, "GPU init: n_features=%d (1..%d), n_rows=%lld", n_features, ig::FP, (long long)n_rows);
  const int G = ig_blocks(n_rows);
  if (G > n_parts) return set_err(CNMF_ERR_ARG, "partials hold %lld rows, the pass needs %d", (long long)n_parts, G);
  const int64_t rpb = (n_rows + G - 1) / G;
  const size_t lds = (size_t)ig::GT * ig::FP * 8;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  switch (x_dtype) {
    case CNMF_F32: hipLaunchKernelGGL(ig_gram_kernel<float>, dim3(G), dim3(256), lds, hs, static_cast<const float*>(X), n_rows, n_features, rpb, partials); break;
    case CNMF_F64: hipLaunchKernelGGL(ig_gram_kernel<double>, dim3(G), dim3(256), lds, hs, static_cast<const double*>(X), n_rows, n_features, rpb, partials); break;
    case CNMF_BF16: hipLaunchKernelGGL(ig_gram_kernel<bf16_t>, dim3(G), dim3(256), lds, hs, static_cast<const bf16_t*>(X), n_rows, n_features, rpb, partials); break;
    default: return set_err(CNMF_ERR_ARG, "x_dtype %d", x_dtype);
  }
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

int cnmf_init_xm(const void* X, int x_dtype, int64_t n_rows, int n_features, int k, const double* M, double* U,
                 void* stream) {
  if (!X || !M || !U) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (n_rows < 1 || n_features < 1 || n_features > ig::FP || k < 1 || k > ig::KMAX)
    return set_err(CNMF_ERR_UNSUPPORTED, "GPU init: n_features=%d (1..%d), k=%d (1..%d)", n_features, ig::FP, k, ig::KMAX);
  const int ncu = device_cus();
  const int64_t n_tiles = (n_rows + ig::GT - 1) / ig::GT;
  const int G = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, 4 * (int64_t)std::max(ncu, 1)));
  const size_t lds = (size_t)ig::FP * ig::KMAX * 8 + (size_t)ig::GT * (n_features + 1) * 8;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  switch (x_dtype) {
    case CNMF_F32: hipLaunchKernelGGL(ig_xm_kernel<float>, dim3(G), dim3(256), lds, hs, static_cast<const float*>(X), n_rows, n_features, k, M, U); break;
    case CNMF_F64: hipLaunchKernelGGL(ig_xm_kernel<double>, dim3(G), dim3(256), lds, hs, static_cast<const double*>(X), n_rows, n_features, k, M, U); break;
    case CNMF_BF16: hipLaunchKernelGGL(ig_xm_kernel<bf16_t>, dim3(G), dim3(256), lds, hs, static_cast<const bf16_t*>(X), n_rows, n_features, k, M, U); break;
    default: return set_err(CNMF_ERR_ARG, "x_dtype %d", x_dtype);
  }
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

int64_t cnmf_init_stats_rows(int64_t n_rows) { return n_rows > 0 ? ig_blocks(n_rows) : 0; }

int cnmf_init_stats(const double* U, int64_t n_rows, int k, double* out, int64_t n_parts, void* stream) {
  if (!U || !out) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (n_rows < 1 || k < 1 || k > ig::KMAX) return set_err(CNMF_ERR_SHAPE, "invalid shape");
  const int G = ig_blocks(n_rows);
  if (G > n_parts) return set_err(CNMF_ERR_ARG, "out holds %lld rows, the pass needs %d", (long long)n_parts, G);
  const int64_t rpb = (n_rows + G - 1) / G;
  hipLaunchKernelGGL(ig_stats_kernel, dim3(G), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), U, n_rows, k, rpb, out);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

int cnmf_init_fill(const double* U, int64_t n_rows, int k, const double* coef, const int* part, const double* sgn,
                   double eps, double fill, void* W, int w_dtype, void* stream) {
  if (!U || !coef || !part || !sgn || !W) return set_err(CNMF_ERR_ARG, "null pointer argument");
  if (n_rows < 1 || k < 1 || k > ig::KMAX) return set_err(CNMF_ERR_SHAPE, "invalid shape");
  const int ncu = device_cus();
  const int G = (int)std::max<int64_t>(1, std::min<int64_t>((n_rows * k + 255) / 256, 8 * (int64_t)std::max(ncu, 1)));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  if (w_dtype == CNMF_F32)
    hipLaunchKernelGGL(ig_fill_kernel<float>, dim3(G), dim3(256), 0, hs, U, n_rows, k, coef, part, sgn, eps, fill, static_cast<float*>(W));
  else if (w_dtype == CNMF_F64)
    hipLaunchKernelGGL(ig_fill_kernel<double>, dim3(G), dim3(256), 0, hs, U, n_rows, k, coef, part, sgn, eps, fill, static_cast<double*>(W));
  else
    return set_err(CNMF_ERR_ARG, "w_dtype %d", w_dtype);
  HIP_CHECK(hipGetLastError());
  return CNMF_OK;
}

}  // extern "C"
