// fcg_samg.hip -- the scalar smoothed-aggregation AMG of K_TT as a native object behind the C ABI
// (fcg_samg_create / _setup / _apply / _solve): the thermal block's multigrid in the monolithic TSI
// preconditioner (fcg_tsi_gmres_solve_amg) and a solver for a conduction problem on its own.  The
// host plan (aggregates, patterns, product plans) is fcg_samg_plan.cpp; this file is the numeric
// setup per K_TT and the cycle.
//
// Layout.  Every level is a scalar CSR matrix (int64 row pointers, int32 ascending columns).  Level
// 0 is the caller's K_TT read in place on the thermo context's k_TT graph: no copy, no permuted
// image.  P, P^T (values gathered through the transpose permutation), A P and A_c = P^T (A P) are
// stored per step on the patterns of the plan.
//
// Kernels.  A group of LPR lanes (4, 16 or 64, by the matrix's longest row: 16 for hex8 rows of
// 27 entries, 64 for hex27 rows of up to 125) serves a row and sums by butterfly, so every sum has
// one fixed order: no atomics on doubles, two setups or applies give the same bits.
//   scsr_spmv_kernel   y = alpha A x (+ y), or the residual y = b - A x
//   scsr_cheb_kernel   one Chebyshev degree fused: r_i = b_i - (A x)_i, d_i = c_d d_i + c_r r_i /
//                      a_ii, x'_i = x_i + d_i, x' a second buffer (the two ping-pong, so the kernel
//                      never reads an x it has written).  One pass over A's row per degree against
//                      the five launches and vector passes of cheb() in fcg_amg_solver.hip; both
//                      take their coefficients from fcg_amgs::ChebCoef.
// The dot product, the vector update, the flexible-CG steps, the Lanczos recurrence and the dense
// coarsest level are the structural AMG's, through fcg_amg_shared.hpp (fcg_amg_vec.hip).
// Byte model of a level-0 smoother degree: 12 bytes per non-zero (value + column) plus about 40
// bytes per row (b, x, d read, d, x' written; the row pointer and 1 / a_ii on top), the gathered
// x mostly from L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "fcg_amg_shared.hpp"
#include "fcg_samg_plan.hpp"
#include "fcg_status.hpp"
#include "fcg_tsi_internal.hpp"
#include "fourc_gpu.h"

namespace fcg_samgs {

using fcg_amgs::kBlock;

inline unsigned blocks_for(int64_t n) { return unsigned(std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }
// lanes per row for a matrix whose longest row has w entries
inline int lanes_for(int w) { return w <= 8 ? 4 : w <= 48 ? 16 : 64; }

template <int LPR>
__device__ inline double row_dot(const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const double* __restrict__ vals, const double* __restrict__ x, int64_t i, int64_t n, int lane)
{
  double a = 0.0;
  if (i < n)
  {
    const int64_t e = ptr[i + 1];
    for (int64_t k = ptr[i] + lane; k < e; k += LPR) a += vals[k] * x[col[k]];
  }
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o, LPR);
  return a;
}

// mode 0: y = alpha A x; 1: y += alpha A x; 2: y = b - A x
template <int LPR>
__global__ __launch_bounds__(kBlock) void scsr_spmv_kernel(int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, const double* __restrict__ x,
    const double* __restrict__ b, double* y, double alpha, int mode)
{
  const int lane = threadIdx.x % LPR;
  const int64_t i = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPR;
  const bool tail = i < n && lane == 0;
  const double add = tail ? (mode == 2 ? b[i] : mode == 1 ? y[i] : 0.0) : 0.0;  // before the row walk
  const double a = row_dot<LPR>(ptr, col, vals, x, i, n, lane);
  if (tail) y[i] = mode == 2 ? add - a : mode == 1 ? add + alpha * a : alpha * a;
}

// one Chebyshev degree (the modes of fcg_chebyshev_step), with z = (b - A x) / a_ii:
//   mode 0: d = c_r z,          x' = x + d
//   mode 1: d = c_d d + c_r z,  x' = x + d
//   mode 2: d = c_r b / a_ii,   x' = d      (first degree from x = 0: A and x are not read)
template <int LPR>
__global__ __launch_bounds__(kBlock) void scsr_cheb_kernel(int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, const double* __restrict__ dinv,
    const double* __restrict__ b, const double* __restrict__ x, double* __restrict__ d,
    double* __restrict__ xo, double c_d, double c_r, int mode)
{
  const int lane = threadIdx.x % LPR;
  const int64_t i = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPR;
  // the row's vector entries are asked for before the row walk, so their latency hides behind it
  const bool tail = i < n && lane == 0;
  const double bi = tail ? b[i] : 0.0, di = tail ? dinv[i] : 0.0, xi = tail ? x[i] : 0.0;
  const double dold = tail && mode == 1 ? d[i] : 0.0;
  const double a = row_dot<LPR>(ptr, col, vals, x, i, n, lane);
  if (!tail) return;
  const double z = (bi - a) * di;
  const double dn = mode == 1 ? c_d * dold + c_r * z : c_r * z;
  d[i] = dn;
  xo[i] = xi + dn;
}

__global__ __launch_bounds__(kBlock) void cheb_first_kernel(int64_t n, const double* __restrict__ dinv,
    const double* __restrict__ b, double* __restrict__ d, double* __restrict__ xo, double c_r)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double dn = c_r * (b[i] * dinv[i]);
  d[i] = dn;
  xo[i] = dn;
}

// dinv[i] = 1 / a_ii; a missing, zero or non-finite diagonal entry sets the flag (tsi_dtt_kernel)
__global__ __launch_bounds__(kBlock) void diag_kernel(int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, double* __restrict__ dinv, int32_t* flag)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  double d = 0.0;
  for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k)
    if (col[k] == i) d = vals[k];
  const double inv = 1.0 / d;
  if (d == 0.0 || !isfinite(inv))
  {
    atomicMax(flag, 1);
    dinv[i] = 0.0;
    return;
  }
  dinv[i] = inv;
}

// P = T - w D^-1 (A T) on P's pattern, one thread per entry (i, j): (A T)_ij sums a_ik tent_k over
// the neighbours k of i in aggregate j, in the row's order
__global__ __launch_bounds__(kBlock) void smooth_p_kernel(int64_t nnz_p, const int32_t* __restrict__ p_row,
    const int32_t* __restrict__ p_col, const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const double* __restrict__ vals, const int32_t* __restrict__ agg, const double* __restrict__ tent,
    const double* __restrict__ dinv, double w, double* __restrict__ p_vals)
{
  const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= nnz_p) return;
  const int64_t i = p_row[e];
  const int32_t j = p_col[e];
  double s = 0.0;
  for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k)
  {
    const int32_t c = col[k];
    if (agg[c] == j) s += vals[k] * tent[c];
  }
  p_vals[e] = (agg[i] == j ? tent[i] : 0.0) - w * (dinv[i] * s);
}

// C = A B from the product plan, one thread per entry of C, the pairs in the plan's order
__global__ __launch_bounds__(kBlock) void product_kernel(int64_t nnz_c, const int64_t* __restrict__ pp,
    const int32_t* __restrict__ pa, const int32_t* __restrict__ pb, const double* __restrict__ va,
    const double* __restrict__ vb, double* __restrict__ vc)
{
  const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= nnz_c) return;
  double s = 0.0;
  for (int64_t t = pp[e]; t < pp[e + 1]; ++t) s += va[pa[t]] * vb[pb[t]];
  vc[e] = s;
}

__global__ __launch_bounds__(kBlock) void gather_kernel(int64_t n, const int64_t* __restrict__ perm,
    const double* __restrict__ src, double* __restrict__ dst)
{
  const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e < n) dst[e] = src[perm[e]];
}

// D (zeroed, row-major n x n) = the CSR matrix, one thread per row
__global__ __launch_bounds__(kBlock) void to_dense_kernel(int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, double* __restrict__ D)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) D[i * n + col[k]] = vals[k];
}

// z = dinv .* r
__global__ __launch_bounds__(kBlock) void scale_kernel(const double* __restrict__ dinv,
    const double* __restrict__ r, double* __restrict__ z, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) z[i] = dinv[i] * r[i];
}

// Lanczos start: a fixed pseudo-random vector in [-0.5, 0.5), zero where the row is masked out
__global__ __launch_bounds__(kBlock) void random_kernel(double* v, const uint8_t* __restrict__ skip, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t h = uint64_t(i) * 0x9E3779B97F4A7C15ull + 20251015u;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  const double u = double(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
  v[i] = skip && skip[i] ? 0.0 : u;
}

struct Fail {
  int code;
  std::string msg;
};
inline void ck(hipError_t e, const char* what)
{
  if (e == hipSuccess) return;
  const std::string m = std::string(what) + ": " + hipGetErrorString(e);
  throw Fail{fcg_device_error(), m};
}

struct DCsr {
  int64_t n = 0, n_cols = 0, nnz = 0;
  const int64_t* ptr = nullptr;
  const int32_t* col = nullptr;
  double* vals = nullptr;  // level 0's A: NULL, the caller's K_TT is passed with every call
  int lanes = 16;
};

struct DPlan {
  int64_t* ptr = nullptr;
  int32_t *a = nullptr, *b = nullptr;
};

struct DStep {
  DCsr P, Pt, AP;
  int32_t* agg = nullptr;
  double* tent = nullptr;
  int32_t* p_row = nullptr;
  int64_t* perm = nullptr;
  DPlan pAP, pAc;
};

struct DLevel {
  DCsr A;
  double* dinv = nullptr;
  double lmax = 0.0;
  // host time of the level's share of the last numeric setup (every share ends in a stream
  // synchronisation): the Lanczos estimate, P, A P and A_c of the step below it; on the coarsest
  // level the dense inverse
  double setup_ms = 0.0;
  double* v[8] = {};  // work vectors: level 0 has eight, the others six
};

void launch_spmv(const DCsr& A, const double* vals, const double* x, const double* b, double* y,
    double alpha, int mode, hipStream_t s)
{
  if (A.n == 0) return;
  if (A.lanes == 4)
    hipLaunchKernelGGL(scsr_spmv_kernel<4>, dim3(blocks_for(A.n * 4)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, x, b, y, alpha, mode);
  else if (A.lanes == 16)
    hipLaunchKernelGGL(scsr_spmv_kernel<16>, dim3(blocks_for(A.n * 16)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, x, b, y, alpha, mode);
  else
    hipLaunchKernelGGL(scsr_spmv_kernel<64>, dim3(blocks_for(A.n * 64)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, x, b, y, alpha, mode);
}

void launch_cheb(const DCsr& A, const double* vals, const double* dinv, const double* b, const double* x,
    double* d, double* xo, double c_d, double c_r, int mode, hipStream_t s)
{
  if (A.n == 0) return;
  if (mode == 2)
    hipLaunchKernelGGL(cheb_first_kernel, dim3(blocks_for(A.n)), dim3(kBlock), 0, s, A.n, dinv, b, d, xo, c_r);
  else if (A.lanes == 4)
    hipLaunchKernelGGL(scsr_cheb_kernel<4>, dim3(blocks_for(A.n * 4)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, dinv, b, x, d, xo, c_d, c_r, mode);
  else if (A.lanes == 16)
    hipLaunchKernelGGL(scsr_cheb_kernel<16>, dim3(blocks_for(A.n * 16)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, dinv, b, x, d, xo, c_d, c_r, mode);
  else
    hipLaunchKernelGGL(scsr_cheb_kernel<64>, dim3(blocks_for(A.n * 64)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
        vals, dinv, b, x, d, xo, c_d, c_r, mode);
}

}  // namespace fcg_samgs

struct fcg_samg {
  fcg_tsi_ctx* tctx = nullptr;
  int device = 0;
  fcg_amg_options opt{};
  fcg_samgs::Plan plan;  // host patterns (fcg_samg_level_matrix reads them)
  std::vector<fcg_samgs::DLevel> levels;
  std::vector<fcg_samgs::DStep> steps;
  std::vector<void*> allocs;
  int64_t bytes = 0;
  uint8_t* skip = nullptr;  // [n0] Dirichlet marks
  double* partial = nullptr;
  double* sc = nullptr;  // [8]
  int32_t* flag = nullptr;
  double* cbuf[2] = {nullptr, nullptr};
  double* cwork = nullptr;
  double* cinv = nullptr;
  const double* last_K = nullptr;
  bool ready = false;
  std::string last_error;
};

namespace fcg_samgs {

template <typename T>
T* dalloc(fcg_samg* h, int64_t n)
{
  void* p = nullptr;
  const size_t b = sizeof(T) * size_t(std::max<int64_t>(n, 1));
  ck(hipMalloc(&p, b), "hipMalloc");
  h->allocs.push_back(p);
  h->bytes += int64_t(b);
  h->tctx->device_bytes += int64_t(b);
  return static_cast<T*>(p);
}
template <typename T>
T* upload(fcg_samg* h, const std::vector<T>& v)
{
  T* p = dalloc<T>(h, int64_t(v.size()));
  if (!v.empty()) ck(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice), "hipMemcpy");
  return p;
}

void upload_pattern(fcg_samg* h, const Pattern& P, DCsr& D, bool with_vals)
{
  D.n = P.n_rows;
  D.n_cols = P.n_cols;
  D.nnz = P.nnz();
  D.ptr = upload(h, P.ptr);
  D.col = upload(h, P.col);
  D.vals = with_vals ? dalloc<double>(h, D.nnz) : nullptr;
  D.lanes = lanes_for(P.widest());
}

double dot_host(fcg_samg* h, const double* a, const double* b, int64_t n, hipStream_t s)
{
  return fcg_amgs::dot_host(a, b, n, h->partial, h->sc + 6, s, ck);
}
void dot_dev(fcg_samg* h, const double* a, const double* b, int64_t n, double* out, hipStream_t s)
{
  fcg_amgs::dot(a, b, n, h->partial, out, s);
}

inline const double* vals_of(const fcg_samg* h, int l, const double* K) { return l == 0 ? K : h->levels[size_t(l)].A.vals; }

// lambda_max(D^-1 A) of level l by the 10-step Lanczos both AMGs run (fcg_amgs::lanczos_steps:
// Jacobi-preconditioned CG, here on a fixed random vector, zero on level 0's Dirichlet rows); the
// tridiagonal's largest eigenvalue by the shared Sturm bisection
void estimate_lmax(fcg_samg* h, int l, const double* K, hipStream_t s)
{
  DLevel& L = h->levels[size_t(l)];
  const int64_t n = L.A.n;
  const int o = l == 0 ? 3 : 1;
  double *r = L.v[o], *z = L.v[o + 1], *p = L.v[o + 2], *q = L.v[o + 3];
  const double* vals = vals_of(h, l, K);
  const dim3 g(blocks_for(n)), bl(kBlock);
  hipLaunchKernelGGL(random_kernel, g, bl, 0, s, r, l == 0 ? h->skip : nullptr, n);
  hipLaunchKernelGGL(scale_kernel, g, bl, 0, s, L.dinv, r, z, n);
  ck(hipMemcpyAsync(p, z, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, s), "copy");
  const fcg_amgs::LanczosSteps t = fcg_amgs::lanczos_steps(
      [&](const double* x, double* y) { launch_spmv(L.A, vals, x, nullptr, y, 1.0, 0, s); },
      [&](const double* x, double* y) { hipLaunchKernelGGL(scale_kernel, g, bl, 0, s, L.dinv, x, y, n); },
      [&](const double* x, const double* y) { return dot_host(h, x, y, n, s); }, r, z, p, q, n, s);
  if (t.al.empty()) throw Fail{FCG_ERR_SINGULAR, "scalar AMG Lanczos estimate on level " + std::to_string(l) + ": p.Ap <= 0"};
  L.lmax = fcg_amgs::lanczos_lmax(t.al, t.be);
  if (!(L.lmax > 0.0) || !std::isfinite(L.lmax))
    throw Fail{FCG_ERR_SINGULAR, "scalar AMG: lambda_max estimate of level " + std::to_string(l) + " is not positive"};
}

void diag_setup(fcg_samg* h, int l, const double* K, hipStream_t s)
{
  DLevel& L = h->levels[size_t(l)];
  int32_t bad = 0;
  ck(hipMemsetAsync(h->flag, 0, sizeof(int32_t), s), "memset");
  hipLaunchKernelGGL(diag_kernel, dim3(blocks_for(L.A.n)), dim3(kBlock), 0, s, L.A.n, L.A.ptr, L.A.col,
      vals_of(h, l, K), L.dinv, h->flag);
  ck(hipGetLastError(), "diag_kernel");
  ck(hipMemcpyAsync(&bad, h->flag, sizeof(bad), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  if (bad)
    throw Fail{FCG_ERR_SINGULAR, l == 0 ? std::string("a zero, missing or non-finite diagonal entry of K_TT")
                                        : "scalar AMG level " + std::to_string(l) + ": a zero or non-finite diagonal entry"};
}

void setup(fcg_samg* h, const double* K, hipStream_t s)
{
  h->ready = false;
  h->cinv = nullptr;
  const int nl = int(h->levels.size());
  using clock = std::chrono::steady_clock;
  auto t0 = clock::now();
  auto lap = [&](int l) {
    const auto t1 = clock::now();
    h->levels[size_t(l)].setup_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  };
  diag_setup(h, 0, K, s);
  for (int l = 0; l + 1 < nl; ++l)
  {
    DLevel& L = h->levels[size_t(l)];
    DStep& st = h->steps[size_t(l)];
    const double* vals = vals_of(h, l, K);
    estimate_lmax(h, l, K, s);
    hipLaunchKernelGGL(smooth_p_kernel, dim3(blocks_for(st.P.nnz)), dim3(kBlock), 0, s, st.P.nnz, st.p_row,
        st.P.col, L.A.ptr, L.A.col, vals, st.agg, st.tent, L.dinv, h->opt.omega / L.lmax, st.P.vals);
    hipLaunchKernelGGL(product_kernel, dim3(blocks_for(st.AP.nnz)), dim3(kBlock), 0, s, st.AP.nnz, st.pAP.ptr,
        st.pAP.a, st.pAP.b, vals, st.P.vals, st.AP.vals);
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(st.Pt.nnz)), dim3(kBlock), 0, s, st.Pt.nnz, st.perm,
        st.P.vals, st.Pt.vals);
    DLevel& C = h->levels[size_t(l) + 1];
    hipLaunchKernelGGL(product_kernel, dim3(blocks_for(C.A.nnz)), dim3(kBlock), 0, s, C.A.nnz, st.pAc.ptr,
        st.pAc.a, st.pAc.b, st.Pt.vals, st.AP.vals, C.A.vals);
    ck(hipGetLastError(), "Galerkin products");
    diag_setup(h, l + 1, K, s);
    lap(l);
  }
  if (nl == 1) estimate_lmax(h, 0, K, s);  // no coarse level: the cycle is level 0's smoother alone
  if (nl > 1)
  {
    // the coarsest level's dense inverse (the structural AMG's Gauss-Jordan kernels)
    const DLevel& C = h->levels.back();
    const int64_t n = C.A.n;
    int32_t bad = 0;
    ck(hipMemsetAsync(h->cbuf[0], 0, sizeof(double) * size_t(n * n), s), "memset");
    ck(hipMemsetAsync(h->flag, 0, sizeof(int32_t), s), "memset");
    hipLaunchKernelGGL(to_dense_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, C.A.ptr, C.A.col, C.A.vals,
        h->cbuf[0]);
    const int inv = fcg_amgs::dense_inverse(h->cbuf, h->cwork, n, h->flag, s);
    ck(hipGetLastError(), "dense inverse");
    ck(hipMemcpyAsync(&bad, h->flag, sizeof(bad), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
    ck(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (bad) throw Fail{FCG_ERR_SINGULAR, "scalar AMG: the coarsest level is not positive definite (a pivot <= 0)"};
    h->cinv = h->cbuf[inv];
  }
  lap(nl - 1);
  h->last_K = K;
  h->ready = true;
}

// nu Chebyshev degrees on level l; the iterate moves from `from` (NULL: x = 0) through the two
// buffers and ends in the one returned
double* cheb(fcg_samg* h, int l, const double* K, const double* b, const double* from, double* buf0,
    double* buf1, double* d, hipStream_t s)
{
  const fcg_amg_options& op = h->opt;
  const DLevel& L = h->levels[size_t(l)];
  const double* vals = vals_of(h, l, K);
  fcg_amgs::ChebCoef c(L.lmax, op.boost, op.ratio);
  double* out = buf0;
  launch_cheb(L.A, vals, L.dinv, b, from, d, out, 0.0, c.first(), from ? 0 : 2, s);
  for (int k = 1; k < op.nu; ++k)
  {
    const fcg_amgs::ChebCoef::Degree g = c.next();
    double* nxt = out == buf0 ? buf1 : buf0;
    launch_cheb(L.A, vals, L.dinv, b, out, d, nxt, g.c_d, g.c_r, 1, s);
    out = nxt;
  }
  return out;
}

// one V-cycle on level l: x = M_l b, x one of the level's buffers, the other one scratch
void vcycle(fcg_samg* h, int l, const double* K, const double* b, double* x, double* x2, hipStream_t s)
{
  const int nl = int(h->levels.size());
  DLevel& L = h->levels[size_t(l)];
  if (nl == 1)
  {
    // no coarse level (a mesh below coarse_max): the smoother alone
    const int sw = h->opt.nu - 1;
    double* out = cheb(h, l, K, b, nullptr, sw % 2 ? x2 : x, sw % 2 ? x : x2, l == 0 ? L.v[1] : L.v[3], s);
    (void)out;
    return;
  }
  if (l == nl - 1)
  {
    fcg_amgs::dense_mv(h->cinv, b, x, L.A.n, s);
    return;
  }
  double* d = l == 0 ? L.v[1] : L.v[3];
  double* r = l == 0 ? L.v[2] : L.v[4];
  // 2 nu - 1 buffer changes in all (odd): starting in the scratch buffer ends in x
  double* cur = cheb(h, l, K, b, nullptr, x2, x, d, s);
  double* oth = cur == x ? x2 : x;
  launch_spmv(L.A, vals_of(h, l, K), cur, b, r, 1.0, 2, s);
  DStep& st = h->steps[size_t(l)];
  DLevel& C = h->levels[size_t(l) + 1];
  launch_spmv(st.Pt, st.Pt.vals, r, nullptr, C.v[0], 1.0, 0, s);
  vcycle(h, l + 1, K, C.v[0], C.v[1], C.v[2], s);
  launch_spmv(st.P, st.P.vals, C.v[1], nullptr, cur, 1.0, 1, s);
  cur = cheb(h, l, K, b, cur, oth, cur, d, s);
  (void)cur;  // == x
}

void run_fcg(fcg_samg* h, const double* K, const double* b, double* x, double rtol, int max_iter,
    int* iterations, double* rel, hipStream_t s)
{
  DLevel& L = h->levels[0];
  const int64_t n = L.A.n;
  double *r = L.v[3], *z = L.v[4], *p = L.v[5], *q = L.v[6], *ro = L.v[7];
  double* sc = h->sc;
  *iterations = 0;
  *rel = 0.0;
  ck(hipMemsetAsync(x, 0, sizeof(double) * size_t(n), s), "memset");
  const double bn = std::sqrt(dot_host(h, b, b, n, s));
  if (!std::isfinite(bn)) throw Fail{FCG_ERR_SINGULAR, "fcg_samg_solve: non-finite right-hand side"};
  if (bn == 0.0) return;
  ck(hipMemcpyAsync(r, b, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, s), "copy");
  vcycle(h, 0, K, r, z, L.v[0], s);
  ck(hipMemcpyAsync(p, z, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, s), "copy");
  dot_dev(h, r, z, n, sc + 0, s);
  double rz = 0.0;
  ck(hipMemcpyAsync(&rz, sc, sizeof(double), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  if (!(rz > 0.0)) throw Fail{FCG_ERR_SINGULAR, "fcg_samg_solve: indefinite V-cycle (r.z <= 0)"};
  int it = 0;
  while (it < max_iter)
  {
    ++it;
    launch_spmv(L.A, K, p, nullptr, q, 1.0, 0, s);
    dot_dev(h, p, q, n, sc + 1, s);
    fcg_amgs::fcg_step(sc, p, q, x, r, ro, n, s);
    dot_dev(h, r, r, n, sc + 3, s);
    vcycle(h, 0, K, r, z, L.v[0], s);
    dot_dev(h, r, z, n, sc + 2, s);
    dot_dev(h, z, ro, n, sc + 5, s);
    double hs[6];
    ck(hipMemcpyAsync(hs, sc, sizeof(hs), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
    ck(hipStreamSynchronize(s), "hipStreamSynchronize");
    const double rn = std::sqrt(hs[3]);
    if (!std::isfinite(rn)) throw Fail{FCG_ERR_SINGULAR, "fcg_samg_solve: non-finite residual"};
    if (rn <= rtol * bn) break;
    if (!(hs[2] > 0.0)) throw Fail{FCG_ERR_SINGULAR, "fcg_samg_solve: indefinite V-cycle (r.z <= 0)"};
    fcg_amgs::fcg_dir(sc, z, p, n, s);
    fcg_amgs::fcg_shift(sc, s);
  }
  // the true residual at return
  launch_spmv(L.A, K, x, b, r, 1.0, 2, s);
  *iterations = it;
  *rel = std::sqrt(dot_host(h, r, r, n, s)) / bn;
}

void free_all(fcg_samg* h)
{
  for (void* p : h->allocs) (void)hipFree(p);
  h->allocs.clear();
  if (h->tctx) h->tctx->device_bytes -= h->bytes;
  h->bytes = 0;
}

}  // namespace fcg_samgs

extern "C" {

void fcg_samg_default_options(fcg_amg_options* opt)
{
  if (!opt) return;
  fcg_amg_default_options(opt);
  opt->coarse_max = 300;
}

int fcg_samg_create(fcg_tsi_ctx* tctx, const int64_t* rowptr_tt, const int32_t* col_tt, int64_t n_dbc,
    const int32_t* dbc_rows_t, const fcg_amg_options* opt, fcg_samg** out)
{
  using namespace fcg_samgs;
  if (out) *out = nullptr;
  if (!tctx || !out) return FCG_ERR_ARG;
  const fcg::TsiDevice& d = tctx->d;
  if (d.n_cols_t != d.n_rows_t)
  {
    tctx->last_error = "fcg_samg_create: single-rank thermo contexts only (n_cols_t = n_rows_t)";
    return FCG_ERR_ARG;
  }
  if (!d.col_tt)
  {
    tctx->last_error = "fcg_samg_create: the thermo context does not keep its k_TT graph on the device (its "
                       "numbering is not node-consistent)";
    return FCG_ERR_ARG;
  }
  const int64_t n = d.n_rows_t;
  if (n_dbc < 0 || (n_dbc > 0 && !dbc_rows_t) || (n > 0 && (!rowptr_tt || !col_tt)))
  {
    tctx->last_error = "fcg_samg_create: a negative count, or an array missing";
    return FCG_ERR_ARG;
  }
  if (n > 0 && rowptr_tt[n] != d.nnz_tt)
  {
    tctx->last_error = "fcg_samg_create: the graph is not the context's k_TT graph (entry counts differ)";
    return FCG_ERR_ARG;
  }
  fcg_amg_options o;
  if (opt)
    o = *opt;
  else
    fcg_samg_default_options(&o);
  if (o.nu < 1 || o.max_levels < 1 || o.coarse_max < 1 || !(o.omega >= 0.0) || !(o.ratio > 1.0) || !(o.boost > 0.0))
  {
    tctx->last_error = "fcg_samg_create: options out of range (nu, max_levels, coarse_max >= 1, omega >= 0, "
                       "ratio > 1, boost > 0)";
    return FCG_ERR_ARG;
  }
  std::vector<uint8_t> skip(size_t(n), 0);
  for (int64_t k = 0; k < n_dbc; ++k)
  {
    if (dbc_rows_t[k] < 0 || dbc_rows_t[k] >= n)
    {
      tctx->last_error = "fcg_samg_create: Dirichlet row " + std::to_string(dbc_rows_t[k]) + " outside the row map";
      return FCG_ERR_ARG;
    }
    skip[size_t(dbc_rows_t[k])] = 1;
  }
  fcg_samg* h = new fcg_samg;
  h->tctx = tctx;
  h->device = tctx->device;
  h->opt = o;
  std::string err;
  if (!build_plan(n, rowptr_tt, col_tt, skip.data(), o.coarse_max, o.max_levels, h->plan, err))
  {
    tctx->last_error = "fcg_samg_create: " + err;
    delete h;
    return FCG_ERR_ARG;
  }
  const size_t ns = h->plan.steps.size();
  const int64_t nc = ns ? h->plan.steps.back().n_agg : 0;
  if (nc > fcg_amgs::kDenseMax)
  {
    tctx->last_error = "fcg_samg_create: the coarsest level has " + std::to_string(nc) + " rows, more than the "
                       "dense inverse takes (4096): raise max_levels or lower coarse_max";
    delete h;
    return FCG_ERR_ARG;
  }
  if (!fcg_use_device(h->device))
  {
    tctx->last_error = "fcg_samg_create: the context's device is not available";
    delete h;
    return FCG_ERR_DEVICE;
  }
  try
  {
    h->levels.resize(ns + 1);
    h->steps.resize(ns);
    DLevel& L0 = h->levels[0];
    L0.A.n = L0.A.n_cols = n;
    L0.A.nnz = d.nnz_tt;
    L0.A.ptr = d.rowptr_tt;
    L0.A.col = d.col_tt;
    L0.A.lanes = lanes_for(h->plan.widest0);
    for (size_t l = 0; l <= ns; ++l)
    {
      DLevel& L = h->levels[l];
      if (l > 0) upload_pattern(h, h->plan.steps[l - 1].Ac, L.A, true);
      L.dinv = dalloc<double>(h, L.A.n);
      for (int k = 0; k < (l == 0 ? 8 : 6); ++k) L.v[k] = dalloc<double>(h, L.A.n);
    }
    for (size_t l = 0; l < ns; ++l)
    {
      const PlanStep& ps = h->plan.steps[l];
      DStep& st = h->steps[l];
      upload_pattern(h, ps.P, st.P, true);
      upload_pattern(h, ps.Pt, st.Pt, true);
      upload_pattern(h, ps.AP, st.AP, true);
      st.agg = upload(h, ps.agg);
      st.tent = upload(h, ps.tent);
      st.p_row = upload(h, ps.p_row);
      st.perm = upload(h, ps.perm);
      st.pAP.ptr = upload(h, ps.pAP.ptr);
      st.pAP.a = upload(h, ps.pAP.a);
      st.pAP.b = upload(h, ps.pAP.b);
      st.pAc.ptr = upload(h, ps.pAc.ptr);
      st.pAc.a = upload(h, ps.pAc.a);
      st.pAc.b = upload(h, ps.pAc.b);
    }
    h->skip = upload(h, skip);
    h->partial = dalloc<double>(h, fcg_amgs::kMaxPartials);
    h->sc = dalloc<double>(h, 8);
    h->flag = dalloc<int32_t>(h, 1);
    if (ns)
    {
      h->cbuf[0] = dalloc<double>(h, nc * nc);
      h->cbuf[1] = dalloc<double>(h, nc * nc);
      h->cwork = dalloc<double>(h, fcg_amgs::dense_inverse_work(nc));
    }
    // the device holds the product plans now; the host keeps the patterns for fcg_samg_level_matrix
    for (PlanStep& ps : h->plan.steps)
    {
      ps.pAP = ProductPlan();
      ps.pAc = ProductPlan();
    }
  }
  catch (const Fail& f)
  {
    tctx->last_error = "fcg_samg_create: " + f.msg;
    free_all(h);
    delete h;
    return f.code;
  }
  *out = h;
  return FCG_OK;
}

int fcg_samg_setup(fcg_samg* h, const double* d_Ktt, void* stream)
{
  using namespace fcg_samgs;
  if (!h) return FCG_ERR_ARG;
  if (h->levels[0].A.n == 0)
  {
    h->ready = true;
    return FCG_OK;
  }
  if (!d_Ktt)
  {
    h->last_error = "fcg_samg_setup: K_TT is NULL";
    return FCG_ERR_ARG;
  }
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    setup(h, d_Ktt, stream ? static_cast<hipStream_t>(stream) : h->tctx->stream);
  }
  catch (const Fail& f)
  {
    h->last_error = "fcg_samg_setup: " + f.msg;
    return f.code;
  }
  return FCG_OK;
}

int fcg_samg_apply(fcg_samg* h, const double* d_Ktt, const double* d_r, double* d_z, void* stream)
{
  using namespace fcg_samgs;
  if (!h) return FCG_ERR_ARG;
  if (!h->ready)
  {
    h->last_error = "fcg_samg_apply: no numeric setup for this K_TT (call fcg_samg_setup first)";
    return FCG_ERR_ARG;
  }
  if (h->levels[0].A.n == 0) return FCG_OK;
  if (!d_Ktt || !d_r || !d_z)
  {
    h->last_error = "fcg_samg_apply: a NULL matrix or vector";
    return FCG_ERR_ARG;
  }
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->tctx->stream;
    vcycle(h, 0, d_Ktt, d_r, d_z, h->levels[0].v[0], s);
    ck(hipGetLastError(), "V-cycle");
  }
  catch (const Fail& f)
  {
    h->last_error = "fcg_samg_apply: " + f.msg;
    return f.code;
  }
  return FCG_OK;
}

int fcg_samg_solve(fcg_samg* h, const double* d_Ktt, const double* d_b, double* d_x, double rtol,
    int max_iter, int* iterations, double* rel_residual, void* stream)
{
  using namespace fcg_samgs;
  if (!h) return FCG_ERR_ARG;
  int it = 0;
  double rel = 0.0;
  if (iterations) *iterations = 0;
  if (rel_residual) *rel_residual = 0.0;
  if (!h->ready)
  {
    h->last_error = "fcg_samg_solve: no numeric setup for this K_TT (call fcg_samg_setup first)";
    return FCG_ERR_ARG;
  }
  if (h->levels[0].A.n == 0) return FCG_OK;
  if (!d_Ktt || !d_b || !d_x || !(rtol >= 0.0) || max_iter < 0)
  {
    h->last_error = "fcg_samg_solve: a NULL matrix or vector, rtol < 0 or max_iter < 0";
    return FCG_ERR_ARG;
  }
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    run_fcg(h, d_Ktt, d_b, d_x, rtol, max_iter, &it, &rel, stream ? static_cast<hipStream_t>(stream) : h->tctx->stream);
  }
  catch (const Fail& f)
  {
    h->last_error = f.msg;
    return f.code;
  }
  if (iterations) *iterations = it;
  if (rel_residual) *rel_residual = rel;
  return FCG_OK;
}

int fcg_samg_levels(const fcg_samg* h) { return h ? int(h->levels.size()) : 0; }

int fcg_samg_level_info(const fcg_samg* h, int level, int64_t* rows, int64_t* nnz, double* lmax)
{
  if (!h || level < 0 || level >= int(h->levels.size())) return FCG_ERR_ARG;
  const fcg_samgs::DLevel& L = h->levels[size_t(level)];
  if (rows) *rows = L.A.n;
  if (nnz) *nnz = L.A.nnz;
  if (lmax) *lmax = L.lmax;
  return FCG_OK;
}

int64_t fcg_samg_level_matrix(const fcg_samg* h, int level, int which, int64_t* ptr, int32_t* col,
    double* vals, int64_t capacity)
{
  using namespace fcg_samgs;
  if (!h || level < 0 || (which != 0 && which != 1)) return -1;
  const int nl = int(h->levels.size());
  if (level >= nl || (which == 1 && level + 1 >= nl)) return -1;
  const DCsr& M = which == 0 ? h->levels[size_t(level)].A : h->steps[size_t(level)].P;
  if (!ptr && !col && !vals) return M.nnz;
  if (!ptr || !col || !vals || capacity < M.nnz || !h->ready) return -1;
  if (!fcg_use_device(h->device)) return -1;
  const double* dv = which == 0 && level == 0 ? h->last_K : M.vals;
  hipError_t he = hipDeviceSynchronize();
  if (he == hipSuccess) he = hipMemcpy(ptr, M.ptr, sizeof(int64_t) * size_t(M.n + 1), hipMemcpyDeviceToHost);
  if (he == hipSuccess && M.nnz) he = hipMemcpy(col, M.col, sizeof(int32_t) * size_t(M.nnz), hipMemcpyDeviceToHost);
  if (he == hipSuccess && M.nnz) he = hipMemcpy(vals, dv, sizeof(double) * size_t(M.nnz), hipMemcpyDeviceToHost);
  if (he != hipSuccess)
  {
    (void)hipGetLastError();
    return -1;
  }
  return M.nnz;
}

double fcg_samg_setup_ms(const fcg_samg* h, int level)
{
  if (!h || level >= int(h->levels.size())) return -1.0;
  if (level >= 0) return h->levels[size_t(level)].setup_ms;
  double t = 0.0;
  for (const auto& L : h->levels) t += L.setup_ms;
  return t;
}

const char* fcg_samg_last_error(const fcg_samg* h) { return h ? h->last_error.c_str() : ""; }

int fcg_samg_destroy(fcg_samg* h)
{
  if (!h) return FCG_OK;
  (void)hipSetDevice(h->device);
  fcg_samgs::free_all(h);
  delete h;
  return FCG_OK;
}

// the thermo context a handle was created on (fcg_tsi_gmres_solve_amg checks it)
const fcg_tsi_ctx* fcg_samg_context(const fcg_samg* h) { return h ? h->tctx : nullptr; }

// The level-0 kernels on any scalar CSR matrix (device arrays; row_width: the longest row, which
// selects the lanes per row).  fcg_scsr_spmv mode 0: y = alpha A x, 1: y += alpha A x, 2: y = b - A x.
int fcg_scsr_spmv(int device, int64_t n, int64_t row_width, const int64_t* d_ptr, const int32_t* d_col,
    const double* d_vals, const double* d_x, const double* d_b, double* d_y, double alpha, int mode,
    void* stream)
{
  using namespace fcg_samgs;
  if (n < 0 || row_width < 0 || mode < 0 || mode > 2) return FCG_ERR_ARG;
  if (n == 0) return FCG_OK;
  if (!d_ptr || !d_col || !d_vals || !d_x || !d_y || (mode == 2 && !d_b)) return FCG_ERR_ARG;
  if (!fcg_use_device(device)) return FCG_ERR_DEVICE;
  DCsr A;
  A.n = n;
  A.ptr = d_ptr;
  A.col = d_col;
  A.lanes = lanes_for(int(std::min<int64_t>(row_width, 1 << 20)));
  launch_spmv(A, d_vals, d_x, d_b, d_y, alpha, mode, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? FCG_OK : fcg_device_error();
}

int fcg_scsr_chebyshev_step(int device, int64_t n, int64_t row_width, const int64_t* d_ptr,
    const int32_t* d_col, const double* d_vals, const double* d_dinv, const double* d_b,
    const double* d_x, double* d_d, double* d_x_out, double c_d, double c_r, int mode, void* stream)
{
  using namespace fcg_samgs;
  if (n < 0 || row_width < 0 || mode < 0 || mode > 2) return FCG_ERR_ARG;
  if (n == 0) return FCG_OK;
  if (!d_dinv || !d_b || !d_d || !d_x_out || d_x == d_x_out) return FCG_ERR_ARG;
  if (mode != 2 && (!d_ptr || !d_col || !d_vals || !d_x)) return FCG_ERR_ARG;
  if (!fcg_use_device(device)) return FCG_ERR_DEVICE;
  DCsr A;
  A.n = n;
  A.ptr = d_ptr;
  A.col = d_col;
  A.lanes = lanes_for(int(std::min<int64_t>(row_width, 1 << 20)));
  launch_cheb(A, d_vals, d_dinv, d_b, d_x, d_d, d_x_out, c_d, c_r, mode, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? FCG_OK : fcg_device_error();
}

}  // extern "C"
