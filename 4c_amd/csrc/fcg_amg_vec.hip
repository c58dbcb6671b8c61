// fcg_amg_vec.hip -- the kernels the structural AMG (fcg_amg_solver.hip, fcg_amg_coupled.hip) and
// the scalar AMG of K_TT (fcg_samg.hip) share, behind the host launchers of fcg_amg_shared.hpp: the
// dot product, the vector update and the flexible-CG steps, the Sturm bisection of the Lanczos
// estimate and the dense coarsest level.  The launchers take raw pointers and a stream, no handle,
// and check nothing: each caller wraps what can fail in its own ck.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fcg_amg_shared.hpp"

namespace fcg_amgs {

// one thread per entry; at least one workgroup, so that n = 0 is a launch that does nothing
static unsigned grid_for(int64_t n) { return unsigned(std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }

__device__ inline double block_sum(double v, double* sbuf)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sbuf[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < int(blockDim.x >> 6); ++i) t += sbuf[i];
  __syncthreads();
  return t;
}

// partial[block] = sum over the block's grid-stride share of a . b (fixed assignment)
__global__ __launch_bounds__(kBlock) void dot_kernel(const double* __restrict__ a,
    const double* __restrict__ b, int64_t n, double* partial)
{
  __shared__ double sbuf[kBlock / 64];
  double t = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock)
    t += a[i] * b[i];
  const double s = block_sum(t, sbuf);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out = sum of n partials (one block, fixed order)
__global__ __launch_bounds__(kBlock) void reduce_kernel(const double* __restrict__ partial, int n,
    double* out)
{
  __shared__ double sbuf[kBlock / 64];
  double t = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) t += partial[i];
  const double s = block_sum(t, sbuf);
  if (threadIdx.x == 0) *out = s;
}

// y = a x + b y
__global__ __launch_bounds__(kBlock) void axpby_kernel(double a, const double* __restrict__ x,
    double b, double* y, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) y[i] = a * x[i] + b * y[i];
}

// FCG step, scalars on the device (sc[0] = r.z, sc[1] = p.q): alpha = r.z / p.q; x += alpha p;
// r_old = r; r -= alpha q
__global__ __launch_bounds__(kBlock) void fcg_step_kernel(const double* __restrict__ sc,
    const double* __restrict__ p, const double* __restrict__ q, double* x, double* r, double* r_old,
    int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double alpha = sc[0] / sc[1];
  x[i] += alpha * p[i];
  r_old[i] = r[i];
  r[i] -= alpha * q[i];
}
// FCG direction (Polak-Ribiere): p = z + beta p, beta = (r.z new - z.r_old) / r.z (sc[2], sc[5], sc[0])
__global__ __launch_bounds__(kBlock) void fcg_dir_kernel(const double* __restrict__ sc,
    const double* __restrict__ z, double* p, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double beta = (sc[2] - sc[5]) / sc[0];
  p[i] = z[i] + beta * p[i];
}
__global__ void shift_kernel(double* sc) { sc[0] = sc[2]; }

void dot(const double* a, const double* b, int64_t n, double* partial, double* out, hipStream_t s)
{
  const unsigned g = unsigned(std::min<int64_t>(kMaxPartials, grid_for(n)));
  hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(kBlock), 0, s, a, b, n, partial);
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kBlock), 0, s, partial, int(g), out);
}
void axpby(double a, const double* x, double b, double* y, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, a, x, b, y, n);
}
void fcg_step(const double* sc, const double* p, const double* q, double* x, double* r, double* r_old,
    int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(fcg_step_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, sc, p, q, x, r, r_old, n);
}
void fcg_dir(const double* sc, const double* z, double* p, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(fcg_dir_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, sc, z, p, n);
}
void fcg_shift(double* sc, hipStream_t s) { hipLaunchKernelGGL(shift_kernel, dim3(1), dim3(1), 0, s, sc); }

// Block Gauss-Jordan inversion (no pivoting: the coarsest Galerkin operator is symmetric positive
// definite), kGJ pivots per step, A -> B out of place.  With the pivot block P = A[K, K], its row
// panel R = A[K, :] and column panel C = A[:, K]:
//   B[K, K] = P^-1,  B[K, j] = P^-1 R_j,  B[i, K] = -C_i P^-1,  B[i, j] = A_ij - C_i P^-1 R_j;
// after ceil(n / kGJ) steps the buffer holds A^-1.  Step part 1 (gj_panel_kernel): every
// workgroup inverts P in LDS (scalar Gauss-Jordan; a pivot that is not positive sets *bad), then
// W = P^-1 R for its 256 columns and the copy C of the column panel for its 256 rows (both zero
// beyond the last pivot of a short final block); workgroup 0 stores P^-1.  Part 2 (gj_update_kernel)
// forms B.
constexpr int kGJ = 32;

__global__ __launch_bounds__(kBlock) void gj_panel_kernel(const double* __restrict__ A, int64_t n, int64_t k0,
    double* __restrict__ Pinv, double* __restrict__ W, double* __restrict__ C, int32_t* bad)
{
  __shared__ double P[kGJ][kGJ + 1];
  const int t = threadIdx.x;
  const int b = int(min<int64_t>(kGJ, n - k0));
  for (int e = t; e < kGJ * kGJ; e += kBlock)
  {
    const int r = e / kGJ, c = e % kGJ;
    P[r][c] = (r < b && c < b) ? A[(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int m = 0; m < kGJ; ++m)
  {
    const double piv = P[m][m];
    double v[kGJ * kGJ / kBlock];
    const double inv = 1.0 / piv;
#pragma unroll
    for (int u = 0; u < kGJ * kGJ / kBlock; ++u)
    {
      const int e = t + kBlock * u, r = e / kGJ, c = e % kGJ;
      if (r == m) v[u] = c == m ? inv : P[m][c] * inv;
      else if (c == m) v[u] = -P[r][m] * inv;
      else v[u] = P[r][c] - P[r][m] * (P[m][c] * inv);
    }
    if (blockIdx.x == 0 && t == 0 && !(piv > 0.0)) *bad = 1;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kGJ * kGJ / kBlock; ++u)
    {
      const int e = t + kBlock * u;
      P[e / kGJ][e % kGJ] = v[u];
    }
    __syncthreads();
  }
  if (blockIdx.x == 0)
    for (int e = t; e < kGJ * kGJ; e += kBlock) Pinv[e] = P[e / kGJ][e % kGJ];
  const int64_t j = int64_t(blockIdx.x) * kBlock + t;
  if (j >= n) return;
  double w[kGJ];
#pragma unroll
  for (int m = 0; m < kGJ; ++m) w[m] = 0.0;
  for (int q = 0; q < b; ++q)
  {
    const double r = A[(k0 + q) * n + j];
#pragma unroll
    for (int m = 0; m < kGJ; ++m) w[m] += P[m][q] * r;
  }
#pragma unroll
  for (int m = 0; m < kGJ; ++m) W[int64_t(m) * n + j] = w[m];
#pragma unroll
  for (int m = 0; m < kGJ; ++m) C[j * kGJ + m] = m < b ? A[j * n + k0 + m] : 0.0;
}

// grid (ceil(n / kBlock), n): blockIdx.y = row i (its C_i is uniform over the workgroup)
__global__ __launch_bounds__(kBlock) void gj_update_kernel(const double* __restrict__ A, double* __restrict__ B,
    int64_t n, int64_t k0, const double* __restrict__ Pinv, const double* __restrict__ W,
    const double* __restrict__ C)
{
  const int64_t i = blockIdx.y;
  const int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  const int64_t ik = i - k0, jk = j - k0;
  const bool i_in = ik >= 0 && ik < kGJ && i < n, j_in = jk >= 0 && jk < kGJ;
  double v;
  if (i_in)
    v = j_in ? Pinv[ik * kGJ + jk] : W[ik * n + j];
  else
  {
    const double* c = C + i * kGJ;
    double s = 0.0;
    if (j_in)
    {
#pragma unroll
      for (int m = 0; m < kGJ; ++m) s += c[m] * Pinv[m * kGJ + jk];
      v = -s;
    }
    else
    {
#pragma unroll
      for (int m = 0; m < kGJ; ++m) s += c[m] * W[int64_t(m) * n + j];
      v = A[i * n + j] - s;
    }
  }
  B[i * n + j] = v;
}

// y = D x, D dense row-major n x n: one wavefront per row (fixed-order reduction)
__global__ __launch_bounds__(kBlock) void dense_mv_kernel(const double* __restrict__ D,
    const double* __restrict__ x, double* y, int64_t n)
{
  const int64_t row = int64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* d = D + row * n;
  double t = 0.0;
  for (int64_t j = lane; j < n; j += 64) t += d[j] * x[j];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) y[row] = t;
}

// largest eigenvalue of the Lanczos tridiagonal (bisection on the Sturm sequence)
double lanczos_lmax(const std::vector<double>& al, const std::vector<double>& be)
{
  const int k = int(al.size());
  std::vector<double> a(static_cast<size_t>(k)), e(static_cast<size_t>(k), 0.0);
  for (int i = 0; i < k; ++i)
  {
    a[size_t(i)] = 1.0 / al[size_t(i)] + (i > 0 ? be[size_t(i - 1)] / al[size_t(i - 1)] : 0.0);
    if (i + 1 < k) e[size_t(i)] = std::sqrt(be[size_t(i)]) / al[size_t(i)];
  }
  double hi = 0.0;
  for (int i = 0; i < k; ++i)
    hi = std::max(hi, a[size_t(i)] + (i > 0 ? std::fabs(e[size_t(i - 1)]) : 0.0) + (i + 1 < k ? std::fabs(e[size_t(i)]) : 0.0));
  double lo = 0.0;
  auto count_below = [&](double x) {  // eigenvalues < x
    int c = 0;
    double dd = 1.0;
    for (int i = 0; i < k; ++i)
    {
      dd = a[size_t(i)] - x - (i > 0 ? e[size_t(i - 1)] * e[size_t(i - 1)] / dd : 0.0);
      if (dd == 0.0) dd = -1e-300;
      if (dd < 0.0) ++c;
    }
    return c;
  };
  for (int it = 0; it < 200 && hi - lo > 1e-14 * hi; ++it)
  {
    const double mid = 0.5 * (lo + hi);
    if (count_below(mid) >= k) hi = mid;
    else lo = mid;
  }
  return hi;
}

// the dense coarsest level's launches
int64_t dense_inverse_work(int64_t n) { return 2 * kGJ * n + kGJ * kGJ; }

int dense_inverse(double* const buf[2], double* work, int64_t n, int32_t* d_flag, hipStream_t s)
{
  double *Pinv = work, *W = Pinv + kGJ * kGJ, *C = W + kGJ * n;
  const int64_t steps = (n + kGJ - 1) / kGJ;
  for (int64_t t = 0; t < steps; ++t)
  {
    const double* src = buf[t & 1];
    hipLaunchKernelGGL(gj_panel_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, src, n, t * kGJ, Pinv, W, C,
        d_flag);
    hipLaunchKernelGGL(gj_update_kernel, dim3(grid_for(n), unsigned(n)), dim3(kBlock), 0, s, src,
        buf[(t + 1) & 1], n, t * kGJ, Pinv, W, C);
  }
  return int(steps & 1);
}

void dense_mv(const double* D, const double* x, double* y, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(dense_mv_kernel, dim3(unsigned((n + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, s,
      D, x, y, n);
}

}  // namespace fcg_amgs
