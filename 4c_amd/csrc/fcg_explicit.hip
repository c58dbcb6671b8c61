// fcg_explicit.hip -- explicit structural dynamics (DYNAMICTYPE CentrDiff): the vector update of
// one central-difference step in one pass, and a rigorous bound on the stable time step.
//
// Reference: Solid::EXPLICIT::CentrDiff (4C_structure_new_expl_centrdiff.cpp) advances
//   v_{n+1/2} = v_n + dt/2 a_n,  d_{n+1} = d_n + dt v_{n+1/2},  evaluate f_int(d_{n+1}),
//   a_{n+1} = M^-1 (f_ext - f_int - f_visc),  v_{n+1} = v_{n+1/2} + dt/2 a_{n+1}
// with a lumped M.  Written as one pass per evaluate -- what follows an evaluate and what precedes
// the next one are both row-local -- the step is, per free row,
//   a = (fext - fint) / m - damp_m vhalf,  v = vhalf + dt_prev/2 a,
//   vhalf' = v + dt_next/2 a,  d' = d + dt_next vhalf'
// (include/fourc_gpu.h has the contract).
//
//  * centrdiff_kernel: a stream of 6 reads and up to 5 writes per row, two rows (16 bytes) per
//    lane when every pointer is 16-byte aligned, else one; grid-stride, grid capped at
//    kExplicitPartials workgroups; the row count's odd last row goes to thread 0.  With d_ekin
//    each workgroup leaves the sum of its m v^2 in the context's partial buffer (lanes in a fixed
//    order) and sum_partials_kernel adds the partials in index order.
//  * rowbound_kernel: LPR lanes per row sum |K_ij| over the row's entries (ghost columns
//    included), divide by the row's mass and keep the maximum; max_partials_kernel takes the
//    maximum of the workgroups' partials.
// No atomics on doubles anywhere: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <limits>
#include <string>

#include "fcg_internal.hpp"
#include "fcg_status.hpp"

namespace fcg {

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t work)
{
  const int64_t g = (work + kBlock - 1) / kBlock;
  return int(g < 1 ? 1 : (g > kExplicitPartials ? kExplicitPartials : g));
}

// the workgroup's sum (MAX: maximum) of v in a fixed order: the lanes of a wavefront by halving
// distances, then the wavefronts in index order; the result is valid in thread 0
template <bool MAX>
__device__ inline double block_reduce(double v)
{
  __shared__ double part[kBlock / 64];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
  {
    const double w = __shfl_down(v, o, 64);
    v = MAX ? fmax(v, w) : v + w;
  }
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = v;
  __syncthreads();
  double r = part[0];
  for (int k = 1; k < kBlock / 64; ++k) r = MAX ? fmax(r, part[k]) : r + part[k];
  return r;
}

// ---------------------------------------------------------------------------- the step
struct StepArgs {
  const double* fext;
  const double* fint;
  const double* m;
  const uint8_t* fixed;  // or NULL
  double* d;
  double* vhalf;
  double* v;        // or NULL
  double* a;        // or NULL
  double* partial;  // [gridDim.x], EKIN only
  int64_t n;
  double hdt_prev, hdt_next, dt_next, damp_m;  // hdt = dt / 2
};

// one row: (d, vh) advance in place, v and a come back; returns m v^2
__device__ inline double step_row(const StepArgs& A, double fe, double fi, double m, bool fixed,
    double& d, double& vh, double& v, double& a)
{
  if (fixed)
  {
    a = v = vh = 0.0;
    return 0.0;
  }
  a = (fe - fi) / m - A.damp_m * vh;
  v = vh + A.hdt_prev * a;
  vh = v + A.hdt_next * a;
  d = d + A.dt_next * vh;
  return m * v * v;
}

template <bool VEC, bool EKIN>
__global__ __launch_bounds__(kBlock) void centrdiff_kernel(StepArgs A)
{
  const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  double e = 0.0;
  if (VEC)
  {
    const int64_t n2 = A.n / 2;
    const double2* fe = reinterpret_cast<const double2*>(A.fext);
    const double2* fi = reinterpret_cast<const double2*>(A.fint);
    const double2* mm = reinterpret_cast<const double2*>(A.m);
    const uint16_t* fx = reinterpret_cast<const uint16_t*>(A.fixed);
    double2* dd = reinterpret_cast<double2*>(A.d);
    double2* hh = reinterpret_cast<double2*>(A.vhalf);
    for (int64_t i = gid; i < n2; i += stride)
    {
      const double2 f0 = fe[i], f1 = fi[i], m = mm[i];
      double2 d = dd[i], h = hh[i], v, a;
      const unsigned fix = fx ? fx[i] : 0u;
      e += step_row(A, f0.x, f1.x, m.x, (fix & 0xffu) != 0, d.x, h.x, v.x, a.x);
      e += step_row(A, f0.y, f1.y, m.y, (fix >> 8) != 0, d.y, h.y, v.y, a.y);
      dd[i] = d;
      hh[i] = h;
      if (A.v) reinterpret_cast<double2*>(A.v)[i] = v;
      if (A.a) reinterpret_cast<double2*>(A.a)[i] = a;
    }
  }
  // VEC: the last row of an odd count, by thread 0; else every row
  const int64_t first = !VEC ? gid : (gid == 0 ? (A.n & ~int64_t(1)) : A.n);
  for (int64_t i = first; i < A.n; i += stride)
  {
    double d = A.d[i], h = A.vhalf[i], v, a;
    e += step_row(A, A.fext[i], A.fint[i], A.m[i], A.fixed && A.fixed[i] != 0, d, h, v, a);
    A.d[i] = d;
    A.vhalf[i] = h;
    if (A.v) A.v[i] = v;
    if (A.a) A.a[i] = a;
  }
  if (EKIN)
  {
    e = block_reduce<false>(e);
    if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
  }
}

// out = scale * sum_k partial[k] (MAX: max_k partial[k]), k in index order per thread, one workgroup
template <bool MAX>
__global__ __launch_bounds__(kBlock) void fold_partials_kernel(const double* __restrict__ partial,
    int n, double scale, double* out)
{
  double s = 0.0;  // the partials of the row bound are >= 0
  for (int k = threadIdx.x; k < n; k += kBlock) s = MAX ? fmax(s, partial[k]) : s + partial[k];
  s = block_reduce<MAX>(s);
  if (threadIdx.x == 0) *out = MAX ? s : scale * s;
}

// ---------------------------------------------------------------------------- the row bound
// Every pass of the loop takes kBlock / LPR consecutive rows per workgroup, so the rows of a
// wavefront are neighbours in the CSR values; all lanes run the same number of passes (the
// shuffles are never inside divergent code).  A refused row sets the solver flag word and leaves
// the lowest such row in bad_row.
template <int LPR>
__global__ __launch_bounds__(kBlock) void rowbound_kernel(const int64_t* __restrict__ rowptr,
    const double* __restrict__ K, const double* __restrict__ m, const uint8_t* __restrict__ fixed,
    int64_t n_rows, double* partial, int32_t* flag, int32_t* bad_row)
{
  constexpr int kRows = kBlock / LPR;
  const int lane = threadIdx.x % LPR;
  double best = 0.0;
  for (int64_t base = int64_t(blockIdx.x) * kRows; base < n_rows; base += int64_t(gridDim.x) * kRows)
  {
    const int64_t r = base + threadIdx.x / LPR;
    const bool live = r < n_rows && !(fixed && fixed[r] != 0);
    const int64_t s = live ? rowptr[r] : 0, e = live ? rowptr[r + 1] : 0;
    double sum = 0.0;
    for (int64_t j = s + lane; j < e; j += LPR) sum += fabs(K[j]);
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, LPR);
    if (live)
    {
      const double mi = m[r];
      const double q = sum / mi;
      if (mi > 0.0 && isfinite(mi) && isfinite(q)) best = fmax(best, q);  // q finite: sum is
      else if (lane == 0)
      {
        atomicMax(flag, 1);
        atomicMin(bad_row, int32_t(r));
      }
    }
  }
  best = block_reduce<true>(best);
  if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

hipError_t ensure_work(DeviceMesh& m, int64_t& bytes)
{
  if (m.explicit_work) return hipSuccess;
  const size_t nb = sizeof(double) * size_t(kExplicitPartials + 2);
  const hipError_t he = hipMalloc(reinterpret_cast<void**>(&m.explicit_work), nb);
  if (he != hipSuccess)
  {
    m.explicit_work = nullptr;
    return he;
  }
  bytes += int64_t(nb);
  return hipSuccess;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

}  // namespace fcg

extern "C" {

int fcg_centrdiff_step(fcg_ctx* ctx, double dt_prev, double dt_next, double damp_m,
    const double* d_fext_row, const double* d_fint_row, const double* d_m_lumped_row,
    const uint8_t* d_fixed_row, double* d_d_row, double* d_vhalf_row, double* d_v_row,
    double* d_a_row, double* d_ekin, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!(dt_prev >= 0.0) || !(dt_next >= 0.0) || !(damp_m >= 0.0) || !std::isfinite(dt_prev) ||
      !std::isfinite(dt_next) || !std::isfinite(damp_m))
  {
    ctx->last_error = "fcg_centrdiff_step: dt_prev, dt_next and damp_m must be finite and >= 0";
    return FCG_ERR_ARG;
  }
  fcg::DeviceMesh& m = ctx->mesh;
  if (m.n_rows == 0) return FCG_OK;
  if (!d_fext_row || !d_fint_row || !d_m_lumped_row || !d_d_row || !d_vhalf_row)
  {
    ctx->last_error = "fcg_centrdiff_step: d_fext_row, d_fint_row, d_m_lumped_row, d_d_row or "
                      "d_vhalf_row is NULL";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  hipError_t he = d_ekin ? fcg::ensure_work(m, ctx->device_bytes) : hipSuccess;
  if (he == hipSuccess)
  {
    fcg::StepArgs A;
    A.fext = d_fext_row;
    A.fint = d_fint_row;
    A.m = d_m_lumped_row;
    A.fixed = d_fixed_row;
    A.d = d_d_row;
    A.vhalf = d_vhalf_row;
    A.v = d_v_row;
    A.a = d_a_row;
    A.partial = m.explicit_work;
    A.n = m.n_rows;
    A.hdt_prev = 0.5 * dt_prev;
    A.hdt_next = 0.5 * dt_next;
    A.dt_next = dt_next;
    A.damp_m = damp_m;
    // 16 bytes per lane needs every vector on a 16-byte boundary (NULL is) and the mask on a
    // 2-byte one; a view that starts at an odd double falls back to one row per lane
    const bool vec = m.n_rows >= 2 && fcg::aligned16(d_fext_row) && fcg::aligned16(d_fint_row) &&
                     fcg::aligned16(d_m_lumped_row) && fcg::aligned16(d_d_row) &&
                     fcg::aligned16(d_vhalf_row) && fcg::aligned16(d_v_row) &&
                     fcg::aligned16(d_a_row) && (reinterpret_cast<uintptr_t>(d_fixed_row) & 1u) == 0;
    const int grid = fcg::grid_for(vec ? m.n_rows / 2 : m.n_rows);
#define FCG_STEP(VEC, EKIN) \
  hipLaunchKernelGGL((fcg::centrdiff_kernel<VEC, EKIN>), dim3(grid), dim3(fcg::kBlock), 0, s, A)
    if (vec)
    {
      if (d_ekin) FCG_STEP(true, true);
      else FCG_STEP(true, false);
    }
    else
    {
      if (d_ekin) FCG_STEP(false, true);
      else FCG_STEP(false, false);
    }
#undef FCG_STEP
    he = hipGetLastError();
    if (he == hipSuccess && d_ekin)
    {
      hipLaunchKernelGGL((fcg::fold_partials_kernel<false>), dim3(1), dim3(fcg::kBlock), 0, s,
          m.explicit_work, grid, 0.5, d_ekin);
      he = hipGetLastError();
    }
  }
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("fcg_centrdiff_step: HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  return FCG_OK;
}

int fcg_stable_dt(fcg_ctx* ctx, const double* d_K_vals, const double* d_m_lumped_row,
    const uint8_t* d_fixed_row, double* lambda_bound, double* dt_crit, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (lambda_bound) *lambda_bound = 0.0;
  if (dt_crit) *dt_crit = std::numeric_limits<double>::infinity();
  fcg::DeviceMesh& m = ctx->mesh;
  if (m.n_rows == 0) return FCG_OK;
  if (!d_K_vals || !d_m_lumped_row)
  {
    ctx->last_error = "fcg_stable_dt: d_K_vals or d_m_lumped_row is NULL";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  hipError_t he = fcg::ensure_work(m, ctx->device_bytes);
  int32_t* flag = m.err + 2;  // the solver flag word: evaluate's sticky flags are left alone
  double* d_lambda = m.explicit_work ? m.explicit_work + fcg::kExplicitPartials : nullptr;
  int32_t* d_bad = reinterpret_cast<int32_t*>(d_lambda + 1);
  double lambda = 0.0, bad_mass = 0.0;
  int32_t bad = 0, bad_row = INT32_MAX;
  if (he == hipSuccess) he = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
  if (he == hipSuccess) he = hipMemsetAsync(d_bad, 0x7f, sizeof(int32_t), s);
  if (he == hipSuccess)
  {
    // hex27 rows hold up to 375 entries, hex8 rows up to 81
    const int lpr = m.npe == 27 ? 64 : 16;
    const int rows_per_block = fcg::kBlock / lpr;
    const int64_t g = (m.n_rows + rows_per_block - 1) / rows_per_block;
    const int grid = int(g > fcg::kExplicitPartials ? fcg::kExplicitPartials : g);
    if (lpr == 64)
      hipLaunchKernelGGL((fcg::rowbound_kernel<64>), dim3(grid), dim3(fcg::kBlock), 0, s, m.rowptr,
          d_K_vals, d_m_lumped_row, d_fixed_row, m.n_rows, m.explicit_work, flag, d_bad);
    else
      hipLaunchKernelGGL((fcg::rowbound_kernel<16>), dim3(grid), dim3(fcg::kBlock), 0, s, m.rowptr,
          d_K_vals, d_m_lumped_row, d_fixed_row, m.n_rows, m.explicit_work, flag, d_bad);
    he = hipGetLastError();
    if (he == hipSuccess)
    {
      hipLaunchKernelGGL((fcg::fold_partials_kernel<true>), dim3(1), dim3(fcg::kBlock), 0, s,
          m.explicit_work, grid, 1.0, d_lambda);
      he = hipGetLastError();
    }
  }
  if (he == hipSuccess) he = hipMemcpyAsync(&lambda, d_lambda, sizeof(lambda), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipMemcpyAsync(&bad_row, d_bad, sizeof(bad_row), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he == hipSuccess && bad && bad_row >= 0 && bad_row < m.n_rows)
    he = hipMemcpy(&bad_mass, d_m_lumped_row + bad_row, sizeof(bad_mass), hipMemcpyDeviceToHost);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("fcg_stable_dt: HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (bad)
  {
    ctx->last_error = "fcg_stable_dt: free row " + std::to_string(bad_row) + ": ";
    if (!(bad_mass > 0.0) || !std::isfinite(bad_mass))
      ctx->last_error += "m_lumped = " + std::to_string(bad_mass) + " is not positive and finite";
    else
      ctx->last_error += "sum_j |K_ij| / m_lumped is not finite";
    return FCG_ERR_ARG;
  }
  if (lambda_bound) *lambda_bound = lambda;
  if (dt_crit && lambda > 0.0) *dt_crit = 2.0 / std::sqrt(lambda);
  return FCG_OK;
}

}  // extern "C"
