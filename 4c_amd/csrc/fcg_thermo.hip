// fcg_thermo.hip -- the transient thermal field on the TSI context: the capacity matrix of the
// thermo element and the one-step-theta pass that turns k_TT and f_T into the effective tangent
// and the residual of a time step.
//
// Reference (paths relative to the 4C tree):
//   C        calc_thermo_fintcapa / linear_thermo_contribution: ecapa = sum_g capa fac N N^T with
//            capa = MAT_Fourier CAPA (4C_thermo_ele_impl.cpp:802-891, 4C_mat_fourier.cpp), the
//            element's own Gauss rule (DisTypeToOptGaussRule, 4C_thermo_ele_impl_utils.hpp:28-50)
//   OST      Thermo::TimIntOneStepTheta::evaluate_rhs_tang_residual (4C_thermo_timint_ost.cpp):
//            r = C (T_{n+1} - T_n)/dt + theta (F_int,n+1 - F_ext,n+1) + (1-theta)(F_int,n - F_ext,n),
//            tang = C/dt + theta K_TT; the element forms ecapa (T_{n+1} - T_n), never C T - C T_n
//
// Kernels: capacity_kernel (one wavefront per owned node: per incidence of the node, in ascending
// column-element order -- its element and local node are the context's inc_ele / inc_loc, uploaded
// by fcg_tsi_create from the host plan -- lane g forms det J and capa w det J N_a at Gauss point g, lane b sums over
// g in Gauss-point order and adds into the node's row image in LDS; the row is written once) and
// ost_combine_kernel (4 / 16 / 64 lanes per owned thermo row: K <- fma(theta, K, C/dt) and the row
// sum C (T - T_n) in one walk of the row).  Owned rows only, no atomics on doubles, bitwise
// reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "fcg_hex8_element.hpp"
#include "fcg_status.hpp"
#include "fcg_tsi_internal.hpp"
#include "fourc_gpu.h"

namespace fcg {
namespace {

constexpr int kOstBlock = 256;

int thermo_grid(int64_t work, int cap) { return int(work < cap ? (work > 0 ? work : 1) : cap); }

struct CapacityArgs {
  int64_t n_rownodes;
  const int64_t* inc_ptr;
  const int32_t* inc_ele;
  const uint8_t* inc_loc;
  const int32_t* rn_trow;
  const uint16_t* pos_tt;
  const int64_t* rowptr_tt;
  const int32_t* ele_nodes;
  const int32_t* ele_gid;
  const double* node_x;
  const double* tables;
  const double* ele_capa;  // [n_ele] or null
  double capa;
  double* Ctt;
  int32_t* err;
  int overwrite;
};

template <int NPE>
__global__ __launch_bounds__(64) void capacity_kernel(CapacityArgs A)
{
  constexpr int NGP = NPE;
  constexpr int MAXN = NPE == 8 ? 27 : 125;  // node neighbours of a row
  __shared__ double sN[NGP * NPE];  // [g][n]
  __shared__ double sX[NPE * 3];
  __shared__ double sfa[NGP];       // capa w det J N_a at the Gauss points
  __shared__ double img[MAXN];
  const int lane = threadIdx.x;
  const double* dNgp = A.tables;
  const double* Ngp = A.tables + NGP * NPE * 3;
  const double* wgp = Ngp + NGP * NPE + NPE * NPE * 3;
  for (int v = lane; v < NGP * NPE; v += 64) sN[v] = Ngp[v];

  for (int64_t r = blockIdx.x; r < A.n_rownodes; r += gridDim.x)
  {
    const int32_t trow = A.rn_trow[r];
    const int64_t btt = A.rowptr_tt[trow];
    const int ltt = int(A.rowptr_tt[trow + 1] - btt);
    for (int v = lane; v < MAXN; v += 64) img[v] = 0.0;
    for (int64_t q = A.inc_ptr[r]; q < A.inc_ptr[r + 1]; ++q)
    {
      const int32_t e = A.inc_ele[q];
      const int a = A.inc_loc[q];
      const int32_t* en = A.ele_nodes + int64_t(e) * NPE;
      __syncthreads();  // the previous incidence has read sX and sfa
      for (int v = lane; v < 3 * NPE; v += 64)
      {
        const int c = v / 3, d = v - 3 * c;
        sX[v] = A.node_x[3 * int64_t(en[c]) + d];
      }
      __syncthreads();
      if (lane < NGP)
      {
        // the Jacobian of tsi_element_kernel's Gauss-point stage, from the reference coordinates
        const double* dN = dNgp + 3 * NPE * lane;
        double J[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) J[k] = 0.0;
        for (int c = 0; c < NPE; ++c)
        {
          const double d0 = dN[3 * c], d1 = dN[3 * c + 1], d2 = dN[3 * c + 2];
          const double x0 = sX[3 * c], x1 = sX[3 * c + 1], x2 = sX[3 * c + 2];
          J[0] += d0 * x0; J[1] += d1 * x0; J[2] += d2 * x0;
          J[3] += d0 * x1; J[4] += d1 * x1; J[5] += d2 * x1;
          J[6] += d0 * x2; J[7] += d1 * x2; J[8] += d2 * x2;
        }
        const double det = h8_invert3x3(J);
        // eval_shape_func_and_derivs_at_int_point (4C_thermo_ele_impl.cpp:2663-2664)
        const int bad = det == 0.0 ? int(FCG_ERR_SINGULAR) : det < 1e-16 ? int(FCG_ERR_NODAL_DETJ) : 0;
        if (bad)
        {
          atomicMax(&A.err[0], bad);
          atomicMin(&A.err[1], A.ele_gid[e]);
        }
        const double c = A.ele_capa ? A.ele_capa[e] : A.capa;
        sfa[lane] = c * (det * wgp[lane]) * sN[NPE * lane + a];
      }
      __syncthreads();
      if (lane < NPE)
      {
        double s = 0.0;
        for (int g = 0; g < NGP; ++g) s += sfa[g] * sN[NPE * g + lane];
        img[A.pos_tt[q * NPE + lane]] += s;  // the nodes of an element have distinct columns
      }
    }
    __syncthreads();
    for (int v = lane; v < ltt; v += 64)
    {
      if (A.overwrite)
        A.Ctt[btt + v] = img[v];
      else
        A.Ctt[btt + v] += img[v];
    }
    __syncthreads();
  }
}

// K_TT[j] <- fma(theta, K_TT[j], C[j] / dt);  f_T[i] <- theta f_T[i] + (1/dt) sum_j C_ij (T_j - Tn_j) + h_i
template <int LPR>
__global__ __launch_bounds__(kOstBlock) void ost_combine_kernel(int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ C, const double* __restrict__ T,
    const double* __restrict__ Tn, const double* __restrict__ h, double* __restrict__ K,
    double* __restrict__ f, double theta, double dt, double inv_dt)
{
  const int lane = threadIdx.x % LPR;
  const int64_t i = (int64_t(blockIdx.x) * kOstBlock + threadIdx.x) / LPR;
  const bool tail = f && i < n && lane == 0;
  const double fi = tail ? f[i] : 0.0;  // before the row walk
  const double hi = tail && h ? h[i] : 0.0;
  double a = 0.0;
  if (i < n)
  {
    const int64_t e = ptr[i + 1];
    for (int64_t k = ptr[i] + lane; k < e; k += LPR)
    {
      const double c = C[k];
      if (f)
      {
        const int32_t j = col[k];
        a += c * (T[j] - Tn[j]);
      }
      if (K) K[k] = fma(theta, K[k], c / dt);
    }
  }
  if (!f) return;  // uniform over the grid
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o, LPR);
  if (tail) f[i] = fma(theta, fi, inv_dt * a) + hi;
}

}  // namespace
}  // namespace fcg

extern "C" {

int fcg_tsi_capacity(fcg_tsi_ctx* ctx, double capa, const double* ele_capa, int mode, double* d_Ctt,
    void* stream_ptr, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::TsiDevice& d = ctx->d;
  if ((mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE) || (d.nnz_tt > 0 && !d_Ctt))
  {
    ctx->last_error = "invalid capacity arguments";
    return FCG_ERR_ARG;
  }
  // Mat::PAR::Fourier: a heat capacity that is not positive has no capacity matrix
  if (ele_capa)
  {
    for (int64_t e = 0; e < d.n_ele; ++e)
      if (!(ele_capa[e] > 0.0) || !std::isfinite(ele_capa[e]))
      {
        ctx->last_error = "ele_capa[" + std::to_string(e) + "] = " + std::to_string(ele_capa[e]) +
                          ": the heat capacity must be positive and finite";
        return FCG_ERR_ARG;
      }
  }
  else if (!(capa > 0.0) || !std::isfinite(capa))
  {
    ctx->last_error = "capa = " + std::to_string(capa) + ": the heat capacity must be positive and finite";
    return FCG_ERR_ARG;
  }
  if (d.n_rownodes == 0) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  hipError_t he = hipSuccess;
  if (ele_capa && d.n_ele > 0)
  {
    if (!d.ele_capa)
    {
      he = hipMalloc(reinterpret_cast<void**>(&d.ele_capa), sizeof(double) * d.n_ele);
      if (he == hipSuccess) ctx->device_bytes += int64_t(sizeof(double)) * d.n_ele;
    }
    // a blocking copy: the caller's table may go away after the call
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hipMemcpy(d.ele_capa, ele_capa, sizeof(double) * d.n_ele, hipMemcpyHostToDevice);
  }
  const int32_t init[2] = {0, INT32_MAX};
  if (he == hipSuccess) he = hipMemcpyAsync(d.err, init, sizeof(init), hipMemcpyHostToDevice, s);
  if (he == hipSuccess)
  {
    fcg::CapacityArgs a;
    a.n_rownodes = d.n_rownodes;
    a.inc_ptr = d.inc_ptr;
    a.inc_ele = d.inc_ele;
    a.inc_loc = d.inc_loc;
    a.rn_trow = d.rn_trow;
    a.pos_tt = d.pos_tt;
    a.rowptr_tt = d.rowptr_tt;
    a.ele_nodes = d.ele_nodes;
    a.ele_gid = d.ele_gid;
    a.node_x = d.node_x;
    a.tables = d.tables;
    a.ele_capa = ele_capa ? d.ele_capa : nullptr;
    a.capa = capa;
    a.Ctt = d_Ctt;
    a.err = d.err;
    a.overwrite = mode == FCG_OVERWRITE;
    const int grid = fcg::thermo_grid(d.n_rownodes, 256 * 32);
    if (d.npe == 8)
      hipLaunchKernelGGL(fcg::capacity_kernel<8>, dim3(grid), dim3(64), 0, s, a);
    else
      hipLaunchKernelGGL(fcg::capacity_kernel<27>, dim3(grid), dim3(64), 0, s, a);
    he = hipGetLastError();
  }
  int32_t errv[2] = {0, INT32_MAX};
  if (he == hipSuccess) he = hipMemcpyAsync(errv, d.err, sizeof(errv), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (errv[0] != 0)
  {
    const int32_t gid = errv[1] == INT32_MAX ? -1 : errv[1];
    if (bad_ele_gid) *bad_ele_gid = gid;
    ctx->last_error = errv[0] == FCG_ERR_NODAL_DETJ
                          ? "non-positive jacobian determinant in element " + std::to_string(gid)
                          : "singular 3x3 matrix in element " + std::to_string(gid);
    return errv[0];
  }
  return FCG_OK;
}

int fcg_tsi_ost_combine(fcg_tsi_ctx* ctx, double theta, double dt, const double* d_Ctt,
    const double* d_T_col, const double* d_Tn_col, const double* d_h_row, double* d_Ktt,
    double* d_fT_row, void* stream_ptr)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::TsiDevice& d = ctx->d;
  if (!(theta > 0.0 && theta <= 1.0) || !std::isfinite(dt) || !(dt > 0.0))
  {
    ctx->last_error = "one-step-theta needs theta in (0, 1] and a finite dt > 0";
    return FCG_ERR_ARG;
  }
  if (d.n_rows_t == 0) return FCG_OK;
  if ((!d_Ktt && !d_fT_row) || (d.nnz_tt > 0 && !d_Ctt) || (d_fT_row && (!d_T_col || !d_Tn_col)))
  {
    ctx->last_error = "invalid one-step-theta arguments: no output, or an input missing";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  const int64_t n = d.n_rows_t;
  // lanes per row by the longest row, as the scalar CSR kernels choose them (fcg_samg.hip)
  const int lanes = d.max_row_tt <= 8 ? 4 : d.max_row_tt <= 48 ? 16 : 64;
  const unsigned blocks = unsigned((n * lanes + fcg::kOstBlock - 1) / fcg::kOstBlock);
  const double inv_dt = 1.0 / dt;
  if (lanes == 4)
    hipLaunchKernelGGL(fcg::ost_combine_kernel<4>, dim3(blocks), dim3(fcg::kOstBlock), 0, s, n, d.rowptr_tt,
        d.cols_tt, d_Ctt, d_T_col, d_Tn_col, d_h_row, d_Ktt, d_fT_row, theta, dt, inv_dt);
  else if (lanes == 16)
    hipLaunchKernelGGL(fcg::ost_combine_kernel<16>, dim3(blocks), dim3(fcg::kOstBlock), 0, s, n, d.rowptr_tt,
        d.cols_tt, d_Ctt, d_T_col, d_Tn_col, d_h_row, d_Ktt, d_fT_row, theta, dt, inv_dt);
  else
    hipLaunchKernelGGL(fcg::ost_combine_kernel<64>, dim3(blocks), dim3(fcg::kOstBlock), 0, s, n, d.rowptr_tt,
        d.cols_tt, d_Ctt, d_T_col, d_Tn_col, d_h_row, d_Ktt, d_fT_row, theta, dt, inv_dt);
  if (hipGetLastError() != hipSuccess)
  {
    ctx->last_error = "HIP: the one-step-theta kernel did not launch";
    return fcg_device_error();
  }
  return FCG_OK;
}

}  // extern "C"
