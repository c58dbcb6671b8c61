// fcg_tsi_solve.hip -- the monolithic TSI system [[K_SS, K_ST], [K_TS, K_TT]] as an operator on
// the device and its solve by FGMRES (fcg_krylov.hip) with a 2 x 2 block preconditioner: what
// TSI::Monolithic::linear_solve hands to Belos GMRES (4C_tsi_monolithic.cpp:1040-1130) with the
// block Gauss-Seidel of 4C's block preconditioners (BGS, 4C_linear_solver_preconditioner_block.cpp).
//
// Block layout.  With node-consistent numbering (thermo LID t = structural LID / 3, verified by
// fcg_tsi_create) all four blocks hang on the k_TT node graph: node t with neighbour list
// col_tt[b .. b + l), b = rowptr_tt[t], has
//   K_SS  rows 3t + d at 9 b + 3 d l, entry 3 k + e for neighbour k, column DOF e
//   K_ST  rows 3t + d at 3 b + d l,   entry k
//   K_TS  row  t      at 3 b,         entry 3 k + e
//   K_TT  row  t      at b,           entry k
// so the operator reads one index per neighbour node and 16 values, and no other index array.
// The Krylov vectors are stacked [x_S (3 nn); x_T (nn)].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "fcg_internal.hpp"
#include "fcg_krylov.hpp"
#include "fcg_status.hpp"
#include "fcg_tsi_internal.hpp"

namespace fcg {
namespace {

constexpr int kBlock = 256;

inline unsigned blocks_for(int64_t n) { return unsigned(std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }

// y_S = K_SS x_S + K_ST x_T, y_T = K_TS x_S + K_TT x_T: LPN lanes per owned node stride over its
// neighbours, the four row sums are reduced over the lanes in a fixed (butterfly) order
template <int LPN>
__global__ __launch_bounds__(kBlock) void tsi_block_apply_kernel(const int64_t* __restrict__ rp_tt,
    const int32_t* __restrict__ col_tt, const double* __restrict__ Kss, const double* __restrict__ Kst,
    const double* __restrict__ Kts, const double* __restrict__ Ktt, const double* __restrict__ xs,
    const double* __restrict__ xt, double* __restrict__ ys, double* __restrict__ yt, int64_t nn)
{
  const int lane = threadIdx.x % LPN;
  const int64_t t = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPN;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (t < nn)
  {
    const int64_t b = rp_tt[t];
    const int l = int(rp_tt[t + 1] - b);
    const double* s0 = Kss + 9 * b;
    const double* s1 = s0 + 3 * l;
    const double* s2 = s1 + 3 * l;
    const double* c0 = Kst + 3 * b;
    const double* c1 = c0 + l;
    const double* c2 = c1 + l;
    const double* ts = Kts + 3 * b;
    const double* tt = Ktt + b;
    for (int k = lane; k < l; k += LPN)
    {
      const int64_t c = col_tt[b + k];
      const double x0 = xs[3 * c], x1 = xs[3 * c + 1], x2 = xs[3 * c + 2], xT = xt[c];
      a0 += s0[3 * k] * x0 + s0[3 * k + 1] * x1 + s0[3 * k + 2] * x2 + c0[k] * xT;
      a1 += s1[3 * k] * x0 + s1[3 * k + 1] * x1 + s1[3 * k + 2] * x2 + c1[k] * xT;
      a2 += s2[3 * k] * x0 + s2[3 * k + 1] * x1 + s2[3 * k + 2] * x2 + c2[k] * xT;
      a3 += ts[3 * k] * x0 + ts[3 * k + 1] * x1 + ts[3 * k + 2] * x2 + tt[k] * xT;
    }
  }
#pragma unroll
  for (int o = LPN / 2; o >= 1; o >>= 1)
  {
    a0 += __shfl_xor(a0, o, LPN);
    a1 += __shfl_xor(a1, o, LPN);
    a2 += __shfl_xor(a2, o, LPN);
    a3 += __shfl_xor(a3, o, LPN);
  }
  if (t < nn && lane == 0)
  {
    ys[3 * t] = a0;
    ys[3 * t + 1] = a1;
    ys[3 * t + 2] = a2;
    yt[t] = a3;
  }
}

// r = b - A x on the stacked vectors with the compensated product (fcg_krylov.hpp), 16 lanes per
// stacked row: a structural row 3t + d takes its K_SS and K_ST entries, a thermal row t its K_TS
// and K_TT entries, over the node's neighbour list
__global__ __launch_bounds__(kBlock) void tsi_residual_kernel(const int64_t* __restrict__ rp_tt,
    const int32_t* __restrict__ col_tt, const double* __restrict__ Kss, const double* __restrict__ Kst,
    const double* __restrict__ Kts, const double* __restrict__ Ktt, const double* __restrict__ x,
    const double* __restrict__ b, double* __restrict__ r, int64_t nn)
{
  constexpr int LPR = 16;
  const int lane = threadIdx.x % LPR;
  const int64_t i = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPR;
  const int64_t ns = 3 * nn;
  const double* xs = x;
  const double* xt = x + ns;
  double s = 0.0, c = 0.0;
  if (i < 4 * nn)
  {
    const bool thermal = i >= ns;
    const int64_t t = thermal ? i - ns : i / 3;
    const int64_t d = thermal ? 0 : i - 3 * t;
    const int64_t bb = rp_tt[t];
    const int l = int(rp_tt[t + 1] - bb);
    const double* k3 = thermal ? Kts + 3 * bb : Kss + 9 * bb + 3 * d * l;
    const double* k1 = thermal ? Ktt + bb : Kst + 3 * bb + d * l;
    for (int k = lane; k < l; k += LPR)
    {
      const int64_t cc = col_tt[bb + k];
      dd_fma(s, c, k3[3 * k], xs[3 * cc]);
      dd_fma(s, c, k3[3 * k + 1], xs[3 * cc + 1]);
      dd_fma(s, c, k3[3 * k + 2], xs[3 * cc + 2]);
      dd_fma(s, c, k1[k], xt[cc]);
    }
  }
  const double v = dd_row_residual<LPR>(s, c, i < 4 * nn ? b[i] : 0.0);
  if (i < 4 * nn && lane == 0) r[i] = v;
}

// the thermal half of the block preconditioner: z_T = D_TT^-1 (r_T - [bgs] K_TS z_S), one pass
// over K_TS fused with the scaling
template <int LPN>
__global__ __launch_bounds__(kBlock) void tsi_thermal_precond_kernel(const int64_t* __restrict__ rp_tt,
    const int32_t* __restrict__ col_tt, const double* __restrict__ Kts, const double* __restrict__ dtt,
    const double* __restrict__ rT, const double* __restrict__ zS, double* __restrict__ zT, int64_t nn,
    int bgs)
{
  const int lane = threadIdx.x % LPN;
  const int64_t t = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPN;
  double a = 0.0;
  if (bgs && t < nn)
  {
    const int64_t b = rp_tt[t];
    const int l = int(rp_tt[t + 1] - b);
    const double* ts = Kts + 3 * b;
    for (int k = lane; k < l; k += LPN)
    {
      const int64_t c = col_tt[b + k];
      a += ts[3 * k] * zS[3 * c] + ts[3 * k + 1] * zS[3 * c + 1] + ts[3 * k + 2] * zS[3 * c + 2];
    }
  }
#pragma unroll
  for (int o = LPN / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o, LPN);
  if (t < nn && lane == 0) zT[t] = dtt[t] * (rT[t] - a);
}

// w_T = r_T - K_TS z_S in one pass over K_TS: the right-hand side of the thermal V-cycle under the
// block Gauss-Seidel preconditioner (fcg_tsi_gmres_solve_amg with amg_t)
template <int LPN>
__global__ __launch_bounds__(kBlock) void tsi_thermal_rhs_kernel(const int64_t* __restrict__ rp_tt,
    const int32_t* __restrict__ col_tt, const double* __restrict__ Kts, const double* __restrict__ rT,
    const double* __restrict__ zS, double* __restrict__ wT, int64_t nn)
{
  const int lane = threadIdx.x % LPN;
  const int64_t t = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPN;
  double a = 0.0;
  if (t < nn)
  {
    const int64_t b = rp_tt[t];
    const int l = int(rp_tt[t + 1] - b);
    const double* ts = Kts + 3 * b;
    for (int k = lane; k < l; k += LPN)
    {
      const int64_t c = col_tt[b + k];
      a += ts[3 * k] * zS[3 * c] + ts[3 * k + 1] * zS[3 * c + 1] + ts[3 * k + 2] * zS[3 * c + 2];
    }
  }
#pragma unroll
  for (int o = LPN / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o, LPN);
  if (t < nn && lane == 0) wT[t] = rT[t] - a;
}

// dtt[t] = 1 / K_TT(t, t); a missing, zero or non-finite diagonal entry sets the flag
__global__ __launch_bounds__(kBlock) void tsi_dtt_kernel(const int64_t* __restrict__ rp_tt,
    const int32_t* __restrict__ col_tt, const double* __restrict__ Ktt, double* __restrict__ dtt,
    int64_t nn, int32_t* flag)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nn) return;
  double d = 0.0;
  for (int64_t j = rp_tt[t]; j < rp_tt[t + 1]; ++j)
    if (col_tt[j] == t) d = Ktt[j];
  const double inv = 1.0 / d;
  if (d == 0.0 || !isfinite(inv))
  {
    atomicMax(flag, 1);
    dtt[t] = 0.0;
    return;
  }
  dtt[t] = inv;
}

// Dirichlet rows, one wavefront per listed row: the first n_s entries are structural rows (K_ST
// row := 0), the others thermal rows (K_TS row := 0, K_TT row := unit row, rhs_T := 0).
// flag 2: a row outside the map; 1: a thermal row without a diagonal entry (left untouched).
struct TsiDbcArgs {
  int64_t n_s, n_t, n_rows_s, n_rows_t;
  const int32_t* rows_s;
  const int32_t* rows_t;
  const int64_t* rp_st;
  const int64_t* rp_ts;
  const int64_t* rp_tt;
  const int32_t* col_tt;
  double *Kst, *Kts, *Ktt, *rhsT;
  int32_t* flag;
};

__global__ __launch_bounds__(kBlock) void tsi_dirichlet_kernel(TsiDbcArgs A)
{
  const int64_t k = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (k >= A.n_s + A.n_t) return;
  if (k < A.n_s)
  {
    const int32_t r = A.rows_s[k];
    if (r < 0 || r >= A.n_rows_s)
    {
      if (lane == 0) atomicMax(A.flag, 2);
      return;
    }
    if (A.Kst)
      for (int64_t j = A.rp_st[r] + lane; j < A.rp_st[r + 1]; j += 64) A.Kst[j] = 0.0;
    return;
  }
  const int32_t t = A.rows_t[k - A.n_s];
  if (t < 0 || t >= A.n_rows_t)
  {
    if (lane == 0) atomicMax(A.flag, 2);
    return;
  }
  int found = 0;
  for (int64_t j = A.rp_tt[t] + lane; j < A.rp_tt[t + 1]; j += 64) found |= A.col_tt[j] == t;
  if (!__any(found))
  {
    if (lane == 0) atomicMax(A.flag, 1);
    return;
  }
  if (A.Kts)
    for (int64_t j = A.rp_ts[t] + lane; j < A.rp_ts[t + 1]; j += 64) A.Kts[j] = 0.0;
  if (A.Ktt)
    for (int64_t j = A.rp_tt[t] + lane; j < A.rp_tt[t + 1]; j += 64) A.Ktt[j] = A.col_tt[j] == t ? 1.0 : 0.0;
  if (A.rhsT && lane == 0) A.rhsT[t] = 0.0;
}

// the structural context's CSR graph is the 3 x 3 expansion of the k_TT graph
__global__ __launch_bounds__(kBlock) void tsi_graph_check_kernel(int64_t n_rows_s,
    const int64_t* __restrict__ rp_ss, const int32_t* __restrict__ col_ss,
    const int64_t* __restrict__ rp_tt, const int32_t* __restrict__ col_tt, int32_t* flag)
{
  int bad = 0;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < n_rows_s; r += int64_t(gridDim.x) * kBlock)
  {
    const int64_t t = r / 3, d = r - 3 * t;
    const int64_t b = rp_tt[t], lt = rp_tt[t + 1] - b;
    const int64_t rb = rp_ss[r];
    if (rb != 9 * b + 3 * d * lt || rp_ss[r + 1] - rb != 3 * lt)
    {
      bad = 1;
      continue;
    }
    for (int64_t j = 0; j < 3 * lt; ++j)
      if (col_ss[rb + j] != 3 * col_tt[b + j / 3] + int32_t(j % 3)) bad = 1;
  }
  if (bad) atomicOr(flag, 1);
}

int device_fail(fcg_tsi_ctx* t, hipError_t he)
{
  t->last_error = std::string("HIP: ") + hipGetErrorString(he);
  return fcg_device_error();
}

// the conditions on the TSI context alone
int qualify_thermo(fcg_tsi_ctx* t, const char* who)
{
  const TsiDevice& d = t->d;
  if (!d.node_consistent)
  {
    t->last_error = std::string(who) + ": the thermo numbering is not node-consistent (thermo LID = "
                    "structural LID / 3, block graphs the expansions of the k_TT node graph)";
    return FCG_ERR_ARG;
  }
  if (d.n_cols_s != d.n_rows_s || d.n_cols_t != d.n_rows_t)
  {
    t->last_error = std::string(who) + ": single-rank systems only (n_cols = n_rows in both fields)";
    return FCG_ERR_ARG;
  }
  return FCG_OK;
}

// ... and on the pair; the graph identity is checked on the device once per structural context
int qualify_pair(fcg_ctx* sctx, fcg_tsi_ctx* t, hipStream_t s, const char* who)
{
  if (!sctx)
  {
    t->last_error = std::string(who) + ": no structural context";
    return FCG_ERR_ARG;
  }
  if (const int rc = qualify_thermo(t, who)) return rc;
  TsiDevice& d = t->d;
  const DeviceMesh& m = sctx->mesh;
  if (sctx->device != t->device)
  {
    t->last_error = std::string(who) + ": the structural and the TSI context are on different devices";
    return FCG_ERR_ARG;
  }
  if (!m.square_local || m.n_rows != m.n_cols)
  {
    t->last_error = std::string(who) + ": the structural context is not single-rank (column map = row map)";
    return FCG_ERR_ARG;
  }
  if (m.n_rows != d.n_rows_s || m.nnz != 9 * d.nnz_tt || 3 * m.n_rownodes != m.n_rows)
  {
    t->last_error = std::string(who) + ": the structural context's graph is not the 3 x 3 expansion of "
                    "the k_TT graph (sizes differ)";
    return FCG_ERR_ARG;
  }
  if (d.solve_with == static_cast<const void*>(sctx) || d.n_rows_s == 0) return FCG_OK;
  int32_t flag = 0;
  hipError_t he = hipMemcpyAsync(d.err, &flag, sizeof(flag), hipMemcpyHostToDevice, s);
  if (he == hipSuccess)
  {
    hipLaunchKernelGGL(tsi_graph_check_kernel, dim3(std::min(4096u, blocks_for(d.n_rows_s))), dim3(kBlock),
        0, s, d.n_rows_s, m.rowptr, m.col_lid, d.rowptr_tt, d.col_tt, d.err);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpyAsync(&flag, d.err, sizeof(flag), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) return device_fail(t, he);
  if (flag)
  {
    t->last_error = std::string(who) + ": the structural context's graph is not the 3 x 3 expansion of "
                    "the k_TT graph";
    return FCG_ERR_ARG;
  }
  d.solve_with = sctx;
  return FCG_OK;
}

hipError_t launch_block_apply(const TsiDevice& d, const double* Kss, const double* Kst, const double* Kts,
    const double* Ktt, const double* xs, const double* xt, double* ys, double* yt, hipStream_t s)
{
  const int64_t nn = d.n_rows_t;
  if (nn == 0) return hipSuccess;
  if (d.npe == 27)
    hipLaunchKernelGGL(tsi_block_apply_kernel<64>, dim3(blocks_for(nn * 64)), dim3(kBlock), 0, s,
        d.rowptr_tt, d.col_tt, Kss, Kst, Kts, Ktt, xs, xt, ys, yt, nn);
  else
    hipLaunchKernelGGL(tsi_block_apply_kernel<16>, dim3(blocks_for(nn * 16)), dim3(kBlock), 0, s,
        d.rowptr_tt, d.col_tt, Kss, Kst, Kts, Ktt, xs, xt, ys, yt, nn);
  return hipGetLastError();
}

// the monolithic operator and the 2 x 2 block preconditioner on stacked vectors
struct TsiOps : KrylovOps {
  fcg_ctx* sctx;
  fcg_tsi_ctx* tctx;
  fcg_amg* amg;
  const double *Kss, *Kst, *Kts, *Ktt;
  const double* dinv;  // nodal block Jacobi of K_SS (amg NULL)
  const double* dtt;   // 1 / diag K_TT
  fcg_samg* amg_t = nullptr;  // the thermal V-cycle in place of dtt
  double* wT = nullptr;       // its right-hand side under bgs
  int bgs;
  int apply(const double* x, double* y, hipStream_t s) override
  {
    const int64_t ns = tctx->d.n_rows_s;
    const hipError_t he = launch_block_apply(tctx->d, Kss, Kst, Kts, Ktt, x, x + ns, y, y + ns, s);
    if (he == hipSuccess) return FCG_OK;
    error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  int residual(const double* b, const double* x, double* r, int64_t n, hipStream_t s) override
  {
    const TsiDevice& d = tctx->d;
    hipLaunchKernelGGL(tsi_residual_kernel, dim3(blocks_for(n * 16)), dim3(kBlock), 0, s, d.rowptr_tt,
        d.col_tt, Kss, Kst, Kts, Ktt, x, b, r, d.n_rows_t);
    const hipError_t he = hipGetLastError();
    if (he == hipSuccess) return FCG_OK;
    error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  int precond(const double* r, double* z, hipStream_t s) override
  {
    const TsiDevice& d = tctx->d;
    const int64_t ns = d.n_rows_s, nn = d.n_rows_t;
    if (amg)
    {
      const int rc = fcg_amg_apply(amg, Kss, r, z, s);
      if (rc != FCG_OK)
      {
        error = fcg_amg_last_error(amg);
        return rc;
      }
    }
    else
    {
      const int rc = fcg_block_jacobi_apply(sctx, dinv, r, z, 1.0, 0, s);
      if (rc != FCG_OK)
      {
        error = sctx->last_error;
        return rc;
      }
    }
    if (amg_t)
    {
      const double* rhs = r + ns;
      if (bgs)
      {
        if (d.npe == 27)
          hipLaunchKernelGGL(tsi_thermal_rhs_kernel<64>, dim3(blocks_for(nn * 64)), dim3(kBlock), 0, s,
              d.rowptr_tt, d.col_tt, Kts, r + ns, z, wT, nn);
        else
          hipLaunchKernelGGL(tsi_thermal_rhs_kernel<16>, dim3(blocks_for(nn * 16)), dim3(kBlock), 0, s,
              d.rowptr_tt, d.col_tt, Kts, r + ns, z, wT, nn);
        rhs = wT;
      }
      const int rc = fcg_samg_apply(amg_t, Ktt, rhs, z + ns, s);
      if (rc != FCG_OK) error = fcg_samg_last_error(amg_t);
      return rc;
    }
    if (d.npe == 27)
      hipLaunchKernelGGL(tsi_thermal_precond_kernel<64>, dim3(blocks_for(nn * 64)), dim3(kBlock), 0, s,
          d.rowptr_tt, d.col_tt, Kts, dtt, r + ns, z, z + ns, nn, bgs);
    else
      hipLaunchKernelGGL(tsi_thermal_precond_kernel<16>, dim3(blocks_for(nn * 16)), dim3(kBlock), 0, s,
          d.rowptr_tt, d.col_tt, Kts, dtt, r + ns, z, z + ns, nn, bgs);
    const hipError_t he = hipGetLastError();
    if (he == hipSuccess) return FCG_OK;
    error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
};

}  // namespace
}  // namespace fcg

extern "C" {

int fcg_tsi_block_apply(fcg_ctx* sctx, fcg_tsi_ctx* tctx, const double* d_Kss, const double* d_Kst,
    const double* d_Kts, const double* d_Ktt, const double* d_xs, const double* d_xt, double* d_ys,
    double* d_yt, void* stream)
{
  if (!tctx) return FCG_ERR_ARG;
  (void)hipSetDevice(tctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : tctx->stream;
  if (const int rc = fcg::qualify_pair(sctx, tctx, s, "fcg_tsi_block_apply")) return rc;
  const fcg::TsiDevice& d = tctx->d;
  if (d.n_rows_t == 0) return FCG_OK;
  if (!d_Kss || !d_Kst || !d_Kts || !d_Ktt || !d_xs || !d_xt || !d_ys || !d_yt)
  {
    tctx->last_error = "fcg_tsi_block_apply: a NULL block or vector";
    return FCG_ERR_ARG;
  }
  const hipError_t he = fcg::launch_block_apply(d, d_Kss, d_Kst, d_Kts, d_Ktt, d_xs, d_xt, d_ys, d_yt, s);
  if (he != hipSuccess) return fcg::device_fail(tctx, he);
  return FCG_OK;
}

int fcg_tsi_dirichlet_apply(fcg_tsi_ctx* tctx, int64_t n_dbc_s, const int32_t* d_rows_s,
    int64_t n_dbc_t, const int32_t* d_rows_t, double* d_Kst, double* d_Kts, double* d_Ktt,
    double* d_rhs_T, void* stream)
{
  if (!tctx) return FCG_ERR_ARG;
  if (const int rc = fcg::qualify_thermo(tctx, "fcg_tsi_dirichlet_apply")) return rc;
  if (n_dbc_s < 0 || n_dbc_t < 0 || (n_dbc_s > 0 && !d_rows_s) || (n_dbc_t > 0 && !d_rows_t))
  {
    tctx->last_error = "fcg_tsi_dirichlet_apply: a negative count, or rows missing";
    return FCG_ERR_ARG;
  }
  if (n_dbc_s + n_dbc_t == 0) return FCG_OK;
  (void)hipSetDevice(tctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : tctx->stream;
  fcg::TsiDevice& d = tctx->d;
  fcg::TsiDbcArgs a;
  a.n_s = n_dbc_s;
  a.n_t = n_dbc_t;
  a.n_rows_s = d.n_rows_s;
  a.n_rows_t = d.n_rows_t;
  a.rows_s = d_rows_s;
  a.rows_t = d_rows_t;
  a.rp_st = d.rowptr_st;
  a.rp_ts = d.rowptr_ts;
  a.rp_tt = d.rowptr_tt;
  a.col_tt = d.col_tt;
  a.Kst = d_Kst;
  a.Kts = d_Kts;
  a.Ktt = d_Ktt;
  a.rhsT = d_rhs_T;
  a.flag = d.err;
  int32_t flag = 0;
  hipError_t he = hipMemcpyAsync(d.err, &flag, sizeof(flag), hipMemcpyHostToDevice, s);
  if (he == hipSuccess)
  {
    hipLaunchKernelGGL(fcg::tsi_dirichlet_kernel, dim3(fcg::blocks_for((n_dbc_s + n_dbc_t) * 64)),
        dim3(fcg::kBlock), 0, s, a);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpyAsync(&flag, d.err, sizeof(flag), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) return fcg::device_fail(tctx, he);
  if (flag)
  {
    tctx->last_error = flag == 2 ? "fcg_tsi_dirichlet_apply: a Dirichlet row outside the row map"
                                 : "fcg_tsi_dirichlet_apply: a thermal Dirichlet row without a diagonal entry";
    return FCG_ERR_ARG;
  }
  return FCG_OK;
}

int fcg_tsi_gmres_solve(fcg_ctx* sctx, fcg_tsi_ctx* tctx, fcg_amg* amg_s, const double* d_Kss,
    const double* d_Kst, const double* d_Kts, const double* d_Ktt, const double* d_bs,
    const double* d_bt, double* d_xs, double* d_xt, const fcg_gmres_options* opt, int* iterations,
    double* rel_residual, void* stream)
{
  return fcg_tsi_gmres_solve_amg(sctx, tctx, amg_s, nullptr, d_Kss, d_Kst, d_Kts, d_Ktt, d_bs, d_bt, d_xs,
      d_xt, opt, iterations, rel_residual, stream);
}

int fcg_tsi_gmres_solve_amg(fcg_ctx* sctx, fcg_tsi_ctx* tctx, fcg_amg* amg_s, fcg_samg* amg_t,
    const double* d_Kss, const double* d_Kst, const double* d_Kts, const double* d_Ktt,
    const double* d_bs, const double* d_bt, double* d_xs, double* d_xt, const fcg_gmres_options* opt,
    int* iterations, double* rel_residual, void* stream)
{
  if (!tctx) return FCG_ERR_ARG;
  if (iterations) *iterations = 0;
  if (rel_residual) *rel_residual = 0.0;
  (void)hipSetDevice(tctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : tctx->stream;
  if (const int rc = fcg::qualify_pair(sctx, tctx, s, "fcg_tsi_gmres_solve")) return rc;
  if (!opt || opt->restart < 1 || opt->restart > fcg::kKrylovMaxRestart || opt->max_iter < 0 ||
      !(opt->rtol >= 0.0) || (opt->precond != 0 && opt->precond != 1))
  {
    tctx->last_error = "fcg_tsi_gmres_solve: restart must lie in [1, 128], max_iter >= 0, rtol >= 0 "
                       "and precond be 0 or 1";
    return FCG_ERR_ARG;
  }
  if (amg_t && fcg_samg_context(amg_t) != tctx)
  {
    tctx->last_error = "fcg_tsi_gmres_solve: the thermal AMG was created on another thermo context";
    return FCG_ERR_ARG;
  }
  fcg::TsiDevice& d = tctx->d;
  const int64_t ns = d.n_rows_s, nn = d.n_rows_t, n = ns + nn;
  if (n == 0) return FCG_OK;
  if (!d_Kss || !d_Kst || !d_Kts || !d_Ktt || !d_bs || !d_bt || !d_xs || !d_xt)
  {
    tctx->last_error = "fcg_tsi_gmres_solve: a NULL block or vector";
    return FCG_ERR_ARG;
  }
  // work space: the core's, then stacked b and x, the nodal block inverses of K_SS and 1 / diag K_TT
  const int64_t core = fcg::krylov_work_doubles(n, opt->restart);
  // (with amg_t one more thermal vector, the V-cycle's right-hand side)
  hipError_t he = fcg::krylov_reserve(&d.krylov_work, &d.krylov_doubles,
      core + 2 * n + 3 * ns + nn + (amg_t ? nn : 0), &tctx->device_bytes);
  if (he != hipSuccess)
  {
    tctx->last_error = std::string("fcg_tsi_gmres_solve: work space: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  double* b = d.krylov_work + core;
  double* x = b + n;
  double* dinv = x + n;
  double* dtt = dinv + 3 * ns;
  if (!amg_s)
  {
    const int rc = fcg_block_jacobi_setup(sctx, d_Kss, dinv, s);
    if (rc != FCG_OK)
    {
      tctx->last_error = std::string("fcg_tsi_gmres_solve: K_SS: ") + fcg_last_error(sctx);
      return rc;
    }
  }
  int32_t* flag = sctx->mesh.err + 2;  // the solver flag word
  int32_t bad = 0;
  he = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
  if (he == hipSuccess)
  {
    hipLaunchKernelGGL(fcg::tsi_dtt_kernel, dim3(fcg::blocks_for(nn)), dim3(fcg::kBlock), 0, s, d.rowptr_tt,
        d.col_tt, d_Ktt, dtt, nn, flag);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipMemcpyAsync(b, d_bs, sizeof(double) * ns, hipMemcpyDeviceToDevice, s);
  if (he == hipSuccess) he = hipMemcpyAsync(b + ns, d_bt, sizeof(double) * nn, hipMemcpyDeviceToDevice, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) return fcg::device_fail(tctx, he);
  if (bad)
  {
    tctx->last_error = "fcg_tsi_gmres_solve: a zero, missing or non-finite diagonal entry of K_TT";
    return FCG_ERR_SINGULAR;
  }
  fcg::TsiOps ops;
  ops.sctx = sctx;
  ops.tctx = tctx;
  ops.amg = amg_s;
  ops.Kss = d_Kss;
  ops.Kst = d_Kst;
  ops.Kts = d_Kts;
  ops.Ktt = d_Ktt;
  ops.dinv = dinv;
  ops.dtt = dtt;
  ops.amg_t = amg_t;
  ops.wT = dtt + nn;
  ops.bgs = opt->precond;
  std::string err;
  const int rc = fcg::fgmres(ops, n, b, x, opt->restart, opt->max_iter, opt->rtol, d.krylov_work, flag,
      s, iterations, rel_residual, err);
  if (rc != FCG_OK)
  {
    tctx->last_error = "fcg_tsi_gmres_solve: " + err;
    return rc;
  }
  he = hipMemcpyAsync(d_xs, x, sizeof(double) * ns, hipMemcpyDeviceToDevice, s);
  if (he == hipSuccess) he = hipMemcpyAsync(d_xt, x + ns, sizeof(double) * nn, hipMemcpyDeviceToDevice, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) return fcg::device_fail(tctx, he);
  return FCG_OK;
}

}  // extern "C"
