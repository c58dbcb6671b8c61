// fcg_tsi.hip -- thermo-structure interaction (TSI), geometrically linear, on the device: the
// temperature-dependent blocks of 4C's monolithic TSI tangent and the temperature-dependent parts
// of both residuals (BASELINE config 5).
//
// Reference (paths relative to the 4C tree):
//   f_S thermal stress   SolidScatraEleCalc::evaluate_nonlinear_force_stiffness_mass with a
//                        "temperature" state (4C_solid_scatra_3D_ele_calc.cpp:272-403) and
//                        Mat::ThermoStVenantKirchhoff::evaluate (4C_mat_thermostvenantkirchhoff.cpp:141-174)
//   k_ST                 struct_calc_stifftemp -> evaluate_d_stress_d_scalar
//                        (4C_solid_scatra_3D_ele_calc.cpp:405-490; dS/dT :250-295), assembled with
//                        AssembleStrategy(0, 1, k_st) by TSI::Monolithic::apply_str_coupl_matrix
//                        (4C_tsi_monolithic.cpp:1694-1767)
//   k_TT, f_T            calc_thermo_fintcond: linear_thermo_contribution (4C_thermo_ele_impl.cpp:802-891,
//                        Fourier conduction 4C_mat_fourier.cpp:147-192) + linear_disp_contribution (:899-1043)
//   k_TS                 calc_thermo_coupltang: linear_coupled_tang (4C_thermo_ele_impl.cpp:1046-1194)
// With a constant Young's modulus the stress-temperature modulus m = -(2 mu + 3 lambda) alpha_T
// (st_modulus, 4C_mat_thermostvenantkirchhoff.cpp:331-369) is constant, B_L^T (m,m,m,0,0,0) =
// m N_XYZ(a), and every block reduces to Gauss-point scalars:
//   f_S(a)   += sum_g fac m (T_g - T_0) N_XYZ(a)
//   K_ST(a,b) = sum_g fac m N_XYZ(a) N_b                                   (3 x 1 per node pair)
//   K_TS(a,b) = -timefac timefac_d sum_g fac N_a T_g m N_XYZ(b)^T            (1 x 3)
//   K_TT(a,b) = sum_g fac (k N_XYZ(a).N_XYZ(b) - m tr(e')_g N_a N_b)
//   f_T(a)    = sum_g fac (k N_XYZ(a).grad T_g - m tr(e')_g N_a T_g)
// with T_g = N.T, grad T_g = N_XYZ T and tr(e')_g = sum_b N_XYZ(b).v_b (e' = B_L v).
//
// Kernels: tsi_element_kernel (one wavefront per element: Gauss-point stage into LDS, then the
// node pairs; the block rows of every owned node go to an incidence-ordered scratch record) and
// tsi_assemble_kernel (one wavefront per owned node: its 3 k_ST rows, its k_TS row and its k_TT row
// are summed in element order in an LDS row image and written once, coalesced).  Owned rows only,
// no atomics, bitwise reproducible -- the contract of the structural path.
//
// fcg_tsi_create is the driver of the context's creation: the host stages of fcg_tsi_plan.cpp
// (descriptor checks, node rows, row layout, incidences, positions, tables, node consistency,
// constants), then the context (device, stream) and the upload of what the stages filled.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fcg_hex8_element.hpp"
#include "fcg_internal.hpp"
#include "fcg_status.hpp"
#include "fcg_tsi_internal.hpp"
#include "fcg_tsi_plan.hpp"
#include "fcg_upload.hpp"

namespace fcg {
namespace {

// scratch record of incidence (e, a): K_ST rows [3][npe] | K_TS row [npe][3] | K_TT row [npe] |
// f_S thermal part [3] | f_T [1]
__host__ __device__ constexpr int tsi_rec(int npe) { return 7 * npe + 4; }

template <int NPE>
struct TsiShared {
  double X[NPE * 3];
  double V[NPE * 3];
  double T[NPE];
  double N[NPE * NPE];        // [g][n]
  double NX[NPE * NPE * 3];   // [g][n][d]
  double fac[NPE], Tg[NPE], tr[NPE], gT[NPE * 3];
  int bad;
};

struct TsiElementArgs {
  int64_t n_ele;
  const int32_t* ele_nodes;
  const double* node_x;
  const int32_t* dof_col_s;
  const int32_t* dof_col_t;
  const double* v_col;
  const double* T_col;
  const int32_t* inc_of;
  const double* tables;
  double* scratch;
  int32_t* err;
  double m, T0, conduct, kts_fac;
  int want;  // fcg_tsi_part bits
};

template <int NPE>
__global__ __launch_bounds__(64) void tsi_element_kernel(TsiElementArgs A)
{
  constexpr int NGP = NPE;
  constexpr int REC = tsi_rec(NPE);
  __shared__ TsiShared<NPE> sh;
  const int lane = threadIdx.x;
  const double* dNgp = A.tables;
  const double* Ngp = A.tables + NGP * NPE * 3;
  const double* dNnode = Ngp + NGP * NPE;
  const double* wgp = dNnode + NPE * NPE * 3;
  for (int v = lane; v < NGP * NPE; v += 64) sh.N[v] = Ngp[v];
  const bool want_st = A.want & FCG_TSI_STIFFTEMP;
  const bool want_fs = A.want & FCG_TSI_STRUCT_FORCE;
  const bool want_t = A.want & FCG_TSI_THERMO_FINTCOND;
  const bool want_ts = A.want & FCG_TSI_COUPLTANG;

  for (int64_t e = blockIdx.x; e < A.n_ele; e += gridDim.x)
  {
    const int32_t* en = A.ele_nodes + e * NPE;
    for (int v = lane; v < 3 * NPE; v += 64)
    {
      const int a = v / 3, d = v - 3 * (v / 3);
      const int node = en[a];
      sh.X[v] = A.node_x[3 * int64_t(node) + d];
      sh.V[v] = want_t ? A.v_col[A.dof_col_s[node] + d] : 0.0;
    }
    for (int a = lane; a < NPE; a += 64) sh.T[a] = A.T_col[A.dof_col_t[en[a]]];
    if (lane == 0) sh.bad = 0;
    __syncthreads();

    // Gauss-point stage (eval_shape_func_and_derivs_at_int_point, 4C_thermo_ele_impl.cpp:2613-2671;
    // evaluate_jacobian_mapping, 4C_solid_3D_ele_calc_lib.hpp:435-448) and the nodal det J check
    // of struct_calc_stifftemp (4C_solid_scatra_3D_ele_calc.cpp:441, calc_lib.hpp:475-496)
    for (int t = lane; t < NGP + (want_st ? NPE : 0); t += 64)
    {
      const bool gp = t < NGP;
      const int g = gp ? t : t - NGP;
      const double* dN = (gp ? dNgp : dNnode) + 3 * NPE * g;
      double J[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) J[k] = 0.0;
      for (int c = 0; c < NPE; ++c)
      {
        const double d0 = dN[3 * c], d1 = dN[3 * c + 1], d2 = dN[3 * c + 2];
        const double x0 = sh.X[3 * c], x1 = sh.X[3 * c + 1], x2 = sh.X[3 * c + 2];
        J[0] += d0 * x0; J[1] += d1 * x0; J[2] += d2 * x0;
        J[3] += d0 * x1; J[4] += d1 * x1; J[5] += d2 * x1;
        J[6] += d0 * x2; J[7] += d1 * x2; J[8] += d2 * x2;
      }
      const double det = h8_invert3x3(J);
      if (!gp)
      {
        if (det == 0.0) atomicMax(&sh.bad, int(FCG_ERR_SINGULAR));
        else if (!(det > 0)) atomicMax(&sh.bad, int(FCG_ERR_NODAL_DETJ));
        continue;
      }
      // the thermo element throws for det < 1e-16 in both of its actions
      // (eval_shape_func_and_derivs_at_int_point, 4C_thermo_ele_impl.cpp:2663-2664)
      if (det == 0.0) atomicMax(&sh.bad, int(FCG_ERR_SINGULAR));
      else if ((want_t || want_ts) && det < 1e-16) atomicMax(&sh.bad, int(FCG_ERR_NODAL_DETJ));
      const double fac = det * wgp[g];
      double Tg = 0.0, tr = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
      for (int c = 0; c < NPE; ++c)
      {
        const double d0 = dN[3 * c], d1 = dN[3 * c + 1], d2 = dN[3 * c + 2];
        const double n0 = J[0] * d0 + J[3] * d1 + J[6] * d2;
        const double n1 = J[1] * d0 + J[4] * d1 + J[7] * d2;
        const double n2 = J[2] * d0 + J[5] * d1 + J[8] * d2;
        double* nx = sh.NX + 3 * (NPE * g + c);
        nx[0] = n0;
        nx[1] = n1;
        nx[2] = n2;
        const double Tc = sh.T[c];
        Tg += sh.N[NPE * g + c] * Tc;
        g0 += n0 * Tc;
        g1 += n1 * Tc;
        g2 += n2 * Tc;
        tr += n0 * sh.V[3 * c] + n1 * sh.V[3 * c + 1] + n2 * sh.V[3 * c + 2];
      }
      sh.fac[g] = fac;
      sh.Tg[g] = Tg;
      sh.tr[g] = tr;
      sh.gT[3 * g] = g0;
      sh.gT[3 * g + 1] = g1;
      sh.gT[3 * g + 2] = g2;
    }
    __syncthreads();
    if (sh.bad)
    {
      if (lane == 0)
      {
        atomicMax(&A.err[0], sh.bad);
        atomicMin(&A.err[1], int32_t(e));
      }
      __syncthreads();
      continue;
    }
    const int32_t* inc = A.inc_of + e * NPE;
    const double m = A.m, k = A.conduct;

    // node pairs (a, b): K_ST(a,b) [3], K_TS(a,b) [3], K_TT(a,b)
    if (want_st || want_ts || want_t)
      for (int p = lane; p < NPE * NPE; p += 64)
      {
        const int a = p / NPE, b = p - NPE * (p / NPE);
        const int32_t ia = inc[a];
        if (ia < 0) continue;
        double st0 = 0, st1 = 0, st2 = 0, ts0 = 0, ts1 = 0, ts2 = 0, tt = 0;
        for (int g = 0; g < NGP; ++g)
        {
          const double fac = sh.fac[g];
          const double* na = sh.NX + 3 * (NPE * g + a);
          const double* nb = sh.NX + 3 * (NPE * g + b);
          const double Na = sh.N[NPE * g + a], Nb = sh.N[NPE * g + b];
          const double cst = fac * m * Nb;
          st0 += cst * na[0];
          st1 += cst * na[1];
          st2 += cst * na[2];
          const double cts = fac * Na * sh.Tg[g] * m;
          ts0 += cts * nb[0];
          ts1 += cts * nb[1];
          ts2 += cts * nb[2];
          tt += fac * (k * (na[0] * nb[0] + na[1] * nb[1] + na[2] * nb[2]) - m * sh.tr[g] * Na * Nb);
        }
        double* rec = A.scratch + int64_t(ia) * REC;
        rec[b] = st0;
        rec[NPE + b] = st1;
        rec[2 * NPE + b] = st2;
        rec[3 * NPE + 3 * b] = A.kts_fac * ts0;
        rec[3 * NPE + 3 * b + 1] = A.kts_fac * ts1;
        rec[3 * NPE + 3 * b + 2] = A.kts_fac * ts2;
        rec[6 * NPE + b] = tt;
      }
    // per node: f_S thermal part [3], f_T
    if (want_fs || want_t)
      for (int a = lane; a < NPE; a += 64)
      {
        const int32_t ia = inc[a];
        if (ia < 0) continue;
        double f0 = 0, f1 = 0, f2 = 0, ft = 0;
        for (int g = 0; g < NGP; ++g)
        {
          const double fac = sh.fac[g];
          const double* na = sh.NX + 3 * (NPE * g + a);
          const double c = fac * m * (sh.Tg[g] - A.T0);
          f0 += c * na[0];
          f1 += c * na[1];
          f2 += c * na[2];
          const double* gt = sh.gT + 3 * g;
          ft += fac * (k * (na[0] * gt[0] + na[1] * gt[1] + na[2] * gt[2]) -
                          m * sh.tr[g] * sh.N[NPE * g + a] * sh.Tg[g]);
        }
        double* rec = A.scratch + int64_t(ia) * REC + 7 * NPE;
        rec[0] = f0;
        rec[1] = f1;
        rec[2] = f2;
        rec[3] = ft;
      }
    __syncthreads();
  }
}

struct TsiAssembleArgs {
  int64_t n_rownodes;
  const int64_t* inc_ptr;
  const int32_t* rn_srow;
  const int32_t* rn_trow;
  const uint16_t* pos_st;
  const uint16_t* pos_ts;
  const uint16_t* pos_tt;
  const double* scratch;
  const int64_t* rowptr_st;
  const int64_t* rowptr_ts;
  const int64_t* rowptr_tt;
  double* Kst;
  double* Kts;
  double* Ktt;
  double* fs;
  double* fT;
  int want;
  int overwrite;
};

template <int NPE>
__global__ __launch_bounds__(64) void tsi_assemble_kernel(TsiAssembleArgs A)
{
  constexpr int REC = tsi_rec(NPE);
  constexpr int MAXN = NPE == 8 ? 27 : 125;  // node neighbours of a row
  __shared__ double img_st[3 * MAXN];
  __shared__ double img_ts[3 * MAXN];
  __shared__ double img_tt[MAXN];
  const int lane = threadIdx.x;
  const bool st = A.want & FCG_TSI_STIFFTEMP;
  const bool ts = A.want & FCG_TSI_COUPLTANG;
  const bool tt = A.want & FCG_TSI_THERMO_FINTCOND;
  const bool fs = A.want & FCG_TSI_STRUCT_FORCE;
  for (int64_t r = blockIdx.x; r < A.n_rownodes; r += gridDim.x)
  {
    const int32_t srow = A.rn_srow[r], trow = A.rn_trow[r];
    const int lst = st ? int(A.rowptr_st[srow + 1] - A.rowptr_st[srow]) : 0;
    const int64_t bts = ts ? A.rowptr_ts[trow] : 0;
    const int lts = ts ? int(A.rowptr_ts[trow + 1] - bts) : 0;
    const int64_t btt = tt ? A.rowptr_tt[trow] : 0;
    const int ltt = tt ? int(A.rowptr_tt[trow + 1] - btt) : 0;
    for (int v = lane; v < 3 * MAXN; v += 64)
    {
      img_st[v] = 0.0;
      img_ts[v] = 0.0;
    }
    for (int v = lane; v < MAXN; v += 64) img_tt[v] = 0.0;
    double facc = 0.0;
    __syncthreads();
    for (int64_t q = A.inc_ptr[r]; q < A.inc_ptr[r + 1]; ++q)
    {
      const double* rec = A.scratch + q * REC;
      // 7 npe matrix entries of one incidence: distinct LDS targets
      for (int v = lane; v < 7 * NPE; v += 64)
      {
        if (v < 3 * NPE)
        {
          if (!st) continue;
          const int i = v / NPE, b = v - NPE * i;
          img_st[i * MAXN + A.pos_st[q * NPE + b]] += rec[v];
        }
        else if (v < 6 * NPE)
        {
          if (!ts) continue;
          const int w = v - 3 * NPE, b = w / 3, j = w - 3 * b;
          img_ts[A.pos_ts[q * NPE + b] + j] += rec[v];
        }
        else
        {
          if (!tt) continue;
          const int b = v - 6 * NPE;
          img_tt[A.pos_tt[q * NPE + b]] += rec[v];
        }
      }
      if (lane < 4) facc += rec[7 * NPE + lane];
      __syncthreads();
    }
    if (st)
      for (int v = lane; v < 3 * lst; v += 64)
      {
        const int i = v / lst, c = v - lst * i;
        double* dst = A.Kst + A.rowptr_st[srow + i] + c;
        if (A.overwrite)
          *dst = img_st[i * MAXN + c];
        else
          *dst += img_st[i * MAXN + c];
      }
    if (ts)
      for (int v = lane; v < lts; v += 64)
      {
        if (A.overwrite)
          A.Kts[bts + v] = img_ts[v];
        else
          A.Kts[bts + v] += img_ts[v];
      }
    if (tt)
      for (int v = lane; v < ltt; v += 64)
      {
        if (A.overwrite)
          A.Ktt[btt + v] = img_tt[v];
        else
          A.Ktt[btt + v] += img_tt[v];
      }
    // f_S: the thermal-stress part is added to the structural residual (its mechanical part comes
    // from fcg_evaluate_device); f_T follows the mode
    if (fs && lane < 3) A.fs[srow + lane] += facc;
    if (tt && lane == 3)
    {
      if (A.overwrite)
        A.fT[trow] = facc;
      else
        A.fT[trow] += facc;
    }
    __syncthreads();
  }
}

// The structural context of a fused call describes the same mesh with the node graph of the TSI
// context: same elements, node coordinates and column DOFs, K rows = the 3 x 3 expansion of the k_TT rows.
struct FusedCheckArgs {
  int64_t n_node, n_ele8, n_rows_s;
  const int32_t* s_dof_col;
  const int32_t* t_dof_col_s;
  const int32_t* s_ele;
  const int32_t* t_ele;
  const double* s_x;
  const double* t_x;
  const int64_t* rp_ss;
  const int32_t* col_ss;
  const int64_t* rp_tt;
  const int32_t* col_tt;
  int32_t* flag;
};

__global__ __launch_bounds__(256) void tsi_fused_check_kernel(FusedCheckArgs A)
{
  const int64_t i0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t st = int64_t(gridDim.x) * blockDim.x;
  int bad = 0;
  for (int64_t i = i0; i < A.n_node; i += st)
    if (A.s_dof_col[i] != A.t_dof_col_s[i] || A.s_x[3 * i] != A.t_x[3 * i] ||
        A.s_x[3 * i + 1] != A.t_x[3 * i + 1] || A.s_x[3 * i + 2] != A.t_x[3 * i + 2])
      bad = 1;
  for (int64_t i = i0; i < A.n_ele8; i += st)
    if (A.s_ele[i] != A.t_ele[i]) bad = 1;
  for (int64_t r = i0; r < A.n_rows_s; r += st)
  {
    const int64_t t = r / 3, d = r - 3 * t;
    const int64_t b = A.rp_tt[t], lt = A.rp_tt[t + 1] - b;
    const int64_t rb = A.rp_ss[r];
    if (rb != 9 * b + 3 * d * lt || A.rp_ss[r + 1] - rb != 3 * lt)
    {
      bad = 1;
      continue;
    }
    for (int64_t j = 0; j < 3 * lt; ++j)
      if (A.col_ss[rb + j] != 3 * A.col_tt[b + j / 3] + int32_t(j % 3)) bad = 1;
  }
  if (bad) atomicOr(A.flag, 1);
}

std::mutex g_tsi_err_mutex;
std::string g_tsi_create_error;

void set_tsi_create_error(const std::string& s)
{
  std::lock_guard<std::mutex> lk(g_tsi_err_mutex);
  g_tsi_create_error = s;
}

int grid_for(int64_t work, int cap) { return int(work < cap ? (work > 0 ? work : 1) : cap); }

namespace plan = tsi_plan;  // the host stages of fcg_tsi_create (fcg_tsi_plan.cpp)

int open_tsi_context(const fcg_tsi_desc* D, fcg_tsi_ctx*& ctx, std::string& why)
{
  ctx = new fcg_tsi_ctx();
  ctx->device = D->device;
  hipError_t he = hipSetDevice(D->device);
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);  // ordered with the null stream (torch's default)
  if (he != hipSuccess)
  {
    why = std::string("HIP: ") + hipGetErrorString(he);
    delete ctx;
    ctx = nullptr;
    return fcg_device_error();
  }
  return FCG_OK;
}

// sizes, constants and flags of the context, from the descriptor and the plan
void fill_tsi_device(TsiDevice& d, const fcg_tsi_desc* D, const plan::NodeRows& N, const plan::Incidences& I,
    const plan::Constants& C, bool node_consistent, int max_row_tt)
{
  d.npe = plan::npe_of(D);
  d.n_ele = D->n_ele;
  d.n_node = D->n_node;
  d.n_rownodes = N.nrn();
  d.n_inc = I.n_inc;
  d.n_rows_s = D->n_rows_s;
  d.n_cols_s = D->n_cols_s;
  d.n_rows_t = D->n_rows_t;
  d.n_cols_t = D->n_cols_t;
  d.nnz_st = C.nnz_st;
  d.nnz_ts = C.nnz_ts;
  d.nnz_tt = C.nnz_tt;
  d.m = C.m;
  d.lambda = C.lambda;
  d.mu = C.mu;
  d.node_consistent = node_consistent;
  d.fusable = node_consistent && d.npe == 8;
  d.T0 = D->inittemp;
  d.conduct = D->conduct;
  d.max_row_tt = max_row_tt;
}

// the descriptor's arrays and the plan's tables; the first error wins, the later calls still run,
// and device_bytes counts what was allocated
hipError_t upload_tsi(fcg_tsi_ctx* ctx, const fcg_tsi_desc* D, const plan::NodeRows& N,
    const plan::Incidences& I, const plan::Constants& C, const std::vector<double>& tab)
{
  TsiDevice& d = ctx->d;
  const int npe = d.npe;
  const int64_t nrn = d.n_rownodes, n_inc = d.n_inc;
  int64_t& bytes = ctx->device_bytes;
  hipError_t he = hipSuccess;
  auto chk = [&](hipError_t x) {
    if (he == hipSuccess) he = x;
  };
  chk(upload(&d.ele_nodes, D->ele_nodes, D->n_ele * npe, bytes));
  chk(upload(&d.ele_gid, D->ele_gid ? D->ele_gid : C.ele_gid.data(), D->n_ele, bytes));
  chk(upload(&d.node_x, D->node_x, D->n_node * 3, bytes));
  chk(upload(&d.dof_col_s, D->node_dof_col_s, D->n_node, bytes));
  chk(upload(&d.dof_col_t, D->node_dof_col_t, D->n_node, bytes));
  chk(upload(&d.inc_of, I.inc_of.data(), D->n_ele * npe, bytes));
  chk(upload(&d.inc_ptr, I.inc_ptr.data(), nrn + 1, bytes));
  chk(upload(&d.rn_srow, N.srow.data(), nrn, bytes));
  chk(upload(&d.rn_trow, N.trow.data(), nrn, bytes));
  chk(upload(&d.pos_st, I.pos_st.data(), n_inc * npe, bytes));
  chk(upload(&d.pos_ts, I.pos_ts.data(), n_inc * npe, bytes));
  chk(upload(&d.pos_tt, I.pos_tt.data(), n_inc * npe, bytes));
  chk(upload(&d.rowptr_st, D->rowptr_st, D->n_rows_s + 1, bytes));
  chk(upload(&d.rowptr_ts, D->rowptr_ts, D->n_rows_t + 1, bytes));
  chk(upload(&d.rowptr_tt, D->rowptr_tt, D->n_rows_t + 1, bytes));
  chk(upload(&d.tables, tab.data(), int64_t(tab.size()), bytes));
  // scratch and the error words start as zeros
  const int64_t n_scratch = n_inc * tsi_rec(npe);
  chk(upload<double>(&d.scratch, nullptr, n_scratch, bytes));
  if (d.scratch) chk(hipMemset(d.scratch, 0, sizeof(double) * n_scratch));
  chk(upload<int32_t>(&d.err, nullptr, 2, bytes));
  if (d.err) chk(hipMemset(d.err, 0, sizeof(int32_t) * 2));
  if (d.node_consistent) chk(upload(&d.col_tt, D->col_tt, d.nnz_tt, bytes));
  // the one-step-theta pass walks the k_TT rows of any context
  if (d.node_consistent)
    d.cols_tt = d.col_tt;
  else
    chk(upload(&d.cols_tt, D->col_tt, d.nnz_tt, bytes));
  // the capacity kernel's view of an incidence: its column element and local node
  chk(upload(&d.inc_ele, I.inc_ele.data(), n_inc, bytes));
  chk(upload(&d.inc_loc, I.inc_loc.data(), n_inc, bytes));
  return he;
}

}  // namespace
}  // namespace fcg

extern "C" {

const char* fcg_tsi_last_error(const fcg_tsi_ctx* ctx)
{
  if (ctx) return ctx->last_error.c_str();
  std::lock_guard<std::mutex> lk(fcg::g_tsi_err_mutex);
  return fcg::g_tsi_create_error.c_str();
}

int fcg_tsi_destroy(fcg_tsi_ctx* ctx)
{
  if (!ctx) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  fcg::TsiDevice& d = ctx->d;
  void* ptrs[] = {d.ele_nodes, d.ele_gid, d.node_x, d.dof_col_s, d.dof_col_t, d.inc_of, d.inc_ptr,
      d.rn_srow, d.rn_trow, d.pos_st, d.pos_ts, d.pos_tt, d.rowptr_st, d.rowptr_ts, d.rowptr_tt,
      d.tables, d.scratch, d.err, d.col_tt, d.krylov_work, d.cols_tt == d.col_tt ? nullptr : d.cols_tt,
      d.inc_ele, d.inc_loc, d.ele_capa};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return FCG_OK;
}

// The stages of a TSI context's creation, in order; the host ones are fcg_tsi_plan.cpp's.  Every
// FCG_ERR_ARG is found before the first device call (open_tsi_context).
int fcg_tsi_create(const fcg_tsi_desc* D, fcg_tsi_ctx** out)
{
  namespace plan = fcg::tsi_plan;
  if (!D || !out) return FCG_ERR_ARG;
  *out = nullptr;
  std::string why;
  int rc = FCG_OK;
  auto failed = [&](int code) {
    rc = code;
    if (rc != FCG_OK) fcg::set_tsi_create_error(why);
    return rc != FCG_OK;
  };
  if (failed(plan::check_descriptor(D, why))) return rc;
  plan::NodeRows rows;
  if (failed(plan::build_node_rows(D, rows, why))) return rc;
  if (failed(plan::check_row_layout(D, rows, why))) return rc;
  plan::Incidences inc;
  if (failed(plan::build_incidences(D, rows, inc, why))) return rc;
  if (failed(plan::build_positions(D, rows, inc, why))) return rc;
  // the rest of the host plan (no error exit)
  const std::vector<double> tables = plan::build_tables(D->celltype);
  const bool node_consistent = plan::node_consistent(D);
  const plan::Constants constants = plan::build_constants(D);

  fcg_tsi_ctx* ctx = nullptr;
  if (failed(fcg::open_tsi_context(D, ctx, why))) return rc;
  fcg::fill_tsi_device(ctx->d, D, rows, inc, constants, node_consistent, plan::max_row_tt(D));
  const hipError_t he = fcg::upload_tsi(ctx, D, rows, inc, constants, tables);
  if (he != hipSuccess)
  {
    fcg::set_tsi_create_error(std::string("HIP allocation/copy failed: ") + hipGetErrorString(he));
    fcg_tsi_destroy(ctx);
    return fcg_device_error();
  }
  ctx->h_dof_col_t.assign(D->node_dof_col_t, D->node_dof_col_t + D->n_node);
  ctx->h_dof_row_t.assign(D->node_dof_row_t, D->node_dof_row_t + D->n_node);
  *out = ctx;
  return FCG_OK;
}

int fcg_tsi_evaluate_device(fcg_tsi_ctx* ctx, int parts, int mode, const double* d_v_col,
    const double* d_T_col, double timefac, double timefac_d, double* d_fs_row, double* d_Kst,
    double* d_fT_row, double* d_Ktt, double* d_Kts, void* stream_ptr, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::TsiDevice& d = ctx->d;
  const bool st = parts & FCG_TSI_STIFFTEMP, ts = parts & FCG_TSI_COUPLTANG;
  const bool tt = parts & FCG_TSI_THERMO_FINTCOND, fs = parts & FCG_TSI_STRUCT_FORCE;
  if ((parts & ~0xF) || !parts || (mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE) ||
      (d.n_ele > 0 && !d_T_col) || (tt && d.n_ele > 0 && !d_v_col) ||
      (fs && d.n_rows_s > 0 && !d_fs_row) || (st && d.nnz_st > 0 && !d_Kst) ||
      (tt && d.n_rows_t > 0 && (!d_fT_row || (d.nnz_tt > 0 && !d_Ktt))) ||
      (ts && d.nnz_ts > 0 && !d_Kts))
  {
    ctx->last_error = "invalid TSI evaluate arguments";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  const int32_t init[2] = {0, INT32_MAX};
  hipError_t he = hipMemcpyAsync(d.err, init, sizeof(init), hipMemcpyHostToDevice, s);
  if (he == hipSuccess && d.n_ele > 0)
  {
    fcg::TsiElementArgs a;
    a.n_ele = d.n_ele;
    a.ele_nodes = d.ele_nodes;
    a.node_x = d.node_x;
    a.dof_col_s = d.dof_col_s;
    a.dof_col_t = d.dof_col_t;
    a.v_col = d_v_col;
    a.T_col = d_T_col;
    a.inc_of = d.inc_of;
    a.tables = d.tables;
    a.scratch = d.scratch;
    a.err = d.err;
    a.m = d.m;
    a.T0 = d.T0;
    a.conduct = d.conduct;
    a.kts_fac = -timefac * timefac_d;  // linear_coupled_tang (4C_thermo_ele_impl.cpp:1189)
    a.want = parts;
    const int grid = fcg::grid_for(d.n_ele, 256 * 32);
    if (d.npe == 8)
      hipLaunchKernelGGL(fcg::tsi_element_kernel<8>, dim3(grid), dim3(64), 0, s, a);
    else
      hipLaunchKernelGGL(fcg::tsi_element_kernel<27>, dim3(grid), dim3(64), 0, s, a);
    he = hipGetLastError();
  }
  if (he == hipSuccess && d.n_rownodes > 0)
  {
    fcg::TsiAssembleArgs a;
    a.n_rownodes = d.n_rownodes;
    a.inc_ptr = d.inc_ptr;
    a.rn_srow = d.rn_srow;
    a.rn_trow = d.rn_trow;
    a.pos_st = d.pos_st;
    a.pos_ts = d.pos_ts;
    a.pos_tt = d.pos_tt;
    a.scratch = d.scratch;
    a.rowptr_st = d.rowptr_st;
    a.rowptr_ts = d.rowptr_ts;
    a.rowptr_tt = d.rowptr_tt;
    a.Kst = d_Kst;
    a.Kts = d_Kts;
    a.Ktt = d_Ktt;
    a.fs = d_fs_row;
    a.fT = d_fT_row;
    a.want = parts;
    a.overwrite = mode == FCG_OVERWRITE;
    const int grid = fcg::grid_for(d.n_rownodes, 256 * 32);
    if (d.npe == 8)
      hipLaunchKernelGGL(fcg::tsi_assemble_kernel<8>, dim3(grid), dim3(64), 0, s, a);
    else
      hipLaunchKernelGGL(fcg::tsi_assemble_kernel<27>, dim3(grid), dim3(64), 0, s, a);
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
    int32_t gid = -1;
    if (errv[1] >= 0 && errv[1] < d.n_ele)
      (void)hipMemcpy(&gid, d.ele_gid + errv[1], sizeof(int32_t), hipMemcpyDeviceToHost);
    if (bad_ele_gid) *bad_ele_gid = gid;
    ctx->last_error = errv[0] == FCG_ERR_NODAL_DETJ
                          ? "non-positive jacobian determinant in element " + std::to_string(gid)
                          : "singular 3x3 matrix in element " + std::to_string(gid);
    return errv[0];
  }
  return FCG_OK;
}

int fcg_tsi_evaluate_fused(fcg_ctx* sctx, fcg_tsi_ctx* ctx, int mode, const double* d_u_col,
    const double* d_v_col, const double* d_T_col, double timefac, double timefac_d,
    double* d_fs_row, double* d_Kss, double* d_Kst, double* d_fT_row, double* d_Ktt,
    double* d_Kts, void* stream_ptr, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!sctx)
  {
    ctx->last_error = "no structural context";
    return FCG_ERR_ARG;
  }
  fcg::TsiDevice& d = ctx->d;
  const fcg::DeviceMesh& m = sctx->mesh;
  auto rel_eq = [](double a, double b) { return std::fabs(a - b) <= 1e-14 * std::fabs(b); };
  if (m.n_mat > 0)
  {
    ctx->last_error =
        "fused TSI takes one material: the structural context carries per-element materials "
        "(fcg_set_element_materials)";
    return FCG_ERR_ARG;
  }
  if (m.path != FCG_PATH_STRUCTURED || m.kinem != 0 || m.material != FCG_MAT_STVK || m.npe != 8 ||
      !d.fusable || sctx->device != ctx->device || m.n_node != d.n_node || m.n_ele != d.n_ele ||
      m.n_rows != d.n_rows_s || m.n_cols != d.n_cols_s || m.nnz != 9 * d.nnz_tt ||
      !rel_eq(m.lambda, d.lambda) || !rel_eq(m.mu, d.mu))
  {
    ctx->last_error =
        "fused TSI needs a structured hex8 StVK context with linear kinematics, the TSI material's "
        "E and nu, and node-consistent thermo numbering (thermo LID = structural LID / 3)";
    return FCG_ERR_ARG;
  }
  if ((mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE) ||
      (d.n_ele > 0 && (!d_u_col || !d_v_col || !d_T_col)) ||
      (d.n_rows_s > 0 && (!d_fs_row || !d_Kss || !d_Kst || !d_fT_row || !d_Ktt || !d_Kts)))
  {
    ctx->last_error = "invalid fused TSI evaluate arguments";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  // the fused pass re-initialises the structural context's flags: a queued (async) evaluate's
  // failure is reported first, as fcg_evaluate_host does, instead of being overwritten
  if (sctx->pending)
  {
    const int rc = fcg_check_error(sctx, bad_ele_gid);
    if (rc != FCG_OK) return rc;
  }
  hipStream_t s = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  hipError_t he = hipSuccess;
  if (d.fused_with != static_cast<const void*>(sctx))
  {
    fcg::FusedCheckArgs c;
    c.n_node = d.n_node;
    c.n_ele8 = d.n_ele * 8;
    c.n_rows_s = d.n_rows_s;
    c.s_dof_col = m.node_dof_col;
    c.t_dof_col_s = d.dof_col_s;
    c.s_ele = m.ele_nodes;
    c.t_ele = d.ele_nodes;
    c.s_x = m.node_x;
    c.t_x = d.node_x;
    c.rp_ss = m.rowptr;
    c.col_ss = m.col_lid;
    c.rp_tt = d.rowptr_tt;
    c.col_tt = d.col_tt;
    c.flag = d.err;
    int32_t flag = 0;
    he = hipMemcpyAsync(d.err, &flag, sizeof(flag), hipMemcpyHostToDevice, s);
    if (he == hipSuccess)
    {
      const int64_t work = std::max(std::max(d.n_node, d.n_ele * 8), d.n_rows_s);
      hipLaunchKernelGGL(fcg::tsi_fused_check_kernel, dim3(fcg::grid_for((work + 255) / 256, 4096)),
          dim3(256), 0, s, c);
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, d.err, sizeof(flag), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess)
    {
      ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
      return fcg_device_error();
    }
    if (flag)
    {
      ctx->last_error = "structural context and TSI context do not share the mesh and node graph";
      return FCG_ERR_ARG;
    }
    d.fused_with = sctx;
  }
  const int32_t init[2] = {0, INT32_MAX};
  sctx->mesh.err_clean = false;  // the fused sweep reports through the structural context's flags
  he = hipMemcpyAsync(m.err, init, sizeof(init), hipMemcpyHostToDevice, s);
  if (he == hipSuccess)
  {
    fcg::SweepTsi t;
    t.v_col = d_v_col;
    t.T_col = d_T_col;
    t.Ngp = d.tables + 8 * 8 * 3;
    t.Kst = d_Kst;
    t.Kts = d_Kts;
    t.Ktt = d_Ktt;
    t.fT = d_fT_row;
    t.m = d.m;
    t.T0 = d.T0;
    t.conduct = d.conduct;
    t.kts = -timefac * timefac_d;  // linear_coupled_tang (4C_thermo_ele_impl.cpp:1189)
    // the structural sweep + a thermal-only pass (default), or the one fused pass; read at
    // every call (the call synchronises anyway)
    const char* split_env = std::getenv("FCG_TSI_SPLIT");
    t.split = !(split_env && split_env[0] == '0');
    he = fcg::launch_sweep_h8_tsi(m, d_u_col, mode == FCG_OVERWRITE, d_Kss, d_fs_row, t, s);
  }
  int32_t errv[2] = {0, INT32_MAX};
  if (he == hipSuccess) he = hipMemcpyAsync(errv, m.err, sizeof(errv), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (errv[0] != 0)
  {
    int32_t gid = -1;
    if (errv[1] >= 0 && errv[1] < m.n_ele)
      (void)hipMemcpy(&gid, m.ele_gid + errv[1], sizeof(int32_t), hipMemcpyDeviceToHost);
    if (bad_ele_gid) *bad_ele_gid = gid;
    ctx->last_error = errv[0] == FCG_ERR_NODAL_DETJ
                          ? "non-positive jacobian determinant in element " + std::to_string(gid)
                          : "singular 3x3 matrix in element " + std::to_string(gid);
    return errv[0];
  }
  return FCG_OK;
}

}  // extern "C"
