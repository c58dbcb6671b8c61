// fcg_tsi_surface.hip -- thermal boundary conditions on the TSI context: heat convection against a
// surrounding temperature and a prescribed surface heat flux, integrated once per surface on the
// device and applied per Newton iteration in one short pass over the surface rows.
//
// Reference (paths relative to the 4C tree; pointers only, the formulas are restated here):
//   4C_thermo_ele_boundary_impl.cpp, action calc_thermo_fextconvection: efext = N coeff (T - T_surr)
//   fac and etang = N coeff N^T fac per Gauss point of the boundary element, fac = w |dA|;
//   Thermo::TimInt::apply_force_external_conv adds them to the internal force and the tangent of the
//   thermal field.  With linear kinematics |dA| is the reference configuration's and the
//   coefficient is constant per face, so per surface
//     M_f,ab = sum_g w_g |dA_g| N_a(g) N_b(g),  m_f,a = sum_g w_g |dA_g| N_a(g),
//     A = sum_f coeff_f M_f,  g = sum_f coeff_f surtemp_f m_f,  q = sum_f flux_f m_f
//   on the surface rows, and per evaluate f_T += s_c (A T - s_t g), K_TT += s_c A; the heat flux
//   load is f_ext += s_q q.  |dA| = |X,r x X,s| at the quad_4point / quad_9point rule's points.
//
// Kernels: surface_setup_kernel (one wavefront per surface row: per incidence of the row, in
// ascending face order, lane g forms the two tangent vectors, |dA| and w |dA| N_a at Gauss point g,
// lane b sums over g in Gauss-point order and adds coeff_f times that into the compact row image in
// LDS, lane 0 carries the row's g and q; the row is written once), convection_apply_kernel (4 / 16 /
// 64 lanes per surface row: the row product A T and K_TT[s_pos] += s_c A in one walk of the compact
// row) and surface_flux_kernel.  Owned rows only, no atomics on doubles, bitwise reproducible.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "fcg_status.hpp"
#include "fcg_tsi_internal.hpp"
#include "fcg_tsi_surface_plan.hpp"
#include "fcg_upload.hpp"
#include "fourc_gpu.h"

struct fcg_tsi_surface {
  fcg_tsi_ctx* ctx = nullptr;
  int nfn = 4;
  int64_t n_faces = 0, nsr = 0, nse = 0, n_inc = 0;
  int max_row = 0;
  bool is_set = false;
  int64_t device_bytes = 0;
  // the plan (fcg_tsi_surface_plan.hpp) and the faces
  int32_t* s_row = nullptr;       // [nsr]
  int64_t* inc_ptr = nullptr;     // [nsr + 1]
  int32_t* inc_face = nullptr;    // [n_inc]
  uint8_t* inc_loc = nullptr;     // [n_inc]
  int64_t* s_ptr = nullptr;       // [nsr + 1]
  int32_t* s_col = nullptr;       // [nse]
  int64_t* s_pos = nullptr;       // [nse]
  uint16_t* slot = nullptr;       // [n_inc][nfn]
  int32_t* face_nodes = nullptr;  // [n_faces][nfn]
  double* tables = nullptr;       // N | dN/dr | dN/ds at the Gauss points | w
  // the condition's per-face values and what the setup kernel makes of them
  double* coeff = nullptr;        // [n_faces]
  double* surtemp = nullptr;      // [n_faces]
  double* flux = nullptr;         // [n_faces]
  double* A = nullptr;            // [nse]
  double* g = nullptr;            // [nsr]
  double* q = nullptr;            // [nsr]
  int32_t* err = nullptr;         // [2]
};

namespace fcg {
namespace {

namespace splan = tsi_surface_plan;

constexpr int kApplyBlock = 256;

struct SurfaceSetupArgs {
  int64_t nsr;
  const int64_t* inc_ptr;
  const int32_t* inc_face;
  const uint8_t* inc_loc;
  const uint16_t* slot;
  const int64_t* s_ptr;
  const int32_t* face_nodes;
  const double* node_x;
  const double* tables;
  const double* coeff;
  const double* surtemp;
  const double* flux;
  double* A;
  double* g;
  double* q;
  int32_t* err;
};

template <int NFN>
__global__ __launch_bounds__(64) void surface_setup_kernel(SurfaceSetupArgs S)
{
  constexpr int NGP = NFN;
  constexpr int MAXN = NFN == 4 ? 27 : 125;  // a compact row is part of a k_TT row
  __shared__ double sN[NGP * NFN];   // [g][n]
  __shared__ double sdr[NGP * NFN];  // dN/dr [g][n]
  __shared__ double sds[NGP * NFN];  // dN/ds [g][n]
  __shared__ double sw[NGP];
  __shared__ double sX[NFN * 3];
  __shared__ double sfa[NGP];        // w |dA| N_a at the Gauss points
  __shared__ double img[MAXN];
  const int lane = threadIdx.x;
  for (int v = lane; v < NGP * NFN; v += 64)
  {
    sN[v] = S.tables[v];
    sdr[v] = S.tables[NGP * NFN + v];
    sds[v] = S.tables[2 * NGP * NFN + v];
  }
  if (lane < NGP) sw[lane] = S.tables[3 * NGP * NFN + lane];

  for (int64_t i = blockIdx.x; i < S.nsr; i += gridDim.x)
  {
    const int64_t b0 = S.s_ptr[i];
    const int len = int(S.s_ptr[i + 1] - b0);
    for (int v = lane; v < MAXN; v += 64) img[v] = 0.0;
    double gi = 0.0, qi = 0.0;  // lane 0's
    for (int64_t k = S.inc_ptr[i]; k < S.inc_ptr[i + 1]; ++k)
    {
      const int32_t f = S.inc_face[k];
      const int a = S.inc_loc[k];
      const int32_t* fn = S.face_nodes + int64_t(f) * NFN;
      __syncthreads();  // the previous incidence has read sX and sfa
      for (int v = lane; v < 3 * NFN; v += 64)
      {
        const int c = v / 3, d = v - 3 * c;
        sX[v] = S.node_x[3 * int64_t(fn[c]) + d];
      }
      __syncthreads();
      if (lane < NGP)
      {
        const double* dr = sdr + NFN * lane;
        const double* ds = sds + NFN * lane;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int c = 0; c < NFN; ++c)
        {
          const double x0 = sX[3 * c], x1 = sX[3 * c + 1], x2 = sX[3 * c + 2];
          r0 += dr[c] * x0; r1 += dr[c] * x1; r2 += dr[c] * x2;
          s0 += ds[c] * x0; s1 += ds[c] * x1; s2 += ds[c] * x2;
        }
        const double n0 = r1 * s2 - r2 * s1, n1 = r2 * s0 - r0 * s2, n2 = r0 * s1 - r1 * s0;
        const double dA = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        if (!(dA > 0.0 && dA < HUGE_VAL))  // zero, infinite or not a number
        {
          atomicMax(&S.err[0], int(FCG_ERR_SINGULAR));
          atomicMin(&S.err[1], f);
        }
        sfa[lane] = (sw[lane] * dA) * sN[NFN * lane + a];
      }
      __syncthreads();
      if (lane < NFN)
      {
        double s = 0.0;
        for (int g = 0; g < NGP; ++g) s += sfa[g] * sN[NFN * g + lane];
        img[S.slot[k * NFN + lane]] += S.coeff[f] * s;  // the nodes of a face have distinct columns
      }
      if (lane == 0)
      {
        double m = 0.0;
        for (int g = 0; g < NGP; ++g) m += sfa[g];
        gi += (S.coeff[f] * S.surtemp[f]) * m;
        qi += S.flux[f] * m;
      }
    }
    __syncthreads();
    for (int v = lane; v < len; v += 64) S.A[b0 + v] = img[v];
    if (lane == 0)
    {
      S.g[i] = gi;
      S.q[i] = qi;
    }
    __syncthreads();
  }
}

// K_TT[s_pos[k]] <- fma(s_c, A[k], K_TT[s_pos[k]]);  f_T[s_row[i]] += s_c (sum_k A[k] T[s_col[k]] - s_t g[i])
template <int LPR>
__global__ __launch_bounds__(kApplyBlock) void convection_apply_kernel(int64_t n,
    const int32_t* __restrict__ s_row, const int64_t* __restrict__ s_ptr, const int32_t* __restrict__ s_col,
    const int64_t* __restrict__ s_pos, const double* __restrict__ A, const double* __restrict__ g,
    const double* __restrict__ T, double* __restrict__ K, double* __restrict__ f, double s_c, double s_t)
{
  const int lane = threadIdx.x % LPR;
  const int64_t i = (int64_t(blockIdx.x) * kApplyBlock + threadIdx.x) / LPR;
  double acc = 0.0;
  if (i < n)
  {
    const int64_t e = s_ptr[i + 1];
    for (int64_t k = s_ptr[i] + lane; k < e; k += LPR)
    {
      const double a = A[k];
      if (f) acc += a * T[s_col[k]];
      if (K)
      {
        const int64_t p = s_pos[k];
        K[p] = fma(s_c, a, K[p]);
      }
    }
  }
  if (!f) return;  // uniform over the grid
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, LPR);
  if (i < n && lane == 0)
  {
    const int32_t r = s_row[i];
    f[r] += s_c * (acc - s_t * g[i]);
  }
}

__global__ __launch_bounds__(kApplyBlock) void surface_flux_kernel(int64_t n, const int32_t* __restrict__ s_row,
    const double* __restrict__ q, double* __restrict__ f, double s_q)
{
  const int64_t i = int64_t(blockIdx.x) * kApplyBlock + threadIdx.x;
  if (i < n) f[s_row[i]] += s_q * q[i];
}

int surface_grid(int64_t work, int cap) { return int(work < cap ? (work > 0 ? work : 1) : cap); }

// the plan's tables and the buffers of the condition; the first error wins, the later calls still run
hipError_t upload_surface(fcg_tsi_surface* s, const splan::Plan& P, const int32_t* face_nodes,
    const std::vector<double>& tab)
{
  int64_t& bytes = s->device_bytes;
  hipError_t he = hipSuccess;
  auto chk = [&](hipError_t x) {
    if (he == hipSuccess) he = x;
  };
  chk(upload(&s->s_row, P.s_row.data(), s->nsr, bytes));
  chk(upload(&s->inc_ptr, P.inc_ptr.data(), s->nsr + 1, bytes));
  chk(upload(&s->inc_face, P.inc_face.data(), s->n_inc, bytes));
  chk(upload(&s->inc_loc, P.inc_loc.data(), s->n_inc, bytes));
  chk(upload(&s->s_ptr, P.s_ptr.data(), s->nsr + 1, bytes));
  chk(upload(&s->s_col, P.s_col.data(), s->nse, bytes));
  chk(upload(&s->s_pos, P.s_pos.data(), s->nse, bytes));
  chk(upload(&s->slot, P.slot.data(), s->n_inc * s->nfn, bytes));
  chk(upload(&s->face_nodes, face_nodes, s->n_faces * s->nfn, bytes));
  chk(upload(&s->tables, tab.data(), int64_t(tab.size()), bytes));
  chk(upload<double>(&s->coeff, nullptr, s->n_faces, bytes));
  chk(upload<double>(&s->surtemp, nullptr, s->n_faces, bytes));
  chk(upload<double>(&s->flux, nullptr, s->n_faces, bytes));
  chk(upload<double>(&s->A, nullptr, s->nse, bytes));
  chk(upload<double>(&s->g, nullptr, s->nsr, bytes));
  chk(upload<double>(&s->q, nullptr, s->nsr, bytes));
  chk(upload<int32_t>(&s->err, nullptr, 2, bytes));
  return he;
}

// one value per face from the scalar or the table; false (with the face) when `ok` refuses a value
template <class Ok>
bool face_values(std::vector<double>& out, int64_t n, double scalar, const double* table, Ok ok, int64_t& bad)
{
  out.resize(size_t(n));
  for (int64_t f = 0; f < n; ++f)
  {
    const double v = table ? table[f] : scalar;
    if (!ok(v))
    {
      bad = table ? f : (n > 0 ? 0 : -1);
      return false;
    }
    out[size_t(f)] = v;
  }
  if (n == 0 && !table && !ok(scalar))
  {
    bad = -1;
    return false;
  }
  return true;
}

}  // namespace
}  // namespace fcg

extern "C" {

int fcg_tsi_surface_destroy(fcg_tsi_surface* s)
{
  if (!s) return FCG_OK;
  if (s->ctx) (void)hipSetDevice(s->ctx->device);
  void* ptrs[] = {s->s_row, s->inc_ptr, s->inc_face, s->inc_loc, s->s_ptr, s->s_col, s->s_pos, s->slot,
      s->face_nodes, s->tables, s->coeff, s->surtemp, s->flux, s->A, s->g, s->q, s->err};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
  return FCG_OK;
}

// The stages of a surface's creation, in order; the host ones are fcg_tsi_surface_plan.cpp's.  The
// k_TT graph is read back from the context (the descriptor's arrays are the caller's and may be gone).
int fcg_tsi_surface_create(fcg_tsi_ctx* tctx, int64_t n_faces, const int32_t* face_nodes, fcg_tsi_surface** out)
{
  namespace splan = fcg::tsi_surface_plan;
  if (!tctx || !out) return FCG_ERR_ARG;
  *out = nullptr;
  const fcg::TsiDevice& d = tctx->d;
  std::string why;
  auto failed = [&](int rc) {
    if (rc != FCG_OK) tctx->last_error = why;
    return rc != FCG_OK;
  };
  splan::Maps M;
  M.celltype = d.npe == 27 ? FCG_HEX27 : FCG_HEX8;
  M.n_node = d.n_node;
  M.n_rows_t = d.n_rows_t;
  M.n_cols_t = d.n_cols_t;
  M.node_dof_col_t = tctx->h_dof_col_t.data();
  M.node_dof_row_t = tctx->h_dof_row_t.data();
  int rc = splan::check_faces(M, n_faces, face_nodes, why);
  if (failed(rc)) return rc;
  splan::Plan P;
  rc = splan::build_rows(M, n_faces, face_nodes, P, why);
  if (failed(rc)) return rc;
  (void)hipSetDevice(tctx->device);
  std::vector<int64_t> rowptr_tt;
  std::vector<int32_t> col_tt;
  if (P.nsr() > 0)
  {
    rowptr_tt.resize(size_t(d.n_rows_t + 1));
    col_tt.resize(size_t(d.nnz_tt));
    hipError_t he = hipMemcpy(rowptr_tt.data(), d.rowptr_tt, sizeof(int64_t) * rowptr_tt.size(), hipMemcpyDeviceToHost);
    if (he == hipSuccess && d.nnz_tt > 0)
      he = hipMemcpy(col_tt.data(), d.cols_tt, sizeof(int32_t) * col_tt.size(), hipMemcpyDeviceToHost);
    if (he != hipSuccess)
    {
      tctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
      return fcg_device_error();
    }
    M.rowptr_tt = rowptr_tt.data();
    M.col_tt = col_tt.data();
  }
  rc = splan::build_compact_rows(M, face_nodes, P, why);
  if (failed(rc)) return rc;
  const std::vector<double> tables = splan::build_tables(P.nfn);

  fcg_tsi_surface* s = new fcg_tsi_surface();
  s->ctx = tctx;
  s->nfn = P.nfn;
  s->n_faces = n_faces;
  s->nsr = P.nsr();
  s->nse = P.nse();
  s->n_inc = P.n_inc();
  s->max_row = P.max_row;
  const hipError_t he = fcg::upload_surface(s, P, face_nodes, tables);
  if (he != hipSuccess)
  {
    tctx->last_error = std::string("HIP allocation/copy failed: ") + hipGetErrorString(he);
    fcg_tsi_surface_destroy(s);
    return fcg_device_error();
  }
  *out = s;
  return FCG_OK;
}

int fcg_tsi_surface_set(fcg_tsi_surface* s, double coeff, const double* face_coeff, double surtemp,
    const double* face_surtemp, double flux, const double* face_flux, int64_t* bad_face)
{
  if (!s) return FCG_ERR_ARG;
  fcg_tsi_ctx* ctx = s->ctx;
  if (bad_face) *bad_face = -1;
  // every refusal comes before the first write: the tables of an earlier set stay as they were
  std::vector<double> hc, ht, hq;
  int64_t bad = -1;
  auto name = [&](const char* what, const double* table, double scalar) {
    const double v = table && bad >= 0 ? table[bad] : scalar;
    return std::string(table ? "face_" : "") + what + (table ? "[" + std::to_string(bad) + "]" : "") + " = " +
           std::to_string(v) + (bad >= 0 ? " (face " + std::to_string(bad) + ")" : "");
  };
  if (!fcg::face_values(hc, s->n_faces, coeff, face_coeff, [](double v) { return std::isfinite(v) && v >= 0.0; }, bad))
  {
    if (bad_face) *bad_face = bad;
    ctx->last_error = name("coeff", face_coeff, coeff) + ": the heat transfer coefficient must be finite and >= 0";
    return FCG_ERR_ARG;
  }
  if (!fcg::face_values(ht, s->n_faces, surtemp, face_surtemp, [](double v) { return std::isfinite(v); }, bad))
  {
    if (bad_face) *bad_face = bad;
    ctx->last_error = name("surtemp", face_surtemp, surtemp) + ": the surrounding temperature must be finite";
    return FCG_ERR_ARG;
  }
  if (!fcg::face_values(hq, s->n_faces, flux, face_flux, [](double v) { return std::isfinite(v); }, bad))
  {
    if (bad_face) *bad_face = bad;
    ctx->last_error = name("flux", face_flux, flux) + ": the heat flux must be finite";
    return FCG_ERR_ARG;
  }
  if (s->nsr == 0 || s->n_faces == 0)
  {
    s->is_set = true;
    return FCG_OK;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  // an apply of the earlier tables may still run on a stream of the caller's
  hipError_t he = hipDeviceSynchronize();
  const size_t nb = sizeof(double) * size_t(s->n_faces);
  if (he == hipSuccess) he = hipMemcpy(s->coeff, hc.data(), nb, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(s->surtemp, ht.data(), nb, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(s->flux, hq.data(), nb, hipMemcpyHostToDevice);
  const int32_t init[2] = {0, INT32_MAX};
  if (he == hipSuccess) he = hipMemcpyAsync(s->err, init, sizeof(init), hipMemcpyHostToDevice, st);
  if (he == hipSuccess)
  {
    fcg::SurfaceSetupArgs a;
    a.nsr = s->nsr;
    a.inc_ptr = s->inc_ptr;
    a.inc_face = s->inc_face;
    a.inc_loc = s->inc_loc;
    a.slot = s->slot;
    a.s_ptr = s->s_ptr;
    a.face_nodes = s->face_nodes;
    a.node_x = ctx->d.node_x;
    a.tables = s->tables;
    a.coeff = s->coeff;
    a.surtemp = s->surtemp;
    a.flux = s->flux;
    a.A = s->A;
    a.g = s->g;
    a.q = s->q;
    a.err = s->err;
    const int grid = fcg::surface_grid(s->nsr, 256 * 32);
    if (s->nfn == 4)
      hipLaunchKernelGGL(fcg::surface_setup_kernel<4>, dim3(grid), dim3(64), 0, st, a);
    else
      hipLaunchKernelGGL(fcg::surface_setup_kernel<9>, dim3(grid), dim3(64), 0, st, a);
    he = hipGetLastError();
  }
  int32_t errv[2] = {0, INT32_MAX};
  if (he == hipSuccess) he = hipMemcpyAsync(errv, s->err, sizeof(errv), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess)
  {
    s->is_set = false;
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (errv[0] != 0)
  {
    const int64_t face = errv[1] == INT32_MAX ? -1 : errv[1];
    if (bad_face) *bad_face = face;
    s->is_set = false;  // the tables hold the degenerate face's values
    ctx->last_error = "zero or non-finite area element |dA| in face " + std::to_string(face);
    return errv[0];
  }
  s->is_set = true;
  return FCG_OK;
}

int fcg_tsi_surface_info(const fcg_tsi_surface* s, int64_t* n_rows, int64_t* n_entries, int64_t* device_bytes)
{
  if (!s) return FCG_ERR_ARG;
  if (n_rows) *n_rows = s->nsr;
  if (n_entries) *n_entries = s->nse;
  if (device_bytes) *device_bytes = s->device_bytes;
  return FCG_OK;
}

int fcg_tsi_surface_tables(const fcg_tsi_surface* s, const int32_t** d_rows, const int64_t** d_ptr,
    const int32_t** d_col, const int64_t** d_pos, const double** d_A, const double** d_g, const double** d_q)
{
  if (!s) return FCG_ERR_ARG;
  if (d_rows) *d_rows = s->s_row;
  if (d_ptr) *d_ptr = s->s_ptr;
  if (d_col) *d_col = s->s_col;
  if (d_pos) *d_pos = s->s_pos;
  if (d_A) *d_A = s->A;
  if (d_g) *d_g = s->g;
  if (d_q) *d_q = s->q;
  return FCG_OK;
}

int fcg_tsi_convection(fcg_tsi_surface* s, double coeff_scale, double surtemp_scale, const double* d_T_col,
    double* d_fT_row, double* d_Ktt, void* stream_ptr)
{
  if (!s) return FCG_ERR_ARG;
  fcg_tsi_ctx* ctx = s->ctx;
  if (!s->is_set)
  {
    ctx->last_error = "fcg_tsi_convection before a successful fcg_tsi_surface_set";
    return FCG_ERR_ARG;
  }
  if (s->nsr == 0) return FCG_OK;
  if ((!d_fT_row && !d_Ktt) || (d_fT_row && !d_T_col))
  {
    ctx->last_error = "invalid convection arguments: no output, or a residual without the temperatures";
    return FCG_ERR_ARG;
  }
  if (!std::isfinite(coeff_scale) || !std::isfinite(surtemp_scale))
  {
    ctx->last_error = "the scales of a convection condition must be finite";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t st = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  // lanes per row by the longest compact row, as fcg_tsi_ost_combine chooses them
  const int lanes = s->max_row <= 8 ? 4 : s->max_row <= 48 ? 16 : 64;
  const unsigned blocks = unsigned((s->nsr * lanes + fcg::kApplyBlock - 1) / fcg::kApplyBlock);
  if (lanes == 4)
    hipLaunchKernelGGL(fcg::convection_apply_kernel<4>, dim3(blocks), dim3(fcg::kApplyBlock), 0, st, s->nsr,
        s->s_row, s->s_ptr, s->s_col, s->s_pos, s->A, s->g, d_T_col, d_Ktt, d_fT_row, coeff_scale, surtemp_scale);
  else if (lanes == 16)
    hipLaunchKernelGGL(fcg::convection_apply_kernel<16>, dim3(blocks), dim3(fcg::kApplyBlock), 0, st, s->nsr,
        s->s_row, s->s_ptr, s->s_col, s->s_pos, s->A, s->g, d_T_col, d_Ktt, d_fT_row, coeff_scale, surtemp_scale);
  else
    hipLaunchKernelGGL(fcg::convection_apply_kernel<64>, dim3(blocks), dim3(fcg::kApplyBlock), 0, st, s->nsr,
        s->s_row, s->s_ptr, s->s_col, s->s_pos, s->A, s->g, d_T_col, d_Ktt, d_fT_row, coeff_scale, surtemp_scale);
  if (hipGetLastError() != hipSuccess)
  {
    ctx->last_error = "HIP: the convection kernel did not launch";
    return fcg_device_error();
  }
  return FCG_OK;
}

int fcg_tsi_surface_flux(fcg_tsi_surface* s, double scale, double* d_f_row, void* stream_ptr)
{
  if (!s) return FCG_ERR_ARG;
  fcg_tsi_ctx* ctx = s->ctx;
  if (!s->is_set)
  {
    ctx->last_error = "fcg_tsi_surface_flux before a successful fcg_tsi_surface_set";
    return FCG_ERR_ARG;
  }
  if (s->nsr == 0) return FCG_OK;
  if (!d_f_row || !std::isfinite(scale))
  {
    ctx->last_error = "invalid heat flux arguments: no output, or a scale that is not finite";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t st = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  const unsigned blocks = unsigned((s->nsr + fcg::kApplyBlock - 1) / fcg::kApplyBlock);
  hipLaunchKernelGGL(fcg::surface_flux_kernel, dim3(blocks), dim3(fcg::kApplyBlock), 0, st, s->nsr, s->s_row, s->q,
      d_f_row, scale);
  if (hipGetLastError() != hipSuccess)
  {
    ctx->last_error = "HIP: the heat flux kernel did not launch";
    return fcg_device_error();
  }
  return FCG_OK;
}

}  // extern "C"
