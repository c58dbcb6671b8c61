// fcg_mass.hip -- inertia for structural dynamics (DYNAMICTYPE GenAlpha): the consistent mass of
// the displacement-based solid elements and the effective tangent of the time integrator.
//
// Reference: struct_calc_nlnstiffmass fills systemmatrix2 with
//   M_(3a+d)(3b+d) = sum_g rho w_g det J_g N_a(xi_g) N_b(xi_g)
// (the mass part of evaluate_nonlinear_force_stiffness_mass, 4C_solid_3D_ele_calc.cpp) on the
// element's stiffness Gauss rule, J from the reference coordinates; LUMPMASS lumps by row sums.
// The block between two nodes is m_ab I_3, so the
// time integrator keeps one double per (row node, neighbour node) -- nnz / 9 -- and the full CSR
// form exists for hosts that want systemmatrix2.
//
//  * mass plan (first mass call, kept on the context): per column node with an owned row the list
//    of its (column element, local node) incidences, ascending by element -- count, scan, fill and
//    a per-node sort, so the summation order does not depend on the order atomics hand out slots;
//  * mass_kernel: one wavefront per owned row node walks that list, integrates m_ab for the
//    element's nodes b and adds it at b's position in the node's sorted row (binary search);
//  * efft_kernel: K <- cK K + cM M in place and / or y = M x from the compact form, one pass over
//    the node rows (the per-Newton-iteration kernel of 4c_amd/dynamics.py).
// No atomics on doubles anywhere: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "fcg_internal.hpp"
#include "fcg_shape.hpp"
#include "fcg_status.hpp"

namespace fcg {

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t work, int cap) { return int(work < cap ? (work > 0 ? work : 1) : cap); }

hipError_t exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, hipStream_t s)
{
  size_t bytes = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, int64_t(0), size_t(n),
      rocprim::plus<int64_t>(), s);
  if (e != hipSuccess) return e;
  void* tmp = nullptr;
  e = hipMallocAsync(&tmp, bytes > 0 ? bytes : 1, s);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(tmp, bytes, in, out, int64_t(0), size_t(n), rocprim::plus<int64_t>(), s);
  hipError_t f = hipFreeAsync(tmp, s);
  return e != hipSuccess ? e : f;
}

// The Gauss rule of the mass: the element's stiffness rule, with the 27-point rule's constants in
// full double precision (sqrt(3/5), 5/9, 8/9).  fcg_shape.hpp's gauss_rule keeps the reference's
// 13-digit constants for the stiffness, whose weights sum to 8 (1 + 1.5e-13); carried into the mass
// that factor would sit on every entry and on the total mass, which the partition of unity otherwise
// gives as rho V to rounding (det J of a hex27 is of degree 5 per direction: integrated exactly).
// The entries differ from the 13-digit rule's by 1.5e-13 relative.  hex8: the same rule (w = 1).
void mass_gauss_rule(int celltype, double* xi, double* w)
{
  gauss_rule(celltype, xi, w);
  if (celltype != kHex27) return;
  const double a = std::sqrt(0.6), w1 = 5.0 / 9.0, w2 = 8.0 / 9.0;
  for (int g = 0; g < 27; ++g)
  {
    double wg[3];
    for (int d = 0; d < 3; ++d)
    {
      const int p = kHex27NodePos[g][d];
      xi[3 * g + d] = p == 0 ? -a : (p == 2 ? a : 0.0);
      wg[d] = p == 1 ? w2 : w1;
    }
    w[g] = wg[0] * wg[1] * wg[2];
  }
}

// ---------------------------------------------------------------------------- the mass plan
__global__ void mass_count(int64_t n_all, const int32_t* __restrict__ ele_nodes,
    const int32_t* __restrict__ dof_row, int64_t* cnt)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n_all;
       i += int64_t(gridDim.x) * blockDim.x)
  {
    const int32_t n = ele_nodes[i];
    if (dof_row[n] >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[n]), 1ull);
  }
}

// incidence key = element * 32 + local node (npe <= 27), so that sorting the keys sorts by element
__global__ void mass_fill(int64_t n_all, int npe, const int32_t* __restrict__ ele_nodes,
    const int32_t* __restrict__ dof_row, const int64_t* __restrict__ ptr, int64_t* cursor,
    int64_t* inc)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n_all;
       i += int64_t(gridDim.x) * blockDim.x)
  {
    const int32_t n = ele_nodes[i];
    if (dof_row[n] < 0) continue;
    const unsigned long long k = atomicAdd(reinterpret_cast<unsigned long long*>(&cursor[n]), 1ull);
    const int64_t e = i / npe;
    inc[ptr[n] + int64_t(k)] = e * 32 + (i - e * npe);
  }
}

// the short lists in ascending order (insertion sort, one thread per node)
__global__ void mass_sort(int64_t n_node, const int64_t* __restrict__ ptr, int64_t* inc)
{
  for (int64_t n = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; n < n_node;
       n += int64_t(gridDim.x) * blockDim.x)
  {
    const int64_t k0 = ptr[n], k1 = ptr[n + 1];
    for (int64_t i = k0 + 1; i < k1; ++i)
    {
      const int64_t v = inc[i];
      int64_t j = i;
      for (; j > k0 && inc[j - 1] > v; --j) inc[j] = inc[j - 1];
      inc[j] = v;
    }
  }
}

// ---------------------------------------------------------------------------- mass integration
// tab: N[NGP][NPE] | dN[NGP][NPE][3] | w[NGP] at the points of mass_gauss_rule.
// One wavefront per column node n with an owned row.  Per incidence (e, a): lane g forms det J at
// Gauss point g and c_g = w_g det J_g N_a(xi_g); lane b sums m_ab = sum_g c_g N_b(xi_g) in Gauss
// point order and adds rho_e m_ab at the position of b's column triple in the node's sorted row
// (distinct b -> distinct positions; the incidences run one after the other).  acc[] in LDS is the
// node's compact row.  Outputs, each optional: the CSR values (3 rows; OVERWRITE writes every
// entry of the rows, ACCUMULATE adds the block diagonals), the compact row, the row sum.
struct MassArgs {
  const int32_t* ele_nodes;
  const double* node_x;
  const int32_t* dof_row;
  const int32_t* kcol;
  const int64_t* rowptr;
  const int32_t* col_lid;
  const int64_t* ptr;
  const int64_t* inc;
  const double* tab;
  const double* ele_rho;  // [n_ele] or NULL
  double rho;
  int64_t n_node;
  int max_rowlen;  // the LDS row's capacity
  double* M;       // [nnz] or NULL
  int overwrite;
  double* m_node;  // [nnz / 9] or NULL
  double* lumped;  // [n_rows] or NULL
  int32_t* flag;     // solver flag word: 1 = det J <= 0 at a Gauss point
  int32_t* bad_ele;  // lowest column element with such a point
};

template <int NPE, int NGP>
__global__ __launch_bounds__(64) void mass_kernel(MassArgs A)
{
  extern __shared__ double lds[];
  __shared__ double cg[32];
  double* acc = lds;  // [max_rowlen]: acc[p] = m of the triple that starts at position p
  const double* Ntab = A.tab;
  const double* dN = A.tab + NGP * NPE;
  const double* wg = dN + NGP * NPE * 3;
  const int lane = threadIdx.x;
  for (int64_t n = blockIdx.x; n < A.n_node; n += gridDim.x)
  {
    const int32_t row0 = A.dof_row[n];
    if (row0 < 0) continue;  // uniform over the wavefront
    const int64_t s = A.rowptr[row0];
    const int len = int(A.rowptr[row0 + 1] - s);
    if (len > A.max_rowlen) continue;  // cannot happen: max_rowlen is the longest node row
    for (int p = lane; p < len; p += 64) acc[p] = 0.0;
    __syncthreads();
    const int64_t k0 = A.ptr[n], k1 = A.ptr[n + 1];
    for (int64_t k = k0; k < k1; ++k)
    {
      const int64_t key = A.inc[k];
      const int64_t e = key >> 5;
      const int a = int(key & 31);
      const int32_t* en = A.ele_nodes + e * NPE;
      if (lane < NGP)
      {
        double J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const double* d = dN + lane * NPE * 3;
        for (int b = 0; b < NPE; ++b)
        {
          const double* X = A.node_x + 3 * int64_t(en[b]);
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) J[3 * i + j] += d[3 * b + i] * X[j];
        }
        const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) +
                           J[2] * (J[3] * J[7] - J[4] * J[6]);
        if (!(det > 0.0))
        {
          atomicMax(A.flag, 1);
          atomicMin(A.bad_ele, int32_t(e));
        }
        cg[lane] = wg[lane] * det * Ntab[lane * NPE + a];
      }
      __syncthreads();
      if (lane < NPE)
      {
        double mab = 0.0;
        for (int g = 0; g < NGP; ++g) mab += cg[g] * Ntab[g * NPE + lane];
        const double rho = A.ele_rho ? A.ele_rho[e] : A.rho;
        const int32_t c = A.kcol[en[lane]];
        // position of the column triple in the sorted row
        int lo = 0, hi = len;
        while (lo < hi)
        {
          const int mid = (lo + hi) >> 1;
          if (A.col_lid[s + mid] < c) lo = mid + 1;
          else hi = mid;
        }
        if (lo + 2 < len && A.col_lid[s + lo] == c) acc[lo] += rho * mab;
      }
      __syncthreads();
    }
    if (A.M)
    {
      // is position p the start of a node's triple?  Every triple of an element node was found
      // above; columns no element node owns (a caller's extra couplings) carry no mass.
      for (int j = lane; j < 3 * len; j += 64)
      {
        const int d = (j >= len) + (j >= 2 * len);
        const int p = j - d * len;
        const double v = p >= d ? acc[p - d] : 0.0;  // acc is 0 off the triple starts
        // acc[p - d] != 0 only at a triple start, and then p is the triple's entry d
        if (A.overwrite) A.M[s + j] = v;
        else if (v != 0.0) A.M[s + j] += v;
      }
    }
    if (A.m_node)
      for (int t = lane; 3 * t < len; t += 64) A.m_node[s / 9 + t] = acc[3 * t];
    if (A.lumped && lane == 0)
    {
      double sum = 0.0;
      for (int p = 0; p < len; ++p) sum += acc[p];  // zeros between the triple starts
      A.lumped[row0] = sum;
      A.lumped[row0 + 1] = sum;
      A.lumped[row0 + 2] = sum;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------- effective tangent
// One node per LPN lanes, as spmv_node_kernel, but over the node's 3 len contiguous K values as
// one flat range [s, s + 3 len): entry j lies in row d = j / len at position p = j - d len, in the
// triple t = p / 3; it is on its block's diagonal when p - 3 t == d.  Flat, the stores are
// contiguous over the lanes and go in 16-byte pairs from the first even index on (s is a multiple
// of 9, so every other node row starts odd: one scalar head entry, then pairs, then a scalar tail).
//   KM 0: K not touched, 1: K = cM M (K not read: cK == 0), 2: K = cK K + cM M
//   Y: y_row = M x_col, partial sums per lane in flat order, then the lanes in butterfly order.
// The K loads depend on nothing but the loop index, the m_node loads neither (1/9 of the bytes);
// only x waits for its column index, and only when Y.
template <int KM, bool Y>
__device__ inline double efft_entry(int64_t s, int j, int len, const double* __restrict__ mb,
    const int32_t* __restrict__ col, const double* __restrict__ x, double kin, double cK, double cM,
    double& a0, double& a1, double& a2)
{
  const int d = (j >= len) + (j >= 2 * len);
  const int p = j - d * len;
  const int t = p / 3;
  const double kd = KM == 2 ? __dmul_rn(cK, kin) : 0.0;
  if (p - 3 * t != d) return kd;
  const double m = mb[t];
  if (Y)
  {
    const double v = m * x[col[s + p]];
    if (d == 0) a0 += v;
    else if (d == 1) a1 += v;
    else a2 += v;
  }
  return __fma_rn(cM, m, kd);
}

template <int LPN, int KM, bool Y>
__global__ __launch_bounds__(kBlock) void efft_kernel(const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ row0_of, const int32_t* __restrict__ col,
    const double* __restrict__ m_node, double* K, const double* __restrict__ x,
    double* __restrict__ y, int64_t n_nodes, double cK, double cM)
{
  const int lane = threadIdx.x % LPN;
  const int64_t node = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPN;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int32_t row0 = 0;
  if (node < n_nodes)
  {
    row0 = row0_of[node];
    const int64_t s = rowptr[row0];
    const int len = int(rowptr[row0 + 1] - s);
    const int n3 = 3 * len;
    const double* mb = m_node + s / 9;
    const int head = int(s & 1);
    if (head && lane == 0 && n3 > 0)
    {
      const double k = efft_entry<KM, Y>(s, 0, len, mb, col, x, KM == 2 ? K[s] : 0.0, cK, cM, a0, a1, a2);
      if (KM) K[s] = k;
    }
    for (int j = head + 2 * lane; j + 1 < n3; j += 2 * LPN)
    {
      double2 kv = make_double2(0.0, 0.0);
      if (KM == 2) kv = *reinterpret_cast<const double2*>(K + s + j);
      kv.x = efft_entry<KM, Y>(s, j, len, mb, col, x, kv.x, cK, cM, a0, a1, a2);
      kv.y = efft_entry<KM, Y>(s, j + 1, len, mb, col, x, kv.y, cK, cM, a0, a1, a2);
      if (KM) *reinterpret_cast<double2*>(K + s + j) = kv;
    }
    // the last entry when the pairs leave one over: its lane is the one whose pair would start there
    const int jt = n3 - 1;
    if (n3 > head && ((n3 - head) & 1) && lane == ((jt - head) / 2) % LPN)
    {
      const double k = efft_entry<KM, Y>(s, jt, len, mb, col, x, KM == 2 ? K[s + jt] : 0.0, cK, cM, a0, a1, a2);
      if (KM) K[s + jt] = k;
    }
  }
  if (Y)
  {
#pragma unroll
    for (int o = LPN / 2; o >= 1; o >>= 1)
    {
      a0 += __shfl_xor(a0, o, LPN);
      a1 += __shfl_xor(a1, o, LPN);
      a2 += __shfl_xor(a2, o, LPN);
    }
    if (node < n_nodes && lane == 0)
    {
      y[row0] = a0;
      y[row0 + 1] = a1;
      y[row0 + 2] = a2;
    }
  }
}

template <int LPN>
hipError_t launch_efft_lpn(const DeviceMesh& m, double cK, double cM, const double* m_node, double* K,
    const double* x, double* y, hipStream_t s)
{
  const dim3 grid(unsigned((m.n_rownodes * LPN + kBlock - 1) / kBlock)), block(kBlock);
  const int km = !K ? 0 : (cK == 0.0 ? 1 : 2);
#define FCG_EFFT(KM, Y)                                                                          \
  hipLaunchKernelGGL((efft_kernel<LPN, KM, Y>), grid, block, 0, s, m.rowptr, m.rownode_row0,     \
      m.col_lid, m_node, K, x, y, m.n_rownodes, cK, cM)
  if (y)
  {
    if (km == 0) FCG_EFFT(0, true);
    else if (km == 1) FCG_EFFT(1, true);
    else FCG_EFFT(2, true);
  }
  else
  {
    if (km == 1) FCG_EFFT(1, false);
    else FCG_EFFT(2, false);
  }
#undef FCG_EFFT
  return hipGetLastError();
}

}  // namespace

hipError_t launch_effective_tangent(const DeviceMesh& m, double cK, double cM, const double* d_m_node,
    double* d_K, const double* d_x_col, double* d_y_row, hipStream_t s)
{
  if (m.n_rownodes == 0) return hipSuccess;
  return m.npe == 27 ? launch_efft_lpn<64>(m, cK, cM, d_m_node, d_K, d_x_col, d_y_row, s)
                     : launch_efft_lpn<16>(m, cK, cM, d_m_node, d_K, d_x_col, d_y_row, s);
}

hipError_t mass_plan_build(DeviceMesh& m, int64_t& bytes, hipStream_t s)
{
  if (m.mass_ptr) return hipSuccess;
  const int64_t n_all = m.n_ele * m.npe;
  const int ngp = m.npe;  // hex8: 8 points, hex27: 27 (the stiffness rules)
  int64_t *cnt = nullptr, *cursor = nullptr, *ptr = nullptr, *inc = nullptr;
  double* tab = nullptr;
  int32_t* bad = nullptr;
  hipError_t he = hipSuccess;
  auto chk = [&](hipError_t x) {
    if (he == hipSuccess) he = x;
  };
  const size_t nb = sizeof(int64_t) * size_t(m.n_node + 1);
  chk(hipMalloc(reinterpret_cast<void**>(&cnt), nb));
  chk(hipMalloc(reinterpret_cast<void**>(&cursor), nb));
  chk(hipMalloc(reinterpret_cast<void**>(&ptr), nb));
  if (he == hipSuccess)
  {
    chk(hipMemsetAsync(cnt, 0, nb, s));
    chk(hipMemsetAsync(cursor, 0, nb, s));
  }
  const int grida = grid_for((n_all + 255) / 256, 256 * 16);
  const int gridn = grid_for((m.n_node + 255) / 256, 256 * 16);
  if (he == hipSuccess && n_all > 0)
  {
    hipLaunchKernelGGL(mass_count, dim3(grida), dim3(256), 0, s, n_all, m.ele_nodes, m.node_dof_row, cnt);
    chk(hipGetLastError());
  }
  if (he == hipSuccess) he = exclusive_scan_i64(cnt, ptr, m.n_node + 1, s);
  int64_t n_inc = 0;
  chk(hipMemcpyAsync(&n_inc, ptr + m.n_node, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  chk(hipStreamSynchronize(s));
  const size_t ib = sizeof(int64_t) * size_t(std::max<int64_t>(n_inc, 1));
  chk(hipMalloc(reinterpret_cast<void**>(&inc), ib));
  if (he == hipSuccess && n_all > 0)
  {
    hipLaunchKernelGGL(mass_fill, dim3(grida), dim3(256), 0, s, n_all, m.npe, m.ele_nodes,
        m.node_dof_row, ptr, cursor, inc);
    chk(hipGetLastError());
    hipLaunchKernelGGL(mass_sort, dim3(gridn), dim3(256), 0, s, m.n_node, ptr, inc);
    chk(hipGetLastError());
  }
  // N | dN | w at the Gauss points of the mass rule
  std::vector<double> t(size_t(ngp) * m.npe * 4 + ngp);
  {
    double xi[81], w[27];
    mass_gauss_rule(m.celltype, xi, w);
    for (int g = 0; g < ngp; ++g)
    {
      shape_values(m.celltype, &xi[3 * g], &t[size_t(g) * m.npe]);
      shape_deriv(m.celltype, &xi[3 * g], &t[size_t(ngp) * m.npe + size_t(g) * m.npe * 3]);
      t[size_t(ngp) * m.npe * 4 + g] = w[g];
    }
  }
  const size_t tb = sizeof(double) * t.size();
  chk(hipMalloc(reinterpret_cast<void**>(&tab), tb));
  chk(hipMalloc(reinterpret_cast<void**>(&bad), sizeof(int32_t)));
  if (he == hipSuccess) chk(hipMemcpyAsync(tab, t.data(), tb, hipMemcpyHostToDevice, s));
  chk(hipStreamSynchronize(s));  // t and the sort are done before anything is handed over or freed
  if (cnt) (void)hipFree(cnt);
  if (cursor) (void)hipFree(cursor);
  if (he != hipSuccess)
  {
    for (void* p : {static_cast<void*>(ptr), static_cast<void*>(inc), static_cast<void*>(tab),
             static_cast<void*>(bad)})
      if (p) (void)hipFree(p);
    return he;
  }
  m.mass_ptr = ptr;
  m.mass_inc = inc;
  m.mass_tab = tab;
  m.mass_bad = bad;
  bytes += int64_t(nb + ib + tb + sizeof(int32_t));
  return hipSuccess;
}

hipError_t launch_mass(const DeviceMesh& m, double density, const double* d_ele_density,
    double* d_M, bool overwrite, double* d_m_node, double* d_lumped, hipStream_t s)
{
  MassArgs A;
  A.ele_nodes = m.ele_nodes;
  A.node_x = m.node_x;
  A.dof_row = m.node_dof_row;
  A.kcol = m.node_dof_kcol ? m.node_dof_kcol : m.node_dof_col;
  A.rowptr = m.rowptr;
  A.col_lid = m.col_lid;
  A.ptr = m.mass_ptr;
  A.inc = m.mass_inc;
  A.tab = m.mass_tab;
  A.ele_rho = d_ele_density;
  A.rho = density;
  A.n_node = m.n_node;
  A.max_rowlen = std::max<int32_t>(m.max_rowlen, 1);
  A.M = d_M;
  A.overwrite = overwrite ? 1 : 0;
  A.m_node = d_m_node;
  A.lumped = d_lumped;
  A.flag = m.err + 2;
  A.bad_ele = m.mass_bad;
  const size_t lds = sizeof(double) * size_t(std::max<int32_t>(m.max_rowlen, 1));
  const dim3 grid(grid_for(m.n_node, 256 * 64)), block(64);
  if (m.npe == 27) hipLaunchKernelGGL((mass_kernel<27, 27>), grid, block, lds, s, A);
  else hipLaunchKernelGGL((mass_kernel<8, 8>), grid, block, lds, s, A);
  return hipGetLastError();
}

}  // namespace fcg

namespace {

// what the two mass entry points share: checks, the plan, the density table, the launch and the
// flag (the stream has drained when this returns)
int mass_call(fcg_ctx* ctx, const char* who, double density, const double* ele_density, double* d_M,
    bool overwrite, double* d_m_node, double* d_lumped, void* stream)
{
  fcg::DeviceMesh& m = ctx->mesh;
  if (ele_density)
  {
    for (int64_t e = 0; e < m.n_ele; ++e)
      if (!(ele_density[e] > 0.0))
      {
        ctx->last_error = std::string(who) + ": ele_density[" + std::to_string(e) + "] = " +
                          std::to_string(ele_density[e]) + " is not positive";
        return FCG_ERR_ARG;
      }
  }
  else if (!(density > 0.0))
  {
    ctx->last_error = std::string(who) + ": density = " + std::to_string(density) + " is not positive";
    return FCG_ERR_ARG;
  }
  if (m.n_rows == 0) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  hipError_t he = fcg::mass_plan_build(m, ctx->device_bytes, s);
  if (he == hipSuccess && ele_density && m.n_ele > 0)
  {
    if (!m.mass_rho)
    {
      he = hipMalloc(reinterpret_cast<void**>(&m.mass_rho), sizeof(double) * size_t(m.n_ele));
      if (he == hipSuccess) ctx->device_bytes += int64_t(sizeof(double)) * m.n_ele;
      else m.mass_rho = nullptr;
    }
    // an earlier mass call on another stream may still read the table
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he == hipSuccess)
      he = hipMemcpy(m.mass_rho, ele_density, sizeof(double) * size_t(m.n_ele), hipMemcpyHostToDevice);
  }
  int32_t bad = 0, bad_ele = 0, gid = -1;
  int32_t* flag = m.err + 2;  // the solver flag word: evaluate's sticky flags are left alone
  if (he == hipSuccess) he = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
  if (he == hipSuccess) he = hipMemsetAsync(m.mass_bad, 0x7f, sizeof(int32_t), s);
  if (he == hipSuccess)
    he = fcg::launch_mass(m, density, ele_density ? m.mass_rho : nullptr, d_M, overwrite, d_m_node,
        d_lumped, s);
  if (he == hipSuccess) he = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipMemcpyAsync(&bad_ele, m.mass_bad, sizeof(bad_ele), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he == hipSuccess && bad && bad_ele >= 0 && bad_ele < m.n_ele)
    he = hipMemcpy(&gid, m.ele_gid + bad_ele, sizeof(gid), hipMemcpyDeviceToHost);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string(who) + ": HIP: " + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (bad)
  {
    ctx->last_error = std::string(who) + ": det J <= 0 at a Gauss point of element GID " +
                      std::to_string(gid);
    return FCG_ERR_NODAL_DETJ;
  }
  return FCG_OK;
}

// the compact node form needs rows that are all owned nodes' DOF triples
bool node_form(fcg_ctx* ctx, const char* who)
{
  const fcg::DeviceMesh& m = ctx->mesh;
  if (m.triple_rows && 3 * m.n_rownodes == m.n_rows) return true;
  ctx->last_error = std::string(who) + ": every owned row must belong to an owned node's DOF triple "
                    "and hold node DOF triples only (fcg_mass_assemble takes any graph)";
  return false;
}

}  // namespace

extern "C" {

int fcg_mass_assemble(fcg_ctx* ctx, double density, const double* ele_density, int mode,
    double* d_M_vals, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE)
  {
    ctx->last_error = "fcg_mass_assemble: mode must be FCG_ACCUMULATE or FCG_OVERWRITE";
    return FCG_ERR_ARG;
  }
  if (ctx->mesh.n_rows > 0 && !d_M_vals)
  {
    ctx->last_error = "fcg_mass_assemble: d_M_vals is NULL";
    return FCG_ERR_ARG;
  }
  return mass_call(ctx, "fcg_mass_assemble", density, ele_density, d_M_vals, mode == FCG_OVERWRITE,
      nullptr, nullptr, stream);
}

int fcg_mass_nodal(fcg_ctx* ctx, double density, const double* ele_density, double* d_m_node,
    double* d_m_lumped_row, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!node_form(ctx, "fcg_mass_nodal")) return FCG_ERR_ARG;
  if (ctx->mesh.n_rows > 0 && !d_m_node && !d_m_lumped_row)
  {
    ctx->last_error = "fcg_mass_nodal: neither d_m_node nor d_m_lumped_row given";
    return FCG_ERR_ARG;
  }
  return mass_call(ctx, "fcg_mass_nodal", density, ele_density, nullptr, false, d_m_node,
      d_m_lumped_row, stream);
}

int fcg_effective_tangent(fcg_ctx* ctx, double cK, double cM, const double* d_m_node,
    double* d_K_vals, const double* d_x_col, double* d_y_row, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!node_form(ctx, "fcg_effective_tangent")) return FCG_ERR_ARG;
  if (ctx->mesh.n_rows == 0) return FCG_OK;
  if (!d_K_vals && !d_x_col && !d_y_row)
  {
    ctx->last_error = "fcg_effective_tangent: d_K_vals, d_x_col and d_y_row are all NULL";
    return FCG_ERR_ARG;
  }
  if (!d_m_node || (d_x_col == nullptr) != (d_y_row == nullptr))
  {
    ctx->last_error = "fcg_effective_tangent: d_m_node is NULL, or only one of d_x_col / d_y_row given";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const hipError_t he =
      fcg::launch_effective_tangent(ctx->mesh, cK, cM, d_m_node, d_K_vals, d_x_col, d_y_row, s);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  return FCG_OK;
}

}  // extern "C"
