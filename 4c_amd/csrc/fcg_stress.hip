// fcg_stress.hip -- the output side of the solid elements: stresses, strains and strain energy at
// the Gauss points, and their nodal form.
//
// Reference: struct_calc_stress (SolidEleCalc::calculate_stress: per Gauss point the kinematics of
// evaluate, So3Material::evaluate, then assemble_strain_type_to_matrix_row /
// assemble_stress_type_to_matrix_row in stress-like Voigt order xx yy zz xy yz xz, shear STRAINS as
// tensor components) and struct_calc_energy (calculate_internal_energy: sum_g w_g det J_g psi(E_g));
// the nodal form is Core::FE::extrapolate_gauss_points_to_nodes followed by the division by the
// nodal element count (GAUSS_POINT_DATA_OUTPUT_TYPE nodes).
//
//  * gp_stress_kernel: one lane per (element, Gauss point) -- a wavefront holds 8 hex8 or 2 hex27
//    elements, four wavefronts per workgroup share the dN table in LDS.  The wavefront stages X and
//    u of its elements in LDS (one node per lane), each lane forms J, H = grad_X u, E, S and psi in
//    registers, and the six components go through an LDS image of the wavefront's [e][g][6] run,
//    which is contiguous in the output: the stores are 16 bytes per lane over consecutive lanes.
//    Elements are walked in column-element order on every path (ele_nodes, node_x, node_dof_col are
//    kept by all of them); on FCG_PATH_GATHER the material table is in storage-slot order, so the
//    kernel reads it through the inverse of ele_orig.
//  * gp_to_nodes_kernel: one wavefront per column node with an owned row walks the mass plan's
//    (element, local node) list in ascending element order (the keys in one load over the lanes,
//    handed round by shuffles), lane i accumulates Xinv[a][g] gp[e][g][c] for its (g, c), the
//    Gauss points are summed in order through LDS.
// No atomics on doubles: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "fcg_internal.hpp"
#include "fcg_shape.hpp"
#include "fcg_status.hpp"

namespace fcg {

namespace {

constexpr int kWaves = 4;  // wavefronts per workgroup

inline int grid_for(int64_t work, int cap) { return int(work < cap ? (work > 0 ? work : 1) : cap); }

struct StressArgs {
  const int32_t* ele_nodes;
  const double* node_x;
  const int32_t* dof_col;
  const double* u;          // [n_cols] or NULL (u = 0, linear kinematics only)
  const double* tab;        // dN[NGP][NPE][3] | w[NGP] on the stiffness rule
  const double* ele_mat;    // [n_ele][4] per-element constants (TAB) or NULL
  const int32_t* mat_slot;  // [n_ele] record of column element e in ele_mat, NULL = e
  double c0, c1, c2;        // StVK: lambda, mu, cdiag; CoupNeoHooke: c, beta
  int64_t n_ele;
  double* stress;           // [n_ele][NGP][6] or NULL
  double* strain;           // [n_ele][NGP][6] or NULL
  double* energy;           // [n_ele] or NULL
  int cauchy, ea;           // the spatial measures instead of PK2 / GL (SPATIAL instantiations)
  int vec2;                 // stress and strain are 16-byte aligned
  int32_t* flag;            // solver flag word: bit 0 det J <= 0, bit 1 det F == 0
  int32_t* bad;             // [2] lowest column element with det J <= 0 / with det F == 0
};

// out = A T A^T for a symmetric T in Voigt order xx yy zz xy yz xz, A row-major
__device__ inline void sym_transform(const double* A, const double* T, double* out)
{
  const double t[9] = {T[0], T[3], T[5], T[3], T[1], T[4], T[5], T[4], T[2]};
  double AT[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      AT[3 * i + j] = A[3 * i] * t[j] + A[3 * i + 1] * t[3 + j] + A[3 * i + 2] * t[6 + j];
  auto dot = [&](int i, int j) {
    return AT[3 * i] * A[3 * j] + AT[3 * i + 1] * A[3 * j + 1] + AT[3 * i + 2] * A[3 * j + 2];
  };
  out[0] = dot(0, 0);
  out[1] = dot(1, 1);
  out[2] = dot(2, 2);
  out[3] = dot(0, 1);
  out[4] = dot(1, 2);
  out[5] = dot(0, 2);
}

__device__ inline double det3(const double* M)
{
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
         M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// inv = M^-1 given det M (row-major)
__device__ inline void inv3(const double* M, double det, double* inv)
{
  const double r = 1.0 / det;
  inv[0] = (M[4] * M[8] - M[5] * M[7]) * r;
  inv[1] = (M[2] * M[7] - M[1] * M[8]) * r;
  inv[2] = (M[1] * M[5] - M[2] * M[4]) * r;
  inv[3] = (M[5] * M[6] - M[3] * M[8]) * r;
  inv[4] = (M[0] * M[8] - M[2] * M[6]) * r;
  inv[5] = (M[2] * M[3] - M[0] * M[5]) * r;
  inv[6] = (M[3] * M[7] - M[4] * M[6]) * r;
  inv[7] = (M[1] * M[6] - M[0] * M[7]) * r;
  inv[8] = (M[0] * M[4] - M[1] * M[3]) * r;
}

// One Gauss point: xu = the element's [b][X0 X1 X2 u0 u1 u2], dn = dN[b][3] at the point.
// S, E: the stress and the strain asked for (tensor components), wpsi = det J psi(E) (the caller
// applies the weight).  Returns 0, or bit 0 for det J <= 0, bit 1 for det F == 0.
template <int NPE, int KIN, int MAT, bool SPATIAL>
__device__ inline int gauss_point(const double* xu, const double* dn, double c0, double c1,
    double c2, bool cauchy, bool ea, bool want_psi, double* S, double* E, double& detj_psi)
{
  // J[k][j] = dX_j / dxi_k and G[i][k] = sum_b u_bi dN_b,k in one pass over the nodes
  double J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // a few nodes in flight hide the LDS latency; unrolled in full the loads of all nodes are
  // hoisted and the kernel takes every register
#pragma unroll NPE == 27 ? 3 : 4
  for (int b = 0; b < NPE; ++b)
  {
    const double d[3] = {dn[3 * b], dn[3 * b + 1], dn[3 * b + 2]};
    const double* p = xu + 6 * b;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        J[3 * k + j] += d[k] * p[j];
        G[3 * j + k] += p[3 + j] * d[k];
      }
  }
  int bad = 0;
  const double det = det3(J);
  if (!(det > 0.0)) bad |= 1;
  double iJ[9];  // iJ[j][k] = dxi_k / dX_j
  inv3(J, det, iJ);
  double H[9];  // H[i][j] = du_i / dX_j
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      H[3 * i + j] = G[3 * i] * iJ[3 * j] + G[3 * i + 1] * iJ[3 * j + 1] + G[3 * i + 2] * iJ[3 * j + 2];
  // Green-Lagrange strain 1/2 (H + H^T + H^T H), linear kinematics: its symmetric gradient part
  auto gl = [&](int i, int j) {
    double e = H[3 * i + j] + H[3 * j + i];
    if (KIN == FCG_TOTLAG) e += H[i] * H[j] + H[3 + i] * H[3 + j] + H[6 + i] * H[6 + j];
    return 0.5 * e;
  };
  const double Et[6] = {gl(0, 0), gl(1, 1), gl(2, 2), gl(0, 1), gl(1, 2), gl(0, 2)};
  double Sp[6], psi = 0.0;
  if (MAT == FCG_MAT_STVK)
  {
    // S = C E, C_00 = cdiag, C_01 = lambda, C_33 = mu on the doubled shears; psi = 1/2 E^T C E
    const double lambda = c0, mu = c1, cdiag = c2;
    Sp[0] = cdiag * Et[0] + lambda * Et[1] + lambda * Et[2];
    Sp[1] = lambda * Et[0] + cdiag * Et[1] + lambda * Et[2];
    Sp[2] = lambda * Et[0] + lambda * Et[1] + cdiag * Et[2];
    Sp[3] = mu * (2.0 * Et[3]);
    Sp[4] = mu * (2.0 * Et[4]);
    Sp[5] = mu * (2.0 * Et[5]);
    psi = 0.5 * (Et[0] * Sp[0] + Et[1] * Sp[1] + Et[2] * Sp[2] +
                 2.0 * (Et[3] * Sp[3] + Et[4] * Sp[4] + Et[5] * Sp[5]));
  }
  else
  {
    // ElastHyper / CoupNeoHooke from the principal invariants of C = 2 E + I
    // (neohooke_stress_cmat of fcg_kernels.hip without the tangent): S = 2 c I + 2 I3 dPI3 C^-1
    const double c = c0, beta = c1;
    const double C0 = 2.0 * Et[0] + 1.0, C1 = 2.0 * Et[1] + 1.0, C2 = 2.0 * Et[2] + 1.0;
    const double c3 = 2.0 * Et[3], c4 = 2.0 * Et[4], c5 = 2.0 * Et[5];
    const double I3 = C0 * C1 * C2 + 2 * c3 * c4 * c5 - C1 * c5 * c5 - C2 * c3 * c3 - C0 * c4 * c4;
    double iC[6];
    iC[0] = (C1 * C2 - c4 * c4) / I3;
    iC[1] = (C0 * C2 - c5 * c5) / I3;
    iC[2] = (C0 * C1 - c3 * c3) / I3;
    iC[3] = (c5 * c4 - c3 * C2) / I3;
    iC[4] = (c3 * c5 - C0 * c4) / I3;
    iC[5] = (c3 * c4 - c5 * C1) / I3;
    double dP2 = NAN;
    const double lg = I3 > 0 ? log(I3) : NAN;
    if (I3 > 0) dP2 = -c * exp(lg * (-beta - 1.));
    const double g0 = 2. * c, g2 = 2. * I3 * dP2;
    Sp[0] = g0 + g2 * iC[0];
    Sp[1] = g0 + g2 * iC[1];
    Sp[2] = g0 + g2 * iC[2];
    Sp[3] = g2 * iC[3];
    Sp[4] = g2 * iC[4];
    Sp[5] = g2 * iC[5];
    if (want_psi)
    {
      // CoupNeoHooke::add_strain_energy: c (I1 - 3) + c / beta (I3^-beta - 1), beta = 0: - c ln I3
      const double I1 = C0 + C1 + C2;
      psi = beta != 0.0 ? c / beta * (exp(lg * (-beta)) - 1.) + c * (I1 - 3.) : c * (I1 - 3. - lg);
    }
  }
  detj_psi = det * psi;
#pragma unroll
  for (int i = 0; i < 6; ++i)
  {
    S[i] = Sp[i];
    E[i] = Et[i];
  }
  if (KIN == FCG_TOTLAG && SPATIAL)
  {
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = H[i] + ((i & 3) == 0 ? 1.0 : 0.0);
    const double detF = det3(F);
    if (detF == 0.0) bad |= 2;
    if (cauchy)
    {
      // sigma = 1 / det F  F S F^T
      double t[6];
      sym_transform(F, Sp, t);
      const double r = 1.0 / detF;
#pragma unroll
      for (int i = 0; i < 6; ++i) S[i] = t[i] * r;
    }
    if (ea)
    {
      // e = F^-T E F^-1
      double iF[9];
      inv3(F, detF, iF);
      const double iFt[9] = {iF[0], iF[3], iF[6], iF[1], iF[4], iF[7], iF[2], iF[5], iF[8]};
      sym_transform(iFt, Et, E);
    }
  }
  return bad;
}

// the wavefront's run of `count` doubles, contiguous in LDS and in the output
__device__ inline void flush_run(const double* src, double* dst, int count, int lane, bool vec2)
{
  if (vec2)
    for (int i = 2 * lane; i < count; i += 128)  // count is even
      *reinterpret_cast<double2*>(dst + i) = *reinterpret_cast<const double2*>(src + i);
  else
    for (int i = lane; i < count; i += 64) dst[i] = src[i];
}

template <int NPE, int KIN, int MAT, bool TAB, bool SPATIAL>
__global__ __launch_bounds__(64 * kWaves) void gp_stress_kernel(StressArgs A)
{
  constexpr int NGP = NPE;
  constexpr int EPW = 64 / NGP;                       // elements per wavefront: 8 / 2
  constexpr int DNS = NPE * 3 + (NPE == 8 ? 1 : 0);   // dN row stride: the points on distinct banks
  constexpr int XUS = NPE * 6 + 1;                    // element stride of X | u: likewise
  constexpr int RUN = EPW * NGP * 6;                  // doubles of a wavefront's output run
  __shared__ double s_dN[NGP * DNS];
  __shared__ double s_xu[kWaves][EPW * XUS];
  __shared__ __align__(16) double s_out[kWaves][RUN];
  __shared__ double s_en[kWaves][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int el = lane / NGP, g = lane - el * NGP;  // hex27: lanes 54 .. 63 idle (el == 2)
  for (int i = threadIdx.x; i < NGP * NPE * 3; i += 64 * kWaves)
  {
    const int gg = i / (NPE * 3);
    s_dN[gg * DNS + (i - gg * NPE * 3)] = A.tab[i];
  }
  const double wg = A.tab[NGP * NPE * 3 + g];
  __syncthreads();
  const int64_t n_grp = (A.n_ele + EPW - 1) / EPW;
  const int64_t n_blk = (n_grp + kWaves - 1) / kWaves;
  double* xu = s_xu[wave];
  double* out = s_out[wave];
  // every wavefront of the workgroup makes the same number of trips (the barriers are uniform)
  for (int64_t bg = blockIdx.x; bg < n_blk; bg += gridDim.x)
  {
    const int64_t e0 = (bg * kWaves + wave) * EPW;
    const int64_t left = A.n_ele - e0;
    const int nval = left <= 0 ? 0 : (left < EPW ? int(left) : EPW);
    if (lane < nval * NPE)
    {
      const int32_t n = A.ele_nodes[e0 * NPE + lane];
      const int le = lane / NPE;
      double* d = xu + le * XUS + (lane - le * NPE) * 6;
      const double* X = A.node_x + 3 * int64_t(n);
      d[0] = X[0];
      d[1] = X[1];
      d[2] = X[2];
      if (A.u)
      {
        const double* u = A.u + A.dof_col[n];
        d[3] = u[0];
        d[4] = u[1];
        d[5] = u[2];
      }
      else
        d[3] = d[4] = d[5] = 0.0;
    }
    __syncthreads();
    const bool act = el < nval;
    double S[6], E[6], wpsi = 0.0;
    if (act)
    {
      const int64_t e = e0 + el;
      double c0 = A.c0, c1 = A.c1, c2 = A.c2;
      if (TAB)
      {
        const double* mp = A.ele_mat + 4 * int64_t(A.mat_slot ? A.mat_slot[e] : e);
        c0 = mp[0];
        c1 = mp[1];
        c2 = mp[2];
      }
      const int bad = gauss_point<NPE, KIN, MAT, SPATIAL>(xu + el * XUS, s_dN + g * DNS, c0, c1, c2,
          A.cauchy != 0, A.ea != 0, A.energy != nullptr, S, E, wpsi);
      wpsi *= wg;
      if (bad)
      {
        atomicOr(A.flag, bad);
        if (bad & 1) atomicMin(A.bad, int32_t(e));
        if (bad & 2) atomicMin(A.bad + 1, int32_t(e));
      }
    }
    if (A.stress)
    {
      if (act)
#pragma unroll
        for (int i = 0; i < 6; ++i) out[6 * lane + i] = S[i];
      __syncthreads();
      flush_run(out, A.stress + e0 * (NGP * 6), nval * NGP * 6, lane, A.vec2 != 0);
      __syncthreads();
    }
    if (A.strain)
    {
      if (act)
#pragma unroll
        for (int i = 0; i < 6; ++i) out[6 * lane + i] = E[i];
      __syncthreads();
      flush_run(out, A.strain + e0 * (NGP * 6), nval * NGP * 6, lane, A.vec2 != 0);
    }
    if (A.energy)
    {
      s_en[wave][lane] = wpsi;
      __syncthreads();
      if (lane < nval)
      {
        double sum = 0.0;
        for (int q = 0; q < NGP; ++q) sum += s_en[wave][lane * NGP + q];  // Gauss-point order
        A.energy[e0 + lane] = sum;
      }
    }
    __syncthreads();  // the next trip overwrites xu, out and s_en
  }
}

template <int NPE, int KIN, int MAT>
void launch_stress_kin(const StressArgs& A, bool tab, bool spatial, dim3 grid, hipStream_t s)
{
  const dim3 block(64 * kWaves);
  constexpr bool SP = KIN == FCG_TOTLAG;  // linear kinematics has no spatial instantiation
  if (tab)
  {
    if (SP && spatial) hipLaunchKernelGGL((gp_stress_kernel<NPE, KIN, MAT, true, SP>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((gp_stress_kernel<NPE, KIN, MAT, true, false>), grid, block, 0, s, A);
  }
  else
  {
    if (SP && spatial) hipLaunchKernelGGL((gp_stress_kernel<NPE, KIN, MAT, false, SP>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((gp_stress_kernel<NPE, KIN, MAT, false, false>), grid, block, 0, s, A);
  }
}

template <int NPE>
void launch_stress_npe(const DeviceMesh& m, const StressArgs& A, bool spatial, dim3 grid, hipStream_t s)
{
  const bool tab = A.ele_mat != nullptr;
  if (m.kinem == FCG_LINEAR)  // StVK only (fcg_create); the spatial measures are the material ones
    launch_stress_kin<NPE, FCG_LINEAR, FCG_MAT_STVK>(A, tab, false, grid, s);
  else if (m.material == FCG_MAT_STVK)
    launch_stress_kin<NPE, FCG_TOTLAG, FCG_MAT_STVK>(A, tab, spatial, grid, s);
  else
    launch_stress_kin<NPE, FCG_TOTLAG, FCG_MAT_ELASTHYPER_COUPNEOHOOKE>(A, tab, spatial, grid, s);
}

__global__ void invert_slots(int64_t n, const int32_t* __restrict__ ele_orig, int32_t* slot_of)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * blockDim.x)
    slot_of[ele_orig[i]] = int32_t(i);
}

// ---------------------------------------------------------------------------- nodal form
// One wavefront per column node n with an owned row.  Lane i owns the entries i, i + 64, ... of an
// element's [g][6] block; over the node's incidences (e, a), ascending by element, it accumulates
// Xinv[a][g] gp[e][g][c]; the Gauss points are then summed in order by six lanes, one per component,
// and divided by the number of elements.
//
// U incidences of the list from position j on (keys in the lanes of `mine`): all their loads are
// issued before the first sum, the sums stay in list order
template <int NPE, int U>
__device__ inline void nodes_accumulate(long long mine, int j, int lane, const double* __restrict__ gp,
    const double* s_xinv, double* acc)
{
  constexpr int BLK = NPE * 6, SL = (BLK + 63) / 64;
  double v[U][SL], x[U][SL];
#pragma unroll
  for (int t = 0; t < U; ++t)
  {
    const long long key = __shfl(mine, j + t);
    const double* ge = gp + (key >> 5) * BLK;
    const double* xa = s_xinv + int(key & 31) * NPE;
#pragma unroll
    for (int q = 0; q < SL; ++q)
    {
      const int i = lane + 64 * q;
      v[t][q] = i < BLK ? ge[i] : 0.0;
      x[t][q] = i < BLK ? xa[i / 6] : 0.0;
    }
  }
#pragma unroll
  for (int t = 0; t < U; ++t)
#pragma unroll
    for (int q = 0; q < SL; ++q) acc[q] += x[t][q] * v[t][q];
}

template <int NPE>
__global__ __launch_bounds__(64 * kWaves) void gp_to_nodes_kernel(int64_t n_node,
    const int32_t* __restrict__ dof_row, const int64_t* __restrict__ ptr,
    const int64_t* __restrict__ inc, const double* __restrict__ xinv, const double* __restrict__ gp,
    double* __restrict__ node)
{
  constexpr int NGP = NPE;
  constexpr int BLK = NGP * 6;            // 48 / 162 doubles of an element
  constexpr int SL = (BLK + 63) / 64;     // entries per lane: 1 / 3
  __shared__ double s_part[kWaves][BLK];
  __shared__ double s_xinv[NPE * NGP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < NPE * NGP; i += 64 * kWaves) s_xinv[i] = xinv[i];
  __syncthreads();
  const int64_t n_blk = (n_node + kWaves - 1) / kWaves;
  for (int64_t bg = blockIdx.x; bg < n_blk; bg += gridDim.x)
  {
    const int64_t n = bg * kWaves + wave;
    const bool act = n < n_node && dof_row[n] >= 0;  // uniform over the wavefront
    int64_t k0 = 0, k1 = 0;
    if (act)
    {
      k0 = ptr[n];
      k1 = ptr[n + 1];
      double acc[SL];
#pragma unroll
      for (int q = 0; q < SL; ++q) acc[q] = 0.0;
      // the list's keys in one load over the lanes, handed round by shuffles: the gp loads of the
      // incidences then depend on nothing but the loop index and overlap
      for (int64_t kb = k0; kb < k1; kb += 64)
      {
        const int nk = k1 - kb < 64 ? int(k1 - kb) : 64;
        const long long mine = lane < nk ? inc[kb + lane] : 0;
        int j = 0;
        for (; j + 4 <= nk; j += 4) nodes_accumulate<NPE, 4>(mine, j, lane, gp, s_xinv, acc);
        for (; j < nk; ++j) nodes_accumulate<NPE, 1>(mine, j, lane, gp, s_xinv, acc);
      }
#pragma unroll
      for (int q = 0; q < SL; ++q)
      {
        const int i = lane + 64 * q;
        if (i < BLK) s_part[wave][i] = acc[q];
      }
    }
    __syncthreads();
    if (act && lane < 6 && k1 > k0)
    {
      double sum = 0.0;
      for (int q = 0; q < NGP; ++q) sum += s_part[wave][6 * q + lane];
      node[6 * n + lane] = sum / double(k1 - k0);
    }
    __syncthreads();
  }
}

// X^-1 of X[g][a] = N_a(xi_g) on the stiffness rule: Gauss-Jordan with partial pivoting (host,
// double).  Row-major [a][g]: nodal_a = sum_g inv[a][g] gp_g.  False for a singular X.
bool extrapolation_matrix(int celltype, std::vector<double>& inv)
{
  const int n = num_nodes(celltype);
  double xi[81], w[27];
  gauss_rule(celltype, xi, w);
  std::vector<double> M(size_t(n) * n);
  for (int g = 0; g < n; ++g) shape_values(celltype, &xi[3 * g], &M[size_t(g) * n]);
  inv.assign(size_t(n) * n, 0.0);
  for (int i = 0; i < n; ++i) inv[size_t(i) * n + i] = 1.0;
  for (int c = 0; c < n; ++c)
  {
    int p = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(M[size_t(r) * n + c]) > std::fabs(M[size_t(p) * n + c])) p = r;
    if (M[size_t(p) * n + c] == 0.0) return false;
    if (p != c)
      for (int j = 0; j < n; ++j)
      {
        std::swap(M[size_t(p) * n + j], M[size_t(c) * n + j]);
        std::swap(inv[size_t(p) * n + j], inv[size_t(c) * n + j]);
      }
    const double d = 1.0 / M[size_t(c) * n + c];
    for (int j = 0; j < n; ++j)
    {
      M[size_t(c) * n + j] *= d;
      inv[size_t(c) * n + j] *= d;
    }
    for (int r = 0; r < n; ++r)
    {
      const double f = M[size_t(r) * n + c];
      if (r == c || f == 0.0) continue;
      for (int j = 0; j < n; ++j)
      {
        M[size_t(r) * n + j] -= f * M[size_t(c) * n + j];
        inv[size_t(r) * n + j] -= f * inv[size_t(c) * n + j];
      }
    }
  }
  return true;
}

}  // namespace

// dN | w on the stiffness rule (gauss_rule: the reference's 13-digit hex27 constants), X^-1 and the
// two failing-element words, once per context
hipError_t stress_tables_build(DeviceMesh& m, int64_t& bytes, hipStream_t s)
{
  if (m.stress_tab) return hipSuccess;
  const int npe = m.npe, ngp = m.npe;
  std::vector<double> t(size_t(ngp) * npe * 3 + ngp), xinv;
  double xi[81], w[27];
  gauss_rule(m.celltype, xi, w);
  for (int g = 0; g < ngp; ++g)
  {
    shape_deriv(m.celltype, &xi[3 * g], &t[size_t(g) * npe * 3]);
    t[size_t(ngp) * npe * 3 + g] = w[g];
  }
  if (!extrapolation_matrix(m.celltype, xinv)) return hipErrorInvalidValue;
  t.insert(t.end(), xinv.begin(), xinv.end());
  double* tab = nullptr;
  int32_t* bad = nullptr;
  const size_t tb = sizeof(double) * t.size();
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&tab), tb);
  if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&bad), 2 * sizeof(int32_t));
  if (he == hipSuccess) he = hipMemcpyAsync(tab, t.data(), tb, hipMemcpyHostToDevice, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);  // t goes out of scope
  if (he != hipSuccess)
  {
    if (tab) (void)hipFree(tab);
    if (bad) (void)hipFree(bad);
    return he;
  }
  m.stress_tab = tab;
  m.stress_xinv = tab + size_t(ngp) * npe * 3 + ngp;
  m.stress_bad = bad;
  bytes += int64_t(tb + 2 * sizeof(int32_t));
  return hipSuccess;
}

// FCG_PATH_GATHER keeps ele_mat in storage-slot order: the record of column element e
hipError_t stress_slots_build(DeviceMesh& m, int64_t& bytes, hipStream_t s)
{
  if (m.stress_slot || m.path != FCG_PATH_GATHER || !m.ele_orig || m.n_ele == 0) return hipSuccess;
  int32_t* slot = nullptr;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&slot), sizeof(int32_t) * size_t(m.n_ele));
  if (he != hipSuccess) return he;
  hipLaunchKernelGGL(invert_slots, dim3(grid_for((m.n_ele + 255) / 256, 4096)), dim3(256), 0, s,
      m.n_ele, m.ele_orig, slot);
  he = hipGetLastError();
  if (he != hipSuccess)
  {
    (void)hipFree(slot);
    return he;
  }
  m.stress_slot = slot;
  bytes += int64_t(sizeof(int32_t)) * m.n_ele;
  return hipSuccess;
}

hipError_t launch_gp_stress(const DeviceMesh& m, bool cauchy, bool ea, const double* d_u_col,
    double* d_stress, double* d_strain, double* d_energy, hipStream_t s)
{
  StressArgs A;
  A.ele_nodes = m.ele_nodes;
  A.node_x = m.node_x;
  A.dof_col = m.node_dof_col;
  A.u = d_u_col;
  A.tab = m.stress_tab;
  A.ele_mat = m.ele_mat;
  A.mat_slot = m.path == FCG_PATH_GATHER ? m.stress_slot : nullptr;
  if (m.material == FCG_MAT_STVK)
  {
    A.c0 = m.lambda;
    A.c1 = m.mu;
    A.c2 = m.cdiag;
  }
  else
  {
    A.c0 = m.nh_c;
    A.c1 = m.nh_beta;
    A.c2 = 0.0;
  }
  A.n_ele = m.n_ele;
  A.stress = d_stress;
  A.strain = d_strain;
  A.energy = d_energy;
  const bool totlag = m.kinem == FCG_TOTLAG;
  A.cauchy = totlag && cauchy && d_stress;
  A.ea = totlag && ea && d_strain;
  A.vec2 = ((reinterpret_cast<uintptr_t>(d_stress) | reinterpret_cast<uintptr_t>(d_strain)) & 15) == 0;
  A.flag = m.err + 2;
  A.bad = m.stress_bad;
  const int epw = 64 / m.npe;
  const int64_t n_blk = ((m.n_ele + epw - 1) / epw + kWaves - 1) / kWaves;
  const dim3 grid(grid_for(n_blk, 256 * 8));
  const bool spatial = A.cauchy || A.ea;
  if (m.npe == 27) launch_stress_npe<27>(m, A, spatial, grid, s);
  else launch_stress_npe<8>(m, A, spatial, grid, s);
  return hipGetLastError();
}

hipError_t launch_gp_to_nodes(const DeviceMesh& m, const double* d_gp, double* d_node, hipStream_t s)
{
  const dim3 grid(grid_for((m.n_node + kWaves - 1) / kWaves, 256 * 16)), block(64 * kWaves);
  if (m.npe == 27)
    hipLaunchKernelGGL((gp_to_nodes_kernel<27>), grid, block, 0, s, m.n_node, m.node_dof_row,
        m.mass_ptr, m.mass_inc, m.stress_xinv, d_gp, d_node);
  else
    hipLaunchKernelGGL((gp_to_nodes_kernel<8>), grid, block, 0, s, m.n_node, m.node_dof_row,
        m.mass_ptr, m.mass_inc, m.stress_xinv, d_gp, d_node);
  return hipGetLastError();
}

}  // namespace fcg

extern "C" {

int fcg_gp_stress(fcg_ctx* ctx, int stress_type, int strain_type, const double* d_u_col,
    double* d_stress, double* d_strain, double* d_energy, void* stream, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::DeviceMesh& m = ctx->mesh;
  auto refuse = [&](const char* why) {
    ctx->last_error = std::string("fcg_gp_stress: ") + why;
    return FCG_ERR_ARG;
  };
  if (stress_type != FCG_STRESS_NONE && stress_type != FCG_STRESS_PK2 && stress_type != FCG_STRESS_CAUCHY)
    return refuse("stress_type must be FCG_STRESS_NONE, FCG_STRESS_PK2 or FCG_STRESS_CAUCHY");
  if (strain_type != FCG_STRAIN_NONE && strain_type != FCG_STRAIN_GL && strain_type != FCG_STRAIN_EA)
    return refuse("strain_type must be FCG_STRAIN_NONE, FCG_STRAIN_GL or FCG_STRAIN_EA");
  if (!d_stress && !d_strain && !d_energy) return refuse("d_stress, d_strain and d_energy are all NULL");
  if (d_stress && stress_type == FCG_STRESS_NONE)
    return refuse("d_stress given with stress_type FCG_STRESS_NONE");
  if (!d_stress && stress_type != FCG_STRESS_NONE) return refuse("stress_type given without d_stress");
  if (d_strain && strain_type == FCG_STRAIN_NONE)
    return refuse("d_strain given with strain_type FCG_STRAIN_NONE");
  if (!d_strain && strain_type != FCG_STRAIN_NONE) return refuse("strain_type given without d_strain");
  if (!d_u_col && m.kinem != FCG_LINEAR)
    return refuse("d_u_col is NULL (allowed for FCG_LINEAR only, meaning u = 0)");
  if (m.n_ele == 0) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  hipError_t he = fcg::stress_tables_build(m, ctx->device_bytes, s);
  if (he == hipSuccess && m.ele_mat) he = fcg::stress_slots_build(m, ctx->device_bytes, s);
  int32_t flags = 0, bad[2] = {0, 0}, gid = -1;
  int32_t* flag = m.err + 2;  // the solver flag word: evaluate's sticky flags are left alone
  if (he == hipSuccess) he = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
  if (he == hipSuccess) he = hipMemsetAsync(m.stress_bad, 0x7f, 2 * sizeof(int32_t), s);
  if (he == hipSuccess)
    he = fcg::launch_gp_stress(m, stress_type == FCG_STRESS_CAUCHY, strain_type == FCG_STRAIN_EA,
        d_u_col, d_stress, d_strain, d_energy, s);
  if (he == hipSuccess) he = hipMemcpyAsync(&flags, flag, sizeof(flags), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipMemcpyAsync(bad, m.stress_bad, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  // the lowest failing column element decides the code (det J first when both fail there)
  int code = FCG_OK;
  int32_t e = -1;
  if (he == hipSuccess && flags)
  {
    const bool dj = (flags & 1) != 0, df = (flags & 2) != 0;
    if (dj && (!df || bad[0] <= bad[1]))
    {
      code = FCG_ERR_NODAL_DETJ;
      e = bad[0];
    }
    else
    {
      code = FCG_ERR_SINGULAR;
      e = bad[1];
    }
    if (e >= 0 && e < m.n_ele)
      he = hipMemcpy(&gid, m.ele_gid + e, sizeof(gid), hipMemcpyDeviceToHost);
  }
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("fcg_gp_stress: HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (code != FCG_OK)
  {
    if (bad_ele_gid) *bad_ele_gid = gid;
    ctx->last_error = std::string("fcg_gp_stress: ") +
                      (code == FCG_ERR_NODAL_DETJ ? "det J <= 0" : "det F == 0") +
                      " at a Gauss point of element GID " + std::to_string(gid);
  }
  return code;
}

int fcg_gp_to_nodes(fcg_ctx* ctx, const double* d_gp, double* d_node, void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::DeviceMesh& m = ctx->mesh;
  if (m.n_rows == 0 || m.n_ele == 0) return FCG_OK;
  if (!d_gp || !d_node)
  {
    ctx->last_error = "fcg_gp_to_nodes: d_gp or d_node is NULL";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  hipError_t he = fcg::stress_tables_build(m, ctx->device_bytes, s);
  if (he == hipSuccess) he = fcg::mass_plan_build(m, ctx->device_bytes, s);
  if (he == hipSuccess) he = fcg::launch_gp_to_nodes(m, d_gp, d_node, s);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("fcg_gp_to_nodes: HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  return FCG_OK;
}

}  // extern "C"
