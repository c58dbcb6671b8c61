// fcg_sweep.hip -- fused hex8 element evaluation + global assembly on structured (GridGenerator)
// lattices: the row-block sweep.
//
// A workgroup owns a 4 x 4 column of row nodes over a z-segment of node planes and sweeps the
// element layers bottom to top.  Per layer L (the elements between node planes L and L+1):
//   A. one lane per (element, Gauss point) of the 5 x 5 elements touching the tile's node
//      columns: J, J^-1, det J (and det J > 0 at node g), N_XYZ, strain or F, StVK stress
//      (4C_solid_3D_ele_calc_lib.hpp:380-496, 579-676, 682-799; 4C_mat_stvenantkirchhoff.cpp:169-177).
//      Into LDS go sqrt|fac| N_XYZ of the 8 nodes and the stress (with F for TotLag);
//   B. sixteen lanes per node column, four element visits each (fcg_visit_table.h): a lane sums
//      over the elements holding both nodes of its blocks (A, B) and all Gauss points
//        linear: G = sum fac a b^T,                 K_AB = lambda G + mu G^T + mu tr(G) I
//        TotLag: G = sum fac (Fa)(Fb)^T, H = sum fac (a.b) F F^T, geo = sum fac a.S.b,
//                K_AB = lambda G + mu G^T + mu H + geo I
//      (= B_a^T C B_b + K_geo of calc_lib.hpp:872-927 for the isotropic C of fill_cmat) and
//      writes the 3 x 3 block straight into its 3 CSR rows -- or keeps the lower-layer part of
//      an in-plane block (dz = 0) in LDS until the next layer adds the upper part.
//      The residual rows f_A = sum fac F S N_XYZ_A (calc_lib.hpp:851-860) are summed the same way,
//      16 lanes per column.
// Every entry of an owned row is written exactly once, by one lane, in a fixed summation order:
// no atomics, no row image in LDS, bitwise reproducible.
// The linear tangent (K + r, the headline; MODE 3 below) writes a row within one layer.  The 9
// blocks of plane P's row with the plane below (dz = -1) are finished in layer P-1, the other 18
// in layer P; on a lattice-numbered mesh they are the row's first 216 of 648 bytes, and written as
// they finish they leave two cache lines per row half-filled in L2 for a layer, which then go to
// memory twice (1.18 x the K bytes written at 1M elements).  So a dz = -1 block waits one layer
// in LDS (hold_lo), its lane swapping it for the next one, and leaves beside the row's other
// blocks: 1.03 x.  On regular lattice tiles (REGK below) all of it is addressed in closed form.
// Layers without elements -- below the element box, on the top node plane -- are left out.
// TotLag, the TSI passes and the internal-force kernels write blocks as they finish (MODE 0).
// Owned-rows-only assembly and column
// positions follow SparseMatrix::assemble (4C_linalg_sparsematrix.cpp:474-543, positions resolved
// per node row by fcg_create), the residual LinAlg::assemble (4C_linalg_utils_sparse_algebra_assemble.cpp:72-92).
//
// Linear kinematics: f_int = K u exactly (E = B u, f = sum fac B^T C B u), so the residual rows are
// summed from the finished blocks, f_A += K_AB u_B, and stage A needs neither strains nor stresses.
//
// Latency hiding: two workgroups per CU for linear kinematics (LDS 59 KB, 70 KB with hold_lo), one for TotLag
// (85 KB), plus, inside a workgroup, register prefetch of the next node plane (coordinates,
// displacements) and plane record while the current layer computes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fcg_hex8_element.hpp"
#include "fcg_internal.hpp"
#include "fcg_visit_table.h"

namespace fcg {

namespace {

constexpr int TX = 4, TY = 4;              // node columns per tile
constexpr int EXN = TX + 1, EYN = TY + 1;  // element columns per layer
constexpr int NSLOT = EXN * EYN;           // 25 elements per layer
constexpr int NXN = TX + 2;                // node columns per row of the node grid (6 x 6)
constexpr int NNODE = NXN * (TY + 2);
// plane record (uint32 words): row0[16] | rowlen[16] | rbase[16] (int64) | npos[16][27] (uint16)
constexpr int PR_ROW0 = 0, PR_LEN = 16, PR_BASE = 32, PR_NPOS = 64;
// LDS image of sqrt|fac| N_XYZ: [dim][Gauss-point pair p][slot][node ^ swizzle][2], the two
// Gauss points 2p, 2p+1 of a node side by side so that one ds_read_b128 fetches both.  The node
// swizzle (p + 4 (slot & 1)) spreads the stage-A stores of an element's 8 lanes (and of the
// 2 elements of a 16-lane store group) over distinct banks.
__device__ constexpr int nx_sw(int p, int slot) { return (p + 4 * (slot & 1)) & 7; }
__device__ constexpr int nx2i(int d, int p, int slot, int n)
{
  return (((d * 4 + p) * NSLOT + slot) * 8 + (n ^ nx_sw(p, slot))) * 2;
}

// hex8 node offsets in 4C node order (4C_io_gridgenerator.cpp:371-379)
__device__ constexpr int node_ox(int n) { return ((n & 3) == 1 || (n & 3) == 2) ? 1 : 0; }
__device__ constexpr int node_oy(int n) { return (n & 3) >= 2 ? 1 : 0; }
__device__ constexpr int node_oz(int n) { return n >> 2; }

struct SweepArgs {
  const double* u_col;
  const double* lat_x;       // [LZ][LY][LX][3] node coordinates on the column-node lattice
  const int32_t* lat_dof;    // [LZ][LY][LX] column LID of the first DOF, -1 = no node
  const int32_t* elem_at;    // [EZ][EY][EX] column element or -1
  const uint32_t* plane_rec; // [tiles_y][tiles_x][NK][PLANE_REC_WORDS]
  // regular lattice tiles (REGK kernels): compact records, plane run per tile, position pattern
  const uint32_t* reg_rec;   // [tiles_y][tiles_x][NK][REG_REC_WORDS]
  const int32_t* reg_tile;   // [tiles_y][tiles_x][2]
  const int32_t* reg_pos;    // [32], 27 used
  const double* tables;
  double* K;
  double* fint;
  int32_t* err;
  unsigned long long* stamps;  // diagnostic phase timers (NULL = off, the production setting)
  StVK mat;
  // fused TSI blocks (TSI instantiation only): v, T by column LID (thermo LID = structural / 3),
  // shape values at the Gauss points [8][8], the k_ST / k_TS / k_TT values and f_T by row LID
  const double* v_col;
  const double* T_col;
  const double* Ngp;
  double* Kst;
  double* Kts;
  double* Ktt;
  double* fT;
  double tsi_m, tsi_T0, tsi_k, tsi_kts;  // m, T_0, Fourier k, -timefac timefac_d
  int32_t tiles_x, tiles_y, seg_planes;
  int32_t I0, J0, K0, NI, NJ, NK;
  int32_t EX0, EY0, EZ0, EX, EY, EZ;  // element box; the node lattice box is EX+1 x EY+1 x EZ+1
  int32_t skip_empty;  // linear structural passes: leave out the layers without elements
};

// node data per lattice column: X | u, and for TSI v | T
template <bool TSI>
constexpr int node_comps() { return TSI ? 10 : 6; }

// Record strides (doubles) of the per-(Gauss point, slot) arrays gp and tg below.  Stage A's lane
// (slot s, Gauss point g) stores record 25 g + s; with 16 doubles (32 dwords) every record began on
// bank 0 (mod 32), so a 16-lane ds_write_b64 group was a 16-way conflict and the visit loads at one
// Gauss point saw two distinct banks.  18 (36 dwords) starts record r on bank 4 (g + s) mod 32
// for the stores and 36 s mod 64 for the loads, 16-byte aligned for ds_*_b128 (1M hex8 TotLag
// 2.76 -> 2.40 ms, profiles/r05/r05_gp_stride_ab.txt).  tg (TSI) at 6 instead of 4 measured the
// same (4.31-4.40 vs 4.31-4.35 ms fused), so it stays at 4.
#ifndef FCG_GP_STRIDE
#define FCG_GP_STRIDE 18
#endif
#ifndef FCG_TG_STRIDE
#define FCG_TG_STRIDE 4
#endif

template <int KIN, bool TSI, bool TH = false, bool DEFER = false>
struct SweepShared {
  alignas(16) double nx[3 * 4 * NSLOT * 8 * 2];  // sqrt|fac| N_XYZ, see nx2i()
  // TotLag: F (column-major) | S (Voigt) | c = fac / sqrt|fac| | pad  (linear kinematics: unused)
  alignas(16) double gp[KIN ? 8 : 1][KIN ? NSLOT : 1][KIN ? FCG_GP_STRIDE : 16];
  // TSI: c = fac / sqrt|fac| | T_g | m c sqrt|fac| tr(B_L v)_g = m fac tr(e')_g | pad
  alignas(16) double tg[TSI ? 8 : 1][TSI ? NSLOT : 1][TSI ? FCG_TG_STRIDE : 4];
  double node[3][NNODE][node_comps<TSI>()];  // node columns of the 6 x 6 grid, ring by plane mod 3
  uint32_t prec[3][PLANE_REC_WORDS];  // plane records, ring by plane mod 3
  double gxi[8][4];  // Gauss point coordinates (stage A forms the shape derivatives from them)
  double Ng[TSI ? 8 : 1][8];  // TSI: shape values N_n at Gauss point g
  // the same, node-major rows of 10 (16-byte aligned): the thermal pass's visit reads a node's
  // values at Gauss points (2p, 2p + 1) as one ds_read_b128
  alignas(16) double NgT[TSI ? 8 : 1][10];
  double w8[8];
  uint32_t neg[NSLOT];  // bit g set: fac < 0 at Gauss point g
  // lower-layer parts of the in-plane blocks (dz = 0) of node plane L+1: written by the D-side
  // lane k + 8, read by the U-side lane k of the next layer in the same instruction that precedes
  // the next write (LDS operations of a wavefront complete in order): one buffer suffices.
  // [column][in-plane neighbour (dy+1)*3 + dx+1][3x3 | TSI: k_ST 3 | k_TS 3 | k_TT 1]
  // (TSI rows padded to 18 doubles: with 16 every (column, t) record started on the same bank;
  // thermal-only pass TH: k_ST 3 | k_TS 3 | k_TT 1, padded to 9)
#ifdef FCG_PROBE_WG3
  double hold[1][9][TSI ? (TH ? 9 : 18) : 9];  // timing probe only: one column's buffer for all
#else
  // structural rows 10 apart (16-byte aligned: the 9 held entries as 4 ds_read_b128 + 1
  // ds_read_b64 and 4 ds_write_b128 + 1 ds_write_b64 instead of ds_read2_b64 / ds_write2_b64
  // pairs): headline -0.1 to -0.6 %, TotLag -0.9 % (profiles/r06/r06_sweep_hold10_ab.txt);
  // FCG_HOLD9 = the round-5 rows (A/B)
#if defined(FCG_HOLD9)
  static constexpr int kHs = 9;
#else
  static constexpr int kHs = 10;
#endif
  // (the thermal pass's 7 held values keep rows of 9: aligned rows of 10 measured +0.3 % on the
  // two-field tangent, r06_sweep_hold10_ab.txt)
  // Structural passes: one more column, never written after the prologue has zeroed it.  A lane
  // whose block adds no held part reads its nine zeros, so that every lane of the wave adds what
  // it read without a branch (see emit).
  alignas(16) double hold[TX * TY + (TSI ? 0 : 1)][9][TSI ? (TH ? 9 : 18) : kHs];
#endif
  // DEFER (the linear tangent kernels): the blocks of node plane L+1's rows with the plane below
  // (dz = -1, finished in layer L) wait here and are written in layer L+1 beside the row's other
  // blocks, so that each row's cache lines are filled within one layer.  Slot (column, t) belongs
  // to the one lane that emits block t of that column every layer: it reads the held block
  // before it holds the next one (a wavefront's LDS operations execute in order), one buffer.
#ifdef FCG_HOLDLO9
  double hold_lo[DEFER ? TX * TY : 1][9][9];  // A/B probe: the round-5 rows
#else
  // rows 10 apart, 16-byte aligned as hold: renumbered 1M box through AUTO 1.149 -> 1.085 ms
  alignas(16) double hold_lo[DEFER ? TX * TY : 1][9][10];
#endif
};

__device__ inline int ring(int p) { return (p % 3 + 3) % 3; }

// Cross-lane moves of a double by DPP (all lanes of the row active)
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // lane i <-> 7-i within 8
constexpr int kDppRowRor8 = 0x128;     // lane i <- lane i+8 (mod 16) within a row of 16
template <int CTRL>
__device__ inline double dpp_f64(double v)
{
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// 4C hex8 node index of the node at (ox, oy, oz) of an element (4C_io_gridgenerator.cpp:371-379)
__device__ inline int node_at(int ox, int oy, int oz) { return 4 * oz + (oy ? (ox ? 2 : 3) : (ox ? 1 : 0)); }

// Stage A for element slot s, Gauss point g of layer L (element e, -1 = none).  Written for a
// small register footprint: node data stays in LDS and N_XYZ is recomputed where needed.
// The checks that depend on the reference coordinates alone -- det J at node g, det J == 0 at
// Gauss point g, the sign of fac -- run when CHECKED is set.  GEOM is the create-time geometry
// pass (sweep_geometry_pass): this same arithmetic up to fac and nothing behind it, the codes
// into A.err[0..1] as in an evaluate and "some fac < 0" into A.err[2].  A context whose pass found
// nothing runs CHECKED = false from then on: lat_x does not change during a context's life.
// A check that reads u (TotLag: F singular) stays in every instantiation.
template <int KIN, bool TSI, bool CHECKED, bool GEOM, class SH>
__device__ inline void sweep_stage_a(SH& sh, const SweepArgs& A, int s, int g,
    int sx, int sy, int L, int e)
{
  constexpr int NC = node_comps<TSI>();
  const bool valid = e >= 0;
  const double* nd[8];
#pragma unroll
  for (int n = 0; n < 8; ++n)
    nd[n] = sh.node[ring(L + node_oz(n))][(sy + node_oy(n)) * NXN + sx + node_ox(n)];
  // CHECKED: the nodal determinant's reads of the same coordinates, further down, bring all of
  // them in at once.  Without that block the compiler reads the nodes two by two and waits for
  // each pair (four exposed LDS round trips per layer): read all eight first, with the Gauss
  // point's coordinates and weight, in one round trip.
  double X[8][3];
#pragma unroll
  for (int n = 0; n < 8; ++n)
#pragma unroll
    for (int d = 0; d < 3; ++d) X[n][d] = nd[n][d];
  const double gx0 = sh.gxi[g][0], gx1 = sh.gxi[g][1], gx2 = sh.gxi[g][2], wg = sh.w8[g];
  if constexpr (!CHECKED) __builtin_amdgcn_sched_barrier(0);
  // shape derivatives at Gauss point g from its coordinates (no table loads)
  const H8dN dn = h8_dn_products(gx0, gx1, gx2);
  double J[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) J[q] = 0.0;
#pragma unroll
  for (int n = 0; n < 8; ++n)
  {
    const double x0 = X[n][0], x1 = X[n][1], x2 = X[n][2];
    double d0, d1, d2;
    h8_dn(dn, n, d0, d1, d2);
    J[0] += d0 * x0; J[1] += d1 * x0; J[2] += d2 * x0;
    J[3] += d0 * x1; J[4] += d1 * x1; J[5] += d2 * x1;
    J[6] += d0 * x2; J[7] += d1 * x2; J[8] += d2 * x2;
  }
  int bad = 0;
  // det J at node g (calc_lib.hpp:475-496): at a hex8 corner the shape derivatives are
  // +-1/2 on the node and its neighbour along each parametric direction, so J's columns are
  // half the three edge vectors through the node and det J = det(edges) / 8 (same sign).
  if constexpr (CHECKED)
  {
    const int ox = node_ox(g), oy = node_oy(g), oz = node_oz(g);
    const double* zl = sh.node[ring(L)][0];
    const double* zh = sh.node[ring(L + 1)][0];
    const double* pz = oz ? zh : zl;
    const int cxy = (sy + oy) * NXN + sx + ox;
    const double* o = pz + NC * cxy;
    const double* ex_ = pz + NC * (cxy + (ox ? -1 : 1));
    const double* ey_ = pz + NC * (cxy + (oy ? -NXN : NXN));
    const double* ez_ = (oz ? zl : zh) + NC * cxy;
    // edge vectors oriented along +xi, +eta, +zeta
    const double sgx = ox ? 1.0 : -1.0, sgy = oy ? 1.0 : -1.0, sgz = oz ? 1.0 : -1.0;
    const double a0 = sgx * (o[0] - ex_[0]), a1 = sgx * (o[1] - ex_[1]), a2 = sgx * (o[2] - ex_[2]);
    const double b0 = sgy * (o[0] - ey_[0]), b1 = sgy * (o[1] - ey_[1]), b2 = sgy * (o[2] - ey_[2]);
    const double c0 = sgz * (o[0] - ez_[0]), c1 = sgz * (o[1] - ez_[1]), c2 = sgz * (o[2] - ez_[2]);
    const double detn = a0 * (b1 * c2 - b2 * c1) + b0 * (c1 * a2 - c2 * a1) + c0 * (a1 * b2 - a2 * b1);
    if (detn == 0.0) bad = 2;
    else if (!(detn > 0)) bad = 1;
  }
  const double det = h8_invert3x3(J);
  if (CHECKED && det == 0.0) bad = 2;
  // the thermo element's check (4C_thermo_ele_impl.cpp:2663-2664)
  else if (TSI && det < 1e-16 && bad == 0) bad = 1;
  const double fac = det * wg;
  if constexpr (GEOM)
  {
    if (valid && bad)
    {
      atomicMax(&A.err[0], bad);
      atomicMin(&A.err[1], e);
    }
    if (valid && fac < 0.0) atomicMax(&A.err[2], 1);
    return;
  }
  // missing element (outside the column set): all its LDS data become exact zeros
  const double sq = valid ? sqrt(fabs(fac)) : 0.0;
  const double cf = fac < 0.0 ? -sq : sq;  // fac / sqrt|fac|
  if (KIN == 0)
  {
    // linear: scale J^-1 once; N_XYZ below is then sqrt|fac| N_XYZ, the strain sqrt|fac| E
#pragma unroll
    for (int q = 0; q < 9; ++q) J[q] *= sq;
  }
  const double ns = KIN == 0 ? 1.0 : sq;  // remaining scale of the stored N_XYZ
  // N_XYZ of node n (J now holds J^-1, column-major)
  auto nxyz = [&](int n, double& n0, double& n1, double& n2) {
    double d0, d1, d2;
    h8_dn(dn, n, d0, d1, d2);
    n0 = J[0] * d0 + J[3] * d1 + J[6] * d2;
    n1 = J[1] * d0 + J[4] * d1 + J[7] * d2;
    n2 = J[2] * d0 + J[5] * d1 + J[8] * d2;
  };
  double E[6] = {0, 0, 0, 0, 0, 0};
  double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double Tg = 0.0, trv = 0.0;  // TSI: T_g = N.T, sqrt|fac| tr(B_L v)
#pragma unroll
  for (int n = 0; n < 8; ++n)
  {
    double n0, n1, n2;
    nxyz(n, n0, n1, n2);
    if (TSI)
    {
      trv += n0 * nd[n][6] + n1 * nd[n][7] + n2 * nd[n][8];
      Tg += sh.Ng[TSI ? g : 0][n] * nd[n][9];
    }
    sh.nx[nx2i(0, g >> 1, s, n) + (g & 1)] = KIN == 0 ? n0 : ns * n0;
    sh.nx[nx2i(1, g >> 1, s, n) + (g & 1)] = KIN == 0 ? n1 : ns * n1;
    sh.nx[nx2i(2, g >> 1, s, n) + (g & 1)] = KIN == 0 ? n2 : ns * n2;
    if (KIN == 1)
    {
      // hex8: F = x N_XYZ^T from current coordinates (calc_lib.hpp:585-595)
      const double u0 = nd[n][3], u1 = nd[n][4], u2 = nd[n][5];
      const double q0 = nd[n][0] + u0, q1 = nd[n][1] + u1, q2 = nd[n][2] + u2;
      F[0] += q0 * n0; F[1] += q1 * n0; F[2] += q2 * n0;
      F[3] += q0 * n1; F[4] += q1 * n1; F[5] += q2 * n1;
      F[6] += q0 * n2; F[7] += q1 * n2; F[8] += q2 * n2;
    }
  }
  if (KIN == 1)
  {
    double Fi[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Fi[q] = F[q];
    if (h8_invert3x3(Fi) == 0.0) bad = 2;
    double C[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        C[r + 3 * q] = F[3 * r] * F[3 * q] + F[3 * r + 1] * F[3 * q + 1] + F[3 * r + 2] * F[3 * q + 2];
    E[0] = 0.5 * (C[0] - 1.0);
    E[1] = 0.5 * (C[4] - 1.0);
    E[2] = 0.5 * (C[8] - 1.0);
    E[3] = C[3];
    E[4] = C[7];
    E[5] = C[2];
  }
  if (KIN == 1)
  {
    const StVK& m = A.mat;
    double S[6];
    S[0] = m.cdiag * E[0] + m.lambda * E[1] + m.lambda * E[2];
    S[1] = m.lambda * E[0] + m.cdiag * E[1] + m.lambda * E[2];
    S[2] = m.lambda * E[0] + m.lambda * E[1] + m.cdiag * E[2];
    S[3] = m.mu * E[3];
    S[4] = m.mu * E[4];
    S[5] = m.mu * E[5];
    double* P = sh.gp[KIN ? g : 0][KIN ? s : 0];
#pragma unroll
    for (int q = 0; q < 9; ++q) P[q] = F[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) P[9 + q] = S[q];
    P[15] = cf;
  }
  if (TSI)
  {
    double* t = sh.tg[TSI ? g : 0][TSI ? s : 0];
    t[0] = cf;
    t[1] = Tg;
    t[2] = A.tsi_m * cf * trv;
  }
  if constexpr (CHECKED || KIN == 1)
  {
    if (valid && bad)
    {
      atomicMax(&A.err[0], bad);
      atomicMin(&A.err[1], e);
    }
  }
  if constexpr (CHECKED)
  {
    const unsigned long long neg = __ballot(valid && fac < 0.0);
    if (g == 0) sh.neg[s] = uint32_t((neg >> (threadIdx.x & 56)) & 0xFFull);
  }
}

// One element visit: accumulate the blocks (a, b1) into acc1 and (a, b2) into acc2 over the
// Gauss points of element slot `slot`.  Acc layout: G[9] (row-major, G[3r+q] = sum a'_r b'_q)
// then, for TotLag, H[6] and geo; for TSI (linear) sum c N_b a[3], sum c N_a T_g b[3] and
// sum m fac tr(e') N_a N_b (the factors m, -timefac timefac_d and k enter in tsi_block).
// TH (the thermal-only pass beside the linear structural sweep): no G, the thermal sums at
// acc[0..5], fac a.b at acc[6] (k_TT's conduction part) and sum m fac tr(e') N_a N_b at acc[7].
template <int KIN, bool NEG, bool TSI, bool TH = false, class SH>
__device__ inline void sweep_visit(const SH& sh, int slot, int a, int b1, int b2,
    uint32_t nm, double* acc1, double* acc2)
{
#ifndef FCG_TH_PAIRS
#define FCG_TH_PAIRS 1
#endif
  // thermal pass: the shape values of nodes a, b1, b2 at all 8 Gauss points as 12 explicit
  // 16-byte reads (the compiler paired the per-point 8-byte reads across points into
  // ds_read2_b64, 8 LDS cycles per 16 bytes against 4)
  double2 nA[TH && FCG_TH_PAIRS ? 4 : 1], n1[TH && FCG_TH_PAIRS ? 4 : 1], n2[TH && FCG_TH_PAIRS ? 4 : 1];
  if constexpr (TH && FCG_TH_PAIRS)
  {
#pragma unroll
    for (int p = 0; p < 4; ++p)
    {
      nA[p] = *reinterpret_cast<const double2*>(&sh.NgT[a][2 * p]);
      n1[p] = *reinterpret_cast<const double2*>(&sh.NgT[b1][2 * p]);
      n2[p] = *reinterpret_cast<const double2*>(&sh.NgT[b2][2 * p]);
    }
  }
  auto gp_body = [&](int g, double a0, double a1, double a2, double p0, double p1, double p2,
                     double q0, double q1, double q2) {
    if (TH)
    {
      const double* t = sh.tg[g][slot];
#if FCG_TH_PAIRS
      const double2 t01 = *reinterpret_cast<const double2*>(t), t23 = *reinterpret_cast<const double2*>(t + 2);
      const double cf = t01.x, Tg = t01.y, qq = t23.x;
      const double Na = (g & 1) ? nA[g >> 1].y : nA[g >> 1].x, N1 = (g & 1) ? n1[g >> 1].y : n1[g >> 1].x,
                   N2 = (g & 1) ? n2[g >> 1].y : n2[g >> 1].x;
#else
      const double cf = t[0], Tg = t[1], qq = t[2];
      const double Na = sh.Ng[g][a], N1 = sh.Ng[g][b1], N2 = sh.Ng[g][b2];
#endif
      const double c1 = cf * N1, c2 = cf * N2, ct = cf * Na * Tg, qa = qq * Na;
      acc1[0] += c1 * a0; acc1[1] += c1 * a1; acc1[2] += c1 * a2;
      acc2[0] += c2 * a0; acc2[1] += c2 * a1; acc2[2] += c2 * a2;
      acc1[3] += ct * p0; acc1[4] += ct * p1; acc1[5] += ct * p2;
      acc2[3] += ct * q0; acc2[4] += ct * q1; acc2[5] += ct * q2;
      acc1[7] += qa * N1;
      acc2[7] += qa * N2;
      // fac a.b: sqrt|fac| a . sqrt|fac| b with the sign of fac
      const double sg = (NEG && ((nm >> g) & 1u)) ? -1.0 : 1.0;
      acc1[6] += sg * (a0 * p0 + a1 * p1 + a2 * p2);
      acc2[6] += sg * (a0 * q0 + a1 * q1 + a2 * q2);
      return;
    }
    if (TSI)
    {
      // unflipped sqrt|fac| N_XYZ times c = fac / sqrt|fac| gives fac N_XYZ
      const double* t = sh.tg[TSI ? g : 0][TSI ? slot : 0];
      const double cf = t[0], Tg = t[1], qq = t[2];
      const double Na = sh.Ng[TSI ? g : 0][a], N1 = sh.Ng[TSI ? g : 0][b1],
                   N2 = sh.Ng[TSI ? g : 0][b2];
      const double c1 = cf * N1, c2 = cf * N2, ct = cf * Na * Tg, qa = qq * Na;
      acc1[9] += c1 * a0; acc1[10] += c1 * a1; acc1[11] += c1 * a2;
      acc2[9] += c2 * a0; acc2[10] += c2 * a1; acc2[11] += c2 * a2;
      acc1[12] += ct * p0; acc1[13] += ct * p1; acc1[14] += ct * p2;
      acc2[12] += ct * q0; acc2[13] += ct * q1; acc2[14] += ct * q2;
      acc1[15] += qa * N1;
      acc2[15] += qa * N2;
    }
    if (NEG && ((nm >> g) & 1u))
    {
      a0 = -a0;
      a1 = -a1;
      a2 = -a2;
    }
    if (KIN == 0)
    {
#ifdef FCG_PROBE_NOG
      // timing probe only (wrong results): the loads kept, 4 of the 18 FMAs
      const double sa = a0 + a1 + a2;
      acc1[0] += sa * (p0 + p1 + p2);
      acc2[0] += sa * (q0 + q1 + q2);
      return;
#endif
      acc1[0] += a0 * p0; acc1[1] += a0 * p1; acc1[2] += a0 * p2;
      acc1[3] += a1 * p0; acc1[4] += a1 * p1; acc1[5] += a1 * p2;
      acc1[6] += a2 * p0; acc1[7] += a2 * p1; acc1[8] += a2 * p2;
      acc2[0] += a0 * q0; acc2[1] += a0 * q1; acc2[2] += a0 * q2;
      acc2[3] += a1 * q0; acc2[4] += a1 * q1; acc2[5] += a1 * q2;
      acc2[6] += a2 * q0; acc2[7] += a2 * q1; acc2[8] += a2 * q2;
    }
    else
    {
      const double* P = sh.gp[g][slot];
      const double F0 = P[0], F1 = P[1], F2 = P[2], F3 = P[3], F4 = P[4], F5 = P[5], F6 = P[6],
                   F7 = P[7], F8 = P[8];
      const double S0 = P[9], S1 = P[10], S2 = P[11], S3 = P[12], S4 = P[13], S5 = P[14];
      const double fa0 = F0 * a0 + F3 * a1 + F6 * a2;
      const double fa1 = F1 * a0 + F4 * a1 + F7 * a2;
      const double fa2 = F2 * a0 + F5 * a1 + F8 * a2;
      const double M0 = F0 * F0 + F3 * F3 + F6 * F6, M1 = F1 * F1 + F4 * F4 + F7 * F7,
                   M2 = F2 * F2 + F5 * F5 + F8 * F8, M3 = F0 * F1 + F3 * F4 + F6 * F7,
                   M4 = F1 * F2 + F4 * F5 + F7 * F8, M5 = F2 * F0 + F5 * F3 + F8 * F6;
      // a.S (S symmetric): geo = (S a).b
      const double sa0 = S0 * a0 + S3 * a1 + S5 * a2;
      const double sa1 = S3 * a0 + S1 * a1 + S4 * a2;
      const double sa2 = S5 * a0 + S4 * a1 + S2 * a2;
      auto one = [&](double* acc, double b0, double bb1, double bb2) {
        const double fb0 = F0 * b0 + F3 * bb1 + F6 * bb2;
        const double fb1 = F1 * b0 + F4 * bb1 + F7 * bb2;
        const double fb2 = F2 * b0 + F5 * bb1 + F8 * bb2;
        acc[0] += fa0 * fb0; acc[1] += fa0 * fb1; acc[2] += fa0 * fb2;
        acc[3] += fa1 * fb0; acc[4] += fa1 * fb1; acc[5] += fa1 * fb2;
        acc[6] += fa2 * fb0; acc[7] += fa2 * fb1; acc[8] += fa2 * fb2;
        const double ab = a0 * b0 + a1 * bb1 + a2 * bb2;
        acc[9] += ab * M0;
        acc[10] += ab * M1;
        acc[11] += ab * M2;
        acc[12] += ab * M3;
        acc[13] += ab * M4;
        acc[14] += ab * M5;
        acc[15] += sa0 * b0 + sa1 * bb1 + sa2 * bb2;
      };
      one(acc1, p0, p1, p2);
      one(acc2, q0, q1, q2);
    }
  };
  auto load_p = [&](int p, double2* v) {
    const int nd[3] = {a, b1, b2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) v[3 * k + d] = *reinterpret_cast<const double2*>(&sh.nx[nx2i(d, p, slot, nd[k])]);
  };
#ifndef FCG_VISIT_NOPIPE
  // structural passes: software-pipelined, the nine N_XYZ pairs of Gauss-point pair p + 1 are in
  // flight while pair p computes (the scheduling barrier keeps the loads ahead of the FMAs; the
  // compiler otherwise issues each pair's loads after the previous pair's FMAs and waits for them,
  // an exposed LDS round trip per pair at two waves per SIMD).  +47 VGPRs (189 -> 236, still two
  // workgroups per CU); the TSI instantiations would spill, they keep the plain loop.
#ifdef FCG_VISIT_PIPE_TSI
  if constexpr (true)
#else
  if constexpr (!TSI)
#endif
  {
  double2 buf[2][9];
  load_p(0, buf[0]);
#pragma unroll
  for (int p = 0; p < 4; ++p)
  {
    if (p < 3) load_p(p + 1, buf[(p + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    const double2* v = buf[p & 1];
    gp_body(2 * p, v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, v[8].x);
    gp_body(2 * p + 1, v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y, v[8].y);
  }
  return;
  }
#endif
#pragma unroll
  for (int p = 0; p < 4; ++p)
  {
    double2 v[9];
    load_p(p, v);
    gp_body(2 * p, v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, v[8].x);
    gp_body(2 * p + 1, v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y, v[8].y);
  }
}

// TSI blocks of an accumulated (linear) part: k_ST(A,B) [3] | k_TS(A,B) [3] | k_TT(A,B)
template <bool TH = false>
__device__ inline void tsi_block(const SweepArgs& A, const double* acc, double* Tv)
{
  const double m = A.tsi_m, mk = A.tsi_m * A.tsi_kts;
  constexpr int o = TH ? 0 : 9;
  Tv[0] = m * acc[o + 0];
  Tv[1] = m * acc[o + 1];
  Tv[2] = m * acc[o + 2];
  Tv[3] = mk * acc[o + 3];
  Tv[4] = mk * acc[o + 4];
  Tv[5] = mk * acc[o + 5];
  Tv[6] = TH ? A.tsi_k * acc[6] - acc[7] : A.tsi_k * (acc[0] + acc[4] + acc[8]) - acc[15];
}

// K_AB of an accumulated part (isotropic StVK)
template <int KIN>
__device__ inline void block_k(const StVK& m, const double* acc, double* Kb)
{
  const double lam = m.lambda, mu = m.mu;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q)
    {
      // the contraction spelled out (fma(lam, G_rq, mu G_qr), what the compiler has always made of
      // lam * G_rq + mu * G_qr here): left to the compiler, which of the two products is fused
      // depends on the code around the inlined call, and the last bits of K with it
      Kb[3 * r + q] = __builtin_fma(lam, acc[3 * r + q], mu * acc[3 * q + r]);
    }
  if (KIN == 0)
  {
    const double tr = mu * (acc[0] + acc[4] + acc[8]);
    Kb[0] += tr;
    Kb[4] += tr;
    Kb[8] += tr;
  }
  else
  {
    Kb[0] += mu * acc[9] + acc[15];
    Kb[4] += mu * acc[10] + acc[15];
    Kb[8] += mu * acc[11] + acc[15];
    Kb[1] += mu * acc[12]; Kb[3] += mu * acc[12];
    Kb[5] += mu * acc[13]; Kb[7] += mu * acc[13];
    Kb[2] += mu * acc[14]; Kb[6] += mu * acc[14];
  }
}

// Diagnostic phase stamps: thread 0 of each workgroup adds the cycles of every phase (including
// the barrier wait that ends it) into A.stamps[phase]; off (uniform branch, no s_memtime) when
// A.stamps is NULL.  Phases: 0 element stage (A), 1 visit stage (B); [5] counts workgroups.
#define FCG_STAMP(i)                                                                               \
  if (A.stamps && tid == 0)                                                                        \
  {                                                                                                \
    const unsigned long long now = __builtin_amdgcn_s_memtime();                                  \
    st_acc[i] += now - st_last;                                                                    \
    st_last = now;                                                                                 \
  }

// MODE 0: structure (K, f_int); 1: fused TSI (K_SS, k_ST, k_TS, k_TT, f_S, f_T in one pass);
// 2: the thermal-only pass that follows a MODE-0 linear sweep (k_ST, k_TS, k_TT, f_T, and
// k_ST (T - T_0) added into f_S) -- 8 accumulators per block instead of 16, no K stores;
// 3: structure with the lower-plane blocks deferred one layer (hold_lo): the linear tangent
// kernel.  Written in two layers' parts a row leaves lines half-written in L2 between the two:
// 1.18x the K bytes written on the lattice-numbered 1M box (the lines at a row's start and at its
// byte 216), 1.4x on the renumbered one, whose rows do not list the lattice neighbours plane by
// plane (input-file numbering: a row's 27 triples land all over its 648 bytes);
// 4: the create-time geometry pass (sweep_geometry_pass): the loop's loads of the reference
// coordinates and the element lattice and stage A's checks, no u, no visit stage, no stores.
// CHECKED = false (structural passes of a context whose geometry pass found nothing): stage A
// without the reference-geometry checks, the visit stage without the negative-fac mask and the
// NEG visit.  The arithmetic that gives nx, gp, K and f is the same: same bits.
template <int KIN, bool WANT_K, bool OVERWRITE, int MODE, bool CHECKED = true>
#ifndef FCG_SWEEP_WGS
#define FCG_SWEEP_WGS 2
#endif
__global__ __launch_bounds__(256, KIN ? 1 : FCG_SWEEP_WGS) void sweep_h8_kernel(SweepArgs A)
{
  constexpr bool TSI = MODE == 1 || MODE == 2, TH = MODE == 2, DEFER = MODE == 3, GEOM = MODE == 4;
  static_assert(!GEOM || (KIN == 0 && !WANT_K && CHECKED), "the geometry pass is one instantiation");
  static_assert(CHECKED || !TSI, "the TSI passes keep the checks");
  static_assert(!TSI || (KIN == 0 && WANT_K), "TSI is geometrically linear, full tangent");
  static_assert(!DEFER || WANT_K, "deferred blocks are K blocks");
  __shared__ SweepShared<KIN, TSI, TH, DEFER> sh;
  constexpr int NACC = TH ? 8 : ((KIN || TSI) ? 16 : 9);
  constexpr int NC = node_comps<TSI>();
  constexpr int NLD = (NNODE * NC + 255) / 256;  // node-load items per lane
  constexpr int NF = TSI ? 4 : 3;                // residual rows per node: f_S (3) | f_T
  const int tid = threadIdx.x;
  unsigned long long st_acc[3] = {0, 0, 0};
  unsigned long long st_last = A.stamps ? __builtin_amdgcn_s_memtime() : 0ull;
  const int tile = blockIdx.x;
  const int tx = tile % A.tiles_x;
  const int ty = (tile / A.tiles_x) % A.tiles_y;
  const int tz = tile / (A.tiles_x * A.tiles_y);
  const int i0 = A.I0 + TX * tx, j0 = A.J0 + TY * ty;
  const int kz0 = A.K0 + A.seg_planes * tz;
  const int kz1 = min(kz0 + A.seg_planes, A.K0 + A.NK);
  const uint32_t* prec_tile = A.plane_rec + (int64_t(ty) * A.tiles_x + tx) * A.NK * PLANE_REC_WORDS;
  const int64_t LX = A.EX + 1, LY = A.EY + 1;
  // Regular layers (REGK: the unchecked linear MODE-0 and MODE-3 kernels).  fcg_create has found, per tile,
  // a run of node planes whose rows all have 81 entries, one pattern of neighbour positions and
  // rows / bases in arithmetic progression along a tile row, with all 25 elements of every layer
  // between them present (classify_regular_tiles).  The layers rlo <= L < rhi of this workgroup
  // lie inside the run and the write range: their emits take pos from lane constants, len = 81
  // as a literal and row0 / base from the four tile rows' words of the record, with no validity
  // branch; their element ids are not loaded; and a plane both of whose layers are regular is
  // loaded as its compact record (12 words instead of 288), put where the full record holds the
  // same words.  All of it is workgroup-uniform (scalar compares).
  constexpr bool REGK = (MODE == 0 || MODE == 3) && KIN == 0 && !CHECKED;
  int rlo = 0, rhi = 0;
  const uint32_t* creg_tile = nullptr;
  if constexpr (REGK)
  {
    const int64_t txy = int64_t(ty) * A.tiles_x + tx;
    rlo = max(A.K0 + A.reg_tile[2 * txy], kz0);
    rhi = min(A.K0 + A.reg_tile[2 * txy + 1], kz1) - 1;
    creg_tile = A.reg_rec + txy * A.NK * REG_REC_WORDS;
  }
  auto reg_layer = [&](int L) -> bool { return REGK && L >= rlo && L < rhi; };
  auto reg_plane = [&](int p) -> bool { return REGK && p > rlo && p < rhi; };  // layers p - 1 and p

  if (tid < 24) sh.gxi[tid / 3][tid % 3] = A.tables[392 + tid];
  if (tid < 8) sh.w8[tid] = A.tables[384 + tid];
  if (TSI && tid < 64)
  {
    (&sh.Ng[0][0])[tid] = A.Ngp[tid];
    sh.NgT[TSI ? (tid & 7) : 0][tid >> 3] = A.Ngp[tid];
  }

  // stage-A lane: element slot s, Gauss point g
  const int s = tid >> 3, g = tid & 7;
  const bool a_lane = s < NSLOT;
  const int sx = s % EXN, sy = s / EXN;
  const int ex = i0 - 1 + sx, ey = j0 - 1 + sy;
  const bool exy_in = a_lane && ex >= A.EX0 && ex < A.EX0 + A.EX && ey >= A.EY0 && ey < A.EY0 + A.EY;
  auto load_elem = [&](int lz) -> int {
    // a regular layer holds all 25 elements, and REGK kernels use the id only as "present"
    if (reg_layer(lz)) return a_lane ? 0 : -1;
    if (!exy_in || lz < A.EZ0 || lz >= A.EZ0 + A.EZ) return -1;
    return A.elem_at[(int64_t(lz - A.EZ0) * A.EY + (ey - A.EY0)) * A.EX + (ex - A.EX0)];
  };
  // node-load items tid + 256 j: column ncol of the 6 x 6 node grid, component ncomp
  // (X 0-2, u 3-5; TSI: v 6-8, T 9)
  bool n_lane[NLD], nxy_in[NLD];
  int ncol[NLD], ncomp[NLD];
  int64_t nlat_xy[NLD];
#pragma unroll
  for (int j = 0; j < NLD; ++j)
  {
    const int v = tid + 256 * j;
    n_lane[j] = v < NNODE * NC;
    ncol[j] = v / NC;
    ncomp[j] = v - NC * (v / NC);
    const int ni = i0 - 1 + ncol[j] % NXN, nj = j0 - 1 + ncol[j] / NXN;
    nxy_in[j] = n_lane[j] && ni >= A.EX0 && ni <= A.EX0 + A.EX && nj >= A.EY0 && nj <= A.EY0 + A.EY;
    nlat_xy[j] = nxy_in[j] ? int64_t(nj - A.EY0) * LX + (ni - A.EX0) : 0;
  }
  // node loads in two steps, so that no load waits on another inside a layer: the DOF of a plane
  // is fetched one layer before its values (load_dof), the values (load_val) are issued before
  // stage A and consumed after it -- the wait for them then also covers the previous layer's K
  // stores (gfx9 counts stores in vmcnt), which stage A has had time to retire.
  auto node_li = [&](int j, int P) -> int64_t { return int64_t(P - A.EZ0) * LX * LY + nlat_xy[j]; };
  auto node_in = [&](int j, int P) -> bool { return nxy_in[j] && P >= A.EZ0 && P <= A.EZ0 + A.EZ; };
  auto load_dof = [&](int j, int P) -> int32_t {
    if (GEOM || !node_in(j, P) || ncomp[j] < 3) return -1;  // (the geometry pass reads no u)
    return A.lat_dof[node_li(j, P)];
  };
  // One load instruction behind a selected address, not a load per branch: the lanes of a wave
  // take different branches, the branches run one after the other, and where the second one's
  // address arithmetic reused the first one's destination registers the compiler had to wait for
  // every access in flight (vmcnt(0): the previous layer's K stores) at the top of the layer.
  auto load_val = [&](int j, int P, int32_t dof) -> double {
    const int cp = ncomp[j];
    const bool has = node_in(j, P) && (cp < 3 || dof >= 0);
    const double* src = A.lat_x + (3 * node_li(j, P) + cp);
    if (cp >= 3) src = A.u_col + (dof + cp - 3);
    if (TSI && cp >= 6) src = A.v_col + (dof + cp - 6);
    if (TSI && cp >= 9) src = A.T_col + dof / 3;
    return has ? *src : 0.0;
  };
  auto load_node = [&](int j, int P) -> double { return load_val(j, P, load_dof(j, P)); };
  auto load_rec = [&](int p, uint32_t* w) {
    const bool in = p >= kz0 && p < kz1;
    const uint32_t* src = prec_tile + int64_t(in ? p - A.K0 : 0) * PLANE_REC_WORDS;
    // (a compact plane lies inside the write range) one load behind a selected address and
    // predicate, as load_val: lanes 0..11 fetch the compact record's words, nobody a second word
    const bool cp = reg_plane(p);
    if (cp) src = creg_tile + int64_t(p - A.K0) * REG_REC_WORDS;
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
      const int v = tid + 256 * k;
      if (v < PLANE_REC_WORDS) w[k] = (in && (!cp || v < 12)) ? src[v] : (v < PR_LEN ? 0xFFFFFFFFu : 0u);
    }
  };
  auto store_rec = [&](int p, const uint32_t* w) {
    // compact word v: row0 of tile row v (v < 4), else half (v & 1) of tile row (v - 4) / 2's base,
    // each at the place of the row's first column in the full record; the slot's other words are
    // stale and not read (both layers of a compact plane take the regular emit)
    const bool cp = reg_plane(p);
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
      const int v = tid + 256 * k;
      const int at = cp ? (v < 4 ? PR_ROW0 + 4 * v : PR_BASE + 8 * (((v - 4) >> 1) & 3) + (v & 1)) : v;
      if (v < PLANE_REC_WORDS && (!cp || v < 12)) sh.prec[ring(p)][at] = w[k];
    }
  };

  // visit lane: node column c, task k
  const int c = tid >> 4, k = tid & 15;
  const int cx = c % TX, cy = c / TX;
  const uint32_t vis0 = kVisit[k][0], vis1 = kVisit[k][1];
  // regular layers: entry offset of this lane's three blocks from the base of its tile row's
  // first column (the pattern's position plus 243 per column), lane constants
  int32_t rp_a = 0, rp_b = 0, rp_s = 0;  // first visit's block, second visit's, self block
  if constexpr (REGK && WANT_K)
  {
    rp_a = A.reg_pos[(vis0 >> 16) & 31] + 243 * cx;
    rp_b = A.reg_pos[(vis1 >> 16) & 31] + 243 * cx;
    rp_s = A.reg_pos[(vis1 >> 11) & 31] + 243 * cx;
  }

  // Layers without elements (the linear structural passes; workgroup-uniform scalar compares, and
  // never true at a rank's interior face, whose ghost layer holds elements):
  // * the bottom segment's first layer, K0 - 1, lies below the element box.  Its sums are +0 (a
  //   missing element stores exact zeros, and every sum starts from the constant +0), it writes
  //   nothing (wl is false, and no row of plane K0 has a neighbour below) and what it holds equals
  //   the prologue's zeros: the sweep starts one layer later, at L0;
  // * the top segment's last layer lies on the top node plane: no stage A and no visits, the emits
  //   run on the zero accumulators (the held in-plane parts and plane L's f rows are due).
  constexpr bool SKIPE = KIN == 0 && !TSI && !GEOM;
  const bool skip_e = SKIPE && A.skip_empty != 0;
  const int L0 = (skip_e && kz0 - 1 < A.EZ0) ? kz0 : kz0 - 1;
  // --- prologue: node planes L0, L0+1 and their records; prefetch plane L0+2
#pragma unroll
  for (int j = 0; j < NLD; ++j)
    if (n_lane[j])
    {
      sh.node[ring(L0)][ncol[j]][ncomp[j]] = load_node(j, L0);
      sh.node[ring(L0 + 1)][ncol[j]][ncomp[j]] = load_node(j, L0 + 1);
    }
  {
    uint32_t w[2];
    load_rec(L0, w);
    store_rec(L0, w);
    load_rec(L0 + 1, w);
    store_rec(L0 + 1, w);
  }
  int32_t dof_nxt[NLD];  // DOF of plane L+2's node-load items at the top of layer L
#pragma unroll
  for (int j = 0; j < NLD; ++j) dof_nxt[j] = n_lane[j] ? load_dof(j, L0 + 2) : -1;
  int e_cur = load_elem(L0);
  for (int v = tid; v < int(sizeof(sh.hold) / sizeof(double)); v += 256) (&sh.hold[0][0][0])[v] = 0.0;
  if constexpr (DEFER)
    for (int v = tid; v < int(sizeof(sh.hold_lo) / sizeof(double)); v += 256) (&sh.hold_lo[0][0][0])[v] = 0.0;
  double fkeep[NF];  // lane k = 8: D-side residual part of plane L+1's rows
#pragma unroll
  for (int d = 0; d < NF; ++d) fkeep[d] = 0.0;
  // the prologue's loads land here, so that the compiler's wait bookkeeping does not carry them
  // into the loop (where the first use of e_cur would otherwise wait for every load in flight)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int L = L0; L < kz1; ++L)
  {
    const bool empty_top = skip_e && L >= A.EZ0 + A.EZ;  // no element in this layer (see L0)
    // issue the loads of plane L+2 (values, record), plane L+3's DOFs and layer L+1's element
    const int e_nxt = load_elem(L + 1);
    double node_nxt[NLD];
    int32_t dof_nn[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j)
    {
#ifdef FCG_PROBE_TH_NOPREFETCH
      if (TH)
      {
        // timing probe only (wrong results): the thermal pass without its plane prefetch
        node_nxt[j] = 0.0;
        dof_nn[j] = -1;
        continue;
      }
#endif
      node_nxt[j] = n_lane[j] ? load_val(j, L + 2, dof_nxt[j]) : 0.0;
      dof_nn[j] = n_lane[j] ? load_dof(j, L + 3) : -1;
    }
    uint32_t rec_nxt[2];
    load_rec(L + 2, rec_nxt);
    // A. element stage
#ifdef FCG_PROBE_NOSTAGEA
    // timing probe only (wrong results): no element stage
    if (a_lane && e_cur == -12345) sweep_stage_a<KIN, TSI, CHECKED, GEOM>(sh, A, s, g, sx, sy, L, e_cur);
#else
    if (a_lane && !empty_top) sweep_stage_a<KIN, TSI, CHECKED, GEOM>(sh, A, s, g, sx, sy, L, e_cur);
#endif
    __syncthreads();
    FCG_STAMP(0);
    // commit plane L+2 (nodes and record into plane L-1's ring slot)
#pragma unroll
    for (int j = 0; j < NLD; ++j)
    {
      if (n_lane[j]) sh.node[ring(L + 2)][ncol[j]][ncomp[j]] = node_nxt[j];
      dof_nxt[j] = dof_nn[j];
    }
    store_rec(L + 2, rec_nxt);
    if constexpr (GEOM)
    {
      e_cur = e_nxt;
      __syncthreads();
      continue;
    }
#ifdef FCG_SWEEP_COMMIT_STAMP
    // diagnostic builds only (it costs the fused TSI pass a spill)
    if (A.stamps)
    {
      // phase 2: the commit's wait for plane L+2's loads (and, behind them in vmcnt, the previous
      // layer's K stores)
      __asm__ volatile("" ::"v"(rec_nxt[0]), "v"(node_nxt[0]));
      FCG_STAMP(2);
    }
#endif

    // B. visit stage
    const bool wl = L >= kz0, wl1 = L + 1 < kz1;
    constexpr bool kRingSel = !TSI && (!DEFER || KIN == 0);
    const int rL = ring(L), rL1 = ring(L + 1);
    const uint32_t* recL = sh.prec[rL];
    const uint32_t* recL1 = sh.prec[rL1];
    // linear kinematics: this lane's share of f_A = sum_B K_AB u_B for the row node A of its side
    // (plane L + (k >> 3))
    double fpart[NF];
#pragma unroll
    for (int d = 0; d < NF; ++d) fpart[d] = 0.0;
    // the visit stage, once per emit flavour: REG (a regular layer of a REGK kernel) takes the
    // record-free emit described at rlo / rhi above, everything else the records
    const bool regL = reg_layer(L);
    auto visit_stage = [&](auto reg_c)
    {
      constexpr bool REG = decltype(reg_c)::value;
      // finished block t of this lane's column (this layer's elements): hold it, or write it plus
      // the part held by lane k + 8 (same role, D side) since the previous layer.  TSI: Tv holds
      // the block's k_ST / k_TS / k_TT entries (tsi_block), treated the same way.
#ifdef FCG_PROBE_WG3
      constexpr bool kProbeWg3 = true;
#else
      constexpr bool kProbeWg3 = false;
#endif
      // An emit in two steps.  emit_load issues every LDS read the block needs -- its record
      // fields, the neighbour's u and (kBranchFree) the nine held entries -- with no branch between
      // them: one LDS round trip.  emit_finish does the rest.  The two blocks that end a layer
      // (the second visit's and the self block) load together ahead of either's work, so that the
      // pair exposes one round trip, not two (see the end of the visit stage).
      constexpr bool kBranchFree = !TSI && (!DEFER || KIN == 0) && !kProbeWg3;
      struct EmitIn {
        int32_t row0, len32;
        uint32_t base_lo, base_hi;
        uint16_t pos;
        const double* ub;
        double u0, u1, u2;
        double* h;
        double held[9];
      };
      auto emit_load = [&](int act, int t, EmitIn& in) {
        // (DEFER: a lower-plane block is written one layer later, into plane L's row)
        const uint32_t* rec = (act == kActWriteL1 && !DEFER) ? recL1 : recL;
        if constexpr (REG)
        {
          // the base of the tile row's first column: the one record field a regular emit reads
          in.row0 = 0;
          in.pos = 0;
          in.len32 = 81;
          in.base_lo = WANT_K ? rec[PR_BASE + 8 * cy] : 0u;
          in.base_hi = WANT_K ? rec[PR_BASE + 8 * cy + 1] : 0u;
        }
        else
        {
          in.row0 = WANT_K ? int32_t(rec[PR_ROW0 + c]) : -1;
          in.pos = WANT_K ? reinterpret_cast<const uint16_t*>(rec + PR_NPOS)[27 * c + t] : 0;
          in.base_lo = WANT_K ? rec[PR_BASE + 2 * c] : 0u;
          in.base_hi = WANT_K ? rec[PR_BASE + 2 * c + 1] : 0u;
          in.len32 = WANT_K ? int32_t(rec[PR_LEN + c]) : 0;
        }
        if (KIN == 0)
        {
          const int dx = t % 3 - 1, dy = (t / 3) % 3 - 1, dz = t / 9 - 1;
          // the neighbour's plane is L or L + 1 (a layer's elements touch no other): a select
          // between two uniform ring slots where the registers allow it, not a per-lane % 3
          const int rU = kRingSel ? (((k >> 3) + dz) ? rL1 : rL) : ring(L + (k >> 3) + dz);
          in.ub = &sh.node[rU][(cy + 1 + dy) * NXN + cx + 1 + dx][3];
          in.u0 = in.ub[0];
          in.u1 = in.ub[1];
          in.u2 = in.ub[2];
        }
        if constexpr (kBranchFree)
        {
          // every lane reads nine entries and adds them (emit_finish): the U side its held part,
          // every other lane the zeros of the spare column (Kb + 0 is Kb but for the sign of a
          // zero; the D side's sum is not used).  No branch around the reads, no select or copy
          // behind them.
          // DEFER: a lower-plane block (t < 9) swaps with its slot of hold_lo the same way -- the
          // lane reads the block held since the previous layer and stores this layer's
          const bool lo = DEFER && act == kActWriteL1;
          in.h = sh.hold[c][(act == kActHold || act == kActWriteLHold) ? t - 9 : 0];
          if constexpr (DEFER) in.h = lo ? sh.hold_lo[c][t] : in.h;
          const double* hr = (act == kActWriteLHold || lo) ? in.h : sh.hold[TX * TY][0];
#pragma unroll
          for (int i = 0; i < 9; ++i) in.held[i] = hr[i];
        }
      };
      // rp: the block's entry offset in a regular layer (rp_a / rp_b / rp_s)
      auto emit_finish = [&](int act, int t, const EmitIn& in, int32_t rp, double* Kb, double* Tv) {
        const bool to_l1 = act == kActWriteL1 && !DEFER;
        const int32_t row0 = in.row0, len32 = in.len32;
        const uint32_t base_lo = in.base_lo, base_hi = in.base_hi;
        const uint16_t pos = in.pos;
        if (KIN == 0)
        {
          const double* ub = in.ub;
          const double u0 = in.u0, u1 = in.u1, u2 = in.u2;
          if (!TH)
#pragma unroll
            for (int r = 0; r < 3; ++r)  // (contraction spelled out as in block_k, the compiler's own so far)
              fpart[r] += __builtin_fma(Kb[3 * r + 2], u2, __builtin_fma(Kb[3 * r], u0, Kb[3 * r + 1] * u1));
          if (TSI)
          {
            // f_S += k_ST (T - T_0) (partition of unity), f_T = k_TT T (exact for linear TSI)
            const double TB = ub[6];
            const double dT = TB - A.tsi_T0;
#pragma unroll
            for (int r = 0; r < 3; ++r) fpart[r] += Tv[r] * dT;
            fpart[NF - 1] += Tv[6] * TB;
          }
        }
        // in-plane blocks: every lane of the pair reads the held entry first, then the holder
        // (D side) stores this layer's part and the U side adds the part held since last layer
        if constexpr (kBranchFree)
        {
          // (the caller has put a compiler barrier between the reads and this write: all reads
          // issue before any write, and the LDS executes a wavefront's operations in order)
          const bool lo = DEFER && act == kActWriteL1;
          if (act == kActHold || lo)
          {
#pragma unroll
            for (int i = 0; i < 9; ++i) in.h[i] = Kb[i];
          }
          // (DEFER: the held lower-plane block leaves as it is, bit for bit -- it belongs to plane
          // L's row, and the fields emit_load has read are plane L's; in a regular layer plane L's
          // row is a regular row, whichever path the layer that held the block took)
#pragma unroll
          for (int i = 0; i < 9; ++i) Kb[i] = lo ? in.held[i] : in.held[i] + Kb[i];
        }
        else
        if (act == kActHold || act == kActWriteLHold)
        {
          constexpr int NK = TH ? 0 : 9;  // structural entries held (none in the thermal pass)
          constexpr int NH = NK + (TSI ? 7 : 0);
#ifdef FCG_PROBE_WG3
          double* h = sh.hold[0][t - 9];
#else
          double* h = sh.hold[c][t - 9];
#endif
          double held[NH];
#pragma unroll
          for (int i = 0; i < NH; ++i) held[i] = h[i];
          // all reads issue before any write (the compiler must not sink the U side's reads into
          // its branch behind the D side's writes; the LDS executes a wavefront's ops in order)
          __asm__ volatile("" ::: "memory");
          if (act == kActHold)
          {
#pragma unroll
            for (int i = 0; i < NK; ++i) h[i] = Kb[i];
            if (TSI)
#pragma unroll
              for (int i = 0; i < 7; ++i) h[NK + i] = Tv[i];
          }
          else
          {
#pragma unroll
            for (int i = 0; i < NK; ++i) Kb[i] = held[i] + Kb[i];
            if (TSI)
#pragma unroll
              for (int i = 0; i < 7; ++i) Tv[i] = held[NK + i] + Tv[i];
          }
        }
        if (act == kActHold || !WANT_K) return;
        if constexpr (DEFER && !kBranchFree)
        {
          if (act == kActWriteL1)
          {
            // (TotLag: no branch-free hold) the block held since the previous layer belongs to
            // plane L's row: it is written now, beside that row's other blocks and by the same
            // stores (the fields emit_load has read are plane L's); this layer's block waits
            double* h = sh.hold_lo[c][t];
            double old[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) old[i] = h[i];
            __asm__ volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < 9; ++i) h[i] = Kb[i];
#pragma unroll
            for (int i = 0; i < 9; ++i) Kb[i] = old[i];
          }
        }
        // (a regular layer lies inside the write range, its rows are owned and hold all 27 blocks)
        if constexpr (!REG)
          if (!(to_l1 ? wl1 : wl) || row0 < 0 || pos == 0xFFFF) return;
        const int64_t base = int64_t(base_lo) | (int64_t(base_hi) << 32);
        const int64_t len = REG ? int64_t(81) : int64_t(len32);
#ifdef FCG_PROBE_KL2
        // timing probe only (wrong results): the same stores, folded into 256 KB (L2-resident)
        double* dst = A.K + ((base + pos) & 0x7FFF);
#else
        double* dst = A.K + base + (REG ? int64_t(rp) : int64_t(pos));
#endif
#ifdef FCG_PROBE_NOKSTORE
        // timing probe only (wrong results): no K stores
        if (Kb[0] == 12345.678) dst[0] = Kb[1];
        if (false)
#else
        if (!TH)
#endif
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int qq = 0; qq < 3; ++qq)
            {
              if (OVERWRITE)
#ifdef FCG_PROBE_KNT  // timing probe: non-temporal K stores (4.2 ms instead of 0.98: partial lines)
                __builtin_nontemporal_store(Kb[3 * r + qq], dst + r * len + qq);
#else
                dst[r * len + qq] = Kb[3 * r + qq];
#endif
              else
                dst[r * len + qq] += Kb[3 * r + qq];
            }
#if defined(FCG_PROBE_TH_NOSTORE) || defined(FCG_PROBE_TH_1STORE)
        if (TH)
        {
          // timing probes only (wrong results): no thermal stores / one 8-byte store per block
#ifdef FCG_PROBE_TH_1STORE
          A.Ktt[base / 9 + pos / 3] = Tv[0] + Tv[1] + Tv[2] + Tv[3] + Tv[4] + Tv[5] + Tv[6];
#else
          if (Tv[0] == 12345.678) A.Ktt[0] = Tv[1];
#endif
          return;
        }
#endif
        if (TSI)
        {
          // node-consistent block graphs (checked by fcg_tsi_evaluate_fused): the k_ST rows of the
          // node start at base / 3 (length len / 3), its k_TS row at base / 3, its k_TT row at
          // base / 9; the neighbour's thermo column sits at pos / 3, its displacements at pos
          const int64_t bst = base / 3, lst = len / 3, pst = pos / 3;
#ifdef FCG_PROBE_TSI_STORE_INTERLEAVED
          if constexpr (true)  // timing probe: the order before round 6
#else
          if constexpr (false)
#endif
          {
#pragma unroll
          for (int r = 0; r < 3; ++r)
          {
            double* d1 = A.Kst + bst + r * lst + pst;
            double* d2 = A.Kts + bst + pos + r;
            if (OVERWRITE)
            {
              *d1 = Tv[r];
              *d2 = Tv[3 + r];
            }
            else
            {
              *d1 += Tv[r];
              *d2 += Tv[3 + r];
            }
          }
          }
          else
          {
          // k_TS's three adjacent values first, with no k_ST store between them (the two arrays
          // may alias as far as the compiler knows), so that they leave as one 16-byte and one
          // 8-byte store instead of three 8-byte stores
          double* d2 = A.Kts + bst + pos;
#pragma unroll
          for (int r = 0; r < 3; ++r)
          {
            if (OVERWRITE)
              d2[r] = Tv[3 + r];
            else
              d2[r] += Tv[3 + r];
          }
#pragma unroll
          for (int r = 0; r < 3; ++r)
          {
            double* d1 = A.Kst + bst + r * lst + pst;
            if (OVERWRITE)
              *d1 = Tv[r];
            else
              *d1 += Tv[r];
          }
          }
          double* d3 = A.Ktt + base / 9 + pst;
          if (OVERWRITE)
            *d3 = Tv[6];
          else
            *d3 += Tv[6];
        }
      };
      auto emit = [&](int act, int t, int32_t rp, double* Kb, double* Tv) {
        EmitIn in;
        emit_load(act, t, in);
        __asm__ volatile("" ::: "memory");
        emit_finish(act, t, in, rp, Kb, Tv);
      };
      double acc1[NACC], acc2[NACC];
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc1[i] = acc2[i] = 0.0;
      // the two element visits of this lane; acc2 is finished after a visit when flush2 is set.
      // Without TSI both visits' negative-fac masks are read up front (one LDS round trip instead
      // of one ahead of each visit's branch; the TSI instantiation has no registers to spare).
      auto slot_of = [&](uint32_t w) { return (cx + int(w & 1)) + EXN * (cy + int((w >> 1) & 1)); };
      uint32_t nm_pre[2] = {0u, 0u};
      if constexpr (!TSI && CHECKED)
      {
        nm_pre[0] = sh.neg[slot_of(vis0)];
        nm_pre[1] = sh.neg[slot_of(vis1)];
      }
      // the two visits unrolled where the registers allow it (the structural linear passes: 254
      // VGPRs, no spills; the next visit's loads then overlap the first one's emit, -3 % on the
      // headline kernel, profiles/r06/r06_sweep_visit_unroll_ab.txt); the TSI passes spill
      // unrolled, and the TotLag ones keep the rolled loop (FCG_SWEEP_VISIT_UNROLL=0/1 overrides)
#ifndef FCG_SWEEP_VISIT_UNROLL
#define FCG_SWEEP_VISIT_UNROLL (!TSI && KIN == 0)
#endif
      constexpr int kVisitUnroll = (FCG_SWEEP_VISIT_UNROLL) ? 2 : 1;
      // unrolled: the second visit's block waits for the self block, and the two load together
      // (not in the deferred kernels: paired, the unchecked one spills 4 VGPRs at 256 and measured
      // slower than unpaired, profiles/sweep_rows/headline_ab.txt)
      constexpr bool kPairEmits = kVisitUnroll == 2 && kBranchFree && !DEFER;
      double Kb2[9];
#pragma unroll kVisitUnroll
      for (int v = 0; v < 2; ++v)
      {
        const uint32_t w = v == 0 ? vis0 : vis1;
        const int a = (w >> 2) & 7, b1 = (w >> 5) & 7, b2 = (w >> 8) & 7;
        const int slot = slot_of(w);
        if constexpr (!CHECKED)
        {
          // An always-taken uniform branch on a value the compiler cannot see through: the visit
          // keeps a basic block of its own, as under the checked kernel's mask branch.  Inlined
          // into the surrounding block it costs spills (10-16 VGPRs on the headline kernel, 150
          // and more on MODE 3 and TotLag); so placed it frees 9 (253 -> 244).  One s_cmp and
          // one s_cbranch per visit, no LDS read behind it.  The one case in which it is not taken:
          // a layer without elements, whose accumulators stay +0.
          uint32_t skipv = SKIPE ? uint32_t(__builtin_amdgcn_readfirstlane(empty_top ? 1 : 0)) : 0u;
          __asm__ volatile("" : "+s"(skipv));
          if (skipv == 0u) sweep_visit<KIN, false, TSI, TH>(sh, slot, a, b1, b2, 0u, acc1, acc2);
        }
        else
        {
          const uint32_t nm = TSI ? sh.neg[slot] : (v == 0 ? nm_pre[0] : nm_pre[1]);
          if (empty_top)
          {
            // (a layer without elements: the accumulators stay +0)
          }
          else if (nm == 0u)
            sweep_visit<KIN, false, TSI, TH>(sh, slot, a, b1, b2, nm, acc1, acc2);
          else
            sweep_visit<KIN, true, TSI, TH>(sh, slot, a, b1, b2, nm, acc1, acc2);
        }
        if ((w >> 24) & 1u)
        {
          double Kb[9], Tv[7];
          if (!TH) block_k<KIN>(A.mat, acc2, Kb);
          if (TSI) tsi_block<TH>(A, acc2, Tv);
#pragma unroll
          for (int i = 0; i < NACC; ++i) acc2[i] = 0.0;
          if (kPairEmits && v == 1)
          {
#pragma unroll
            for (int i = 0; i < 9; ++i) Kb2[i] = Kb[i];
          }
          else
            emit(int((w >> 21) & 7), int((w >> 16) & 31), v == 0 ? rp_a : rp_b, Kb, Tv);
        }
      }
      // acc1: the self block's two halves meet in lane r = 2 (order: qy = 1 half + qy = 0 half)
      {
        const int pair = int((vis1 >> 26) & 3);
        double Kb[9], Tv[7];
        if (!TH)
        {
          block_k<KIN>(A.mat, acc1, Kb);
#pragma unroll
          for (int i = 0; i < 9; ++i)
          {
            const double o = dpp_f64<kDppXor1>(Kb[i]);
            Kb[i] = pair == kPairRecv ? Kb[i] + o : Kb[i];  // a select, not a branch per entry
          }
        }
        if (TSI)
        {
          tsi_block<TH>(A, acc1, Tv);
#pragma unroll
          for (int i = 0; i < 7; ++i)
          {
            const double o = dpp_f64<kDppXor1>(Tv[i]);
            Tv[i] = pair == kPairRecv ? Tv[i] + o : Tv[i];
          }
        }
        if constexpr (kPairEmits)
        {
          // the reads of both blocks, then (behind a compiler barrier: no hold write may pass a
          // read; the two blocks' hold slots differ) the second visit's block and the self block
          const bool fl2 = (vis1 >> 24) & 1u, own = pair != kPairGive;
          const int act = int((vis1 >> 21) & 7), t2 = int((vis1 >> 16) & 31), t1 = int((vis1 >> 11) & 31);
          EmitIn in2, in1;
          // (every lane loads, with no branch: the visit word of a lane without the block still
          // carries valid fields, the self block's t of its pair lane, so its reads stay in bounds)
          emit_load(act, t2, in2);
          emit_load(act, t1, in1);
          __asm__ volatile("" ::: "memory");
          if (fl2) emit_finish(act, t2, in2, rp_b, Kb2, Tv);
          // (the second block's work stays behind the first's: interleaved, the two cost spills)
          __builtin_amdgcn_sched_barrier(0);
          if (own) emit_finish(act, t1, in1, rp_s, Kb, Tv);
        }
        else if (pair != kPairGive)
          emit(int((vis1 >> 21) & 7), int((vis1 >> 11) & 31), rp_s, Kb, Tv);
      }
    };
    if (WANT_K || KIN == 0)
    {
      if constexpr (REGK)
      {
        if (regL)
          visit_stage(std::true_type{});
        else
          visit_stage(std::false_type{});
      }
      else
        visit_stage(std::false_type{});
    }
    // residual rows of the column: the 8 lanes of a side sum their parts by a butterfly (every
    // lane ends with the same bits); lane 8 keeps plane L+1's D-side part for the next layer, lane
    // 0 adds the part lane 8 kept in the previous layer and writes plane L's rows.
    {
      double f[NF];
      if (KIN == 0)
      {
#pragma unroll
        for (int d = 0; d < NF; ++d) f[d] = fpart[d];
      }
      else
      {
        // f_A = sum_e sum_g fac F S N_XYZ_A: lane k takes Gauss points 4h..4h+3 (h = k & 1) of
        // quadrant q = (k >> 1) & 3 for the row node on side k >> 3 (0: plane L, the elements'
        // bottom node; 1: plane L+1, their top node)
        const int fside = k >> 3, fq = (k >> 1) & 3, fh = k & 1;
        const int fqx = fq & 1, fqy = fq >> 1;
        const int fslot = (cx + fqx) + EXN * (cy + fqy);
        const int fn = node_at(1 - fqx, 1 - fqy, fside);
#pragma unroll
        for (int d = 0; d < 3; ++d) f[d] = 0.0;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
        {
          const int gq = 4 * fh + gg;
          const double a0 = sh.nx[nx2i(0, gq >> 1, fslot, fn) + (gq & 1)],
                       a1 = sh.nx[nx2i(1, gq >> 1, fslot, fn) + (gq & 1)],
                       a2 = sh.nx[nx2i(2, gq >> 1, fslot, fn) + (gq & 1)];
          const double* P = sh.gp[KIN ? gq : 0][KIN ? fslot : 0];
          const double t0 = P[9] * a0 + P[12] * a1 + P[14] * a2;
          const double t1 = P[12] * a0 + P[10] * a1 + P[13] * a2;
          const double t2 = P[14] * a0 + P[13] * a1 + P[11] * a2;
          const double cc = P[15];
          f[0] += cc * (P[0] * t0 + P[3] * t1 + P[6] * t2);
          f[1] += cc * (P[1] * t0 + P[4] * t1 + P[7] * t2);
          f[2] += cc * (P[2] * t0 + P[5] * t1 + P[8] * t2);
        }
      }
      // read ahead of the butterfly (a regular layer: the tile row's first row0 plus 3 per column)
      const int32_t frow0 = int32_t(recL[PR_ROW0 + (regL ? 4 * cy : c)]) + (regL ? 3 * cx : 0);
      double fp[NF];
#pragma unroll
      for (int d = 0; d < NF; ++d)
      {
        f[d] += dpp_f64<kDppXor1>(f[d]);
        f[d] += dpp_f64<kDppXor2>(f[d]);
        f[d] += dpp_f64<kDppHalfMirror>(f[d]);
        fp[d] = dpp_f64<kDppRowRor8>(fkeep[d]);
      }
      if (k == 8)
      {
#pragma unroll
        for (int d = 0; d < NF; ++d) fkeep[d] = f[d];
      }
      else if (k == 0 && wl)
      {
        const int32_t row0 = frow0;
        if (row0 >= 0)
        {
#pragma unroll
          for (int d = 0; d < 3; ++d)
          {
#ifdef FCG_PROBE_TH_NORMW
            if (OVERWRITE)  // timing probe only (wrong f_S): no read-modify-write in the thermal pass
#else
            if (OVERWRITE && !TH)  // the thermal pass adds k_ST (T - T_0) to the structural f_S
#endif
              A.fint[row0 + d] = fp[d] + f[d];
            else
              A.fint[row0 + d] += fp[d] + f[d];
          }
          if (TSI)
          {
            // thermo row of the node = first structural row / 3 (checked at the fused call)
            if (OVERWRITE)
              A.fT[row0 / 3] = fp[NF - 1] + f[NF - 1];
            else
              A.fT[row0 / 3] += fp[NF - 1] + f[NF - 1];
          }
        }
      }
    }
    e_cur = e_nxt;
    __syncthreads();
    FCG_STAMP(1);
  }
  if (A.stamps && tid == 0)
  {
    for (int i = 0; i < 3; ++i) atomicAdd(&A.stamps[i], st_acc[i]);
    atomicAdd(&A.stamps[5], 1ull);
  }
}

}  // namespace

namespace {
SweepArgs sweep_args(const DeviceMesh& m, const double* d_u_col, double* d_K, double* d_fint)
{
  SweepArgs a{};
  a.u_col = d_u_col;
  a.lat_x = m.lat_x;
  a.lat_dof = m.lat_dof;
  a.elem_at = m.elem_at;
  a.plane_rec = m.plane_rec;
  a.reg_rec = m.reg_rec;
  a.reg_tile = m.reg_tile;
  a.reg_pos = m.reg_pos;
  a.tables = m.tables;
  a.K = d_K;
  a.fint = d_fint;
  a.err = m.err;
  a.stamps = m.stamps;
  a.mat = StVK{m.lambda, m.mu, m.cdiag};
  a.tiles_x = m.tiles_x;
  a.tiles_y = m.tiles_y;
  a.seg_planes = m.seg_planes;
  a.I0 = m.I0; a.J0 = m.J0; a.K0 = m.K0; a.NI = m.NI; a.NJ = m.NJ; a.NK = m.NK;
  a.EX0 = m.EX0; a.EY0 = m.EY0; a.EZ0 = m.EZ0; a.EX = m.EX; a.EY = m.EY; a.EZ = m.EZ;
  a.skip_empty = m.sweep_skip_empty ? 1 : 0;
  return a;
}
}  // namespace

#define FCG_SWEEP_C(KIN, CHECKED)                                                                  \
  if (want_k && m.sweep_defer && overwrite)                                                        \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, true, true, 3, CHECKED>), grid, block, 0, stream, a);  \
  else if (want_k && m.sweep_defer)                                                                \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, true, false, 3, CHECKED>), grid, block, 0, stream, a); \
  else if (want_k && overwrite)                                                                    \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, true, true, 0, CHECKED>), grid, block, 0, stream, a);  \
  else if (want_k)                                                                                 \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, true, false, 0, CHECKED>), grid, block, 0, stream, a); \
  else if (overwrite)                                                                              \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, false, true, 0, CHECKED>), grid, block, 0, stream, a); \
  else                                                                                             \
    hipLaunchKernelGGL((sweep_h8_kernel<KIN, false, false, 0, CHECKED>), grid, block, 0, stream, a);
// a context whose geometry pass found a code or a negative fac (or FCG_SWEEP_CHECKED=1) keeps the
// checked kernels: errors and values on every call as the checks give them
#define FCG_SWEEP(KIN)                                                                             \
  if (m.sweep_checked)                                                                             \
  {                                                                                                \
    FCG_SWEEP_C(KIN, true)                                                                         \
  }                                                                                                \
  else                                                                                             \
  {                                                                                                \
    FCG_SWEEP_C(KIN, false)                                                                        \
  }

// The TotLag instantiations live in their own translation unit, fcg_sweep_totlag.hip (this file
// with FCG_SWEEP_TOTLAG_TU), compiled without the SLP vectorizer: its pairing of the F / S
// arithmetic into 2-wide vectors costs the TotLag sweep 7-10 % (same-box A/B, 1M hex8: 3.09 ->
// 2.79 ms; profiles/r05/r05_noslp_sweep_ab.txt), while the linear and TSI sweeps gain nothing.
hipError_t launch_sweep_h8_totlag(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream);

#ifdef FCG_SWEEP_TOTLAG_TU
hipError_t launch_sweep_h8_totlag(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream)
{
  const int64_t ntiles = int64_t(m.tiles_x) * m.tiles_y * m.tiles_z;
  if (ntiles == 0) return hipSuccess;
  const SweepArgs a = sweep_args(m, d_u_col, d_K, d_fint);
  const dim3 grid{static_cast<unsigned>(ntiles), 1, 1};
  const dim3 block{256, 1, 1};
  FCG_SWEEP(1)
  return hipGetLastError();
}
#else
hipError_t launch_sweep_h8(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream)
{
  if (m.kinem != 0) return launch_sweep_h8_totlag(m, d_u_col, want_k, overwrite, d_K, d_fint, stream);
  const int64_t ntiles = int64_t(m.tiles_x) * m.tiles_y * m.tiles_z;
  if (ntiles == 0) return hipSuccess;
  const SweepArgs a = sweep_args(m, d_u_col, d_K, d_fint);
  const dim3 grid{static_cast<unsigned>(ntiles), 1, 1};
  const dim3 block{256, 1, 1};
  FCG_SWEEP(0)
  return hipGetLastError();
}

// The reference-geometry checks of stage A, once per context: the sweep's own kernel (MODE 4) on
// the sweep's grid, so the elements seen (ghost layers included) and every sign decision are the
// evaluates'.  Leaves the worst code, the lowest rejected column element and "some evaluated
// element has fac < 0 at a Gauss point" in m, and picks the kernels the evaluates launch.
hipError_t sweep_geometry_pass(DeviceMesh& m, bool force_checked, hipStream_t stream)
{
  m.geom_code = 0;
  m.geom_ele = INT32_MAX;
  m.geom_neg = false;
  m.sweep_checked = true;
  const int64_t ntiles = int64_t(m.tiles_x) * m.tiles_y * m.tiles_z;
  if (ntiles > 0)
  {
    int32_t* d_out = nullptr;
    int32_t out[3] = {0, INT32_MAX, 0};
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(out));
    if (he != hipSuccess) return he;
    he = hipMemcpyAsync(d_out, out, sizeof(out), hipMemcpyHostToDevice, stream);
    if (he == hipSuccess)
    {
      SweepArgs a = sweep_args(m, nullptr, nullptr, nullptr);
      a.err = d_out;
      a.stamps = nullptr;
      const dim3 grid{static_cast<unsigned>(ntiles), 1, 1};
      const dim3 block{256, 1, 1};
      hipLaunchKernelGGL((sweep_h8_kernel<0, false, false, 4>), grid, block, 0, stream, a);
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (he != hipSuccess) return he;
    m.geom_code = out[0];
    m.geom_ele = out[1];
    m.geom_neg = out[2] != 0;
  }
  m.sweep_checked = force_checked || m.geom_code != 0 || m.geom_neg;
  return hipSuccess;
}

hipError_t launch_sweep_h8_tsi(const DeviceMesh& m, const double* d_u_col, bool overwrite,
    double* d_K, double* d_fint, const SweepTsi& t, hipStream_t stream)
{
  const int64_t ntiles = int64_t(m.tiles_x) * m.tiles_y * m.tiles_z;
  if (ntiles == 0) return hipSuccess;
  SweepArgs a = sweep_args(m, d_u_col, d_K, d_fint);
  a.v_col = t.v_col;
  a.T_col = t.T_col;
  a.Ngp = t.Ngp;
  a.Kst = t.Kst;
  a.Kts = t.Kts;
  a.Ktt = t.Ktt;
  a.fT = t.fT;
  a.tsi_m = t.m;
  a.tsi_T0 = t.T0;
  a.tsi_k = t.conduct;
  a.tsi_kts = t.kts;
  const dim3 grid{static_cast<unsigned>(ntiles), 1, 1};
  const dim3 block{256, 1, 1};
  if (!t.split)
  {
    if (overwrite)
      hipLaunchKernelGGL((sweep_h8_kernel<0, true, true, 1>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((sweep_h8_kernel<0, true, false, 1>), grid, block, 0, stream, a);
    return hipGetLastError();
  }
  // split: the linear structural sweep (K_SS, f_S = K_SS u), then the thermal-only pass
  if (overwrite)
  {
    hipLaunchKernelGGL((sweep_h8_kernel<0, true, true, 0>), grid, block, 0, stream, a);
    hipLaunchKernelGGL((sweep_h8_kernel<0, true, true, 2>), grid, block, 0, stream, a);
  }
  else
  {
    hipLaunchKernelGGL((sweep_h8_kernel<0, true, false, 0>), grid, block, 0, stream, a);
    hipLaunchKernelGGL((sweep_h8_kernel<0, true, false, 2>), grid, block, 0, stream, a);
  }
  return hipGetLastError();
}
#endif  // FCG_SWEEP_TOTLAG_TU
#undef FCG_SWEEP
#undef FCG_SWEEP_C

}  // namespace fcg
