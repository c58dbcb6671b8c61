// fcg_tsi_internal.hpp -- the TSI context's layout, shared by fcg_tsi.hip (create: the upload of
// the host plan of fcg_tsi_plan.cpp; evaluate), fcg_tsi_solve.hip (the monolithic block operator
// and its solve), fcg_thermo.hip (capacity matrix and one-step-theta pass) and fcg_tsi_surface.hip (thermal
// boundary conditions).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace fcg {

struct TsiDevice {
  int npe = 8;
  int64_t n_ele = 0, n_node = 0, n_rownodes = 0, n_inc = 0;
  int64_t n_rows_s = 0, n_cols_s = 0, n_rows_t = 0, n_cols_t = 0;
  int64_t nnz_st = 0, nnz_ts = 0, nnz_tt = 0;
  double m = 0, T0 = 0, conduct = 0;
  int32_t* ele_nodes = nullptr;
  int32_t* ele_gid = nullptr;
  double* node_x = nullptr;
  int32_t* dof_col_s = nullptr;
  int32_t* dof_col_t = nullptr;
  int32_t* inc_of = nullptr;     // [n_ele][npe]
  int64_t* inc_ptr = nullptr;    // [n_rownodes + 1]
  int32_t* rn_srow = nullptr;    // [n_rownodes] first structural row
  int32_t* rn_trow = nullptr;    // [n_rownodes] thermo row
  uint16_t* pos_st = nullptr;    // [n_inc][npe] position of node b's thermo column in the k_ST rows
  uint16_t* pos_ts = nullptr;    // [n_inc][npe] position of node b's displacement triple in the k_TS row
  uint16_t* pos_tt = nullptr;    // [n_inc][npe] position of node b's thermo column in the k_TT row
  int64_t* rowptr_st = nullptr;
  int64_t* rowptr_ts = nullptr;
  int64_t* rowptr_tt = nullptr;
  double* tables = nullptr;      // dN at GPs [npe][npe][3] | N at GPs [npe][npe] | dN at nodes | w
  double* scratch = nullptr;     // [n_inc][tsi_rec(npe)]
  int32_t* err = nullptr;        // [2]
  // node-consistent numbering verified at create (thermo LID = structural LID / 3, the three block
  // graphs expansions of the k_TT node graph): what the block operator and its solve need, with
  // the k_TT graph on the device.  fusable = node_consistent && hex8 (fcg_tsi_evaluate_fused);
  // fused_with / solve_with: the structural context last verified against, for either use
  bool node_consistent = false;
  bool fusable = false;
  double lambda = 0, mu = 0;
  int32_t* col_tt = nullptr;
  const void* fused_with = nullptr;
  const void* solve_with = nullptr;
  // fcg_tsi_gmres_solve's work space (fcg_tsi_solve.hip), allocated on the first solve
  double* krylov_work = nullptr;
  int64_t krylov_doubles = 0;
  // the transient thermal field (fcg_thermo.hip).  cols_tt: the k_TT columns of any context (col_tt
  // itself when that is kept, else a copy of its own); max_row_tt: the longest k_TT row.  The
  // capacity kernel's plan, uploaded at create with the other tables: the column element and the
  // local node of every incidence.  ele_capa: the staging buffer of a per-element capacity table,
  // allocated by the first fcg_tsi_capacity that is given one
  int32_t* cols_tt = nullptr;
  int max_row_tt = 0;
  int32_t* inc_ele = nullptr;    // [n_inc]
  uint8_t* inc_loc = nullptr;    // [n_inc]
  double* ele_capa = nullptr;    // [n_ele]
};

}  // namespace fcg

struct fcg_tsi_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  fcg::TsiDevice d;
  std::string last_error;
  int64_t device_bytes = 0;
  // host copies of the descriptor's thermo maps [n_node], for the plans made after create
  // (fcg_tsi_surface_create, fcg_tsi_surface.hip)
  std::vector<int32_t> h_dof_col_t, h_dof_row_t;
};

// the thermo context a scalar AMG handle was created on (fcg_samg.hip)
struct fcg_samg;
extern "C" const fcg_tsi_ctx* fcg_samg_context(const fcg_samg* h);
