// fcg_tsi_surface_plan.hpp -- the host side of fcg_tsi_surface_create: the checks of the face list,
// the surface rows (owned nodes on a face), their incidences, the compact rows with their positions
// in the k_TT value array, and the quad4 / quad9 shape tables, as plain structs of vectors.  Pure
// host index arithmetic (no HIP): fcg_tsi_surface.hip runs the stages in order and uploads what
// they fill; tests/cxx/tsi_surface_plan_check.cpp checks the tables against the faces on a CPU.
//
// A stage that can refuse its input returns an fcg_status and the message in `why`.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fourc_gpu.h"

namespace fcg {
namespace tsi_surface_plan {

// what the plan reads of a TSI descriptor: the thermo maps of the column nodes and the k_TT graph
struct Maps {
  int32_t celltype = FCG_HEX8;
  int64_t n_node = 0, n_rows_t = 0, n_cols_t = 0;
  const int32_t* node_dof_col_t = nullptr;
  const int32_t* node_dof_row_t = nullptr;
  const int64_t* rowptr_tt = nullptr;
  const int32_t* col_tt = nullptr;
};
inline Maps maps_of(const fcg_tsi_desc* d)
{
  Maps m;
  m.celltype = d->celltype;
  m.n_node = d->n_node;
  m.n_rows_t = d->n_rows_t;
  m.n_cols_t = d->n_cols_t;
  m.node_dof_col_t = d->node_dof_col_t;
  m.node_dof_row_t = d->node_dof_row_t;
  m.rowptr_tt = d->rowptr_tt;
  m.col_tt = d->col_tt;
  return m;
}

// nodes of a face = Gauss points of its rule: quad4 with 2x2, quad9 with 3x3
inline int nfn_of(int32_t celltype) { return celltype == FCG_HEX27 ? 9 : 4; }
// the longest compact row the setup kernel's LDS row image holds: a compact row is part of a k_TT row
inline int max_compact_row(int32_t celltype) { return celltype == FCG_HEX27 ? 125 : 27; }

// --- face checks: n_faces >= 0, every node id in [0, n_node), no node twice in a face
int check_faces(const Maps& M, int64_t n_faces, const int32_t* face_nodes, std::string& why);

struct Plan {
  int nfn = 4;
  int64_t n_faces = 0;
  // surface rows: the owned nodes that lie on a face, ascending by thermo row
  std::vector<int32_t> s_row;     // [nsr] thermo row
  // incidences = (face f, local node a) with node a owned, grouped by surface row, faces ascending
  std::vector<int64_t> inc_ptr;   // [nsr + 1]
  std::vector<int32_t> inc_face;  // [n_inc]
  std::vector<uint8_t> inc_loc;   // [n_inc]
  // compact rows: per surface row the thermo columns of its incident faces' nodes, ascending
  std::vector<int64_t> s_ptr;     // [nsr + 1]
  std::vector<int32_t> s_col;     // [nse] thermo column
  std::vector<int64_t> s_pos;     // [nse] position of the entry in the k_TT value array
  std::vector<uint16_t> slot;     // [n_inc][nfn] place of face node b in the compact row
  int max_row = 0;                // the longest compact row
  int64_t nsr() const { return int64_t(s_row.size()); }
  int64_t n_inc() const { return int64_t(inc_face.size()); }
  int64_t nse() const { return int64_t(s_col.size()); }
};
int build_rows(const Maps& M, int64_t n_faces, const int32_t* face_nodes, Plan& P, std::string& why);
int build_compact_rows(const Maps& M, const int32_t* face_nodes, Plan& P, std::string& why);

// --- tables: N at GPs [ngp][nfn] | dN/dr [ngp][nfn] | dN/ds [ngp][nfn] | w [ngp], ngp = nfn
std::vector<double> build_tables(int nfn);

}  // namespace tsi_surface_plan
}  // namespace fcg
