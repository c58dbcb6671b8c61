// fcg_tsi_plan.hpp -- the host side of fcg_tsi_create: descriptor checks, the owned-node rows, the
// layout check of the three block graphs, incidences and column positions, the shape tables, the
// node-consistency classification and the material constants, as plain structs of vectors.  Pure
// host index arithmetic (no HIP): fcg_tsi.hip runs the stages in order and uploads what they fill;
// tests/cxx/tsi_plan_check.cpp checks the tables against the connectivity on a CPU.
//
// A stage that can refuse its input returns an fcg_status and the message in `why`.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fourc_gpu.h"

namespace fcg {
namespace tsi_plan {

inline int npe_of(const fcg_tsi_desc* d) { return d->celltype == FCG_HEX27 ? 27 : 8; }
// node neighbours of a row: the longest k_TT row the assembly's LDS row image holds
inline int max_neighbours(const fcg_tsi_desc* d) { return d->celltype == FCG_HEX27 ? 125 : 27; }

// --- descriptor checks: everything fcg_tsi_create refuses before it looks at the maps, in order
int check_descriptor(const fcg_tsi_desc* d, std::string& why);

// --- node rows: the owned nodes ascending by structural row; the structural rows and the thermo
// row of a node are owned together
struct NodeRows {
  std::vector<int32_t> rownodes;    // [nrn] column node of each row node
  std::vector<int32_t> rn_of_node;  // [n_node] row node of a column node, -1 = not owned
  std::vector<int32_t> srow;        // [nrn] first structural row
  std::vector<int32_t> trow;        // [nrn] thermo row
  int64_t nrn() const { return int64_t(rownodes.size()); }
};
int build_node_rows(const fcg_tsi_desc* d, NodeRows& N, std::string& why);

// --- the 3 k_ST rows of a node share one list of at most max_neighbours thermo columns; its k_TS
// and k_TT rows fit the row image
int check_row_layout(const fcg_tsi_desc* d, const NodeRows& N, std::string& why);

// --- incidences = (column element e, local node a) with node a owned, grouped by the owned node
// and ordered by element index inside a node
struct Incidences {
  int64_t n_inc = 0;
  std::vector<int64_t> inc_ptr;  // [nrn + 1]
  std::vector<int32_t> inc_of;   // [n_ele][npe] incidence id or -1
  std::vector<int32_t> inc_ele;  // [n_inc] column element
  std::vector<uint8_t> inc_loc;  // [n_inc] local node
  // [n_inc][npe] position of node b's thermo column in the k_ST rows, of its displacement triple in
  // the k_TS row, of its thermo column in the k_TT row (build_positions)
  std::vector<uint16_t> pos_st, pos_ts, pos_tt;
};
int build_incidences(const fcg_tsi_desc* d, const NodeRows& N, Incidences& I, std::string& why);
int build_positions(const fcg_tsi_desc* d, const NodeRows& N, Incidences& I, std::string& why);

// --- tables: dN at GPs [npe][npe][3] | N at GPs [npe][npe] | dN at nodes [npe][npe][3] | w [npe]
std::vector<double> build_tables(int32_t celltype);

// --- node-consistent numbering (what the block operator, its solve and fcg_tsi_evaluate_fused
// require): thermo DOF LIDs are the structural ones / 3 and the three block graphs are expansions
// of one node graph (the k_TT graph).  No error exit
bool node_consistent(const fcg_tsi_desc* d);
int max_row_tt(const fcg_tsi_desc* d);

// --- material constants, entry counts and the element GIDs of a descriptor without them
struct Constants {
  double m = 0, lambda = 0, mu = 0;  // st_modulus and the Lame constants
  int64_t nnz_st = 0, nnz_ts = 0, nnz_tt = 0;
  std::vector<int32_t> ele_gid;      // [n_ele] 0, 1, ... when the descriptor has none, else empty
};
Constants build_constants(const fcg_tsi_desc* d);

}  // namespace tsi_plan
}  // namespace fcg
