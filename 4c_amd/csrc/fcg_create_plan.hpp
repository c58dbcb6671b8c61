// fcg_create_plan.hpp -- the host side of fcg_create: descriptor checks, node rows, the choice of
// the assembly path and each path's plan tables, as plain structs of vectors.  Pure host index
// arithmetic (no HIP): fcg_context.cpp runs the stages in order and uploads what they fill;
// tests/cxx/create_plan_check.cpp checks the tables against the connectivity on a CPU.
//
// A stage that can refuse its input returns an fcg_status and the message in `why`.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "fourc_gpu.h"

namespace fcg {

// One record per (tile, node plane): row0[16] | rowlen[16] | rbase[16] (int64) | npos[16][27]
// (uint16, column position of lattice neighbour t inside the node's rows, 0xFFFF = absent).
constexpr int PLANE_REC_WORDS = 288;
// Compact record of a regular (tile, node plane), see StructHost::reg_rec.
constexpr int REG_REC_WORDS = 16;

namespace create {

template <class F>
void parallel_for(int64_t n, F f)
{
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < 4096) nt = 1;
  std::vector<std::thread> th;
  std::atomic<int64_t> next{0};
  const int64_t chunk = 1024;
  auto body = [&]() {
    for (;;)
    {
      const int64_t s = next.fetch_add(chunk);
      if (s >= n) break;
      const int64_t e = std::min(n, s + chunk);
      for (int64_t i = s; i < e; ++i) f(i);
    }
  };
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(body);
  body();
  for (auto& t : th) t.join();
}

extern const int kOff8[8][3];  // hex8 4C node order

uint64_t morton_key(const double* x, const double* lo, const double* hi);
std::vector<int64_t> morton_order(const std::vector<uint64_t>& key);

// --- descriptor checks: everything fcg_create refuses before it looks at the graph, in order
int check_descriptor(const fcg_desc* d, std::string& why);

// the column LIDs the matrix graph is written in
inline const int32_t* kcol_of(const fcg_desc* d) { return d->node_dof_kcol ? d->node_dof_kcol : d->node_dof_col; }

// --- node rows: the owned nodes ascending by row LID, each with 3 consecutive rows of one pattern
struct NodeRows {
  std::vector<int32_t> rownodes;    // [nrn] column node of each row node
  std::vector<int32_t> rn_of_node;  // [n_node] row node of a column node, -1 = not owned
  std::vector<int32_t> row0;        // [nrn] first row LID
  int32_t max_rowlen = 0;
  bool triple_rows = true;  // every node row is made of DOF triples (c, c+1, c+2) only
  // operator support (build_operator_support)
  std::vector<int64_t> diag;  // [n_rows] position of the diagonal entry in K values, -1 = none
  bool rowcol = false;        // owned column triple == row triple (DeviceMesh::owned_cols_first)
  bool square_local = false;  // ... and the column map is the row map (single rank)
  bool owned_cols_first = false;
  int64_t nrn() const { return int64_t(rownodes.size()); }
};
int build_node_rows(const fcg_desc* d, NodeRows& N, std::string& why);
// column LIDs' diagonal positions and whether the matrix column map is the row map; no error exit
void build_operator_support(const fcg_desc* d, NodeRows& N);

// Structured plan (hex8 row-block sweep kernel).  Verifies the lattice hint against the connectivity:
// every element node must sit at lattice position ijk(e) + offset(a) consistently across
// elements, no two elements/nodes may share a position, and every owned node row must hold
// exactly the DOF triples of its existing lattice neighbours.
struct StructHost {
  int32_t lo[3] = {0, 0, 0}, n[3] = {0, 0, 0};    // owned-node box
  int32_t elo[3] = {0, 0, 0}, en[3] = {0, 0, 0};  // column-element box
  int32_t tiles_x = 0, tiles_y = 0, tiles_z = 0, seg = 0;
  std::vector<int32_t> elem_at, rownode_at;
  std::vector<uint16_t> nbr_pos;
  std::vector<double> lat_x;        // node coordinates on the column-node lattice
  std::vector<int32_t> lat_dof;     // column LID of the node's first DOF, -1 = none
  std::vector<uint32_t> plane_rec;  // [tiles_y][tiles_x][NK][PLANE_REC_WORDS]
  // Regular lattice tiles (classify_regular_tiles): a (tile, node plane) whose 16 columns are
  // owned rows of 81 entries with the context's one neighbour-position pattern reg_pos, row0
  // advancing by 3 and base by 243 along each of the tile's four y-rows.  Its compact record:
  // row0 of the four y-rows [4] | their bases [4] (int64) | 1.  A plane that is not regular has
  // an all-zero compact record.
  std::vector<uint32_t> reg_rec;    // [tiles_y][tiles_x][NK][REG_REC_WORDS]
  // per tile the longest run [lo, hi) of node planes (relative to the owned box) whose layers
  // lo .. hi-2 are regular: planes L and L+1 regular and all 25 elements of the layer present
  std::vector<int32_t> reg_tile;    // [tiles_y][tiles_x][2]
  int32_t reg_pos[27] = {};         // the pattern (all zero when no row has 27 neighbours)
  // (tile, layer) pairs the sweep's workgroups run: all, and those inside their tile's run and
  // their segment's write range
  int64_t reg_layers = 0, layers_total = 0;
};
// fills the reg_* members from the plan's tables (pure index arithmetic)
void classify_regular_tiles(StructHost& P);
bool detect_lattice_hex8(const fcg_desc* d, std::vector<int32_t>& ijk, std::vector<int32_t>& canon,
    std::string& why);
bool build_structured_plan(const fcg_desc* d, const std::vector<int32_t>& rownodes,
    const std::vector<int32_t>& row0, const int32_t* kcol, int cus, StructHost& P, std::string& why);

// Colour-ordered direct assembly plan (hex27 on a verified lattice), see build_colored_plan
struct ColorHost {
  std::vector<int32_t> col_ele;
  std::vector<uint8_t> ft;
  int64_t color_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // pencil order (hex27 StVK, fcg_hex27.hip): colour (ey & 1) + 2 (ez & 1); inside a colour the
  // maximal runs of lattice-consecutive elements along x ("pencils"), each walked in x order by
  // one workgroup.  pen_ele: elements by colour, pencil, ex; pen_ptr: pencil ranges in pen_ele;
  // pen_color: pencil range of colour c.  nb[e]: bit (dx+1) + 3 (dy+1) + 9 (dz+1) = lattice
  // neighbour e + (dx, dy, dz) exists; bits 27, 28 = ey & 1, ez & 1.
  std::vector<int32_t> pen_ele;
  std::vector<int64_t> pen_ptr;
  int64_t pen_color[5] = {0, 0, 0, 0, 0};
  std::vector<uint32_t> nb;
};
bool build_colored_plan(const fcg_desc* d, ColorHost& P, std::string& why);

// --- path choice: structured (hex8 sweep), coloured (hex27 lattice), gather (hex8 node rows) or,
// with all three false, general.  `cus`: compute units of the target device.
struct PathChoice {
  bool structured = false, colored = false, gather = false;
  StructHost sp;
  ColorHost cp;
  int path() const
  {
    return structured ? FCG_PATH_STRUCTURED : colored ? FCG_PATH_COLORED : gather ? FCG_PATH_GATHER : FCG_PATH_GENERAL;
  }
};
int choose_path(const fcg_desc* d, const NodeRows& N, int cus, PathChoice& P, std::string& why);

// --- incidences = (column element e, local node a) with node a owned, grouped by the owned node
// and ordered by element index inside a node; empty on the structured path
struct Incidences {
  int64_t n_inc = 0;
  std::vector<int64_t> inc_ptr;   // [nrn + 1]
  std::vector<int32_t> inc_of;    // [n_ele][npe] incidence id or -1
  std::vector<int32_t> inc_ele;   // [n_inc]
  std::vector<uint8_t> inc_a;     // [n_inc]
  std::vector<int32_t> inc_row0;  // [n_inc] (coloured path only)
  std::vector<uint16_t> inc_pos;  // [n_inc][npe] column position of node b's triple in the row
};
int build_incidences(const fcg_desc* d, const NodeRows& N, const PathChoice& P, Incidences& I,
    std::string& why);
// the stride fast path's positions; then the gather path gives way to the general one when a
// row holds columns that are not node DOF triples (an error when the gather path was requested)
int build_incidence_positions(const fcg_desc* d, const NodeRows& N, PathChoice& P, Incidences& I,
    std::string& why);

// Morton order of the row nodes' coordinates in the bounding box of all column nodes (gather
// records, hex27 assembly order).  `lo` / `hi` (optional) return that box.
std::vector<int64_t> rownode_morton_order(const fcg_desc* d, const NodeRows& N, double* lo = nullptr,
    double* hi = nullptr);

// --- node-row gather plan (hex8): records of <= 8 incidences per row node, see build_gather_plan
struct GatherHost {
  int64_t n_rec = 0, n_single = 0;
  std::vector<int64_t> multi_ptr;  // [n_multi + 1] record range of each node with > 8 elements
  std::vector<int32_t> rec_row0, rec_meta, rec_ele;
  std::vector<int64_t> rec_base;
  std::vector<uint8_t> rec_a;
  std::vector<uint32_t> rec_tmap;
  std::vector<int32_t> eorig, edof;  // storage slot -> element; [n_ele][8] first DOF column LIDs
  std::vector<double> ex;            // [n_ele][8][3] node coordinates in storage-slot order
  std::vector<double> gauss;         // [8][4] xi, eta, zeta, weight of the hex8 stiffness rule
};
void build_gather_plan(const fcg_desc* d, const NodeRows& N, const Incidences& I, GatherHost& G);

// hex27 slab schedule (DeviceMesh::h27_*), see build_h27_ring
struct H27Ring {
  int64_t nslab = 0, ring = 0;
  std::vector<int64_t> asm_ptr;
  std::vector<int32_t> rows, rslot0, slot;
};
void build_h27_ring(int64_t n_ele, int64_t S, int lag, const std::vector<int64_t>& inc_ptr,
    const std::vector<int32_t>& inc_ele, const std::vector<uint8_t>& inc_a,
    const std::vector<int64_t>& morton, H27Ring& R);

// Elements per slab of the hex27 slab schedule (0 = one slab) and the element workgroups per
// launch.  slab_env / el_grid_env: the values of FCG_H27_SLAB / FCG_H27_EL_GRID or NULL;
// mem_free < 0: unknown, mem_total stands in.
struct H27Schedule {
  int64_t slab = 0;
  int el_grid = 512;
};
H27Schedule h27_schedule(int64_t n_ele, int64_t n_inc, int64_t nnz, int64_t record_bytes,
    int64_t mem_free, int64_t mem_total, int cus, const char* slab_env, const char* el_grid_env);

}  // namespace create
}  // namespace fcg
