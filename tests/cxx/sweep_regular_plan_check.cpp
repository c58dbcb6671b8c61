// sweep_regular_plan_check -- the regular-tile classifier of the structured plan
// (4c_amd/csrc/fcg_create_plan.cpp, classify_regular_tiles), on a CPU through the host plan stage:
// the number of regular (tile, layer) pairs of a box equals the count derived here from the tile
// geometry; every plane flagged regular reproduces its full record's row0, len, base and npos
// from the compact record and the position pattern; a small box, a box with a hole and a two-rank
// split classify as their geometry says.  Links the plan unit and the box-mesh builder only (no
// libfourc_gpu, no ROCm).  Prints PASS, or the failed condition (exit 1).  TEST INFRASTRUCTURE.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fcg_create_plan.hpp"
#include "fourc_gpu.h"

namespace plan = fcg::create;

namespace {

const char* g_mesh = "";

#define CHECK(cond)                                                                  \
  do                                                                                 \
  {                                                                                  \
    if (!(cond))                                                                     \
    {                                                                                \
      std::printf("FAIL [%s] %s (line %d)\n", g_mesh, #cond, __LINE__);              \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

// a descriptor that owns its arrays
struct Mesh {
  fcg_desc d;
  std::vector<int32_t> ele_nodes, dof_col, dof_row, col_lid, ijk;
  std::vector<double> x;
  std::vector<int64_t> rowptr;
  void point()
  {
    d.n_ele = int64_t(ele_nodes.size()) / 8;
    d.n_node = int64_t(dof_col.size());
    d.n_rows = int64_t(rowptr.size()) - 1;
    d.ele_nodes = ele_nodes.data();
    d.ele_gid = nullptr;
    d.node_x = x.data();
    d.node_dof_col = dof_col.data();
    d.node_dof_row = dof_row.data();
    d.rowptr = rowptr.data();
    d.col_lid = col_lid.data();
    d.ele_ijk = ijk.empty() ? nullptr : ijk.data();
  }
};

// the box without its elements at the lattice positions in `holes`; the graph is rebuilt from
// the remaining elements (sorted rows, DOF triples) over the box's own DOF numbering
Mesh box(int nx, int ny, int nz, int rank, int nranks, const std::vector<std::vector<int>>& holes = {})
{
  fcg_box b{};
  b.celltype = FCG_HEX8;
  b.interval[0] = nx; b.interval[1] = ny; b.interval[2] = nz;
  for (int k = 0; k < 3; ++k) b.upper[k] = 1.0;
  b.jitter = 0.1;
  b.jitter_seed = 20251015;
  fcg_box_mesh* bm = nullptr;
  CHECK(fcg_box_mesh_create_ex(&b, rank, nranks, FCG_BOX_GHOSTED, &bm) == FCG_OK);
  Mesh m;
  CHECK(fcg_box_mesh_desc(bm, FCG_LINEAR, 10.0, 0.25, 0, &m.d) == FCG_OK);
  const fcg_desc& s = m.d;
  CHECK(s.ele_ijk != nullptr);
  m.x.assign(s.node_x, s.node_x + 3 * s.n_node);
  m.dof_col.assign(s.node_dof_col, s.node_dof_col + s.n_node);
  m.dof_row.assign(s.node_dof_row, s.node_dof_row + s.n_node);
  if (holes.empty())
  {
    m.ele_nodes.assign(s.ele_nodes, s.ele_nodes + s.n_ele * 8);
    m.ijk.assign(s.ele_ijk, s.ele_ijk + 3 * s.n_ele);
    m.rowptr.assign(s.rowptr, s.rowptr + s.n_rows + 1);
    m.col_lid.assign(s.col_lid, s.col_lid + s.rowptr[s.n_rows]);
  }
  else
  {
    CHECK(nranks == 1);
    std::vector<std::vector<int32_t>> cols(s.n_rows);
    for (int64_t e = 0; e < s.n_ele; ++e)
    {
      bool hole = false;
      for (const auto& h : holes)
        hole = hole || (s.ele_ijk[3 * e] == h[0] && s.ele_ijk[3 * e + 1] == h[1] && s.ele_ijk[3 * e + 2] == h[2]);
      if (hole) continue;
      m.ele_nodes.insert(m.ele_nodes.end(), s.ele_nodes + 8 * e, s.ele_nodes + 8 * e + 8);
      m.ijk.insert(m.ijk.end(), s.ele_ijk + 3 * e, s.ele_ijk + 3 * e + 3);
      for (int a = 0; a < 8; ++a)
      {
        const int32_t ra = s.node_dof_row[s.ele_nodes[8 * e + a]];
        if (ra < 0) continue;
        for (int bb = 0; bb < 8; ++bb)
          for (int q = 0; q < 3; ++q) cols[ra].push_back(s.node_dof_col[s.ele_nodes[8 * e + bb]] + q);
      }
    }
    m.rowptr.assign(1, 0);
    for (int64_t n = 0; n < s.n_node; ++n)
    {
      const int32_t r = s.node_dof_row[n];
      if (r < 0) continue;
      std::sort(cols[r].begin(), cols[r].end());
      cols[r].erase(std::unique(cols[r].begin(), cols[r].end()), cols[r].end());
      cols[r + 1] = cols[r + 2] = cols[r];
    }
    for (int64_t r = 0; r < s.n_rows; ++r)
    {
      m.col_lid.insert(m.col_lid.end(), cols[r].begin(), cols[r].end());
      m.rowptr.push_back(int64_t(m.col_lid.size()));
    }
  }
  m.point();
  fcg_box_mesh_destroy(bm);
  return m;
}

plan::StructHost planned(Mesh& m, int cus)
{
  m.d.material = FCG_MAT_STVK;
  m.d.kinematics = FCG_LINEAR;
  m.d.path = FCG_PATH_STRUCTURED;
  std::string why;
  plan::NodeRows rows;
  plan::PathChoice choice;
  CHECK(plan::check_descriptor(&m.d, why) == FCG_OK);
  CHECK(plan::build_node_rows(&m.d, rows, why) == FCG_OK);
  CHECK(plan::choose_path(&m.d, rows, cus, choice, why) == FCG_OK);
  CHECK(choice.structured);
  return choice.sp;
}

// every plane flagged regular: the full record from the compact one; every run inside the flags
void check_records(const plan::StructHost& P)
{
  const int64_t NK = P.n[2], W = fcg::PLANE_REC_WORDS, CW = fcg::REG_REC_WORDS;
  const int64_t ntile = int64_t(P.tiles_x) * P.tiles_y;
  CHECK(int64_t(P.reg_rec.size()) == ntile * NK * CW && int64_t(P.reg_tile.size()) == 2 * ntile);
  int64_t layers = 0, total = 0;
  for (int64_t t = 0; t < ntile; ++t)
  {
    for (int64_t k = 0; k < NK; ++k)
    {
      const uint32_t* cr = P.reg_rec.data() + (t * NK + k) * CW;
      const uint32_t* rec = P.plane_rec.data() + (t * NK + k) * W;
      const uint16_t* np = reinterpret_cast<const uint16_t*>(rec + 64);
      if (cr[12] == 0u)
      {
        for (int i = 0; i < CW; ++i) CHECK(cr[i] == 0u);
        continue;
      }
      CHECK(cr[12] == 1u);
      for (int c = 0; c < 16; ++c)
      {
        const int cx = c % 4, cy = c / 4;
        const int64_t base = int64_t(uint64_t(cr[4 + 2 * cy]) | (uint64_t(cr[4 + 2 * cy + 1]) << 32)) + 243 * cx;
        CHECK(rec[c] == cr[cy] + 3u * cx);
        CHECK(rec[16 + c] == 81u);
        CHECK(int64_t(uint64_t(rec[32 + 2 * c]) | (uint64_t(rec[32 + 2 * c + 1]) << 32)) == base);
        for (int q = 0; q < 27; ++q) CHECK(int32_t(np[27 * c + q]) == P.reg_pos[q]);
      }
    }
    const int64_t lo = P.reg_tile[2 * t], hi = P.reg_tile[2 * t + 1];
    CHECK(lo >= 0 && hi <= NK && (hi == lo || hi >= lo + 2));
    for (int64_t k = lo; k < hi; ++k) CHECK(P.reg_rec[(t * NK + k) * CW + 12] == 1u);
    for (int64_t tz = 0; tz < P.tiles_z; ++tz)
    {
      const int64_t kz0 = int64_t(P.seg) * tz, kz1 = std::min<int64_t>(kz0 + P.seg, NK);
      total += kz1 - kz0 + 1;
      layers += std::max<int64_t>(0, std::min(hi, kz1) - 1 - std::max(lo, kz0));
    }
  }
  CHECK(layers == P.reg_layers && total == P.layers_total);
  std::printf("%s: %d x %d tiles, %d segments of %d planes, %lld of %lld (tile, layer) pairs regular\n", g_mesh,
      P.tiles_x, P.tiles_y, P.tiles_z, P.seg, (long long)P.reg_layers, (long long)P.layers_total);
}

// The count from the geometry of a single-rank nx x ny x nz box: a node has 27 neighbours when it
// is interior in x, y and z; a tile (4 x 4 nodes from 4 tx, 4 ty) is regular on the interior
// planes 1 .. nz - 1 when its 16 columns are interior in x and y; workgroup tz writes the planes
// [seg tz, seg (tz + 1)) and a layer L is regular when planes L and L + 1 are regular and written.
int64_t box_count(int nx, int ny, int nz, const plan::StructHost& P)
{
  int64_t tiles = 0;
  for (int ty = 0; ty < P.tiles_y; ++ty)
    for (int tx = 0; tx < P.tiles_x; ++tx)
      if (4 * tx >= 1 && 4 * tx + 3 <= nx - 1 && 4 * ty >= 1 && 4 * ty + 3 <= ny - 1) ++tiles;
  int64_t layers = 0;
  for (int tz = 0; tz < P.tiles_z; ++tz)
    for (int L = P.seg * tz; L + 1 < std::min(P.seg * (tz + 1), nz + 1); ++L)
      if (L >= 1 && L + 1 <= nz - 1) ++layers;
  return tiles * layers;
}

}  // namespace

int main()
{
  for (int cus : {256, 8})  // one z-segment and several
  {
    g_mesh = "box 38x37x11";
    Mesh m = box(38, 37, 11, 0, 1);
    const plan::StructHost P = planned(m, cus);
    CHECK(P.tiles_x == 10 && P.tiles_y == 10);
    check_records(P);
    CHECK(P.reg_layers > 0 && P.reg_layers == box_count(38, 37, 11, P));
    CHECK(P.layers_total == int64_t(100) * (12 + P.tiles_z));
    // GridGenerator numbering: the 27 neighbours' triples in lattice order
    for (int t = 0; t < 27; ++t) CHECK(P.reg_pos[t] == 3 * t);
  }
  {
    g_mesh = "box 6x5x4";
    Mesh m = box(6, 5, 4, 0, 1);
    const plan::StructHost P = planned(m, 256);
    check_records(P);
    CHECK(P.reg_layers == 0 && P.reg_layers == box_count(6, 5, 4, P));
  }
  {
    // element (18, 17, 5) missing: its 8 corner nodes lose a neighbour, so the tiles holding them
    // (nodes 18..19 x 17..18: tiles (4, 4)) keep a shorter run, every other tile its own
    g_mesh = "box 38x37x11 with a hole";
    Mesh m = box(38, 37, 11, 0, 1, {{18, 17, 5}});
    Mesh full = box(38, 37, 11, 0, 1);
    const plan::StructHost P = planned(m, 256), F = planned(full, 256);
    check_records(P);
    CHECK(P.reg_layers > 0 && P.reg_layers < F.reg_layers);
    const int64_t NK = P.n[2];
    for (int64_t t = 0; t < int64_t(P.tiles_x) * P.tiles_y; ++t)
    {
      const bool holed = t == 4 * P.tiles_x + 4;
      for (int64_t k = 0; k < NK; ++k)
      {
        const bool lost = holed && (k == 5 || k == 6);
        CHECK(P.reg_rec[(t * NK + k) * fcg::REG_REC_WORDS + 12] ==
              (lost ? 0u : F.reg_rec[(t * NK + k) * fcg::REG_REC_WORDS + 12]));
      }
      if (!holed) CHECK(P.reg_tile[2 * t] == F.reg_tile[2 * t] && P.reg_tile[2 * t + 1] == F.reg_tile[2 * t + 1]);
    }
    // planes 1..4 and 7..10 stay regular around the hole: the longer run wins (the first of equals)
    CHECK(P.reg_tile[2 * (4 * P.tiles_x + 4)] == 1 && P.reg_tile[2 * (4 * P.tiles_x + 4) + 1] == 5);
  }
  for (int r = 0; r < 2; ++r)
  {
    g_mesh = r ? "box 38x37x11 rank 1 of 2" : "box 38x37x11 rank 0 of 2";
    Mesh m = box(38, 37, 11, r, 2);
    const plan::StructHost P = planned(m, 256);
    check_records(P);
  }
  std::printf("PASS\n");
  return 0;
}
