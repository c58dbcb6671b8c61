// fcg_create_plan.cpp -- the assembly plan of fcg_create (this path's FillComplete), host only:
// fcg_context.cpp runs these stages and uploads their tables.
//
// Plan built once per pattern (the reference rebuilds nothing either: the stiffness keeps
// its graph, `savegraph=true`, 4C_structure_new_timint_basedataglobalstate.cpp:650-652):
//   * incidences = (column element e, local node a) with node a owned by this rank, grouped by
//     the owned node (ascending row LID) and ordered by element index inside a node -- the order
//     in which the assembly kernel sums, hence bitwise-reproducible results;
//   * for every incidence and every local node b of the element, the position of b's first DOF
//     column inside the row of a -- the stride-3 fast path of SparseMatrix::assemble
//     (4C_linalg_sparsematrix.cpp:497-543) resolved once on the host instead of by a
//     lower_bound per element and row at every Newton iteration.
#include "fcg_create_plan.hpp"

#include <array>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "fcg_shape.hpp"

namespace fcg {
namespace create {

const int kOff8[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1},
    {0, 1, 1}};  // hex8 4C node order (4C_io_gridgenerator.cpp:371-379)

// Morton (Z-order) key of a point of the box [lo, hi]: 21 bits per axis, interleaved.  Sorting by
// it puts points that are close in space close in the order (gather plan).
uint64_t morton_key(const double* x, const double* lo, const double* hi)
{
  uint64_t key = 0;
  uint32_t q[3];
  for (int k = 0; k < 3; ++k)
  {
    const double ext = hi[k] - lo[k];
    const double t = ext > 0 ? (x[k] - lo[k]) / ext : 0.0;
    q[k] = uint32_t(std::min(2097151.0, std::max(0.0, t * 2097151.0)));
  }
  for (int b = 20; b >= 0; --b)
    for (int k = 0; k < 3; ++k) key = (key << 1) | ((q[k] >> b) & 1u);
  return key;
}

// Permutation sorting items by their Morton keys (ties by index: deterministic)
std::vector<int64_t> morton_order(const std::vector<uint64_t>& key)
{
  std::vector<int64_t> ord(key.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = int64_t(i);
  std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
    return key[a] != key[b] ? key[a] < key[b] : a < b;
  });
  return ord;
}

// Lattice positions (ex, ey, ez) of a hex8 mesh whose elements stack like a GridGenerator box,
// found from the connectivity alone (an input-file mesh without the fcg_desc.ele_ijk hint), with
// every element's own local numbering allowed to be any proper rotation of 4C's (mesh generators
// rotate element frames): element 0's local frame fixes the lattice axes; across every shared face
// (matched by sorting the sorted node quadruples) the neighbour's other four nodes sit one step
// along the face normal from their edge partners on the face; then every element must occupy one
// unit cell, with a right-handed local frame.  Returns the cells and the connectivity in 4C's
// local order for those cells (canon, what the row-block sweep reads); false (and why) otherwise
// -- build_structured_plan verifies the result like a given hint.
bool detect_lattice_hex8(const fcg_desc* d, std::vector<int32_t>& ijk, std::vector<int32_t>& canon,
    std::string& why)
{
  const int64_t n = d->n_ele;
  if (d->celltype != FCG_HEX8 || n == 0 || n >= (int64_t(1) << 31) / 6)
  {
    why = "not a hex8 mesh";
    return false;
  }
  // local faces (4C hex8 order) and, per local node, its three edge partners
  static const int kFace[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {3, 2, 6, 7},
      {0, 3, 7, 4}, {1, 2, 6, 5}};
  int partner[8][3];
  for (int u = 0; u < 8; ++u)
  {
    int c = 0;
    for (int v = 0; v < 8; ++v)
    {
      int diff = 0;
      for (int k = 0; k < 3; ++k) diff += kOff8[u][k] != kOff8[v][k];
      if (diff == 1) partner[u][c++] = v;
    }
  }
  // faces as sorted node quadruples, bucketed by their smallest node (a counting sort: at most 12
  // faces of a hex8 mesh start at one node), matched inside each bucket
  std::vector<std::array<int32_t, 4>> fv(6 * n);
  parallel_for(n, [&](int64_t e) {
    const int32_t* en = d->ele_nodes + 8 * e;
    for (int f = 0; f < 6; ++f)
    {
      std::array<int32_t, 4>& F = fv[6 * e + f];
      for (int k = 0; k < 4; ++k) F[k] = en[kFace[f][k]];
      std::sort(F.begin(), F.end());
    }
  });
  std::vector<int64_t> boff(d->n_node + 1, 0);
  for (int64_t i = 0; i < 6 * n; ++i) ++boff[fv[i][0] + 1];
  for (int64_t nd = 0; nd < d->n_node; ++nd) boff[nd + 1] += boff[nd];
  std::vector<int32_t> bface(6 * n);
  {
    std::vector<int64_t> fill(boff.begin(), boff.end() - 1);
    for (int64_t i = 0; i < 6 * n; ++i) bface[fill[fv[i][0]]++] = int32_t(i);
  }
  std::vector<int32_t> nbr(6 * n, -1);  // element across local face f of e
  std::atomic<int> shared3{0};
  parallel_for(d->n_node, [&](int64_t nd) {
    for (int64_t i = boff[nd]; i < boff[nd + 1]; ++i)
    {
      const int32_t fi = bface[i];
      int matches = 0;
      for (int64_t j = boff[nd]; j < boff[nd + 1]; ++j)
      {
        const int32_t fj = bface[j];
        if (fj != fi && fv[fj] == fv[fi])
        {
          ++matches;
          nbr[fi] = fj / 6;
        }
      }
      if (matches > 1) shared3 = 1;
    }
  });
  if (shared3)
  {
    why = "a face is shared by more than two elements";
    return false;
  }
  std::vector<std::array<int32_t, 4>>().swap(fv);

  // node positions spread from element 0 (its local frame = the lattice axes)
  const int64_t unset = INT64_MIN;
  std::vector<int64_t> pos(3 * int64_t(d->n_node), unset);
  auto set_pos = [&](int32_t node, const int64_t* p) -> bool {
    int64_t* q = &pos[3 * int64_t(node)];
    if (q[0] == unset)
    {
      q[0] = p[0];
      q[1] = p[1];
      q[2] = p[2];
      return true;
    }
    return q[0] == p[0] && q[1] == p[1] && q[2] == p[2];
  };
  std::vector<uint8_t> done(n, 0);
  {
    const int32_t* en = d->ele_nodes;
    for (int a = 0; a < 8; ++a)
    {
      const int64_t p[3] = {kOff8[a][0], kOff8[a][1], kOff8[a][2]};
      if (!set_pos(en[a], p))
      {
        why = "an element repeats a node";
        return false;
      }
    }
  }
  std::vector<int32_t> stack{0};
  done[0] = 1;
  int64_t seen = 1;
  while (!stack.empty())
  {
    const int32_t e = stack.back();
    stack.pop_back();
    const int32_t* en = d->ele_nodes + 8 * int64_t(e);
    for (int f = 0; f < 6; ++f)
    {
      const int32_t g = nbr[6 * int64_t(e) + f];
      if (g < 0) continue;
      // the face normal (out of e, into g): the coordinate the face's nodes share, away from
      // e's other nodes
      const int32_t* fn = en;
      int axis = -1;
      int64_t sgn = 0;
      const int64_t* p0 = &pos[3 * int64_t(fn[kFace[f][0]])];
      for (int k = 0; k < 3 && axis < 0; ++k)
      {
        bool same = true;
        for (int q = 1; q < 4; ++q) same = same && pos[3 * int64_t(fn[kFace[f][q]]) + k] == p0[k];
        if (same) axis = k;
      }
      if (axis < 0)
      {
        why = "an element is not a lattice cell";
        return false;
      }
      for (int a = 0; a < 8; ++a)
      {
        const int64_t c = pos[3 * int64_t(en[a]) + axis];
        if (c != p0[axis]) sgn = p0[axis] > c ? 1 : -1;
      }
      // g's nodes off the face: one step along the normal from their edge partner on the face
      const int32_t* gn = d->ele_nodes + 8 * int64_t(g);
      const int32_t sh[4] = {en[kFace[f][0]], en[kFace[f][1]], en[kFace[f][2]], en[kFace[f][3]]};
      auto on_face = [&](int32_t node) { return node == sh[0] || node == sh[1] || node == sh[2] || node == sh[3]; };
      int placed = 0;
      for (int u = 0; u < 8; ++u)
      {
        if (!on_face(gn[u])) continue;
        for (int j = 0; j < 3; ++j)
        {
          const int32_t m = gn[partner[u][j]];
          if (on_face(m)) continue;
          int64_t p[3] = {pos[3 * int64_t(gn[u])], pos[3 * int64_t(gn[u]) + 1], pos[3 * int64_t(gn[u]) + 2]};
          p[axis] += sgn;
          if (!set_pos(m, p))
          {
            why = "face neighbours give inconsistent lattice positions";
            return false;
          }
          ++placed;
        }
      }
      if (placed != 4)
      {
        why = "an element is not a lattice cell";
        return false;
      }
      if (!done[g])
      {
        done[g] = 1;
        stack.push_back(g);
        ++seen;
      }
    }
  }
  if (seen != n)
  {
    why = "the elements are not one face-connected block";
    return false;
  }
  // every element one unit cell with a right-handed local frame; cells and 4C-order connectivity
  int64_t mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX};
  for (int64_t nd = 0; nd < d->n_node; ++nd)
    if (pos[3 * nd] != unset)
      for (int k = 0; k < 3; ++k) mn[k] = std::min(mn[k], pos[3 * nd + k]);
  ijk.assign(3 * n, 0);
  canon.assign(8 * n, -1);
  std::atomic<int> bad{0};
  parallel_for(n, [&](int64_t e) {
    const int32_t* en = d->ele_nodes + 8 * e;
    int64_t c[3] = {INT64_MAX, INT64_MAX, INT64_MAX};
    for (int a = 0; a < 8; ++a)
      for (int k = 0; k < 3; ++k) c[k] = std::min(c[k], pos[3 * int64_t(en[a]) + k]);
    int32_t* out = &canon[8 * e];
    for (int a = 0; a < 8; ++a)
    {
      int off[3], slot = -1;
      for (int k = 0; k < 3; ++k) off[k] = int(pos[3 * int64_t(en[a]) + k] - c[k]);
      for (int b = 0; b < 8; ++b)
        if (off[0] == kOff8[b][0] && off[1] == kOff8[b][1] && off[2] == kOff8[b][2]) slot = b;
      if (slot < 0 || out[slot] != -1)
      {
        bad = 1;
        return;
      }
      out[slot] = en[a];
    }
    // handedness of the local frame: local x, y, z axes (nodes 1, 3, 4 from node 0)
    int64_t ax[3][3];
    const int idx[3] = {1, 3, 4};
    for (int q = 0; q < 3; ++q)
      for (int k = 0; k < 3; ++k) ax[q][k] = pos[3 * int64_t(en[idx[q]]) + k] - pos[3 * int64_t(en[0]) + k];
    const int64_t det = ax[0][0] * (ax[1][1] * ax[2][2] - ax[1][2] * ax[2][1]) -
                        ax[0][1] * (ax[1][0] * ax[2][2] - ax[1][2] * ax[2][0]) +
                        ax[0][2] * (ax[1][0] * ax[2][1] - ax[1][1] * ax[2][0]);
    if (det != 1)
    {
      bad = 2;
      return;
    }
    for (int k = 0; k < 3; ++k)
    {
      const int64_t v = c[k] - mn[k];
      if (v >= INT32_MAX)
      {
        bad = 1;
        return;
      }
      ijk[3 * e + k] = int32_t(v);
    }
  });
  if (bad != 0)
  {
    why = bad == 2 ? "an element's local frame is mirrored against the lattice"
                   : "an element is not a lattice cell";
    return false;
  }
  return true;  // uniqueness of positions and nodes: build_structured_plan's checks
}

bool build_structured_plan(const fcg_desc* d, const std::vector<int32_t>& rownodes,
    const std::vector<int32_t>& row0, const int32_t* kcol, int cus, StructHost& P, std::string& why)
{
  if (d->celltype != FCG_HEX8 || !d->ele_ijk)
  {
    why = "no lattice hint, or not hex8";
    return false;
  }
  if (d->n_ele == 0 || rownodes.empty())
  {
    why = "nothing to evaluate";
    return false;
  }
  int64_t mn[3], mx[3];
  for (int k = 0; k < 3; ++k)
  {
    mn[k] = INT32_MAX;
    mx[k] = INT32_MIN;
  }
  for (int64_t e = 0; e < d->n_ele; ++e)
    for (int k = 0; k < 3; ++k)
    {
      mn[k] = std::min<int64_t>(mn[k], d->ele_ijk[3 * e + k]);
      mx[k] = std::max<int64_t>(mx[k], d->ele_ijk[3 * e + k]);
    }
  const int64_t EX = mx[0] - mn[0] + 1, EY = mx[1] - mn[1] + 1, EZ = mx[2] - mn[2] + 1;
  if ((EX + 1) * (EY + 1) * (EZ + 1) > 8 * d->n_ele + 4096)
  {
    why = "element lattice box far larger than the element set";
    return false;
  }
  P.elo[0] = int32_t(mn[0]); P.elo[1] = int32_t(mn[1]); P.elo[2] = int32_t(mn[2]);
  P.en[0] = int32_t(EX); P.en[1] = int32_t(EY); P.en[2] = int32_t(EZ);
  P.elem_at.assign(EX * EY * EZ, -1);
  for (int64_t e = 0; e < d->n_ele; ++e)
  {
    const int64_t idx = ((d->ele_ijk[3 * e + 2] - mn[2]) * EY + (d->ele_ijk[3 * e + 1] - mn[1])) * EX +
                        (d->ele_ijk[3 * e] - mn[0]);
    if (P.elem_at[idx] != -1)
    {
      why = "two elements at one lattice position";
      return false;
    }
    P.elem_at[idx] = int32_t(e);
  }
  // node lattice positions, relative to the element box origin, in [0, E+1)
  const int64_t NXn = EX + 1, NYn = EY + 1, NZn = EZ + 1;
  std::vector<int64_t> npos(d->n_node, -1);
  for (int64_t e = 0; e < d->n_ele; ++e)
  {
    const int64_t ex = d->ele_ijk[3 * e] - mn[0], ey = d->ele_ijk[3 * e + 1] - mn[1],
                  ez = d->ele_ijk[3 * e + 2] - mn[2];
    for (int a = 0; a < 8; ++a)
    {
      const int64_t p = ((ez + kOff8[a][2]) * NYn + ey + kOff8[a][1]) * NXn + ex + kOff8[a][0];
      const int32_t node = d->ele_nodes[8 * e + a];
      if (npos[node] == -1)
        npos[node] = p;
      else if (npos[node] != p)
      {
        why = "connectivity does not match the lattice hint";
        return false;
      }
    }
  }
  std::vector<int32_t> node_at(NXn * NYn * NZn, -1);
  for (int64_t nd = 0; nd < d->n_node; ++nd)
  {
    if (npos[nd] < 0) continue;
    if (node_at[npos[nd]] != -1)
    {
      why = "two nodes at one lattice position";
      return false;
    }
    node_at[npos[nd]] = int32_t(nd);
  }
  // owned-node box
  int64_t lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {-1, -1, -1};
  for (int32_t nd : rownodes)
  {
    if (npos[nd] < 0)
    {
      why = "owned node outside every column element";
      return false;
    }
    const int64_t q[3] = {npos[nd] % NXn, (npos[nd] / NXn) % NYn, npos[nd] / (NXn * NYn)};
    for (int k = 0; k < 3; ++k)
    {
      lo[k] = std::min(lo[k], q[k]);
      hi[k] = std::max(hi[k], q[k]);
    }
  }
  for (int k = 0; k < 3; ++k)
  {
    P.lo[k] = int32_t(lo[k] + mn[k]);  // in the hint's lattice coordinates
    P.n[k] = int32_t(hi[k] - lo[k] + 1);
  }
  P.rownode_at.assign(int64_t(P.n[0]) * P.n[1] * P.n[2], -1);
  for (size_t r = 0; r < rownodes.size(); ++r)
  {
    const int64_t p = npos[rownodes[r]];
    const int64_t q[3] = {p % NXn - lo[0], (p / NXn) % NYn - lo[1], p / (NXn * NYn) - lo[2]};
    P.rownode_at[(q[2] * P.n[1] + q[1]) * P.n[0] + q[0]] = int32_t(r);
  }
  // neighbour column positions per owned node row
  const int64_t nrn = int64_t(rownodes.size());
  P.nbr_pos.assign(nrn * 27, 0xFFFF);
  std::string err;
  std::mutex err_m;
  parallel_for(nrn, [&](int64_t r) {
    const int64_t p = npos[rownodes[r]];
    const int64_t i = p % NXn, jj = (p / NXn) % NYn, k = p / (NXn * NYn);
    const int64_t s = d->rowptr[row0[r]];
    const int64_t len = d->rowptr[row0[r] + 1] - s;
    const int32_t* cols = d->col_lid + s;
    int count = 0;
    for (int t = 0; t < 27; ++t)
    {
      const int64_t x = i + t % 3 - 1, y = jj + (t / 3) % 3 - 1, z = k + t / 9 - 1;
      if (x < 0 || x >= NXn || y < 0 || y >= NYn || z < 0 || z >= NZn) continue;
      const int32_t m = node_at[(z * NYn + y) * NXn + x];
      if (m < 0) continue;
      // coupled only through an element holding both nodes (meshes with holes: a lattice
      // neighbour across a missing element is no column of the row, and its position stays absent)
      bool coupled = false;
      for (int64_t ez = std::max(k, z) - 1; ez <= std::min(k, z) && !coupled; ++ez)
        for (int64_t ey = std::max(jj, y) - 1; ey <= std::min(jj, y) && !coupled; ++ey)
          for (int64_t ex = std::max(i, x) - 1; ex <= std::min(i, x) && !coupled; ++ex)
            if (ex >= 0 && ey >= 0 && ez >= 0 && ex < EX && ey < EY && ez < EZ &&
                P.elem_at[(ez * EY + ey) * EX + ex] >= 0)
              coupled = true;
      if (!coupled) continue;
      const int32_t c = kcol[m];
      const int32_t* it = std::lower_bound(cols, cols + len, c);
      const int64_t pos = it - cols;
      if (it == cols + len || *it != c || pos + 3 > len || cols[pos + 1] != c + 1 ||
          cols[pos + 2] != c + 2)
      {
        std::lock_guard<std::mutex> lk(err_m);
        err = "row lacks a lattice neighbour's DOF triple";
        return;
      }
      P.nbr_pos[r * 27 + t] = uint16_t(pos);
      ++count;
    }
    if (3 * count != len)
    {
      std::lock_guard<std::mutex> lk(err_m);
      err = "row holds columns beyond the lattice neighbours";
    }
  });
  if (!err.empty())
  {
    why = err;
    return false;
  }
  // tiles: 4 x 4 node columns, z split into segments.  The workgroups are alike, so the sweep
  // runs in rounds of `slots` resident workgroups (CUs x workgroups per CU: 2 for the linear /
  // TSI sweep, 1 for TotLag, LDS-bound); a segment of s planes costs s + 1 element layers (it
  // starts one layer early).  Pick the segment count with the least rounds x layers -- e.g. 100^3
  // linear on 256 CUs: 3 segments of 34 planes, 2,028 workgroups in 4 full rounds, where a fixed
  // ">= 2,048 workgroups" rule gave 4 segments, 2,704 workgroups and a 28 %-full sixth round.
  P.tiles_x = (P.n[0] + 3) / 4;
  P.tiles_y = (P.n[1] + 3) / 4;
  const int64_t txy = int64_t(P.tiles_x) * P.tiles_y;
  // FCG_SWEEP_WGS_PER_CU: occupancy probes (tools/exp_lib.sh builds with another launch bound)
  const char* wenv = std::getenv("FCG_SWEEP_WGS_PER_CU");
  const int wpc = wenv ? std::max(1, std::atoi(wenv)) : 2;
  const char* tenv = std::getenv("FCG_SWEEP_TOTLAG_WGS_PER_CU");  // the same, TotLag
  const int tpc = tenv ? std::max(1, std::atoi(tenv)) : 1;
  const int64_t slots = int64_t(std::max(1, cus)) * (d->kinematics == FCG_TOTLAG ? tpc : wpc);
  int64_t nseg = 1;
  double best = 0.0;
  for (int64_t k = 1; k <= std::min<int64_t>(P.n[2], 64); ++k)
  {
    const int64_t segk = (P.n[2] + k - 1) / k;
    const int64_t wgs = txy * ((P.n[2] + segk - 1) / segk);
    const double cost = double((wgs + slots - 1) / slots) * double(segk + 1);
    if (k == 1 || cost < best)
    {
      best = cost;
      nseg = k;
    }
  }
  P.seg = int32_t((P.n[2] + nseg - 1) / nseg);
  P.tiles_z = (P.n[2] + P.seg - 1) / P.seg;
  // lattice node tables (coordinates and DOF column LIDs, by lattice position)
  P.lat_x.assign(3 * NXn * NYn * NZn, 0.0);
  P.lat_dof.assign(NXn * NYn * NZn, -1);
  for (int64_t nd = 0; nd < d->n_node; ++nd)
  {
    if (npos[nd] < 0) continue;
    for (int k = 0; k < 3; ++k) P.lat_x[3 * npos[nd] + k] = d->node_x[3 * nd + k];
    P.lat_dof[npos[nd]] = d->node_dof_col[nd];
  }
  // plane records: row bookkeeping of the 16 node columns of every tile, per node plane
  const int64_t W = fcg::PLANE_REC_WORDS;
  P.plane_rec.assign(int64_t(P.tiles_y) * P.tiles_x * P.n[2] * W, 0u);
  parallel_for(int64_t(P.tiles_y) * P.tiles_x * P.n[2], [&](int64_t idx) {
    const int64_t k = idx % P.n[2];
    const int64_t t = idx / P.n[2];
    const int64_t tx = t % P.tiles_x, ty = t / P.tiles_x;
    uint32_t* rec = P.plane_rec.data() + idx * W;
    uint16_t* np = reinterpret_cast<uint16_t*>(rec + 64);
    for (int c = 0; c < 16; ++c)
    {
      const int64_t i = 4 * tx + c % 4, jj = 4 * ty + c / 4;
      int32_t r = -1;
      if (i < P.n[0] && jj < P.n[1]) r = P.rownode_at[(k * P.n[1] + jj) * P.n[0] + i];
      if (r < 0)
      {
        rec[c] = 0xFFFFFFFFu;
        for (int q = 0; q < 27; ++q) np[27 * c + q] = 0xFFFF;
        continue;
      }
      const int64_t base = d->rowptr[row0[r]];
      rec[c] = uint32_t(row0[r]);
      rec[16 + c] = uint32_t(d->rowptr[row0[r] + 1] - base);
      rec[32 + 2 * c] = uint32_t(uint64_t(base) & 0xFFFFFFFFu);
      rec[32 + 2 * c + 1] = uint32_t(uint64_t(base) >> 32);
      for (int q = 0; q < 27; ++q) np[27 * c + q] = P.nbr_pos[r * 27 + q];
    }
  });
  classify_regular_tiles(P);
  return true;
}

// Regular lattice tiles.  On a lattice-numbered box nearly every plane record holds the same few
// numbers: 81 entries per row, one pattern of neighbour positions, rows and bases in arithmetic
// progression along a tile row.  The sweep's linear kernel then needs 12 words of a plane
// instead of 288 and no record field in front of its K stores (fcg_sweep.hip, REG).
void classify_regular_tiles(StructHost& P)
{
  const int64_t W = fcg::PLANE_REC_WORDS, NK = P.n[2];
  const int64_t ntile = int64_t(P.tiles_y) * P.tiles_x;
  P.reg_rec.assign(ntile * NK * REG_REC_WORDS, 0u);
  P.reg_tile.assign(2 * ntile, 0);
  std::fill(P.reg_pos, P.reg_pos + 27, 0);
  P.reg_layers = 0;
  P.layers_total = 0;
  // the pattern: the most frequent one among the rows with all 27 neighbours (rows beside ghost
  // columns, numbered behind the owned ones, have patterns of their own)
  std::map<std::array<uint16_t, 27>, int64_t> seen;
  const int64_t nrn = int64_t(P.nbr_pos.size()) / 27;
  for (int64_t r = 0; r < nrn; ++r)
  {
    std::array<uint16_t, 27> a;
    bool full = true;
    for (int t = 0; t < 27; ++t)
    {
      a[t] = P.nbr_pos[r * 27 + t];
      full = full && a[t] != 0xFFFF;
    }
    if (full) ++seen[a];
  }
  std::array<uint16_t, 27> pat{};
  int64_t most = 0;
  for (const auto& kv : seen)
    if (kv.second > most)
    {
      most = kv.second;
      pat = kv.first;
    }
  if (most > 0)
    for (int t = 0; t < 27; ++t) P.reg_pos[t] = pat[t];
  // planes
  std::vector<uint8_t> plane_ok(ntile * NK, 0);
  if (most > 0)
    parallel_for(ntile * NK, [&](int64_t idx) {
      const uint32_t* rec = P.plane_rec.data() + idx * W;
      const uint16_t* np = reinterpret_cast<const uint16_t*>(rec + 64);
      auto base_of = [&](int c) { return int64_t(uint64_t(rec[32 + 2 * c]) | (uint64_t(rec[32 + 2 * c + 1]) << 32)); };
      for (int c = 0; c < 16; ++c)
      {
        if (rec[c] == 0xFFFFFFFFu || rec[16 + c] != 81u) return;
        for (int t = 0; t < 27; ++t)
          if (np[27 * c + t] != pat[t]) return;
        const int c0 = c & ~3, cx = c & 3;
        if (int64_t(rec[c]) != int64_t(rec[c0]) + 3 * cx || base_of(c) != base_of(c0) + 243 * cx) return;
      }
      uint32_t* cr = P.reg_rec.data() + idx * REG_REC_WORDS;
      for (int y = 0; y < 4; ++y)
      {
        cr[y] = rec[4 * y];
        cr[4 + 2 * y] = rec[32 + 8 * y];
        cr[4 + 2 * y + 1] = rec[32 + 8 * y + 1];
      }
      cr[12] = 1u;
      plane_ok[idx] = 1;
    });
  // runs of regular layers per tile; the elements of a layer: x, y one column around the tile
  const int64_t EX = P.en[0], EY = P.en[1], EZ = P.en[2];
  for (int64_t t = 0; t < ntile; ++t)
  {
    const int64_t tx = t % P.tiles_x, ty = t / P.tiles_x;
    const int64_t x0 = int64_t(P.lo[0]) - P.elo[0] + 4 * tx, y0 = int64_t(P.lo[1]) - P.elo[1] + 4 * ty;
    auto layer_ok = [&](int64_t k) {
      if (k + 1 >= NK || !plane_ok[t * NK + k] || !plane_ok[t * NK + k + 1]) return false;
      const int64_t ez = int64_t(P.lo[2]) - P.elo[2] + k;
      if (ez < 0 || ez >= EZ) return false;
      for (int64_t ey = y0 - 1; ey < y0 + 4; ++ey)
        for (int64_t ex = x0 - 1; ex < x0 + 4; ++ex)
          if (ex < 0 || ey < 0 || ex >= EX || ey >= EY || P.elem_at[(ez * EY + ey) * EX + ex] < 0) return false;
      return true;
    };
    int64_t best_lo = 0, best_n = 0, run_lo = 0, run_n = 0;
    for (int64_t k = 0; k < NK; ++k)
    {
      if (layer_ok(k))
      {
        if (run_n == 0) run_lo = k;
        if (++run_n > best_n)
        {
          best_n = run_n;
          best_lo = run_lo;
        }
      }
      else
        run_n = 0;
    }
    const int64_t lo = best_lo, hi = best_n > 0 ? best_lo + best_n + 1 : best_lo;
    P.reg_tile[2 * t] = int32_t(lo);
    P.reg_tile[2 * t + 1] = int32_t(hi);
    // the sweep's segments: workgroup tz writes planes [kz0, kz1) and runs layers kz0 - 1 .. kz1 - 1
    for (int64_t tz = 0; tz < P.tiles_z; ++tz)
    {
      const int64_t kz0 = int64_t(P.seg) * tz, kz1 = std::min<int64_t>(kz0 + P.seg, NK);
      P.layers_total += kz1 - kz0 + 1;
      P.reg_layers += std::max<int64_t>(0, std::min(hi, kz1) - 1 - std::max(lo, kz0));
    }
  }
}

// Colour-ordered direct assembly plan (hex27 on a verified lattice).  Element e at lattice
// position (ex, ey, ez) gets colour (ex & 1) + 2 (ey & 1) + 4 (ez & 1); two elements of one colour
// share no node, so the eight colour launches write disjoint rows.  The elements holding both
// nodes a, b of e form the product over the axes of {e} or {e, e -+ 1} (the latter when a and b
// both lie on e's lower / upper face along that axis); the first of them in colour order is the
// even one along every such axis, or e itself when the odd/even partner does not exist.  Bits of
// ft[e]: 2d = e comes first along axis d for pairs on its lower face, 2d+1 = on its upper face.
// The hint must place every element node at 2 ijk(e) + position(a) consistently (unique nodes
// and positions), which makes lattice neighbours share exactly their face nodes.
bool build_colored_plan(const fcg_desc* d, ColorHost& P, std::string& why)
{
  if (d->celltype != FCG_HEX27 || !d->ele_ijk)
  {
    why = "no lattice hint, or not hex27";
    return false;
  }
  if (d->n_ele == 0)
  {
    why = "nothing to evaluate";
    return false;
  }
  int64_t mn[3], mx[3];
  for (int k = 0; k < 3; ++k)
  {
    mn[k] = INT32_MAX;
    mx[k] = INT32_MIN;
  }
  for (int64_t e = 0; e < d->n_ele; ++e)
    for (int k = 0; k < 3; ++k)
    {
      mn[k] = std::min<int64_t>(mn[k], d->ele_ijk[3 * e + k]);
      mx[k] = std::max<int64_t>(mx[k], d->ele_ijk[3 * e + k]);
    }
  const int64_t EX = mx[0] - mn[0] + 1, EY = mx[1] - mn[1] + 1, EZ = mx[2] - mn[2] + 1;
  if (EX * EY * EZ > 8 * d->n_ele + 4096)
  {
    why = "element lattice box far larger than the element set";
    return false;
  }
  std::vector<int32_t> elem_at(EX * EY * EZ, -1);
  for (int64_t e = 0; e < d->n_ele; ++e)
  {
    const int64_t idx = ((d->ele_ijk[3 * e + 2] - mn[2]) * EY + (d->ele_ijk[3 * e + 1] - mn[1])) * EX +
                        (d->ele_ijk[3 * e] - mn[0]);
    if (elem_at[idx] != -1)
    {
      why = "two elements at one lattice position";
      return false;
    }
    elem_at[idx] = int32_t(e);
  }
  // node positions on the (2E+1)^3 lattice of the element box
  const int64_t NXn = 2 * EX + 1, NYn = 2 * EY + 1;
  std::vector<int64_t> npos(d->n_node, -1);
  for (int64_t e = 0; e < d->n_ele; ++e)
  {
    const int64_t ex = d->ele_ijk[3 * e] - mn[0], ey = d->ele_ijk[3 * e + 1] - mn[1],
                  ez = d->ele_ijk[3 * e + 2] - mn[2];
    for (int a = 0; a < 27; ++a)
    {
      const int64_t p = ((2 * ez + fcg::kHex27NodePos[a][2]) * NYn + 2 * ey + fcg::kHex27NodePos[a][1]) *
                            NXn + 2 * ex + fcg::kHex27NodePos[a][0];
      const int32_t node = d->ele_nodes[27 * e + a];
      if (npos[node] == -1)
        npos[node] = p;
      else if (npos[node] != p)
      {
        why = "connectivity does not match the lattice hint";
        return false;
      }
    }
  }
  {
    std::vector<int64_t> sorted;
    sorted.reserve(d->n_node);
    for (int64_t nd = 0; nd < d->n_node; ++nd)
      if (npos[nd] >= 0) sorted.push_back(npos[nd]);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    {
      why = "two nodes at one lattice position";
      return false;
    }
  }
  P.ft.assign(d->n_ele, 0);
  std::vector<int64_t> cnt(8, 0);
  std::vector<uint8_t> color(d->n_ele);
  for (int64_t e = 0; e < d->n_ele; ++e)
  {
    const int64_t c[3] = {d->ele_ijk[3 * e] - mn[0], d->ele_ijk[3 * e + 1] - mn[1],
        d->ele_ijk[3 * e + 2] - mn[2]};
    uint8_t bits = 0, col = 0;
    for (int k = 0; k < 3; ++k)
    {
      const bool even = (d->ele_ijk[3 * e + k] & 1) == 0;
      int64_t lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
      lo[k] -= 1;
      hi[k] += 1;
      auto exists = [&](const int64_t* q) {
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] >= EX || q[1] >= EY || q[2] >= EZ) return false;
        return elem_at[(q[2] * EY + q[1]) * EX + q[0]] >= 0;
      };
      if (even || !exists(lo)) bits |= uint8_t(1u << (2 * k));
      if (even || !exists(hi)) bits |= uint8_t(1u << (2 * k + 1));
      if (!even) col |= uint8_t(1u << k);
    }
    P.ft[e] = bits;
    color[e] = col;
    cnt[col]++;
  }
  P.color_ptr[0] = 0;
  for (int c = 0; c < 8; ++c) P.color_ptr[c + 1] = P.color_ptr[c] + cnt[c];
  P.col_ele.resize(d->n_ele);
  std::vector<int64_t> fill(P.color_ptr, P.color_ptr + 8);
  for (int64_t e = 0; e < d->n_ele; ++e) P.col_ele[fill[color[e]]++] = int32_t(e);

  // pencil order: walk the lattice box colour by colour, (ez, ey) rows, x runs
  P.nb.assign(d->n_ele, 0u);
  P.pen_ele.clear();
  P.pen_ele.reserve(d->n_ele);
  P.pen_ptr.assign(1, 0);
  auto at = [&](int64_t x, int64_t y, int64_t z) -> int32_t {
    if (x < 0 || y < 0 || z < 0 || x >= EX || y >= EY || z >= EZ) return -1;
    return elem_at[(z * EY + y) * EX + x];
  };
  for (int c = 0; c < 4; ++c)
  {
    P.pen_color[c] = int64_t(P.pen_ptr.size()) - 1;
    // parity of the absolute lattice index (the same colours on every rank of a box split)
    for (int64_t z = 0; z < EZ; ++z)
    {
      if (((z + mn[2]) & 1) != (c >> 1)) continue;
      for (int64_t y = 0; y < EY; ++y)
      {
        if (((y + mn[1]) & 1) != (c & 1)) continue;
        for (int64_t x = 0; x < EX; ++x)
        {
          const int32_t e = at(x, y, z);
          if (e < 0) continue;
          if (at(x - 1, y, z) < 0 && !P.pen_ele.empty() && int64_t(P.pen_ele.size()) != P.pen_ptr.back())
            P.pen_ptr.push_back(int64_t(P.pen_ele.size()));  // a new run starts
          P.pen_ele.push_back(e);
          uint32_t bits = 0;
          for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx)
                if (at(x + dx, y + dy, z + dz) >= 0) bits |= 1u << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1));
          bits |= uint32_t((y + mn[1]) & 1) << 27;
          bits |= uint32_t((z + mn[2]) & 1) << 28;
          P.nb[e] = bits;
        }
      }
    }
    if (int64_t(P.pen_ele.size()) != P.pen_ptr.back()) P.pen_ptr.push_back(int64_t(P.pen_ele.size()));
  }
  P.pen_color[4] = int64_t(P.pen_ptr.size()) - 1;
  return true;
}

// hex27 slab schedule (DeviceMesh::h27_*): elements in slabs of S consecutive elements; a row
// node is assembled after the slab of its last incident element (its completing slab c), and its
// records occupy consecutive ring slots from the moment its first element is evaluated (slab smin)
// until that assembly.  Rows are laid out in the ring in assembly order (by c, then Morton order),
// so a slot is reused by a later row; the smallest ring is the one in which every row's slots were
// last held by rows assembled at least 1 + lag slabs before the row's first writer slab (element
// and assembly launches alternate on one stream: lag 0).
void build_h27_ring(int64_t n_ele, int64_t S, int lag, const std::vector<int64_t>& inc_ptr,
    const std::vector<int32_t>& inc_ele, const std::vector<uint8_t>& inc_a,
    const std::vector<int64_t>& morton, H27Ring& R)
{
  const int64_t nrn = int64_t(inc_ptr.size()) - 1;
  R.nslab = (n_ele + S - 1) / S;
  std::vector<int32_t> smin(nrn, 0), cmax(nrn, 0);
  parallel_for(nrn, [&](int64_t r) {
    int64_t lo = INT64_MAX, hi = 0;
    for (int64_t k = inc_ptr[r]; k < inc_ptr[r + 1]; ++k)
    {
      const int64_t sl = int64_t(inc_ele[k]) / S;
      lo = std::min(lo, sl);
      hi = std::max(hi, sl);
    }
    smin[r] = int32_t(lo == INT64_MAX ? 0 : lo);
    cmax[r] = int32_t(hi);
  });
  // rows by completing slab, Morton order inside a slab (a stable counting sort of the Morton list)
  R.asm_ptr.assign(R.nslab + 1, 0);
  for (int64_t r = 0; r < nrn; ++r) R.asm_ptr[cmax[r] + 1]++;
  for (int64_t c = 0; c < R.nslab; ++c) R.asm_ptr[c + 1] += R.asm_ptr[c];
  R.rows.assign(nrn, 0);
  {
    std::vector<int64_t> fill(R.asm_ptr.begin(), R.asm_ptr.end() - 1);
    for (int64_t i = 0; i < nrn; ++i)
    {
      const int64_t r = morton[i];
      R.rows[fill[cmax[r]]++] = int32_t(r);
    }
  }
  std::vector<int64_t> P(nrn + 1, 0);  // first ring position (unwrapped) of the j-th row
  int64_t maxn = 1;
  for (int64_t j = 0; j < nrn; ++j)
  {
    const int64_t n = inc_ptr[R.rows[j] + 1] - inc_ptr[R.rows[j]];
    P[j + 1] = P[j] + n;
    maxn = std::max(maxn, n);
  }
  const int64_t n_inc = P[nrn];
  // does a ring of `ring` slots keep every row's slots free until its first writer slab?
  auto fits = [&](int64_t ring) {
    int64_t jp = 0;  // the row holding position P[j] + n - 1 - ring, found by a forward scan
    for (int64_t j = 0; j < nrn; ++j)
    {
      const int64_t last = P[j + 1] - 1 - ring;
      if (last < 0) continue;
      while (P[jp + 1] <= last) ++jp;
      if (cmax[R.rows[jp]] > smin[R.rows[j]] - 1 - lag) return false;
    }
    return true;
  };
  int64_t lo = maxn, hi = std::max<int64_t>(maxn, n_inc);
  while (lo < hi)
  {
    const int64_t mid = lo + (hi - lo) / 2;
    if (fits(mid))
      hi = mid;
    else
      lo = mid + 1;
  }
  R.ring = lo;
  R.rslot0.assign(nrn, 0);
  R.slot.assign(size_t(n_ele) * 27, -1);
  for (int64_t j = 0; j < nrn; ++j)
  {
    const int64_t r = R.rows[j];
    R.rslot0[r] = int32_t(P[j] % R.ring);
    for (int64_t k = inc_ptr[r]; k < inc_ptr[r + 1]; ++k)
      R.slot[size_t(inc_ele[k]) * 27 + inc_a[k]] = int32_t((P[j] + (k - inc_ptr[r])) % R.ring);
  }
}

// Output: the owned incidences' block rows (assemble27_kernel reads each once, contiguous).
// Slab schedule of the incidence records (DeviceMesh::h27_*): FCG_H27_SLAB elements per
// slab (0 = one slab); by default only when one record per incidence, the caller's K
// values and 4 GB of headroom would not fit the device's free memory (1M hex27: 53 GB of
// 288 GB -> one slab).  Measured at 1M hex27 TotLag: slabs of 5,000 / 10,000 /
// 20,000 elements keep a ring of 1.18 / 1.24 / 2.30 GB instead of 53 GB, at 64.5 / 59.9 /
// 56.9 ms per evaluate instead of 51.5 ms (every slab boundary drains the element kernel's
// two-element pipeline), so that meshes of several million hex27 elements fit one GPU
// beside their tangent
H27Schedule h27_schedule(int64_t n_ele, int64_t n_inc, int64_t nnz, int64_t record_bytes,
    int64_t mem_free, int64_t mem_total, int cus, const char* slab_env, const char* el_grid_env)
{
  H27Schedule s;
  s.slab = slab_env ? std::atoll(slab_env) : 0;
  s.el_grid = el_grid_env ? std::max(1, std::atoi(el_grid_env)) : 2 * cus;  // the resident workgroups
  // the full scratch whenever it fits: the slab schedule costs about +25 % per evaluate, so
  // it is taken only when the records plus the caller's K values (and 4 GB of headroom for the
  // vectors and the solver) would not fit the device's free memory now
  const double full = double(n_inc) * double(record_bytes);
  if (mem_free < 0) mem_free = mem_total;
  const double need = full + double(nnz) * sizeof(double) + double(int64_t(4) << 30);
  if (!slab_env && mem_free > 0 && need > double(mem_free)) s.slab = std::max<int64_t>(4096, n_ele / 200);
  return s;
}

// a refused descriptor: FCG_ERR_ARG and why
static int refuse(std::string& why, std::string msg)
{
  why = std::move(msg);
  return FCG_ERR_ARG;
}

int check_descriptor(const fcg_desc* d, std::string& why)
{
  if (d->abi_version != FCG_ABI_VERSION) return refuse(why, "abi_version mismatch");
  if ((d->celltype != FCG_HEX8 && d->celltype != FCG_HEX27) ||
      (d->kinematics != FCG_LINEAR && d->kinematics != FCG_TOTLAG))
    return refuse(why, "unsupported celltype/kinematics");
  // Mat::PAR::StVenantKirchhoff parameter checks (4C_mat_stvenantkirchhoff.cpp:26-28)
  if (!(d->youngs > 0.0) || d->poisson >= 0.5 || d->poisson < -1.0)
    return refuse(why, "Young's modulus must be > 0 and Poisson's ratio in [-1;0.5)");
  if (d->material != FCG_MAT_STVK && d->material != FCG_MAT_ELASTHYPER_COUPNEOHOOKE)
    return refuse(why, "unsupported material");
  if (d->material == FCG_MAT_ELASTHYPER_COUPNEOHOOKE && d->kinematics != FCG_TOTLAG)
    return refuse(why, "ElastHyper is supported with KINEM nonlinear (TotLag) only");
  if (d->material != FCG_MAT_STVK && d->path == FCG_PATH_STRUCTURED && d->celltype == FCG_HEX8)
    return refuse(why, "the structured sweep implements StVenantKirchhoff only (hex8 "
                       "ElastHyper/CoupNeoHooke: FCG_PATH_GATHER or FCG_PATH_GENERAL)");
  // rowptr = col_lid = NULL: the graph is built on the device (FillComplete of the first
  // assembly); one of the two alone is an error
  const bool build_graph = d->n_rows > 0 && !d->rowptr && !d->col_lid;
  if (d->n_ele < 0 || d->n_node < 0 || d->n_rows < 0 || d->n_cols < 0 ||
      (d->n_ele > 0 && (!d->ele_nodes || !d->node_x || !d->node_dof_col || !d->node_dof_row)) ||
      (d->n_rows > 0 && !build_graph && (!d->rowptr || !d->col_lid)) || d->n_ele >= (int64_t(1) << 31))
    return refuse(why, "invalid descriptor arrays/sizes");
  const int npe = d->celltype == FCG_HEX27 ? 27 : 8;
  // --- validate connectivity
  for (int64_t i = 0; i < d->n_ele * npe; ++i)
    if (d->ele_nodes[i] < 0 || d->ele_nodes[i] >= d->n_node)
      return refuse(why, "element references a node outside [0, n_node)");
  for (int64_t n = 0; n < d->n_node; ++n)
  {
    if (d->node_dof_col[n] < 0 || d->node_dof_col[n] + 3 > d->n_cols) return refuse(why, "node_dof_col out of range");
    if (d->node_dof_row[n] >= 0 && d->node_dof_row[n] + 3 > d->n_rows)
      return refuse(why, "node_dof_row out of range");
  }
  return FCG_OK;
}

int build_node_rows(const fcg_desc* d, NodeRows& N, std::string& why)
{
  const int maxrow = d->celltype == FCG_HEX27 ? 375 : 81;
  // --- owned row nodes, ascending by row LID
  for (int64_t n = 0; n < d->n_node; ++n)
    if (d->node_dof_row[n] >= 0) N.rownodes.push_back(int32_t(n));
  std::sort(N.rownodes.begin(), N.rownodes.end(),
      [&](int32_t a, int32_t b) { return d->node_dof_row[a] < d->node_dof_row[b]; });
  N.rn_of_node.assign(d->n_node, -1);
  for (size_t i = 0; i < N.rownodes.size(); ++i) N.rn_of_node[N.rownodes[i]] = int32_t(i);
  const int64_t nrn = N.nrn();

  // --- CSR structure of node rows: 3 consecutive rows with identical column lists
  const std::vector<int32_t>& row0 = N.row0;
  N.row0.resize(nrn);
  for (int64_t r = 0; r < nrn; ++r)
  {
    N.row0[r] = d->node_dof_row[N.rownodes[r]];
    const int64_t s = d->rowptr[row0[r]];
    const int64_t len = d->rowptr[row0[r] + 1] - s;
    N.max_rowlen = std::max<int32_t>(N.max_rowlen, int32_t(len));
    if (len > maxrow || d->rowptr[row0[r] + 2] - d->rowptr[row0[r] + 1] != len ||
        d->rowptr[row0[r] + 3] - d->rowptr[row0[r] + 2] != len)
      return refuse(why, "node rows must have 3 equal-length rows of <= 3*neighbours columns");
  }
  // whether every node row holds node DOF triples (c, c + 1, c + 2) only: the node-row SpMV and the
  // AMG's block copy walk a row by triples; a caller's graph may hold other columns as well (the
  // general path assembles it all the same), and then the operator goes row by row
  std::atomic<bool> triple_rows{true}, pattern_differs{false};
  parallel_for(nrn, [&](int64_t r) {
    const int64_t s = d->rowptr[row0[r]];
    const int64_t len = d->rowptr[row0[r] + 1] - s;
    for (int i = 1; i < 3; ++i)
      if (std::memcmp(d->col_lid + s, d->col_lid + s + i * len, sizeof(int32_t) * len) != 0)
        pattern_differs.store(true, std::memory_order_relaxed);
    const int32_t* c = d->col_lid + s;
    bool triples = len % 3 == 0;
    for (int64_t j = 0; triples && j < len; j += 3)
      triples = c[j + 1] == c[j] + 1 && c[j + 2] == c[j] + 2;
    if (!triples) triple_rows.store(false, std::memory_order_relaxed);
  });
  if (pattern_differs)
    return refuse(why, "the 3 rows of a node must share one column pattern");
  N.triple_rows = triple_rows.load();
  return FCG_OK;
}

void build_operator_support(const fcg_desc* d, NodeRows& N)
{
  const int32_t* kcol = kcol_of(d);
  N.diag.assign(d->n_rows, -1);
  std::atomic<bool> rowcol_ok{3 * N.nrn() == d->n_rows};  // owned column triple == row triple
  parallel_for(N.nrn(), [&](int64_t r) {
    const int32_t nd = N.rownodes[r];
    if (kcol[nd] != N.row0[r]) rowcol_ok.store(false, std::memory_order_relaxed);
    for (int dd = 0; dd < 3; ++dd)
    {
      const int64_t row = N.row0[r] + dd;
      const int32_t* b = d->col_lid + d->rowptr[row];
      const int32_t* e = d->col_lid + d->rowptr[row + 1];
      const int32_t* it = std::lower_bound(b, e, kcol[nd] + dd);
      if (it != e && *it == kcol[nd] + dd) N.diag[row] = d->rowptr[row] + (it - b);
    }
  });
  N.rowcol = rowcol_ok.load();
  N.square_local = N.rowcol && d->n_rows == d->n_cols;
  N.owned_cols_first = N.rowcol;
}

int choose_path(const fcg_desc* d, const NodeRows& N, int cus, PathChoice& P, std::string& why)
{
  const int32_t* kcol = kcol_of(d);
  // --- structured (row-block sweep) plan when a verified lattice hint is present
  if (d->path != FCG_PATH_GENERAL && d->path != FCG_PATH_GATHER && d->material == FCG_MAT_STVK)
  {
    // an input-file hex8 mesh without the hint: look for the lattice in the connectivity
    // (FCG_DETECT_LATTICE=0 turns this off)
    static const bool detect = [] {
      const char* e = std::getenv("FCG_DETECT_LATTICE");
      return !(e && e[0] == '0');
    }();
    std::vector<int32_t> found_ijk, found_nodes;
    fcg_desc dl;
    if (!d->ele_ijk && d->celltype == FCG_HEX8 && detect &&
        detect_lattice_hex8(d, found_ijk, found_nodes, why))
    {
      // the sweep reads the cells and the nodes in 4C's local order for them (element frames of
      // an input file may be any rotation of it; K and f do not depend on the local numbering)
      dl = *d;
      dl.ele_ijk = found_ijk.data();
      dl.ele_nodes = found_nodes.data();
      P.structured = build_structured_plan(&dl, N.rownodes, N.row0, kcol, cus, P.sp, why);
    }
    else if (d->ele_ijk)
      P.structured = build_structured_plan(d, N.rownodes, N.row0, kcol, cus, P.sp, why);
    else if (why.empty())
      why = "no lattice hint";
    if (!P.structured && d->path == FCG_PATH_STRUCTURED && d->celltype == FCG_HEX8)
      return refuse(why, "structured path requested but the lattice hint does not verify: " + why);
  }
  // --- colour-ordered direct assembly (hex27 on a verified lattice, any material)
  // AUTO keeps hex27 on the general path: it measured faster (hex27 40^3 on one MI355X: 4.2 vs
  // 5.2 ms linear, 4.8 vs 6.6 ms TotLag -- the colour launches write K in 72-byte runs that share
  // cache lines with other colours' runs); the colour-ordered path needs no scratch (1M hex27:
  // 53 GB less device memory) and is taken when requested.
  if ((d->path == FCG_PATH_STRUCTURED || d->path == FCG_PATH_COLORED) && d->celltype == FCG_HEX27)
  {
    P.colored = build_colored_plan(d, P.cp, why);
    if (!P.colored)
      return refuse(why, "lattice path requested but the lattice hint does not verify: " + why);
  }
  if (d->path == FCG_PATH_COLORED && d->celltype != FCG_HEX27)
    return refuse(why, "the colour-ordered path is implemented for hex27");
  // --- node-row gather: hex8 StVK meshes without a verified lattice (AUTO), or on request (StVK
  // and ElastHyper/CoupNeoHooke; AUTO keeps CoupNeoHooke on the general path)
  if (d->path == FCG_PATH_GATHER && d->celltype != FCG_HEX8)
    return refuse(why, "the gather path is implemented for hex8 (StVenantKirchhoff and "
                       "ElastHyper/CoupNeoHooke)");
  P.gather = !P.structured && d->celltype == FCG_HEX8 &&
             (d->path == FCG_PATH_GATHER || (d->path == FCG_PATH_AUTO && d->material == FCG_MAT_STVK));
  return FCG_OK;
}

int build_incidences(const fcg_desc* d, const NodeRows& N, const PathChoice& P, Incidences& I,
    std::string& why)
{
  const int npe = d->celltype == FCG_HEX27 ? 27 : 8;
  const int64_t nrn = N.nrn();
  const int64_t n_en = P.structured ? 0 : d->n_ele * npe;
  I.inc_ptr.assign(nrn + 1, 0);
  for (int64_t i = 0; i < n_en; ++i)
  {
    const int32_t rn = N.rn_of_node[d->ele_nodes[i]];
    if (rn >= 0) I.inc_ptr[rn + 1]++;
  }
  for (int64_t r = 0; r < nrn; ++r) I.inc_ptr[r + 1] += I.inc_ptr[r];
  I.n_inc = I.inc_ptr[nrn];
  if (I.n_inc >= (int64_t(1) << 31))
    return refuse(why, "too many incidences for one context (> 2^31)");
  I.inc_of.assign(n_en, -1);
  I.inc_ele.resize(I.n_inc);
  I.inc_a.resize(I.n_inc);
  I.inc_row0.resize(P.colored ? I.n_inc : 0);
  if (!P.structured)
  {
    std::vector<int64_t> fill(I.inc_ptr.begin(), I.inc_ptr.end() - 1);
    for (int64_t e = 0; e < d->n_ele; ++e)
      for (int a = 0; a < npe; ++a)
      {
        const int32_t rn = N.rn_of_node[d->ele_nodes[e * npe + a]];
        if (rn < 0) continue;
        const int64_t k = fill[rn]++;
        I.inc_of[e * npe + a] = int32_t(k);
        I.inc_ele[k] = int32_t(e);
        I.inc_a[k] = uint8_t(a);
        if (P.colored) I.inc_row0[k] = N.row0[rn];
      }
  }
  return FCG_OK;
}

int build_incidence_positions(const fcg_desc* d, const NodeRows& N, PathChoice& P, Incidences& I,
    std::string& why)
{
  const int npe = d->celltype == FCG_HEX27 ? 27 : 8;
  const int32_t* kcol = kcol_of(d);
  // --- positions of every element node's DOF triple inside the row (stride fast path)
  I.inc_pos.resize(I.n_inc * npe);
  std::atomic<bool> missing{false};
  parallel_for(P.structured ? 0 : N.nrn(), [&](int64_t r) {
    const int64_t s = d->rowptr[N.row0[r]];
    const int64_t len = d->rowptr[N.row0[r] + 1] - s;
    const int32_t* cols = d->col_lid + s;
    for (int64_t k = I.inc_ptr[r]; k < I.inc_ptr[r + 1]; ++k)
    {
      const int32_t* en = d->ele_nodes + int64_t(I.inc_ele[k]) * npe;
      for (int b = 0; b < npe; ++b)
      {
        const int32_t c = kcol[en[b]];
        const int32_t* it = std::lower_bound(cols, cols + len, c);
        const int64_t pos = it - cols;
        if (it == cols + len || *it != c || pos + 3 > len || cols[pos + 1] != c + 1 ||
            cols[pos + 2] != c + 2)
        {
          missing.store(true, std::memory_order_relaxed);
          return;
        }
        I.inc_pos[k * npe + b] = uint16_t(pos);
      }
    }
  });
  if (missing)
    return refuse(why, "matrix graph lacks an element coupling or a node's DOF columns are not "
          "contiguous (SparseMatrix::assemble stride fast path)");
  // the gather path addresses a row by node triples (one byte each): every element node's columns
  // must start a triple of the row, which holds when the row is made of node DOF triples only
  if (P.gather)
    for (int64_t i = 0; i < I.n_inc * npe && P.gather; ++i)
      if (I.inc_pos[i] % 3 != 0) P.gather = false;
  if (!P.gather && d->path == FCG_PATH_GATHER)
    return refuse(why, "gather path: a row holds columns that are not node DOF triples");
  return FCG_OK;
}

std::vector<int64_t> rownode_morton_order(const fcg_desc* d, const NodeRows& N, double* lo_out,
    double* hi_out)
{
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int64_t n = 0; n < d->n_node; ++n)
    for (int k = 0; k < 3; ++k)
    {
      lo[k] = std::min(lo[k], d->node_x[3 * n + k]);
      hi[k] = std::max(hi[k], d->node_x[3 * n + k]);
    }
  std::vector<uint64_t> key(N.nrn());
  parallel_for(N.nrn(), [&](int64_t r) { key[r] = morton_key(d->node_x + 3 * int64_t(N.rownodes[r]), lo, hi); });
  for (int k = 0; k < 3 && lo_out && hi_out; ++k)
  {
    lo_out[k] = lo[k];
    hi_out[k] = hi[k];
  }
  return morton_order(key);
}

// Records of <= 8 incidences per row node (a node without elements keeps one empty record,
// which zeroes its rows under OVERWRITE): first one record per node with <= 8 elements, in
// row order, then the records of the other nodes, node by node
//
// Locality (input-file meshes carry arbitrary node and element numbers): the records follow
// the Morton order of their row nodes' coordinates and the element data the Morton order of
// the element centroids, so that the wavefronts working at the same time, and the records of
// one XCD's contiguous range, share elements and displacements in L2 instead of re-reading
// them from HBM (6.7 GB fetched per 1M-hex8 evaluate in random order).
void build_gather_plan(const fcg_desc* d, const NodeRows& N, const Incidences& I, GatherHost& G)
{
  const int64_t nrn = N.nrn();
  const std::vector<int64_t>& inc_ptr = I.inc_ptr;
  double lo[3], hi[3];
  const std::vector<int64_t> rorder = rownode_morton_order(d, N, lo, hi);
  std::vector<uint64_t> ekey(d->n_ele);
  parallel_for(d->n_ele, [&](int64_t e) {
    double c[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < 8; ++b)
      for (int k = 0; k < 3; ++k) c[k] += 0.125 * d->node_x[3 * int64_t(d->ele_nodes[e * 8 + b]) + k];
    ekey[e] = morton_key(c, lo, hi);
  });
  const std::vector<int64_t> eorder = morton_order(ekey);  // storage slot -> element
  std::vector<int32_t> eslot(d->n_ele);                     // element -> storage slot
  for (int64_t i = 0; i < d->n_ele; ++i) eslot[eorder[i]] = int32_t(i);
  std::vector<int64_t> rec_start(nrn), nrec(nrn);
  G.multi_ptr.assign(1, 0);
  G.n_single = 0;
  for (int64_t i = 0; i < nrn; ++i)
  {
    const int64_t r = rorder[i];
    nrec[r] = std::max<int64_t>(1, (inc_ptr[r + 1] - inc_ptr[r] + 7) / 8);
    if (nrec[r] == 1) rec_start[r] = G.n_single++;
  }
  for (int64_t i = 0; i < nrn; ++i)
  {
    const int64_t r = rorder[i];
    if (nrec[r] > 1)
    {
      rec_start[r] = G.n_single + G.multi_ptr.back();
      G.multi_ptr.push_back(G.multi_ptr.back() + nrec[r]);
    }
  }
  for (auto& v : G.multi_ptr) v += G.n_single;
  const int64_t n_rec = G.n_rec = G.multi_ptr.back();
  G.rec_row0.resize(n_rec);
  G.rec_meta.resize(n_rec);
  G.rec_ele.assign(n_rec * 8, -1);
  G.rec_base.resize(n_rec);
  G.rec_a.assign(n_rec * 8, 0);
  G.rec_tmap.assign(n_rec * 32, 0x88888888u);
  parallel_for(nrn, [&](int64_t r) {
    const int64_t nr = nrec[r];
    const int32_t row0 = N.row0[r];
    for (int64_t i = 0; i < nr; ++i)
    {
      const int64_t R = rec_start[r] + i;
      const int64_t k0 = inc_ptr[r] + 8 * i;
      const int ns = int(std::min<int64_t>(8, std::max<int64_t>(0, inc_ptr[r + 1] - k0)));
      G.rec_row0[R] = row0;
      G.rec_meta[R] = ns | (i == 0 ? 16 : 0) | (i == nr - 1 ? 32 : 0) |
                      int32_t(d->rowptr[row0 + 1] - d->rowptr[row0]) << 8;
      G.rec_base[R] = d->rowptr[row0];
      // per column triple t of the rows: which element node of slot s lands there (nibble s;
      // 8 = none) -- stage 4 of the kernel sums a triple's blocks in slot (element) order
      for (int s = 0; s < ns; ++s)
      {
        G.rec_ele[R * 8 + s] = eslot[I.inc_ele[k0 + s]];
        G.rec_a[R * 8 + s] = I.inc_a[k0 + s];
        for (int b = 0; b < 8; ++b)
        {
          uint32_t& w = G.rec_tmap[R * 32 + I.inc_pos[(k0 + s) * 8 + b] / 3];
          w = (w & ~(15u << (4 * s))) | (uint32_t(b) << (4 * s));
        }
      }
    }
  });
  G.ex.resize(d->n_ele * 24);
  G.edof.resize(d->n_ele * 8);
  G.eorig.resize(d->n_ele);
  parallel_for(d->n_ele, [&](int64_t i) {
    const int64_t e = eorder[i];
    G.eorig[i] = int32_t(e);
    for (int b = 0; b < 8; ++b)
    {
      const int32_t nd = d->ele_nodes[e * 8 + b];
      for (int k = 0; k < 3; ++k) G.ex[i * 24 + 3 * b + k] = d->node_x[3 * int64_t(nd) + k];
      G.edof[i * 8 + b] = d->node_dof_col[nd];
    }
  });
  // Gauss points of the hex8 stiffness rule: xi, eta, zeta, weight
  G.gauss.resize(32);
  double xi[81], w[27];
  gauss_rule(kHex8, xi, w);
  for (int g = 0; g < 8; ++g)
  {
    for (int k = 0; k < 3; ++k) G.gauss[4 * g + k] = xi[3 * g + k];
    G.gauss[4 * g + 3] = w[g];
  }
}

}  // namespace create
}  // namespace fcg
