// fcg_tsi_surface_plan.cpp -- the host stages of fcg_tsi_surface_create
// (fcg_tsi_surface_plan.hpp).  No HIP: this unit compiles and links with a host compiler alone.
#include "fcg_tsi_surface_plan.hpp"

#include <algorithm>

#include "fcg_quad_shape.hpp"

namespace fcg {
namespace tsi_surface_plan {

int check_faces(const Maps& M, int64_t n_faces, const int32_t* face_nodes, std::string& why)
{
  if (M.celltype != FCG_HEX8 && M.celltype != FCG_HEX27)
  {
    why = "unsupported celltype";
    return FCG_ERR_ARG;
  }
  if (n_faces < 0 || (n_faces > 0 && !face_nodes))
  {
    why = "n_faces < 0, or faces without face_nodes";
    return FCG_ERR_ARG;
  }
  const int nfn = nfn_of(M.celltype);
  for (int64_t f = 0; f < n_faces; ++f)
  {
    const int32_t* fn = face_nodes + f * nfn;
    for (int a = 0; a < nfn; ++a)
    {
      if (fn[a] < 0 || fn[a] >= M.n_node)
      {
        why = "face " + std::to_string(f) + ": node " + std::to_string(fn[a]) + " outside [0, n_node)";
        return FCG_ERR_ARG;
      }
      for (int b = 0; b < a; ++b)
        if (fn[b] == fn[a])
        {
          why = "face " + std::to_string(f) + ": node " + std::to_string(fn[a]) + " is repeated";
          return FCG_ERR_ARG;
        }
    }
  }
  return FCG_OK;
}

int build_rows(const Maps& M, int64_t n_faces, const int32_t* face_nodes, Plan& P, std::string& why)
{
  const int nfn = nfn_of(M.celltype);
  P.nfn = nfn;
  P.n_faces = n_faces;
  // incidences per thermo row, then the rows that have any, ascending
  std::vector<int32_t> count(size_t(M.n_rows_t), 0);
  for (int64_t i = 0; i < n_faces * nfn; ++i)
  {
    const int32_t t = M.node_dof_row_t[face_nodes[i]];
    if (t >= M.n_rows_t)
    {
      why = "face " + std::to_string(i / nfn) + ": a node's thermo row is outside the row map";
      return FCG_ERR_ARG;
    }
    if (t >= 0) count[size_t(t)]++;
  }
  P.s_row.clear();
  P.inc_ptr.assign(1, 0);
  std::vector<int32_t> sr_of_row(size_t(M.n_rows_t), -1);
  for (int64_t t = 0; t < M.n_rows_t; ++t)
    if (count[size_t(t)] > 0)
    {
      sr_of_row[size_t(t)] = int32_t(P.s_row.size());
      P.s_row.push_back(int32_t(t));
      P.inc_ptr.push_back(P.inc_ptr.back() + count[size_t(t)]);
    }
  const int64_t n_inc = P.inc_ptr.back();
  P.inc_face.resize(size_t(n_inc));
  P.inc_loc.resize(size_t(n_inc));
  std::vector<int64_t> fill(P.inc_ptr.begin(), P.inc_ptr.end() - 1);
  for (int64_t f = 0; f < n_faces; ++f)
    for (int a = 0; a < nfn; ++a)
    {
      const int32_t t = M.node_dof_row_t[face_nodes[f * nfn + a]];
      if (t < 0) continue;
      const int64_t k = fill[size_t(sr_of_row[size_t(t)])]++;
      P.inc_face[size_t(k)] = int32_t(f);
      P.inc_loc[size_t(k)] = uint8_t(a);
    }
  return FCG_OK;
}

int build_compact_rows(const Maps& M, const int32_t* face_nodes, Plan& P, std::string& why)
{
  const int nfn = P.nfn;
  const int64_t nsr = P.nsr();
  P.s_ptr.assign(1, 0);
  P.s_col.clear();
  P.s_pos.clear();
  P.slot.assign(size_t(P.n_inc() * nfn), 0);
  P.max_row = 0;
  std::vector<int32_t> cols;
  for (int64_t i = 0; i < nsr; ++i)
  {
    cols.clear();
    for (int64_t q = P.inc_ptr[i]; q < P.inc_ptr[i + 1]; ++q)
    {
      const int32_t* fn = face_nodes + int64_t(P.inc_face[q]) * nfn;
      for (int b = 0; b < nfn; ++b)
      {
        const int32_t c = M.node_dof_col_t[fn[b]];
        if (c < 0 || c >= M.n_cols_t)
        {
          why = "face " + std::to_string(P.inc_face[q]) + ": a node's thermo column is outside the column map";
          return FCG_ERR_ARG;
        }
        cols.push_back(c);
      }
    }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    if (int(cols.size()) > max_compact_row(M.celltype))
    {
      why = "thermo row " + std::to_string(P.s_row[i]) + ": more than " +
            std::to_string(max_compact_row(M.celltype)) + " surface columns";
      return FCG_ERR_ARG;
    }
    // the positions in the k_TT row (columns ascending, as fcg_tsi_create's own search assumes)
    const int32_t trow = P.s_row[i];
    const int64_t btt = M.rowptr_tt[trow];
    const int32_t* ctt = M.col_tt + btt;
    const int64_t ltt = M.rowptr_tt[trow + 1] - btt;
    for (int32_t c : cols)
    {
      const int32_t* it = std::lower_bound(ctt, ctt + ltt, c);
      if (it == ctt + ltt || *it != c)
      {
        // name the lowest face of the row that brings the column
        int64_t face = -1;
        for (int64_t q = P.inc_ptr[i]; q < P.inc_ptr[i + 1] && face < 0; ++q)
          for (int b = 0; b < nfn; ++b)
            if (M.node_dof_col_t[face_nodes[int64_t(P.inc_face[q]) * nfn + b]] == c) face = P.inc_face[q];
        why = "face " + std::to_string(face) + ": the k_TT graph has no entry (row " + std::to_string(trow) +
              ", column " + std::to_string(c) + ")";
        return FCG_ERR_ARG;
      }
      P.s_col.push_back(c);
      P.s_pos.push_back(btt + (it - ctt));
    }
    const int32_t* crow = P.s_col.data() + P.s_ptr[i];
    const int64_t lrow = int64_t(cols.size());
    for (int64_t q = P.inc_ptr[i]; q < P.inc_ptr[i + 1]; ++q)
    {
      const int32_t* fn = face_nodes + int64_t(P.inc_face[q]) * nfn;
      for (int b = 0; b < nfn; ++b)
        P.slot[size_t(q * nfn + b)] =
            uint16_t(std::lower_bound(crow, crow + lrow, M.node_dof_col_t[fn[b]]) - crow);
    }
    P.s_ptr.push_back(int64_t(P.s_col.size()));
    P.max_row = std::max(P.max_row, int(lrow));
  }
  return FCG_OK;
}

std::vector<double> build_tables(int nfn)
{
  const int ngp = nfn;
  std::vector<double> tab(size_t(3 * ngp * nfn + ngp));
  double xg[9][2], wg[9];
  quad_rule(nfn, xg, wg);
  double* Ng = tab.data();
  double* dr = Ng + ngp * nfn;
  double* ds = dr + ngp * nfn;
  double* w = ds + ngp * nfn;
  for (int g = 0; g < ngp; ++g)
  {
    double N[9], dN[2][9];
    quad_shape(nfn, xg[g][0], xg[g][1], N, dN);
    for (int i = 0; i < nfn; ++i)
    {
      Ng[nfn * g + i] = N[i];
      dr[nfn * g + i] = dN[0][i];
      ds[nfn * g + i] = dN[1][i];
    }
    w[g] = wg[g];
  }
  return tab;
}

}  // namespace tsi_surface_plan
}  // namespace fcg
