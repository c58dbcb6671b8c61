// fcg_tsi_plan.cpp -- the host stages of fcg_tsi_create (fcg_tsi_plan.hpp).  No HIP: this unit
// compiles and links with a host compiler alone.
#include "fcg_tsi_plan.hpp"

#include <algorithm>
#include <cstring>

#include "fcg_shape.hpp"

namespace fcg {
namespace tsi_plan {

int check_descriptor(const fcg_tsi_desc* D, std::string& why)
{
  if (D->abi_version != FCG_ABI_VERSION)
  {
    why = "abi_version mismatch";
    return FCG_ERR_ARG;
  }
  if (D->celltype != FCG_HEX8 && D->celltype != FCG_HEX27)
  {
    why = "unsupported celltype";
    return FCG_ERR_ARG;
  }
  // Mat::PAR::ThermoStVenantKirchhoff (4C_mat_thermostvenantkirchhoff.cpp:35-36)
  if (!(D->youngs > 0.0) || D->poisson >= 0.5 || D->poisson < -1.0)
  {
    why = "Poisson's ratio must be in [-1;0.5) and Young's modulus > 0";
    return FCG_ERR_ARG;
  }
  const int npe = npe_of(D);
  if (D->n_ele < 0 || D->n_node < 0 || D->n_ele >= (int64_t(1) << 31) ||
      (D->n_ele > 0 && (!D->ele_nodes || !D->node_x || !D->node_dof_col_s || !D->node_dof_col_t ||
                           !D->node_dof_row_s || !D->node_dof_row_t)) ||
      (D->n_rows_s > 0 && (!D->rowptr_st || !D->col_st)) ||
      (D->n_rows_t > 0 && (!D->rowptr_ts || !D->col_ts || !D->rowptr_tt || !D->col_tt)))
  {
    why = "invalid descriptor arrays/sizes";
    return FCG_ERR_ARG;
  }
  for (int64_t i = 0; i < D->n_ele * npe; ++i)
    if (D->ele_nodes[i] < 0 || D->ele_nodes[i] >= D->n_node)
    {
      why = "element references a node outside [0, n_node)";
      return FCG_ERR_ARG;
    }
  return FCG_OK;
}

int build_node_rows(const fcg_tsi_desc* D, NodeRows& N, std::string& why)
{
  std::vector<int32_t>& rownodes = N.rownodes;
  rownodes.clear();
  for (int64_t n = 0; n < D->n_node; ++n)
  {
    const int32_t rs = D->node_dof_row_s[n], rt = D->node_dof_row_t[n];
    const int32_t cs = D->node_dof_col_s[n], ct = D->node_dof_col_t[n];
    if ((rs >= 0) != (rt >= 0) || cs < 0 || cs + 3 > D->n_cols_s || ct < 0 || ct >= D->n_cols_t ||
        rs + 3 > D->n_rows_s || rt >= D->n_rows_t)
    {
      why = "node DOF maps out of range, or a node owned in one field only";
      return FCG_ERR_ARG;
    }
    if (rs >= 0) rownodes.push_back(int32_t(n));
  }
  std::sort(rownodes.begin(), rownodes.end(),
      [&](int32_t a, int32_t b) { return D->node_dof_row_s[a] < D->node_dof_row_s[b]; });
  const int64_t nrn = N.nrn();
  N.rn_of_node.assign(D->n_node, -1);
  N.srow.resize(nrn);
  N.trow.resize(nrn);
  for (int64_t r = 0; r < nrn; ++r)
  {
    N.rn_of_node[rownodes[r]] = int32_t(r);
    N.srow[r] = D->node_dof_row_s[rownodes[r]];
    N.trow[r] = D->node_dof_row_t[rownodes[r]];
  }
  return FCG_OK;
}

int check_row_layout(const fcg_tsi_desc* D, const NodeRows& N, std::string& why)
{
  const int maxn = max_neighbours(D);
  for (int64_t r = 0; r < N.nrn(); ++r)
  {
    const int64_t* p = D->rowptr_st + N.srow[r];
    const int64_t l = p[1] - p[0];
    if (l > maxn || p[2] - p[1] != l || p[3] - p[2] != l ||
        std::memcmp(D->col_st + p[0], D->col_st + p[1], sizeof(int32_t) * l) != 0 ||
        std::memcmp(D->col_st + p[0], D->col_st + p[2], sizeof(int32_t) * l) != 0 ||
        D->rowptr_ts[N.trow[r] + 1] - D->rowptr_ts[N.trow[r]] > 3 * maxn ||
        D->rowptr_tt[N.trow[r] + 1] - D->rowptr_tt[N.trow[r]] > maxn)
    {
      why = "k_ST/k_TS/k_TT rows do not have the node-graph layout";
      return FCG_ERR_ARG;
    }
  }
  return FCG_OK;
}

int build_incidences(const fcg_tsi_desc* D, const NodeRows& N, Incidences& I, std::string& why)
{
  const int npe = npe_of(D);
  const int64_t nrn = N.nrn();
  I.inc_ptr.assign(nrn + 1, 0);
  for (int64_t i = 0; i < D->n_ele * npe; ++i)
  {
    const int32_t rn = N.rn_of_node[D->ele_nodes[i]];
    if (rn >= 0) I.inc_ptr[rn + 1]++;
  }
  for (int64_t r = 0; r < nrn; ++r) I.inc_ptr[r + 1] += I.inc_ptr[r];
  I.n_inc = I.inc_ptr[nrn];
  if (I.n_inc >= (int64_t(1) << 31))
  {
    why = "too many incidences for one context (> 2^31)";
    return FCG_ERR_ARG;
  }
  I.inc_of.assign(D->n_ele * npe, -1);
  I.inc_ele.resize(I.n_inc);
  I.inc_loc.resize(I.n_inc);
  std::vector<int64_t> fill(I.inc_ptr.begin(), I.inc_ptr.end() - 1);
  for (int64_t e = 0; e < D->n_ele; ++e)
    for (int a = 0; a < npe; ++a)
    {
      const int32_t rn = N.rn_of_node[D->ele_nodes[e * npe + a]];
      if (rn < 0) continue;
      const int64_t k = fill[rn]++;
      I.inc_of[e * npe + a] = int32_t(k);
      I.inc_ele[k] = int32_t(e);
      I.inc_loc[k] = uint8_t(a);
    }
  return FCG_OK;
}

// column positions (SparseMatrix::assemble's row search, 4C_linalg_sparsematrix.cpp:471-543,
// resolved once)
int build_positions(const fcg_tsi_desc* D, const NodeRows& N, Incidences& I, std::string& why)
{
  const int npe = npe_of(D);
  I.pos_st.resize(I.n_inc * npe);
  I.pos_ts.resize(I.n_inc * npe);
  I.pos_tt.resize(I.n_inc * npe);
  for (int64_t r = 0; r < N.nrn(); ++r)
  {
    const int32_t srow = N.srow[r], trow = N.trow[r];
    const int32_t* cst = D->col_st + D->rowptr_st[srow];
    const int64_t lst = D->rowptr_st[srow + 1] - D->rowptr_st[srow];
    const int32_t* cts = D->col_ts + D->rowptr_ts[trow];
    const int64_t lts = D->rowptr_ts[trow + 1] - D->rowptr_ts[trow];
    const int32_t* ctt = D->col_tt + D->rowptr_tt[trow];
    const int64_t ltt = D->rowptr_tt[trow + 1] - D->rowptr_tt[trow];
    for (int64_t k = I.inc_ptr[r]; k < I.inc_ptr[r + 1]; ++k)
    {
      const int32_t* en = D->ele_nodes + int64_t(I.inc_ele[k]) * npe;
      for (int b = 0; b < npe; ++b)
      {
        const int32_t tc = D->node_dof_col_t[en[b]], sc = D->node_dof_col_s[en[b]];
        const int32_t* i1 = std::lower_bound(cst, cst + lst, tc);
        const int32_t* i2 = std::lower_bound(cts, cts + lts, sc);
        const int32_t* i3 = std::lower_bound(ctt, ctt + ltt, tc);
        if (i1 == cst + lst || *i1 != tc || i3 == ctt + ltt || *i3 != tc ||
            i2 + 3 > cts + lts || i2[0] != sc || i2[1] != sc + 1 || i2[2] != sc + 2)
        {
          why = "a TSI block graph lacks an element coupling, or a node's "
                "displacement columns are not contiguous";
          return FCG_ERR_ARG;
        }
        I.pos_st[k * npe + b] = uint16_t(i1 - cst);
        I.pos_ts[k * npe + b] = uint16_t(i2 - cts);
        I.pos_tt[k * npe + b] = uint16_t(i3 - ctt);
      }
    }
  }
  return FCG_OK;
}

// hex_8point / hex_27point: the thermo element's DisTypeToOptGaussRule
// (4C_thermo_ele_impl_utils.hpp:28-50) is the solid's rule
std::vector<double> build_tables(int32_t celltype)
{
  const int npe = celltype == FCG_HEX27 ? 27 : 8;
  const int ct = celltype == FCG_HEX27 ? kHex27 : kHex8;
  std::vector<double> tab(npe * npe * 3 * 2 + npe * npe + npe);
  double xi[81], w[27], xn[81];
  gauss_rule(ct, xi, w);
  node_param_coords(ct, xn);
  double* dNg = tab.data();
  double* Ng = dNg + npe * npe * 3;
  double* dNn = Ng + npe * npe;
  double* wg = dNn + npe * npe * 3;
  for (int g = 0; g < npe; ++g)
  {
    shape_deriv(ct, &xi[3 * g], dNg + 3 * npe * g);
    shape_values(ct, &xi[3 * g], Ng + npe * g);
    shape_deriv(ct, &xn[3 * g], dNn + 3 * npe * g);
    wg[g] = w[g];
  }
  return tab;
}

bool node_consistent(const fcg_tsi_desc* D)
{
  bool ok = D->n_rows_s == 3 * D->n_rows_t && D->n_cols_s == 3 * D->n_cols_t;
  for (int64_t n = 0; ok && n < D->n_node; ++n)
    ok = D->node_dof_col_s[n] == 3 * D->node_dof_col_t[n] &&
         D->node_dof_row_s[n] == (D->node_dof_row_t[n] < 0 ? D->node_dof_row_s[n] : 3 * D->node_dof_row_t[n]);
  for (int64_t t = 0; ok && t < D->n_rows_t; ++t)
  {
    const int64_t b = D->rowptr_tt[t], lt = D->rowptr_tt[t + 1] - b;
    ok = D->rowptr_ts[t] == 3 * b && D->rowptr_ts[t + 1] - D->rowptr_ts[t] == 3 * lt;
    for (int d = 0; ok && d < 3; ++d)
      ok = D->rowptr_st[3 * t + d] == 3 * b + d * lt &&
           std::memcmp(D->col_st + D->rowptr_st[3 * t + d], D->col_tt + b, sizeof(int32_t) * lt) == 0;
    for (int64_t j = 0; ok && j < 3 * lt; ++j)
      ok = D->col_ts[3 * b + j] == 3 * D->col_tt[b + j / 3] + int32_t(j % 3);
  }
  if (ok && D->n_rows_t > 0)
    ok = D->rowptr_st[D->n_rows_s] == 3 * D->rowptr_tt[D->n_rows_t] &&
         D->rowptr_ts[D->n_rows_t] == 3 * D->rowptr_tt[D->n_rows_t];
  return ok;
}

int max_row_tt(const fcg_tsi_desc* D)
{
  int longest = 0;
  for (int64_t t = 0; t < D->n_rows_t; ++t)
    longest = std::max(longest, int(D->rowptr_tt[t + 1] - D->rowptr_tt[t]));
  return longest;
}

Constants build_constants(const fcg_tsi_desc* D)
{
  Constants C;
  C.nnz_st = D->n_rows_s ? D->rowptr_st[D->n_rows_s] : 0;
  C.nnz_ts = D->n_rows_t ? D->rowptr_ts[D->n_rows_t] : 0;
  C.nnz_tt = D->n_rows_t ? D->rowptr_tt[D->n_rows_t] : 0;
  // st_modulus (4C_mat_thermostvenantkirchhoff.cpp:331-369)
  {
    const double c1 = D->youngs / (1.0 + D->poisson);
    const double b1 = c1 * D->poisson / (1.0 - 2.0 * D->poisson);
    const double mu = 0.5 * c1, lambda = b1;
    C.m = (-1.0) * (2.0 * mu + 3.0 * lambda) * D->thexpans;
    C.lambda = lambda;
    C.mu = mu;
  }
  if (!D->ele_gid)
  {
    C.ele_gid.resize(D->n_ele);
    for (int64_t e = 0; e < D->n_ele; ++e) C.ele_gid[e] = int32_t(e);
  }
  return C;
}

}  // namespace tsi_plan
}  // namespace fcg
