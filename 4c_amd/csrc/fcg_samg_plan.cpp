// fcg_samg_plan.cpp -- the host plan of the scalar smoothed-aggregation AMG of K_TT (the numeric
// half is fcg_samg.hip).  K_TT is the scalar conduction operator, one DOF per node, its near-null
// space the constant: the textbook case of Vanek, Mandel, Brezina (Computing 56 (1996)), what
// MueLu builds for the thermal block of 4C's TSI block preconditioners.  Per level:
//
//  * aggregation: fcg_amg_aggregate on the level's graph (fcg_amg_setup.cpp); Dirichlet nodes are
//    `skip` nodes on level 0, so they join no aggregate and their prolongator rows stay empty;
//  * tentative prolongator: with the level's near-null-space vector B (level 0: B = 1 on the
//    aggregated nodes) node i has the single entry B_i / |B_agg(i)|_2 in column agg(i) and the
//    coarse near-null space is |B_agg|_2 -- on level 0, 1 / sqrt |agg| and sqrt |agg|.  Every
//    column has unit 2-norm;
//  * patterns: P on the pattern of A T (rows of unaggregated nodes empty), A P, P^T with the
//    permutation that gathers its values, A_c = P^T (A P), and the product plans of both products
//    (fcg_bsr_symbolic / fcg_bsr_transpose_pattern / fcg_bsr_product_plan at block size 1).
// Host only: no HIP header, no device call.
#include "fcg_samg_plan.hpp"

#include <algorithm>
#include <cmath>
#include <climits>

#include "fourc_gpu.h"

namespace fcg_samgs {
namespace {

bool symbolic(const int64_t* a_ptr, const int32_t* a_col, int64_t n_rows, const Pattern& B, Pattern& C)
{
  C.n_rows = n_rows;
  C.n_cols = B.n_cols;
  C.ptr.assign(size_t(n_rows) + 1, 0);
  const int64_t nnz = fcg_bsr_symbolic(n_rows, a_ptr, a_col, B.ptr.data(), B.col.data(), B.n_cols,
      C.ptr.data(), nullptr);
  if (nnz < 0) return false;
  C.col.assign(size_t(std::max<int64_t>(nnz, 1)), 0);
  if (fcg_bsr_symbolic(n_rows, a_ptr, a_col, B.ptr.data(), B.col.data(), B.n_cols, C.ptr.data(),
          C.col.data()) != nnz)
    return false;
  C.col.resize(size_t(nnz));
  return true;
}

bool product_plan(const int64_t* a_ptr, const int32_t* a_col, int64_t n_rows, const Pattern& B,
    const Pattern& C, ProductPlan& pl)
{
  pl.ptr.assign(size_t(C.nnz()) + 1, 0);
  const int64_t np = fcg_bsr_product_plan(n_rows, a_ptr, a_col, B.ptr.data(), B.col.data(),
      C.ptr.data(), C.col.data(), C.n_cols, pl.ptr.data(), nullptr, nullptr);
  if (np < 0) return false;
  pl.a.assign(size_t(std::max<int64_t>(np, 1)), 0);
  pl.b.assign(size_t(std::max<int64_t>(np, 1)), 0);
  if (fcg_bsr_product_plan(n_rows, a_ptr, a_col, B.ptr.data(), B.col.data(), C.ptr.data(),
          C.col.data(), C.n_cols, pl.ptr.data(), pl.a.data(), pl.b.data()) != np)
    return false;
  pl.a.resize(size_t(np));
  pl.b.resize(size_t(np));
  return true;
}

}  // namespace

bool build_plan(int64_t n, const int64_t* rowptr, const int32_t* col, const uint8_t* skip,
    int64_t coarse_max, int max_levels, Plan& out, std::string& err)
{
  out = Plan();
  if (n < 0 || (n > 0 && (!rowptr || !col)) || (n > 0 && rowptr[0] != 0))
  {
    err = "no graph";
    return false;
  }
  if (n > INT32_MAX)
  {
    err = "more than 2^31 - 1 rows";
    return false;
  }
  for (int64_t i = 0; i < n; ++i)
  {
    if (rowptr[i + 1] < rowptr[i])
    {
      err = "rowptr decreases at row " + std::to_string(i);
      return false;
    }
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if (col[k] < 0 || col[k] >= n || (k > rowptr[i] && col[k] <= col[k - 1]))
      {
        err = "row " + std::to_string(i) + ": a column outside the map or columns not ascending";
        return false;
      }
    out.widest0 = int(std::max<int64_t>(out.widest0, rowptr[i + 1] - rowptr[i]));
  }
  out.n0 = n;
  // the current level: its graph, near-null-space vector and skip marks
  const int64_t* a_ptr = rowptr;
  const int32_t* a_col = col;
  int64_t na = n;
  std::vector<double> ns(size_t(n), 1.0);
  for (int level = 1; level < max_levels && na > coarse_max; ++level)
  {
    PlanStep st;
    st.agg.assign(size_t(na), -1);
    st.n_agg = fcg_amg_aggregate(na, a_ptr, a_col, level == 1 ? skip : nullptr, st.agg.data());
    if (st.n_agg < 0)
    {
      err = "aggregation failed on level " + std::to_string(level - 1);
      return false;
    }
    if (st.n_agg == 0 || st.n_agg >= na) break;  // nothing to coarsen (all Dirichlet), or no gain
    // tentative prolongator: the aggregates' nodes in ascending order, one fixed summation order
    st.ns_c.assign(size_t(st.n_agg), 0.0);
    for (int64_t i = 0; i < na; ++i)
      if (st.agg[size_t(i)] >= 0) st.ns_c[size_t(st.agg[size_t(i)])] += ns[size_t(i)] * ns[size_t(i)];
    for (auto& v : st.ns_c) v = std::sqrt(v);
    st.tent.assign(size_t(na), 0.0);
    for (int64_t i = 0; i < na; ++i)
      if (st.agg[size_t(i)] >= 0) st.tent[size_t(i)] = ns[size_t(i)] / st.ns_c[size_t(st.agg[size_t(i)])];
    // P on the pattern of A T: the aggregates of row i's neighbours, empty for an unaggregated i
    st.P.n_rows = na;
    st.P.n_cols = st.n_agg;
    st.P.ptr.assign(size_t(na) + 1, 0);
    std::vector<int32_t> row;
    for (int64_t i = 0; i < na; ++i)
    {
      if (st.agg[size_t(i)] >= 0)
      {
        row.clear();
        for (int64_t k = a_ptr[i]; k < a_ptr[i + 1]; ++k)
          if (st.agg[size_t(a_col[k])] >= 0) row.push_back(st.agg[size_t(a_col[k])]);
        row.push_back(st.agg[size_t(i)]);  // T's own entry, should the graph lack the diagonal
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        st.P.col.insert(st.P.col.end(), row.begin(), row.end());
        st.p_row.insert(st.p_row.end(), row.size(), int32_t(i));
      }
      st.P.ptr[size_t(i) + 1] = int64_t(st.P.col.size());
    }
    if (st.P.nnz() > INT32_MAX)
    {
      err = "prolongator with more than 2^31 - 1 entries";
      return false;
    }
    // A P, P^T, A_c = P^T (A P)
    if (!symbolic(a_ptr, a_col, na, st.P, st.AP) || !product_plan(a_ptr, a_col, na, st.P, st.AP, st.pAP))
    {
      err = "pattern of A P on level " + std::to_string(level - 1);
      return false;
    }
    st.Pt.n_rows = st.n_agg;
    st.Pt.n_cols = na;
    st.Pt.ptr.assign(size_t(st.n_agg) + 1, 0);
    st.Pt.col.assign(size_t(st.P.nnz()), 0);
    st.perm.assign(size_t(st.P.nnz()), 0);
    if (fcg_bsr_transpose_pattern(na, st.n_agg, st.P.ptr.data(), st.P.col.data(), st.Pt.ptr.data(),
            st.Pt.col.data(), st.perm.data()) != FCG_OK)
    {
      err = "pattern of P^T on level " + std::to_string(level - 1);
      return false;
    }
    if (!symbolic(st.Pt.ptr.data(), st.Pt.col.data(), st.n_agg, st.AP, st.Ac) ||
        !product_plan(st.Pt.ptr.data(), st.Pt.col.data(), st.n_agg, st.AP, st.Ac, st.pAc))
    {
      err = "pattern of P^T A P on level " + std::to_string(level - 1);
      return false;
    }
    ns = st.ns_c;
    out.steps.push_back(std::move(st));
    const PlanStep& done = out.steps.back();  // (the vectors' buffers moved with the step)
    a_ptr = done.Ac.ptr.data();
    a_col = done.Ac.col.data();
    na = done.n_agg;
  }
  return true;
}

}  // namespace fcg_samgs
