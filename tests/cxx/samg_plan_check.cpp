// samg_plan_check -- the host plan of the scalar AMG (4c_amd/csrc/fcg_samg_plan.cpp) checked on a
// CPU on the node graph of the hex8 (6, 5, 4) box with the x = 0 face skipped: aggregates,
// tentative prolongator, patterns and product plans of every level.  Links the plan, the graph
// routines of fcg_amg_setup.cpp and the box-mesh builder only (no libfourc_gpu, no ROCm).  Prints
// PASS, or the failed condition with the offending index (exit 1).  TEST INFRASTRUCTURE.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "fcg_samg_plan.hpp"
#include "fourc_gpu.h"

using namespace fcg_samgs;

#define CHECK(cond, index)                                                                          \
  do                                                                                                \
  {                                                                                                 \
    if (!(cond))                                                                                    \
    {                                                                                               \
      std::printf("FAIL %s at index %lld (line %d)\n", #cond, (long long)(index), __LINE__);        \
      std::exit(1);                                                                                 \
    }                                                                                               \
  } while (0)

namespace {

// C's pattern holds every structural product of A B, columns ascending; every plan pair lands on
// its entry and the plan lists each product once
void check_product(const int64_t* a_ptr, const int32_t* a_col, int64_t n_rows, const Pattern& B,
    const Pattern& C, const ProductPlan& pl)
{
  CHECK(C.n_rows == n_rows && C.n_cols == B.n_cols, n_rows);
  CHECK(int64_t(C.ptr.size()) == n_rows + 1 && int64_t(pl.ptr.size()) == C.nnz() + 1, n_rows);
  int64_t products = 0;
  for (int64_t i = 0; i < n_rows; ++i)
  {
    for (int64_t c = C.ptr[i]; c < C.ptr[i + 1]; ++c)
    {
      CHECK(C.col[c] >= 0 && C.col[c] < C.n_cols, c);
      CHECK(c == C.ptr[i] || C.col[c] > C.col[c - 1], c);
    }
    for (int64_t k = a_ptr[i]; k < a_ptr[i + 1]; ++k)
      for (int64_t q = B.ptr[a_col[k]]; q < B.ptr[a_col[k] + 1]; ++q)
      {
        ++products;
        CHECK(std::binary_search(C.col.begin() + C.ptr[i], C.col.begin() + C.ptr[i + 1], B.col[q]), i);
      }
    for (int64_t c = C.ptr[i]; c < C.ptr[i + 1]; ++c)
    {
      CHECK(pl.ptr[c + 1] >= pl.ptr[c], c);
      for (int64_t t = pl.ptr[c]; t < pl.ptr[c + 1]; ++t)
      {
        const int64_t a = pl.a[t], b = pl.b[t];
        CHECK(a >= a_ptr[i] && a < a_ptr[i + 1], t);
        CHECK(b >= B.ptr[a_col[a]] && b < B.ptr[a_col[a] + 1], t);
        CHECK(B.col[b] == C.col[c], t);
        CHECK(t == pl.ptr[c] || a > pl.a[t - 1], t);  // A's row order, each product once
      }
    }
  }
  CHECK(pl.ptr.back() == products && int64_t(pl.a.size()) == products && int64_t(pl.b.size()) == products, products);
}

}  // namespace

int main()
{
  fcg_box b{};
  b.celltype = FCG_HEX8;
  b.interval[0] = 6; b.interval[1] = 5; b.interval[2] = 4;
  for (int k = 0; k < 3; ++k) b.upper[k] = 1.0;
  b.jitter = 0.1;
  b.jitter_seed = 20251015;
  fcg_box_mesh* bm = nullptr;
  CHECK(fcg_box_mesh_create_ex(&b, 0, 1, FCG_BOX_GHOSTED, &bm) == FCG_OK, 0);
  fcg_desc d;
  CHECK(fcg_box_mesh_desc(bm, FCG_LINEAR, 210.0, 0.3, 0, &d) == FCG_OK, 0);
  // the node graph: node t = rows 3t .. 3t + 2, its neighbours the column triples of row 3t
  const int64_t n = d.n_rows / 3;
  CHECK(n == 7 * 6 * 5, n);
  std::vector<int64_t> ptr(size_t(n) + 1, 0);
  std::vector<int32_t> col;
  for (int64_t t = 0; t < n; ++t)
  {
    for (int64_t k = d.rowptr[3 * t]; k < d.rowptr[3 * t + 1]; k += 3) col.push_back(d.col_lid[k] / 3);
    ptr[size_t(t) + 1] = int64_t(col.size());
  }
  std::vector<uint8_t> skip(size_t(n), 0);
  int64_t n_skip = 0;
  for (int64_t v = 0; v < d.n_node; ++v)
    if (d.node_dof_row[v] >= 0 && d.node_x[3 * v] == 0.0)
    {
      skip[size_t(d.node_dof_row[v] / 3)] = 1;
      ++n_skip;
    }
  CHECK(n_skip == 6 * 5, n_skip);

  Plan plan;
  std::string err;
  CHECK(build_plan(n, ptr.data(), col.data(), skip.data(), 4, 10, plan, err), 0);
  CHECK(plan.n0 == n && plan.widest0 == 27, plan.widest0);
  CHECK(plan.steps.size() >= 2, plan.steps.size());  // at least three levels

  const int64_t* a_ptr = ptr.data();
  const int32_t* a_col = col.data();
  int64_t na = n;
  std::vector<double> ns(size_t(n), 1.0);
  for (size_t l = 0; l < plan.steps.size(); ++l)
  {
    const PlanStep& st = plan.steps[l];
    CHECK(st.n_agg > 0 && st.n_agg < na, l);  // the level sizes decrease
    CHECK(int64_t(st.agg.size()) == na && int64_t(st.tent.size()) == na, l);
    // every node that is not skipped in exactly one aggregate, skipped nodes in none
    std::vector<int64_t> size(size_t(st.n_agg), 0);
    std::vector<double> norm2(size_t(st.n_agg), 0.0), b2(size_t(st.n_agg), 0.0);
    for (int64_t i = 0; i < na; ++i)
    {
      const bool skipped = l == 0 && skip[size_t(i)];
      if (skipped)
      {
        CHECK(st.agg[i] == -1 && st.tent[i] == 0.0, i);
        CHECK(st.P.ptr[i + 1] == st.P.ptr[i], i);  // an empty prolongator row
        continue;
      }
      CHECK(st.agg[i] >= 0 && st.agg[i] < st.n_agg, i);
      ++size[size_t(st.agg[i])];
      norm2[size_t(st.agg[i])] += st.tent[i] * st.tent[i];
      b2[size_t(st.agg[i])] += ns[size_t(i)] * ns[size_t(i)];
    }
    for (int64_t a = 0; a < st.n_agg; ++a)
    {
      CHECK(size[size_t(a)] > 0, a);
      CHECK(std::fabs(norm2[size_t(a)] - 1.0) <= 8 * 2.3e-16 * double(size[size_t(a)]), a);  // unit columns
      CHECK(std::fabs(st.ns_c[size_t(a)] - std::sqrt(b2[size_t(a)])) <= 4e-16 * st.ns_c[size_t(a)], a);
      if (l == 0) CHECK(std::fabs(st.ns_c[size_t(a)] - std::sqrt(double(size[size_t(a)]))) <= 1e-15 * st.ns_c[size_t(a)], a);
    }
    if (l == 0)
      for (int64_t i = 0; i < na; ++i)
        if (st.agg[i] >= 0) CHECK(std::fabs(st.tent[i] - 1.0 / std::sqrt(double(size[size_t(st.agg[i])]))) <= 1e-15, i);
    // P: the pattern of A T on the aggregated rows, ascending, with the row of every entry
    CHECK(st.P.n_rows == na && st.P.n_cols == st.n_agg && int64_t(st.p_row.size()) == st.P.nnz(), l);
    for (int64_t i = 0; i < na; ++i)
    {
      std::set<int32_t> want;
      if (st.agg[i] >= 0)
      {
        want.insert(st.agg[i]);
        for (int64_t k = a_ptr[i]; k < a_ptr[i + 1]; ++k)
          if (st.agg[a_col[k]] >= 0) want.insert(st.agg[a_col[k]]);
      }
      CHECK(st.P.ptr[i + 1] - st.P.ptr[i] == int64_t(want.size()), i);
      CHECK(std::equal(want.begin(), want.end(), st.P.col.begin() + st.P.ptr[i]), i);
      for (int64_t e = st.P.ptr[i]; e < st.P.ptr[i + 1]; ++e) CHECK(st.p_row[e] == i, e);
    }
    // P^T and its permutation
    CHECK(st.Pt.n_rows == st.n_agg && st.Pt.n_cols == na && st.Pt.nnz() == st.P.nnz(), l);
    std::vector<char> seen(size_t(st.P.nnz()), 0);
    for (int64_t j = 0; j < st.n_agg; ++j)
      for (int64_t t = st.Pt.ptr[j]; t < st.Pt.ptr[j + 1]; ++t)
      {
        const int64_t e = st.perm[t];
        CHECK(e >= 0 && e < st.P.nnz() && !seen[size_t(e)], t);
        seen[size_t(e)] = 1;
        CHECK(st.P.col[e] == j && st.p_row[e] == st.Pt.col[t], t);
        CHECK(t == st.Pt.ptr[j] || st.Pt.col[t] > st.Pt.col[t - 1], t);
      }
    check_product(a_ptr, a_col, na, st.P, st.AP, st.pAP);
    check_product(st.Pt.ptr.data(), st.Pt.col.data(), st.n_agg, st.AP, st.Ac, st.pAc);
    CHECK(st.Ac.n_rows == st.n_agg && st.Ac.n_cols == st.n_agg, l);
    std::printf("level %zu: %lld rows -> %lld aggregates, P %lld, A P %lld, A_c %lld entries\n", l,
        (long long)na, (long long)st.n_agg, (long long)st.P.nnz(), (long long)st.AP.nnz(),
        (long long)st.Ac.nnz());
    a_ptr = st.Ac.ptr.data();
    a_col = st.Ac.col.data();
    na = st.n_agg;
    ns = st.ns_c;
  }
  CHECK(na <= 4 || plan.steps.size() == 9, na);
  // a malformed graph is refused
  std::vector<int32_t> bad(col);
  std::swap(bad[0], bad[1]);
  CHECK(!build_plan(n, ptr.data(), bad.data(), skip.data(), 4, 10, plan, err) && !err.empty(), 0);
  fcg_box_mesh_destroy(bm);
  std::printf("PASS\n");
  return 0;
}
