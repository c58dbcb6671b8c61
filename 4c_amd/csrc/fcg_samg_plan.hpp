// fcg_samg_plan.hpp -- the host plan of the scalar smoothed-aggregation AMG (fcg_samg_plan.cpp):
// every pattern, permutation and product plan of the hierarchy, built once per graph.  No HIP:
// tests/cxx/samg_plan_check.cpp links the plan with g++ alone.  Not part of the public ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcg_samgs {

struct Pattern {
  int64_t n_rows = 0, n_cols = 0;
  std::vector<int64_t> ptr;  // [n_rows + 1]
  std::vector<int32_t> col;  // ascending per row
  int64_t nnz() const { return ptr.empty() ? 0 : ptr.back(); }
  int widest() const
  {
    int64_t w = 0;
    for (int64_t i = 0; i < n_rows; ++i) w = ptr[size_t(i) + 1] - ptr[size_t(i)] > w ? ptr[size_t(i) + 1] - ptr[size_t(i)] : w;
    return int(w);
  }
};

// C = A B on C's pattern: entry c sums vals_a[a[t]] * vals_b[b[t]] for t in [ptr[c], ptr[c + 1])
struct ProductPlan {
  std::vector<int64_t> ptr;
  std::vector<int32_t> a, b;
};

// level l -> l + 1
struct PlanStep {
  int64_t n_agg = 0;
  std::vector<int32_t> agg;   // [n fine] aggregate of every node, -1: none (a Dirichlet node)
  std::vector<double> tent;   // [n fine] the node's entry of the tentative prolongator (0: none)
  std::vector<double> ns_c;   // [n_agg] the coarse near-null space
  Pattern P;                  // pattern of A T, the rows of unaggregated nodes empty
  std::vector<int32_t> p_row; // [nnz P] row of every entry
  Pattern AP, Pt, Ac;         // A P, P^T, P^T (A P)
  std::vector<int64_t> perm;  // Pt entry t = P entry perm[t]
  ProductPlan pAP, pAc;
};

// level 0 is the caller's graph (not copied); level l >= 1 has the pattern steps[l - 1].Ac
struct Plan {
  int64_t n0 = 0;
  int widest0 = 0;  // longest row of level 0
  std::vector<PlanStep> steps;
};

// rowptr / col: the level-0 graph (n rows, columns ascending per row); skip[i] != 0: a Dirichlet
// node.  Coarsens until a level has at most coarse_max rows or max_levels levels exist.  Returns
// false with err set on a malformed graph.
bool build_plan(int64_t n, const int64_t* rowptr, const int32_t* col, const uint8_t* skip,
    int64_t coarse_max, int max_levels, Plan& out, std::string& err);

}  // namespace fcg_samgs
