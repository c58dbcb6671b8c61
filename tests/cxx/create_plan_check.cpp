// create_plan_check -- the host plans of fcg_create (4c_amd/csrc/fcg_create_plan.cpp) checked
// against the connectivity itself, on a CPU: the gather records and their tmap nibbles, the hex27
// slab ring and the slab-size rule.  Links the plan unit and the box-mesh builder only (no
// libfourc_gpu, no ROCm).  Prints PASS, or the failed condition with the offending index (exit 1).
// TEST INFRASTRUCTURE.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "fcg_create_plan.hpp"
#include "fourc_gpu.h"

namespace plan = fcg::create;

namespace {

const char* g_mesh = "";

#define CHECK(cond, index)                                                                     \
  do                                                                                           \
  {                                                                                            \
    if (!(cond))                                                                               \
    {                                                                                          \
      std::printf("FAIL [%s] %s at index %lld (line %d)\n", g_mesh, #cond, (long long)(index), \
          __LINE__);                                                                           \
      std::exit(1);                                                                            \
    }                                                                                          \
  } while (0)

// a descriptor that owns its arrays
struct Mesh {
  fcg_desc d;
  std::vector<int32_t> ele_nodes, dof_col, dof_row, col_lid;
  std::vector<double> x;
  std::vector<int64_t> rowptr;
  int npe() const { return d.celltype == FCG_HEX27 ? 27 : 8; }
  void point()
  {
    d.n_ele = int64_t(ele_nodes.size()) / npe();
    d.n_node = int64_t(dof_col.size());
    d.n_rows = int64_t(rowptr.size()) - 1;
    d.ele_nodes = ele_nodes.data();
    d.ele_gid = nullptr;
    d.node_x = x.data();
    d.node_dof_col = dof_col.data();
    d.node_dof_row = dof_row.data();
    d.rowptr = rowptr.data();
    d.col_lid = col_lid.data();
    d.ele_ijk = nullptr;
  }
};

Mesh box(int celltype, int nx, int ny, int nz, int rank, int nranks, double jitter)
{
  fcg_box b{};
  b.celltype = celltype;
  b.interval[0] = nx; b.interval[1] = ny; b.interval[2] = nz;
  for (int k = 0; k < 3; ++k) b.upper[k] = 1.0;
  b.jitter = jitter;
  b.jitter_seed = 20251015;
  fcg_box_mesh* bm = nullptr;
  CHECK(fcg_box_mesh_create_ex(&b, rank, nranks, FCG_BOX_GHOSTED, &bm) == FCG_OK, rank);
  Mesh m;
  CHECK(fcg_box_mesh_desc(bm, FCG_LINEAR, 210.0, 0.3, 0, &m.d) == FCG_OK, rank);
  const fcg_desc& s = m.d;
  m.ele_nodes.assign(s.ele_nodes, s.ele_nodes + s.n_ele * m.npe());
  m.x.assign(s.node_x, s.node_x + 3 * s.n_node);
  m.dof_col.assign(s.node_dof_col, s.node_dof_col + s.n_node);
  m.dof_row.assign(s.node_dof_row, s.node_dof_row + s.n_node);
  m.rowptr.assign(s.rowptr, s.rowptr + s.n_rows + 1);
  m.col_lid.assign(s.col_lid, s.col_lid + s.rowptr[s.n_rows]);
  m.point();
  fcg_box_mesh_destroy(bm);
  return m;
}

// node and element numbers permuted (the DOF LIDs, hence the graph, stay)
Mesh permuted(const Mesh& a, unsigned seed)
{
  std::mt19937 rng(seed);
  std::vector<int32_t> pn(a.d.n_node), pe(a.d.n_ele);
  std::iota(pn.begin(), pn.end(), 0);
  std::iota(pe.begin(), pe.end(), 0);
  std::shuffle(pn.begin(), pn.end(), rng);  // old node -> new node
  std::shuffle(pe.begin(), pe.end(), rng);  // old element -> new element
  Mesh m = a;
  for (int64_t n = 0; n < a.d.n_node; ++n)
  {
    for (int k = 0; k < 3; ++k) m.x[3 * pn[n] + k] = a.x[3 * n + k];
    m.dof_col[pn[n]] = a.dof_col[n];
    m.dof_row[pn[n]] = a.dof_row[n];
  }
  for (int64_t e = 0; e < a.d.n_ele; ++e)
    for (int b = 0; b < 8; ++b) m.ele_nodes[8 * pe[e] + b] = pn[a.ele_nodes[8 * e + b]];
  m.point();
  return m;
}

// the stages of fcg_create up to the incidence positions
struct Stages {
  plan::NodeRows rows;
  plan::PathChoice choice;
  plan::Incidences inc;
};
void run_stages(const fcg_desc* d, Stages& S)
{
  std::string why;
  CHECK(plan::check_descriptor(d, why) == FCG_OK, 0);
  CHECK(plan::build_node_rows(d, S.rows, why) == FCG_OK, 0);
  CHECK(plan::choose_path(d, S.rows, 256, S.choice, why) == FCG_OK, 0);
  CHECK(plan::build_incidences(d, S.rows, S.choice, S.inc, why) == FCG_OK, 0);
  CHECK(plan::build_incidence_positions(d, S.rows, S.choice, S.inc, why) == FCG_OK, 0);
  plan::build_operator_support(d, S.rows);
}

void check_gather(const char* name, Mesh& m)
{
  g_mesh = name;
  m.d.path = FCG_PATH_GATHER;
  const fcg_desc* d = &m.d;
  Stages S;
  run_stages(d, S);
  CHECK(S.choice.gather && S.choice.path() == FCG_PATH_GATHER, 0);
  plan::GatherHost G;
  plan::build_gather_plan(d, S.rows, S.inc, G);
  const int64_t n_ele = d->n_ele, n_rec = G.n_rec;
  const int32_t* kcol = plan::kcol_of(d);

  // element data in storage-slot order
  CHECK(int64_t(G.eorig.size()) == n_ele && int64_t(G.ex.size()) == 24 * n_ele &&
            int64_t(G.edof.size()) == 8 * n_ele, n_ele);
  std::vector<int> hit(n_ele, 0);
  for (int64_t s = 0; s < n_ele; ++s)
  {
    CHECK(G.eorig[s] >= 0 && G.eorig[s] < n_ele, s);
    CHECK(++hit[G.eorig[s]] == 1, s);
    for (int b = 0; b < 8; ++b)
    {
      const int32_t nd = m.ele_nodes[8 * G.eorig[s] + b];
      for (int k = 0; k < 3; ++k) CHECK(G.ex[24 * s + 3 * b + k] == m.x[3 * nd + k], 24 * s + 3 * b + k);
      CHECK(G.edof[8 * s + b] == m.dof_col[nd], 8 * s + b);
    }
  }

  // the records of every row node, found by their row0 (a row LID belongs to one node)
  CHECK(int64_t(G.rec_row0.size()) == n_rec && int64_t(G.rec_meta.size()) == n_rec &&
            int64_t(G.rec_base.size()) == n_rec && int64_t(G.rec_ele.size()) == 8 * n_rec &&
            int64_t(G.rec_a.size()) == 8 * n_rec && int64_t(G.rec_tmap.size()) == 32 * n_rec, n_rec);
  std::map<int32_t, int32_t> node_of_row0;
  std::vector<int64_t> k_of_node(d->n_node, 0);  // incidences of a node, from the connectivity
  for (int64_t n = 0; n < d->n_node; ++n)
    if (m.dof_row[n] >= 0) node_of_row0[m.dof_row[n]] = int32_t(n);
  for (int64_t i = 0; i < 8 * n_ele; ++i) k_of_node[m.ele_nodes[i]]++;
  std::map<int32_t, std::vector<int64_t>> recs;  // node -> its records, ascending
  for (int64_t R = 0; R < n_rec; ++R)
  {
    CHECK(node_of_row0.count(G.rec_row0[R]) == 1, R);
    recs[node_of_row0[G.rec_row0[R]]].push_back(R);
  }
  int64_t owned_inc = 0, singles = 0;
  for (const auto& nr : node_of_row0)
  {
    const int32_t row0 = nr.first, nd = nr.second;
    const int64_t k = k_of_node[nd];
    const std::vector<int64_t>& rr = recs[nd];
    owned_inc += k;
    CHECK(int64_t(rr.size()) == std::max<int64_t>(1, (k + 7) / 8), nd);
    int64_t slots = 0;
    for (size_t i = 0; i < rr.size(); ++i)
    {
      const int64_t R = rr[i];
      CHECK(G.rec_base[R] == m.rowptr[row0], R);
      CHECK((G.rec_meta[R] >> 8) == m.rowptr[row0 + 1] - m.rowptr[row0], R);
      CHECK(((G.rec_meta[R] & 16) != 0) == (i == 0), R);
      CHECK(((G.rec_meta[R] & 32) != 0) == (i + 1 == rr.size()), R);
      CHECK((G.rec_meta[R] & 15) <= 8, R);
      slots += G.rec_meta[R] & 15;
      // one record: among the single ones; more: one multi_ptr range, in order
      if (rr.size() == 1)
        CHECK(R < G.n_single, R);
      else
        CHECK(R >= G.n_single && R == rr[0] + int64_t(i), R);
    }
    CHECK(slots == k, nd);
    if (rr.size() == 1) ++singles;
  }
  CHECK(singles == G.n_single, singles);
  CHECK(!G.multi_ptr.empty() && G.multi_ptr.front() == G.n_single && G.multi_ptr.back() == n_rec, 0);
  for (size_t j = 0; j + 1 < G.multi_ptr.size(); ++j)
  {
    CHECK(G.multi_ptr[j] < G.multi_ptr[j + 1], j);
    const std::vector<int64_t>& rr = recs[node_of_row0[G.rec_row0[G.multi_ptr[j]]]];
    CHECK(rr.front() == G.multi_ptr[j] && int64_t(rr.size()) == G.multi_ptr[j + 1] - G.multi_ptr[j], j);
  }

  // every owned incidence in exactly one slot of its node's records; the tmap nibbles
  std::vector<int> seen(8 * n_ele, 0);
  for (int64_t R = 0; R < n_rec; ++R)
  {
    const int32_t row0 = G.rec_row0[R], nd = node_of_row0[row0];
    const int ns = G.rec_meta[R] & 15;
    const int32_t* cols = m.col_lid.data() + m.rowptr[row0];
    const int64_t ntrip = (m.rowptr[row0 + 1] - m.rowptr[row0]) / 3;
    for (int s = 0; s < 8; ++s)
    {
      const int32_t slot = G.rec_ele[8 * R + s];
      if (s >= ns)
      {
        CHECK(slot == -1, 8 * R + s);
        for (int t = 0; t < 32; ++t) CHECK(((G.rec_tmap[32 * R + t] >> (4 * s)) & 15u) == 8u, 32 * R + t);
        continue;
      }
      CHECK(slot >= 0 && slot < n_ele, 8 * R + s);
      const int32_t e = G.eorig[slot], a = G.rec_a[8 * R + s];
      CHECK(a < 8 && m.ele_nodes[8 * e + a] == nd, 8 * R + s);
      CHECK(++seen[8 * e + a] == 1, 8 * e + a);
      for (int t = 0; t < 32; ++t)
      {
        uint32_t expect = 8;
        for (int b = 0; b < 8; ++b)
          if (t < ntrip && kcol[m.ele_nodes[8 * e + b]] == cols[3 * t]) expect = uint32_t(b);
        CHECK(((G.rec_tmap[32 * R + t] >> (4 * s)) & 15u) == expect, 32 * R + t);
      }
    }
  }
  for (int64_t i = 0; i < 8 * n_ele; ++i)
    CHECK(seen[i] == (m.dof_row[m.ele_nodes[i]] >= 0 ? 1 : 0), i);
  CHECK(owned_inc == S.inc.n_inc, owned_inc);
  CHECK(G.gauss.size() == 32, 0);
}

void check_ring(const char* name, Mesh& m)
{
  g_mesh = name;
  m.d.path = FCG_PATH_GENERAL;
  const fcg_desc* d = &m.d;
  Stages S;
  run_stages(d, S);
  CHECK(S.choice.path() == FCG_PATH_GENERAL, 0);
  const std::vector<int64_t> order = plan::rownode_morton_order(d, S.rows);
  const int64_t n_ele = d->n_ele, nrn = S.rows.nrn();
  std::vector<int32_t> rn_of(d->n_node, -1);  // from the descriptor: rows ascending by row LID
  {
    std::map<int32_t, int32_t> by_row;
    for (int64_t n = 0; n < d->n_node; ++n)
      if (m.dof_row[n] >= 0) by_row[m.dof_row[n]] = int32_t(n);
    int32_t r = 0;
    for (const auto& kv : by_row) rn_of[kv.second] = r++;
    CHECK(r == nrn, r);
  }
  const int64_t sizes[3] = {1, 3, n_ele - 1};
  for (int64_t S_el : sizes)
  {
    plan::H27Ring R;
    plan::build_h27_ring(n_ele, S_el, 0, S.inc.inc_ptr, S.inc.inc_ele, S.inc.inc_a, order, R);
    const int64_t nslab = (n_ele + S_el - 1) / S_el;
    CHECK(R.nslab == nslab && int64_t(R.asm_ptr.size()) == nslab + 1, S_el);
    CHECK(int64_t(R.slot.size()) == 27 * n_ele && int64_t(R.rows.size()) == nrn &&
              int64_t(R.rslot0.size()) == nrn, S_el);
    // the row nodes' incidences in element order, and the slab of the last one
    std::vector<std::vector<int64_t>> incs(nrn);
    for (int64_t i = 0; i < 27 * n_ele; ++i)
    {
      const int32_t r = rn_of[m.ele_nodes[i]];
      CHECK((R.slot[i] == -1) == (r < 0), i);
      if (r >= 0)
      {
        CHECK(R.slot[i] >= 0 && R.slot[i] < R.ring, i);
        incs[r].push_back(i);
      }
    }
    CHECK(R.asm_ptr.front() == 0 && R.asm_ptr.back() == nrn, S_el);
    std::vector<int> listed(nrn, 0);
    std::vector<int64_t> done_slab(nrn, 0);
    for (int64_t c = 0; c < nslab; ++c)
    {
      CHECK(R.asm_ptr[c] <= R.asm_ptr[c + 1], c);
      for (int64_t j = R.asm_ptr[c]; j < R.asm_ptr[c + 1]; ++j)
      {
        const int32_t r = R.rows[j];
        CHECK(r >= 0 && r < nrn, j);
        CHECK(++listed[r] == 1, j);
        done_slab[r] = c;
        if (!incs[r].empty()) CHECK(c == (incs[r].back() / 27) / S_el, j);
      }
    }
    for (int64_t r = 0; r < nrn; ++r) CHECK(listed[r] == 1, r);
    // live records (from the element's slab to the row's) hold distinct slots
    int64_t max_live = 0;
    for (int64_t t = 0; t < nslab; ++t)
    {
      std::vector<int64_t> holder(R.ring, -1);
      int64_t live = 0;
      for (int64_t r = 0; r < nrn; ++r)
        for (int64_t i : incs[r])
          if ((i / 27) / S_el <= t && t <= done_slab[r])
          {
            CHECK(holder[R.slot[i]] == -1, i);
            holder[R.slot[i]] = i;
            ++live;
          }
      max_live = std::max(max_live, live);
    }
    CHECK(R.ring >= max_live, S_el);
    for (int64_t r = 0; r < nrn; ++r)
      for (size_t q = 0; q < incs[r].size(); ++q)
        CHECK(R.slot[incs[r][q]] == (R.rslot0[r] + int64_t(q)) % R.ring, incs[r][q]);
  }
}

void check_slab_size()
{
  g_mesh = "slab size";
  const int64_t rec = 256 * 8, GB = int64_t(1) << 30;
  const int64_t n_inc = 1000000, nnz = 5000000;  // 1.9 GB of records + 40 MB of K + 4 GB headroom = 5.9 GB
  plan::H27Schedule s = plan::h27_schedule(100, n_inc, nnz, rec, GB, 8 * GB, 256, "5", nullptr);
  CHECK(s.slab == 5 && s.el_grid == 512, 0);
  s = plan::h27_schedule(100, n_inc, nnz, rec, GB, 8 * GB, 256, "0", "7");
  CHECK(s.slab == 0 && s.el_grid == 7, 1);
  s = plan::h27_schedule(100, n_inc, nnz, rec, 7 * GB, 8 * GB, 304, nullptr, nullptr);
  CHECK(s.slab == 0 && s.el_grid == 608, 2);
  s = plan::h27_schedule(100, n_inc, nnz, rec, 5 * GB, 8 * GB, 256, nullptr, nullptr);
  CHECK(s.slab == 4096, 3);
  s = plan::h27_schedule(2000000, n_inc, nnz, rec, 5 * GB, 8 * GB, 256, nullptr, nullptr);
  CHECK(s.slab == 10000, 4);
  // free memory unknown: the total stands in
  s = plan::h27_schedule(100, n_inc, nnz, rec, -1, 5 * GB, 256, nullptr, nullptr);
  CHECK(s.slab == 4096, 5);
  s = plan::h27_schedule(100, n_inc, nnz, rec, -1, 8 * GB, 256, nullptr, nullptr);
  CHECK(s.slab == 0, 6);
}

}  // namespace

int main()
{
  Mesh b322 = box(FCG_HEX8, 3, 2, 2, 0, 1, 0.1);
  Mesh perm = permuted(b322, 7);
  check_gather("hex8 3x2x2 permuted", perm);

  for (int rank = 0; rank < 2; ++rank)
  {
    Mesh part = box(FCG_HEX8, 4, 2, 2, rank, 2, 0.0);
    CHECK(part.d.n_rows < part.d.n_cols, rank);  // owned rows fewer than the column nodes' DOFs
    part.d.ele_ijk = nullptr;
    check_gather(rank == 0 ? "hex8 4x2x2 rank 0 of 2" : "hex8 4x2x2 rank 1 of 2", part);
  }

  // the element list twice: 16 incidences at interior nodes, the same couplings
  Mesh twice = perm;
  twice.ele_nodes.insert(twice.ele_nodes.end(), perm.ele_nodes.begin(), perm.ele_nodes.end());
  twice.point();
  check_gather("hex8 3x2x2 elements doubled", twice);

  // one more owned node that no element references: three rows holding its own triple
  Mesh lone = perm;
  const int32_t c = int32_t(lone.d.n_cols), r = int32_t(lone.d.n_rows);
  lone.x.insert(lone.x.end(), {2.0, 2.0, 2.0});
  lone.dof_col.push_back(c);
  lone.dof_row.push_back(r);
  for (int k = 0; k < 3; ++k)
  {
    lone.col_lid.insert(lone.col_lid.end(), {c, c + 1, c + 2});
    lone.rowptr.push_back(lone.rowptr.back() + 3);
  }
  lone.d.n_cols += 3;
  lone.point();
  check_gather("hex8 3x2x2 plus a node without elements", lone);

  Mesh h27 = box(FCG_HEX27, 2, 2, 2, 0, 1, 0.0);
  check_ring("hex27 2x2x2", h27);
  Mesh h27r = box(FCG_HEX27, 2, 2, 2, 0, 2, 0.0);
  check_ring("hex27 2x2x2 rank 0 of 2", h27r);

  check_slab_size();
  std::printf("PASS\n");
  return 0;
}
