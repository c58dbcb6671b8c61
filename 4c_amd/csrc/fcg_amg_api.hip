// fcg_amg_api.hip -- the C ABI of the structural AMG (fourc_gpu.h: fcg_amg_create / _setup /
// _iterate / _solve / _apply, the level queries, fcg_amg_precond_setup / _apply for the coarse
// levels coupled across ranks, fcg_amg_destroy): argument checks, the handle's construction, and
// the translation of fcg_amgs::Fail into return codes and last_error.  The work is in
// fcg_amg_solver.hip and fcg_amg_coupled.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fcg_amg_internal.hpp"

extern "C" {

void fcg_amg_default_options(fcg_amg_options* opt)
{
  if (!opt) return;
  opt->nu = 2;
  opt->max_levels = 10;
  opt->coarse_max = 3000;
  opt->coarse_max_iter = 500;
  opt->coarse_rtol = 1e-2;
  opt->omega = 4.0 / 3.0;
  opt->ratio = 20.0;
  opt->boost = 1.1;
}

int fcg_amg_create(fcg_ctx* ctx, const int64_t* rowptr, const int32_t* col_lid,
    const double* node_x, int64_t n_dbc, const int32_t* dbc_rows, const fcg_amg_options* opt,
    fcg_amg** out)
{
  using namespace fcg_amgs;
  if (!ctx || !rowptr || !col_lid || !node_x || !out || n_dbc < 0 || (n_dbc > 0 && !dbc_rows))
    return FCG_ERR_ARG;
  *out = nullptr;
  const fcg::DeviceMesh& m = ctx->mesh;
  if (!m.owned_cols_first || m.n_rows % 3 != 0 || m.n_rows == 0)
  {
    ctx->last_error = "fcg_amg_create: 3 DOFs per owned node (rows 3b..3b+2), owned columns first";
    return FCG_ERR_ARG;
  }
  if (!m.triple_rows)
  {
    // the block copies of K (node_csr_to_bsr_kernel, perm_csr_to_bsr_kernel) read a row by triples
    ctx->last_error = "fcg_amg_create: a row of the context holds columns that are not node DOF triples";
    return FCG_ERR_ARG;
  }
  fcg_amg* h = new fcg_amg();
  h->ctx = ctx;
  h->device = ctx->device;
  h->local = !m.square_local;
  if (opt) h->opt = *opt;
  else fcg_amg_default_options(&h->opt);
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    const int64_t n = m.n_rows, nb = n / 3;
    h->n0 = n;
    h->nb0 = nb;
    // level 0 block graph: block row b = rows 3b..3b+2 (one pattern of DOF triples)
    // (local: the owned block only -- owned column LIDs are < n and, the columns being sorted,
    // come before every ghost column)
    std::vector<int64_t> bptr(size_t(nb) + 1, 0);
    for (int64_t b = 0; b < nb; ++b)
    {
      const int64_t len = rowptr[3 * b + 1] - rowptr[3 * b];
      if (len % 3 != 0 || rowptr[3 * b + 2] - rowptr[3 * b + 1] != len || rowptr[3 * b + 3] - rowptr[3 * b + 2] != len)
        throw Fail{FCG_ERR_ARG, "fcg_amg_create: rows 3b..3b+2 must share one pattern of DOF triples"};
      int64_t own = 0;
      while (own < len / 3 && col_lid[rowptr[3 * b] + 3 * own] < n) ++own;
      for (int64_t k = own; k < len / 3; ++k)
        if (col_lid[rowptr[3 * b] + 3 * k] < n)
          throw Fail{FCG_ERR_ARG, "fcg_amg_create: row columns must be sorted (owned before ghosts)"};
      bptr[size_t(b) + 1] = bptr[size_t(b)] + own;
    }
    std::vector<int32_t> bcol(size_t(bptr.back()));
    for (int64_t b = 0; b < nb; ++b)
      for (int64_t k = 0; k < bptr[size_t(b) + 1] - bptr[size_t(b)]; ++k)
      {
        const int32_t c = col_lid[rowptr[3 * b] + 3 * k];
        if (c < 0 || c % 3 != 0 || c >= n) throw Fail{FCG_ERR_ARG, "fcg_amg_create: column triples must start at 3 c"};
        bcol[size_t(bptr[size_t(b)] + k)] = c / 3;
      }
    // single rank: level 0 in the Morton order of the node coordinates (21 bits per axis)
    std::vector<int32_t> new2old;
    if (!h->local && !env_off("FCG_AMG_REORDER") && nb > 1)
    {
      double lo[3] = {node_x[0], node_x[1], node_x[2]}, hi[3] = {node_x[0], node_x[1], node_x[2]};
      for (int64_t b = 0; b < nb; ++b)
        for (int d = 0; d < 3; ++d)
        {
          lo[d] = std::min(lo[d], node_x[3 * b + d]);
          hi[d] = std::max(hi[d], node_x[3 * b + d]);
        }
      std::vector<uint64_t> key(static_cast<size_t>(nb));
      for (int64_t b = 0; b < nb; ++b)
      {
        uint64_t m = 0;
        uint32_t q[3];
        for (int d = 0; d < 3; ++d)
        {
          const double ext = hi[d] - lo[d];
          const double f = ext > 0.0 ? (node_x[3 * b + d] - lo[d]) / ext : 0.0;
          q[d] = uint32_t(std::min(2097151.0, std::max(0.0, f * 2097151.0)));
        }
        for (int bit = 20; bit >= 0; --bit)
          for (int d = 0; d < 3; ++d) m = (m << 1) | ((q[d] >> bit) & 1u);
        key[size_t(b)] = m;
      }
      new2old.resize(size_t(nb));
      for (int64_t b = 0; b < nb; ++b) new2old[size_t(b)] = int32_t(b);
      std::stable_sort(new2old.begin(), new2old.end(),
          [&](int32_t a, int32_t c) { return key[size_t(a)] < key[size_t(c)]; });
      std::vector<int32_t> old2new(static_cast<size_t>(nb));
      for (int64_t p = 0; p < nb; ++p) old2new[size_t(new2old[size_t(p)])] = int32_t(p);
      std::vector<int64_t> pptr(size_t(nb) + 1, 0);
      std::vector<int32_t> pcol(bcol.size()), pk(bcol.size());
      std::vector<std::pair<int32_t, int32_t>> row;
      for (int64_t p = 0; p < nb; ++p)
      {
        const int64_t r = new2old[size_t(p)];
        row.clear();
        for (int64_t k = bptr[size_t(r)]; k < bptr[size_t(r) + 1]; ++k)
          row.emplace_back(old2new[size_t(bcol[size_t(k)])], int32_t(k - bptr[size_t(r)]));
        std::sort(row.begin(), row.end());
        pptr[size_t(p) + 1] = pptr[size_t(p)] + int64_t(row.size());
        for (size_t m = 0; m < row.size(); ++m)
        {
          pcol[size_t(pptr[size_t(p)]) + m] = row[m].first;
          pk[size_t(pptr[size_t(p)]) + m] = row[m].second;
        }
      }
      bptr.swap(pptr);
      bcol.swap(pcol);
      h->new2old = upload(h, new2old);
      h->old_k = upload(h, pk);
      h->pb = dalloc<double>(h, n);
      h->px = dalloc<double>(h, n);
    }
    make_bsr(h, h->A0, bptr, bcol, 3, 3, nb);
    if (h->local)
    {
      // the rank's whole rows (ghost column triples included), for the coarse level coupled
      // across ranks (A_1 = P_0^T A P_0 with the global operator): block column = column LID / 3
      if (m.n_cols % 3 != 0) throw Fail{FCG_ERR_ARG, "fcg_amg_create: 3 DOFs per column node"};
      h->full_ptr.assign(size_t(nb) + 1, 0);
      for (int64_t b = 0; b < nb; ++b) h->full_ptr[size_t(b) + 1] = h->full_ptr[size_t(b)] + (rowptr[3 * b + 1] - rowptr[3 * b]) / 3;
      h->full_col.resize(size_t(h->full_ptr.back()));
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t k = 0; k < h->full_ptr[size_t(b) + 1] - h->full_ptr[size_t(b)]; ++k)
        {
          const int32_t c = col_lid[rowptr[3 * b] + 3 * k];
          if (c < 0 || c % 3 != 0 || c >= m.n_cols)
            throw Fail{FCG_ERR_ARG, "fcg_amg_create: column triples must start at 3 c"};
          h->full_col[size_t(h->full_ptr[size_t(b)] + k)] = c / 3;
        }
    }
    h->A0_diag = upload(h, diag_index(h->A0));
    h->A0_dinv = dalloc<double>(h, 9 * nb);
    h->ctx_dinv = dalloc<double>(h, 9 * nb);
    std::vector<uint8_t> dbc(size_t(n), 0);
    for (int64_t k = 0; k < n_dbc; ++k)
    {
      if (dbc_rows[k] < 0 || dbc_rows[k] >= n) throw Fail{FCG_ERR_ARG, "fcg_amg_create: Dirichlet row out of range"};
      dbc[size_t(dbc_rows[k])] = 1;
    }
    // level 0's order (identity without reordering)
    std::vector<double> xl;
    const double* X0 = node_x;
    if (!new2old.empty())
    {
      std::vector<uint8_t> dp(static_cast<size_t>(n));
      xl.resize(size_t(3 * nb));
      for (int64_t p = 0; p < nb; ++p)
        for (int d = 0; d < 3; ++d)
        {
          dp[size_t(3 * p + d)] = dbc[size_t(3 * int64_t(new2old[size_t(p)]) + d)];
          xl[size_t(3 * p + d)] = node_x[3 * int64_t(new2old[size_t(p)]) + d];
        }
      dbc.swap(dp);
      X0 = xl.data();
    }
    std::vector<double> mask(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) mask[size_t(i)] = dbc[size_t(i)] ? 0.0 : 1.0;
    h->mask0 = upload(h, mask);
    // near-null space: rigid-body modes about the centroid, Dirichlet rows zeroed
    double cen[3] = {0, 0, 0};
    for (int64_t b = 0; b < nb; ++b)
      for (int d = 0; d < 3; ++d) cen[d] += X0[3 * b + d] / double(nb);
    std::vector<double> ns(size_t(nb) * 18, 0.0);
    std::vector<uint8_t> skip(size_t(nb), 0);
    for (int64_t b = 0; b < nb; ++b)
    {
      const double x = X0[3 * b] - cen[0], y = X0[3 * b + 1] - cen[1], z = X0[3 * b + 2] - cen[2];
      double* B = ns.data() + 18 * b;  // [3][6]
      B[0 * 6 + 0] = B[1 * 6 + 1] = B[2 * 6 + 2] = 1.0;
      B[0 * 6 + 3] = -y; B[1 * 6 + 3] = x;
      B[1 * 6 + 4] = -z; B[2 * 6 + 4] = y;
      B[0 * 6 + 5] = z;  B[2 * 6 + 5] = -x;
      int nd = 0;
      for (int d = 0; d < 3; ++d)
        if (dbc[size_t(3 * b + d)])
        {
          ++nd;
          for (int j = 0; j < 6; ++j) B[d * 6 + j] = 0.0;
        }
      skip[size_t(b)] = nd == 3;
    }
    coarsen(h, &h->A0, 3, std::move(ns), skip.data());
    if (h->levels.empty()) throw Fail{FCG_ERR_ARG, "fcg_amg_create: no coarse level (aggregation did not coarsen)"};
    for (double** v : {&h->r0, &h->d0, &h->z0, &h->q0, &h->p0, &h->ro0, &h->fr, &h->fz, &h->fx})
      *v = dalloc<double>(h, n);
    h->partial = dalloc<double>(h, kMaxPartials);
    h->sc = dalloc<double>(h, 16);  // [0, 6) outer FCG, 6 host dots, [8, 13) coarsest CG
    h->flag = dalloc<int32_t>(h, 1);
  }
  catch (const Fail& f)
  {
    ctx->last_error = f.msg;
    fcg_amg_destroy(h);
    return f.code;
  }
  *out = h;
  return FCG_OK;
}

int fcg_amg_setup(fcg_amg* h, const double* d_K_vals, void* stream)
{
  using namespace fcg_amgs;
  if (!h || !d_K_vals) return FCG_ERR_ARG;
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->ctx->stream;
    hipEvent_t e0, e1;
    ck(hipEventCreate(&e0), "hipEventCreate");
    ck(hipEventCreate(&e1), "hipEventCreate");
    ck(hipEventRecord(e0, s), "hipEventRecord");
    if (h->gexec)  // its kernel arguments hold the previous setup's lambda_max values
    {
      (void)hipGraphExecDestroy(h->gexec);
      h->gexec = nullptr;
    }
    setup(h, d_K_vals, s);
    ck(hipEventRecord(e1, s), "hipEventRecord");
    ck(hipEventSynchronize(e1), "hipEventSynchronize");
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    h->setup_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->ready = true;
    h->local_ready = true;
  }
  catch (const Fail& f)
  {
    h->ready = false;
    h->local_ready = false;
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    return f.code;
  }
  return FCG_OK;
}

int fcg_amg_iterate(fcg_amg* h, const double* d_K_vals, const double* d_b_row, double* d_x_row,
    double rtol, int max_iter, int* iterations, double* rel_residual, void* stream)
{
  using namespace fcg_amgs;
  if (!h || !d_K_vals || !d_b_row || !d_x_row || !(rtol >= 0.0) || max_iter < 0) return FCG_ERR_ARG;
  if (h->local)
  {
    // a rank of a partition: level 0 is only the owned block, so iterating here would solve the
    // block-diagonal local system and report it converged -- the solve across ranks is
    // fcg_dfcg_solve (this handle then serves as its preconditioner through setup / apply)
    h->last_error = "fcg_amg_iterate: multi-rank context (ghost columns) -- solve with fcg_dfcg_solve";
    h->ctx->last_error = h->last_error;
    return FCG_ERR_ARG;
  }
  if (!h->ready || !h->local_ready)
  {
    h->last_error = "fcg_amg_iterate: no numeric setup of the handle's own hierarchy for this K (call fcg_amg_setup first)";
    return FCG_ERR_ARG;
  }
  int it = 0;
  double rel = 0.0;
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->ctx->stream;
    run_fcg(h, d_K_vals, d_b_row, d_x_row, rtol, max_iter, &it, &rel, s);
  }
  catch (const Fail& f)
  {
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    if (iterations) *iterations = it;
    if (rel_residual) *rel_residual = rel;
    return f.code;
  }
  if (iterations) *iterations = it;
  if (rel_residual) *rel_residual = rel;
  return FCG_OK;
}

int fcg_amg_solve(fcg_amg* h, const double* d_K_vals, const double* d_b_row, double* d_x_row,
    double rtol, int max_iter, int* iterations, double* rel_residual, void* stream)
{
  if (iterations) *iterations = 0;
  if (rel_residual) *rel_residual = 0.0;
  if (!h || !d_K_vals || !d_b_row || !d_x_row || !(rtol >= 0.0) || max_iter < 0) return FCG_ERR_ARG;
  if (h->local)
  {
    h->last_error = "fcg_amg_solve: multi-rank context (ghost columns) -- solve with fcg_dfcg_solve";
    h->ctx->last_error = h->last_error;
    return FCG_ERR_ARG;
  }
  const int rc = fcg_amg_setup(h, d_K_vals, stream);
  if (rc != FCG_OK) return rc;
  return fcg_amg_iterate(h, d_K_vals, d_b_row, d_x_row, rtol, max_iter, iterations, rel_residual, stream);
}

int fcg_amg_level_info(const fcg_amg* h, int level, int64_t* dofs, int64_t* blocks, double* lmax)
{
  if (!h || level < 0 || level > int(h->levels.size())) return FCG_ERR_ARG;
  if (level == 0)
  {
    if (dofs) *dofs = h->n0;
    if (blocks) *blocks = h->A0.nnzb;
    if (lmax) *lmax = h->lmax0;
    return FCG_OK;
  }
  const fcg_amgs::Level& c = h->levels[size_t(level - 1)];
  if (dofs) *dofs = c.A.n * 6;
  if (blocks) *blocks = c.A.nnzb;
  if (lmax) *lmax = c.lmax;
  return FCG_OK;
}

int fcg_amg_levels(const fcg_amg* h) { return h ? int(h->levels.size()) + 1 : 0; }

double fcg_amg_setup_ms(const fcg_amg* h) { return h ? h->setup_ms : -1.0; }

int fcg_amg_stats(const fcg_amg* h, int* coarse_dense, int* graph_launches)
{
  if (!h) return FCG_ERR_ARG;
  if (coarse_dense) *coarse_dense = h->cinv ? 1 : 0;
  if (graph_launches) *graph_launches = h->graph_launches;
  return FCG_OK;
}

const char* fcg_amg_last_error(const fcg_amg* h) { return h ? h->last_error.c_str() : ""; }

// Host copies of what the last fcg_amg_setup left on the device (tests rebuild the hierarchy and
// the V-cycle from them): synchronises and copies, starts no kernel, changes nothing in the handle
int64_t fcg_amg_level_matrix(const fcg_amg* h, int level, int which, int64_t* ptr, int32_t* col,
    double* vals, int64_t capacity)
{
  using namespace fcg_amgs;
  if (!h || level < 0 || which < 0 || which > 4) return -1;
  const int nl = int(h->levels.size()) + 1;
  if (level >= nl) return -1;
  const Bsr& A = level == 0 ? h->A0 : h->levels[size_t(level - 1)].A;
  const Bsr* M = nullptr;
  const double* dv = nullptr;
  int64_t count = 0;
  if (which <= 2)
  {
    if (which != 0 && level + 1 >= nl) return -1;
    M = which == 0 ? &A : which == 1 ? &h->steps[size_t(level)].P : &h->steps[size_t(level)].T;
    dv = M->vals;
    count = M->nnzb * M->br * M->bc;
  }
  else if (which == 3)
  {
    // the smoother's inverses: level 0 in the context's order smooths with the context's own
    dv = level == 0 ? (h->new2old ? h->A0_dinv : h->ctx_dinv) : h->levels[size_t(level - 1)].dinv;
    count = A.n * A.br * A.br;
  }
  else
  {
    const int64_t n = A.n * A.br;
    if (level + 1 != nl || !h->cinv || h->cn != n) return -1;
    dv = h->cinv;
    count = n * n;
  }
  if (!ptr && !col && !vals) return count;
  if (!vals || (M && (!ptr || !col)) || capacity < count || !h->ready || !h->local_ready) return -1;
  if (!fcg_use_device(h->device)) return -1;
  hipError_t he = hipDeviceSynchronize();
  if (M)
  {
    if (he == hipSuccess) he = hipMemcpy(ptr, M->ptr, sizeof(int64_t) * size_t(M->n + 1), hipMemcpyDeviceToHost);
    if (he == hipSuccess && M->nnzb) he = hipMemcpy(col, M->col, sizeof(int32_t) * size_t(M->nnzb), hipMemcpyDeviceToHost);
  }
  if (he == hipSuccess && count) he = hipMemcpy(vals, dv, sizeof(double) * size_t(count), hipMemcpyDeviceToHost);
  if (he != hipSuccess)
  {
    (void)hipGetLastError();
    return -1;
  }
  return count;
}

int fcg_amg_level_order(const fcg_amg* h, int32_t* new2old)
{
  if (!h || !new2old) return FCG_ERR_ARG;
  if (!h->new2old)
  {
    for (int64_t p = 0; p < h->nb0; ++p) new2old[p] = int32_t(p);
    return FCG_OK;
  }
  if (!fcg_use_device(h->device)) return fcg_device_error();
  if (hipMemcpy(new2old, h->new2old, sizeof(int32_t) * size_t(h->nb0), hipMemcpyDeviceToHost) != hipSuccess)
  {
    (void)hipGetLastError();
    return FCG_ERR_DEVICE;
  }
  return FCG_OK;
}

int fcg_amg_apply(fcg_amg* h, const double* d_K_vals, const double* d_r_row, double* d_z_row,
    void* stream)
{
  using namespace fcg_amgs;
  if (!h || !d_K_vals || !d_r_row || !d_z_row) return FCG_ERR_ARG;
  if (!h->ready || !h->local_ready)
  {
    // after fcg_dfcg_solve's coupled setup only the coupled application is valid on this handle
    h->last_error = "fcg_amg_apply: no numeric setup of the handle's own hierarchy for this K (call fcg_amg_setup first)";
    return FCG_ERR_ARG;
  }
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->ctx->stream;
    if (h->new2old)
    {
      node_perm(h, d_r_row, h->pb, 0, s);
      vcycle(h, 0, d_K_vals, h->pb, h->px, s);
      node_perm(h, h->px, d_z_row, 1, s);
      ck(hipGetLastError(), "node_perm_kernel");
    }
    else
      vcycle(h, 0, d_K_vals, d_r_row, d_z_row, s);
  }
  catch (const Fail& f)
  {
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    return f.code;
  }
  return FCG_OK;
}

// fcg_dfcg_solve's preconditioner (internal, fcg_internal.hpp): the numeric setup and one
// application -- coupled across ranks when the handle is rank-local and the transport names more
// than one rank (the coupled levels are built on the first call), else the handle's own V-cycle
int fcg_amg_precond_setup(fcg_amg* h, const double* d_K, const fcg_transport* tr, void* stream)
{
  using namespace fcg_amgs;
  // test hook: FCG_AMG_INJECT_FAIL_RANK=r makes rank r's local setup fail (tests/test_multigpu.py)
  static const int inject = [] {
    const char* e = std::getenv("FCG_AMG_INJECT_FAIL_RANK");
    return e ? std::atoi(e) : -1;
  }();
  int rc = FCG_OK;
  if (tr && tr->nranks > 1 && h->local)
  {
    try
    {
      ck(hipSetDevice(h->device), "hipSetDevice");
      h->local_ready = false;  // only the block inverses follow this K
      setup_coupled_local(h, d_K, stream ? static_cast<hipStream_t>(stream) : h->ctx->stream);
      h->ready = true;
    }
    catch (const Fail& f)
    {
      h->ready = false;
      h->last_error = f.msg;
      h->ctx->last_error = f.msg;
      rc = f.code;
    }
  }
  else
    rc = fcg_amg_setup(h, d_K, stream);
  if (rc == FCG_OK && tr && tr->nranks > 1 && tr->rank == inject)
  {
    h->ready = false;
    h->last_error = "coupled AMG: injected setup failure (FCG_AMG_INJECT_FAIL_RANK)";
    rc = FCG_ERR_SINGULAR;
  }
  if (!tr || tr->nranks <= 1) return rc;
  // Every rank of the transport enters the coupled levels' chain of collectives (imports, the
  // A_1 all-reduce) or none does: a go/no-go all-reduce of {local setup failed, handle not
  // rank-local} first, a status all-reduce after the build and numeric setup.  A rank that fails
  // alone would otherwise leave the others waiting in their next collective.
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->ctx->stream;
  auto agree = [&](double bad, double nonlocal, double* out) -> int {
    try
    {
      if (!h->agree) h->agree = dalloc<double>(h, 2);
      const double v[2] = {bad, nonlocal};
      ck(hipMemcpyAsync(h->agree, v, sizeof(v), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
      ck(tr->allreduce_fn(tr->user, h->agree, 2, s), "transport all-reduce (go/no-go)");
      ck(hipMemcpyAsync(out, h->agree, 2 * sizeof(double), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
      ck(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    catch (const Fail& f)
    {
      h->last_error = f.msg;
      h->ctx->last_error = f.msg;
      return f.code;
    }
    return FCG_OK;
  };
  double g[2] = {0.0, 0.0};
  const int ra = agree(rc != FCG_OK ? 1.0 : 0.0, h->local ? 0.0 : 1.0, g);
  if (ra != FCG_OK) return ra;
  auto others_failed = [&](int code) {
    h->ready = false;
    h->last_error = "coupled AMG: the setup failed on another rank of the transport";
    h->ctx->last_error = h->last_error;
    return code;
  };
  if (g[0] > 0.0) return rc != FCG_OK ? rc : others_failed(FCG_ERR_DEVICE);
  if (g[1] > 0.0 && g[1] < double(tr->nranks))
  {
    h->last_error = "coupled AMG: the ranks disagree on whether their handles are rank-local";
    h->ctx->last_error = h->last_error;
    h->ready = false;
    return FCG_ERR_ARG;
  }
  if (!h->local) return FCG_OK;  // no rank's handle is rank-local: each keeps its own V-cycle
  int code = FCG_OK;
  // the build and the numeric setup over the guarded transport: a rank failing inside them meets
  // the others at their next collective (or at the final status below) and all stop together
  Guard G;
  G.in = tr;
  G.h = h;
  G.s = s;
  const fcg_transport gt = guarded(tr, &G);
  // test hook: FCG_AMG_INJECT_BUILD_FAIL="r:k" makes rank r throw inside coupled_build when it
  // reaches its k-th guarded collective (tests/test_multigpu.py, tests/cxx/config3_native.cpp)
  static const std::pair<int, int64_t> inject_build = [] {
    const char* e = std::getenv("FCG_AMG_INJECT_BUILD_FAIL");
    const char* c = e ? std::strchr(e, ':') : nullptr;
    return e ? std::make_pair(std::atoi(e), c ? int64_t(std::atoll(c + 1)) : int64_t(0))
             : std::make_pair(-1, int64_t(0));
  }();
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    if (tr->rank < 0 || tr->rank >= tr->nranks) throw Fail{FCG_ERR_ARG, "coupled AMG: transport rank out of range"};
    if (!h->cpl)
    {
      try
      {
        if (tr->rank == inject_build.first) G.fail_at = inject_build.second;
        coupled_build(h, &gt, s);
        G.fail_at = -1;
      }
      catch (const Fail&)
      {
        // a failed build leaves no half-built coupling behind (its device buffers stay listed
        // in the handle's allocations until fcg_amg_destroy)
        if (h->cpl) fcg_amg_destroy(h->cpl->g);
        delete h->cpl;
        h->cpl = nullptr;
        throw;
      }
    }
    else if (h->cpl->rank != tr->rank || h->cpl->nranks != tr->nranks)
      throw Fail{FCG_ERR_ARG, "coupled AMG: the transport's rank / rank count changed"};
    coupled_setup(h, d_K, &gt, s);
  }
  catch (const Fail& f)
  {
    h->ready = false;
    if (G.remote)
      return others_failed(FCG_ERR_DEVICE);  // met another rank's failure at a collective: done
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    code = f.code;
  }
  // the final status: the ranks that finished and the ranks that failed on their own meet here (a
  // rank that failed is at the same count of checkpoints as the others' next one)
  bool any = false;
  try
  {
    any = guard_checkpoint(&G, code != FCG_OK ? 1.0 : 0.0);
  }
  catch (const Fail& f)
  {
    h->ready = false;
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    return code != FCG_OK ? code : f.code;
  }
  if (code != FCG_OK) return code;
  if (any) return others_failed(FCG_ERR_DEVICE);
  return FCG_OK;
}

int fcg_amg_precond_apply(fcg_amg* h, const double* d_K, const fcg_transport* tr, const double* d_r,
    double* d_z, void* stream)
{
  using namespace fcg_amgs;
  if (!h->cpl || !tr || tr->nranks <= 1) return fcg_amg_apply(h, d_K, d_r, d_z, stream);
  try
  {
    ck(hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->ctx->stream;
    coupled_apply(h, d_K, tr, d_r, d_z, s);
  }
  catch (const Fail& f)
  {
    h->last_error = f.msg;
    h->ctx->last_error = f.msg;
    return f.code;
  }
  return FCG_OK;
}

int fcg_amg_coupled_levels(const fcg_amg* h)
{
  if (!h || !h->cpl || !h->cpl->g) return 0;
  int n = int(h->cpl->g->levels.size());
  for (const fcg_amgs::Dist* d = h->cpl->d; d; d = d->next) ++n;
  return n;
}

int fcg_amg_coupled_stats(const fcg_amg* h, int64_t* out, int n)
{
  if (!h || !out || n < 0) return FCG_ERR_ARG;
  const fcg_amgs::Coupled* c = h->cpl;
  int64_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (c && c->g)
  {
    for (const fcg_amgs::Dist* d = c->d; d; d = d->next) ++v[0];
    v[1] = c->d ? c->d->na : c->n_agg_tot;
    v[2] = c->n_agg_tot;
    v[3] = c->ar_setup;
    v[4] = c->ar_apply;
    v[5] = c->x_setup;
    v[6] = c->x_apply;
    v[7] = fcg_amgs::hierarchy_bytes(c->g);
    v[8] = c->rep_n;
  }
  const int k = std::min(n, 9);
  for (int i = 0; i < k; ++i) out[i] = v[i];
  return k;
}

int fcg_amg_destroy(fcg_amg* h)
{
  if (!h) return FCG_OK;
  if (h->cpl)
  {
    fcg_amg_destroy(h->cpl->g);
    delete h->cpl;
    h->cpl = nullptr;
  }
  (void)hipSetDevice(h->device);
  if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
  if (h->gs)
  {
    (void)hipStreamSynchronize(h->gs);
    (void)hipStreamDestroy(h->gs);
  }
  for (hipEvent_t e : h->gev)
    if (e) (void)hipEventDestroy(e);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return FCG_OK;
}

}  // extern "C"
