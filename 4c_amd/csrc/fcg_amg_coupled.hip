// fcg_amg_coupled.hip -- the structural AMG's coarse levels coupled across ranks (fcg_dfcg_solve
// with a rank-local handle; the scheme and its types Coupled and Dist are described in
// fcg_amg_internal.hpp): the exchange kernels and counted collectives, the build of the coupled and
// distributed levels on the first solve (coupled_build, build_dist), their numeric setup per tangent
// (coupled_setup, dist_setup), the V-cycle of the global system (coupled_apply) and the guarded
// transport the build and setup run over.  The smoother, the Lanczos estimate and the replicated
// hierarchy's cycle are the single-rank ones of fcg_amg_solver.hip, through Ops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fcg_amg_internal.hpp"

namespace fcg_amgs {

// element-wise sum over the ranks of a host vector, through the transport's device all-reduce
void host_allsum(const fcg_transport* tr, std::vector<double>& v, hipStream_t s)
{
  DevBuf d(int64_t(v.size()));
  if (!v.empty())
    ck(hipMemcpyAsync(d.p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
  ck(tr->allreduce_fn(tr->user, d.p, int64_t(v.size()), s), "transport all-reduce");
  if (!v.empty())
    ck(hipMemcpyAsync(v.data(), d.p, sizeof(double) * v.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
}

// the all-reduce of the coupled levels, counted
void allreduce_counted(Coupled* c, const fcg_transport* tr, double* p, int64_t n, hipStream_t s, const char* what)
{
  ck(tr->allreduce_fn(tr->user, p, n, s), what);
  c->ctr_ar += n;
}

// one exchange of w-double items on pattern x (reverse: the owner -> requester direction), counted
void exchange_counted(Coupled* c, const fcg_transport* tr, Xch& x, int w, bool reverse, const double* sb,
    double* rb, hipStream_t s, const char* what)
{
  const std::vector<int64_t>& sc = reverse ? x.rcnt : x.scnt;
  const std::vector<int64_t>& rc = reverse ? x.scnt : x.rcnt;
  x.sd.assign(sc.size(), 0);
  x.rd.assign(rc.size(), 0);
  for (size_t q = 0; q < sc.size(); ++q)
  {
    x.sd[q] = sc[q] * w;
    x.rd[q] = rc[q] * w;
    c->ctr_x += x.sd[q];
  }
  ck(tr->exchange_fn(tr->user, sb, x.sd.data(), rb, x.rd.data(), s), what);
}

// build-time exchange of host vectors: out[q] goes to rank q (out[me] empty), returns what every
// rank sent to this one (counts first, then the payload, both through exchange_fn)
std::vector<std::vector<double>> host_exchange(const fcg_transport* tr, const std::vector<std::vector<double>>& out,
    hipStream_t s)
{
  const int R = tr->nranks, me = tr->rank;
  std::vector<int64_t> one(static_cast<size_t>(R), 1);
  one[static_cast<size_t>(me)] = 0;
  std::vector<double> cnt_s, cnt_r(static_cast<size_t>(R - 1), 0.0);
  for (int q = 0; q < R; ++q)
    if (q != me) cnt_s.push_back(double(out[static_cast<size_t>(q)].size()));
  DevBuf ds(R), dr(R);
  ck(hipMemcpyAsync(ds.p, cnt_s.data(), sizeof(double) * cnt_s.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
  ck(tr->exchange_fn(tr->user, ds.p, one.data(), dr.p, one.data(), s), "transport exchange (counts)");
  ck(hipMemcpyAsync(cnt_r.data(), dr.p, sizeof(double) * cnt_r.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  std::vector<int64_t> sc(static_cast<size_t>(R), 0), rc(static_cast<size_t>(R), 0);
  std::vector<double> flat;
  for (int q = 0, k = 0; q < R; ++q)
  {
    if (q == me) continue;
    sc[static_cast<size_t>(q)] = int64_t(out[static_cast<size_t>(q)].size());
    rc[static_cast<size_t>(q)] = int64_t(cnt_r[static_cast<size_t>(k++)]);
    flat.insert(flat.end(), out[static_cast<size_t>(q)].begin(), out[static_cast<size_t>(q)].end());
  }
  int64_t nr = 0;
  for (int64_t v : rc) nr += v;
  DevBuf ps(int64_t(flat.size())), pr(nr);
  if (!flat.empty())
    ck(hipMemcpyAsync(ps.p, flat.data(), sizeof(double) * flat.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
  ck(tr->exchange_fn(tr->user, ps.p, sc.data(), pr.p, rc.data(), s), "transport exchange (build)");
  std::vector<double> got(static_cast<size_t>(nr));
  if (nr) ck(hipMemcpyAsync(got.data(), pr.p, sizeof(double) * static_cast<size_t>(nr), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  std::vector<std::vector<double>> in(static_cast<size_t>(R));
  for (int q = 0, o = 0; q < R; ++q)
  {
    in[static_cast<size_t>(q)].assign(got.begin() + o, got.begin() + o + rc[static_cast<size_t>(q)]);
    o += int(rc[static_cast<size_t>(q)]);
  }
  return in;
}

// channel (k, col) of a 3 x 6 BSR's rows as a DOF vector: DOF d of owned node i gets entry
// (d, col) of the row's k-th block (col < 0: the block's global column id -- l2g[col] or col +
// off --, -1 past the row's end)
__global__ __launch_bounds__(kBlock) void pack_channel_kernel(int64_t nb, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, int k, int c, int64_t off,
    double* out)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= 3 * nb) return;
  const int64_t i = t / 3, d = t - 3 * i;
  const int64_t p = ptr[i] + k;
  const bool in = p < ptr[i + 1];
  out[t] = c < 0 ? (in ? double(int64_t(col[p]) + off) : -1.0) : (in ? vals[p * 18 + d * 6 + c] : 0.0);
}

// ... and back into the ghost rows (column nodes nb .. nc-1) of an extended BSR
__global__ __launch_bounds__(kBlock) void scatter_channel_kernel(int64_t nb, int64_t nc,
    const int64_t* __restrict__ ptr, const double* __restrict__ in, int k, int c, double* vals)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t i = nb + t / 3, d = t % 3;
  if (i >= nc) return;
  const int64_t p = ptr[i] + k;
  if (p < ptr[i + 1]) vals[p * 18 + d * 6 + c] = in[3 * i + d];
}

// out[pos[k]] = vals[k] (36 doubles per block): this rank's blocks into the replicated operator
__global__ __launch_bounds__(kBlock) void scatter_blocks_kernel(int64_t nnzb, const int64_t* __restrict__ pos,
    const double* __restrict__ vals, double* out)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nnzb * 36) return;
  const int64_t k = t / 36, q = t - 36 * k;
  out[pos[k] * 36 + q] = vals[t];
}

// out[pos[k]] += vals[k] (36 doubles per block; pos unique within one launch)
__global__ __launch_bounds__(kBlock) void add_blocks_kernel(int64_t nnzb, const int64_t* __restrict__ pos,
    const double* __restrict__ vals, double* out)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nnzb * 36) return;
  const int64_t k = t / 36, q = t - 36 * k;
  out[pos[k] * 36 + q] += vals[t];
}

// dst[k] = src[idx[k]] (6 doubles per item)
__global__ __launch_bounds__(kBlock) void gather_items_kernel(int64_t n, const int32_t* __restrict__ idx,
    const double* __restrict__ src, double* dst)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n * 6) return;
  const int64_t k = t / 6, c = t - 6 * k;
  dst[t] = src[int64_t(idx[k]) * 6 + c];
}

// dst[idx[k]] += src[k] (6 doubles per item; idx unique within one launch)
__global__ __launch_bounds__(kBlock) void add_items_kernel(int64_t n, const int32_t* __restrict__ idx,
    const double* __restrict__ src, double* dst)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n * 6) return;
  const int64_t k = t / 6, c = t - 6 * k;
  dst[int64_t(idx[k]) * 6 + c] += src[t];
}

// M slots of 36 doubles per item: the P_1 row of owned node idx[k] (zeros past the row's end)
__global__ __launch_bounds__(kBlock) void pack_rows_kernel(int64_t n, const int32_t* __restrict__ idx, int M,
    const int64_t* __restrict__ ptr, const double* __restrict__ vals, double* out)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n * M * 36) return;
  const int64_t k = t / (int64_t(M) * 36), rem = t - k * M * 36, j = rem / 36, e = rem - 36 * j;
  const int64_t l = idx[k], p = ptr[l] + j;
  out[t] = p < ptr[l + 1] ? vals[p * 36 + e] : 0.0;
}

// ... into the ghost rows of an extended BSR (item k = ghost k in column order: row k below d0,
// k + na above)
__global__ __launch_bounds__(kBlock) void unpack_rows_kernel(int64_t n, int64_t d0, int64_t na, int M,
    const int64_t* __restrict__ ptr, const double* __restrict__ in, double* vals)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n * M * 36) return;
  const int64_t k = t / (int64_t(M) * 36), rem = t - k * M * 36, j = rem / 36, e = rem - 36 * j;
  const int64_t row = k < d0 ? k : k + na, p = ptr[row] + j;
  if (p < ptr[row + 1]) vals[p * 36 + e] = in[t];
}

void copy_dd(double* dst, const double* src, int64_t n, hipStream_t s)
{
  if (n > 0) ck(hipMemcpyAsync(dst, src, sizeof(double) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, s), "copy");
}

// the owned rows of a 3 x 6 BSR (global ids) followed by the ghost rows' ids, imported from their
// owners one block slot at a time (M slots); returns the extended pattern in global ids
void extend_pattern(fcg_amg* h, Coupled* c, const Bsr& B, int64_t off, int M, const fcg_transport* tr,
    hipStream_t s, std::vector<int64_t>& pp, std::vector<int32_t>& pc)
{
  const fcg::DeviceMesh& m = h->ctx->mesh;
  const int64_t nb0 = h->nb0, nc = c->nc_nodes;
  std::vector<std::vector<int32_t>> gid(static_cast<size_t>(nc - nb0));
  std::vector<double> colv(static_cast<size_t>(m.n_cols));
  const dim3 gp(blocks_for(3 * std::max<int64_t>(1, nb0))), bl(kBlock);
  for (int k = 0; k < M; ++k)
  {
    hipLaunchKernelGGL(pack_channel_kernel, gp, bl, 0, s, nb0, B.ptr, B.col, B.vals, k, -1, off, c->chan);
    ck(hipGetLastError(), "pack_channel_kernel");
    ck(tr->import_fn(tr->user, c->chan, c->chan_col, s), "transport import (ghost row ids)");
    ck(hipMemcpyAsync(colv.data(), c->chan_col, sizeof(double) * colv.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
    ck(hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int64_t i = nb0; i < nc; ++i)
    {
      const double id = colv[static_cast<size_t>(3 * i)];
      if (id >= 0.0) gid[static_cast<size_t>(i - nb0)].push_back(int32_t(id));
    }
  }
  pp.assign(static_cast<size_t>(nc) + 1, 0);
  pc.clear();
  for (int64_t i = 0; i < nb0; ++i)
  {
    for (int64_t k = B.ptr_h[static_cast<size_t>(i)]; k < B.ptr_h[static_cast<size_t>(i) + 1]; ++k) pc.push_back(int32_t(B.col_h[static_cast<size_t>(k)] + off));
    pp[static_cast<size_t>(i) + 1] = int64_t(pc.size());
  }
  for (int64_t i = nb0; i < nc; ++i)
  {
    const auto& row = gid[static_cast<size_t>(i - nb0)];
    for (size_t k = 1; k < row.size(); ++k)
      if (row[k] <= row[k - 1]) throw Fail{FCG_ERR_ARG, "coupled AMG: ghost row not sorted"};
    pc.insert(pc.end(), row.begin(), row.end());
    pp[static_cast<size_t>(i) + 1] = int64_t(pc.size());
  }
}

// the ghost rows' values of an extended BSR (pattern from extend_pattern), 6 channels per slot
void extend_values(fcg_amg* h, Coupled* c, const Bsr& B, Bsr& E, int M, const fcg_transport* tr, hipStream_t s)
{
  const int64_t nb0 = h->nb0, nc = c->nc_nodes;
  if (B.nnzb > 0)
    ck(hipMemcpyAsync(E.vals, B.vals, sizeof(double) * static_cast<size_t>(B.nnzb) * 18, hipMemcpyDeviceToDevice, s), "copy");
  const dim3 gp(blocks_for(3 * std::max<int64_t>(1, nb0))), gg(blocks_for(3 * std::max<int64_t>(1, nc - nb0))),
      bl(kBlock);
  for (int k = 0; k < M; ++k)
    for (int col = 0; col < 6; ++col)
    {
      hipLaunchKernelGGL(pack_channel_kernel, gp, bl, 0, s, nb0, B.ptr, B.col, B.vals, k, col, int64_t(0), c->chan);
      ck(hipGetLastError(), "pack_channel_kernel");
      ck(tr->import_fn(tr->user, c->chan, c->chan_col, s), "transport import (ghost rows)");
      if (nc > nb0)
        hipLaunchKernelGGL(scatter_channel_kernel, gg, bl, 0, s, nb0, nc, E.ptr, c->chan_col, k, col, E.vals);
      ck(hipGetLastError(), "scatter_channel_kernel");
    }
}

int widest_over_ranks(const Bsr& B, int rank, int R, const fcg_transport* tr, hipStream_t s)
{
  std::vector<double> v(static_cast<size_t>(R), 0.0);
  int64_t w = 0;
  for (int64_t i = 0; i < B.n; ++i) w = std::max(w, B.ptr_h[static_cast<size_t>(i) + 1] - B.ptr_h[static_cast<size_t>(i)]);
  v[static_cast<size_t>(rank)] = double(w);
  host_allsum(tr, v, s);
  int M = 0;
  for (double x : v) M = std::max(M, int(x));
  return M;
}

// a BSR whose device arrays hold the pattern only (no values), freed with the object
struct TmpPattern {
  Bsr b;
  TmpPattern(const std::vector<int64_t>& ptr, const std::vector<int32_t>& col)
  {
    b.n = int64_t(ptr.size()) - 1;
    b.nnzb = ptr.back();
    b.ptr_h = ptr;
    b.col_h = col;
    ck(hipMalloc(&b.ptr, sizeof(int64_t) * ptr.size()), "hipMalloc");
    ck(hipMalloc(&b.col, sizeof(int32_t) * std::max<size_t>(1, col.size())), "hipMalloc");
    ck(hipMemcpy(b.ptr, ptr.data(), sizeof(int64_t) * ptr.size(), hipMemcpyHostToDevice), "hipMemcpy");
    if (!col.empty()) ck(hipMemcpy(b.col, col.data(), sizeof(int32_t) * col.size(), hipMemcpyHostToDevice), "hipMemcpy");
  }
  ~TmpPattern()
  {
    if (b.ptr) (void)hipFree(b.ptr);
    if (b.col) (void)hipFree(b.col);
  }
  TmpPattern(const TmpPattern&) = delete;
  TmpPattern& operator=(const TmpPattern&) = delete;
};

// the replicated operator's pattern: the union of every rank's blocks (rows row_off + i of its
// part, global columns), gathered once, sorted and deduplicated identically everywhere; pos =
// each of this rank's blocks in it
void gather_replicated(Coupled* c, const fcg_transport* tr, const std::vector<int64_t>& cp,
    const std::vector<int32_t>& cc, int64_t row_off, int64_t n_tot, hipStream_t s,
    std::vector<int64_t>& gptr, std::vector<int32_t>& gcol, std::vector<int64_t>& pos)
{
  const int64_t R = c->nranks;
  std::vector<int64_t> keys;
  {
    std::vector<double> cnt(static_cast<size_t>(R), 0.0);
    cnt[static_cast<size_t>(c->rank)] = double(cc.size());
    host_allsum(tr, cnt, s);
    int64_t first = 0, total = 0;
    for (int64_t q = 0; q < R; ++q)
    {
      if (q < c->rank) first += int64_t(cnt[static_cast<size_t>(q)]);
      total += int64_t(cnt[static_cast<size_t>(q)]);
    }
    std::vector<double> pairs(static_cast<size_t>(2 * total), 0.0);
    const int64_t nrows = int64_t(cp.size()) - 1;
    for (int64_t i = 0; i < nrows; ++i)
      for (int64_t k = cp[static_cast<size_t>(i)]; k < cp[static_cast<size_t>(i) + 1]; ++k)
      {
        pairs[static_cast<size_t>(2 * (first + k))] = double(row_off + i);
        pairs[static_cast<size_t>(2 * (first + k) + 1)] = double(cc[static_cast<size_t>(k)]);
      }
    host_allsum(tr, pairs, s);
    keys.resize(static_cast<size_t>(total));
    for (int64_t k = 0; k < total; ++k)
      keys[static_cast<size_t>(k)] = int64_t(pairs[static_cast<size_t>(2 * k)]) * n_tot + int64_t(pairs[static_cast<size_t>(2 * k + 1)]);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  }
  gptr.assign(static_cast<size_t>(n_tot) + 1, 0);
  gcol.assign(keys.size(), 0);
  for (size_t k = 0; k < keys.size(); ++k)
  {
    gptr[static_cast<size_t>(keys[k] / n_tot) + 1] += 1;
    gcol[k] = int32_t(keys[k] % n_tot);
  }
  for (int64_t i = 0; i < n_tot; ++i) gptr[static_cast<size_t>(i) + 1] += gptr[static_cast<size_t>(i)];
  pos.assign(cc.size(), 0);
  const int64_t nrows = int64_t(cp.size()) - 1;
  for (int64_t i = 0; i < nrows; ++i)
    for (int64_t k = cp[static_cast<size_t>(i)]; k < cp[static_cast<size_t>(i) + 1]; ++k)
      pos[static_cast<size_t>(k)] = int64_t(std::lower_bound(keys.begin(), keys.end(), (row_off + i) * n_tot + cc[static_cast<size_t>(k)]) - keys.begin());
}

// the replicated hierarchy below the replicated operator (pattern gptr / gcol, near-null space ns)
void build_replicated(fcg_amg* h, Coupled* c, std::vector<int64_t> gptr, std::vector<int32_t> gcol,
    int64_t n_tot, std::vector<double> ns)
{
  fcg_amg* g = new fcg_amg();
  c->g = g;
  g->ctx = h->ctx;
  g->device = h->device;
  g->opt = h->opt;
  g->steps.emplace_back();  // step 0 (into the replicated level) is the ranks' prolongator
  g->levels.emplace_back();
  {
    Level& L1 = g->levels[0];
    make_bsr(g, L1.A, std::move(gptr), std::move(gcol), 6, 6, n_tot);
    L1.diag = upload(g, diag_index(L1.A));
    L1.dinv = dalloc<double>(g, 36 * n_tot);
    for (double** v : {&L1.x, &L1.b, &L1.r, &L1.d, &L1.z, &L1.p, &L1.q}) *v = dalloc<double>(g, 6 * n_tot);
  }
  c->rep_nnzb = g->levels[0].A.nnzb;
  c->rep_n = n_tot;
  coarsen(g, &g->levels[0].A, 6, std::move(ns), nullptr);
  g->partial = dalloc<double>(g, kMaxPartials);
  g->sc = dalloc<double>(g, 16);
  g->flag = dalloc<int32_t>(g, 1);
  c->gb = dalloc<double>(h, 6 * n_tot);
  c->ge = dalloc<double>(h, 6 * n_tot);
}

// Is coarse level `level` (global size n_agg_tot block rows, at least min_agg_per_rank on every
// rank) distributed across the ranks?  Default: when its global size passes FCG_AMG_DIST_MIN DOFs
// (50000), so that the replicated level below stays under that size whatever the rank count.
// FCG_AMG_DIST=1 forces level 1 (the deeper levels keep the size rule), 0 distributes none;
// FCG_AMG_DIST_LEVELS caps the distributed levels (default 8).  The inputs are the same on every
// rank, so every rank decides alike.
bool distribute_level(const fcg_transport* tr, int level, int64_t n_agg_tot, int64_t min_agg_per_rank)
{
  if (!tr->exchange_fn || min_agg_per_rank < 1) return false;
  const char* e = std::getenv("FCG_AMG_DIST");
  if (e && e[0] == '0') return false;
  const char* lv = std::getenv("FCG_AMG_DIST_LEVELS");
  if (level > (lv ? std::atoi(lv) : 8)) return false;
  if (level == 1 && e && e[0] == '1') return true;
  const char* m = std::getenv("FCG_AMG_DIST_MIN");
  const int64_t min_dofs = m ? std::atoll(m) : 50000;
  return 6 * n_agg_tot > min_dofs;
}

// Coarse level `level` distributed: its owned rows from the partial rows C of the level above (C's
// rows and columns numbered by LA, this level's ids the level above's prolongator reaches, own
// range included), its import plans, and the prolongator to the next level, which is distributed
// in turn (d->next, recursively) or replicated (C2 gathered, the replicated hierarchy built).  ns:
// the near-null space of this rank's nodes of the level (36 doubles each).
Dist* build_dist(fcg_amg* h, Coupled* c, const fcg_transport* tr, const std::vector<int64_t>& counts,
    const std::vector<int64_t>& LA, const Bsr& C, const std::vector<double>& ns, int level, hipStream_t s)
{
  Dist* d = new Dist();
  std::unique_ptr<Dist> guard_d(d);  // freed if the build throws before it is linked
  d->level = level;
  const int R = c->nranks, me = c->rank;
  d->R = R;
  d->me = me;
  d->agg_off.assign(static_cast<size_t>(R) + 1, 0);
  for (int q = 0; q < R; ++q) d->agg_off[static_cast<size_t>(q) + 1] = d->agg_off[static_cast<size_t>(q)] + counts[static_cast<size_t>(q)];
  for (int q = 0; q < me; ++q) d->off += counts[static_cast<size_t>(q)];
  d->na = counts[static_cast<size_t>(me)];
  d->NL = int64_t(LA.size());
  d->own0 = int64_t(std::lower_bound(LA.begin(), LA.end(), d->off) - LA.begin());
  const int64_t na = d->na, own0 = d->own0, off = d->off;
  if (own0 + na > d->NL || LA[static_cast<size_t>(own0)] != off || LA[static_cast<size_t>(own0 + na - 1)] != off + na - 1)
    throw Fail{FCG_ERR_ARG, "coupled AMG: an owned aggregate is missing from P's columns"};
  auto owner = [&](int64_t gid) {
    return int(std::upper_bound(d->agg_off.begin(), d->agg_off.end(), gid) - d->agg_off.begin()) - 1;
  };
  d->c_lo = C.ptr_h[static_cast<size_t>(own0)];
  d->c_hi = C.ptr_h[static_cast<size_t>(own0 + na)];
  // 1. the partial rows of the other ranks' aggregates go to their owners: (row, column) pairs once
  std::vector<std::vector<double>> out(static_cast<size_t>(R));
  d->rows.scnt.assign(static_cast<size_t>(R), 0);
  for (int64_t r = 0; r < d->NL; ++r)
  {
    if (r >= own0 && r < own0 + na) continue;
    const int q = owner(LA[static_cast<size_t>(r)]);
    for (int64_t k = C.ptr_h[static_cast<size_t>(r)]; k < C.ptr_h[static_cast<size_t>(r) + 1]; ++k)
    {
      out[static_cast<size_t>(q)].push_back(double(LA[static_cast<size_t>(r)]));
      out[static_cast<size_t>(q)].push_back(double(LA[static_cast<size_t>(C.col_h[static_cast<size_t>(k)])]));
    }
    d->rows.scnt[static_cast<size_t>(q)] += C.ptr_h[static_cast<size_t>(r) + 1] - C.ptr_h[static_cast<size_t>(r)];
  }
  std::vector<std::vector<double>> in = host_exchange(tr, out, s);
  d->rows.rcnt.assign(static_cast<size_t>(R), 0);
  std::vector<std::vector<int64_t>> rowcols(static_cast<size_t>(na));
  for (int64_t i = 0; i < na; ++i)
  {
    rowcols[static_cast<size_t>(i)].push_back(off + i);  // the diagonal block
    for (int64_t k = C.ptr_h[static_cast<size_t>(own0 + i)]; k < C.ptr_h[static_cast<size_t>(own0 + i) + 1]; ++k)
      rowcols[static_cast<size_t>(i)].push_back(LA[static_cast<size_t>(C.col_h[static_cast<size_t>(k)])]);
  }
  for (int q = 0; q < R; ++q)
  {
    const auto& v = in[static_cast<size_t>(q)];
    d->rows.rcnt[static_cast<size_t>(q)] = int64_t(v.size() / 2);
    for (size_t k = 0; k + 1 < v.size(); k += 2)
    {
      const int64_t rg = int64_t(v[k]);
      if (rg < off || rg >= off + na) throw Fail{FCG_ERR_ARG, "coupled AMG: partial row sent to the wrong rank"};
      rowcols[static_cast<size_t>(rg - off)].push_back(int64_t(v[k + 1]));
    }
  }
  d->rows.finish();
  std::vector<int64_t> DA;
  for (auto& row : rowcols)
  {
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    DA.insert(DA.end(), row.begin(), row.end());
  }
  std::sort(DA.begin(), DA.end());
  DA.erase(std::unique(DA.begin(), DA.end()), DA.end());
  d->NA = int64_t(DA.size());
  d->d0 = int64_t(std::lower_bound(DA.begin(), DA.end(), off) - DA.begin());
  auto da = [&](int64_t g) { return int32_t(std::lower_bound(DA.begin(), DA.end(), g) - DA.begin()); };
  std::vector<int64_t> aptr(static_cast<size_t>(na) + 1, 0);
  std::vector<int32_t> acol;
  for (int64_t i = 0; i < na; ++i)
  {
    for (int64_t g : rowcols[static_cast<size_t>(i)]) acol.push_back(da(g));
    aptr[static_cast<size_t>(i) + 1] = int64_t(acol.size());
  }
  make_bsr(h, d->A, aptr, acol, 6, 6, d->NA);
  auto block_of = [&](int64_t i, int32_t col) {
    const auto b = acol.begin() + aptr[static_cast<size_t>(i)], e = acol.begin() + aptr[static_cast<size_t>(i) + 1];
    const auto it = std::lower_bound(b, e, col);
    if (it == e || *it != col) throw Fail{FCG_ERR_ARG, "coupled AMG: level-1 block not in the pattern"};
    return int64_t(it - acol.begin());
  };
  {
    std::vector<int64_t> diag(static_cast<size_t>(na)), po(static_cast<size_t>(d->c_hi - d->c_lo)), pr(static_cast<size_t>(d->rows.nr));
    for (int64_t i = 0; i < na; ++i)
    {
      diag[static_cast<size_t>(i)] = block_of(i, int32_t(d->d0 + i));
      for (int64_t k = C.ptr_h[static_cast<size_t>(own0 + i)]; k < C.ptr_h[static_cast<size_t>(own0 + i) + 1]; ++k)
        po[static_cast<size_t>(k - d->c_lo)] = block_of(i, da(LA[static_cast<size_t>(C.col_h[static_cast<size_t>(k)])]));
    }
    int64_t o = 0;
    for (int q = 0; q < R; ++q)
    {
      const auto& v = in[static_cast<size_t>(q)];
      for (size_t k = 0; k + 1 < v.size(); k += 2)
        pr[static_cast<size_t>(o++)] = block_of(int64_t(v[k]) - off, da(int64_t(v[k + 1])));
    }
    d->diag = upload(h, diag);
    d->pos_own = upload(h, po);
    d->pos_recv = upload(h, pr);
  }
  d->dinv = dalloc<double>(h, 36 * na);
  d->rows_s = dalloc<double>(h, 36 * d->rows.ns);
  d->rows_r = dalloc<double>(h, 36 * d->rows.nr);
  // 2. the level-1 import: A's ghost columns (DA outside [d0, d0 + na)) from their owners
  {
    std::vector<std::vector<double>> req(static_cast<size_t>(R));
    d->imp.rcnt.assign(static_cast<size_t>(R), 0);
    for (int64_t j = 0; j < d->NA; ++j)
    {
      if (j >= d->d0 && j < d->d0 + na) continue;
      const int q = owner(DA[static_cast<size_t>(j)]);
      req[static_cast<size_t>(q)].push_back(double(DA[static_cast<size_t>(j)]));
      d->imp.rcnt[static_cast<size_t>(q)] += 1;
    }
    std::vector<std::vector<double>> want = host_exchange(tr, req, s);
    d->imp.scnt.assign(static_cast<size_t>(R), 0);
    std::vector<int32_t> idx;
    for (int q = 0; q < R; ++q)
    {
      d->imp.scnt[static_cast<size_t>(q)] = int64_t(want[static_cast<size_t>(q)].size());
      for (double g : want[static_cast<size_t>(q)])
      {
        const int64_t l = int64_t(g) - off;
        if (l < 0 || l >= na) throw Fail{FCG_ERR_ARG, "coupled AMG: import request for a foreign aggregate"};
        idx.push_back(int32_t(l));
      }
    }
    d->imp.finish();
    d->imp_idx = upload(h, idx);
    d->imp_idx_h = std::move(idx);
    d->imp_s = dalloc<double>(h, 6 * d->imp.ns);
    d->imp_r = dalloc<double>(h, 6 * d->imp.nr);
    d->xe = dalloc<double>(h, 6 * d->NA);
  }
  // 3. restriction / prolongation: LA's other-rank aggregates with their owners
  {
    std::vector<std::vector<double>> req(static_cast<size_t>(R));
    d->pex.scnt.assign(static_cast<size_t>(R), 0);
    for (int64_t r = 0; r < d->NL; ++r)
    {
      if (r >= own0 && r < own0 + na) continue;
      const int q = owner(LA[static_cast<size_t>(r)]);
      req[static_cast<size_t>(q)].push_back(double(LA[static_cast<size_t>(r)]));
      d->pex.scnt[static_cast<size_t>(q)] += 1;
    }
    std::vector<std::vector<double>> got = host_exchange(tr, req, s);
    d->pex.rcnt.assign(static_cast<size_t>(R), 0);
    std::vector<int32_t> idx;
    for (int q = 0; q < R; ++q)
    {
      d->pex.rcnt[static_cast<size_t>(q)] = int64_t(got[static_cast<size_t>(q)].size());
      for (double g : got[static_cast<size_t>(q)])
      {
        const int64_t l = int64_t(g) - off;
        if (l < 0 || l >= na) throw Fail{FCG_ERR_ARG, "coupled AMG: restriction entry for a foreign aggregate"};
        idx.push_back(int32_t(l));
      }
    }
    d->pex.finish();
    d->pex_idx = upload(h, idx);
    d->pex_s = dalloc<double>(h, 6 * d->pex.ns);
    d->pex_r = dalloc<double>(h, 6 * d->pex.nr);
    d->y = dalloc<double>(h, 6 * d->NL);
  }
  for (double** v : {&d->x, &d->b, &d->r, &d->dd, &d->z, &d->p, &d->q}) *v = dalloc<double>(h, 6 * na);
  // 4. level 2: a rank-local aggregation of A's owned block, its tentative prolongator T_1
  std::vector<int32_t> agg1(static_cast<size_t>(na), -1);
  std::vector<double> tent(static_cast<size_t>(na) * 36), ns2;
  {
    std::vector<int64_t> optr(static_cast<size_t>(na) + 1, 0);
    std::vector<int32_t> ocol;
    for (int64_t i = 0; i < na; ++i)
    {
      for (int64_t k = aptr[static_cast<size_t>(i)]; k < aptr[static_cast<size_t>(i) + 1]; ++k)
        if (acol[static_cast<size_t>(k)] >= d->d0 && acol[static_cast<size_t>(k)] < d->d0 + na) ocol.push_back(int32_t(acol[static_cast<size_t>(k)] - d->d0));
      optr[static_cast<size_t>(i) + 1] = int64_t(ocol.size());
    }
    d->n2 = fcg_amg_aggregate(na, optr.data(), ocol.data(), nullptr, agg1.data());
    if (d->n2 <= 0) throw Fail{FCG_ERR_ARG, "coupled AMG: level-1 aggregation failed"};
    ns2.assign(static_cast<size_t>(d->n2) * 36, 0.0);
    int64_t nd = 0;
    if (int64_t(ns.size()) != 36 * na) throw Fail{FCG_ERR_ARG, "coupled AMG: near-null space size"};
    ck(fcg_amg_tentative(na, 6, ns.data(), agg1.data(), d->n2, tent.data(), ns2.data(), &nd),
        "fcg_amg_tentative (distributed level)");
  }
  std::vector<int64_t> counts2(static_cast<size_t>(R), 0);
  int64_t min2 = 0;
  {
    std::vector<double> v(static_cast<size_t>(R), 0.0);
    v[static_cast<size_t>(me)] = double(d->n2);
    host_allsum(tr, v, s);
    min2 = int64_t(v[0]);
    for (int q = 0; q < R; ++q)
    {
      counts2[static_cast<size_t>(q)] = int64_t(v[static_cast<size_t>(q)]);
      if (q < me) d->off2 += counts2[static_cast<size_t>(q)];
      d->n2_tot += counts2[static_cast<size_t>(q)];
      min2 = std::min(min2, counts2[static_cast<size_t>(q)]);
    }
  }
  // the next level distributed too when it is still large (and coarser than this one)
  const int64_t n1_tot = d->agg_off.back();
  const bool next_dist = d->n2_tot < n1_tot && distribute_level(tr, level + 1, d->n2_tot, min2);
  // T_1,ext: A's column rows of T_1 (global level-2 ids), the ghost ones from their owners once
  std::vector<int64_t> eptr(static_cast<size_t>(d->NA) + 1, 0);
  std::vector<int32_t> ecol;
  std::vector<double> ev;
  {
    std::vector<std::vector<double>> rowsout(static_cast<size_t>(R));
    for (int q = 0, o = 0; q < R; ++q)
      for (int64_t k = 0; k < d->imp.scnt[static_cast<size_t>(q)]; ++k)
      {
        const int32_t l = d->imp_idx_h[static_cast<size_t>(o++)];
        const int32_t a = agg1[static_cast<size_t>(l)];
        rowsout[static_cast<size_t>(q)].push_back(a >= 0 ? double(d->off2 + a) : -1.0);
        for (int t = 0; t < 36; ++t) rowsout[static_cast<size_t>(q)].push_back(a >= 0 ? tent[static_cast<size_t>(36 * l + t)] : 0.0);
      }
    std::vector<std::vector<double>> rin = host_exchange(tr, rowsout, s);
    std::vector<double> gh;  // the ghost rows in DA order (ascending global id = rank order)
    for (int q = 0; q < R; ++q) gh.insert(gh.end(), rin[static_cast<size_t>(q)].begin(), rin[static_cast<size_t>(q)].end());
    if (int64_t(gh.size()) != 37 * d->imp.nr) throw Fail{FCG_ERR_ARG, "coupled AMG: T_1 ghost rows incomplete"};
    for (int64_t j = 0, gi = 0; j < d->NA; ++j)
    {
      if (j >= d->d0 && j < d->d0 + na)
      {
        const int64_t l = j - d->d0;
        if (agg1[static_cast<size_t>(l)] >= 0)
        {
          ecol.push_back(int32_t(d->off2 + agg1[static_cast<size_t>(l)]));
          ev.insert(ev.end(), tent.begin() + 36 * l, tent.begin() + 36 * (l + 1));
        }
      }
      else
      {
        const double* row = gh.data() + 37 * gi++;
        if (row[0] >= 0.0)
        {
          ecol.push_back(int32_t(row[0]));
          ev.insert(ev.end(), row + 1, row + 37);
        }
      }
      eptr[static_cast<size_t>(j) + 1] = int64_t(ecol.size());
    }
  }
  // P_1 = (I - w D^-1 A) T_1,ext on the pattern of A T_1,ext (smoothed with the distributed A_1:
  // its rows reach the neighbour ranks' level-2 aggregates), its transpose, and P_1,ext: the ghost
  // rows' patterns from their owners once (M1 column slots per row), their values per tangent
  std::vector<int64_t> a1p, tp, ep, ap1, c2p;
  std::vector<int32_t> a1c, tc, ec, ac1, c2c;
  symbolic(d->A, eptr, ecol, d->n2_tot, a1p, a1c);
  {
    std::vector<double> v(static_cast<size_t>(R), 0.0);
    int64_t w = 0;
    for (int64_t i = 0; i < na; ++i) w = std::max(w, a1p[static_cast<size_t>(i) + 1] - a1p[static_cast<size_t>(i)]);
    v[static_cast<size_t>(me)] = double(w);
    host_allsum(tr, v, s);
    for (double x : v) d->M1 = std::max(d->M1, int(x));
  }
  {
    std::vector<std::vector<double>> rowsout(static_cast<size_t>(R));
    for (int q = 0, o = 0; q < R; ++q)
      for (int64_t k = 0; k < d->imp.scnt[static_cast<size_t>(q)]; ++k)
      {
        const int32_t l = d->imp_idx_h[static_cast<size_t>(o++)];
        const int64_t b0 = a1p[static_cast<size_t>(l)], b1 = a1p[static_cast<size_t>(l) + 1];
        for (int64_t j = 0; j < d->M1; ++j)
          rowsout[static_cast<size_t>(q)].push_back(b0 + j < b1 ? double(a1c[static_cast<size_t>(b0 + j)]) : -1.0);
      }
    std::vector<std::vector<double>> rin = host_exchange(tr, rowsout, s);
    std::vector<double> gh;
    for (int q = 0; q < R; ++q) gh.insert(gh.end(), rin[static_cast<size_t>(q)].begin(), rin[static_cast<size_t>(q)].end());
    if (int64_t(gh.size()) != d->M1 * d->imp.nr) throw Fail{FCG_ERR_ARG, "coupled AMG: P_1 ghost rows incomplete"};
    ep.assign(static_cast<size_t>(d->NA) + 1, 0);
    for (int64_t j = 0, gi = 0; j < d->NA; ++j)
    {
      if (j >= d->d0 && j < d->d0 + na)
      {
        const int64_t l = j - d->d0;
        ec.insert(ec.end(), a1c.begin() + a1p[static_cast<size_t>(l)], a1c.begin() + a1p[static_cast<size_t>(l) + 1]);
      }
      else
      {
        for (int64_t k = 0; k < d->M1; ++k)
        {
          const double col = gh[static_cast<size_t>(d->M1 * gi + k)];
          if (col >= 0.0) ec.push_back(int32_t(col));
        }
        ++gi;
      }
      ep[static_cast<size_t>(j) + 1] = int64_t(ec.size());
    }
  }
  // the column space of P_1: the global level-2 ids (replicated next level), or the next level's
  // LA -- the level-2 ids P_1,ext reaches, ascending (P_1's own rows reach every owned aggregate)
  std::vector<int64_t> LA2;
  d->n2_cols = d->n2_tot;
  std::vector<int32_t> ag(static_cast<size_t>(na));
  for (int64_t i = 0; i < na; ++i)
    ag[static_cast<size_t>(i)] = agg1[static_cast<size_t>(i)] >= 0 ? int32_t(d->off2 + agg1[static_cast<size_t>(i)]) : -1;
  if (next_dist)
  {
    LA2.assign(ec.begin(), ec.end());
    std::sort(LA2.begin(), LA2.end());
    LA2.erase(std::unique(LA2.begin(), LA2.end()), LA2.end());
    auto g2l = [&](int32_t g) {
      const auto it = std::lower_bound(LA2.begin(), LA2.end(), int64_t(g));
      if (it == LA2.end() || *it != g) throw Fail{FCG_ERR_ARG, "coupled AMG: level-2 aggregate outside P_1,ext's columns"};
      return int32_t(it - LA2.begin());
    };
    for (auto* v : {&ecol, &a1c, &ec})
      for (auto& x : *v) x = g2l(x);
    for (auto& x : ag)
      if (x >= 0) x = g2l(x);
    d->n2_cols = int64_t(LA2.size());
  }
  d->agg1 = upload(h, ag);
  d->tent1 = upload(h, tent);
  make_bsr(h, d->T1ext, eptr, ecol, 6, 6, d->n2_cols);
  if (!ev.empty())
    ck(hipMemcpy(d->T1ext.vals, ev.data(), sizeof(double) * ev.size(), hipMemcpyHostToDevice), "hipMemcpy");
  make_bsr(h, d->AT1, a1p, a1c, 6, 6, d->n2_cols);
  make_bsr(h, d->P1, a1p, a1c, 6, 6, d->n2_cols);
  {
    tp.assign(static_cast<size_t>(d->n2_cols) + 1, 0);
    tc.assign(std::max<size_t>(1, a1c.size()), 0);
    std::vector<int64_t> perm(std::max<size_t>(1, a1c.size()));
    ck(fcg_bsr_transpose_pattern(na, d->n2_cols, a1p.data(), a1c.data(), tp.data(), tc.data(), perm.data()),
        "fcg_bsr_transpose_pattern (P_1)");
    tc.resize(a1c.size());
    perm.resize(a1c.size());
    make_bsr(h, d->P1t, tp, tc, 6, 6, na);
    d->p1_perm = upload(h, perm);
  }
  make_bsr(h, d->P1ext, ep, ec, 6, 6, d->n2_cols);
  d->p1_s = dalloc<double>(h, 36 * d->M1 * d->imp.ns);
  d->p1_r = dalloc<double>(h, 36 * d->M1 * d->imp.nr);
  // this rank's part of A_2 = P_1^T (A P_1,ext): rows of every level-2 aggregate its P_1 reaches
  symbolic(d->A, ep, ec, d->n2_cols, ap1, ac1);
  make_bsr(h, d->AP1, ap1, ac1, 6, 6, d->n2_cols);
  symbolic(d->P1t, ap1, ac1, d->n2_cols, c2p, c2c);
  make_bsr(h, d->C2, c2p, c2c, 6, 6, d->n2_cols);
  if (next_dist)
  {
    std::vector<double> ns_next(ns2.begin(), ns2.begin() + 36 * d->n2);
    d->next = build_dist(h, c, tr, counts2, LA2, d->C2, ns_next, level + 1, s);
  }
  else
  {
    std::vector<int64_t> gptr, pos;
    std::vector<int32_t> gcol;
    gather_replicated(c, tr, c2p, c2c, 0, d->n2_tot, s, gptr, gcol, pos);
    c->rep_part = &d->C2;
    c->rep_pos = upload(h, pos);
    std::vector<double> nsg(static_cast<size_t>(36 * d->n2_tot), 0.0);
    std::copy(ns2.begin(), ns2.end(), nsg.begin() + 36 * d->off2);
    host_allsum(tr, nsg, s);
    build_replicated(h, c, std::move(gptr), std::move(gcol), d->n2_tot, std::move(nsg));
  }
  return guard_d.release();
}

void coupled_build(fcg_amg* h, const fcg_transport* tr, hipStream_t s)
{
  const fcg::DeviceMesh& m = h->ctx->mesh;
  Coupled* c = new Coupled();
  h->cpl = c;
  c->rank = tr->rank;
  c->nranks = tr->nranks;
  c->nc_nodes = m.n_cols / 3;
  const int64_t nb0 = h->nb0, nc = c->nc_nodes, R = c->nranks;
  const Step& st0 = h->steps[0];
  // aggregates per rank: the global numbering by rank offsets
  std::vector<int64_t> counts(static_cast<size_t>(R), 0);
  int64_t min_agg = 0;
  {
    std::vector<double> v(static_cast<size_t>(R), 0.0);
    v[static_cast<size_t>(c->rank)] = double(st0.n_agg);
    host_allsum(tr, v, s);
    min_agg = int64_t(v[0]);
    for (int64_t q = 0; q < R; ++q)
    {
      counts[static_cast<size_t>(q)] = int64_t(v[static_cast<size_t>(q)]);
      if (q < c->rank) c->off += counts[static_cast<size_t>(q)];
      c->n_agg_tot += counts[static_cast<size_t>(q)];
      min_agg = std::min(min_agg, counts[static_cast<size_t>(q)]);
    }
  }
  const bool dist = distribute_level(tr, 1, c->n_agg_tot, min_agg);
  c->chan = dalloc<double>(h, 3 * nb0);
  c->chan_col = dalloc<double>(h, m.n_cols);
  c->q = dalloc<double>(h, 3 * nb0);
  c->w = dalloc<double>(h, 3 * nb0);
  make_bsr(h, c->Afull, h->full_ptr, h->full_col, 3, 3, nc);
  // T_0 with the ghost rows of its owners (one block per row), then P = (I - w D^-1 A) T_ext on
  // the pattern of A_full T_ext: P's rows reach the neighbour ranks' aggregates (global ids)
  std::vector<int64_t> pp, ap, tp, cp;
  std::vector<int32_t> pc, apc, tc, cc;
  extend_pattern(h, c, st0.T, c->off, widest_over_ranks(st0.T, c->rank, int(R), tr, s), tr, s, pp, pc);
  std::vector<int64_t> LA;  // P's aggregate numbering: global ids (replicated) or LA (distributed)
  int64_t n_p_cols = c->n_agg_tot;
  std::vector<int64_t> pp2;
  std::vector<int32_t> pc2;
  {
    // P's pattern and its ghost rows (global ids)
    symbolic(c->Afull, pp, pc, c->n_agg_tot, ap, apc);
    TmpPattern Pg(ap, apc);
    c->M = widest_over_ranks(Pg.b, c->rank, int(R), tr, s);
    extend_pattern(h, c, Pg.b, 0, c->M, tr, s, pp2, pc2);
  }
  std::vector<int32_t> agg_h(static_cast<size_t>(nb0));
  ck(hipMemcpy(agg_h.data(), st0.agg, sizeof(int32_t) * agg_h.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  if (dist)
  {
    // LA: the aggregates P_ext reaches, ascending (the order of every pattern row is kept)
    LA.assign(pc2.begin(), pc2.end());
    std::sort(LA.begin(), LA.end());
    LA.erase(std::unique(LA.begin(), LA.end()), LA.end());
    auto g2l = [&](int32_t g) {
      const auto it = std::lower_bound(LA.begin(), LA.end(), int64_t(g));
      if (it == LA.end() || *it != g) throw Fail{FCG_ERR_ARG, "coupled AMG: aggregate outside P_ext's columns"};
      return int32_t(it - LA.begin());
    };
    for (auto* v : {&pc, &apc, &pc2})
      for (auto& x : *v) x = g2l(x);
    n_p_cols = int64_t(LA.size());
    const int64_t own0 = int64_t(std::lower_bound(LA.begin(), LA.end(), c->off) - LA.begin());
    for (auto& a : agg_h)
      if (a >= 0) a = int32_t(a + own0);
  }
  else
    for (auto& a : agg_h)
      if (a >= 0) a = int32_t(a + c->off);
  c->agg = upload(h, agg_h);
  make_bsr(h, c->Text, pp, pc, 3, 6, n_p_cols);
  make_bsr(h, c->AT, ap, apc, 3, 6, n_p_cols);
  make_bsr(h, c->P, ap, apc, 3, 6, n_p_cols);
  tp.assign(static_cast<size_t>(n_p_cols) + 1, 0);
  tc.assign(static_cast<size_t>(std::max<int64_t>(ap.back(), 1)), 0);
  std::vector<int64_t> perm(static_cast<size_t>(std::max<int64_t>(ap.back(), 1)));
  ck(fcg_bsr_transpose_pattern(nb0, n_p_cols, ap.data(), apc.data(), tp.data(), tc.data(), perm.data()),
      "fcg_bsr_transpose_pattern");
  tc.resize(static_cast<size_t>(ap.back()));
  perm.resize(static_cast<size_t>(ap.back()));
  make_bsr(h, c->Pt, tp, tc, 6, 3, nb0);
  c->p_perm = upload(h, perm);
  // this rank's part of A_1 = P^T (A P_ext)
  make_bsr(h, c->Pext, pp2, pc2, 3, 6, n_p_cols);
  std::vector<int64_t> app;
  std::vector<int32_t> appc;
  symbolic(c->Afull, c->Pext.ptr_h, c->Pext.col_h, n_p_cols, app, appc);
  make_bsr(h, c->AP, app, appc, 3, 6, n_p_cols);
  symbolic(c->Pt, app, appc, n_p_cols, cp, cc);
  make_bsr(h, c->C, cp, cc, 6, 6, n_p_cols);
  if (dist)
    c->d = build_dist(h, c, tr, counts, LA, c->C, h->ns1, 1, s);
  else
  {
    std::vector<int64_t> gptr, pos;
    std::vector<int32_t> gcol;
    gather_replicated(c, tr, cp, cc, 0, c->n_agg_tot, s, gptr, gcol, pos);
    c->rep_part = &c->C;
    c->rep_pos = upload(h, pos);
    // level 1's near-null space: each aggregate's R factor from its owner
    std::vector<double> ns(static_cast<size_t>(36 * c->n_agg_tot), 0.0);
    std::copy(h->ns1.begin(), h->ns1.end(), ns.begin() + 36 * c->off);
    host_allsum(tr, ns, s);
    build_replicated(h, c, std::move(gptr), std::move(gcol), c->n_agg_tot, std::move(ns));
  }
  // T_0's ghost rows: the tentative prolongator is fixed at create, so they are imported once
  extend_values(h, c, st0.T, c->Text, 1, tr, s);
}

// y = A_1 x on the owned rows: x into the extended vector, its ghost entries imported
void dist_spmv(fcg_amg* h, Dist* d, const fcg_transport* tr, const double* x, double* y, hipStream_t s)
{
  Coupled* c = h->cpl;
  copy_dd(d->xe + 6 * d->d0, x, 6 * d->na, s);
  if (d->imp.ns > 0)
    hipLaunchKernelGGL(gather_items_kernel, dim3(blocks_for(6 * d->imp.ns)), dim3(kBlock), 0, s, d->imp.ns,
        d->imp_idx, x, d->imp_s);
  ck(hipGetLastError(), "gather_items_kernel");
  exchange_counted(c, tr, d->imp, 6, false, d->imp_s, d->imp_r, s, "transport exchange (level-1 import)");
  copy_dd(d->xe, d->imp_r, 6 * d->d0, s);
  copy_dd(d->xe + 6 * (d->d0 + d->na), d->imp_r + 6 * d->d0, 6 * (d->NA - d->d0 - d->na), s);
  ck(fcg_bsr_spmv(h->device, 6, 6, d->A.n, d->A.ptr, d->A.col, d->A.vals, d->xe, y, 1.0, 0, s), "fcg_bsr_spmv (level 1)");
}

void dist_dinv(fcg_amg* h, const Dist* d, const double* r, double* z, double scale, bool acc, hipStream_t s)
{
  ck(fcg_bsr_block_jacobi_apply(h->device, 6, d->na, d->dinv, r, z, scale, acc ? 1 : 0, s),
      "fcg_bsr_block_jacobi_apply (level 1)");
}

// numeric: A_1's owned rows from this rank's blocks and the partial rows of the other ranks, its
// block Jacobi and lambda_max, P_1 and this rank's part of A_2
void dist_setup(fcg_amg* h, Dist* d, const Bsr& C, const fcg_transport* tr, hipStream_t s)
{
  Coupled* c = h->cpl;
  ck(hipMemsetAsync(d->A.vals, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(1, d->A.nnzb)) * 36, s), "memset");
  if (d->c_hi > d->c_lo)
    hipLaunchKernelGGL(add_blocks_kernel, dim3(blocks_for((d->c_hi - d->c_lo) * 36)), dim3(kBlock), 0, s,
        d->c_hi - d->c_lo, d->pos_own, C.vals + 36 * d->c_lo, d->A.vals);
  ck(hipGetLastError(), "add_blocks_kernel");
  copy_dd(d->rows_s, C.vals, 36 * d->c_lo, s);
  copy_dd(d->rows_s + 36 * d->c_lo, C.vals + 36 * d->c_hi, 36 * (C.nnzb - d->c_hi), s);
  exchange_counted(c, tr, d->rows, 36, false, d->rows_s, d->rows_r, s, "transport exchange (partial level-1 rows)");
  for (int q = 0, o = 0; q < d->R; ++q)
  {
    const int64_t n = d->rows.rcnt[static_cast<size_t>(q)];
    if (n > 0)
      hipLaunchKernelGGL(add_blocks_kernel, dim3(blocks_for(n * 36)), dim3(kBlock), 0, s, n, d->pos_recv + o,
          d->rows_r + 36 * o, d->A.vals);
    o += int(n);
  }
  ck(hipGetLastError(), "add_blocks_kernel");
  ck(fcg_bsr_block_jacobi_setup(h->device, 6, d->na, d->A.ptr, d->diag, d->A.vals, d->dinv, h->flag, s),
      d->level == 1 ? "coupled AMG level 1: singular diagonal block"
                    : "coupled AMG distributed level: singular diagonal block");
  Ops o{h, 1, nullptr, s, tr};
  o.dl = d;
  estimate_lmax(o);
  ck(fcg_bsr_spgemm(h->device, 6, 6, 6, d->A.n, d->A.ptr, d->A.col, d->A.vals, d->T1ext.ptr, d->T1ext.col,
         d->T1ext.vals, d->AT1.ptr, d->AT1.col, d->AT1.vals, s), "fcg_bsr_spgemm (A_1 T_1,ext)");
  ck(fcg_amg_smooth_prolongator(h->device, 6, d->na, d->P1.ptr, d->P1.col, d->agg1, d->tent1, d->dinv,
         d->AT1.vals, h->opt.omega / d->lmax, d->P1.vals, s), "fcg_amg_smooth_prolongator (level 1)");
  if (d->P1.nnzb > 0)
    ck(fcg_bsr_transpose_values(h->device, 6, 6, d->P1.nnzb, d->p1_perm, d->P1.vals, d->P1t.vals, s),
        "fcg_bsr_transpose_values (P_1)");
  copy_dd(d->P1ext.vals + 36 * d->P1ext.ptr_h[static_cast<size_t>(d->d0)], d->P1.vals, 36 * d->P1.nnzb, s);
  const int64_t w = 36 * int64_t(d->M1);
  if (d->imp.ns > 0)
    hipLaunchKernelGGL(pack_rows_kernel, dim3(blocks_for(w * d->imp.ns)), dim3(kBlock), 0, s, d->imp.ns, d->imp_idx,
        d->M1, d->P1.ptr, d->P1.vals, d->p1_s);
  ck(hipGetLastError(), "pack_rows_kernel");
  exchange_counted(c, tr, d->imp, int(w), false, d->p1_s, d->p1_r, s, "transport exchange (P_1 ghost rows)");
  if (d->imp.nr > 0)
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(blocks_for(w * d->imp.nr)), dim3(kBlock), 0, s, d->imp.nr, d->d0,
        d->na, d->M1, d->P1ext.ptr, d->p1_r, d->P1ext.vals);
  ck(hipGetLastError(), "unpack_rows_kernel");
  ck(fcg_bsr_spgemm(h->device, 6, 6, 6, d->A.n, d->A.ptr, d->A.col, d->A.vals, d->P1ext.ptr, d->P1ext.col,
         d->P1ext.vals, d->AP1.ptr, d->AP1.col, d->AP1.vals, s), "fcg_bsr_spgemm (A_1 P_1,ext)");
  ck(fcg_bsr_spgemm(h->device, 6, 6, 6, d->P1t.n, d->P1t.ptr, d->P1t.col, d->P1t.vals, d->AP1.ptr,
         d->AP1.col, d->AP1.vals, d->C2.ptr, d->C2.col, d->C2.vals, s), "fcg_bsr_spgemm (P_1^T A_1 P_1)");
  if (d->next) dist_setup(h, d->next, d->C2, tr, s);
}

// (dist_coarse and dist_vcycle call each other, one level further down each time)
void dist_vcycle(fcg_amg* h, const fcg_transport* tr, Dist* d, const double* b, double* x, hipStream_t s);

// y (+)= P A_nd^-1 P^T x through the distributed level nd: the restriction by Pt into nd's LA (rows
// of the level above, bs-wide blocks), whose other-rank entries go to their owners and are added
// there (senders in rank order), nd's V-cycle, the reverse exchange, P back
void dist_coarse(fcg_amg* h, const fcg_transport* tr, Dist* nd, int bs, const Bsr& Pt, const Bsr& P,
    const double* x, double* y, int accumulate, hipStream_t s)
{
  Coupled* c = h->cpl;
  const int64_t na = nd->na, own0 = nd->own0, tail = nd->NL - own0 - na;
  ck(fcg_bsr_spmv(h->device, 6, bs, Pt.n, Pt.ptr, Pt.col, Pt.vals, x, nd->y, 1.0, 0, s), "restriction");
  copy_dd(nd->b, nd->y + 6 * own0, 6 * na, s);
  copy_dd(nd->pex_s, nd->y, 6 * own0, s);
  copy_dd(nd->pex_s + 6 * own0, nd->y + 6 * (own0 + na), 6 * tail, s);
  exchange_counted(c, tr, nd->pex, 6, false, nd->pex_s, nd->pex_r, s, "transport exchange (restriction)");
  for (int q = 0, o = 0; q < nd->R; ++q)
  {
    const int64_t n = nd->pex.rcnt[static_cast<size_t>(q)];
    if (n > 0)
      hipLaunchKernelGGL(add_items_kernel, dim3(blocks_for(6 * n)), dim3(kBlock), 0, s, n, nd->pex_idx + o,
          nd->pex_r + 6 * o, nd->b);
    o += int(n);
  }
  ck(hipGetLastError(), "add_items_kernel");
  dist_vcycle(h, tr, nd, nd->b, nd->x, s);
  if (nd->pex.nr > 0)
    hipLaunchKernelGGL(gather_items_kernel, dim3(blocks_for(6 * nd->pex.nr)), dim3(kBlock), 0, s, nd->pex.nr,
        nd->pex_idx, nd->x, nd->pex_r);
  ck(hipGetLastError(), "gather_items_kernel");
  exchange_counted(c, tr, nd->pex, 6, true, nd->pex_r, nd->pex_s, s, "transport exchange (prolongation)");
  copy_dd(nd->y + 6 * own0, nd->x, 6 * na, s);
  copy_dd(nd->y, nd->pex_s, 6 * own0, s);
  copy_dd(nd->y + 6 * (own0 + na), nd->pex_s + 6 * own0, 6 * tail, s);
  ck(fcg_bsr_spmv(h->device, bs, 6, P.n, P.ptr, P.col, P.vals, nd->y, y, 1.0, accumulate, s), "prolongation");
}

// one V-cycle of a distributed level: Chebyshev with its A, the residual restricted by P_1^T into
// the next level -- distributed in turn (dist_coarse), or replicated (each rank's partial sums,
// completed by the all-reduce, and the replicated hierarchy) -- P_1 back, Chebyshev again
void dist_vcycle(fcg_amg* h, const fcg_transport* tr, Dist* d, const double* b, double* x, hipStream_t s)
{
  Coupled* c = h->cpl;
  Ops o{h, 1, nullptr, s, tr};
  o.dl = d;
  cheb(h, o, b, x, true);
  o.spmv(x, d->r);
  rsub(b, d->r, 6 * d->na, s);
  if (d->next)
    dist_coarse(h, tr, d->next, 6, d->P1t, d->P1, d->r, x, 1, s);
  else
  {
    ck(fcg_bsr_spmv(h->device, 6, 6, d->P1t.n, d->P1t.ptr, d->P1t.col, d->P1t.vals, d->r, c->gb, 1.0, 0, s),
        "restriction (distributed level)");
    allreduce_counted(c, tr, c->gb, 6 * d->n2_tot, s, "transport all-reduce (replicated level)");
    vcycle(c->g, 1, nullptr, c->gb, c->ge, s);
    ck(fcg_bsr_spmv(h->device, 6, 6, d->P1.n, d->P1.ptr, d->P1.col, d->P1.vals, c->ge, x, 1.0, 1, s),
        "prolongation (distributed level)");
  }
  cheb(h, o, b, x, false);
}

// numeric part per tangent, after the local setup (T_0, the nodal block inverses)
void coupled_setup(fcg_amg* h, const double* K, const fcg_transport* tr, hipStream_t s)
{
  Coupled* c = h->cpl;
  c->ctr_ar = c->ctr_x = 0;
  const fcg::DeviceMesh& m = h->ctx->mesh;
  const Step& st0 = h->steps[0];
  const int64_t nb0 = h->nb0;
  ck(fcg_bsr_from_node_csr(h->device, nb0, m.rowptr, c->Afull.ptr, K, c->Afull.vals, s), "fcg_bsr_from_node_csr (full rows)");
  // lambda_max of the global D^-1 A (Lanczos over the ranks): the smoother's and P's
  estimate_lmax(Ops{h, 0, K, s, tr});
  ck(fcg_bsr_spgemm(h->device, 3, 3, 6, nb0, c->Afull.ptr, c->Afull.col, c->Afull.vals, c->Text.ptr,
         c->Text.col, c->Text.vals, c->AT.ptr, c->AT.col, c->AT.vals, s), "fcg_bsr_spgemm (A T_ext)");
  ck(fcg_amg_smooth_prolongator(h->device, 3, nb0, c->P.ptr, c->P.col, c->agg, st0.tent, h->A0_dinv,
         c->AT.vals, h->opt.omega / c->lmax0, c->P.vals, s), "fcg_amg_smooth_prolongator (global)");
  ck(fcg_bsr_transpose_values(h->device, 3, 6, c->P.nnzb, c->p_perm, c->P.vals, c->Pt.vals, s),
      "fcg_bsr_transpose_values");
  extend_values(h, c, c->P, c->Pext, c->M, tr, s);
  ck(fcg_bsr_spgemm(h->device, 3, 3, 6, nb0, c->Afull.ptr, c->Afull.col, c->Afull.vals, c->Pext.ptr,
         c->Pext.col, c->Pext.vals, c->AP.ptr, c->AP.col, c->AP.vals, s), "fcg_bsr_spgemm (A P_ext)");
  ck(fcg_bsr_spgemm(h->device, 6, 3, 6, c->Pt.n, c->Pt.ptr, c->Pt.col, c->Pt.vals, c->AP.ptr, c->AP.col,
         c->AP.vals, c->C.ptr, c->C.col, c->C.vals, s), "fcg_bsr_spgemm (P^T A P)");
  if (c->d) dist_setup(h, c->d, c->C, tr, s);
  // the replicated operator: every rank's blocks scattered into a zeroed buffer, summed
  fcg_amg* g = c->g;
  Level& L1 = g->levels[0];
  ck(hipMemsetAsync(L1.A.vals, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(1, c->rep_nnzb)) * 36, s), "memset");
  if (c->rep_part->nnzb > 0)
    hipLaunchKernelGGL(scatter_blocks_kernel, dim3(blocks_for(c->rep_part->nnzb * 36)), dim3(kBlock), 0, s,
        c->rep_part->nnzb, c->rep_pos, c->rep_part->vals, L1.A.vals);
  ck(hipGetLastError(), "scatter_blocks_kernel");
  allreduce_counted(c, tr, L1.A.vals, c->rep_nnzb * 36, s, c->d ? "transport all-reduce (replicated coarse level)" : "transport all-reduce (A_1)");
  ck(fcg_bsr_block_jacobi_setup(g->device, 6, L1.A.n, L1.A.ptr, L1.diag, L1.A.vals, L1.dinv, g->flag, s),
      c->d ? "coupled AMG replicated level: singular diagonal block" : "coupled AMG level 1: singular diagonal block");
  if (g->steps.size() > 1) estimate_lmax(Ops{g, 1, nullptr, s});
  galerkin_from(g, 1, nullptr, s);
  c->ar_setup = c->ctr_ar;
  c->x_setup = c->ctr_x;
}

// Q x = P A_1^-1 P^T x over all ranks.  Replicated level 1: this rank's rows restricted into the
// global level-1 vector (every rank adds to the aggregates its rows reach), the all-reduce, the
// replicated hierarchy's V-cycle, prolongation into this rank's rows (overwrites y).  Distributed
// level 1: the restriction over LA, whose other-rank entries go to their owners and are added
// there (senders in rank order), the level-1 V-cycle, and the reverse exchange before P.
void coupled_coarse(fcg_amg* h, const fcg_transport* tr, const double* x, double* y, hipStream_t s)
{
  Coupled* c = h->cpl;
  Dist* d = c->d;
  if (!d)
  {
    ck(fcg_bsr_spmv(h->device, 6, 3, c->Pt.n, c->Pt.ptr, c->Pt.col, c->Pt.vals, x, c->gb, 1.0, 0, s), "restriction");
    allreduce_counted(c, tr, c->gb, 6 * c->n_agg_tot, s, "transport all-reduce (level 1)");
    vcycle(c->g, 1, nullptr, c->gb, c->ge, s);
    ck(fcg_bsr_spmv(h->device, 3, 6, c->P.n, c->P.ptr, c->P.col, c->P.vals, c->ge, y, 1.0, 0, s), "prolongation");
    return;
  }
  dist_coarse(h, tr, d, 3, c->Pt, c->P, x, y, 0, s);
}

// y = A x with the global operator: the import of x into the column map, the rank's SpMV
void coupled_spmv(fcg_amg* h, const double* K, const fcg_transport* tr, const double* x, double* y, hipStream_t s)
{
  Coupled* c = h->cpl;
  ck(tr->import_fn(tr->user, x, c->chan_col, s), "transport import");
  ck(fcg_spmv(h->ctx, K, c->chan_col, y, s), "fcg_spmv");
}

// One V-cycle of the global system: Chebyshev smoothing with the global operator (D = the owned
// nodal blocks, lambda_max of the global D^-1 A), the residual restricted by this rank's P_0 into
// level 1, the coarse levels there, prolongation, Chebyshev again -- the single-rank cycle, with
// P_0 from the rank-local aggregation.  (Tried before: a multiplicative cycle with rank-local
// smoothing, indefinite; the balancing form Q r + (I - Q A) M (I - A Q) r with M the rank-local
// V-cycle, 64 FCG iterations against 33 on one rank for the 2-rank test box.)
void coupled_apply(fcg_amg* h, const double* K, const fcg_transport* tr, const double* r, double* z,
    hipStream_t s)
{
  Coupled* c = h->cpl;
  c->ctr_ar = c->ctr_x = 0;
  const int64_t n = h->n0;
  const Ops o{h, 0, K, s, tr};
  cheb(h, o, r, z, true);
  coupled_spmv(h, K, tr, z, c->q, s);
  rsub(r, c->q, n, s);
  coupled_coarse(h, tr, c->q, c->w, s);
  axpby(1.0, c->w, 1.0, z, n, s);
  cheb(h, o, r, z, false);
  c->ar_apply = c->ctr_ar;
  c->x_apply = c->ctr_x;
}

// bytes of a hierarchy's matrices (fcg_amg_coupled_stats)
int64_t hierarchy_bytes(const fcg_amg* g)
{
  int64_t b = 0;
  for (const Level& L : g->levels) b += L.A.nnzb * 36 * 8;
  for (const Step& st : g->steps)
    for (const Bsr* M : {&st.T, &st.P, &st.AT, &st.AP, &st.Pt}) b += M->nnzb * M->br * M->bc * 8;
  b += g->cn * g->cn * 8;
  return b;
}

// all-reduced status: true when some rank reported a failure
bool guard_checkpoint(Guard* g, double mine)
{
  if (!g->h->agree) g->h->agree = dalloc<double>(g->h, 2);
  const double v[2] = {mine, 0.0};
  double out[2] = {0.0, 0.0};
  ck(hipMemcpyAsync(g->h->agree, v, sizeof(v), hipMemcpyHostToDevice, g->s), "hipMemcpyAsync");
  ck(g->in->allreduce_fn(g->in->user, g->h->agree, 2, g->s), "transport all-reduce (status)");
  ck(hipMemcpyAsync(out, g->h->agree, sizeof(out), hipMemcpyDeviceToHost, g->s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(g->s), "hipStreamSynchronize");
  ++g->checkpoints;
  return out[0] > 0.0;
}

int guard_enter(Guard* g)
{
  if (g->fail_at >= 0 && g->checkpoints >= g->fail_at)
  {
    g->fail_at = -1;
    throw Fail{FCG_ERR_ARG, "coupled AMG: injected failure inside the build (FCG_AMG_INJECT_BUILD_FAIL)"};
  }
  if (!guard_checkpoint(g, 0.0)) return FCG_OK;
  g->remote = true;
  return FCG_ERR_DEVICE;
}

int guard_allreduce(void* u, double* d, int64_t n, void* s)
{
  Guard* g = static_cast<Guard*>(u);
  const int rc = guard_enter(g);
  return rc != FCG_OK ? rc : g->in->allreduce_fn(g->in->user, d, n, s);
}

int guard_import(void* u, const double* x_row, double* x_col, void* s)
{
  Guard* g = static_cast<Guard*>(u);
  const int rc = guard_enter(g);
  return rc != FCG_OK ? rc : g->in->import_fn(g->in->user, x_row, x_col, s);
}

int guard_exchange(void* u, const double* sb, const int64_t* sc, double* rb, const int64_t* rc_, void* s)
{
  Guard* g = static_cast<Guard*>(u);
  const int rc = guard_enter(g);
  return rc != FCG_OK ? rc : g->in->exchange_fn(g->in->user, sb, sc, rb, rc_, s);
}

fcg_transport guarded(const fcg_transport* tr, Guard* g)
{
  fcg_transport t = *tr;
  t.user = g;
  t.allreduce_fn = guard_allreduce;
  t.import_fn = guard_import;
  t.exchange_fn = tr->exchange_fn ? guard_exchange : nullptr;
  return t;
}

}  // namespace fcg_amgs
