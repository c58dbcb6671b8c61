// fcg_amg_solver.hip -- the smoothed-aggregation AMG solve as a native C++ object behind the C ABI
// (fcg_amg_create / fcg_amg_solve / fcg_amg_level_info / fcg_amg_destroy): what a C++ host such as
// 4C calls in place of its Belos CG + MueLu preconditioner (4C_solver_nonlin_nox_linearsystem.cpp:
// 275-353, 4C_linear_solver_preconditioner_muelu.cpp) on the tangent a context assembled.  The
// hierarchy and cycle are those of 4c_amd/amg.py (which stays the Python-side mirror and test
// reference): graph setup on the host once (fcg_amg_setup.cpp), numeric setup per tangent and the
// flexible-CG / V-cycle / Chebyshev iteration on the device (fcg_amg.hip kernels, the context's
// fcg_spmv / block-Jacobi on level 0).  Differences from amg.py: the coarsest level is inverted
// densely on the device per tangent (Gauss-Jordan, up to kDenseMax DOFs; above that, or when a
// pivot fails, block-Jacobi CG to a loose tolerance), the scalars of every iteration stay on the
// device except one read per FCG iteration, and with the dense coarsest level one FCG iteration can
// be replayed as a captured HIP graph (FCG_AMG_GRAPH=1).
//
// This file: the host hierarchy build, the single-rank numeric setup, the Chebyshev smoother, the
// coarsest solve, the V-cycle and the flexible CG.  It reaches a transport only through Ops
// (fcg_amg_internal.hpp, with the handle's types); the coarse levels coupled across ranks are
// fcg_amg_coupled.hip, the C ABI is fcg_amg_api.hip, the kernels shared with the scalar AMG of K_TT
// fcg_amg_vec.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fcg_amg_internal.hpp"

namespace fcg_amgs {

// y = b - y
__global__ __launch_bounds__(kBlock) void rsub_kernel(const double* __restrict__ b, double* y, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) y[i] = b[i] - y[i];
}

// ---- the coarsest level as a dense inverse ------------------------------------------------------
// (4C's MueLu coarsest level is a direct solve, Amesos/KLU: 4C_linear_solver_preconditioner_muelu.cpp
// via the xml's "coarse: type"; here the coarsest level has at most coarse_max DOFs, so its inverse
// is formed densely once per tangent and applied as one matrix-vector product per V-cycle)

// D = the 6 x 6 BSR matrix as dense row-major n x n (n = 6 nb; D zeroed before): one thread per
// (block row, block entry)
__global__ __launch_bounds__(kBlock) void bsr6_dense_kernel(int64_t nb, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, double* D)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nb * 36) return;
  const int64_t i = t / 36;
  const int e = int(t - 36 * i), a = e / 6, b = e % 6;
  const int64_t n = 6 * nb;
  for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k)
    D[(6 * i + a) * n + 6 * int64_t(col[k]) + b] = vals[36 * k + e];
}

// coarse CG, scalars on the device: sc[0] = r.z, sc[1] = p.q, sc[2] = r.z new, sc[3] = r.r
__global__ __launch_bounds__(kBlock) void cg_step_kernel(const double* __restrict__ sc,
    const double* __restrict__ p, const double* __restrict__ q, double* x, double* r, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double alpha = sc[1] > 0.0 ? sc[0] / sc[1] : 0.0;
  x[i] += alpha * p[i];
  r[i] -= alpha * q[i];
}
__global__ __launch_bounds__(kBlock) void cg_dir_kernel(const double* __restrict__ sc,
    const double* __restrict__ z, double* p, int64_t n)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double beta = sc[0] != 0.0 ? sc[2] / sc[0] : 0.0;
  p[i] = z[i] + beta * p[i];
}

// deterministic pseudo-random vector in [-0.5, 0.5) times mask (Lanczos start)
__global__ __launch_bounds__(kBlock) void random_kernel(double* v, const double* __restrict__ mask,
    int64_t n, uint32_t seed)
{
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t h = uint64_t(i) * 0x9E3779B97F4A7C15ull + seed;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  const double u = double(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
  v[i] = mask ? u * mask[i] : u;
}

// the context's node-triple K into the reordered BSR copy: block m of level-0 row p is triple
// old_k of context row new2old[p] (16 lanes per row, as node_csr_to_bsr_kernel)
__global__ __launch_bounds__(kBlock) void perm_csr_to_bsr_kernel(int64_t n, const int64_t* __restrict__ rowptr,
    const int64_t* __restrict__ b_ptr, const int32_t* __restrict__ new2old, const int32_t* __restrict__ old_k,
    const double* __restrict__ K, double* b_vals)
{
  const int64_t p = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  if (p >= n) return;
  const int64_t r = new2old[p];
  const int64_t r0 = rowptr[3 * r], r1 = rowptr[3 * r + 1], r2 = rowptr[3 * r + 2];
  for (int64_t q = b_ptr[p] + lane; q < b_ptr[p + 1]; q += 16)
  {
    const int64_t k3 = 3 * int64_t(old_k[q]);
    double* o = b_vals + q * 9;
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
      o[c] = K[r0 + k3 + c];
      o[3 + c] = K[r1 + k3 + c];
      o[6 + c] = K[r2 + k3 + c];
    }
  }
}

// node triples between the context's order and level 0's: gather dst[3p + d] = src[3 new2old[p] + d]
// (to_ctx = 0) or scatter dst[3 new2old[p] + d] = src[3p + d] (to_ctx = 1)
__global__ __launch_bounds__(kBlock) void node_perm_kernel(int64_t nb, const int32_t* __restrict__ new2old,
    const double* __restrict__ src, double* __restrict__ dst, int to_ctx)
{
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= 3 * nb) return;
  const int64_t p = t / 3, d = t - 3 * p;
  const int64_t o = 3 * int64_t(new2old[p]) + d;
  if (to_ctx) dst[o] = src[t];
  else dst[t] = src[o];
}

void make_bsr(fcg_amg* h, Bsr& M, std::vector<int64_t> ptr, std::vector<int32_t> col, int br, int bc,
    int64_t n_cols)
{
  M.n = int64_t(ptr.size()) - 1;
  M.nnzb = ptr.back();
  M.br = br;
  M.bc = bc;
  M.n_cols = n_cols;
  M.ptr_h = std::move(ptr);
  M.col_h = std::move(col);
  M.ptr = upload(h, M.ptr_h);
  M.col = upload(h, M.col_h);
  M.vals = dalloc<double>(h, M.nnzb * br * bc);
  ck(hipMemset(M.vals, 0, sizeof(double) * size_t(std::max<int64_t>(M.nnzb * br * bc, 1))), "hipMemset");
}

void symbolic(const Bsr& A, const std::vector<int64_t>& bp, const std::vector<int32_t>& bc_,
    int64_t n_cols, std::vector<int64_t>& cp, std::vector<int32_t>& cc)
{
  cp.assign(size_t(A.n) + 1, 0);
  const int64_t nnz = fcg_bsr_symbolic(A.n, A.ptr_h.data(), A.col_h.data(), bp.data(), bc_.data(),
      n_cols, cp.data(), nullptr);
  if (nnz < 0) throw Fail{FCG_ERR_ARG, "AMG: symbolic product failed"};
  cc.assign(size_t(std::max<int64_t>(nnz, 1)), 0);
  if (fcg_bsr_symbolic(A.n, A.ptr_h.data(), A.col_h.data(), bp.data(), bc_.data(), n_cols, cp.data(),
          cc.data()) != nnz)
    throw Fail{FCG_ERR_ARG, "AMG: symbolic fill pass"};
  cc.resize(size_t(nnz));
}

std::vector<int64_t> diag_index(const Bsr& A)
{
  std::vector<int64_t> d(size_t(A.n), -1);
  for (int64_t i = 0; i < A.n; ++i)
    for (int64_t k = A.ptr_h[size_t(i)]; k < A.ptr_h[size_t(i) + 1]; ++k)
      if (A.col_h[size_t(k)] == i) d[size_t(i)] = k;
  for (int64_t v : d)
    if (v < 0) throw Fail{FCG_ERR_ARG, "AMG: block row without a diagonal block"};
  return d;
}

bool env_off(const char* name)
{
  const char* v = std::getenv(name);
  return v && std::strcmp(v, "0") == 0;
}

// the pairs of C = X Y on C's pattern, listed on the host and uploaded (the numeric SpGEMM per
// tangent then streams them instead of searching Y's rows for every C block)
Plan make_plan(fcg_amg* h, const Bsr& X, const Bsr& Y, const Bsr& C, const std::vector<int32_t>* agg = nullptr)
{
  Plan pl;
  if (agg)
  {
    // rows of one aggregate are neighbours: forming their blocks together re-reads the Y rows of
    // their shared neighbours from cache (on a renumbered mesh storage order scatters them)
    std::vector<int64_t> rows(size_t(C.n));
    for (int64_t i = 0; i < C.n; ++i) rows[size_t(i)] = i;
    std::stable_sort(rows.begin(), rows.end(), [&](int64_t p, int64_t q) {
      return (*agg)[size_t(p)] < (*agg)[size_t(q)];  // unaggregated rows (-1) first
    });
    std::vector<int64_t> ord;
    ord.reserve(size_t(C.nnzb));
    for (int64_t i : rows)
      for (int64_t ci = C.ptr_h[size_t(i)]; ci < C.ptr_h[size_t(i) + 1]; ++ci) ord.push_back(ci);
    pl.order = upload(h, ord);
  }
  std::vector<int64_t> ptr(size_t(C.nnzb) + 1, 0);
  const int64_t np = fcg_bsr_product_plan(X.n, X.ptr_h.data(), X.col_h.data(), Y.ptr_h.data(),
      Y.col_h.data(), C.ptr_h.data(), C.col_h.data(), C.n_cols, ptr.data(), nullptr, nullptr);
  if (np < 0) throw Fail{FCG_ERR_ARG, "AMG: product plan (count)"};
  std::vector<int32_t> a(size_t(std::max<int64_t>(np, 1))), b(size_t(std::max<int64_t>(np, 1)));
  if (fcg_bsr_product_plan(X.n, X.ptr_h.data(), X.col_h.data(), Y.ptr_h.data(), Y.col_h.data(),
          C.ptr_h.data(), C.col_h.data(), C.n_cols, ptr.data(), a.data(), b.data()) != np)
    throw Fail{FCG_ERR_ARG, "AMG: product plan (fill)"};
  pl.ptr = upload(h, ptr);
  pl.a = upload(h, a);
  pl.b = upload(h, b);
  return pl;
}

// aggregation hierarchy below A_start (block size bs, near-null space ns [n][bs][6]; skip: level-0
// nodes left out of the aggregation, NULL on a coarse start): appends steps and coarse levels until
// a level has at most coarse_max DOFs (and always one step from an empty hierarchy)
void coarsen(fcg_amg* h, const Bsr* A_start, int bs, std::vector<double> ns, const uint8_t* skip)
{
  const Bsr* A = A_start;
  bool first = skip != nullptr;
  while ((A->n * bs > h->opt.coarse_max || h->steps.empty()) && int(h->steps.size()) + 1 < h->opt.max_levels)
  {
    std::vector<int32_t> agg(size_t(A->n));
    const int64_t n_agg = fcg_amg_aggregate(A->n, A->ptr_h.data(), A->col_h.data(), first ? skip : nullptr, agg.data());
    if (n_agg <= 0 || n_agg >= A->n) break;
    std::vector<double> tent(size_t(A->n) * bs * 6), nsc(size_t(n_agg) * 36);
    int64_t nd = 0;
    ck(fcg_amg_tentative(A->n, bs, ns.data(), agg.data(), n_agg, tent.data(), nsc.data(), &nd), "fcg_amg_tentative");
    h->steps.emplace_back();
    Step& st = h->steps.back();
    st.bs = bs;
    st.n_agg = n_agg;
    std::vector<int64_t> tptr(size_t(A->n) + 1, 0);
    std::vector<int32_t> tcol;
    std::vector<double> tvals;
    for (int64_t i = 0; i < A->n; ++i)
    {
      tptr[size_t(i) + 1] = tptr[size_t(i)] + (agg[size_t(i)] >= 0 ? 1 : 0);
      if (agg[size_t(i)] >= 0)
      {
        tcol.push_back(agg[size_t(i)]);
        tvals.insert(tvals.end(), tent.begin() + i * bs * 6, tent.begin() + (i + 1) * bs * 6);
      }
    }
    make_bsr(h, st.T, tptr, tcol, bs, 6, n_agg);
    if (!tvals.empty())
      ck(hipMemcpy(st.T.vals, tvals.data(), sizeof(double) * tvals.size(), hipMemcpyHostToDevice), "hipMemcpy");
    st.agg = upload(h, agg);
    st.tent = upload(h, tent);
    std::vector<int64_t> pp, app, tp, cp;
    std::vector<int32_t> pc, apc, tc, cc;
    symbolic(*A, st.T.ptr_h, st.T.col_h, n_agg, pp, pc);
    make_bsr(h, st.P, pp, pc, bs, 6, n_agg);
    make_bsr(h, st.AT, pp, pc, bs, 6, n_agg);
    symbolic(*A, pp, pc, n_agg, app, apc);
    make_bsr(h, st.AP, app, apc, bs, 6, n_agg);
    tp.assign(size_t(n_agg) + 1, 0);
    tc.assign(size_t(std::max<int64_t>(pp.back(), 1)), 0);
    std::vector<int64_t> perm(size_t(std::max<int64_t>(pp.back(), 1)));
    ck(fcg_bsr_transpose_pattern(A->n, n_agg, pp.data(), pc.data(), tp.data(), tc.data(), perm.data()), "fcg_bsr_transpose_pattern");
    tc.resize(size_t(pp.back()));
    perm.resize(size_t(pp.back()));
    make_bsr(h, st.Pt, tp, tc, 6, bs, A->n);
    st.perm = upload(h, perm);
    symbolic(st.Pt, app, apc, n_agg, cp, cc);
    const bool plans = !env_off("FCG_AMG_PLAN");
    if (plans)  // (before the level list grows: A may point into it)
    {
      const bool by_agg = !env_off("FCG_AMG_PLAN_ORDER");
      st.pAT = make_plan(h, *A, st.T, st.AT, by_agg ? &agg : nullptr);
      st.pAP = make_plan(h, *A, st.P, st.AP, by_agg ? &agg : nullptr);
    }
    h->levels.emplace_back();
    Level& c = h->levels.back();
    make_bsr(h, c.A, cp, cc, 6, 6, n_agg);
    if (plans) st.pC = make_plan(h, st.Pt, st.AP, c.A);
    c.diag = upload(h, diag_index(c.A));
    c.dinv = dalloc<double>(h, 36 * n_agg);
    for (double** v : {&c.x, &c.b, &c.r, &c.d, &c.z, &c.p, &c.q}) *v = dalloc<double>(h, 6 * n_agg);
    if (first) h->ns1 = nsc;  // level 1's near-null space (the coupled coarse level gathers it)
    ns.swap(nsc);
    A = &c.A;
    bs = 6;
    first = false;
  }
}

// ---- device helpers --------------------------------------------------------------------------
void rsub(const double* b, double* y, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(rsub_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, b, y, n);
}

void node_perm(fcg_amg* h, const double* src, double* dst, int to_ctx, hipStream_t s)
{
  hipLaunchKernelGGL(node_perm_kernel, dim3(blocks_for(h->n0)), dim3(kBlock), 0, s, h->nb0, h->new2old, src,
      dst, to_ctx);
}

void dot_dev(fcg_amg* h, const double* a, const double* b, int64_t n, double* out, hipStream_t s)
{
  dot(a, b, n, h->partial, out, s);
}
double dot_host(fcg_amg* h, const double* a, const double* b, int64_t n, hipStream_t s)
{
  return dot_host(a, b, n, h->partial, h->sc + 6, s, [](hipError_t e, const char* what) { ck(e, what); });
}

void apply_A0(fcg_amg* h, const double* K, const double* x, double* y, hipStream_t s)
{
  if (h->local || h->new2old)
    ck(fcg_bsr_spmv(h->device, 3, 3, h->A0.n, h->A0.ptr, h->A0.col, h->A0.vals, x, y, 1.0, 0, s),
        "fcg_bsr_spmv (level 0)");
  else
    ck(fcg_spmv(h->ctx, K, x, y, s), "fcg_spmv");
}

// largest eigenvalue of D^-1 A from a 10-step Lanczos (block-Jacobi CG on a random vector); with
// o.tr the operator is the global one and the inner products are summed over the ranks
void estimate_lmax(const Ops& o)
{
  fcg_amg* h = o.h;
  const int64_t n = o.n();
  double *b = o.d(), *r = o.r(), *z = o.z(), *p = o.p(), *q = o.q();
  auto dot_ranks = [&](const double* x, const double* y) {
    if (!o.tr) return dot_host(h, x, y, n, o.s);
    dot_dev(h, x, y, n, h->sc + 6, o.s);
    ck(o.tr->allreduce_fn(o.tr->user, h->sc + 6, 1, o.s), "transport all-reduce (Lanczos)");
    double v = 0.0;
    ck(hipMemcpyAsync(&v, h->sc + 6, sizeof(double), hipMemcpyDeviceToHost, o.s), "hipMemcpyAsync");
    ck(hipStreamSynchronize(o.s), "hipStreamSynchronize");
    return v;
  };
  hipLaunchKernelGGL(random_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, o.s, b,
      o.l == 0 && !o.dl ? h->mask0 : nullptr, n, 20251015u);
  ck(hipMemcpyAsync(r, b, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, o.s), "copy");
  o.dinv(r, z, 1.0, false);
  ck(hipMemcpyAsync(p, z, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, o.s), "copy");
  const LanczosSteps t = lanczos_steps([&](const double* x, double* y) { o.spmv(x, y); },
      [&](const double* x, double* y) { o.dinv(x, y, 1.0, false); }, dot_ranks, r, z, p, q, n, o.s);
  if (t.al.empty()) throw Fail{FCG_ERR_SINGULAR, "AMG Lanczos estimate: p.Ap <= 0"};
  o.lmax() = lanczos_lmax(t.al, t.be);
}

void cheb(const fcg_amg* hc, const Ops& o, const double* b, double* x, bool x_zero)
{
  const fcg_amg_options& op = hc->opt;
  const int64_t n = o.n();
  ChebCoef c(o.lmax(), op.boost, op.ratio);
  double *r = o.r(), *d = o.d();
  if (x_zero)
  {
    o.dinv(b, d, c.first(), false);
    ck(hipMemcpyAsync(x, d, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, o.s), "copy");
  }
  else
  {
    o.spmv(x, r);
    rsub(b, r, n, o.s);
    o.dinv(r, d, c.first(), false);
    axpby(1.0, d, 1.0, x, n, o.s);
  }
  for (int k = 1; k < op.nu; ++k)
  {
    o.spmv(x, r);
    rsub(b, r, n, o.s);
    const ChebCoef::Degree g = c.next();
    axpby(0.0, d, g.c_d, d, n, o.s);
    o.dinv(r, d, g.c_r, true);
    axpby(1.0, d, 1.0, x, n, o.s);
  }
}

// coarsest level: block-Jacobi CG from x = 0 to |r| <= coarse_rtol |b| (checked every 8 steps;
// scalars on the device in between)
void coarse_solve(fcg_amg* h, const Ops& o, const double* b, double* x)
{
  const int64_t n = o.n();
  if (h->cinv && h->cn == n)
  {
    dense_mv(h->cinv, b, x, n, o.s);
    ck(hipGetLastError(), "dense_mv_kernel");
    return;
  }
  double *r = o.r(), *z = o.z(), *p = o.p(), *q = o.q();
  // its own scalars (the outer FCG keeps r.r in sc[3] across the V-cycle): 0 r.z, 1 p.q,
  // 2 r.z new, 3 r.r, 4 b.b
  double* sc = h->sc + 8;
  const dim3 g(blocks_for(n)), bl(kBlock);
  ck(hipMemsetAsync(x, 0, sizeof(double) * size_t(n), o.s), "memset");
  ck(hipMemcpyAsync(r, b, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, o.s), "copy");
  o.dinv(r, z, 1.0, false);
  ck(hipMemcpyAsync(p, z, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, o.s), "copy");
  dot_dev(h, r, z, n, sc + 0, o.s);
  dot_dev(h, b, b, n, sc + 4, o.s);
  const double tol2 = h->opt.coarse_rtol * h->opt.coarse_rtol;
  for (int it = 0; it < h->opt.coarse_max_iter;)
  {
    for (int k = 0; k < 8 && it < h->opt.coarse_max_iter; ++k, ++it)
    {
      o.spmv(p, q);
      dot_dev(h, p, q, n, sc + 1, o.s);
      hipLaunchKernelGGL(cg_step_kernel, g, bl, 0, o.s, sc, p, q, x, r, n);
      o.dinv(r, z, 1.0, false);
      dot_dev(h, r, z, n, sc + 2, o.s);
      hipLaunchKernelGGL(cg_dir_kernel, g, bl, 0, o.s, sc, z, p, n);
      fcg_shift(sc, o.s);
    }
    dot_dev(h, r, r, n, sc + 3, o.s);
    double hs[5];
    ck(hipMemcpyAsync(hs, sc, sizeof(hs), hipMemcpyDeviceToHost, o.s), "hipMemcpyAsync");
    ck(hipStreamSynchronize(o.s), "hipStreamSynchronize");
    if (!std::isfinite(hs[3])) throw Fail{FCG_ERR_SINGULAR, "AMG coarsest CG: non-finite residual"};
    if (hs[3] <= tol2 * hs[4]) break;
  }
}

void vcycle(fcg_amg* h, int l, const double* K, const double* b, double* x, hipStream_t s)
{
  const Ops o{h, l, K, s};
  if (l == int(h->levels.size()))
  {
    coarse_solve(h, o, b, x);
    return;
  }
  cheb(h, o, b, x, true);
  double* r = o.r();
  o.spmv(x, r);
  rsub(b, r, o.n(), s);
  const Step& st = h->steps[size_t(l)];
  Level& c = h->levels[size_t(l)];
  ck(fcg_bsr_spmv(h->device, 6, st.bs, st.Pt.n, st.Pt.ptr, st.Pt.col, st.Pt.vals, r, c.b, 1.0, 0, s),
      "restriction");
  vcycle(h, l + 1, K, c.b, c.x, s);
  ck(fcg_bsr_spmv(h->device, st.bs, 6, st.P.n, st.P.ptr, st.P.col, st.P.vals, c.x, x, 1.0, 1, s),
      "prolongation");
  cheb(h, o, b, x, false);
}

// the coarsest level's dense inverse (h->cinv), or none (the CG coarse solve) when the level is
// larger than kDenseMax DOFs, FCG_AMG_DENSE=0 or a pivot is not positive
void coarse_factor(fcg_amg* h, hipStream_t s)
{
  h->cinv = nullptr;
  if (h->levels.empty() || env_off("FCG_AMG_DENSE")) return;
  const Bsr& A = h->levels.back().A;
  const int64_t n = 6 * A.n;
  if (n == 0 || n > kDenseMax) return;
  if (h->cn != n)
  {
    h->cbuf[0] = dalloc<double>(h, n * n);
    h->cbuf[1] = dalloc<double>(h, n * n);
    h->cwork = dalloc<double>(h, dense_inverse_work(n));
    h->cn = n;
  }
  ck(hipMemsetAsync(h->cbuf[0], 0, sizeof(double) * size_t(n * n), s), "memset");
  ck(hipMemsetAsync(h->flag, 0, sizeof(int32_t), s), "memset");
  hipLaunchKernelGGL(bsr6_dense_kernel, dim3(blocks_for(A.n * 36)), dim3(kBlock), 0, s, A.n, A.ptr, A.col,
      A.vals, h->cbuf[0]);
  const int inv = dense_inverse(h->cbuf, h->cwork, n, h->flag, s);
  ck(hipGetLastError(), "gj_update_kernel");
  int32_t bad = 0;
  ck(hipMemcpyAsync(&bad, h->flag, sizeof(bad), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  if (!bad) h->cinv = h->cbuf[inv];
}

// the Galerkin hierarchy below level l0 (its operator and block inverses already set): per step
// l >= l0, P_l = (I - omega D^-1 A_l) T_l and A_{l+1} = P_l^T (A_l P_l) on the fixed patterns
void galerkin_from(fcg_amg* h, size_t l0, const double* K, hipStream_t s)
{
  const Bsr* A = l0 == 0 ? &h->A0 : &h->levels[l0 - 1].A;
  const double* dinv = l0 == 0 ? h->A0_dinv : h->levels[l0 - 1].dinv;
  for (size_t l = l0; l < h->steps.size(); ++l)
  {
    Step& st = h->steps[l];
    const double lm = l == 0 ? h->lmax0 : h->levels[l - 1].lmax;
    auto product = [&](Bsr& C, const Bsr& X, const Bsr& Y, const Plan& pl) {
      if (pl.ptr)
        ck(fcg_bsr_spgemm_planned(h->device, X.br, X.bc, Y.bc, C.nnzb, pl.ptr, pl.a, pl.b, X.vals,
               Y.vals, C.vals, pl.order, s),
            "fcg_bsr_spgemm_planned");
      else
        ck(fcg_bsr_spgemm(h->device, X.br, X.bc, Y.bc, X.n, X.ptr, X.col, X.vals, Y.ptr, Y.col, Y.vals,
               C.ptr, C.col, C.vals, s),
            "fcg_bsr_spgemm");
    };
    product(st.AT, *A, st.T, st.pAT);
    ck(fcg_amg_smooth_prolongator(h->device, st.bs, A->n, st.P.ptr, st.P.col, st.agg, st.tent, dinv,
           st.AT.vals, h->opt.omega / lm, st.P.vals, s),
        "fcg_amg_smooth_prolongator");
    product(st.AP, *A, st.P, st.pAP);
    ck(fcg_bsr_transpose_values(h->device, st.bs, 6, st.P.nnzb, st.perm, st.P.vals, st.Pt.vals, s),
        "fcg_bsr_transpose_values");
    Level& c = h->levels[l];
    product(c.A, st.Pt, st.AP, st.pC);
    ck(fcg_bsr_block_jacobi_setup(h->device, 6, c.A.n, c.A.ptr, c.diag, c.A.vals, c.dinv, h->flag, s),
        "AMG coarse level: singular diagonal block");
    if (l + 1 < h->steps.size()) estimate_lmax(Ops{h, int(l) + 1, K, s});
    A = &c.A;
    dinv = c.dinv;
  }
  coarse_factor(h, s);
}

// numeric setup for the tangent K (level-0 values in the context's CSR order)
void setup(fcg_amg* h, const double* K, hipStream_t s)
{
  if (h->new2old)
  {
    // the context's nodal blocks first, for their singularity check (4C's block Jacobi throws on a
    // singular block; the BSR setup below completes empty rows with a unit diagonal instead)
    ck(fcg_block_jacobi_setup(h->ctx, K, h->ctx_dinv, s), "singular nodal block of K (block Jacobi)");
    // reordered level 0: the BSR copy in level 0's order, its block inverses (the smoother's too)
    hipLaunchKernelGGL(perm_csr_to_bsr_kernel, dim3(blocks_for(h->nb0 * 16)), dim3(kBlock), 0, s, h->nb0,
        h->ctx->mesh.rowptr, h->A0.ptr, h->new2old, h->old_k, K, h->A0.vals);
    ck(hipGetLastError(), "perm_csr_to_bsr_kernel");
    ck(fcg_bsr_block_jacobi_setup(h->device, 3, h->nb0, h->A0.ptr, h->A0_diag, h->A0.vals, h->A0_dinv,
           h->flag, s),
        "singular nodal block of K");
    estimate_lmax(Ops{h, 0, K, s});
    galerkin_from(h, 0, K, s);
    return;
  }
  ck(fcg_block_jacobi_setup(h->ctx, K, h->ctx_dinv, s), "singular nodal block of K (block Jacobi)");
  // the BSR copy first: the local level 0 applies it in the lambda_max estimate
  ck(fcg_bsr_from_node_csr(h->device, h->nb0, h->ctx->mesh.rowptr, h->A0.ptr, K, h->A0.vals, s),
      "fcg_bsr_from_node_csr");
  estimate_lmax(Ops{h, 0, K, s});
  ck(fcg_bsr_block_jacobi_setup(h->device, 3, h->nb0, h->A0.ptr, h->A0_diag, h->A0.vals, h->A0_dinv,
         h->flag, s),
      "singular nodal block of K");
  galerkin_from(h, 0, K, s);
}

// The numeric setup a rank-local handle needs when its coarse levels are coupled across ranks
// (fcg_amg_precond_setup): the nodal block inverses of the smoother and of P_0's smoothing only --
// the coupled path builds its own lambda_max, P_0, A_1 and hierarchy, so the rank-local Galerkin
// products, their Lanczos estimates and the dense coarsest inverse are skipped
void setup_coupled_local(fcg_amg* h, const double* K, hipStream_t s)
{
  ck(fcg_block_jacobi_setup(h->ctx, K, h->ctx_dinv, s), "singular nodal block of K (block Jacobi)");
  ck(fcg_bsr_from_node_csr(h->device, h->nb0, h->ctx->mesh.rowptr, h->A0.ptr, K, h->A0.vals, s),
      "fcg_bsr_from_node_csr");
  ck(fcg_bsr_block_jacobi_setup(h->device, 3, h->nb0, h->A0.ptr, h->A0_diag, h->A0.vals, h->A0_dinv,
         h->flag, s),
      "singular nodal block of K");
}

// flexible CG (Polak-Ribiere) preconditioned by one V-cycle; one host read per iteration
void run_fcg_ordered(fcg_amg* h, const double* K, const double* b, double* x, double rtol, int max_iter,
    int* iterations, double* rel, hipStream_t s)
{
  const int64_t n = h->n0;
  // FCG vectors (the V-cycle's level-0 work vectors r0 / d0 are separate)
  double *r = h->fr, *z = h->fz, *pp = h->fx, *q = h->q0, *ro = h->ro0;
  double* sc = h->sc;
  // device scalars: 0 r.z, 1 p.q, 2 r.z new, 3 r.r, 5 z.r_old
  auto body = [&](hipStream_t q_s) {
    apply_A0(h, K, pp, q, q_s);
    dot_dev(h, pp, q, n, sc + 1, q_s);
    fcg_step(sc, pp, q, x, r, ro, n, q_s);
    dot_dev(h, r, r, n, sc + 3, q_s);
    vcycle(h, 0, K, r, z, q_s);
    dot_dev(h, r, z, n, sc + 2, q_s);
    dot_dev(h, z, ro, n, sc + 5, q_s);
  };
  // the graph (the iteration body has no host synchronisation once the coarsest solve is dense):
  // its kernel arguments bake in K, x and the setup's lambda_max values
  const char* ge = std::getenv("FCG_AMG_GRAPH");
  const bool use_graph = !h->graph_off && h->cinv && ge && std::strcmp(ge, "1") == 0;
  hipStream_t w = s;
  if (use_graph)
  {
    if (!h->gs)
    {
      ck(hipStreamCreateWithFlags(&h->gs, hipStreamNonBlocking), "hipStreamCreateWithFlags");
      ck(hipEventCreateWithFlags(&h->gev[0], hipEventDisableTiming), "hipEventCreate");
      ck(hipEventCreateWithFlags(&h->gev[1], hipEventDisableTiming), "hipEventCreate");
    }
    ck(hipEventRecord(h->gev[0], s), "hipEventRecord");
    ck(hipStreamWaitEvent(h->gs, h->gev[0], 0), "hipStreamWaitEvent");
    w = h->gs;
    if (h->gexec && (h->g_K != K || h->g_x != x))
    {
      (void)hipGraphExecDestroy(h->gexec);
      h->gexec = nullptr;
    }
  }
  // the caller's stream waits for the private one on every exit
  struct Join {
    fcg_amg* h;
    hipStream_t s, w;
    ~Join()
    {
      if (w != s && hipEventRecord(h->gev[1], w) == hipSuccess) (void)hipStreamWaitEvent(s, h->gev[1], 0);
    }
  } join{h, s, w};
  ck(hipMemsetAsync(x, 0, sizeof(double) * size_t(n), w), "memset");
  const double bn = std::sqrt(dot_host(h, b, b, n, w));
  *iterations = 0;
  *rel = 0.0;
  if (bn == 0.0) return;
  ck(hipMemcpyAsync(r, b, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, w), "copy");
  vcycle(h, 0, K, r, z, w);
  ck(hipMemcpyAsync(pp, z, sizeof(double) * size_t(n), hipMemcpyDeviceToDevice, w), "copy");
  dot_dev(h, r, z, n, sc + 0, w);
  double rz = 0.0;
  ck(hipMemcpyAsync(&rz, sc, sizeof(double), hipMemcpyDeviceToHost, w), "hipMemcpyAsync");
  ck(hipStreamSynchronize(w), "hipStreamSynchronize");
  if (!(rz > 0.0)) throw Fail{FCG_ERR_SINGULAR, "AMG: indefinite V-cycle (r.z <= 0)"};
  double rn = bn;
  int it = 0;
  while (it < max_iter)
  {
    ++it;
    if (use_graph && !h->gexec && !h->graph_off)
    {
      hipGraph_t graph = nullptr;
      bool ok = hipStreamBeginCapture(w, hipStreamCaptureModeRelaxed) == hipSuccess;
      if (ok)
      {
        try
        {
          body(w);
        }
        catch (const Fail&)
        {
          ok = false;
        }
        ok = hipStreamEndCapture(w, &graph) == hipSuccess && ok && graph;
        ok = ok && hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
      }
      if (!ok)
      {
        (void)hipGetLastError();
        if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
        h->gexec = nullptr;
        h->graph_off = true;  // eager from here on
      }
      h->g_K = K;
      h->g_x = x;
    }
    if (h->gexec)
    {
      ck(hipGraphLaunch(h->gexec, w), "hipGraphLaunch");
      ++h->graph_launches;
    }
    else
      body(w);
    double hs[6];
    ck(hipMemcpyAsync(hs, sc, sizeof(hs), hipMemcpyDeviceToHost, w), "hipMemcpyAsync");
    ck(hipStreamSynchronize(w), "hipStreamSynchronize");
    rn = std::sqrt(hs[3]);
    if (!std::isfinite(rn)) throw Fail{FCG_ERR_SINGULAR, "AMG FCG: non-finite residual"};
    if (rn <= rtol * bn) break;
    if (!(hs[2] > 0.0)) throw Fail{FCG_ERR_SINGULAR, "AMG: indefinite V-cycle (r.z <= 0)"};
    fcg_dir(sc, z, pp, n, w);
    fcg_shift(sc, w);
  }
  *iterations = it;
  *rel = rn / bn;
}

// level 0 reordered: the iteration runs on permuted copies of b and x
void run_fcg(fcg_amg* h, const double* K, const double* b, double* x, double rtol, int max_iter,
    int* iterations, double* rel, hipStream_t s)
{
  if (!h->new2old)
  {
    run_fcg_ordered(h, K, b, x, rtol, max_iter, iterations, rel, s);
    return;
  }
  node_perm(h, b, h->pb, 0, s);
  ck(hipGetLastError(), "node_perm_kernel");
  run_fcg_ordered(h, K, h->pb, h->px, rtol, max_iter, iterations, rel, s);
  node_perm(h, h->px, x, 1, s);
  ck(hipGetLastError(), "node_perm_kernel");
}

}  // namespace fcg_amgs
