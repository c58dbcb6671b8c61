// fcg_krylov.hip -- restarted flexible GMRES on the device, the solver for the tangents that are
// not symmetric (the monolithic TSI matrix: K_ST != K_TS^T; 4C hands these to Belos GMRES,
// 4C_linear_solver_method_linalg.cpp / TSI::Monolithic::linear_solve), and its single-field front
// fcg_gmres_solve.  The TSI front is fcg_tsi_solve.hip.
//
// Algorithm (Saad, "A flexible inner-outer preconditioned GMRES algorithm", SIAM J. Sci. Comput.
// 14, 1993): from x = 0, per inner step j  z_j = P v_j,  w = A z_j,  w orthogonalised against
// v_0..v_j by classical Gram-Schmidt applied twice (CGS2: two passes of "all dot products, then
// one combined update", so the j + 1 dot products of a pass are independent and run as one
// kernel),  h_{j+1,j} = |w|,  v_{j+1} = w / h_{j+1,j};  the Hessenberg column is brought to
// triangular form by Givens rotations and |g_{j+1}| estimates the residual.  At the end of a cycle
// y solves the triangular system and x += Z y; the true residual b - A x is then recomputed: it
// starts the next cycle and is what the caller gets back.  V (m + 1 vectors) and Z (m vectors)
// are both stored: one code path for fixed and for varying preconditioners.
//
// Kernels, all FP64, every sum in a fixed order (no atomics on doubles):
//   multi_dot_kernel        h_i = v_i . w, i = 0..j: w and the basis stream through 16-byte loads
//                           in tiles of kTile = 8 basis vectors (8 accumulators per lane, w read
//                           once per tile), block partials [n_blocks][j + 1] from a capped grid
//   reduce_cols_kernel      second stage: one workgroup per column sums its partials, fixed order
//   multi_axpy_norm_kernel  w -= sum_i h_i v_i with w held in registers over all i (basis loads
//                           unrolled by kTile), block partials of |w|^2 for the new w
//   scalar_step_kernel      one workgroup: |w|^2 from its partials, then lane 0 alone applies the
//                           rotations, updates g, counts the step and sets done / bad -- the role
//                           reduce_kernel plays for fcg_pcg_solve
//   scale_kernel            v_{j+1} = w / h_{j+1,j}
// plus the front's residual (r = b - A x with a compensated product: the residual at a restart is
// 10 orders below |A||x|, and its FP64 rounding would show in the fifth digit of the norm handed
// back), resid / begin_cycle (beta = |r|, g = beta e_0), solve_y (back substitution) and update_x
// (x += Z y) once per cycle.  That is 8 dependent launches per inner step besides
// the operator and the preconditioner; at small n the step is launch-bound.
//
// The host reads the scalar block once per burst of kKrylovBurst = 8 inner steps.  Once `done` is
// set (estimate <= rtol |b|, exact breakdown h_{j+1,j} = 0, or a non-finite value) every kernel of
// the remaining steps of the burst returns at once, so nothing is divided by zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "fcg_internal.hpp"
#include "fcg_krylov.hpp"
#include "fcg_status.hpp"

namespace fcg {

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 8;  // basis vectors per register tile of multi_dot_kernel
// grid cap of the streaming kernels: 2 workgroups per CU of a 256-CU part; one grid pass covers
// kMaxBlocks * kBlock * 2 = 262,144 doubles, longer vectors are strided over
constexpr int64_t kMaxBlocks = 512;

enum { SC_DONE = 0, SC_KCOL = 1, SC_STEPS = 2, SC_BETA = 3, SC_BNORM = 4, SC_EST = 5, SC_TARGET = 6, SC_HN = 7, SC_N = 8 };

// the work space: vectors on an even leading dimension (16-byte loads), then the small arrays
struct Layout {
  int64_t ld = 0;
  int64_t nb = 0;   // blocks of the kernels that take two doubles per lane (16-byte loads)
  int64_t nbn = 0;  // blocks of resid_kernel, one double per lane: nbn >= nb
  int m = 0;
  double *V = nullptr, *Z = nullptr, *P = nullptr, *PN = nullptr, *sc = nullptr, *hcol = nullptr,
         *hpass = nullptr, *H = nullptr, *cs = nullptr, *sn = nullptr, *g = nullptr, *y = nullptr;
  int64_t total = 0;
};

Layout layout(int64_t n, int m, double* base)
{
  Layout L;
  L.m = m;
  L.ld = (n + 1) & ~int64_t(1);
  L.nb = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, ((n >> 1) + kBlock - 1) / kBlock));
  L.nbn = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n + kBlock - 1) / kBlock));
  int64_t o = 0;
  auto take = [&](int64_t k) {
    double* p = base ? base + o : nullptr;
    o += (k + 1) & ~int64_t(1);
    return p;
  };
  L.V = take(int64_t(m + 1) * L.ld);
  L.Z = take(int64_t(m) * L.ld);
  L.P = take(L.nb * (m + 1));
  L.PN = take(L.nbn);  // the norm partials of either kind of kernel
  L.sc = take(SC_N);
  L.hcol = take(m + 2);
  L.hpass = take(m + 2);
  L.H = take(int64_t(m + 1) * m);
  L.cs = take(m);
  L.sn = take(m);
  L.g = take(m + 1);
  L.y = take(m);
  L.total = o;
  return L;
}

// deterministic block sum (wave butterfly, then the waves in order); result valid in thread 0
__device__ inline double block_sum(double v, double* sbuf)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sbuf[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < kBlock / 64; ++i) t += sbuf[i];
  __syncthreads();
  return t;
}

template <bool FULL>
__device__ inline void dot_tile(const double* __restrict__ Vt, int64_t ld, int nt,
    const double* __restrict__ w, int64_t n, double* acc)
{
  const int64_t n2 = n >> 1, ld2 = ld >> 1;
  const double2* w2 = reinterpret_cast<const double2*>(w);
  const double2* v2 = reinterpret_cast<const double2*>(Vt);
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n2; i += int64_t(gridDim.x) * kBlock)
  {
    const double2 ww = w2[i];
#pragma unroll
    for (int k = 0; k < kTile; ++k)
      if (FULL || k < nt)
      {
        const double2 vv = v2[k * ld2 + i];
        acc[k] += vv.x * ww.x + vv.y * ww.y;
      }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < kTile; ++k)
      if (FULL || k < nt) acc[k] += Vt[k * ld + n - 1] * w[n - 1];
}

// partial[block][i] = (v_i . w) over the block's share, i = 0..nv-1
__global__ __launch_bounds__(kBlock) void multi_dot_kernel(const double* __restrict__ V, int64_t ld,
    int nv, const double* __restrict__ w, int64_t n, double* __restrict__ partial,
    const double* __restrict__ sc)
{
  __shared__ double sbuf[kBlock / 64];
  if (sc[SC_DONE] != 0.0) return;
  for (int t0 = 0; t0 < nv; t0 += kTile)
  {
    const int nt = min(kTile, nv - t0);
    double acc[kTile];
#pragma unroll
    for (int k = 0; k < kTile; ++k) acc[k] = 0.0;
    if (nt == kTile)
      dot_tile<true>(V + int64_t(t0) * ld, ld, nt, w, n, acc);
    else
      dot_tile<false>(V + int64_t(t0) * ld, ld, nt, w, n, acc);
#pragma unroll
    for (int k = 0; k < kTile; ++k)
    {
      if (k >= nt) break;  // uniform over the block
      const double t = block_sum(acc[k], sbuf);
      if (threadIdx.x == 0) partial[int64_t(blockIdx.x) * nv + t0 + k] = t;
    }
  }
}

// hpass[i] = sum over the blocks of partial[block][i], one workgroup per column i: each lane takes
// the blocks lane, lane + 256, ... in order, then the fixed-order block sum (a single lane walking
// all blocks is one chain of dependent loads, 0.1 ms at 512 blocks).  hcol[i] = (pass 0) that sum,
// (pass 1) hcol[i] + that sum: the Hessenberg column after both Gram-Schmidt passes
__global__ __launch_bounds__(kBlock) void reduce_cols_kernel(const double* __restrict__ partial,
    int64_t nb, int nv, double* __restrict__ hpass, double* __restrict__ hcol, int pass,
    const double* __restrict__ sc)
{
  __shared__ double sbuf[kBlock / 64];
  if (sc[SC_DONE] != 0.0) return;
  const int i = blockIdx.x;
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kBlock) a += partial[b * nv + i];
  const double t = block_sum(a, sbuf);
  if (threadIdx.x != 0) return;
  hpass[i] = t;
  hcol[i] = pass == 0 ? t : hcol[i] + t;
}

// w -= sum_i h_i v_i, pnorm[block] = the block's share of |w|^2 afterwards
__global__ __launch_bounds__(kBlock) void multi_axpy_norm_kernel(const double* __restrict__ V,
    int64_t ld, int nv, double* __restrict__ w, int64_t n, const double* __restrict__ h,
    double* __restrict__ pnorm, const double* __restrict__ sc)
{
  __shared__ double sh[kKrylovMaxRestart + 1];
  __shared__ double sbuf[kBlock / 64];
  if (sc[SC_DONE] != 0.0) return;
  for (int i = threadIdx.x; i < nv; i += kBlock) sh[i] = h[i];
  __syncthreads();
  const int64_t n2 = n >> 1, ld2 = ld >> 1;
  double2* w2 = reinterpret_cast<double2*>(w);
  const double2* v2 = reinterpret_cast<const double2*>(V);
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n2; i += int64_t(gridDim.x) * kBlock)
  {
    double2 ww = w2[i];
    int k = 0;
    for (; k + kTile <= nv; k += kTile)
    {
      double2 vv[kTile];
#pragma unroll
      for (int q = 0; q < kTile; ++q) vv[q] = v2[(k + q) * ld2 + i];
#pragma unroll
      for (int q = 0; q < kTile; ++q)
      {
        ww.x -= sh[k + q] * vv[q].x;
        ww.y -= sh[k + q] * vv[q].y;
      }
    }
    for (; k < nv; ++k)
    {
      const double2 vv = v2[k * ld2 + i];
      ww.x -= sh[k] * vv.x;
      ww.y -= sh[k] * vv.y;
    }
    w2[i] = ww;
    acc += ww.x * ww.x + ww.y * ww.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    double t = w[n - 1];
    for (int k = 0; k < nv; ++k) t -= sh[k] * V[k * ld + n - 1];
    w[n - 1] = t;
    acc += t * t;
  }
  const double t = block_sum(acc, sbuf);
  if (threadIdx.x == 0) pnorm[blockIdx.x] = t;
}

// r = b - r
__global__ __launch_bounds__(kBlock) void subtract_kernel(const double* __restrict__ b, double* __restrict__ r,
    int64_t n)
{
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock)
    r[i] = b[i] - r[i];
}

struct Scalars {
  double *sc, *hcol, *H, *cs, *sn, *g, *y;
  int m;
};

// the end of inner step j: h_{j+1,j} = sqrt(sum of the |w|^2 partials), the rotations, g, the
// estimate, the step count, done / bad
__global__ __launch_bounds__(kBlock) void scalar_step_kernel(const double* __restrict__ pnorm,
    int64_t nb, int j, Scalars S, int32_t* flag)
{
  __shared__ double sbuf[kBlock / 64];
  if (S.sc[SC_DONE] != 0.0) return;  // uniform: the whole block reads the same word
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) a += pnorm[i];
  const double hn2 = block_sum(a, sbuf);
  if (threadIdx.x != 0) return;
  const double hn = sqrt(hn2);
  double* h = S.hcol;
  bool finite = isfinite(hn);
  for (int i = 0; i <= j; ++i) finite = finite && isfinite(h[i]);
  if (!finite)
  {
    *flag = 1;
    S.sc[SC_DONE] = 1.0;
    return;
  }
  for (int i = 0; i < j; ++i)
  {
    const double t = S.cs[i] * h[i] + S.sn[i] * h[i + 1];
    h[i + 1] = -S.sn[i] * h[i] + S.cs[i] * h[i + 1];
    h[i] = t;
  }
  const double r = hypot(h[j], hn);
  if (r == 0.0)
  {
    // a zero column: A P is singular on the Krylov space
    *flag = 1;
    S.sc[SC_DONE] = 1.0;
    return;
  }
  const double c = h[j] / r, s = hn / r;
  S.cs[j] = c;
  S.sn[j] = s;
  h[j] = r;
  S.g[j + 1] = -s * S.g[j];
  S.g[j] = c * S.g[j];
  double* Hj = S.H + int64_t(j) * (S.m + 1);
  for (int i = 0; i <= j; ++i) Hj[i] = h[i];
  S.sc[SC_KCOL] = double(j + 1);
  S.sc[SC_STEPS] += 1.0;
  const double est = fabs(S.g[j + 1]);
  S.sc[SC_EST] = est;
  S.sc[SC_HN] = hn;
  if (est <= S.sc[SC_TARGET] || hn == 0.0) S.sc[SC_DONE] = 1.0;  // converged, or exact breakdown
}

// fcg_gmres_orthogonalize's end: h[0..nv) = the column after both passes, h[nv] = |w|
__global__ __launch_bounds__(kBlock) void orth_finish_kernel(const double* __restrict__ pnorm, int64_t nb,
    const double* __restrict__ hcol, int nv, double* __restrict__ h)
{
  __shared__ double sbuf[kBlock / 64];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) a += pnorm[i];
  const double t = block_sum(a, sbuf);
  for (int i = threadIdx.x; i < nv; i += kBlock) h[i] = hcol[i];
  if (threadIdx.x == 0) h[nv] = sqrt(t);
}

// v /= sc[SC_HN] (never reached with a zero divisor: done is set with it)
__global__ __launch_bounds__(kBlock) void scale_kernel(double* __restrict__ v, int64_t n,
    const double* __restrict__ sc)
{
  if (sc[SC_DONE] != 0.0) return;
  const double d = sc[SC_HN];
  const int64_t n2 = n >> 1;
  double2* v2 = reinterpret_cast<double2*>(v);
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n2; i += int64_t(gridDim.x) * kBlock)
  {
    double2 t = v2[i];
    t.x /= d;
    t.y /= d;
    v2[i] = t;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] /= d;
}

// r = b - ax (ax NULL: r = b; ax may be r itself; r NULL: nothing stored), pnorm[block] = the
// block's share of |r|^2.  b may be the caller's pointer: no alignment is assumed, 8-byte accesses.
__global__ __launch_bounds__(kBlock) void resid_kernel(const double* b, const double* ax, double* r,
    int64_t n, double* __restrict__ pnorm)
{
  __shared__ double sbuf[kBlock / 64];
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock)
  {
    const double t = ax ? b[i] - ax[i] : b[i];
    if (r) r[i] = t;
    acc += t * t;
  }
  const double t = block_sum(acc, sbuf);
  if (threadIdx.x == 0) pnorm[blockIdx.x] = t;
}

// r = b - K x row by row with the compensated product: 16 lanes per CSR row
constexpr int kLanesPerRow = 16;
__global__ __launch_bounds__(kBlock) void csr_residual_kernel(const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const double* __restrict__ vals, const double* __restrict__ x,
    const double* __restrict__ b, double* __restrict__ r, int64_t n_rows)
{
  constexpr int LPR = kLanesPerRow;
  const int lane = threadIdx.x % LPR;
  const int64_t row = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / LPR;
  double s = 0.0, c = 0.0;
  if (row < n_rows)
    for (int64_t j = rowptr[row] + lane; j < rowptr[row + 1]; j += LPR) dd_fma(s, c, vals[j], x[col[j]]);
  const double t = dd_row_residual<LPR>(s, c, row < n_rows ? b[row] : 0.0);
  if (row < n_rows && lane == 0) r[row] = t;
}

// start of a cycle: beta = |r| from its partials; first: |b| = beta and the target rtol |b|.
// done = the true residual is at the target (b = 0 included); a non-finite beta is bad.
__global__ __launch_bounds__(kBlock) void begin_cycle_kernel(const double* __restrict__ pnorm,
    int64_t nb, int first, double rtol, Scalars S, int32_t* flag)
{
  __shared__ double sbuf[kBlock / 64];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) a += pnorm[i];
  const double b2 = block_sum(a, sbuf);
  if (threadIdx.x != 0) return;
  const double beta = sqrt(b2);
  if (first)
  {
    S.sc[SC_BNORM] = beta;
    S.sc[SC_TARGET] = rtol * beta;
    S.sc[SC_STEPS] = 0.0;
  }
  S.sc[SC_BETA] = beta;
  S.sc[SC_EST] = beta;
  S.sc[SC_HN] = beta;
  S.sc[SC_KCOL] = 0.0;
  S.g[0] = beta;
  if (!isfinite(beta))
  {
    *flag = 1;
    S.sc[SC_DONE] = 1.0;
    return;
  }
  S.sc[SC_DONE] = beta <= S.sc[SC_TARGET] ? 1.0 : 0.0;
}

// y = R^-1 g for the sc[SC_KCOL] columns of the cycle (one lane: at most 128^2 / 2 terms)
__global__ void solve_y_kernel(Scalars S, int32_t* flag)
{
  const int k = int(S.sc[SC_KCOL]);
  const int ldh = S.m + 1;
  bool ok = true;
  for (int i = k - 1; i >= 0; --i)
  {
    double s = S.g[i];
    for (int c = i + 1; c < k; ++c) s -= S.H[i + int64_t(c) * ldh] * S.y[c];
    const double d = S.H[i + int64_t(i) * ldh];
    const double q = d != 0.0 ? s / d : NAN;
    ok = ok && isfinite(q);
    S.y[i] = q;
  }
  if (!ok)
  {
    *flag = 1;
    for (int i = 0; i < k; ++i) S.y[i] = 0.0;
  }
}

// x += sum_{c < kcol} y_c z_c
__global__ __launch_bounds__(kBlock) void update_x_kernel(const double* __restrict__ Z, int64_t ld,
    const double* __restrict__ y, const double* __restrict__ sc, double* __restrict__ x, int64_t n)
{
  __shared__ double sh[kKrylovMaxRestart];
  const int k = int(sc[SC_KCOL]);
  for (int i = threadIdx.x; i < k; i += kBlock) sh[i] = y[i];
  __syncthreads();
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  double t = x[i];
  for (int c = 0; c < k; ++c) t += sh[c] * Z[c * ld + i];
  x[i] = t;
}

}  // namespace

int64_t krylov_work_doubles(int64_t n, int m) { return layout(n, m, nullptr).total; }

// fcg_gmres_set_timing / fcg_gmres_get_timing: per-phase hipEvent sums over the launched steps
struct KrylovTiming {
  bool on = false;
  double ms_precond = 0.0, ms_operator = 0.0, ms_orth = 0.0;
  int64_t steps = 0;
  hipEvent_t ev[kKrylovBurst][4] = {};
  bool have_events = false;
};
static KrylovTiming g_timing;

int KrylovOps::residual(const double* b, const double* x, double* r, int64_t n, hipStream_t s)
{
  const int rc = apply(x, r, s);
  if (rc != FCG_OK) return rc;
  const unsigned g = unsigned(std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n + kBlock - 1) / kBlock)));
  hipLaunchKernelGGL(subtract_kernel, dim3(g), dim3(kBlock), 0, s, b, r, n);
  const hipError_t he = hipGetLastError();
  if (he == hipSuccess) return FCG_OK;
  error = std::string("HIP: ") + hipGetErrorString(he);
  return fcg_device_error();
}

hipError_t krylov_reserve(double** work, int64_t* have, int64_t doubles, int64_t* device_bytes)
{
  if (*work && *have >= doubles) return hipSuccess;
  if (*work)
  {
    (void)hipFree(*work);
    *device_bytes -= *have * int64_t(sizeof(double));
    *work = nullptr;
    *have = 0;
  }
  hipError_t he = hipMalloc(reinterpret_cast<void**>(work), sizeof(double) * size_t(doubles));
  if (he != hipSuccess)
  {
    *work = nullptr;
    return he;
  }
  // a front's preconditioner still runs in the no-op steps after `done` and may then read a basis
  // vector that was never written: start finite
  he = hipMemset(*work, 0, sizeof(double) * size_t(doubles));
  if (he != hipSuccess)
  {
    (void)hipFree(*work);
    *work = nullptr;
    return he;
  }
  *have = doubles;
  *device_bytes += doubles * int64_t(sizeof(double));
  return hipSuccess;
}

int fgmres(KrylovOps& ops, int64_t n, const double* d_b, double* d_x, int m, int max_iter,
    double rtol, double* work, int32_t* flag, hipStream_t s, int* iterations, double* rel_residual,
    std::string& error)
{
  const Layout L = layout(n, m, work);
  const Scalars S{L.sc, L.hcol, L.H, L.cs, L.sn, L.g, L.y, m};
  const dim3 grid(unsigned(L.nb)), one(1), bl(kBlock);
  const dim3 grid_n(unsigned(L.nbn));
  const dim3 grid_all(unsigned((n + kBlock - 1) / kBlock));
  double hsc[SC_N] = {0};
  int32_t bad = 0;
  auto device_fail = [&](hipError_t he) {
    error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  };
  // the scalar block and the flag word, after everything queued so far
  auto read_state = [&]() -> hipError_t {
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(hsc, L.sc, sizeof(hsc), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    return he;
  };
  auto set_out = [&]() {
    if (iterations) *iterations = int(hsc[SC_STEPS]);
    if (rel_residual) *rel_residual = hsc[SC_BNORM] > 0.0 ? hsc[SC_BETA] / hsc[SC_BNORM] : 0.0;
  };

  hipError_t he = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
  if (he == hipSuccess) he = hipMemsetAsync(d_x, 0, sizeof(double) * size_t(n), s);
  if (he != hipSuccess) return device_fail(he);
  // r_0 = b
  hipLaunchKernelGGL(resid_kernel, grid_n, bl, 0, s, d_b, static_cast<const double*>(nullptr), L.V, n, L.PN);
  hipLaunchKernelGGL(begin_cycle_kernel, one, bl, 0, s, L.PN, int64_t(grid_n.x), 1, rtol, S, flag);
  hipLaunchKernelGGL(scale_kernel, grid, bl, 0, s, L.V, n, L.sc);
  he = read_state();
  if (he != hipSuccess) return device_fail(he);
  set_out();
  if (bad)
  {
    error = "non-finite right-hand side";
    return FCG_ERR_SINGULAR;
  }
  bool converged = hsc[SC_DONE] != 0.0;  // b = 0 (x = 0), or rtol >= 1
  while (!converged && int(hsc[SC_STEPS]) < max_iter)
  {
    const int it0 = int(hsc[SC_STEPS]);
    int j = 0;
    bool done = false;
    while (!done && j < m && it0 + j < max_iter)
    {
      const int burst = std::min(kKrylovBurst, std::min(m - j, max_iter - it0 - j));
      const bool timed = g_timing.on && g_timing.have_events;
      for (int k = 0; k < burst; ++k, ++j)
      {
        double* zj = L.Z + int64_t(j) * L.ld;
        double* w = L.V + int64_t(j + 1) * L.ld;
        if (timed) (void)hipEventRecord(g_timing.ev[k][0], s);
        int rc = ops.precond(L.V + int64_t(j) * L.ld, zj, s);
        if (timed) (void)hipEventRecord(g_timing.ev[k][1], s);
        if (rc == FCG_OK) rc = ops.apply(zj, w, s);
        if (timed) (void)hipEventRecord(g_timing.ev[k][2], s);
        if (rc != FCG_OK)
        {
          error = ops.error;
          (void)hipStreamSynchronize(s);
          return rc;
        }
        for (int pass = 0; pass < 2; ++pass)
        {
          hipLaunchKernelGGL(multi_dot_kernel, grid, bl, 0, s, L.V, L.ld, j + 1, w, n, L.P, L.sc);
          hipLaunchKernelGGL(reduce_cols_kernel, dim3(unsigned(j + 1)), bl, 0, s, L.P, L.nb, j + 1, L.hpass, L.hcol, pass, L.sc);
          hipLaunchKernelGGL(multi_axpy_norm_kernel, grid, bl, 0, s, L.V, L.ld, j + 1, w, n, L.hpass, L.PN, L.sc);
        }
        hipLaunchKernelGGL(scalar_step_kernel, one, bl, 0, s, L.PN, L.nb, j, S, flag);
        hipLaunchKernelGGL(scale_kernel, grid, bl, 0, s, w, n, L.sc);
        if (timed) (void)hipEventRecord(g_timing.ev[k][3], s);
      }
      he = read_state();
      if (he != hipSuccess) return device_fail(he);
      for (int k = 0; timed && k < burst; ++k)
      {
        float a = 0.f, b = 0.f, c = 0.f;
        (void)hipEventElapsedTime(&a, g_timing.ev[k][0], g_timing.ev[k][1]);
        (void)hipEventElapsedTime(&b, g_timing.ev[k][1], g_timing.ev[k][2]);
        (void)hipEventElapsedTime(&c, g_timing.ev[k][2], g_timing.ev[k][3]);
        g_timing.ms_precond += a;
        g_timing.ms_operator += b;
        g_timing.ms_orth += c;
        g_timing.steps += 1;
      }
      set_out();
      if (bad)
      {
        error = "non-finite or singular Hessenberg column (a non-finite matrix entry, or A P singular)";
        return FCG_ERR_SINGULAR;
      }
      done = hsc[SC_DONE] != 0.0;
    }
    // x += Z y, then the true residual: it is the answer's, and the next cycle's start
    hipLaunchKernelGGL(solve_y_kernel, one, one, 0, s, S, flag);
    hipLaunchKernelGGL(update_x_kernel, grid_all, bl, 0, s, L.Z, L.ld, L.y, L.sc, d_x, n);
    const int rc = ops.residual(d_b, d_x, L.V, n, s);
    if (rc != FCG_OK)
    {
      error = ops.error;
      (void)hipStreamSynchronize(s);
      return rc;
    }
    hipLaunchKernelGGL(resid_kernel, grid_n, bl, 0, s, static_cast<const double*>(L.V),
        static_cast<const double*>(nullptr), static_cast<double*>(nullptr), n, L.PN);
    hipLaunchKernelGGL(begin_cycle_kernel, one, bl, 0, s, L.PN, int64_t(grid_n.x), 0, rtol, S, flag);
    hipLaunchKernelGGL(scale_kernel, grid, bl, 0, s, L.V, n, L.sc);
    he = read_state();
    if (he != hipSuccess) return device_fail(he);
    set_out();
    if (bad)
    {
      error = "non-finite residual or singular Hessenberg matrix";
      return FCG_ERR_SINGULAR;
    }
    converged = hsc[SC_DONE] != 0.0;
  }
  return FCG_OK;
}

namespace {

// fcg_gmres_solve's operator and preconditioner: the context's CSR product; the nodal block
// Jacobi (dinv from fcg_block_jacobi_setup) or one multigrid cycle
struct SingleFieldOps : KrylovOps {
  fcg_ctx* ctx;
  fcg_amg* amg;
  const double* K;
  const double* dinv;
  int apply(const double* x, double* y, hipStream_t s) override
  {
    const int rc = fcg_spmv(ctx, K, x, y, s);
    if (rc != FCG_OK) error = ctx->last_error;
    return rc;
  }
  int residual(const double* b, const double* x, double* r, int64_t n, hipStream_t s) override
  {
    const DeviceMesh& m = ctx->mesh;
    hipLaunchKernelGGL(csr_residual_kernel, dim3(unsigned((n * kLanesPerRow + kBlock - 1) / kBlock)),
        dim3(kBlock), 0, s, m.rowptr, m.col_lid, K, x, b, r, n);
    const hipError_t he = hipGetLastError();
    if (he == hipSuccess) return FCG_OK;
    error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  int precond(const double* r, double* z, hipStream_t s) override
  {
    if (amg)
    {
      const int rc = fcg_amg_apply(amg, K, r, z, s);
      if (rc != FCG_OK) error = fcg_amg_last_error(amg);
      return rc;
    }
    const int rc = fcg_block_jacobi_apply(ctx, dinv, r, z, 1.0, 0, s);
    if (rc != FCG_OK) error = ctx->last_error;
    return rc;
  }
};

}  // namespace

}  // namespace fcg

extern "C" {

int fcg_gmres_set_timing(int enable)
{
  fcg::KrylovTiming& t = fcg::g_timing;
  if (enable && !t.have_events)
  {
    for (auto& row : t.ev)
      for (hipEvent_t& e : row)
        if (hipEventCreate(&e) != hipSuccess) return fcg_device_error();
    t.have_events = true;
  }
  t.on = enable != 0;
  t.ms_precond = t.ms_operator = t.ms_orth = 0.0;
  t.steps = 0;
  return FCG_OK;
}

int fcg_gmres_get_timing(double* ms_precond, double* ms_operator, double* ms_orth, int64_t* steps)
{
  const fcg::KrylovTiming& t = fcg::g_timing;
  if (ms_precond) *ms_precond = t.ms_precond;
  if (ms_operator) *ms_operator = t.ms_operator;
  if (ms_orth) *ms_orth = t.ms_orth;
  if (steps) *steps = t.steps;
  return FCG_OK;
}

int64_t fcg_gmres_orthogonalize_work(int64_t n, int nv)
{
  if (n < 0 || nv < 1 || nv > fcg::kKrylovMaxRestart) return -1;
  // partials [nb][nv] | norm partials [nbn] | done word | column | pass coefficients
  const fcg::Layout L = fcg::layout(n, 1, nullptr);
  return L.nb * nv + L.nbn + 2 + 2 * (int64_t(nv) + 2);
}

int fcg_gmres_orthogonalize(int device, int64_t n, int nv, const double* d_V, int64_t ld, double* d_w,
    double* d_h, double* d_work, void* stream)
{
  using namespace fcg;
  if (n < 0 || nv < 1 || nv > kKrylovMaxRestart || ld < n || (ld & 1) || !d_V || !d_w || !d_h || !d_work ||
      (reinterpret_cast<uintptr_t>(d_V) & 15) || (reinterpret_cast<uintptr_t>(d_w) & 15))
    return FCG_ERR_ARG;
  if (!fcg_use_device(device)) return fcg_device_error();
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Layout L = layout(n, 1, nullptr);
  double* P = d_work;
  double* PN = P + L.nb * nv;
  double* sc = PN + L.nbn;  // only the done word is read: 0
  double* hcol = sc + 2;
  double* hpass = hcol + nv + 2;
  if (hipMemsetAsync(sc, 0, 2 * sizeof(double), s) != hipSuccess) return fcg_device_error();
  const dim3 grid(unsigned(L.nb)), one(1), bl(kBlock);
  for (int pass = 0; pass < 2; ++pass)
  {
    hipLaunchKernelGGL(multi_dot_kernel, grid, bl, 0, s, d_V, ld, nv, d_w, n, P, sc);
    hipLaunchKernelGGL(reduce_cols_kernel, dim3(unsigned(nv)), bl, 0, s, P, L.nb, nv, hpass, hcol, pass, sc);
    hipLaunchKernelGGL(multi_axpy_norm_kernel, grid, bl, 0, s, d_V, ld, nv, d_w, n, hpass, PN, sc);
  }
  hipLaunchKernelGGL(orth_finish_kernel, one, bl, 0, s, PN, L.nb, hcol, nv, d_h);
  return hipGetLastError() == hipSuccess ? FCG_OK : fcg_device_error();
}

void fcg_gmres_default_options(fcg_gmres_options* opt)
{
  if (!opt) return;
  opt->restart = 50;
  opt->max_iter = 10000;
  opt->rtol = 1e-10;
  opt->precond = 1;
  opt->reserved = 0;
}

int fcg_gmres_solve(fcg_ctx* ctx, fcg_amg* amg, const double* d_K_vals, const double* d_b_row,
    double* d_x_row, const fcg_gmres_options* opt, int* iterations, double* rel_residual,
    void* stream)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!opt || opt->restart < 1 || opt->restart > fcg::kKrylovMaxRestart || opt->max_iter < 0 ||
      !(opt->rtol >= 0.0))
  {
    ctx->last_error = "fcg_gmres_solve: restart must lie in [1, 128], max_iter >= 0 and rtol >= 0";
    return FCG_ERR_ARG;
  }
  fcg::DeviceMesh& m = ctx->mesh;
  if (!m.square_local)
  {
    ctx->last_error = "fcg_gmres_solve needs a single-rank system (matrix column map = row map)";
    return FCG_ERR_ARG;
  }
  const int64_t n = m.n_rows, nn = m.n_rownodes;
  if (iterations) *iterations = 0;
  if (rel_residual) *rel_residual = 0.0;
  if (n == 0) return FCG_OK;
  if (!d_K_vals || !d_b_row || !d_x_row) return FCG_ERR_ARG;
  if (3 * nn != n)
  {
    ctx->last_error = "fcg_gmres_solve: every owned row must belong to an owned node's DOF triple";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const int64_t core = fcg::krylov_work_doubles(n, opt->restart);
  const hipError_t he = fcg::krylov_reserve(&m.krylov_work, &m.krylov_doubles, core + 3 * n, &ctx->device_bytes);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("fcg_gmres_solve: work space: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  double* dinv = m.krylov_work + core;  // 9 doubles per owned node
  if (!amg)
  {
    const int rc = fcg_block_jacobi_setup(ctx, d_K_vals, dinv, s);
    if (rc != FCG_OK) return rc;
  }
  fcg::SingleFieldOps ops;
  ops.ctx = ctx;
  ops.amg = amg;
  ops.K = d_K_vals;
  ops.dinv = dinv;
  std::string err;
  const int rc = fcg::fgmres(ops, n, d_b_row, d_x_row, opt->restart, opt->max_iter, opt->rtol,
      m.krylov_work, m.err + 2, s, iterations, rel_residual, err);
  if (rc != FCG_OK) ctx->last_error = "fcg_gmres_solve: " + err;
  return rc;
}

}  // extern "C"
