// fcg_krylov.hpp -- the restarted flexible GMRES core (fcg_krylov.hip) and the interfaces its
// fronts supply.  Not part of the public ABI: fcg_gmres_solve and fcg_tsi_gmres_solve are.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace fcg {

constexpr int kKrylovMaxRestart = 128;
constexpr int kKrylovBurst = 8;  // inner steps between two host reads of the scalar block

// The operator and the preconditioner of one solve: y = A x and z = P r on vectors of n doubles,
// queued on `s`.  Both return an FCG status; on failure they leave the message in `error`.
// residual: r = b - A x, the true residual the solve restarts from and hands back.  The default
// is apply and a subtraction in FP64, whose rounding (row length x 2^-53 |A||x|) is what limits how
// small a residual can be told from noise; the fronts override it with a compensated product.
struct KrylovOps {
  std::string error;
  virtual ~KrylovOps() = default;
  virtual int apply(const double* x, double* y, hipStream_t s) = 0;
  virtual int precond(const double* r, double* z, hipStream_t s) = 0;
  virtual int residual(const double* b, const double* x, double* r, int64_t n, hipStream_t s);
};

#ifdef __HIPCC__
// Compensated accumulation (Ogita, Rump, Oishi, "Accurate sum and dot product", SIAM J. Sci.
// Comput. 26, 2005: Dot2): (s, c) += a x with the product's and the sum's rounding errors kept
// in c, so s + c is the sum as if formed in twice the precision.  Contraction is switched off in
// these bodies: fused into s + a x, the sum's error term would hold the product's error too and c
// would count it twice (the rounded intrinsics do not keep the compiler from fusing: plain
// operators under the pragma do).
__device__ inline void dd_two_sum(double& s, double& c, double p)
{
#pragma clang fp contract(off)
  const double t = s + p;
  const double z = t - s;
  const double err = (s - (t - z)) + (p - z);
  s = t;
  c = c + err;
}
__device__ inline void dd_fma(double& s, double& c, double a, double x)
{
#pragma clang fp contract(off)
  const double p = a * x;
  c = c + __builtin_fma(a, x, -p);
  dd_two_sum(s, c, p);
}
// the sums of LPR lanes merged in a fixed (butterfly) order, then b - (s + c)
template <int LPR>
__device__ inline double dd_row_residual(double s, double c, double b)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1)
  {
    const double s2 = __shfl_xor(s, o, LPR), c2 = __shfl_xor(c, o, LPR);
    c = c + c2;
    dd_two_sum(s, c, s2);
  }
  double t = b, e = 0.0;
  dd_two_sum(t, e, -s);
  return t + (e - c);
}
#endif

// doubles of work space fgmres needs for n unknowns and restart m
int64_t krylov_work_doubles(int64_t n, int m);

// (Re)allocates *work to at least `doubles` (zero-filled) and keeps *have and *device_bytes right.
hipError_t krylov_reserve(double** work, int64_t* have, int64_t doubles, int64_t* device_bytes);

// Right-preconditioned FGMRES(m) from x = 0 for A x = b.  `flag`: the solver flag word of the
// context (set to 1 by the device for a non-finite or singular quantity).  Returns FCG_OK (also at
// max_iter), FCG_ERR_SINGULAR, a device error, or what ops returned; `error` then says why.
int fgmres(KrylovOps& ops, int64_t n, const double* d_b, double* d_x, int m, int max_iter,
    double rtol, double* work, int32_t* flag, hipStream_t s, int* iterations, double* rel_residual,
    std::string& error);

}  // namespace fcg
