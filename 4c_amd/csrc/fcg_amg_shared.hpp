// fcg_amg_shared.hpp -- what the structural AMG (fcg_amg_solver.hip, fcg_amg_coupled.hip) and the
// scalar AMG of K_TT (fcg_samg.hip) have in common: the vector and flexible-CG kernels behind host
// launchers, the Lanczos estimate of lambda_max (the recurrence here, the Sturm bisection of its
// tridiagonal), the Chebyshev smoother's coefficients and the dense coarsest level (Gauss-Jordan
// inverse, one matrix-vector product per cycle).  The kernels and the functions declared here are
// defined in fcg_amg_vec.hip; the templates are complete here.  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace fcg_amgs {

constexpr int kBlock = 256;          // threads per workgroup of the kernels of both AMGs
constexpr int kMaxPartials = 1024;   // doubles of scratch a dot product needs
constexpr int64_t kDenseMax = 4096;  // largest coarsest level inverted densely (2 x 134 MB)

// ---- vector kernels: asynchronous on s, one thread per entry (at least one workgroup) ------------
// *out = a . b: fixed grid-stride shares into partial[kMaxPartials], then one workgroup sums them
// (the same bits on every run)
void dot(const double* a, const double* b, int64_t n, double* partial, double* out, hipStream_t s);
// y = a x + b y
void axpby(double a, const double* x, double b, double* y, int64_t n, hipStream_t s);
// flexible CG with its scalars on the device, sc[0] = r.z, sc[1] = p.q, sc[2] = r.z new, sc[5] =
// z.r_old.  Step: alpha = r.z / p.q; x += alpha p; r_old = r; r -= alpha q.  Direction
// (Polak-Ribiere): p = z + beta p, beta = (r.z new - z.r_old) / r.z.  Shift: sc[0] = sc[2].
void fcg_step(const double* sc, const double* p, const double* q, double* x, double* r, double* r_old,
    int64_t n, hipStream_t s);
void fcg_dir(const double* sc, const double* z, double* p, int64_t n, hipStream_t s);
void fcg_shift(double* sc, hipStream_t s);

// a . b read back on the host through the device slot; ck(hipError_t, const char*) is the caller's
// check of the copy and the synchronisation (its error code, its message)
template <typename Ck>
double dot_host(const double* a, const double* b, int64_t n, double* partial, double* slot, hipStream_t s,
    Ck&& ck)
{
  dot(a, b, n, partial, slot, s);
  double v = 0.0;
  ck(hipMemcpyAsync(&v, slot, sizeof(double), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
  ck(hipStreamSynchronize(s), "hipStreamSynchronize");
  return v;
}

// ---- lambda_max of D^-1 A ----------------------------------------------------------------------
// The 10-step preconditioned-CG recurrence on the caller's start (r, z = D^-1 r, p = z): spmv(p, q)
// applies A, dinv(r, z) applies D^-1, dot(a, b) returns the inner product on the host (summed over
// the ranks where the operator is).  Yields the step lengths al and the ratios be[i] = r.z new /
// r.z for lanczos_lmax; it stops early when p.Ap or r.z is no longer positive, so al comes back
// empty when the first p.Ap is not positive.
struct LanczosSteps {
  std::vector<double> al, be;
};
template <typename Spmv, typename Dinv, typename Dot>
LanczosSteps lanczos_steps(Spmv&& spmv, Dinv&& dinv, Dot&& dot, double* r, double* z, double* p, double* q,
    int64_t n, hipStream_t s)
{
  LanczosSteps t;
  double rz = dot(r, z);
  for (int it = 0; it < 10; ++it)
  {
    spmv(p, q);
    const double pq = dot(p, q);
    if (!(pq > 0.0)) break;
    const double alpha = rz / pq;
    axpby(-alpha, q, 1.0, r, n, s);
    dinv(r, z);
    const double rzn = dot(r, z);
    t.al.push_back(alpha);
    if (!(rzn > 0.0)) break;
    t.be.push_back(rzn / rz);
    axpby(1.0, z, rzn / rz, p, n, s);
    rz = rzn;
  }
  return t;
}

// largest eigenvalue of the Lanczos tridiagonal of a preconditioned CG run with the step lengths
// al[0..k) and the ratios be[i] = r.z new / r.z (bisection on the Sturm sequence)
double lanczos_lmax(const std::vector<double>& al, const std::vector<double>& be);

// ---- Chebyshev smoother ------------------------------------------------------------------------
// Coefficients of the nu-degree Chebyshev iteration on [lmax / ratio, lmax], lmax = boost times the
// estimate of lambda_max(D^-1 A): the first degree is d = first() D^-1 r, every further one
// d = c_d d + c_r D^-1 r with the pair next() returns (both AMGs: x += d after each).  The values
// are kernel arguments, so the expressions keep their association.
struct ChebCoef {
  double theta, delta, sigma, rho;
  ChebCoef(double lmax_estimate, double boost, double ratio)
  {
    const double lmax = boost * lmax_estimate;
    const double lmin = lmax / ratio;
    theta = 0.5 * (lmax + lmin);
    delta = 0.5 * (lmax - lmin);
    sigma = theta / delta;
    rho = 1.0 / sigma;
  }
  double first() const { return 1.0 / theta; }
  struct Degree {
    double c_d, c_r;
  };
  Degree next()
  {
    const double rho_n = 1.0 / (2.0 * sigma - rho);
    const Degree g{rho_n * rho, 2.0 * rho_n / delta};
    rho = rho_n;
    return g;
  }
};

// ---- the coarsest level, dense -------------------------------------------------------------------
// Gauss-Jordan inverse of the dense row-major n x n matrix in buf[0], ping-ponging with buf[1]
// (work: dense_inverse_work(n) doubles).  Returns the index of the buffer that holds the inverse;
// a pivot that is not positive sets *d_flag (zeroed by the caller).  Asynchronous on s.
int64_t dense_inverse_work(int64_t n);
int dense_inverse(double* const buf[2], double* work, int64_t n, int32_t* d_flag, hipStream_t s);
// y = D x, one wavefront per row, fixed-order reduction
void dense_mv(const double* D, const double* x, double* y, int64_t n, hipStream_t s);

}  // namespace fcg_amgs
