// fcg_amg_shared.hpp -- the pieces of the structural AMG (fcg_amg_solver.hip) that the scalar AMG
// of K_TT (fcg_samg.hip) uses as they are: the Sturm bisection of the Lanczos estimate and the
// dense coarsest level (Gauss-Jordan inverse, one matrix-vector product per cycle).  Defined in
// fcg_amg_solver.hip.  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace fcg_amgs {

constexpr int64_t kDenseMax = 4096;  // largest coarsest level inverted densely (2 x 134 MB)

// largest eigenvalue of the Lanczos tridiagonal of a preconditioned CG run with the step lengths
// al[0..k) and the ratios be[i] = r.z new / r.z (bisection on the Sturm sequence)
double lanczos_lmax(const std::vector<double>& al, const std::vector<double>& be);

// Gauss-Jordan inverse of the dense row-major n x n matrix in buf[0], ping-ponging with buf[1]
// (work: dense_inverse_work(n) doubles).  Returns the index of the buffer that holds the inverse;
// a pivot that is not positive sets *d_flag (zeroed by the caller).  Asynchronous on s.
int64_t dense_inverse_work(int64_t n);
int dense_inverse(double* const buf[2], double* work, int64_t n, int32_t* d_flag, hipStream_t s);
// y = D x, one wavefront per row, fixed-order reduction
void dense_mv(const double* D, const double* x, double* y, int64_t n, hipStream_t s);

}  // namespace fcg_amgs
