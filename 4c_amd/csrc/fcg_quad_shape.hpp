// fcg_quad_shape.hpp -- the surface elements of hex8 / hex27: the quad_4point / quad_9point rules
// (4C_fem_general_utils_integration.cpp, with the reference's truncated constants) and the quad4 /
// quad9 shape functions (4C_fem_general_utils_fem_shapefunctions.hpp:2003-2087, 2148-2274), shared
// by the structural Neumann loads (fcg_neumann.cpp) and the thermal surface plan
// (fcg_tsi_surface_plan.cpp).  Host only.
#pragma once

namespace fcg {

inline void quad_rule(int nfn, double (*xg)[2], double* w)
{
  if (nfn == 4)
  {
    const double a = 0.5773502691896;
    const double p[4][2] = {{-a, -a}, {a, -a}, {a, a}, {-a, a}};
    for (int g = 0; g < 4; ++g)
    {
      xg[g][0] = p[g][0];
      xg[g][1] = p[g][1];
      w[g] = 1.0;
    }
    return;
  }
  const double b = 0.7745966692415, w1 = 0.5555555555556, w2 = 0.8888888888889;
  const double p[9][2] = {{-b, -b}, {b, -b}, {b, b}, {-b, b}, {0.0, -b}, {b, 0.0}, {0.0, b},
      {-b, 0.0}, {0.0, 0.0}};
  const double ww[9] = {w1 * w1, w1 * w1, w1 * w1, w1 * w1, w2 * w1, w1 * w2, w2 * w1, w1 * w2,
      w2 * w2};
  for (int g = 0; g < 9; ++g)
  {
    xg[g][0] = p[g][0];
    xg[g][1] = p[g][1];
    w[g] = ww[g];
  }
}

inline void quad_shape(int nfn, double r, double s, double* N, double (*dN)[9])
{
  const double rp = 1.0 + r, rm = 1.0 - r, sp = 1.0 + s, sm = 1.0 - s;
  if (nfn == 4)
  {
    N[0] = 0.25 * rm * sm;
    N[1] = 0.25 * rp * sm;
    N[2] = 0.25 * rp * sp;
    N[3] = 0.25 * rm * sp;
    dN[0][0] = -0.25 * sm; dN[0][1] = 0.25 * sm; dN[0][2] = 0.25 * sp; dN[0][3] = -0.25 * sp;
    dN[1][0] = -0.25 * rm; dN[1][1] = -0.25 * rp; dN[1][2] = 0.25 * rp; dN[1][3] = 0.25 * rm;
    return;
  }
  const double r2 = 1.0 - r * r, s2 = 1.0 - s * s;
  const double rh = 0.5 * r, sh = 0.5 * s, rs = rh * sh;
  const double rhp = r + 0.5, rhm = r - 0.5, shp = s + 0.5, shm = s - 0.5;
  N[0] = rs * rm * sm;
  N[1] = -rs * rp * sm;
  N[2] = rs * rp * sp;
  N[3] = -rs * rm * sp;
  N[4] = -sh * sm * r2;
  N[5] = rh * rp * s2;
  N[6] = sh * sp * r2;
  N[7] = -rh * rm * s2;
  N[8] = r2 * s2;
  const double d0[9] = {-rhm * sh * sm, -rhp * sh * sm, rhp * sh * sp, rhm * sh * sp,
      2.0 * r * sh * sm, rhp * s2, -2.0 * r * sh * sp, rhm * s2, -2.0 * r * s2};
  const double d1[9] = {-shm * rh * rm, shm * rh * rp, shp * rh * rp, -shp * rh * rm, shm * r2,
      -2.0 * s * rh * rp, shp * r2, 2.0 * s * rh * rm, -2.0 * s * r2};
  for (int i = 0; i < 9; ++i)
  {
    dN[0][i] = d0[i];
    dN[1][i] = d1[i];
  }
}

}  // namespace fcg
