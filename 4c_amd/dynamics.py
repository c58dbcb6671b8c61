"""Structural dynamics on the device: 4C's generalized-alpha time integrator (DYNAMICTYPE GenAlpha,
4C_structure_new_impl_genalpha.cpp) around the assembly, the mass kernels and the linear solvers.

End-point evaluation with linearly interpolated forces (the alphas weigh the OLD state):
  v_{n+1} = gamma/(beta dt) (d_{n+1} - d_n) - (gamma - beta)/beta v_n - (gamma - 2 beta)/(2 beta) dt a_n
  a_{n+1} = (d_{n+1} - d_n)/(beta dt^2) - v_n/(beta dt) - (1 - 2 beta)/(2 beta) a_n
  R = M [(1 - alpha_m) a_{n+1} + alpha_m a_n] + C [(1 - alpha_f) v_{n+1} + alpha_f v_n]
      + (1 - alpha_f) f_int(d_{n+1}) + alpha_f f_int(d_n)
      - [(1 - alpha_f) f_ext(t_{n+1}) + alpha_f f_ext(t_n)]
  K_eff = (1 - alpha_m)/(beta dt^2) M + (1 - alpha_f) gamma/(beta dt) C + (1 - alpha_f) K(d_{n+1})
  C = dampM M + dampK K(d_0)                      (Rayleigh damping with the initial stiffness)

Per Newton iteration: one fcg_evaluate_device (CALC_NLNSTIFF, OVERWRITE), one
fcg_effective_tangent -- K_eff in place and the M (...) product of the residual in the same pass;
mass-proportional damping only changes its cM and its vector --, fcg_dirichlet_apply and the linear
solve (fcg_pcg_solve, or any linear_solver that works from the K values it is handed, e.g.
amg.NativeAMG).  M lives in the compact node form (nnz / 9 doubles, fcg_mass_nodal).

Single rank, homogeneous-in-time Dirichlet conditions (the constrained DOFs keep their initial
displacement, v = a = 0 there); u, v, a, f, K stay in HBM.
"""

import numpy as np
import torch

from . import fcg
from .newton import ForcingTerm, accept_linear_solve


def genalpha_params(rho_inf):
    """(alpha_m, alpha_f, beta, gamma) of the generalized-alpha scheme for the spectral radius
    rho_inf in [0, 1] (Chung & Hulbert 1993; 4C's RHO_INF): second order, unconditionally stable,
    rho_inf = 1 without numerical dissipation."""
    rho_inf = float(rho_inf)
    if not 0.0 <= rho_inf <= 1.0:
        raise ValueError(f"rho_inf must lie in [0, 1], not {rho_inf}")
    alpha_m = (2.0 * rho_inf - 1.0) / (rho_inf + 1.0)
    alpha_f = rho_inf / (rho_inf + 1.0)
    beta = 0.25 * (1.0 - alpha_m + alpha_f) ** 2
    gamma = 0.5 - alpha_m + alpha_f
    return alpha_m, alpha_f, beta, gamma


class GenAlpha:
    def __init__(self, evaluator, density, dt, fext, dbc_rows, rho_inf=1.0, params=None,
                 damping=(0.0, 0.0), lumped=False, ele_density=None, tol_res=1e-10, tol_inc=1e-10,
                 max_iter=20, lin_rtol=1e-13, lin_max_iter=100000, forcing=None,
                 linear_solver=None, rescue_bad_newton_solve=True):
        """fext: a row vector (constant load) or a callable t -> row vector (numpy or device
        tensor).  params: (alpha_m, alpha_f, beta, gamma), else genalpha_params(rho_inf).
        damping = (dampM, dampK): Rayleigh damping C = dampM M + dampK K(d_0); dampK != 0 keeps a
        copy of K(d_0), nnz more doubles of device memory, and adds it with torch.  lumped=True:
        row-sum lumped mass (4C's LUMPMASS) through torch elementwise operations and a diagonal
        update of K.  The Newton and linear-solver options are newton.StaticNewton's."""
        info = evaluator.info
        self.ev = evaluator
        self.dev = torch.device("cuda", evaluator.device)
        self.n = int(info.n_rows)
        if int(info.n_cols) != self.n:
            raise ValueError("GenAlpha is single-rank: the column map must be the row map")
        self.nnz = int(info.nnz)
        self.dt = float(dt)
        if not self.dt > 0.0:
            raise ValueError("dt must be positive")
        self.alpha_m, self.alpha_f, self.beta, self.gamma = (
            params if params is not None else genalpha_params(rho_inf))
        self.damp_m, self.damp_k = float(damping[0]), float(damping[1])
        self.lumped = bool(lumped)
        self._fext = fext
        self.dbc = torch.as_tensor(np.unique(np.asarray(dbc_rows, dtype=np.int32))).to(self.dev)
        self._dbc64 = self.dbc.to(torch.int64)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.m_node, self.m_lumped = evaluator.mass_nodal(density, ele_density)
        if self.lumped:
            rowptr, col = evaluator.graph()
            rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(rowptr))
            diag = np.nonzero(col == rows)[0]
            if len(diag) != self.n:
                raise ValueError("lumped=True needs a diagonal entry in every row")
            self._diag = torch.as_tensor(diag).to(self.dev)
        self.K = torch.empty(self.nnz, **f64)
        self.K0 = None
        self.d = torch.zeros(self.n, **f64)
        self.v = torch.zeros(self.n, **f64)
        self.a = torch.zeros(self.n, **f64)
        self.fint = torch.zeros(self.n, **f64)      # f_int(d_{n+1}) of the last evaluate
        self.fint_n = torch.zeros(self.n, **f64)    # f_int(d_n)
        self.fext_n = torch.zeros(self.n, **f64)    # f_ext(t_n)
        self.r = torch.empty(self.n, **f64)
        self.du = torch.empty(self.n, **f64)
        self.freact = torch.zeros(self.n, **f64)
        self._x = torch.empty(self.n, **f64)
        self._y = torch.empty(self.n, **f64)
        self.t = 0.0
        self.nstep = 0
        self.tol_res, self.tol_inc, self.max_iter = tol_res, tol_inc, max_iter
        self.lin_rtol, self.lin_max_iter = lin_rtol, lin_max_iter
        self.rescue = rescue_bad_newton_solve
        self.forcing = forcing if forcing is not None else ForcingTerm("Constant", constant=lin_rtol)
        self.linear_solver = linear_solver
        if linear_solver is not None and hasattr(linear_solver, "check_dirichlet"):
            linear_solver.check_dirichlet(dbc_rows)
        self.history = []
        self._initialized = False

    # ------------------------------------------------------------------ pieces
    def fext_at(self, t):
        f = self._fext(t) if callable(self._fext) else self._fext
        if not torch.is_tensor(f):
            f = torch.as_tensor(np.asarray(f, dtype=np.float64))
        return f.to(device=self.dev, dtype=torch.float64)

    def mass_times(self, x, y):
        """y = M x (consistent: fcg_effective_tangent without K; lumped: elementwise)."""
        if self.lumped:
            torch.mul(self.m_lumped, x, out=y)
        else:
            self.ev.effective_tangent(0.0, 0.0, self.m_node, None, x, y)
        return y

    def _tangent_and_inertia(self, cK, cM, x, y):
        """self.K <- cK K + cM M and y = M x: one pass over K (consistent mass)."""
        if self.lumped:
            if cK == 0.0:
                self.K.zero_()
            else:
                self.K.mul_(cK)
            self.K.index_add_(0, self._diag, self.m_lumped, alpha=cM)
            torch.mul(self.m_lumped, x, out=y)
        else:
            self.ev.effective_tangent(cK, cM, self.m_node, self.K, x, y)

    def linear_solve(self, b, x, rtol):
        """K x = b to |r| <= rtol |b| from x = 0; returns (iterations, relative residual)."""
        if self.linear_solver is not None:
            return self.linear_solver.solve(self.K, b, x, rtol, self.lin_max_iter)
        return self.ev.pcg_solve(self.K, b, x, rtol, self.lin_max_iter)

    # ------------------------------------------------------------------ initial state
    def initialize(self, u0=None, v0=None):
        """Sets d_0, v_0 and the consistent initial acceleration M a_0 = f_ext(0) - f_int(d_0) - C v_0
        (Dirichlet rows: unit rows, a = v = 0).  The CSR M of the solve is
        fcg_effective_tangent(cK = 0, cM = 1) into the K buffer.  Returns a_0."""
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.d = (torch.zeros(self.n, **f64) if u0 is None
                  else torch.as_tensor(u0, dtype=torch.float64).to(self.dev).clone())
        self.v = (torch.zeros(self.n, **f64) if v0 is None
                  else torch.as_tensor(v0, dtype=torch.float64).to(self.dev).clone())
        self.v[self._dbc64] = 0.0
        self.t, self.nstep, self.history = 0.0, 0, []
        self.ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, self.d, self.fint_n, self.K)
        self.fint.copy_(self.fint_n)
        self.fext_n = self.fext_at(0.0).clone()
        rhs = self.fext_n - self.fint_n
        if self.damp_k != 0.0:
            self.K0 = self.K.clone()
            self.ev.spmv(self.K0, self.v, self._y)
            rhs.sub_(self._y, alpha=self.damp_k)
        if self.damp_m != 0.0:
            rhs.sub_(self.mass_times(self.v, self._y), alpha=self.damp_m)
        if self.lumped:
            self.a = rhs / self.m_lumped
            self.a[self._dbc64] = 0.0
            self.init_lin = (0, 0.0)
        else:
            self.ev.effective_tangent(0.0, 1.0, self.m_node, self.K)
            self.ev.dirichlet_apply(self.dbc, self.K, rhs, None)
            self.a = torch.zeros(self.n, **f64)
            if float(torch.linalg.vector_norm(rhs)) > 0.0:
                self.init_lin = self.linear_solve(rhs, self.a, self.lin_rtol)
            else:
                self.init_lin = (0, 0.0)
            self.a[self._dbc64] = 0.0
        self._initialized = True
        return self.a

    # ------------------------------------------------------------------ one step
    def step(self):
        """Advances (d, v, a, t) by dt; appends a record to `history`; returns d_{n+1}."""
        if not self._initialized:
            self.initialize()
        am, af, beta, gamma, dt = self.alpha_m, self.alpha_f, self.beta, self.gamma, self.dt
        d_n, v_n, a_n = self.d, self.v, self.a
        fext_np1 = self.fext_at(self.t + dt)
        fext_mid = (1.0 - af) * fext_np1 + af * self.fext_n
        c_vd, c_vv, c_va = gamma / (beta * dt), (gamma - beta) / beta, (gamma - 2.0 * beta) / (2.0 * beta) * dt
        c_ad, c_av, c_aa = 1.0 / (beta * dt * dt), 1.0 / (beta * dt), (1.0 - 2.0 * beta) / (2.0 * beta)
        c_damp = (1.0 - af) * gamma / (beta * dt)
        cM = (1.0 - am) * c_ad + c_damp * self.damp_m
        cK = 1.0 - af
        d = d_n.clone()  # constant-displacement predictor
        rec = {"step": self.nstep + 1, "time": self.t + dt, "newton": []}
        ndu = float("inf")
        nr_old = lin_abs = None
        for it in range(self.max_iter + 1):
            self.ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, d, self.fint, self.K)
            inc = d - d_n
            v = c_vd * inc - c_vv * v_n - c_va * a_n
            a = c_ad * inc - c_av * v_n - c_aa * a_n
            v_mid = (1.0 - af) * v + af * v_n
            torch.add(am * a_n, a, alpha=1.0 - am, out=self._x)
            if self.damp_m != 0.0:
                self._x.add_(v_mid, alpha=self.damp_m)
            self._tangent_and_inertia(cK, cM, self._x, self._y)
            torch.add(self._y, self.fint, alpha=1.0 - af, out=self.r)
            self.r.add_(self.fint_n, alpha=af)
            self.r.sub_(fext_mid)
            if self.damp_k != 0.0:
                self.ev.spmv(self.K0, v_mid, self._y)
                self.r.add_(self._y, alpha=self.damp_k)
                self.K.add_(self.K0, alpha=c_damp * self.damp_k)
            self.ev.dirichlet_apply(self.dbc, self.K, self.r, self.freact)
            nr = float(torch.linalg.vector_norm(self.r))
            nrec = {"iter": it, "norm_res": nr, "norm_inc": ndu if it else None}
            if (it > 0 and nr <= self.tol_res and ndu <= self.tol_inc) or (nr == 0.0 and it > 0):
                rec["newton"].append(nrec)
                break
            if it == self.max_iter:
                rec["newton"].append(nrec)
                self.history.append(rec)
                raise RuntimeError(f"GenAlpha step {rec['step']}: Newton did not converge in "
                                   f"{self.max_iter} iterations: {rec['newton'][-3:]}")
            torch.neg(self.r, out=self.r)
            eta = self.forcing.compute(it, nr, nr_old, lin_abs)
            if nr > 0.0:
                lin_it, lin_res = accept_linear_solve(lambda: self.linear_solve(self.r, self.du, eta),
                                                      eta, it, self.rescue, nrec)
            else:
                self.du.zero_()
                lin_it, lin_res = 0, 0.0
            nr_old, lin_abs = nr, lin_res * nr
            nrec.update(lin_iter=lin_it, lin_relres=lin_res, eta=eta)
            rec["newton"].append(nrec)
            ndu = float(torch.linalg.vector_norm(self.du))
            d += self.du
        self.d, self.v, self.a = d, v, a
        self.fint_n.copy_(self.fint)
        self.fext_n = fext_np1.clone()
        self.t += dt
        self.nstep += 1
        rec.update(newton_iter=len(rec["newton"]) - 1, norm_res=rec["newton"][-1]["norm_res"],
                   norm_inc=rec["newton"][-1]["norm_inc"],
                   lin_iter=sum(r.get("lin_iter", 0) for r in rec["newton"]))
        self.history.append(rec)
        return self.d

    def energies(self):
        """(kinetic energy 1/2 v^T M v, None): the internal work is not tracked; the strain energy
        of the current state is internal_energy()."""
        y = self.mass_times(self.v, torch.empty_like(self.v))
        return 0.5 * float(torch.dot(self.v, y)), None

    def internal_energy(self):
        """The strain energy of the current displacement d: the sum of the elements'
        sum_g w_g det J_g psi(E_g) (4C's struct_calc_energy through fcg_gp_stress; single rank, so
        every column element is owned)."""
        return float(torch.sum(self.ev.strain_energy(self.d)))
