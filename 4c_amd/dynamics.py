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


class CentralDifference:
    """4C's explicit central-difference integrator (DYNAMICTYPE CentrDiff,
    4C_structure_new_expl_centrdiff.cpp) with the row-sum lumped mass: per step one
    fcg_evaluate_device (CALC_INTERNALFORCE, OVERWRITE) and one fcg_centrdiff_step, no linear
    solve.  The update after an evaluate and the one before the next are fused, so the state
    leapfrogs: after initialize() and n steps

      v, a   = v_n, a_n            at t = t_n
      vhalf  = v_{n+1/2}
      d      = d_{n+1}             the displacement the next step evaluates; displacement() gives d_n

    with, per free row (fcg_centrdiff_step; Dirichlet rows keep d and have v = a = 0),
      a_n = (f_ext(t_n) - f_int(d_n)) / m - damping_m v_{n-1/2}
      v_n = v_{n-1/2} + dt_{n-1}/2 a_n,  v_{n+1/2} = v_n + dt_n/2 a_n,  d_{n+1} = d_n + dt_n v_{n+1/2}
    dt may be changed between steps (the attribute `dt` is the next drift's step).  The scheme is
    stable for dt < 2 / omega_max; stable_dt() returns a step that is never above that limit.

    Single rank, homogeneous-in-time Dirichlet conditions; d, vhalf, v, a, f_int and the kinetic
    energy stay in HBM, t and nstep are host numbers (they need no device work).  All launches go
    to torch's current stream of the evaluator's device."""

    def __init__(self, evaluator, density, dt, fext, dbc_rows, damping_m=0.0, ele_density=None):
        """fext: a row vector (constant load) or a callable t -> row vector (numpy or device
        tensor).  damping_m: mass-proportional damping C = damping_m M, taken at the half-step
        velocity.  density / ele_density: as Evaluator.mass_nodal."""
        info = evaluator.info
        self.ev = evaluator
        self.dev = torch.device("cuda", evaluator.device)
        self.n = int(info.n_rows)
        if int(info.n_cols) != self.n:
            raise ValueError("CentralDifference is single-rank: the column map must be the row map")
        self.nnz = int(info.nnz)
        self.dt = float(dt)
        if not self.dt > 0.0:
            raise ValueError("dt must be positive")
        self.damp_m = float(damping_m)
        if not self.damp_m >= 0.0:
            raise ValueError("damping_m must not be negative")
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.m_lumped = torch.empty(self.n, **f64)
        evaluator.mass_nodal(density, ele_density, None, self.m_lumped)
        if self.n and not float(self.m_lumped.min()) > 0.0:
            raise ValueError("the lumped mass is not positive on every row")
        dbc = np.unique(np.asarray(dbc_rows, dtype=np.int64))
        if len(dbc) and (dbc[0] < 0 or dbc[-1] >= self.n):
            raise ValueError("a Dirichlet row lies outside the row map")
        fixed = np.zeros(self.n, dtype=np.uint8)
        fixed[dbc] = 1
        self.fixed = torch.as_tensor(fixed).to(self.dev)
        self._fext = fext
        self._fext_const = None if callable(fext) else self._as_row(fext).clone()
        self.d = torch.zeros(self.n, **f64)
        self.vhalf = torch.zeros(self.n, **f64)
        self.v = torch.zeros(self.n, **f64)
        self.a = torch.zeros(self.n, **f64)
        self.fint = torch.zeros(self.n, **f64)
        self.ekin = torch.zeros(1, **f64)
        self.t = 0.0
        self.nstep = 0
        self._dt_last = 0.0  # the step of the drift that produced d
        self._initialized = False

    # ------------------------------------------------------------------ pieces
    def _as_row(self, f):
        if not torch.is_tensor(f):
            f = torch.as_tensor(np.asarray(f, dtype=np.float64))
        f = f.to(device=self.dev, dtype=torch.float64)
        if f.numel() != self.n:
            raise ValueError(f"fext has {f.numel()} entries, the context {self.n} rows")
        return f

    def fext_at(self, t):
        return self._fext_const if self._fext_const is not None else self._as_row(self._fext(t))

    def _advance(self, t_eval, dt_prev):
        """f_int(d), then the fused update with f_ext(t_eval): d is the displacement at t_eval."""
        fext = self.fext_at(t_eval)
        self.ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, self.d, self.fint)
        self.ev.centrdiff_step(dt_prev, self.dt, self.damp_m, fext, self.fint, self.m_lumped,
                               self.fixed, self.d, self.vhalf, self.v, self.a, self.ekin)
        self._dt_last = self.dt

    # ------------------------------------------------------------------ the integration
    def initialize(self, u0=None, v0=None):
        """Sets d_0 and v_0, forms a_0 = (f_ext(0) - f_int(d_0)) / m - damping_m v_0 and takes the
        first half kick and drift (dt_prev = 0).  Returns a_0."""
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.d = (torch.zeros(self.n, **f64) if u0 is None
                  else torch.as_tensor(u0, dtype=torch.float64).to(self.dev).clone())
        self.vhalf = (torch.zeros(self.n, **f64) if v0 is None
                      else torch.as_tensor(v0, dtype=torch.float64).to(self.dev).clone())
        self.t, self.nstep = 0.0, 0
        self._advance(0.0, 0.0)
        self._initialized = True
        return self.a

    def step(self):
        """One evaluate at d_{n+1} and one fused update: (v, a, t) advance to t_{n+1}, d to
        d_{n+2}.  Returns d."""
        if not self._initialized:
            self.initialize()
        t_new = self.t + self._dt_last
        self._advance(t_new, self._dt_last)
        self.t = t_new
        self.nstep += 1
        return self.d

    def run(self, n_steps, check_every=100):
        """n_steps steps.  With a constant fext the evaluator is switched to set_async(1) and the
        steps are queued without any host synchronisation; check_error() runs every check_every
        steps and at the end, and an element error (4C's throws) surfaces as FcgError with the
        step range in which it happened -- the state tensors are then not usable.  A callable fext
        is evaluated on the host per step, in the evaluator's own mode.  The evaluator's async
        setting is restored on every exit path.  Returns d."""
        check_every = max(1, int(check_every))
        prev = self.ev.async_enabled
        failed = False
        try:
            if self._fext_const is not None:
                self.ev.set_async(1)
            lo = self.nstep + 1
            try:
                if not self._initialized:
                    lo = 0  # step 0: the evaluate of initialize()
                    self.initialize()
                for k in range(int(n_steps)):
                    self.step()
                    if (k + 1) % check_every == 0:
                        self.ev.check_error()
                        lo = self.nstep + 1
                self.ev.check_error()
            except fcg.FcgError as e:
                msg = str(e).split(": ", 1)[-1]
                raise fcg.FcgError(e.code, f"CentralDifference.run, steps {lo}..{max(lo, self.nstep)}: "
                                   f"{msg}", e.bad_ele_gid) from e
        except BaseException:
            failed = True
            raise
        finally:
            try:
                self.ev.set_async(prev)
            except fcg.FcgError:
                # leaving async mode reports what was still pending; the context is synchronous now
                if prev:
                    self.ev.set_async(1)
                if not failed:
                    raise
        return self.d

    # ------------------------------------------------------------------ output
    def displacement(self):
        """d_n, the displacement at the time t of v and a: d - dt vhalf (a new tensor)."""
        return torch.add(self.d, self.vhalf, alpha=-self._dt_last)

    def energies(self):
        """(kinetic energy 1/2 v^T M v at t, None), the kinetic part from fcg_centrdiff_step's
        fixed-order sum; the strain energy is internal_energy()."""
        return float(self.ekin), None

    def internal_energy(self):
        """The strain energy of displacement(): the sum of the elements' sum_g w_g det J_g psi(E_g)
        (fcg_gp_stress; single rank, so every column element is owned)."""
        return float(torch.sum(self.ev.strain_energy(self.displacement())))

    def stable_dt(self, safety=1.0):
        """safety x the Gershgorin bound 2 / sqrt(max_i sum_j |K_ij| / m_i) of fcg_stable_dt on the
        free rows, with K assembled at the current d into a buffer that lives only for this call.
        Never above the central-difference limit 2 / omega_max of K(d)."""
        f64 = dict(dtype=torch.float64, device=self.dev)
        K = torch.empty(self.nnz, **f64)
        f = torch.empty(self.n, **f64)
        self.ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, self.d, f, K)
        dt_crit, _ = self.ev.stable_dt(K, self.m_lumped, self.fixed)
        return float(safety) * dt_crit
