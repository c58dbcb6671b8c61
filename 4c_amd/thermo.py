"""Transient heat conduction with every vector and matrix resident in HBM: 4C's THERMAL DYNAMIC /
DYNAMICTYPE OneStepTheta (Thermo::TimIntOneStepTheta) around the thermo context's evaluate
(FCG_TSI_THERMO_FINTCOND with v = 0), its capacity matrix (fcg_tsi_capacity) and the one-step-theta
pass (fcg_tsi_ost_combine).

Per time step, with h = (1 - theta)(f_int,n - f_ext,n) - theta f_ext,n+1 formed once, the Newton loop of
tsi.TsiMonolithic's shape: evaluate K_TT and f_T at T_{n+1}, combine them to the tangent
C/dt + theta K_TT and the residual r = C (T_{n+1} - T_n)/dt + theta f_T + h, b = -r, Dirichlet rows
(unit rows, b = 0: prescribed temperatures keep their T_init values), solve, T += dT; stop when
|dT| <= tol_inc max(1, |T|).  After the step f_int,n becomes f_T at the accepted state.

Heat convection on surfaces (fcg.TsiSurface, 4C's Thermo::TimInt::apply_force_external_conv) is part
of the internal force: one pass per surface right after every evaluate adds s_c(t) (A T - s_t(t) g)
to f_T and s_c(t) A to K_TT, so theta weighs it with the rest and f_int,n carries the old one."""

import ctypes

import numpy as np
import torch

from . import fcg


class ScalarCsr:
    """The k_TT graph of a single-rank TsiEvaluator on the device, for the library's scalar CSR
    product (fcg_scsr_spmv) on any value array of that graph."""

    def __init__(self, tev):
        g = tev.graph
        self.device = tev.device
        dev = torch.device("cuda", tev.device)
        self.n = int(g.n_rows_t)
        self.width = int(np.diff(g.rowptr_tt).max(initial=0))
        self.ptr = torch.as_tensor(np.ascontiguousarray(g.rowptr_tt, dtype=np.int64)).to(dev)
        self.col = torch.as_tensor(np.ascontiguousarray(g.col_tt, dtype=np.int32)).to(dev)

    def spmv(self, vals, x, y):
        """y = A x (asynchronous on torch's current stream)."""
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = fcg.lib().fcg_scsr_spmv(self.device, self.n, self.width, p(self.ptr), p(self.col), p(vals),
                                     p(x), None, p(y), 1.0, 0, fcg._torch_stream(None, self.device))
        if rc != 0:
            raise fcg.FcgError(rc, "fcg_scsr_spmv failed")
        return y


def jacobi_cg(csr, vals, b, x, rtol, max_iter):
    """A x = b from x = 0 by conjugate gradients with the diagonal as preconditioner, the products
    by fcg_scsr_spmv: the solve of the effective thermal tangent when no ScalarAMG is given.  Unit
    Dirichlet rows with b = 0 there keep the iteration in the free rows, where A is symmetric
    positive definite.  -> (steps, true relative residual)."""
    rows = torch.repeat_interleave(torch.arange(csr.n, device=b.device), csr.ptr[1:] - csr.ptr[:-1])
    diag = torch.zeros_like(b)
    on = csr.col.long() == rows
    diag[rows[on]] = vals[on]
    x.zero_()
    nb = torch.linalg.vector_norm(b).item()
    if nb == 0.0:
        return 0, 0.0
    r, q = b.clone(), torch.empty_like(b)
    z = r / diag
    p = z.clone()
    rz = r.dot(z).item()
    it = 0
    while it < max_iter:
        csr.spmv(vals, p, q)
        alpha = rz / p.dot(q).item()
        x.add_(p, alpha=alpha)
        r.sub_(q, alpha=alpha)
        it += 1
        if torch.linalg.vector_norm(r).item() <= rtol * nb:
            # the recurrence's residual drifts from the true one: restart from b - A x
            torch.sub(b, csr.spmv(vals, x, q), out=r)
            if torch.linalg.vector_norm(r).item() <= rtol * nb:
                break
            z = r / diag
            p.copy_(z)
            rz = r.dot(z).item()
            continue
        z = r / diag
        rz1 = r.dot(z).item()
        p.mul_(rz1 / rz).add_(z)
        rz = rz1
    torch.sub(b, csr.spmv(vals, x, q), out=r)
    return it, torch.linalg.vector_norm(r).item() / nb


def convection_list(convection):
    """The drivers' `convection` argument as a list of (surface, coeff_funct, surtemp_funct): a
    fcg.TsiSurface, a tuple (surface, coeff_funct, surtemp_funct) whose functs are callables t -> scale
    or None (scale 1), or a list of these; None: no surface."""
    if convection is None:
        return []
    if isinstance(convection, (fcg.TsiSurface, tuple)):
        convection = [convection]
    out = []
    for c in convection:
        surface, fc, ft = c if isinstance(c, tuple) else (c, None, None)
        if not isinstance(surface, fcg.TsiSurface):
            raise TypeError("convection: a TsiSurface or (TsiSurface, coeff_funct, surtemp_funct)")
        out.append((surface, fc, ft))
    return out


def apply_convection(conv, t, T, fT=None, Ktt=None):
    """Every surface of convection_list's `conv` with the scales of time t onto fT and Ktt."""
    for surface, fc, ft in conv:
        surface.convection(T, fT=fT, Ktt=Ktt, coeff_scale=1.0 if fc is None else float(fc(t)),
                           surtemp_scale=1.0 if ft is None else float(ft(t)))


class OneStepTheta:
    """tsi_ev: the TsiEvaluator of one single-rank mesh with node-consistent thermo numbering.
    capa: MAT_Fourier CAPA (ele_capa: one value per element instead).  fext_t: a row vector
    (tensor or array) or a callable t -> vector.  dbc_t: Dirichlet row LIDs, whose temperatures
    keep their T_init values.  amg_t: an amg.ScalarAMG of tsi_ev (set up on every tangent); None:
    Jacobi-preconditioned conjugate gradients on the library's scalar CSR product.  convection:
    surfaces with a set convection condition (convection_list), applied after every evaluate with
    the scales of the evaluate's time.

    step() advances one time step, run(nstep) several; `history` holds per step the Newton
    iterations and per solve the linear iterations and relative residual (the keys of
    tsi.TsiMonolithic).  Raises RuntimeError when Newton or a linear solve misses its tolerance."""

    def __init__(self, tsi_ev, capa, dt, theta, fext_t, dbc_t, T_init, amg_t=None, tol_inc=1e-13,
                 max_iter=30, lin_rtol=1e-10, lin_max_iter=2000, ele_capa=None, convection=None):
        g = tsi_ev.graph
        if g.n_rows_t != g.n_cols_t:
            raise ValueError("OneStepTheta: single-rank thermo contexts only")
        self.tev, self.dt, self.theta = tsi_ev, float(dt), float(theta)
        self.dev = torch.device("cuda", tsi_ev.device)
        self.nt = int(g.n_rows_t)
        self.fext_t = fext_t
        self.dbc_t = torch.as_tensor(dbc_t).to(device=self.dev, dtype=torch.int32).contiguous()
        self.amg_t = amg_t
        if amg_t is not None:
            amg_t.check_dirichlet(self.dbc_t.cpu().numpy())
        self.conv = convection_list(convection)
        self.tol_inc, self.max_iter = float(tol_inc), int(max_iter)
        self.lin_rtol, self.lin_max_iter = float(lin_rtol), int(lin_max_iter)
        z = lambda n: torch.zeros(int(n), dtype=torch.float64, device=self.dev)
        self.csr = ScalarCsr(tsi_ev)
        self.C = tsi_ev.capacity(capa, ele_capa)
        self.v = z(tsi_ev.mesh.n_cols)  # the structure is at rest
        self.T = self._vec(T_init).clone()
        self.Tn, self.fT, self.h, self.dx = z(self.nt), z(self.nt), z(self.nt), z(self.nt)
        self.Ktt = z(g.nnz_tt)
        self.step_no, self.t = 0, 0.0
        self.history = []
        # start-up: f_int,0 = f_T(T_0), f_ext,0 = fext(0)
        self._fintcond()
        self.fint_n = self.fT.clone()
        self.fext_n = self._load(0.0).clone()

    def _vec(self, a):
        return torch.as_tensor(a).to(device=self.dev, dtype=torch.float64).contiguous()

    def _load(self, t):
        return self._vec(self.fext_t(t) if callable(self.fext_t) else self.fext_t)

    def _fintcond(self):
        self.tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, self.v, self.T, fT=self.fT,
                                 Ktt=self.Ktt)
        apply_convection(self.conv, self.t, self.T, fT=self.fT, Ktt=self.Ktt)

    def heat_content(self):
        """1^T C T, the heat the body holds."""
        return self.csr.spmv(self.C, self.T, self.dx).sum().item()

    def step(self):
        self.step_no += 1
        self.t = self.step_no * self.dt
        th = self.theta
        fe1 = self._load(self.t)
        torch.sub(self.fint_n, self.fext_n, out=self.h)
        self.h.mul_(1.0 - th).sub_(fe1, alpha=th)
        self.Tn.copy_(self.T)
        rec = {"step": self.step_no, "iterations": 0, "gmres_iterations": [], "gmres_rel_residual": []}
        for it in range(self.max_iter):
            self._fintcond()
            self.tev.ost_combine(th, self.dt, self.C, self.T, self.Tn, h=self.h, Ktt=self.Ktt, fT=self.fT)
            self.fT.neg_()  # b = -r, zero on the Dirichlet rows
            self.tev.dirichlet_apply(rows_t=self.dbc_t, Ktt=self.Ktt, rhs_T=self.fT)
            if self.amg_t is not None:
                n, rel = self.amg_t.solve(self.Ktt, self.fT, self.dx, self.lin_rtol, self.lin_max_iter)
            else:
                n, rel = jacobi_cg(self.csr, self.Ktt, self.fT, self.dx, self.lin_rtol, self.lin_max_iter)
            rec["gmres_iterations"].append(n)
            rec["gmres_rel_residual"].append(rel)
            if not rel <= self.lin_rtol:
                self.history.append(rec)
                raise RuntimeError(f"thermo step {self.step_no}: the linear solve stopped at relative "
                                   f"residual {rel:.3e} > {self.lin_rtol:.1e} after {n} iterations")
            self.T.add_(self.dx)
            rec["iterations"] = it + 1
            ninc = torch.linalg.vector_norm(self.dx).item()
            if ninc <= self.tol_inc * max(1.0, torch.linalg.vector_norm(self.T).item()):
                break
        else:
            self.history.append(rec)
            raise RuntimeError(f"thermo Newton did not converge in step {self.step_no}")
        self._fintcond()
        self.fint_n.copy_(self.fT)
        self.fext_n = fe1.clone()
        self.history.append(rec)
        return rec

    def run(self, nstep):
        for _ in range(int(nstep)):
            self.step()
        return self.T
