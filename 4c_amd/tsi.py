"""Monolithic thermo-structure interaction (static, or with a transient thermal field) with every
vector and matrix resident in HBM:
the Newton loop of TSI::Monolithic (4C_tsi_monolithic.cpp: newton_full, setup_system_matrix,
linear_solve) around the library's TSI evaluates, Dirichlet applies and the FGMRES solve of the
non-symmetric block system [[K_SS, K_ST], [K_TS, K_TT]] (fcg_tsi_gmres_solve).

By default both fields are statics with linear kinematics (what fcg_tsi_evaluate_* covers): per
time step the loads are taken at t_{n+1}; per Newton iteration the velocity of the quasi-static structure is
v = (d - d_n) / dt (TSI::Algorithm::calc_velocity), the blocks are evaluated with timefac 1 and
timefac_d 1 / dt, r = f_int - f_ext, the Dirichlet rows are applied to all four blocks and both
residuals, the increment solves K dx = -r and x += dx.  The iteration stops when
|dx| <= tol_inc max(1, |x|) on the stacked vector.

thermal="ost": the thermal field is transient (THERMAL DYNAMIC / DYNAMICTYPE OneStepTheta beside the
quasi-static structure at t_{n+1}).  The evaluates run with timefac theta and timefac_d 1 / dt, so K_TS
arrives theta-weighted; fcg_tsi_ost_combine turns K_TT into C/dt + theta K_TT and f_T into
C (T - T_n)/dt + theta f_T + h with h = (1 - theta)(f_int,n - f_ext,n) - theta f_ext,n+1 formed once per
step (thermo.OneStepTheta; f_int,0 is evaluated at (T_0, v = 0), f_int,n after every step at the
accepted state).  K_ST, K_SS and f_S are those of the static case.

Heat convection on surfaces (fcg.TsiSurface) is a separate pass after either evaluate path: it adds
s_c(t) (A T - s_t(t) g) to f_T and s_c(t) A to K_TT before the combine, and to f_int,n."""

import torch

from . import fcg
from .thermo import apply_convection, convection_list


class TsiMonolithic:
    """struct_ev / tsi_ev: the structural Evaluator (linear kinematics, StVK with the TSI
    material's E and nu) and the TsiEvaluator of one single-rank mesh with node-consistent thermo
    numbering.  fext_s / fext_t: row vectors (tensors or arrays) or callables t -> vector.
    dbc_s / dbc_t: homogeneous Dirichlet row LIDs of the two fields.  fused: one
    fcg_tsi_evaluate_fused per iteration (True), two evaluates (False), or fused when the contexts
    qualify (None).  precond: "bgs" or "diag"; amg: an amg.NativeAMG of struct_ev for the
    structural block (set up on every K_SS), None: nodal block Jacobi; amg_t: an amg.ScalarAMG of
    tsi_ev for the thermal block (set up on every K_TT), None: the diagonal of K_TT.  convection:
    surfaces with a set convection condition (thermo.convection_list's forms).

    step() advances one time step, run(nstep) several; `history` holds per step the Newton
    iterations and per solve the GMRES iterations and relative residual.  Raises RuntimeError when
    Newton or a linear solve misses its tolerance."""

    def __init__(self, struct_ev, tsi_ev, dt, fext_s, fext_t, dbc_s, dbc_t, T_init=None, fused=None,
                 tol_inc=1e-13, max_iter=30, lin_rtol=1e-10, restart=50, lin_max_iter=2000,
                 precond="bgs", amg=None, amg_t=None, thermal="statics", capa=None, theta=1.0,
                 convection=None):
        self.sev, self.tev, self.dt = struct_ev, tsi_ev, float(dt)
        self.dev = torch.device("cuda", struct_ev.device)
        g = tsi_ev.graph
        self.ns, self.nt = int(struct_ev.info.n_rows), int(g.n_rows_t)
        self.fext_s, self.fext_t = fext_s, fext_t
        i32 = lambda a: torch.as_tensor(a).to(device=self.dev, dtype=torch.int32).contiguous()
        self.dbc_s, self.dbc_t = i32(dbc_s), i32(dbc_t)
        self.fused = fused
        self.tol_inc, self.max_iter = float(tol_inc), int(max_iter)
        self.lin_rtol, self.restart, self.lin_max_iter = float(lin_rtol), int(restart), int(lin_max_iter)
        self.precond, self.amg = precond, amg
        if amg is not None:
            amg.check_dirichlet(self.dbc_s.cpu().numpy())
        self.amg_t = amg_t
        if amg_t is not None:
            amg_t.check_dirichlet(self.dbc_t.cpu().numpy())
        z = lambda n: torch.zeros(int(n), dtype=torch.float64, device=self.dev)
        self.d, self.T = z(self.ns), z(self.nt)
        if T_init is not None:
            self.T.copy_(self._vec(T_init))
        self.d_n, self.v = z(self.ns), z(self.ns)
        self.fs, self.fT = z(self.ns), z(self.nt)
        self.dxs, self.dxt = z(self.ns), z(self.nt)
        self.Kss, self.Kst = z(struct_ev.info.nnz), z(g.nnz_st)
        self.Kts, self.Ktt = z(g.nnz_ts), z(g.nnz_tt)
        self.step_no, self.t = 0, 0.0
        self.history = []
        self.conv = convection_list(convection)
        if thermal not in ("statics", "ost"):
            raise ValueError('TsiMonolithic: thermal is "statics" or "ost"')
        self.ost = thermal == "ost"
        self.timefac = 1.0
        if self.ost:
            if capa is None:
                raise ValueError('TsiMonolithic: thermal="ost" needs the heat capacity capa')
            self.theta = self.timefac = float(theta)
            self.C = tsi_ev.capacity(capa)
            self.T_n, self.h = z(self.nt), z(self.nt)
            self.fint_n = z(self.nt)
            self._fint_n()  # at (T_0, v = 0)
            self.fext_n = self._load(self.fext_t, 0.0).clone()

    def _vec(self, a):
        return torch.as_tensor(a).to(device=self.dev, dtype=torch.float64).contiguous()

    def _load(self, f, t):
        return self._vec(f(t) if callable(f) else f)

    def _fint_n(self):
        """f_int,n = f_T at the current (v, T); K_TT is scratch here, every iteration overwrites it."""
        self.tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, self.v, self.T, fT=self.fint_n,
                                 Ktt=self.Ktt)
        apply_convection(self.conv, self.t, self.T, fT=self.fint_n)

    def _evaluate(self):
        if self.fused is not False:
            try:
                self.tev.evaluate_fused(self.sev, fcg.OVERWRITE, self.d, self.v, self.T, self.timefac,
                                        1.0 / self.dt, fs=self.fs, Kss=self.Kss, Kst=self.Kst,
                                        fT=self.fT, Ktt=self.Ktt, Kts=self.Kts)
                self.fused = True
                return
            except fcg.FcgError as e:
                if self.fused is True or e.code != 3:
                    raise
                self.fused = False  # the contexts do not qualify: two evaluates from now on
        self.sev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, self.d, self.fs, self.Kss)
        self.tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, self.v, self.T, self.timefac, 1.0 / self.dt,
                                 fs=self.fs, Kst=self.Kst, fT=self.fT, Ktt=self.Ktt, Kts=self.Kts)

    def step(self):
        self.step_no += 1
        self.t = self.step_no * self.dt
        fes, fet = self._load(self.fext_s, self.t), self._load(self.fext_t, self.t)
        self.d_n.copy_(self.d)
        if self.ost:
            torch.sub(self.fint_n, self.fext_n, out=self.h)
            self.h.mul_(1.0 - self.theta).sub_(fet, alpha=self.theta)
            self.T_n.copy_(self.T)
        rec = {"step": self.step_no, "iterations": 0, "gmres_iterations": [], "gmres_rel_residual": []}
        for it in range(self.max_iter):
            torch.sub(self.d, self.d_n, out=self.v)
            self.v.div_(self.dt)
            self._evaluate()
            apply_convection(self.conv, self.t, self.T, fT=self.fT, Ktt=self.Ktt)
            # b = -(f_int - f_ext), zero on the Dirichlet rows
            self.fs.sub_(fes).neg_()
            if self.ost:
                self.tev.ost_combine(self.theta, self.dt, self.C, self.T, self.T_n, h=self.h, Ktt=self.Ktt,
                                     fT=self.fT)
                self.fT.neg_()
            else:
                self.fT.sub_(fet).neg_()
            self.sev.dirichlet_apply(self.dbc_s, self.Kss, self.fs)
            self.tev.dirichlet_apply(self.dbc_s, self.dbc_t, self.Kst, self.Kts, self.Ktt, self.fT)
            if self.amg is not None:
                self.amg.setup(self.Kss)
            if self.amg_t is not None:
                self.amg_t.setup(self.Ktt)
            n, rel = self.tev.gmres_solve(self.sev, self.Kss, self.Kst, self.Kts, self.Ktt, self.fs,
                                          self.fT, self.dxs, self.dxt, rtol=self.lin_rtol,
                                          max_iter=self.lin_max_iter, restart=self.restart,
                                          precond=self.precond, amg=self.amg, amg_t=self.amg_t)
            rec["gmres_iterations"].append(n)
            rec["gmres_rel_residual"].append(rel)
            if not rel <= self.lin_rtol:
                self.history.append(rec)
                raise RuntimeError(f"TSI step {self.step_no}: GMRES stopped at relative residual "
                                   f"{rel:.3e} > {self.lin_rtol:.1e} after {n} iterations")
            self.d.add_(self.dxs)
            self.T.add_(self.dxt)
            rec["iterations"] = it + 1
            ninc = torch.sqrt(self.dxs.dot(self.dxs) + self.dxt.dot(self.dxt)).item()
            nx = torch.sqrt(self.d.dot(self.d) + self.T.dot(self.T)).item()
            if ninc <= self.tol_inc * max(1.0, nx):
                break
        else:
            self.history.append(rec)
            raise RuntimeError(f"TSI Newton did not converge in step {self.step_no}")
        if self.ost:
            torch.sub(self.d, self.d_n, out=self.v)
            self.v.div_(self.dt)
            self._fint_n()
            self.fext_n = fet.clone()
        self.history.append(rec)
        return rec

    def run(self, nstep):
        for _ in range(int(nstep)):
            self.step()
        return self.d, self.T
