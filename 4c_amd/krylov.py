"""Restarted flexible GMRES (fcg_gmres_solve, csrc/fcg_krylov.hip) as a linear solver object: the
solver for tangents that are not symmetric, with the protocol of amg.NativeAMG, so
newton.StaticNewton(linear_solver=...) and dynamics.GenAlpha accept it unchanged."""

from . import fcg  # noqa: F401  (loads the library)


class Gmres:
    """solve(K, b, x, rtol, max_iter) -> (inner steps taken, true relative residual) on the
    Evaluator `ev` (a single-rank context).  restart: inner steps per cycle, 1..128.  amg: an
    amg.NativeAMG of the same context as preconditioner (its numeric setup is run on every K
    handed to solve, as NativeAMG.solve does); None: the 3 x 3 nodal block Jacobi."""

    def __init__(self, ev, restart=50, amg=None):
        self.ev, self.restart, self.amg = ev, int(restart), amg
        self.history = []

    def check_dirichlet(self, dbc_rows):
        if self.amg is not None:
            self.amg.check_dirichlet(dbc_rows)

    def solve(self, K, b, x, rtol, max_iter=10000, setup=True):
        if self.amg is not None and setup:
            self.amg.setup(K)
        it, rel = self.ev.gmres_solve(K, b, x, rtol=rtol, max_iter=max_iter, restart=self.restart,
                                      amg=self.amg)
        self.history.append((it, rel))
        return it, rel
