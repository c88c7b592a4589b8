"""``ivp_amd.Radau`` -- the direct per-method call ``RADAU::builder()...build().solve(..)`` (src/methods/radau.rs:19-127).

Radau IIA(5), the L-stable 3-stage order-5 implicit Runge-Kutta method, on the device for pure ODEs with up to 8 states
(identity mass matrix, strict arithmetic).  ``solve_ivp(..., Options(method="RADAU"))`` still answers
``IVP_ERR_UNSUPPORTED_METHOD``; this class is the way in, and it carries the struct fields ``solve_ivp`` cannot reach.
"""
from typing import Optional, Sequence

from . import _lib, api


class Radau:
    """The fields of ``struct RADAU`` that ``Options`` does not carry; ``rtol`` / ``atol`` / ``max_steps`` / ``t_eval`` /
    ``first_step`` / ``max_step`` / ``min_step`` / ``dense_output`` / ``max_log`` come from the ``Options`` given to
    ``solve`` / ``solve_batch`` (its ``method`` is ignored; ``max_steps=None`` means unlimited, as in ``solve_ivp``)."""

    def __init__(self, newton_maxiter: int = 7, newton_tol: Optional[float] = None, predictive: bool = True,
                 uround: float = 2.3e-16, safety_factor: float = 0.9, scale_min: float = 0.2, scale_max: float = 8.0):
        self.newton_maxiter = int(newton_maxiter)
        self.newton_tol = None if newton_tol is None else float(newton_tol)
        self.predictive = bool(predictive)
        self.uround = float(uround)
        self.safety_factor = float(safety_factor)
        self.scale_min = float(scale_min)
        self.scale_max = float(scale_max)

    def _c(self) -> _lib.RadauSettingsT:
        s = _lib.RadauSettingsT()
        s.uround, s.safety_factor, s.scale_min, s.scale_max = self.uround, self.safety_factor, self.scale_min, self.scale_max
        s.newton_maxiter = self.newton_maxiter
        s.has_newton_tol = 0 if self.newton_tol is None else 1
        s.newton_tol = 0.0 if self.newton_tol is None else self.newton_tol
        s.predictive = 1 if self.predictive else 0
        return s

    def solve(self, f: api.IVP, t0: float, t1: float, y0: Sequence[float], options: api.Options = None,
              ctx: api.Context = None) -> api.Solution:
        """One trajectory; the ``Solution`` that ``DefaultSolOut`` records (every accepted step, or the ``t_eval`` samples)."""
        return api.solve_ivp(f, t0, t1, y0, options, ctx, _radau=self._c())

    def solve_batch(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None, ctx: api.Context = None,
                    out: api.BatchSolution = None) -> api.BatchSolution:
        """B independent ``solve`` calls; host (numpy) or device (torch) arrays, like ``solve_ivp_batch``."""
        return api.solve_ivp_batch(f, t0, t1, y0, params, options, ctx, out=out, _radau=self._c())
