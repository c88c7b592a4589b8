"""``ivp_amd.Radau`` -- the direct per-method call ``RADAU::builder()...build().solve(..)`` (src/methods/radau.rs:19-127).

Radau IIA(5), the L-stable 3-stage order-5 implicit Runge-Kutta method, on the device (strict arithmetic): pure ODEs with
up to 512 states -- beyond 8 a ``DeviceIVP`` in component form (``ode_comp``, optional ``jac_col``) or ``Dense64()``: up to 64 states one matrix row per lane with the factors in LDS, from 65 to 512 (compiled
problems only) several rows per lane with J and the three factors in global memory, 4 n^2 doubles per trajectory (8 MB at
n = 512: an allocation that fails is ``HipError``) -- and ``M y' = f(t, y)`` with a
constant, possibly singular mass matrix -- a ``DeviceIVP(..., mass=True)`` for up to 8 states, ``mass_col=True`` (the
component form's column hook) from 9 to 64 -- and index-1/2/3 algebraic variables (``nind1`` / ``nind2`` / ``nind3``).
``solve_ivp(..., Options(method="RADAU"))`` still answers ``IVP_ERR_UNSUPPORTED_METHOD``; this class is the way in, and it
carries the struct fields ``solve_ivp`` cannot reach.  Besides the blocking ``solve`` / ``solve_batch`` (bounded ``max_log``
logs) it has the forms the other methods have for batches whose step counts are not known in advance:
``solve_batch(..., wait=False)`` (a ``PendingBatch``; ``BatchPipeline.map(..., radau=...)`` overlaps several),
``solve_batch_logged`` (every accepted step, CSR, one integration) and ``solve_batch_dense`` (every segment, CSR, evaluated on
the device).  Event functions have ONE way in, ``solve_batch_events``: every occurrence of every event as a CSR log, with
everything a plain solve returns beside it (thread form up to 8 states, mass matrix included; component form without a mass
hook up to 64).  Not there: events through the other Radau calls (``solve``, ``solve_batch``, ``solve_batch_logged``,
``solve_batch_dense`` still refuse a problem with event functions), events beyond n = 64, the multi-GPU entry points.

A banded Jacobian has ONE way in as well, ``solve_batch_banded`` / ``solve_banded``: a ``DeviceIVP(..., jac_sparsity=S,
jac_storage="banded")`` (8 < n <= 512, pure ODE, no event functions) keeps J and the three factors by bands -- (WJ + 3 W) n
doubles per trajectory with WJ = ml + mu + 1 and W = 2 ml + mu + 1, 15 n for a tridiagonal system instead of 4 n^2 --
forms J by grouped differences and factorises inside the band.  For a finite
right-hand side and a pattern that holds every structurally non-zero entry the results equal ``solve_batch`` on the same
source compiled without a pattern bit for bit.  Every other call above keeps refusing such a problem, and a pattern without
band storage is refused by all of them.  Not there: the resumable, logged and CSR dense forms, events, mass matrices and
index sets in band storage.
"""
from typing import Optional, Sequence

from . import _lib, api


class Radau:
    """The fields of ``struct RADAU`` that ``Options`` does not carry; ``rtol`` / ``atol`` / ``max_steps`` / ``t_eval`` /
    ``first_step`` / ``max_step`` / ``min_step`` / ``dense_output`` / ``max_log`` come from the ``Options`` given to
    ``solve`` / ``solve_batch`` (its ``method`` is ignored; ``max_steps=None`` means unlimited, as in ``solve_ivp``).
    ``nind1`` / ``nind2`` / ``nind3``: the counts of index-1, index-2 and index-3 variables, in that order in the state
    (radau.rs:210-246: all ``None`` = a pure ODE partition; ``nind1`` omitted = inferred; else they must sum to n, or
    ``ConfigError`` with code -7).  Index-2 / index-3 variables need a problem with a mass matrix."""

    def __init__(self, newton_maxiter: int = 7, newton_tol: Optional[float] = None, predictive: bool = True,
                 uround: float = 2.3e-16, safety_factor: float = 0.9, scale_min: float = 0.2, scale_max: float = 8.0,
                 nind1: Optional[int] = None, nind2: Optional[int] = None, nind3: Optional[int] = None):
        self.newton_maxiter = int(newton_maxiter)
        self.newton_tol = None if newton_tol is None else float(newton_tol)
        self.predictive = bool(predictive)
        self.uround = float(uround)
        self.safety_factor = float(safety_factor)
        self.scale_min = float(scale_min)
        self.scale_max = float(scale_max)
        self.nind1 = None if nind1 is None else int(nind1)
        self.nind2 = None if nind2 is None else int(nind2)
        self.nind3 = None if nind3 is None else int(nind3)

    def _c(self) -> _lib.RadauSettingsT:
        s = _lib.RadauSettingsT()
        s.uround, s.safety_factor, s.scale_min, s.scale_max = self.uround, self.safety_factor, self.scale_min, self.scale_max
        s.newton_maxiter = self.newton_maxiter
        s.has_newton_tol = 0 if self.newton_tol is None else 1
        s.newton_tol = 0.0 if self.newton_tol is None else self.newton_tol
        s.predictive = 1 if self.predictive else 0
        return s

    def _dae(self, f: api.IVP = None) -> Optional[_lib.RadauDaeT]:
        """The partition for ``ivp_radau_solve_dae*``, or None: the DAE entry point is taken only for a problem with a mass
        matrix or a given partition, everything else takes the path it took."""
        if not (getattr(f, "has_mass", False) or any(v is not None for v in (self.nind1, self.nind2, self.nind3))):
            return None
        d = _lib.RadauDaeT()
        d.has_nind1, d.nind1 = (0, 0) if self.nind1 is None else (1, self.nind1)
        d.has_nind2, d.nind2 = (0, 0) if self.nind2 is None else (1, self.nind2)
        d.has_nind3, d.nind3 = (0, 0) if self.nind3 is None else (1, self.nind3)
        return d

    def solve(self, f: api.IVP, t0: float, t1: float, y0: Sequence[float], options: api.Options = None,
              ctx: api.Context = None) -> api.Solution:
        """One trajectory; the ``Solution`` that ``DefaultSolOut`` records (every accepted step, or the ``t_eval`` samples)."""
        return api.solve_ivp(f, t0, t1, y0, options, ctx, _radau=self._c(), _radau_dae=self._dae(f))

    def solve_batch(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None, ctx: api.Context = None,
                    out: api.BatchSolution = None, wait: bool = True):
        """B independent ``solve`` calls; host (numpy) or device (torch) arrays, like ``solve_ivp_batch``.
        ``wait=False`` (device arrays only): enqueue the solve (``ivp_radau_submit_device``) and return a ``PendingBatch``."""
        if not wait and not api._is_torch(y0):
            raise ValueError("wait=False needs device arrays (the host-pointer entry point copies results back at the end)")
        return api.solve_ivp_batch(f, t0, t1, y0, params, options, ctx, out=out, wait=wait, _radau=self._c(), _radau_dae=self._dae(f))

    def solve_batch_banded(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None, ctx: api.Context = None,
                           out: api.BatchSolution = None) -> api.BatchSolution:
        """``solve_batch`` in band storage (``ivp_radau_solve_banded`` / ``_device``), blocking: for a ``DeviceIVP`` compiled
        with ``jac_sparsity=`` and ``jac_storage="banded"`` and nothing else (``ConfigError`` otherwise).  Host (numpy) or device
        (torch) arrays; everything ``solve_batch`` returns, bit for bit what it returns for the same source without a pattern.
        The ``nind*`` fields are not read: there is no DAE partition in band storage."""
        return api.solve_ivp_batch(f, t0, t1, y0, params, options, ctx, out=out, _radau=self._c(), _radau_band=True)

    def solve_banded(self, f: api.IVP, t0: float, t1: float, y0: Sequence[float], options: api.Options = None,
                     ctx: api.Context = None) -> api.Solution:
        """One trajectory through ``solve_batch_banded``: the ``Solution`` of ``solve``."""
        return api.solve_ivp(f, t0, t1, y0, options, ctx, _radau=self._c(), _radau_band=True)

    def solve_batch_logged(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None, ctx: api.Context = None,
                           out: api.BatchSolution = None, reserve: int = 0, two_pass: bool = False) -> api.BatchSolution:
        """Every accepted step of every trajectory in CSR form from ONE integration (``ivp_radau_solve_logged_device``): the
        result, ``reserve``, ``out`` and ``two_pass`` of ``solve_ivp_batch_logged``; no ``max_log`` to guess."""
        return api.solve_ivp_batch_logged(f, t0, t1, y0, params, options, ctx, out=out, reserve=reserve, two_pass=two_pass,
                                          _radau=self._c(), _radau_dae=self._dae(f))

    def solve_batch_dense(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None,
                          ctx: api.Context = None) -> api.BatchSolution:
        """Every trajectory's complete continuous output as a CSR log (``ivp_radau_solve_dense_device``): the result of
        ``solve_ivp_batch_dense`` with 4 n coefficients per segment; ``result.dense`` is a ``BatchContinuousOutput`` with
        ``Method.RADAU`` that evaluates y(t) on the device."""
        return api.solve_ivp_batch_dense(f, t0, t1, y0, params, options, ctx, _radau=self._c(), _radau_dae=self._dae(f))

    def solve_batch_events(self, f: api.IVP, t0, t1, y0, params=None, options: api.Options = None,
                           ctx: api.Context = None) -> api.BatchSolution:
        """Radau with event functions: every occurrence of every event of every trajectory as a CSR log
        (``ivp_radau_solve_events_device``), no ``max_events`` to guess.  The result of ``solve_ivp_batch_events`` --
        ``event_offsets``, ``t_events_csr``, ``y_events_csr``, ``events_of`` / ``events_all``, ``event_info`` with passes and
        staging -- beside everything ``solve_batch`` returns (end state, counters, ``t_eval`` samples with a terminal event's
        appended sample, the bounded step log, dense segments, ``n_event_hits``).  Host (numpy) arrays are moved to the device.
        Refused by the library (``ConfigError``): a problem without event functions, more than 64 states, and everything
        ``solve_batch`` refuses."""
        return api.solve_ivp_batch_events(f, t0, t1, y0, params, options, ctx, _radau=self._c(), _radau_dae=self._dae(f))
