"""CPU model of Radau IIA(5) with event functions: the yardstick of tests/test_gpu_radau_events.py and
tests/test_radau_events_*_cpu.py.

DefaultSolOut WITH events, restated in plain Python floats from the reference:
  * src/solve/solout.rs:141-146   dense segments come first;
  * src/solve/solout.rs:158-165   the event functions are evaluated at every callback; the initial callback (yold empty)
                                  only stores g as prev_event;
  * src/solve/solout.rs:168-176   the crossing test per Direction (src/solve/event.rs: All / Positive / Negative,
                                  EventConfig::terminal_count);
  * src/solve/solout.rs:188-291   Brent's method on the step interpolant: XTOL = 2e-12, RTOL = f64::EPSILON, at most 100
                                  iterations, |fa| <= XTOL / |fb| <= XTOL take the step's ends, termination
                                  |xm| <= tol1 = 2 RTOL |b| + XTOL / 2 or fb == 0;
  * src/solve/solout.rs:297-303   the roots of one step sorted by time, stable, ascending forward and descending backward;
  * src/solve/solout.rs:306-326   every root recorded and counted; terminal_count reached: the event point appended to
                                  Solution.t / Solution.y, prev_event updated, ControlFlag::Interrupt;
  * src/solve/solout.rs:329-338   prev_event and yold updated;
  * src/methods/radau.rs:725-730  Interrupt leaves 'main with Status::UserInterrupt and the step's h: x, y, the counters
                                  are those after the accepted step.
The operation order inside the root search is that of the kernels' so_event_root / so_events (ivp_amd/csrc/rk_core.h),
which match the oracle bit for bit for the other methods: the device is compared bit for bit.  In t_eval mode the device
delivers the terminal point as one more sample with eval_idx = -1 (and t_term); the model appends it to t / y with idx -1.

The step loops are NOT restated here: radau_model.solve / radau_dae_model.solve run unchanged, with their DefaultSolOut
replaced (by name, for the duration of the call) by the subclass below.  They have no interrupt path, so the subclass
raises, and the state RADAU::solve returns after `break 'main` is read from the step loop's frame where the callback was made.
"""
import sys

from tests import radau_dae_model, radau_model
from tests.radau_model import INTERRUPT, fdiv, interpolate, rs_min

XTOL = 2e-12
RTOL = 2.220446049250313e-16   # f64::EPSILON
MAXITER = 100

ALL, POSITIVE, NEGATIVE = 0, 1, -1   # Direction, as ivp_options_t.ev_direction carries it


class EventConfig:
    """src/solve/event.rs: direction and terminal_count (None = never terminal)."""

    def __init__(self, direction=ALL, terminal_count=None):
        self.direction, self.terminal_count = direction, terminal_count


def crossed(left, right, direction):
    """solout.rs:168-176"""
    if direction == ALL:
        return (left <= 0.0 and right >= 0.0) or (left >= 0.0 and right <= 0.0)
    if direction > 0:
        return left < 0.0 and right >= 0.0
    return left > 0.0 and right <= 0.0


def brent_tol1(b):
    """The termination tolerance of the search at the iterate b (solout.rs:227)."""
    return 2.0 * RTOL * abs(b) + 0.5 * XTOL


def event_root(i, xold, x, g_prev, g_cur, y, yold, interp, events, trace=None):
    """solout.rs:194-291 -> (event_t, event_y).  interp = (cont, xold, h) of the accepted step."""
    a, b, fa, fb = xold, x, g_prev, g_cur
    if abs(fa) <= XTOL:
        return a, list(yold)
    if abs(fb) <= XTOL:
        return b, list(y)
    c, fc = a, fa
    d = b - a
    e = d
    for _ in range(MAXITER):
        if fb * fc > 0.0:
            c, fc = a, fa
            d = b - a
            e = d
        if abs(fc) < abs(fb):
            a, b, c = b, c, b
            fa, fb, fc = fb, fc, fb
        tol1 = 2.0 * RTOL * abs(b) + 0.5 * XTOL
        xm = 0.5 * (c - b)
        if abs(xm) <= tol1 or fb == 0.0:
            break
        if abs(e) >= tol1 and abs(fa) > abs(fb):
            if a == c:
                s = fdiv(fb, fa)
                p = 2.0 * xm * s
                q = 1.0 - s
            else:
                q_val, r = fdiv(fa, fc), fdiv(fb, fc)
                s = fdiv(fb, fa)
                p = s * (2.0 * xm * q_val * (q_val - r) - (b - a) * (r - 1.0))
                q = (q_val - 1.0) * (r - 1.0) * (s - 1.0)
            if q > 0.0:
                p = -p
            else:
                q = -q
            if 2.0 * p < rs_min(3.0 * xm * q - abs(tol1 * q), abs(e * q)):
                e = d
                d = fdiv(p, q)
            else:
                d = xm
                e = d
        else:
            d = xm
            e = d
        a, fa = b, fb
        if abs(d) > tol1:
            b += d
        else:
            b += tol1 if xm > 0.0 else -tol1
        fb = events(b, interpolate(b, *interp))[i]
    if trace is not None:
        trace.append((i, b, c, fb, tuple(interp[0]), interp[1], interp[2]))   # the final bracket [b, c] and the polynomial
    return b, interpolate(b, *interp)


class Interrupt(Exception):
    """ControlFlag::Interrupt"""


class EventSolOut(radau_model.SolOut):
    """DefaultSolOut with events, over radau_model.SolOut's recording (dense segments, t_eval samples, the step log)."""

    def __init__(self, x0, t_eval, first_step, collect_dense, events, config):
        super().__init__(x0, t_eval, first_step, collect_dense)
        self.events, self.config = events, config
        ne = len(config)
        self.prev_event = [0.0] * ne
        self.yold = None
        self.t_events = [[] for _ in range(ne)]
        self.y_events = [[] for _ in range(ne)]
        self.hits = [0] * ne
        self.t_term = None
        self.roots = []   # event_root's trace: (event, b, c, g(b), cont, xold, h) of every Brent search that ran
        self.steps_with_two = 0

    def call(self, xold, x, y, interp):
        # solout.rs:141-146 (the base class would do it after the events: the segment of an interrupting step IS collected)
        if self.collect_dense and x != xold and interp is not None and interp[2] != 0.0:
            self.segs.append((list(interp[0]), interp[1], interp[2]))
        g_curr = list(self.events(x, y))
        if self.yold is None:
            self.prev_event = g_curr
        else:
            detected = []
            for i, cfg in enumerate(self.config):
                if crossed(self.prev_event[i], g_curr[i], cfg.direction):
                    et, ey = event_root(i, xold, x, self.prev_event[i], g_curr[i], y, self.yold, interp, self.events, self.roots)
                    detected.append((et, i, ey))
            if len(detected) > 1:
                self.steps_with_two += 1
            forward = x > xold
            for u in range(1, len(detected)):   # stable insertion sort (so_events; Vec::sort_by is stable too)
                v = u
                while v > 0 and (detected[v][0] < detected[v - 1][0] if forward else detected[v][0] > detected[v - 1][0]):
                    detected[v], detected[v - 1] = detected[v - 1], detected[v]
                    v -= 1
            for et, i, ey in detected:
                self.t_events[i].append(et)
                self.y_events[i].append(ey)
                self.hits[i] += 1
                limit = self.config[i].terminal_count
                if limit is not None and self.hits[i] >= limit:
                    self.t.append(et)
                    self.y.append(list(ey))
                    if self.t_eval is not None:
                        self.idx.append(-1)
                    self.t_term = et
                    self.prev_event = g_curr
                    raise Interrupt()
            self.prev_event = g_curr
        self.yold = list(y)
        dense, self.collect_dense = self.collect_dense, False   # collected above
        try:
            super().call(xold, x, y, interp)
        finally:
            self.collect_dense = dense


def _frame_of(tb, code):
    while tb is not None:
        if tb.tb_frame.f_code is code:
            return tb.tb_frame
        tb = tb.tb_next
    raise RuntimeError("the step loop's frame is not on the traceback")


def solve(f, events, config, x0, xend, y0, rtol, atol, model=radau_model, **kw):
    """model.solve(f, x0, xend, y0, rtol, atol, **kw) with `events(x, y) -> list` watched by `config` (a list of
    EventConfig).  The Result of the model plus t_events / y_events (lists per event), n_event_hits, t_term (None unless a
    terminal event interrupted), roots (the trace of every Brent search) and steps_with_two."""
    made = []

    def factory(sx0, t_eval=None, first_step=None, collect_dense=False):
        made.append(EventSolOut(sx0, t_eval, first_step, collect_dense, events, config))
        return made[-1]

    saved = model.SolOut
    model.SolOut = factory
    try:
        try:
            R = model.solve(f, x0, xend, y0, rtol, atol, **kw)
        except Interrupt:
            # radau.rs:727-730: `break 'main` right after the callback -- everything the loop holds at that point is the result
            L = _frame_of(sys.exc_info()[2], model.solve.__code__).f_locals
            R = L["R"]
            R.status, R.t_end, R.y_end, R.h_next = INTERRUPT, L["x"], list(L["y"]), L["h"]
            R.nfev, R.njev, R.nlu, R.nstep, R.naccpt, R.nrejct = L["nfev"], L["njev"], L["nlu"], L["nstep"], L["naccpt"], L["nrejct"]
    finally:
        model.SolOut = saved
    so = made[0]
    R.t, R.y, R.eval_idx, R.segs = so.t, so.y, so.idx, so.segs
    R.t_events, R.y_events, R.n_event_hits, R.t_term = so.t_events, so.y_events, list(so.hits), so.t_term
    R.roots, R.steps_with_two = so.roots, so.steps_with_two
    return R


def solve_dae(f, events, config, x0, xend, y0, rtol, atol, **kw):
    """... over radau_dae_model.solve (mass=, nind1 / nind2 / nind3=)."""
    return solve(f, events, config, x0, xend, y0, rtol, atol, model=radau_dae_model, **kw)
