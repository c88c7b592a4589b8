"""tests/radau_events_model.py (DefaultSolOut with events over the Radau models) against independent truth, and its branches
by name.

Model against truth.  Two problems with analytic event times:
  * relaxation  y' = -k (y - c), k = 50, c = 0.5, y(0) = 2, crossing the level 1 at t* = ln(3) / 50;
  * a stiff linear 2 x 2 system  y1' = -1000 y1 + 999.5 y2, y2' = -y2 (modes -1000 and -1), y(0) = (1, 1), crossing
    y2 = 0.5 at t* = ln 2 on the slow component.
(1) Every event time must be a root of the model's OWN step interpolant to the reference Brent's termination rule
(solout.rs:227-232): the search stops at an iterate b with a bracket end c, g(b) g(c) <= 0, |c - b| / 2 <= tol1 =
2 RTOL |b| + XTOL / 2 (RTOL = f64::EPSILON, XTOL = 2e-12) or g(b) == 0 -- so the polynomial's root lies within
2 tol1 = 4 eps |b| + 2e-12 of the event time.  Checked with mpmath (50 digits) on the collocation polynomial: its root in
the final bracket is located and its distance to the event time is asserted <= 2 tol1.
(2) The distance to the TRUE root is recorded next to it and asserted within the step's local error scale: the event-free
radau_model run of the same problem (same steps: a non-terminal event does not steer the integration) gives E, the largest
deviation of its interpolant from the true solution over 8 points of every step; the event point satisfies
|y(t_e) - level| <= E + |y'| 2 tol1, so |t_e - t*| <= (E + max|y'| 2 tol1) / min|y'| over the interval between the two
(|y'| is monotone for both problems: evaluated at both ends).
Observed (rtol = 1e-6, atol = 1e-8):
  relaxation:  |t_e - root of the polynomial| = 6.6e-18 (2 tol1 = 2.0e-12), E = 2.6e-06, |t_e - t*| = 8.0e-09, bound 1.0e-07
  stiff 2 x 2: |t_e - root of the polynomial| = 8.8e-13 (2 tol1 = 2.0e-12), E = 1.4e-06, |t_e - t*| = 1.6e-06, bound 2.9e-06
(the figures are printed by the test before it asserts).
"""
import math

import mpmath
import pytest

from tests import radau_events_model as EM, radau_model as M

RT, AT = 1e-6, 1e-8


def poly_root_distance(R, level_of):
    """largest |t_e - root of the step polynomial| over the Brent searches of R, and the largest 2 tol1"""
    mpmath.mp.dps = 50
    worst, tol = 0.0, 0.0
    assert R.roots
    for i, b, c, fb, cont, xold, h in R.roots:
        n = len(cont) // 4

        def g(t):
            s = (t - (mpmath.mpf(xold) + mpmath.mpf(h))) / mpmath.mpf(h)
            y = [mpmath.mpf(cont[q]) + s * (mpmath.mpf(cont[n + q]) + (s - mpmath.mpf(M.C2M1)) * (mpmath.mpf(cont[2 * n + q]) +
                 (s - mpmath.mpf(M.C1M1)) * mpmath.mpf(cont[3 * n + q]))) for q in range(n)]
            return level_of(i, y)
        if fb == 0.0:
            root = mpmath.mpf(b)
        else:
            lo, hi = (mpmath.mpf(b), mpmath.mpf(c)) if b < c else (mpmath.mpf(c), mpmath.mpf(b))
            if g(lo) * g(hi) > 0:   # double rounding of g near the root: widen by the bracket's own width
                w = hi - lo
                lo, hi = lo - w, hi + w
            assert g(lo) * g(hi) <= 0, "the final bracket of the search holds no root of the polynomial"
            root = mpmath.findroot(g, (lo, hi), solver="anderson", tol=1e-40)
        worst = max(worst, float(abs(root - mpmath.mpf(b))))
        tol = max(tol, 2.0 * EM.brent_tol1(b))
        assert float(abs(root - mpmath.mpf(b))) <= 2.0 * EM.brent_tol1(b), (i, b, float(root))
    return worst, tol


def interpolant_error(f, truth, t1, y0):
    """E: the event-free model's interpolant against the true solution, 8 points per step, every component"""
    R = M.solve(f, 0.0, t1, y0, RT, AT, dense_output=True)
    E = 0.0
    for cont, xold, h in R.segs:
        for q in range(1, 9):
            t = xold + h * q / 8.0
            E = max(E, max(abs(a - b) for a, b in zip(M.interpolate(t, cont, xold, h), truth(t))))
    return E, R


def test_relaxation_event_time_against_the_polynomial_and_the_truth():
    k, c, lvl = 50.0, 0.5, 1.0
    f = lambda x, y: [-k * (y[0] - c)]
    truth = lambda t: [c + 1.5 * math.exp(-k * t)]
    R = EM.solve(f, lambda x, y: [y[0] - lvl], [EM.EventConfig()], 0.0, 0.3, [2.0], RT, AT)
    assert R.n_event_hits == [1]
    te = R.t_events[0][0]
    d_poly, tol = poly_root_distance(R, lambda i, y: y[0] - lvl)
    E, R0 = interpolant_error(f, truth, 0.3, [2.0])
    tstar = math.log(3.0) / k
    slope = lambda t: k * 1.5 * math.exp(-k * t)
    bound = (E + max(slope(te), slope(tstar)) * tol) / min(slope(te), slope(tstar))
    print(f"relaxation: poly {d_poly:.2e} (2 tol1 {tol:.2e}) E {E:.2e} truth {abs(te - tstar):.2e} bound {bound:.2e}")
    assert abs(te - tstar) <= bound
    assert (R.t, R.y, R.nstep, R.nfev) == (R0.t, R0.y, R0.nstep, R0.nfev)   # a non-terminal event does not steer the integration


def test_stiff_2x2_event_on_the_slow_component():
    A = [[-1000.0, 999.5], [0.0, -1.0]]
    f = M.rhs_dense_linear(A)
    # y2 = e^-t; y1 = a e^-1000 t + (999.5 / 999) e^-t with a = 1 - 999.5 / 999
    truth = lambda t: [(1.0 - 999.5 / 999.0) * math.exp(-1000.0 * t) + 999.5 / 999.0 * math.exp(-t), math.exp(-t)]
    R = EM.solve(f, lambda x, y: [y[1] - 0.5], [EM.EventConfig()], 0.0, 2.0, [1.0, 1.0], RT, AT)
    assert R.n_event_hits == [1]
    te = R.t_events[0][0]
    d_poly, tol = poly_root_distance(R, lambda i, y: y[1] - 0.5)
    E, _ = interpolant_error(f, truth, 2.0, [1.0, 1.0])
    tstar = math.log(2.0)
    slope = lambda t: math.exp(-t)
    bound = (E + max(slope(te), slope(tstar)) * tol) / min(slope(te), slope(tstar))
    print(f"stiff 2x2: poly {d_poly:.2e} (2 tol1 {tol:.2e}) E {E:.2e} truth {abs(te - tstar):.2e} bound {bound:.2e}")
    assert abs(te - tstar) <= bound
    assert abs(R.y_events[0][0][1] - 0.5) <= 1e-11   # on the interpolant the event state sits on the level


# ---- branches by name ------------------------------------------------------------------------------------------------------

A2 = [[0.0, 1.0], [-1.0, 0.0]]   # y = (cos t, -sin t) from (1, 0)


def two(t1, l0, l1, c0=None, c1=None, **kw):
    return EM.solve(M.rhs_dense_linear(A2), lambda x, y: [y[0] - l0, y[1] - l1], [c0 or EM.EventConfig(), c1 or EM.EventConfig()], 0.0, t1,
                    [1.0, 0.0], 1e-4, 1e-7, **kw)


@pytest.mark.parametrize("t1", [3.0, -3.0])
def test_two_events_in_one_step_are_processed_in_chronological_order(t1):
    """forward: y1 = -0.7 at t = 0.7754 comes BEFORE y0 = 0.7 at t = 0.7954 although it is event 1; backward the same with
    y1 = +0.7.  Both roots lie in one step (steps_with_two)."""
    l1 = -0.7 if t1 > 0 else 0.7
    R = two(t1, 0.7, l1)
    assert R.steps_with_two > 0
    a, b = R.t_events[1][0], R.t_events[0][0]
    assert abs(a) < abs(b) and abs(abs(a) - math.asin(0.7)) < 1e-3 and abs(abs(b) - math.acos(0.7)) < 1e-3
    # the earlier root terminal: the later one of the same step is NOT recorded, whatever its index
    R1 = two(t1, 0.7, l1, c1=EM.EventConfig(EM.ALL, 1))
    assert R1.status == M.INTERRUPT and R1.n_event_hits == [0, 1] and R1.t_term == a and R1.t[-1] == a
    # the later root terminal: the earlier one is recorded first
    R0 = two(t1, 0.7, l1, c0=EM.EventConfig(EM.ALL, 1))
    assert R0.status == M.INTERRUPT and R0.n_event_hits == [1, 1] and R0.t_term == b and R0.t_events[1] == [a]
    assert (R0.t_end, R0.y_end, R0.nstep) == (R1.t_end, R1.y_end, R1.nstep)   # both leave after the same accepted step


def test_a_root_exactly_at_a_step_end():
    """g == 0 at an accepted point: the step that ends there records (x, y) itself (|fb| <= XTOL), and with Direction::All the
    step that starts there records the same point again (|fa| <= XTOL: xold, yold) -- the reference's behaviour; Positive
    / Negative see it once or not at all."""
    R0 = M.solve(M.rhs_sho, 0.0, 3.0, [1.0, 0.0], RT, AT)
    k = len(R0.t) // 2
    tk, yk = R0.t[k], R0.y[k][0]
    ev = lambda x, y: [y[0] - yk]
    R = EM.solve(M.rhs_sho, ev, [EM.EventConfig()], 0.0, 3.0, [1.0, 0.0], RT, AT)
    assert R.t_events[0] == [tk, tk] and R.y_events[0] == [R0.y[k], R0.y[k]] and not R.roots   # no search ran
    falling = yk < R0.y[k - 1][0]
    Rn = EM.solve(M.rhs_sho, ev, [EM.EventConfig(EM.NEGATIVE)], 0.0, 3.0, [1.0, 0.0], RT, AT)
    Rp = EM.solve(M.rhs_sho, ev, [EM.EventConfig(EM.POSITIVE)], 0.0, 3.0, [1.0, 0.0], RT, AT)
    # Negative: left > 0 && right <= 0 -- the step that ends on the root; Positive: left < 0 && right >= 0 -- neither step
    assert (Rn.t_events[0], Rp.t_events[0]) == (([tk], []) if falling else ([], [tk]))


def test_direction_filtering():
    cfgs = {EM.ALL: None, EM.POSITIVE: None, EM.NEGATIVE: None}
    for d in cfgs:
        cfgs[d] = EM.solve(M.rhs_sho, lambda x, y: [y[0]], [EM.EventConfig(d)], 0.0, 10.0, [1.0, 0.0], RT, AT).t_events[0]
    assert len(cfgs[EM.ALL]) == 3 and cfgs[EM.NEGATIVE] == cfgs[EM.ALL][0::2] and cfgs[EM.POSITIVE] == cfgs[EM.ALL][1::2]
    assert EM.crossed(-1.0, 0.0, EM.POSITIVE) and not EM.crossed(0.0, 1.0, EM.POSITIVE) and EM.crossed(0.0, 1.0, EM.ALL)
    assert EM.crossed(1.0, 0.0, EM.NEGATIVE) and not EM.crossed(0.0, -1.0, EM.NEGATIVE) and not EM.crossed(1.0, 2.0, EM.ALL)


@pytest.mark.parametrize("count", [1, 3])
def test_terminal_count(count):
    free = EM.solve(M.rhs_sho, lambda x, y: [y[0]], [EM.EventConfig()], 0.0, 20.0, [1.0, 0.0], RT, AT)
    R = EM.solve(M.rhs_sho, lambda x, y: [y[0]], [EM.EventConfig(EM.ALL, count)], 0.0, 20.0, [1.0, 0.0], RT, AT)
    assert R.status == M.INTERRUPT and R.n_event_hits == [count] and R.t_events[0] == free.t_events[0][:count]
    assert R.t_term == R.t_events[0][-1] and R.t[-1] == R.t_term and R.y[-1] == R.y_events[0][-1]   # appended to Solution.t / y
    assert R.t[:-1] == free.t[:len(R.t) - 1]
    # radau.rs:727-730: x, y are the END of the accepted step that held the root (the callback returned before recording
    # it), h is that step's h (not hnew)
    assert R.t[-2] < R.t_term < R.t_end and R.t[-2] + R.h_next == R.t_end
    assert (R.t_end, R.y_end) == (free.t[len(R.t) - 1], free.y[len(R.t) - 1])
    assert R.naccpt == len(R.t) - 1   # records: the initial point, every accepted step but the last, the terminal point


def test_terminal_sample_in_t_eval_mode():
    te = [0.5 * k for k in range(9)]
    R = EM.solve(M.rhs_sho, lambda x, y: [y[0]], [EM.EventConfig(EM.ALL, 1)], 0.0, 4.0, [1.0, 0.0], RT, AT, t_eval=te)
    assert R.status == M.INTERRUPT and abs(R.t_term - math.pi / 2) < 1e-5
    # samples 0, 0.5, 1, 1.5 and those of the interrupting step are NOT taken (the callback returns before sampling) ...
    assert R.eval_idx[-1] == -1 and R.t[-1] == R.t_term and all(t <= R.t_term for t in R.t[:-1])
    assert R.eval_idx[:-1] == list(range(len(R.eval_idx) - 1))
    free = M.solve(M.rhs_sho, 0.0, 4.0, [1.0, 0.0], RT, AT, t_eval=te)
    assert R.y[:-1] == free.y[:len(R.y) - 1]


def test_terminal_event_on_the_first_step():
    k, c = 50.0, 0.5
    R = EM.solve(lambda x, y: [-k * (y[0] - c)], lambda x, y: [y[0] - (2.0 - 1e-9)], [EM.EventConfig(EM.ALL, 1)], 0.0, 0.3, [2.0], RT, AT)
    assert R.status == M.INTERRUPT and R.naccpt == 1 and R.n_event_hits == [1] and 0.0 < R.t_term < R.t_end
    assert R.t == [0.0, R.t_term]   # the initial record and the terminal point


def test_no_event_at_all_equals_the_event_free_model_bit_for_bit():
    R = EM.solve(M.rhs_robertson, lambda x, y: [y[1] - 1.0, y[0] + 1.0], [EM.EventConfig(), EM.EventConfig(EM.ALL, 1)], 0.0, 40.0,
                 [1.0, 0.0, 0.0], RT, AT, dense_output=True)
    R0 = M.solve(M.rhs_robertson, 0.0, 40.0, [1.0, 0.0, 0.0], RT, AT, dense_output=True)
    assert R.n_event_hits == [0, 0] and R.t_events == [[], []] and R.t_term is None
    for k in ("status", "t_end", "y_end", "h_next", "nfev", "njev", "nlu", "nstep", "naccpt", "nrejct", "t", "y", "segs"):
        assert getattr(R, k) == getattr(R0, k), k
    assert M.SolOut is not EM.EventSolOut and M.solve(M.rhs_sho, 0.0, 1.0, [1.0, 0.0], RT, AT).status == M.SUCCESS   # the hook is put back
