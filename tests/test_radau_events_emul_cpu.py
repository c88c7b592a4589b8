"""The Radau kernel bodies with event functions, run on the host (tests/host_emul_radau_events), against the model
(tests/radau_events_model.py) bit for bit: end state, status, every counter, hit counts, event times and states, the step
log with a terminal point appended, t_eval samples with the terminal sample.  N = 1, 2, 3, 5 (mass, index 2) and 8, chunk
lengths 1, 7 and unbounded -- with one attempt per launch every launch boundary falls between two attempts, so prev_event
(global memory, written by the accepted-step callback only) has to carry its sign across a rejected attempt, an
``h *= 0.5`` restart and the boundary itself -- both integration directions, and the terminal interrupt."""
import numpy as np
import pytest

from tests import radau_dae_model, radau_events_model as EM, radau_model as RM
from tests.host_emul_radau_events import emul_radau_events as E

CHUNKS = [1, 7, E.UNBOUNDED]
COUNTERS = ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(res, b, R, n, max_events, t_eval=None, max_log=0):
    """trajectory b of the emulation's result against the model's Result"""
    assert int(res["status"][b]) == R.status
    assert np.array_equal(_bits(res["t_end"][b]), _bits(R.t_end))
    assert np.array_equal(_bits(res["y_end"][:, b]), _bits(R.y_end))
    assert np.array_equal(_bits(res["h_next"][b]), _bits(R.h_next))
    for c in COUNTERS:
        assert int(res[c][b]) == getattr(R, c), c
    for i, (te, ye) in enumerate(zip(R.t_events, R.y_events)):
        assert int(res["n_ev"][i, b]) == len(te) == R.n_event_hits[i]
        k = min(len(te), max_events)
        assert np.array_equal(_bits(res["t_events"][i, :k, b]), _bits(te[:k]))
        if k:
            assert np.array_equal(_bits(res["y_events"][i, :k, :, b]), _bits(ye[:k]))
    if t_eval is not None:
        m = int(res["n_filled"][b])
        assert m == len(R.t) and list(res["eval_idx"][:m, b]) == R.eval_idx
        if m:
            assert np.array_equal(_bits(res["y_eval"][:m, :, b]), _bits(R.y))
        if R.t_term is not None:
            assert R.eval_idx[-1] == -1 and np.array_equal(_bits(res["t_term"][b]), _bits(R.t_term))
    elif max_log:
        m = int(res["n_log"][b])
        assert m == len(R.t) <= max_log
        assert np.array_equal(_bits(res["t_log"][:m, b]), _bits(R.t)) and np.array_equal(_bits(res["y_log"][:m, :, b]), _bits(R.y))


def relax_f(k, c):
    return lambda x, y: [-k * (y[0] - c)]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_n1_relaxation_both_directions_and_terminal(chunk):
    # forward: y falls from 2 through the level 1; backward from 0.8: y rises through it
    cases = [(0.0, 0.3, 2.0, [EM.ALL], [0]), (0.0, 0.3, 2.0, [EM.NEGATIVE], [1]), (0.0, -0.03, 0.8, [EM.ALL], [0]),
             (0.0, -0.03, 0.8, [EM.POSITIVE], [1]), (0.0, 0.3, 2.0, [EM.POSITIVE], [1])]   # (Direction is in integration order)
    for t0, t1, y0, dirs, term in cases:
        par = np.array([[50.0], [0.5], [1.0]])
        res = E.solve_batch("relax", np.array([[y0]]), par, t0, t1, event_direction=dirs, event_terminal=term, max_log=400, chunk=chunk)
        R = EM.solve(relax_f(50.0, 0.5), lambda x, y: [y[0] - 1.0], [EM.EventConfig(dirs[0], term[0] or None)], t0, t1, [y0], 1e-6, 1e-8)
        check(res, 0, R, 1, 16, max_log=400)
        if dirs[0] == EM.POSITIVE and t1 > t0:
            assert R.n_event_hits == [0] and R.status == RM.SUCCESS   # the falling crossing is filtered out
        elif term[0]:
            assert R.status == RM.INTERRUPT and R.n_event_hits == [1]
        else:
            assert R.status == RM.SUCCESS and R.n_event_hits == [1]
        if chunk == 1:
            assert res["chunks"] >= R.nstep   # one attempt per launch: every counted step had a launch of its own


A2 = [[0.0, 1.0], [-1.0, 0.0]]


def lin_events(n, l0, l1):
    return lambda x, y: [y[0] - l0, y[n - 1] - l1]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("t1", [7.0, -7.0])
def test_n2_two_events_in_one_step_both_directions(chunk, t1):
    # y = (cos t, -sin t): y0 = 0.7 and y1 = -0.7 (forward) / +0.7 (backward) are 0.02 apart in time
    l0, l1 = 0.7, -0.7 if t1 > 0 else 0.7
    par = np.array([[v] for row in A2 for v in row] + [[l0], [l1]])
    res = E.solve_batch("lin2", np.array([[1.0], [0.0]]), par, 0.0, t1, rtol=1e-4, atol=1e-7, event_direction=[EM.ALL, EM.ALL],
                        event_terminal=[0, 0], max_events=8, t_eval=np.linspace(0.0, t1, 9), chunk=chunk)
    R = EM.solve(RM.rhs_dense_linear(A2), lin_events(2, l0, l1), [EM.EventConfig(), EM.EventConfig()], 0.0, t1, [1.0, 0.0], 1e-4, 1e-7,
                 t_eval=list(np.linspace(0.0, t1, 9)))
    assert R.steps_with_two > 0 and min(R.n_event_hits) >= 2
    check(res, 0, R, 2, 8, t_eval=True)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_n2_terminal_count_three_and_t_eval_sample(chunk):
    par = np.array([[v] for row in A2 for v in row] + [[0.0], [5.0]])
    te = np.linspace(0.0, 20.0, 11)
    res = E.solve_batch("lin2", np.array([[1.0], [0.0]]), par, 0.0, 20.0, event_direction=[EM.ALL, EM.ALL], event_terminal=[3, 0],
                        max_events=2, t_eval=te, chunk=chunk)
    R = EM.solve(RM.rhs_dense_linear(A2), lin_events(2, 0.0, 5.0), [EM.EventConfig(EM.ALL, 3), EM.EventConfig()], 0.0, 20.0, [1.0, 0.0],
                 1e-6, 1e-8, t_eval=list(te))
    assert R.status == RM.INTERRUPT and R.n_event_hits == [3, 0] and R.eval_idx[-1] == -1
    check(res, 0, R, 2, 2, t_eval=True)   # max_events = 2 < 3 hits: the count runs on past the block


def restart_follows_event_step(R):
    """is the attempt right after an accepted step that held a root an `h *= 0.5` restart?  (R.h_tried: the h of every attempt
    that reached the Newton iteration; an accepted one ends exactly on the next recorded step, a restart halves h)"""
    acc, x, k, armed = R.t[1:], R.t[0], 0, False
    roots = [t for te in R.t_events for t in te]
    for a, h in enumerate(R.h_tried):
        if k < len(acc) and x + h == acc[k]:
            armed = any(x < t <= acc[k] for t in roots)
            x = acc[k]
            k += 1
        else:
            if armed and a + 1 < len(R.h_tried) and R.h_tried[a + 1] == 0.5 * h:
                return True
            armed = False
    return False


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("level, after_event", [(3e-5, False), (100 * 1e-7, True)])
def test_n3_robertson_threshold_with_restarts(chunk, level, after_event):
    # newton_maxiter = 2 makes the Newton iteration run out (`h *= 0.5` restarts) on this problem; y[1] crosses the level twice.
    # With the level 1e-5 the attempt right after the step of the first root is such a restart: prev_event, written by that
    # step's callback, has to survive it (and, at chunk length 1, the launch boundaries around it)
    rad = {"newton_maxiter": 2}
    res = E.solve_batch("robertson", np.array([[1.0], [0.0], [0.0]]), np.array([[level]]), 0.0, 40.0, event_direction=[EM.ALL],
                        event_terminal=[0], max_log=500, dense_output=True, chunk=chunk, radau=rad)
    R = EM.solve(RM.rhs_robertson, lambda x, y: [y[1] - level], [EM.EventConfig()], 0.0, 40.0, [1.0, 0.0, 0.0], 1e-6, 1e-8,
                 settings=RM.Settings(newton_maxiter=2), dense_output=True)
    assert R.n_restart > 10 and R.n_event_hits == [2]
    assert restart_follows_event_step(R) or not after_event
    check(res, 0, R, 3, 16, max_log=500)
    m = int(res["n_seg"][0])
    assert m == len(R.segs)
    for q, (cont, xold, h) in enumerate(R.segs):
        assert np.array_equal(_bits(res["seg_cont"][q, :, 0]), _bits(cont)) and res["seg_xold"][q, 0] == xold and res["seg_h"][q, 0] == h


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("terminal", [0, 1])
def test_n5_pendulum_index2_mass(chunk, terminal):
    y0 = [1.0, 0.0, 0.0, 0.0, 0.0]
    res = E.solve_batch("pendulum2", np.array(y0)[:, None], None, 0.0, 6.0, nind2=1, event_direction=[EM.ALL], event_terminal=[terminal],
                        max_log=400, chunk=chunk)
    R = EM.solve_dae(radau_dae_model.rhs_pendulum_index2, lambda x, y: [y[0]], [EM.EventConfig(EM.ALL, terminal or None)], 0.0, 6.0, y0,
                     1e-6, 1e-8, mass=radau_dae_model.MASS_PENDULUM, nind2=1)
    assert R.n_event_hits == [1 if terminal else 2] and R.status == (RM.INTERRUPT if terminal else RM.SUCCESS)
    check(res, 0, R, 5, 16, max_log=400)


def a8(i, j):
    return -1.0 - 0.25 * i if i == j else (200.0 if (i % 2 and j == i - 1) else 1e-3 * (1 + ((3 * i + 5 * j) % 7)))


A8 = [[a8(i, j) for j in range(8)] for i in range(8)]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_n8_two_events_on_different_components(chunk):
    par = np.array([[v] for row in A8 for v in row] + [[0.9], [10.0]])   # y[0] dips through 0.9 and comes back: the rising crossing is filtered out
    res = E.solve_batch("lin8", np.ones((8, 1)), par, 0.0, 2.0, event_direction=[EM.NEGATIVE, EM.ALL], event_terminal=[0, 0],
                        max_log=300, chunk=chunk)
    R = EM.solve(RM.rhs_dense_linear(A8), lin_events(8, 0.9, 10.0), [EM.EventConfig(EM.NEGATIVE), EM.EventConfig()], 0.0, 2.0, [1.0] * 8,
                 1e-6, 1e-8)
    assert R.n_event_hits[0] == 1 and R.n_event_hits[1] >= 1
    check(res, 0, R, 8, 16, max_log=300)


def test_batch_of_three_is_three_solo_runs():
    """B = 3 with per-trajectory parameters: prev_event / n_ev are [n_events][B] arrays, a lane must touch its own column."""
    ks = [20.0, 50.0, 90.0]
    par = np.array([ks, [0.5] * 3, [1.0] * 3])
    res = E.solve_batch("relax", np.array([[2.0, 3.0, 1.5]]), par, 0.0, 0.3, event_direction=[EM.ALL], event_terminal=[0], max_log=400, chunk=7)
    for b, (k, y0) in enumerate(zip(ks, [2.0, 3.0, 1.5])):
        R = EM.solve(relax_f(k, 0.5), lambda x, y: [y[0] - 1.0], [EM.EventConfig()], 0.0, 0.3, [y0], 1e-6, 1e-8)
        check(res, b, R, 1, 16, max_log=400)
