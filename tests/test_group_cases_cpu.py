"""The references of tests/group_cases.py meet the conditions that make a bit-exact comparison with them worth running.

Oracle only: no kernel is involved.  Every condition holds for every (width, method) pair tests/test_gpu_group_slices.py
uses, for the strict and for the FMA oracle on their own.  A width or method that misses a condition is a reason to change
the batch in group_cases.py, never the condition."""
import numpy as np
import pytest

from tests import group_cases as G


def _attempts(r, method):
    return int(r.nstep) if method == "RK4" else int(r.naccpt) + int(r.nrejct)


@pytest.mark.parametrize("n,method", G.end_state_pairs())
def test_end_state_references_meet_the_conditions(n, method):
    y0, p, t0, t1 = G.method_batch(n, method)
    assert y0.shape == (n, G.batch_size(n)) and sorted(set(p[0])) == [3.0, 40.0, 150.0]
    assert np.count_nonzero(t1 == t0) == 1 and (np.abs(t1[t1 != t0]) <= 2.0).all()
    assert np.count_nonzero(t1 < t0) == (0 if method == "RK4" else 1)     # RK4: one signed first_step for the batch
    runs = {fma: G.references(n, method, fma) for fma in (False, True)}
    for fma, rs in runs.items():
        assert [int(r.status) for r in rs] == [0] * len(rs), (fma, [int(r.status) for r in rs])
        for b, r in enumerate(rs):
            if t1[b] == t0:
                continue
            # chunk_attempts = 7 cuts every non-trivial trajectory into at least 3 launches
            assert _attempts(r, method) > 2 * G.CHUNK, (fma, b, _attempts(r, method))
            if method == "RK4":
                assert np.isfinite(r.y[-1]).all() or p[0, b] == 150.0, (fma, b)
        if method != "RK4":
            assert sum(int(r.nrejct) for r in rs) >= 1, fma
            assert max(int(r.naccpt) for r in rs) >= 30, fma                   # the longest step record of the batch
    # the FMA reference is another computation: at least one bit of y_end differs, else the FMA half proves nothing new
    ys = np.stack([r.y[-1] for r in runs[False]])
    yf = np.stack([r.y[-1] for r in runs[True]])
    assert (ys.view(np.uint64) != yf.view(np.uint64)).any()


@pytest.mark.parametrize("method", ["DOPRI5", "DOP853"])
@pytest.mark.parametrize("n", G.EVENT_WIDTHS)
def test_event_references_meet_the_conditions(n, method):
    for fma in (False, True):
        rs = G.event_references(n, method, fma)
        hits = np.array([[len(t) for t in r.t_events] for r in rs])
        assert hits.sum() >= 3 and (hits[:, 1] > 0).any(), hits            # the negative-direction event occurs too
        ended = [b for b, r in enumerate(rs) if int(r.status) == 1]
        assert ended and all(hits[b, 0] == G.EVENT_TERMINAL[0] for b in ended), (ended, hits)
        assert any(int(r.status) == 0 for r in rs)                        # ... beside trajectories that reach t1
        for b in ended:
            assert float(rs[b].t[-1]) == float(rs[b].t_events[0][-1]) < G.EVENT_T1
