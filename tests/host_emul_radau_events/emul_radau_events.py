"""TEST-ONLY driver of tests/host_emul_radau_events/libemul_radau_events.so (see emul_radau_events.cpp): the Radau kernel
bodies for problems with event functions on the CPU, with the GPU launch loop's chunk schedule.  The argument block is
tests/host_emul/emul.py's KArgs, filled the way ``submit_impl`` fills it for ``ivp_radau_solve_events``."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_emul.emul import IVP_RAD_HAS_NEWTON_TOL, IVP_RAD_PREDICTIVE, RADAU_DEFAULTS, KArgs, VP

_HERE = os.path.dirname(os.path.abspath(__file__))
# name -> (id, n, n_params, n_events, has_mass)
RHS = {"relax": (0, 1, 3, 1, False), "lin2": (1, 2, 6, 2, False), "lin8": (1, 8, 66, 2, False), "robertson": (2, 3, 1, 1, False),
       "pendulum2": (3, 5, 0, 1, True)}
IVP_RAD_NIND2_SHIFT, IVP_RAD_NIND3_SHIFT = 12, 16
UNBOUNDED = 0xFFFFFFFF   # chunk: every attempt of a trajectory in one launch
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", _HERE], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_HERE, "libemul_radau_events.so"))
        L.emul_rev_solve.restype = C.c_int
        L.emul_rev_solve.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(KArgs), C.POINTER(C.c_uint64)]
        L.emul_rev_kargs_size.restype = C.c_size_t
        assert L.emul_rev_kargs_size() == C.sizeof(KArgs), (L.emul_rev_kargs_size(), C.sizeof(KArgs))
        _lib = L
    return _lib


def solve_batch(rhs, y0, params, t0, t1, *, event_direction, event_terminal, rtol=1e-6, atol=1e-8, nind2=0, nind3=0, max_steps=None,
                t_eval=None, first_step=None, max_step=None, min_step=None, dense_output=False, max_log=0, max_events=16, chunk=64,
                radau=None):
    """y0 [n, B], params [n_params, B] or None; event_direction / event_terminal: one entry per event function (terminal 0 =
    never).  The bounded event block comes back as t_events [ne, max_events, B], y_events [ne, max_events, n, B], n_ev [ne, B]."""
    L = lib()
    rid, n, npar, ne_ev, _ = RHS[rhs]
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    B = y0.shape[1]
    params = np.ascontiguousarray(params, dtype=np.float64) if npar else np.zeros((1, B))
    assert y0.shape[0] == n and (not npar or params.shape == (npar, B))
    t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64)).copy()
    t1 = np.atleast_1d(np.asarray(t1, dtype=np.float64)).copy()
    a = KArgs()
    a.B = B
    p = lambda arr: arr.ctypes.data_as(VP)
    a.y0, a.params, a.t0, a.t1 = p(y0), p(params), p(t0), p(t1)
    a.t0_stride, a.t1_stride = int(t0.size > 1), int(t1.size > 1)
    rt = np.broadcast_to(np.asarray(rtol, dtype=np.float64), (n,))
    at = np.broadcast_to(np.asarray(atol, dtype=np.float64), (n,))
    for i in range(8):
        a.rtol[i] = rt[i] if i < n else rt[-1]
        a.atol[i] = at[i] if i < n else at[-1]
    a.first_step = float(first_step or 0.0)
    a.has_first_step = int(first_step is not None)
    a.max_step = float(max_step or 0.0)
    a.has_max_step = int(max_step is not None)
    a.nmax = int(max_steps) if max_steps else 2 ** 64 - 1
    a.min_step = float(min_step or 0.0)
    a.has_min_step = int(min_step is not None)
    rd = {**RADAU_DEFAULTS, **(radau or {})}
    a.ctl_uround, a.ctl_safety = float(rd["uround"]), float(rd["safety_factor"])
    a.ctl_facc1, a.ctl_facc2 = 1.0 / float(rd["scale_min"]), 1.0 / float(rd["scale_max"])
    a.ctl_beta = 0.0 if rd["newton_tol"] is None else float(rd["newton_tol"])
    assert 0 <= nind2 and 0 <= nind3 and nind2 + nind3 <= n
    a.ctl_nstiff = int(rd["newton_maxiter"]) | (IVP_RAD_HAS_NEWTON_TOL if rd["newton_tol"] is not None else 0) | \
        (IVP_RAD_PREDICTIVE if rd["predictive"] else 0) | (nind2 << IVP_RAD_NIND2_SHIFT) | (nind3 << IVP_RAD_NIND3_SHIFT)
    a.has_ctl = 0
    res = {
        "y_end": np.zeros((n, B)), "t_end": np.zeros(B), "h_next": np.zeros(B), "status": np.zeros(B, dtype=np.int32),
        "nfev": np.zeros(B, dtype=np.uint64), "nstep": np.zeros(B, dtype=np.uint64),
        "naccpt": np.zeros(B, dtype=np.uint64), "nrejct": np.zeros(B, dtype=np.uint64),
        "njev": np.zeros(B, dtype=np.uint64), "nlu": np.zeros(B, dtype=np.uint64),
        "n_filled": np.zeros(B, dtype=np.int32), "n_log": np.zeros(B, dtype=np.uint32), "n_seg": np.zeros(B, dtype=np.uint32),
    }
    a.y, a.x, a.h, a.status = p(res["y_end"]), p(res["t_end"]), p(res["h_next"]), p(res["status"])
    a.nfev, a.nstep, a.naccpt, a.nrejct = p(res["nfev"]), p(res["nstep"]), p(res["naccpt"]), p(res["nrejct"])
    a.njev, a.nlu = p(res["njev"]), p(res["nlu"])
    a.chunk = chunk
    a.n_eval = -1
    a.n_filled, a.n_log, a.n_seg = p(res["n_filled"]), p(res["n_log"]), p(res["n_seg"])
    keep = []
    if t_eval is not None:
        te = np.ascontiguousarray(t_eval, dtype=np.float64)
        keep.append(te)
        nev = te.size
        a.n_eval = nev
        a.t_eval = p(te) if nev else None
        res["y_eval"] = np.full((nev + 1, n, B), np.nan)   # a terminal event appends its own sample
        res["eval_idx"] = np.full((nev + 1, B), -7, dtype=np.int32)
        a.y_eval, a.eval_idx = p(res["y_eval"]), p(res["eval_idx"])
    elif max_log > 0:
        res["t_log"] = np.full((max_log, B), np.nan)
        res["y_log"] = np.full((max_log, n, B), np.nan)
        a.t_log, a.y_log = p(res["t_log"]), p(res["y_log"])
    a.max_log = max_log
    if dense_output and max_log > 0:
        res["seg_cont"] = np.full((max_log, 4 * n, B), np.nan)
        res["seg_xold"] = np.full((max_log, B), np.nan)
        res["seg_h"] = np.full((max_log, B), np.nan)
        a.seg_cont, a.seg_xold, a.seg_h = p(res["seg_cont"]), p(res["seg_xold"]), p(res["seg_h"])
        a.collect_dense = 1
    assert len(event_direction) == ne_ev and len(event_terminal) == ne_ev and ne_ev <= 4
    for i in range(ne_ev):
        a.ev_direction[i] = int(event_direction[i])
        a.ev_terminal[i] = int(event_terminal[i] or 0)
    a.max_events = max_events
    res["t_events"] = np.full((ne_ev, max(max_events, 1), B), np.nan)
    res["y_events"] = np.full((ne_ev, max(max_events, 1), n, B), np.nan)
    res["n_ev"] = np.zeros((ne_ev, B), dtype=np.uint32)
    res["t_term"] = np.full(B, np.nan)
    a.t_events, a.y_events, a.n_ev, a.t_term = p(res["t_events"]), p(res["y_events"]), p(res["n_ev"]), p(res["t_term"])
    chunks = C.c_uint64(0)
    rc = L.emul_rev_solve(rid, n, ne_ev, C.byref(a), C.byref(chunks))
    if rc == -5:
        raise ValueError("IVP_ERR_INVALID_STEP_SIZE")
    assert rc == 0, rc
    res["chunks"] = chunks.value
    return res
