"""Base batches for tests/test_gpu_wave_density.py, its helper tests/helpers/wave_density_dump.py and the CPU test of their
preconditions, tests/test_wave_density_cases_cpu.py.

A case is a BASE BATCH of B0 trajectories (67 for Radau: one full wavefront plus three lanes, coprime to 64; 130 for BDF)
with its reference results: tests/radau_model.py / tests/radau_dae_model.py for Radau, the C oracle (strict or FMA build)
for BDF.  The inputs are the ones the other test modules use, widened to B0 trajectories.  A run of B trajectories gives
trajectory b the inputs of base trajectory b mod B0, so every copy must equal its base reference row, bit for bit.

`reference(case)` is computed once per process and cached; `run(case, B, ...)` is the device run, `compare(got, ref, idx)`
the vectorised bit comparison of every member the reference carries (status, t_end, h_next, y_end, the six counters and
every recorded output).  Slots of a padded output past a trajectory's count are never written and are not compared.
"""
import contextlib
import math

import numpy as np

from tests import radau_dae_model as D
from tests import radau_model as M

B0_RADAU, B0_BDF = 67, 130
COUNTERS = ("nfev", "njev", "nlu", "nstep", "naccpt", "nrejct")
RT, AT = 1e-6, 1e-8


class Case:
    def __init__(self, name, family, y0, params, t0, t1, opts, problem, build_ref, *, radau=None, ragged=None, hiprtc=False,
                 fma=False, claims=(), slots=False, chunks=(0,), occ2_tile=False):
        self.name, self.family, self.hiprtc, self.fma = name, family, hiprtc, fma
        self.y0 = np.ascontiguousarray(y0, dtype=np.float64)
        self.params = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
        self.t0, self.t1 = t0, (np.asarray(t1, dtype=np.float64) if np.ndim(t1) else float(t1))
        self.opts = dict(opts)          # ivp_amd.Options keywords
        self.radau = radau              # ivp_amd.Radau keywords (None: a BDF case)
        self.ragged = ragged            # per-trajectory t_eval grids of the base batch, or None
        self.problem = problem          # () -> the ivp_amd problem (built on the device side only)
        self.build_ref = build_ref      # () -> (reference dict, the per-trajectory models or oracle solutions)
        self.claims = set(claims)       # what tests/test_wave_density_cases_cpu.py must find in the first 64 entries
        self.slots = slots              # carries the lane_attempt_slots check (max nstep <= 2 mean nstep is asserted)
        self.chunks = chunks            # chunk_attempts values the in-process runs use
        self.occ2_tile = occ2_tile      # BDF: also tiled past one wave per SIMD, where the first rounds take the occ2 build
        self.B0 = self.y0.shape[1]

    @property
    def kernel_family(self):
        base = {"radau": "Radau", "radau_dae": "Radau DAE", "bdf": "BDF FMA" if self.fma else "BDF strict"}[self.family]
        return base + (" (hiprtc)" if self.hiprtc else "")


_REF = {}


def reference(case):
    """(ref, models): ref maps member -> numpy array whose LAST axis is the base trajectory"""
    if case.name not in _REF:
        _REF[case.name] = case.build_ref()
    return _REF[case.name]


# ---- bit comparison -------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """elementwise `same()` of the Radau tests: bit equality, NaN equal to NaN, signed zeros distinguished"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return a.astype(np.int64) == b.astype(np.int64)


# padded member -> (its count member, axis of the record slot)
PADDED = {"eval_idx": ("n_filled", 0), "y_eval": ("n_filled", 0), "t_log": ("n_log", 0), "y_log": ("n_log", 0),
          "seg_xold": ("n_seg", 0), "seg_h": ("n_seg", 0), "seg_cont": ("n_seg", 0),
          "t_events": ("n_event_hits", 1), "y_events": ("n_event_hits", 1)}


def compare(got, ref, idx, what=""):
    """every member of `ref` (last axis: base trajectory) against `got` (last axis: trajectory b = copy of base idx[b])"""
    idx = np.asarray(idx)
    bad = []
    for k, rv in ref.items():
        if k.startswith("csr_"):
            continue
        g, w = np.asarray(got[k]), rv[..., idx]
        if g.shape != w.shape:
            bad.append(f"{k}: shape {g.shape} against {w.shape}")
            continue
        ok = same_bits(g, w)
        if k in PADDED:
            ck, ax = PADDED[k]
            cnt = np.minimum(ref[ck][..., idx], g.shape[ax])
            slot = np.arange(g.shape[ax])
            valid = slot[:, None] < cnt[None, :] if ax == 0 else slot[None, :, None] < cnt[:, None, :]
            while valid.ndim < g.ndim:
                valid = np.expand_dims(valid, -2)
            ok = ok | ~valid
        elif k == "t_term":
            ok = ok | (ref["status"][idx] != 1)
        if not ok.all():
            cols = np.unique(np.nonzero(~ok)[-1])
            bad.append(f"{k}: {len(cols)} of {len(idx)} trajectories differ, first b = {cols[0]} (base {idx[cols[0]]}): "
                       f"{g[..., cols[0]].ravel()[:6]} against {w[..., cols[0]].ravel()[:6]}")
    if "csr_sizes" in ref:   # per-trajectory grids: the batch's CSR records are the base block, repeated
        sizes = ref["csr_sizes"]
        B = len(idx)
        reps, rem = divmod(B, len(sizes))
        assert np.array_equal(idx, np.arange(B) % len(sizes))
        offs = np.concatenate([[0], np.cumsum(sizes)])
        if not np.array_equal(np.asarray(got["eval_offsets"]), np.concatenate([[0], np.cumsum(sizes[idx])])):
            bad.append("eval_offsets")
        else:
            tile = lambda v: np.concatenate([v] * reps + [v[:offs[rem]]])
            valid = tile(ref["csr_valid"])
            for k, ck in (("y_eval", "csr_y"), ("eval_idx", "csr_idx")):
                g, w = np.asarray(got[k]), tile(ref[ck])
                ok = same_bits(g[:len(w)], w) | ~(valid if g.ndim == 1 else valid[:, None])
                if len(g) < len(w) or not ok.all():
                    bad.append(f"{k} (CSR): {np.count_nonzero(~ok)} values differ")
    assert not bad, f"{what}: " + "; ".join(bad)


# ---- the device run ---------------------------------------------------------------------------------------------------------
OUT_KEYS = ("status", "t_end", "h_next", "y_end") + COUNTERS + (
    "n_filled", "eval_idx", "y_eval", "eval_offsets", "n_log", "t_log", "y_log", "n_seg", "seg_xold", "seg_h", "seg_cont",
    "n_event_hits", "t_events", "y_events", "t_term")

_PROBLEMS = {}


def run(case, B=None, chunk=0, profile=0):
    """The case on the device with B trajectories (default: the base batch), trajectory b taking the inputs of base
    trajectory b mod B0.  Returns (members as numpy arrays, stats)."""
    import torch
    import ivp_amd
    dev = torch.device("cuda:0")
    B = case.B0 if B is None else B
    idx = np.arange(B) % case.B0
    if case.name not in _PROBLEMS:
        _PROBLEMS[case.name] = case.problem()
    f = _PROBLEMS[case.name]
    put = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    y0 = put(case.y0[:, idx])
    par = None if case.params is None else put(case.params[:, idx])
    t1 = put(case.t1[idx]) if np.ndim(case.t1) else case.t1
    kw = dict(case.opts)
    if case.ragged is not None:
        kw["t_eval_per_trajectory"] = [case.ragged[i] for i in idx]
    if case.family == "bdf":
        o = ivp_amd.Options(method="BDF", fp_mode=ivp_amd.FpMode.FAST if case.fma else ivp_amd.FpMode.STRICT,
                            chunk_attempts=chunk, profile=profile, **kw)
        r = ivp_amd.solve_ivp_batch(f, case.t0, t1, y0, par, o)
    else:
        o = ivp_amd.Options(chunk_attempts=chunk, profile=profile, **kw)
        r = ivp_amd.Radau(**case.radau).solve_batch(f, case.t0, t1, y0, par, o)
    torch.cuda.synchronize()
    got = {}
    for k in OUT_KEYS:
        v = getattr(r, k, None)
        if v is not None:
            got[k] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    return got, dict(r.stats)


# ---- references from the Radau models ------------------------------------------------------------------------------------
@contextlib.contextmanager
def _mark_factorisations():
    """While active, every real / complex factorisation of the models opens a new entry in the pivots list it was given:
    ("fact", kind), followed by the row exchanges the models record themselves -- so that exchanges can be compared at the
    same factorisation index."""
    saved = [(mod, name, getattr(mod, name)) for mod in (M, D) for name in ("lu_decomp", "lu_decomp_complex")]

    def real(a, ip, pivots=None):
        if pivots is not None:
            pivots.append(("fact", "real"))
        return saved[0][2](a, ip, pivots)

    def cplx(ar, ai, ip, pivots=None, cases=None):
        if pivots is not None:
            pivots.append(("fact", "complex"))
        return saved[1][2](ar, ai, ip, pivots, cases)

    for mod in (M, D):
        mod.lu_decomp, mod.lu_decomp_complex = real, cplx
    try:
        yield
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)


def pivots_by_factorisation(m):
    out = []
    for p in m.pivots:
        if p[0] == "fact":
            out.append([p[1]])
        else:
            out[-1].append(p[1:])
    return [tuple(v) for v in out]


def attempts_of_model(m):
    """radau_attempt calls of a trajectory (what `it` counts in radau_chunk_body): one per step counted in nstep, plus the
    attempts that end in a singular factor before the step is counted"""
    return m.nstep + m.n_restart_real + m.n_restart_complex


class _Degenerate:
    """t1 == t0: solve_ivp's early return, taken in the init kernel (tests/test_gpu_radau.py,
    test_degenerate_and_nan_intervals_beside_five_healthy_trajectories): status 0, h_next = 0, no counter moves"""

    def __init__(self, t0, y0):
        self.status, self.t_end, self.h_next, self.y_end = 0, float(t0), 0.0, [float(v) for v in y0]
        self.nfev = self.njev = self.nlu = self.nstep = self.naccpt = self.nrejct = 0
        self.n_restart_real = self.n_restart_complex = self.n_restart_newton = 0
        self.newton_counts, self.pivots, self.t, self.y, self.eval_idx, self.segs = [], [], [], [], [], []


def ref_from_models(models, n, opts, ragged=None):
    B = len(models)
    ref = {"status": np.array([m.status for m in models], dtype=np.int64),
           "t_end": np.array([m.t_end for m in models]), "h_next": np.array([m.h_next for m in models]),
           "y_end": np.array([m.y_end for m in models], dtype=np.float64).T.copy()}
    for k in COUNTERS:
        ref[k] = np.array([getattr(m, k) for m in models], dtype=np.int64)
    if opts.get("t_eval") is not None:
        rows = len(opts["t_eval"])
        ref["n_filled"] = np.array([len(m.t) for m in models], dtype=np.int64)
        ref["eval_idx"] = np.zeros((rows, B), dtype=np.int64)
        ref["y_eval"] = np.zeros((rows, n, B))
        for b, m in enumerate(models):
            ref["eval_idx"][:len(m.t), b] = m.eval_idx
            if m.t:
                ref["y_eval"][:len(m.t), :, b] = np.array(m.y)
    elif ragged is not None:
        sizes = np.array([len(g) for g in ragged], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        ref["n_filled"] = np.array([len(m.t) for m in models], dtype=np.int64)
        ref["csr_sizes"] = sizes
        ref["csr_y"], ref["csr_idx"] = np.zeros((int(offs[-1]), n)), np.zeros(int(offs[-1]), dtype=np.int64)
        ref["csr_valid"] = np.zeros(int(offs[-1]), dtype=bool)
        for b, m in enumerate(models):
            lo, k = int(offs[b]), len(m.t)
            ref["csr_valid"][lo:lo + k] = True
            ref["csr_idx"][lo:lo + k] = m.eval_idx
            if k:
                ref["csr_y"][lo:lo + k] = np.array(m.y)
    elif opts.get("max_log"):
        ml = opts["max_log"]
        ref["n_log"] = np.array([len(m.t) for m in models], dtype=np.int64)   # the count runs on past the capacity
        ref["t_log"], ref["y_log"] = np.zeros((ml, B)), np.zeros((ml, n, B))
        for b, m in enumerate(models):
            k = min(ml, len(m.t))
            ref["t_log"][:k, b] = m.t[:k]
            if k:
                ref["y_log"][:k, :, b] = np.array(m.y[:k])
        if opts.get("dense_output"):
            ref["n_seg"] = np.array([len(m.segs) for m in models], dtype=np.int64)
            ref["seg_xold"], ref["seg_h"], ref["seg_cont"] = np.zeros((ml, B)), np.zeros((ml, B)), np.zeros((ml, 4 * n, B))
            for b, m in enumerate(models):
                for q, (cont, xold, h) in enumerate(m.segs[:ml]):
                    ref["seg_xold"][q, b], ref["seg_h"][q, b] = xold, h
                    ref["seg_cont"][q, :, b] = cont
    return ref


def _radau_case(name, problem, rhs_of, y0, params, t0, t1, opts, *, family="radau", radau=None, settings=None, jac=None,
                mass_of=None, nind=(None, None, None), ragged=None, model_kw=None, rtol=RT, atol=AT, **kw):
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    n, B = y0.shape
    opts = dict(rtol=rtol, atol=atol, **opts)
    radau = dict(radau or {})
    if family == "radau_dae":
        radau.update({k: v for k, v in zip(("nind1", "nind2", "nind3"), nind) if v is not None})

    def build():
        mk = dict(model_kw or {})
        for k in ("t_eval", "dense_output", "max_steps", "first_step"):
            if opts.get(k) is not None:
                mk[k] = list(opts[k]) if k == "t_eval" else opts[k]
        if settings:
            mk["settings"] = M.Settings(**settings)
        models = []
        with _mark_factorisations():
            for b in range(B):
                tb = float(t1[b]) if np.ndim(t1) else float(t1)
                yb = [float(v) for v in y0[:, b]]
                if tb == t0:
                    models.append(_Degenerate(t0, yb))
                    continue
                kb = dict(mk)
                if ragged is not None:
                    kb["t_eval"] = [float(v) for v in ragged[b]]
                if family == "radau_dae":
                    models.append(D.solve(rhs_of(b), t0, tb, yb, rtol, atol, mass=mass_of(b), nind1=nind[0], nind2=nind[1], nind3=nind[2], **kb))
                else:
                    models.append(M.solve(rhs_of(b), t0, tb, yb, rtol, atol, jac=jac, **kb))
        return ref_from_models(models, n, opts, ragged), models

    return Case(name, family, y0, params, t0, t1, opts, problem, build, radau=radau, ragged=ragged, **kw)


# ---- Radau, thread form: the inputs of tests/test_gpu_radau.py -------------------------------------------------------------
def vdp_eps_batch(B=67, seed=2024):
    """tests/test_gpu_radau.py's stiff Van der Pol batch (the same numbers)"""
    rng = np.random.default_rng(seed)
    eps = np.exp(rng.uniform(np.log(5e-4), np.log(2e-3), B))
    y0 = np.stack([2.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)])
    return y0, eps[None, :].copy()


def lin_matrix(n):
    """tests/test_gpu_radau.py's dense test matrix: couplings of 200 below the diagonal of every second row become the
    pivots of their columns once U1 / h + 1 < 200 -- at a factorisation index that depends on the trajectory's steps"""
    a = [[1e-3 * (1 + ((3 * i + 5 * j) % 7)) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] = -1.0 - 0.25 * i
        if i % 2:
            a[i][i - 1] = 200.0
    return a


def lin_source(a, with_jac):
    n = len(a)
    lit = lambda v: float(v).hex()
    src = "__device__ void ode(double x, const double* y, double* d, const double* p) {\n"
    for i in range(n):
        src += f"  d[{i}] = " + " + ".join(f"{lit(a[i][j])} * y[{j}]" for j in range(n)) + ";\n"
    src += "}\n"
    if with_jac:
        src += "__device__ void jac(double x, const double* y, double* j, const double* p) {\n"
        src += "".join(f"  j[{i * n + k}] = {lit(a[i][k])};\n" for i in range(n) for k in range(n)) + "}\n"
    return src


def _builtin(name, *a):
    def make():
        import ivp_amd
        return getattr(ivp_amd, name)(*a)
    return make


def _device(src, n, **kw):
    def make():
        import ivp_amd
        return ivp_amd.DeviceIVP(src, n, **kw)
    return make


def _robertson_y0(B, seed=9):
    rng = np.random.default_rng(seed)
    y0 = np.zeros((3, B))
    y0[0] = 1.0 + 0.2 * rng.uniform(-1.0, 1.0, B)
    y0[2] = 0.05 * rng.uniform(0.0, 1.0, B)
    y0[:, 0] = [1.0, 0.0, 0.0]
    return y0


def _lin8_y0(B, seed=88):
    """tests/test_gpu_radau.py's y0 for the 8 x 8 system, scaled over five decades and with random signs per component: the
    step sizes, and with them the factorisation at which the couplings take over as pivots, differ between trajectories"""
    rng = np.random.default_rng(seed)
    base = np.array([1.0, 0.5, -0.5, 0.25, 0.0, 1e-3, -1.0, 2.0])
    y0 = base[:, None] * (10.0 ** rng.uniform(-3.0, 2.0, (1, B))) * rng.choice([-1.0, 1.0], (8, B))
    y0 += 1e-2 * rng.standard_normal((8, B)) * (10.0 ** rng.uniform(-3.0, 2.0, (1, B)))
    y0[:, 0] = base
    return y0


def radau_cases():
    B = B0_RADAU
    y0v, eps = vdp_eps_batch()
    vdp = _builtin("StiffVanDerPol")
    rhs_v = lambda b: M.rhs_vdp_eps(float(eps[0, b]))
    out = [_radau_case("radau_vdp", vdp, rhs_v, y0v, eps, 0.0, 2.0, {}, claims={"newton", "attempts", "reject"}, slots=True,
                       chunks=(0, 1, 7))]
    yr = _robertson_y0(B)
    out.append(_radau_case("radau_robertson_fd", _builtin("Robertson"), lambda b: M.rhs_robertson, yr, None, 0.0, 1e3, {},
                           claims={"newton", "attempts", "reject"}))
    out.append(_radau_case("radau_robertson_jac", _builtin("RobertsonJac"), lambda b: M.rhs_robertson, yr, None, 0.0, 1e3, {},
                           jac=M.jac_robertson, claims={"newton", "attempts", "reject"}))
    a8 = lin_matrix(8)
    out.append(_radau_case("radau_lin8_jit", _device(lin_source(a8, True), 8, jac=True), lambda b: M.rhs_dense_linear(a8), _lin8_y0(B), None,
                           0.0, 5.0, {}, jac=M.jac_dense_linear(a8), rtol=1e-4, atol=1e-6, hiprtc=True,
                           claims={"newton", "attempts", "pivots"}))
    # one batch with, inside its first 64 entries: a NaN right-hand side (17), a zero-length interval (5), trajectories that
    # exhaust max_steps (the long intervals) beside ones that finish, all under newton_maxiter = 2, whose Newton loop runs out
    # of iterations and restarts with half the step hundreds of times
    rng = np.random.default_rng(64)
    t1 = np.exp(rng.uniform(np.log(0.02), np.log(0.6), B))
    t1[5] = 0.0
    epsm = eps.copy()
    epsm[0, 17] = np.nan
    out.append(_radau_case("radau_mixed", vdp, lambda b: M.rhs_vdp_eps(float(epsm[0, b])), y0v, epsm, 0.0, t1, dict(max_steps=60),
                           radau=dict(newton_maxiter=2), settings=dict(newton_maxiter=2),
                           claims={"newton", "attempts", "nan", "zero_length", "max_steps", "newton_restart"}, chunks=(0, 1)))
    # outputs: tests/test_gpu_radau.py's grid (t0, a pair closer than the tolerance, t1, a point outside), ragged grids, a
    # bounded log that the long trajectories overflow, dense segments
    grid = [0.0, 0.1, 0.1 + 1e-13, 0.7, 1.5, 2.0, 2.5]
    out.append(_radau_case("radau_vdp_t_eval", vdp, rhs_v, y0v, eps, 0.0, 2.0, dict(t_eval=grid), claims={"newton", "attempts"}))
    grids = [np.linspace(0.0, 2.0, 3 + (2 * b) % 11) if b % 9 != 2 else np.zeros(0) for b in range(B)]
    out.append(_radau_case("radau_vdp_ragged", vdp, rhs_v, y0v, eps, 0.0, 2.0, {}, ragged=grids, claims={"newton", "attempts"}))
    t1l = np.where(np.arange(B) % 3 == 1, 0.1, 2.0)   # every third trajectory fits the log, the others overflow it
    out.append(_radau_case("radau_vdp_log", vdp, rhs_v, y0v, eps, 0.0, t1l, dict(max_log=48), claims={"attempts", "log_overflow"}))
    out.append(_radau_case("radau_vdp_dense", vdp, rhs_v, y0v, eps, 0.0, 0.9, dict(max_log=224, dense_output=True),
                           claims={"newton", "attempts", "dense_fits"}))
    rngb = np.random.default_rng(4)
    yb = np.stack([np.cos(rngb.uniform(0, 1, B)), np.sin(rngb.uniform(0, 1, B))])
    yb[:, 0], yb[:, 1] = [1.0, 0.0], [0.3, -0.7]
    out.append(_radau_case("radau_sho_backward", _builtin("SHO"), lambda b: M.rhs_sho, yb, None, 1.0, -2.0 - 0.02 * np.arange(B), {},
                           claims={"attempts"}))
    return out


# ---- Radau, M y' = f: the inputs of tests/test_gpu_radau_dae.py -----------------------------------------------------------
ODE = "__device__ void ode(double x, const double* y, double* d, const double* p)"
MASS = "__device__ void mass(double* m, const double* p)"
SCALAR_SRC = f"{ODE} {{ d[0] = p[1] / (1.0 + x * x) - y[0]; }}\n{MASS} {{ m[0] = p[0]; }}\n"
SEMI_SRC = (f"{ODE} {{ d[0] = -y[0] + y[1]; d[1] = y[1] - x / (1.0 + x * x); }}\n"
            f"{MASS} {{ m[0] = p[0]; m[1] = p[1]; m[2] = p[2]; m[3] = p[3]; }}\n")


def pend_src(constraint):
    return (f"{ODE} {{ const double p1 = y[0], p2 = y[1], v1 = y[2], v2 = y[3], lam = y[4];\n"
            f"  d[0] = v1; d[1] = v2; d[2] = -lam * p1; d[3] = -lam * p2 - 1.0; d[4] = {constraint}; }}\n"
            f"{MASS} {{ m[0] = 1.0; m[6] = 1.0; m[12] = 1.0; m[18] = 1.0; }}\n")


PEND2_SRC = pend_src("p1 * v1 + p2 * v2")
PEND3_SRC = pend_src("p1 * p1 + p2 * p2 - 1.0")
PENDSEL_SRC = pend_src("p[0] != 0.0 ? p1 * v1 + p2 * v2 : lam - (v1 * v1 + v2 * v2 - p2)")


def f_scalar(p1):
    return lambda x, y: [M.fdiv(p1, 1.0 + x * x) - y[0]]


def f_semi(x, y):
    return [-y[0] + y[1], y[1] - M.fdiv(x, 1.0 + x * x)]


def f_pend_index1(x, s):
    p1, p2, v1, v2, lam = s
    return [v1, v2, -lam * p1, -lam * p2 - 1.0, lam - (v1 * v1 + v2 * v2 - p2)]


def pend_y0(phi):
    """at rest at angle phi: lam = -sin phi balances gravity along the rod"""
    return [math.cos(phi), math.sin(phi), 0.0, 0.0, 0.0 - math.sin(phi)]


def full_mass(n):
    return [[(1.0 + 0.125 * r) if r == c else (0.01 * (1 + (r + 2 * c) % 5)) * (-1.0 if (r + c) % 3 == 0 else 1.0) for c in range(n)]
            for r in range(n)]


def lin_mass_source(a, ms):
    n = len(a)
    lit = lambda v: float(v).hex()
    src = ODE + " {\n"
    for i in range(n):
        src += f"  d[{i}] = " + " + ".join(f"{lit(a[i][j])} * y[{j}]" for j in range(n)) + ";\n"
    src += "}\n" + MASS + " {\n" + "".join(f"  m[{r * n + c}] = {lit(ms[r][c])};\n" for r in range(n) for c in range(n)) + "}\n"
    return src


def cols(rows):
    return np.array(rows, dtype=np.float64).T.copy()


def radau_dae_cases():
    B = B0_RADAU
    dae = lambda *a, **kw: _radau_case(*a, family="radau_dae", hiprtc=True, **kw)
    out = []
    # n = 1, a mass per trajectory (every 13th is the algebraic equation M = [0])
    p0 = [0.0 if b % 13 == 0 else 0.25 + 0.125 * b for b in range(B)]
    p1 = [1.0 + 0.01 * b for b in range(B)]
    out.append(dae("dae_n1_mass_per_trajectory", _device(SCALAR_SRC, 1, params=(0.0, 1.0), mass=True), lambda b: f_scalar(p1[b]),
                   np.ones((1, B)), cols([[a, b] for a, b in zip(p0, p1)]), 0.0, 2.0, {}, mass_of=lambda b: [[p0[b]]],
                   claims={"newton", "attempts"}))
    # n = 2, semi-explicit and dense mass in alternation, dense output
    semi, dense2 = [[1.0, 0.0], [0.0, 0.0]], [[2.0, 1.0], [1.0, 2.0]]
    flat = lambda m: [v for row in m for v in row]
    rng = np.random.default_rng(22)
    y2 = np.stack([rng.uniform(-1.0, 1.0, B), rng.uniform(-1.0, 1.0, B)])
    y2[:, 0], y2[:, 1] = [0.0, 0.0], [1.0, -0.5]
    m2 = [semi if b % 2 == 0 else dense2 for b in range(B)]
    out.append(dae("dae_n2_semi_explicit_dense", _device(SEMI_SRC, 2, params=flat(semi), mass=True), lambda b: f_semi, y2,
                   cols([flat(m) for m in m2]), 0.0, 2.0, dict(max_log=64, dense_output=True), mass_of=lambda b: m2[b],
                   claims={"newton", "attempts", "dense_fits"}))
    # n = 5, the pendulum at index 2 (tolerance 1e-4: rejections and Newton dyth exits) and at index 3
    yp = cols([pend_y0(-0.6 + 0.02 * b) for b in range(B)])
    mp = lambda b: D.MASS_PENDULUM
    out.append(dae("dae_n5_pendulum_index2", _device(PEND2_SRC, 5, mass=True), lambda b: D.rhs_pendulum_index2, yp, None, 0.0, 2.0, {},
                   mass_of=mp, nind=(4, 1, 0), rtol=1e-4, atol=1e-4, claims={"newton", "attempts", "reject"}, slots=True))
    out.append(dae("dae_n5_pendulum_index3", _device(PEND3_SRC, 5, mass=True), lambda b: D.rhs_pendulum_index3, yp, None, 0.0, 2.0,
                   dict(first_step=1e-3), mass_of=mp, nind=(2, 2, 1), rtol=1e-4, atol=1e-4, claims={"newton", "attempts"}))
    # the pure-ODE partition (5, 0, 0): right for the index-1 form, wrong for alternate trajectories, which carry the
    # index-2 constraint and end in StepSizeTooSmall
    sel = [float(b % 2) for b in range(B)]
    out.append(dae("dae_n5_wrong_partition", _device(PENDSEL_SRC, 5, params=(0.0,), mass=True),
                   lambda b: D.rhs_pendulum_index2 if sel[b] else f_pend_index1, cols([pend_y0(0.1 * (0, 1, 3, 4, 7, 8, 10, 11, 12)[b % 9]) for b in range(B)]),   # angles at which the wrong partition fails
                   cols([[s] for s in sel]), 0.0, 2.0, {}, mass_of=mp, nind=(5, 0, 0), rtol=1e-6, atol=1e-6,
                   claims={"attempts", "wrong_partition"}))
    # n = 8, a full mass matrix
    a8, mm = lin_matrix(8), full_mass(8)
    out.append(dae("dae_n8_full_mass", _device(lin_mass_source(a8, mm), 8, mass=True), lambda b: M.rhs_dense_linear(a8), _lin8_y0(B, 89), None,
                   0.0, 1.5, {}, mass_of=lambda b: mm, claims={"newton", "attempts", "pivots"}))
    return out


# ---- BDF, n <= 8: the C oracle ---------------------------------------------------------------------------------------------
ROBERTSON_JAC_SRC = r"""
__device__ void ode(double t, const double* s, double* d, const double* p)
{
    const double x = s[0], y = s[1], z = s[2];
    d[0] = -0.04 * x + 1e4 * y * z;
    d[1] = 0.04 * x - 1e4 * y * z - 3e7 * y * y;
    d[2] = 3e7 * y * y;
}
__device__ void jac(double t, const double* s, double* j, const double* p)
{
    const double y = s[1], z = s[2];
    j[0] = -0.04;  j[1] = 1e4 * z;               j[2] = 1e4 * y;
    j[3] = 0.04;   j[4] = -1e4 * z - 6e7 * y;    j[5] = -1e4 * y;
                   j[7] = 6e7 * y;
}
"""


def _eval_idx_of(grid, t):
    """the grid indices of the emitted samples: the reference walks the grid in order, so the k-th sample is the first
    grid point after the (k-1)-th one's with that value"""
    out, i = [], 0
    for v in t:
        while grid[i] != v:
            i += 1
        out.append(i)
        i += 1
    return out


def _bdf_case(name, rhs, problem, y0, params, t0, t1, opts, *, fma=False, events=None, oracle_rhs=None, **kw):
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    n, B = y0.shape
    opts = dict(opts)
    oracle_rhs = oracle_rhs or rhs

    def build():
        from oracle import oracle as O
        from tests.common import oracle_batch
        okw = dict(method="BDF", **{k: v for k, v in opts.items() if k not in ("max_log", "max_events")})
        if events:
            okw.update(event_direction=events[0], event_terminal=events[1])
        mode = dict(fma=True) if fma else {}
        ref = {k: v for k, v in oracle_batch(oracle_rhs, y0, params, t0, t1, **mode, **okw).items()
               if k in ("status", "t_end", "h_next", "y_end") + COUNTERS}
        for k in COUNTERS + ("status",):
            ref[k] = ref[k].astype(np.int64)
        sols = []
        recorded = opts.get("t_eval") is not None or opts.get("max_log") or events
        for b in range(B if recorded else 0):
            tb = float(t1[b]) if np.ndim(t1) else float(t1)
            sols.append(O.solve_ivp(oracle_rhs, t0, tb, y0[:, b], params=() if params is None else list(params[:, b]), detpow=True, fma=fma, **okw))
        if sols:   # the two entry points of the oracle agree
            assert [s.nstep for s in sols] == list(ref["nstep"]) and [s.status for s in sols] == list(ref["status"])
        if opts.get("t_eval") is not None:
            grid = np.asarray(opts["t_eval"], dtype=np.float64)
            rows = len(grid) + (1 if events else 0)
            ref["n_filled"] = np.array([len(s.t) for s in sols], dtype=np.int64)
            ref["eval_idx"], ref["y_eval"] = np.zeros((rows, B), dtype=np.int64), np.zeros((rows, n, B))
            for b, s in enumerate(sols):
                k = len(s.t)
                ref["eval_idx"][:k, b] = _eval_idx_of(grid, s.t)
                ref["y_eval"][:k, :, b] = s.y
        elif opts.get("max_log"):
            ml = opts["max_log"]
            assert max(len(s.t) for s in sols) <= ml
            ref["n_log"] = np.array([len(s.t) for s in sols], dtype=np.int64)
            ref["t_log"], ref["y_log"] = np.zeros((ml, B)), np.zeros((ml, n, B))
            for b, s in enumerate(sols):
                ref["t_log"][:len(s.t), b], ref["y_log"][:len(s.t), :, b] = s.t, s.y
            if opts.get("dense_output"):
                ref["n_seg"] = np.array([0 if s.seg_h is None else len(s.seg_h) for s in sols], dtype=np.int64)
                nc = sols[0].seg_cont.shape[1]
                ref["seg_xold"], ref["seg_h"], ref["seg_cont"] = np.zeros((ml, B)), np.zeros((ml, B)), np.zeros((ml, nc, B))
                for b, s in enumerate(sols):
                    k = int(ref["n_seg"][b])
                    if k:
                        ref["seg_xold"][:k, b], ref["seg_h"][:k, b], ref["seg_cont"][:k, :, b] = s.seg_xold, s.seg_h, s.seg_cont
        if events:
            ne, mev = len(events[0]), opts["max_events"]
            ref["n_event_hits"] = np.array([[len(s.t_events[i]) for s in sols] for i in range(ne)], dtype=np.int64)
            assert ref["n_event_hits"].max() <= mev
            ref["t_events"], ref["y_events"] = np.zeros((ne, mev, B)), np.zeros((ne, mev, n, B))
            for b, s in enumerate(sols):
                for i in range(ne):
                    k = len(s.t_events[i])
                    ref["t_events"][i, :k, b], ref["y_events"][i, :k, :, b] = s.t_events[i], s.y_events[i]
            if opts.get("t_eval") is not None:   # the time of the sample a terminal event appends: written in t_eval mode only
                ref["t_term"] = np.array([s.t[-1] if s.status == 1 else 0.0 for s in sols])
        return ref, sols

    return Case(name, "bdf", y0, params, t0, t1, opts, problem, build, fma=fma, **kw)


def _ball(direction, terminal):
    def make():
        import ivp_amd
        return ivp_amd.BouncingBall(9.81, 0.02, ivp_amd.EventConfig(ivp_amd.Direction(direction), terminal))
    return make


def bdf_cases():
    from ivp_amd import workloads as W
    B = B0_BDF
    out = []
    # BASELINE C5's stiff Van der Pol on a short horizon, ragged end times: waves thin out from the first rounds on
    y0, mu, t0, _ = W.vdp_stiff_batch(B)
    rng = np.random.default_rng(130)
    t1 = 3.0 * np.exp(rng.uniform(np.log(0.05), 0.0, B))
    for fma in (False, True):
        out.append(_bdf_case("bdf_vdp" + ("_fma" if fma else ""), "vdp", _builtin("VanDerPol"), y0, mu, t0, t1, dict(rtol=1e-4, atol=1e-6),
                             fma=fma, claims={"attempts", "reject", "ragged_end"}, chunks=(0, 1, 7), occ2_tile=True))
    out.append(_bdf_case("bdf_vdp_uniform", "vdp", _builtin("VanDerPol"), y0, mu, t0, 3.0, dict(rtol=1e-4, atol=1e-6),
                         claims={"attempts", "reject"}, slots=True))
    yr = _robertson_y0(B, 10) * np.array([[1e4], [1e4], [1e4]])
    t1r = 1e4 * np.exp(rng.uniform(np.log(0.01), 0.0, B))
    out.append(_bdf_case("bdf_robertson", "robertson", _builtin("Robertson"), yr, None, 0.0, t1r, dict(rtol=1e-6, atol=1e-6),
                         claims={"attempts", "reject"}))
    out.append(_bdf_case("bdf_robertson_jac", "robertson_jac", _builtin("RobertsonJac"), yr, None, 0.0, t1r, dict(rtol=1e-6, atol=1e-6),
                         claims={"attempts", "reject"}))
    out.append(_bdf_case("bdf_robertson_jac_jit", "robertson_jac", _device(ROBERTSON_JAC_SRC, 3, jac=True), yr, None, 0.0, t1r,
                         dict(rtol=1e-6, atol=1e-6), hiprtc=True, claims={"attempts", "reject"}))
    # tests/test_gpu_parity.py's rational problem: grids with points outside the span and a repeated point
    rng2 = np.random.default_rng(2)
    yq = np.stack([np.full(B, 1 / 3), np.full(B, 2 / 9)]) * (1 + 1e-3 * rng2.standard_normal((2, B)))
    te_f = np.array([4.0, 5.0, 5.01, 5.5, 5.5, 7.0, 8.0, 8.01, 9.0, 9.5])
    te_b = np.array([5.0, 4.99, 3.0, 3.0, 1.5, 1.1, 1.0, 0.5])
    t1f, t1b = 9.0 - 3.5 * rng2.uniform(0, 1, B), 1.0 + 3.5 * rng2.uniform(0, 1, B)   # ragged ends: more grid points fall outside
    t1f[0], t1b[0] = 9.0, 1.0
    out.append(_bdf_case("bdf_rational_t_eval_fwd", "rational", _builtin("Rational"), yq, None, 5.0, t1f, dict(rtol=1e-3, atol=1e-6, t_eval=te_f),
                         claims={"attempts"}))
    out.append(_bdf_case("bdf_rational_t_eval_bwd", "rational", _builtin("Rational"), yq, None, 5.0, t1b, dict(rtol=1e-3, atol=1e-6, t_eval=te_b),
                         claims={"attempts", "reject"}))
    out.append(_bdf_case("bdf_rational_t_eval_fwd_fma", "rational", _builtin("Rational"), yq, None, 5.0, t1f,
                         dict(rtol=1e-3, atol=1e-6, t_eval=te_f), fma=True, claims={"attempts"}))
    # tests/test_gpu_parity.py's SHO batch with step log and dense segments
    rng4 = np.random.default_rng(4)
    ys = np.stack([np.cos(rng4.uniform(0, 1, B)), np.sin(rng4.uniform(0, 1, B))])
    out.append(_bdf_case("bdf_sho_log_dense", "sho", _builtin("SHO"), ys, None, 0.0, 1.0 + 2.0 * rng4.uniform(0, 1, B),
                         dict(rtol=1e-5, atol=1e-8, dense_output=True, max_log=64), claims={"attempts"}))
    # the bouncing ball with a terminal event on the way down
    yb = np.stack([10.0 * (1.0 + 0.1 * rng4.uniform(-1, 1, B)), 5.0 * (1.0 + 0.2 * rng4.uniform(-1, 1, B))])
    pb = np.stack([np.full(B, 9.81), np.full(B, 0.02)])
    out.append(_bdf_case("bdf_ball_terminal_event", "ball", _ball(-1, 1), yb, pb, 0.0, 10.0, dict(rtol=1e-6, atol=1e-9, max_log=96, max_events=4),
                         events=([-1], [1]), claims={"attempts", "terminal_event"}))
    return out


_ALL = {}


def cases(family):
    if family not in _ALL:
        _ALL[family] = {"radau": radau_cases, "radau_dae": radau_dae_cases, "bdf": bdf_cases}[family]()
    return _ALL[family]


def all_cases():
    return cases("radau") + cases("radau_dae") + cases("bdf")


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
