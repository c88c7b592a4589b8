#!/usr/bin/env python3
"""Times the unbounded event output (solve_ivp_batch_events / ivp_batch_solve_events_device) on BASELINE C2 -- 100k CR3BP
orbits, DOPRI5, rtol 1e-6, the crossing event g = y -- in its one-pass form (max_events >= every count: one integration,
pack from the counting solve's block) and its two-pass form (max_events = 0: count, then a filling solve), beside the two
baselines of `bench.py --full` (outputs.events): the bounded events solve at max_events = 16 and the same right-hand side
without events.  The baselines run code this feature does not touch (stepping kernels and solve_ivp_batch are unchanged),
measured here in the same process, the four forms alternating, so that they share whatever else the machine is doing.

The pack kernel alone is timed with HIP events around the library's measurement hook for ivp_event_pack()
(ivp_event_pack_timing_hook, event_kernels.h) on the block of a bounded solve with room for every occurrence; its rate is the bytes the records
need, read once and written once, over that time.

  python tools/bench_events_csr.py [--batch B] [--solves K] [--warmup W] [--packs R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivp_amd  # noqa: E402
from ivp_amd import _lib  # noqa: E402
from ivp_amd import workloads as W  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_sha import kernel_sources_sha256  # noqa: E402

CR3BP_EVENT_SRC = r"""
__device__ void ode(double t, const double* s, double* d, const double* p)
{
    const double mu = p[0];
    const double x = s[0], y = s[1], z = s[2], vx = s[3], vy = s[4], vz = s[5];
    const double a = x + mu, b = x - 1.0 + mu;
    const double r1 = sqrt(a * a + y * y + z * z), r2 = sqrt(b * b + y * y + z * z);
    const double r13 = r1 * r1 * r1, r23 = r2 * r2 * r2;
    d[0] = vx; d[1] = vy; d[2] = vz;
    d[3] = x + 2.0 * vy - (1.0 - mu) * (x + mu) / r13 - mu * (x - 1.0 + mu) / r23;
    d[4] = y - 2.0 * vx - (1.0 - mu) * y / r13 - mu * y / r23;
    d[5] = -(1.0 - mu) * z / r13 - mu * z / r23;
}
__device__ void events(double t, const double* s, double* g, const double* p) { g[0] = s[1]; }   // crossings of the x axis
"""
HBM_COPY_GBS = (4600.0, 4900.0)   # plain device-to-device copy rate, profiles/r04_hbm_calib.log


class EventPackArgs(C.Structure):   # ivp_amd/csrc/event_kernels.h
    _fields_ = [("st_t", C.c_void_p), ("st_y", C.c_void_p), ("hits", C.c_void_p), ("off", C.c_void_p), ("t", C.c_void_p), ("y", C.c_void_p),
                ("err", C.c_void_p), ("B", C.c_ulonglong), ("first", C.c_ulonglong), ("cnt", C.c_uint32), ("cap", C.c_uint32), ("n", C.c_uint32),
                ("n_events", C.c_uint32)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--packs", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_events_csr.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    ctx = ivp_amd.default_context(0)
    y0, p, t0, t1 = W.cr3bp_batch(a.batch)
    y0d, pd = torch.as_tensor(y0, device=dev), torch.as_tensor(p, device=dev)
    B, n = y0.shape[1], y0.shape[0]
    base = dict(method="DOPRI5", rtol=1e-6, atol=1e-9)
    f = ivp_amd.DeviceIVP(CR3BP_EVENT_SRC, n=6, params=(W.ARENSTORF_MU,), ctx=ctx, events=[ivp_amd.EventConfig()])
    f0 = ivp_amd.DeviceIVP(CR3BP_EVENT_SRC.split("__device__ void events")[0], n=6, params=(W.ARENSTORF_MU,), ctx=ctx)
    count = ivp_amd.solve_ivp_batch_events(f, t0, t1, y0d, pd, ivp_amd.Options(max_events=0, **base), ctx)
    most, total = int(count.n_event_hits.max()), count.event_info["total"]
    prev = {}

    def bounded(key, prob, opts):   # as bench.py times it: the result buffers are reused
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # max_events = 16 overflows on some orbits: that is the baseline's state
            prev[key] = ivp_amd.solve_ivp_batch(prob, t0, t1, y0d, pd, opts, ctx, prev.get(key))
        return prev[key]

    forms = {
        "no_events": lambda: bounded("n", f0, ivp_amd.Options(**base)),
        "bounded_max_events_16": lambda: bounded("b", f, ivp_amd.Options(max_events=16, **base)),
        "csr_one_pass": lambda: ivp_amd.solve_ivp_batch_events(f, t0, t1, y0d, pd, ivp_amd.Options(max_events=most, **base), ctx),
        "csr_two_pass": lambda: ivp_amd.solve_ivp_batch_events(f, t0, t1, y0d, pd, ivp_amd.Options(max_events=0, **base), ctx),
    }
    ms = {k: [] for k in forms}
    passes = {}
    for it in range(a.warmup + a.solves):
        for k, fn in forms.items():   # alternating: every form sees the same drift of the machine
            r, t = wall(fn)
            if it >= a.warmup:
                ms[k].append(t)
            if k.startswith("csr"):
                passes[k] = r.event_info["passes"]
                assert r.event_info["total"] == total
    stored16 = int(torch.clamp(prev["b"].n_event_hits, max=16).sum())

    # ---- the pack kernel alone ----
    bnd = ivp_amd.solve_ivp_batch(f, t0, t1, y0d, pd, ivp_amd.Options(max_events=most, **base), ctx)
    one = forms["csr_one_pass"]()
    L = _lib.load()
    hook = L.ivp_event_pack_timing_hook   # checks the size of this file's copy of EventPackArgs before it launches
    hook.restype = C.c_int
    hook.argtypes = [C.POINTER(EventPackArgs), C.c_size_t, C.c_void_p]
    pack = lambda ap, st: hook(ap, C.sizeof(EventPackArgs), st)
    t_out = torch.zeros(max(total, 1), dtype=torch.float64, device=dev)
    y_out = torch.zeros((max(total, 1), n), dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    args = EventPackArgs(bnd.t_events.data_ptr(), bnd.y_events.data_ptr(), bnd.n_event_hits.data_ptr(), one.event_offsets.data_ptr(),
                         t_out.data_ptr(), y_out.data_ptr(), err.data_ptr(), B, 0, B, most, n, 1)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(10):
        assert pack(C.byref(args), stream) == 0
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and torch.equal(t_out[:total], one.t_events_csr) and torch.equal(y_out[:total], one.y_events_csr)
    pack_ms = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.packs):
        e0.record()
        pack(C.byref(args), stream)
        e1.record()
        torch.cuda.synchronize()
        pack_ms.append(e0.elapsed_time(e1))
    # a window long enough to be more than launch latency: R back-to-back launches between one pair of events
    e0.record()
    for _ in range(a.packs):
        pack(C.byref(args), stream)
    e1.record()
    torch.cuda.synchronize()
    pack_train_ms = e0.elapsed_time(e1) / a.packs
    rec_bytes = total * (n + 1) * 8
    moved = 2 * rec_bytes + 4 * B + 8 * (B + 1)      # records read and written once, the counts and the offsets read once
    med = lambda v: float(np.median(v))
    res = {
        "what": "C2 (CR3BP DOPRI5 rtol 1e-6, event g = y, hiprtc right-hand side): wall ms per complete solve, host-synchronised, "
                "the four forms alternating; pack kernel: HIP-event ms per launch",
        "B": B, "records": total, "max_hits": most, "mean_hits": total / B, "record_bytes": rec_bytes,
        "warmup": a.warmup, "solves": a.solves,
        "ms": ms, "median_ms": {k: med(v) for k, v in ms.items()}, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
        "passes": passes,
        "bounded_16_records_stored": stored16, "bounded_16_records_lost": total - stored16,
        "bounded_16_block_bytes": 16 * (n + 1) * 8 * B, "csr_one_pass_staging_bytes": one.event_info["staging_bytes"],
        "ratio_one_pass_over_bounded_16": med(ms["csr_one_pass"]) / med(ms["bounded_max_events_16"]),
        "ratio_two_pass_over_bounded_16": med(ms["csr_two_pass"]) / med(ms["bounded_max_events_16"]),
        "ratio_one_pass_over_no_events": med(ms["csr_one_pass"]) / med(ms["no_events"]),
        "ratio_two_pass_over_no_events": med(ms["csr_two_pass"]) / med(ms["no_events"]),
        "pack": {"cap": most, "launches": a.packs, "median_ms_single_launch": med(pack_ms), "min_ms_single_launch": float(np.min(pack_ms)),
                 "ms_per_launch_back_to_back": pack_train_ms, "bytes_moved": moved,
                 "achieved_GBs_back_to_back": moved / (pack_train_ms * 1e-3) / 1e9,
                 "achieved_GBs_single_launch": moved / (med(pack_ms) * 1e-3) / 1e9,
                 "plain_copy_GBs": list(HBM_COPY_GBS),
                 "frac_of_plain_copy": moved / (pack_train_ms * 1e-3) / 1e9 / HBM_COPY_GBS[0],
                 "note": "bytes_moved is what the records need (read once, written once); the block is read with a stride of cap "
                         "slots per trajectory.  single_launch includes the launch latency; back_to_back amortises it"},
        "kernel_sources_sha256": kernel_sources_sha256(),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
