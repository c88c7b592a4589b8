// rk_launch.h -- host-side entry points into the two kernel builds (strict / fast).
#pragma once
#include <hip/hip_runtime.h>
#include "ivp_kargs.h"

// lanes per trajectory of the large-n kernels (rk_group.h): hiprtc modules of systems with n <= 16 / n <= 32 put 4 / 2
// trajectories into a wavefront, everything larger (and every built-in) uses the whole wavefront
static inline int ivp_group_width(int n) { return n <= 16 ? 16 : (n <= 32 ? 32 : 64); }

enum { IVP_LAUNCH_INIT = 0, IVP_LAUNCH_CHUNK = 1, IVP_LAUNCH_COOP = 2 /* hiprtc modules only */,
       IVP_LAUNCH_SAMPLE = 3 /* flavour 3's second kernel: one lane per noted step (rk_global.h sample_kernel_t; lean builds, DOP853) */,
       IVP_LAUNCH_EVENTS = 4 /* deferred event refinement: one lane per noted step (rk_global.h event_kernel_t; problems with event functions,
                                flavour 1, explicit methods, IvpKArgs.evd_rec != NULL) */,
       IVP_LAUNCH_BALANCED = 5 /* one launch of a balanced bulk round (ivp_balance.h; rk_global.h balanced_chunk_kernel_t): `lanes` = 64 x
                                  the plan's workgroups; DOPRI5 / DOP853, flavours 0 and 2, built-in problems of four or more components
                                  without event functions, compiled-in controller fields -- see ivp_has_balanced() */ };

// whether ivp_launch_strict / _fast / _strict_hoist / _fast_hoist carry a balanced kernel for this solve (methods: ivp_hip.h numbering)
static inline bool ivp_has_balanced(int method, int rhs_id, int full, int has_ctl)
{
    return (method == 1 || method == 2) && (full == 0 || full == 2) && !has_ctl && rhs_id == 3;   // CR3BP: the built-in problem with n >= 4
}

// `lanes` = upper bound of trajectories the launch has to cover (grid = ceil(lanes / 64) one-wave blocks).
// `full` = flavour of the kernel: 0 end state only, 1 the whole device DefaultSolOut, 2 log-only (every accepted step recorded,
// nothing else: no interpolant -- rk_core.h so_log_accepted), 3 deferred t_eval sampling (DOP853, built-in problems without
// event functions: the stepping kernel notes the sampled steps, IVP_LAUNCH_SAMPLE evaluates them -- rk_core.h
// so_defer_samples); tables that do not carry flavour 2 / 3 run them as flavour 1 (the host never asks them for 3).
hipError_t ivp_launch_strict(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
hipError_t ivp_launch_strict_hoist(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
hipError_t ivp_launch_fast_hoist(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
hipError_t ivp_launch_fast(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);

// wave-per-trajectory kernels (rk_group.hip): grid = `trajectories` one-wave blocks; RK23 / DOPRI5 / DOP853 / RK4
hipError_t ivp_launch_group_strict(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s);
hipError_t ivp_launch_group_fast(int what, int method, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s);

// lane-cooperative chunk kernels (rk_coop.h): eight lanes per trajectory, grid = ceil(trajectories / 8) waves;
// DOPRI5 / DOP853, built-in right-hand sides without events
hipError_t ivp_launch_coop_strict(int method, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s);
hipError_t ivp_launch_coop_fast(int method, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s);

// thread-per-trajectory BDF kernels (rk_bdf.hip: pinned-coefficient build, n <= 8)
hipError_t ivp_launch_bdf_strict(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
hipError_t ivp_launch_bdf_fast(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
// ... and the same source under __launch_bounds__(64, 2) for batches that over-subscribe the chip (see rk_bdf.hip)
hipError_t ivp_launch_bdf_strict_occ2(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
hipError_t ivp_launch_bdf_fast_occ2(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);

// thread-per-trajectory Radau IIA(5) kernels (rk_radau.hip: pinned-coefficient build, strict arithmetic, n <= 8,
// built-in right-hand sides 0-10 and 15)
hipError_t ivp_launch_radau_strict(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t lanes, hipStream_t s);
// group-per-trajectory Radau IIA(5) kernels (rk_radau_group.hip: radau_group.h, strict arithmetic, 8 < n <= 64: built-in
// right-hand side 102); grid = `trajectories` one-wave blocks
hipError_t ivp_launch_radau_group_strict(int what, int rhs_id, int full, const IvpKArgs &a, uint32_t trajectories, hipStream_t s);
// largest n of the Radau path with the three factors of a trajectory (3 n^2 doubles) resident in LDS (radau_group.h): the
// bound for the built-in problems and for a problem with a mass matrix (IVP_RHS_HAS_MASS_COL)
#define IVP_RADAU_MAX_N 64
// ... and of its wide form (several rows per lane, every matrix in global memory: 4 n^2 doubles per trajectory, 8 MB at
// n = 512): compiled (hiprtc) problems in component form without a mass hook
#define IVP_RADAU_WIDE_MAX_N 512
