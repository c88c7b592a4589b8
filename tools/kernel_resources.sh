#!/bin/bash
# Register / scratch / occupancy table of every kernel in libivp_hip.so's translation units (hipcc remarks, no GPU needed).
# usage: tools/kernel_resources.sh > profiles/rNN_kernel_resources.txt
TOOLS="$(cd "$(dirname "$0")" && pwd)"
cd "$TOOLS/../ivp_amd/csrc" || exit 1
COMMON="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c -o /dev/null"
run() {  # name, source, flags...
    local name=$1 src=$2; shift 2
    /opt/rocm/bin/hipcc $COMMON "$@" "$src" 2>&1 | python3 "$TOOLS/kernel_resources.py" "$name"
}
run strict      rk_kernels.hip -DIVP_FAST=0 &
run fma         rk_kernels.hip -DIVP_FAST=1 &
run strict_res  rk_kernels.hip -DIVP_FAST=0 -DIVP_HOIST=1 -DIVP_MIN_WAVES=1 &
run fma_res     rk_kernels.hip -DIVP_FAST=1 -DIVP_HOIST=1 -DIVP_MIN_WAVES=1 &
wait
run bdf_strict  rk_bdf.hip -DIVP_FAST=0 &
run bdf_fma     rk_bdf.hip -DIVP_FAST=1 &
run group_strict rk_group.hip -DIVP_FAST=0 &
run group_fma   rk_group.hip -DIVP_FAST=1 &
wait
# the two-waves-per-SIMD BDF build (ivp_amd/csrc/Makefile: *_occ2), whose kernels sit closest to the register limit
run bdf_occ2_strict rk_bdf.hip -DIVP_FAST=0 -DIVP_BDF_MIN_WAVES=2 -mllvm -disable-machine-licm &
run bdf_occ2_fma rk_bdf.hip -DIVP_FAST=1 -DIVP_BDF_MIN_WAVES=2 -mllvm -disable-machine-licm &
run radau_strict rk_radau.hip -DIVP_FAST=0 &
# the mass-matrix instantiations of the Radau kernels (hiprtc modules only): tools/radau_dae_resources.hip, n = 1, 2, 3, 5, 8
run radau_dae "$TOOLS/radau_dae_resources.hip" -DIVP_FAST=0 -I. &
wait
run radau_group_strict rk_radau_group.hip -DIVP_FAST=0 &
# the group-per-trajectory Radau kernels (radau_group.h) at n = 9, 16, 32, 33, 64: tools/radau_group_resources.hip
run radau_group "$TOOLS/radau_group_resources.hip" -DIVP_FAST=0 -I. &
# ... and their mass-matrix instantiations (mass_col functor, hiprtc modules only): tools/radau_group_dae_resources.hip
run radau_group_dae "$TOOLS/radau_group_dae_resources.hip" -DIVP_FAST=0 -I. &
wait
# the wide form of the group Radau kernels (64 < n <= 512, hiprtc modules only) at n = 65, 128, 129, 257, 512:
# tools/radau_wide_resources.hip
run radau_wide "$TOOLS/radau_wide_resources.hip" -DIVP_FAST=0 -I. &
# the Radau kernels of problems with event functions (the built-ins are in radau_strict above): the thread form at n = 8 and
# n = 5 with a mass matrix, the group form at n = 16 and 64: tools/radau_events_resources.hip
run radau_events "$TOOLS/radau_events_resources.hip" -DIVP_FAST=0 -I. &
run radau_events_group "$TOOLS/radau_events_resources.hip" -DIVP_FAST=0 -DIVP_RES_GROUP -I. &
wait
# the band form of the group Radau kernels (radau_band.h, hiprtc modules only): a tridiagonal system at n = 12, 40, 65, 130,
# 512 and ml = mu = 8 at n = 100: tools/radau_band_resources.hip
run radau_band "$TOOLS/radau_band_resources.hip" -DIVP_FAST=0 -I. &
wait
