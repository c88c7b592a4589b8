// ivp_jit.h -- run-time compiled right-hand sides (hiprtc): the device-side `impl IVP for T`.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "ivp_kargs.h"

// col_ptr / row_idx: optional Jacobian sparsity pattern (CSC, one per problem; ivp_rhs_compile_sparse)
int ivp_jit_compile(int device, const char *ode_source, int n, int n_params, int n_events, unsigned flags, void **handle, std::string *log,
                    const int32_t *col_ptr = nullptr, const int32_t *row_idx = nullptr);
int ivp_jit_n_events(void *handle);
bool ivp_jit_has_mass(void *handle);   // compiled with IVP_RHS_HAS_MASS or IVP_RHS_HAS_MASS_COL: honoured by the Radau DAE call only
void ivp_jit_free(void *handle);
// banded storage (IVP_RHS_BANDED): true and the bandwidths for a banded problem; lds_fits: the factors of a trajectory fit
// the LDS budget of the banded kernels (bdf_band.h)
bool ivp_jit_band(void *handle, int *ml, int *mu, bool *lds_fits);
bool ivp_jit_has_sparsity(void *handle);   // compiled with a jac_sparsity pattern (ivp_rhs_compile_sparse)
void ivp_jit_dims(void *handle, int *n, int *n_params);
const char *ivp_jit_last_log(void *handle);   // hiprtc build log / load error of the most recent failure
hipError_t ivp_jit_launch(void *handle, int what, int method, int fp_mode, int full, const IvpKArgs &a,
                          uint32_t lanes, hipStream_t s);
