/* Stand-alone client of the Radau settings / validation code of libivp_hip (include/ivp_hip.h): no GPU, no context.
 * Meant to be linked against a host build of ivp_capi.cpp with -fsanitize=address,undefined
 * (make -C ivp_amd/csrc radau_check_asan), where every call below runs under both sanitizers. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ivp_hip.h"

static int failures = 0;

static void expect(const char *what, int got, int want, const char *msg, const char *needle)
{
    const int ok = got == want && (!needle || strstr(msg, needle) != NULL);
    printf("%-44s rc = %4d (want %4d)  %s%s\n", what, got, want, msg, ok ? "" : "   <-- FAILED");
    if (!ok) failures += 1;
}

int main(void)
{
    ivp_problem_t prob;
    ivp_options_t opt;
    ivp_radau_settings_t s;
    char msg[16];          /* deliberately short: the message must be truncated, not overrun */
    char big[512];
    memset(&prob, 0, sizeof prob);
    prob.rhs_id = IVP_RHS_VDP_EPS;
    prob.n = 2;
    prob.n_params = 1;
    ivp_options_default(&opt);

    memset(&s, 0xAB, sizeof s);
    ivp_radau_settings_default(&s);
    ivp_radau_settings_default(NULL);
    if (s.uround != 2.3e-16 || s.safety_factor != 0.9 || s.scale_min != 0.2 || s.scale_max != 8.0 || s.newton_maxiter != 7 ||
        s.has_newton_tol != 0 || s.predictive != 1 || s.reserved != 0 || s.newton_tol != 0.0) {
        printf("ivp_radau_settings_default: wrong defaults   <-- FAILED\n");
        failures += 1;
    }

    big[0] = 0;
    expect("defaults", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_OK, big, NULL);
    expect("NULL settings = defaults", ivp_radau_check(&prob, 4, &opt, NULL, big, sizeof big), IVP_OK, big, NULL);
    expect("NULL message buffer", ivp_radau_check(&prob, 4, &opt, &s, NULL, 0), IVP_OK, "", NULL);
    expect("NULL problem", ivp_radau_check(NULL, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);
    expect("NULL options", ivp_radau_check(&prob, 4, NULL, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);
    expect("B = 0", ivp_radau_check(&prob, 0, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);

    s.uround = 1.0;
    expect("uround = 1", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_OUT_OF_RANGE, big, "uround");
    expect("... into a 16-byte buffer", ivp_radau_check(&prob, 4, &opt, &s, msg, sizeof msg), IVP_ERR_OUT_OF_RANGE, msg, NULL);
    if (strlen(msg) != sizeof msg - 1) { printf("message not truncated to the buffer   <-- FAILED\n"); failures += 1; }
    ivp_radau_settings_default(&s);
    s.safety_factor = 1e-5;
    expect("safety_factor = 1e-5", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_OUT_OF_RANGE, big, "safety_factor");
    ivp_radau_settings_default(&s);
    s.scale_max = 0.1;
    expect("scale_max < scale_min", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_INVALID_SCALE_FACTORS, big, NULL);
    s.scale_max = NAN;
    expect("scale_max = NaN", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_INVALID_SCALE_FACTORS, big, NULL);
    ivp_radau_settings_default(&s);
    s.newton_maxiter = 0;
    expect("newton_maxiter = 0", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_MUST_BE_POSITIVE, big, "newton_maxiter");
    s.newton_maxiter = -2147483647 - 1;
    expect("newton_maxiter = INT_MIN", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_MUST_BE_POSITIVE, big, NULL);
    s.newton_maxiter = 2147483647;
    expect("newton_maxiter = INT_MAX", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_OUT_OF_RANGE, big, "newton_maxiter");
    s.newton_maxiter = 15;
    s.has_newton_tol = 1;
    s.newton_tol = 1e-3;
    s.predictive = 0;
    expect("newton_maxiter = 15, explicit newton_tol", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_OK, big, NULL);
    ivp_radau_settings_default(&s);

    opt.has_first_step = 1;
    opt.first_step = 0.0;
    expect("first_step = 0", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_INVALID_STEP_SIZE, big, NULL);
    ivp_options_default(&opt);
    opt.rtol = -1.0;
    expect("rtol < 0", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_NEGATIVE_TOLERANCE, big, NULL);
    ivp_options_default(&opt);
    {
        double rv[3] = {1e-6, 1e-6, 1e-6};
        opt.rtol_vec = rv;
        opt.rtol_vec_len = 3;
        expect("rtol_vec of 3 for n = 2", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_TOLERANCE_SIZE_MISMATCH, big, NULL);
        ivp_options_default(&opt);
    }
    opt.fp_mode = IVP_FP_FAST;
    expect("fp_mode = FMA", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    ivp_options_default(&opt);
    opt.variant = 3;
    expect("variant = 3", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    ivp_options_default(&opt);
    prob.rhs_id = IVP_RHS_SHO_EV;
    prob.n = 2;
    prob.n_params = 0;
    expect("a problem with an event function", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    prob.rhs_id = IVP_RHS_LINEAR_DECAY_100;
    prob.n = 100;
    expect("n = 100", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    prob.rhs_id = 12345;
    expect("unknown rhs_id", ivp_radau_check(&prob, 4, &opt, &s, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);

    prob.rhs_id = IVP_RHS_VDP_EPS;
    prob.n = 2;
    prob.n_params = 1;
    opt.method = IVP_RADAU;
    expect("ivp_options_check: method = RADAU", ivp_options_check(&prob, 4, &opt, big, sizeof big), IVP_ERR_UNSUPPORTED_METHOD, big, "RADAU");
    expect("the solve entry points without a context", ivp_radau_solve(NULL, &prob, 4, NULL, NULL, NULL, 1, NULL, 1, &opt, &s, NULL),
           IVP_ERR_BAD_ARGUMENT, "", NULL);
    expect("", ivp_radau_solve_device(NULL, &prob, 4, NULL, NULL, NULL, 1, NULL, 1, &opt, &s, NULL, NULL), IVP_ERR_BAD_ARGUMENT, "", NULL);

    printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
