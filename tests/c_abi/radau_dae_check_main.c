/* Stand-alone client of the Radau DAE validation of libivp_hip (include/ivp_hip.h: ivp_radau_dae_check): no GPU, no context.
 * Every rule of the reference's partition check (radau.rs:210-246), the "not yet" refusals, NULL arguments.
 * tests/test_radau_dae_abi_cpu.py builds it with gcc against the library and runs it. */
#include <stdio.h>
#include <string.h>

#include "ivp_hip.h"

static int failures = 0;

static void expect(const char *what, int got, int want, const char *msg, const char *needle)
{
    const int ok = got == want && (!needle || strstr(msg, needle) != NULL);
    printf("%-52s rc = %4d (want %4d)  %s%s\n", what, got, want, msg, ok ? "" : "   <-- FAILED");
    if (!ok) failures += 1;
}

static ivp_radau_dae_t part(int h1, int n1, int h2, int n2, int h3, int n3)
{
    ivp_radau_dae_t d;
    memset(&d, 0, sizeof d);
    d.has_nind1 = h1; d.nind1 = n1;
    d.has_nind2 = h2; d.nind2 = n2;
    d.has_nind3 = h3; d.nind3 = n3;
    return d;
}

int main(void)
{
    ivp_problem_t prob;
    ivp_options_t opt;
    ivp_radau_settings_t s;
    ivp_radau_dae_t d;
    char msg[16];          /* deliberately short: the message must be truncated, not overrun */
    char big[512];
    memset(&prob, 0, sizeof prob);
    prob.rhs_id = IVP_RHS_ROBERTSON;   /* n = 3, no mass matrix */
    prob.n = 3;
    prob.n_params = 0;
    ivp_options_default(&opt);
    ivp_radau_settings_default(&s);
    if (sizeof(ivp_radau_dae_t) != 32 || sizeof(ivp_radau_settings_t) != 56) {
        printf("struct sizes   <-- FAILED\n");
        failures += 1;
    }

    big[0] = 0;
    expect("NULL dae: a pure ODE partition", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_OK, big, NULL);
    expect("NULL settings and NULL dae", ivp_radau_dae_check(&prob, 4, &opt, NULL, NULL, big, sizeof big), IVP_OK, big, NULL);
    expect("NULL message buffer", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, NULL, 0), IVP_OK, "", NULL);
    expect("NULL problem", ivp_radau_dae_check(NULL, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);
    expect("NULL options", ivp_radau_dae_check(&prob, 4, NULL, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, NULL);
    d = part(0, 77, 0, 77, 0, 77);
    expect("none given (the values are not read)", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_OK, big, NULL);
    d = part(1, 3, 0, 0, 0, 0);
    expect("nind1 = n alone", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_OK, big, NULL);
    d = part(1, 3, 1, 0, 1, 0);
    expect("(3, 0, 0) in full", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_OK, big, NULL);
    d = part(0, 0, 1, 0, 0, 0);
    expect("nind2 = 0, nind1 inferred", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_OK, big, NULL);

    d = part(1, 2, 0, 0, 0, 0);
    expect("nind1 = 2 alone: the sum is not n", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, "partition");
    expect("... into a 16-byte buffer", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, msg, sizeof msg), IVP_ERR_INVALID_DAE_PARTITION, msg, NULL);
    if (strlen(msg) != sizeof msg - 1) { printf("message not truncated to the buffer   <-- FAILED\n"); failures += 1; }
    d = part(1, 2, 1, 1, 1, 1);
    expect("(2, 1, 1): the sum is 4", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);
    d = part(0, 0, 1, 2, 1, 2);
    expect("nind1 omitted, nind2 + nind3 > n", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);
    d = part(0, 0, 1, -1, 0, 0);
    expect("a negative count", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);
    d = part(1, 4, 1, -1, 0, 0);
    expect("a negative count that makes the sum n", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);
    d = part(0, 0, 1, 2147483647, 1, 2147483647);
    expect("counts whose sum overflows int", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);

    d = part(0, 0, 1, 1, 0, 0);
    expect("index-2 variables without a mass matrix", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    d = part(1, 1, 1, 1, 1, 1);
    expect("index-3 variables without a mass matrix", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");

    /* the partition is checked before the step size (radau.rs:210-261), after the struct's own fields */
    opt.has_first_step = 1;
    opt.first_step = 0.0;
    d = part(1, 2, 0, 0, 0, 0);
    expect("bad partition and first_step = 0", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_INVALID_DAE_PARTITION, big, NULL);
    expect("first_step = 0", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_INVALID_STEP_SIZE, big, NULL);
    ivp_options_default(&opt);
    s.newton_maxiter = 0;
    expect("bad partition and newton_maxiter = 0", ivp_radau_dae_check(&prob, 4, &opt, &s, &d, big, sizeof big), IVP_ERR_MUST_BE_POSITIVE, big, NULL);
    ivp_radau_settings_default(&s);

    /* the refusals of the plain Radau call apply unchanged */
    opt.fp_mode = IVP_FP_FAST;
    expect("fp_mode = FMA", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    ivp_options_default(&opt);
    opt.variant = 3;
    expect("variant = 3", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    ivp_options_default(&opt);
    prob.rhs_id = IVP_RHS_SHO_EV;
    prob.n = 2;
    expect("a problem with an event function", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");
    prob.rhs_id = IVP_RHS_LINEAR_DECAY_100;
    prob.n = 100;
    expect("n = 100", ivp_radau_dae_check(&prob, 4, &opt, &s, NULL, big, sizeof big), IVP_ERR_BAD_ARGUMENT, big, "not yet");

    prob.rhs_id = IVP_RHS_ROBERTSON;
    prob.n = 3;
    expect("the solve entry points without a context", ivp_radau_solve_dae(NULL, &prob, 4, NULL, NULL, NULL, 1, NULL, 1, &opt, &s, NULL, NULL),
           IVP_ERR_BAD_ARGUMENT, "", NULL);
    expect("", ivp_radau_solve_dae_device(NULL, &prob, 4, NULL, NULL, NULL, 1, NULL, 1, &opt, &s, NULL, NULL, NULL), IVP_ERR_BAD_ARGUMENT, "", NULL);

    printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
