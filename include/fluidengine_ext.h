/*
 * fluidengine_ext.h — HIP-engine extensions, not part of the oracle ABI.
 *
 * include/fluidengine.h is the symbol set that the HIP library AND the two CPU oracle libraries export.  What only
 * fluidlab_amd/csrc/libfluidengine_hip.so has is declared here; a caller looks these names up on that library alone
 * (fluidlab_amd/_capi.py: EXT_SYMBOLS).  Conventions are those of fluidengine.h: 0 on success, fe_last_error() otherwise.
 *
 * Material-parameter gradients
 * ----------------------------
 * d loss / d mu[p], d loss / d lam[p], d loss / d rho[p] for the per-particle values given to fe_init_particles.  The
 * reference has no counterpart: its mu, lam and rho fields carry no needs_grad (mpm_simulator.py:73-135).
 *
 *   fe_set_option(h, "param_grad", 1)   turns the pass on: every backward substep (fe_substep_grad, fe_step_grad) then adds its
 *                                       contribution to three fp64 accumulators of N entries each, by particle id.  They are allocated
 *                                       and zeroed the first time the option is set.  fe_get_option reports it.  Refused for scenes
 *                                       with MAT_RIGID particles (their density also enters the shape-matching centre of mass);
 *                                       fe_step_grad_batch refuses engines that have it on (no batched form).
 *   fe_reset_grad(h)                    also zeroes the accumulators (like every other adjoint); fe_reset_grad_till_frame does not.
 *
 * A sweep accumulates: after fe_reset_grad, seeding the loss adjoints and the fe_step_grad calls back to frame 0, the
 * accumulators hold the derivative of the loss over all substeps of the sweep.  Out of scope: batched environments, MAT_RIGID
 * bodies, derivatives with respect to p_vol, dt, gravity, the yield bounds or collider friction.
 */
#ifndef FLUIDENGINE_EXT_H
#define FLUIDENGINE_EXT_H

#include "fluidengine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* [N] each, in the caller's particle order; any pointer may be NULL (skipped).  Waits for the engine's stream. */
int fe_param_grad_get(FeEngine* h, double* g_mu, double* g_lam, double* g_rho);
/* the same into DEVICE pointers (memory of the engine's own device) */
int fe_param_grad_get_dev(FeEngine* h, double* g_mu, double* g_lam, double* g_rho);
/* zero the three accumulators and nothing else */
int fe_param_grad_reset(FeEngine* h);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDENGINE_EXT_H */
