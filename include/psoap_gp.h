/*
 * psoap_gp.h -- C ABI of the MI355X (gfx950) Gaussian-process likelihood library.
 *
 * This is the drop-in boundary for PSOAP's dense GP hot path.  The reference has
 * no FFI: the path sits behind Python functions taking NumPy arrays
 * (psoap/covariance.py, psoap/matrix_functions.pyx).  Each entry point below
 * names the reference interface it replaces (paths relative to the reference
 * tree).  Host code (the psoap_amd Python package, or a maintainer's ctypes stub -- see
 * INTEGRATION.md) binds these symbols; there are no torch types, only plain
 * pointers and sizes.  All arrays are C-contiguous fp64 on the HOST unless a
 * parameter is documented as device-resident.
 *
 * Return value: 0 on success, non-zero on a runtime/HIP error (message via
 * psoap_last_error()).  Numerical failure is NOT an error: a non positive-
 * definite matrix or a negative amp/l yields -inf in the output, exactly like
 * psoap/covariance.py:317-318,326-327.
 *
 * Threading: a handle may be used by one host thread at a time.  HIP is
 * initialised lazily by the first call in the calling process (safe after
 * fork(), as psoap/sample_parallel.py:258-278 requires).
 *
 * Several processes on one GPU (that reference's worker-per-chunk model with
 * more chunks than GPUs, psoap/sample_parallel.py:258-278):
 *   - the library serves them in turn: an advisory lock on
 *     <dir>/gpu_<PCI bus id>.lock is held from an upload to the fetch / sync of
 *     the evaluation that reads it, by every other call that touches the device
 *     for its duration, and by a stream while it has tickets outstanding
 *     (released only once its resident launch has left the device when other
 *     processes are there).  <dir> = $PSOAP_LOCK_DIR, else
 *     $XDG_RUNTIME_DIR/psoap, else /tmp/psoap-<uid>: per user, 0700.  Within a
 *     process the lock is counted.  A wait longer than
 *     PSOAP_DEVICE_LOCK_TIMEOUT_S (300) is an error that names the holder.
 *   - the processes on the device are counted: slot files beside the lock, and
 *     where the driver lists them (/sys/class/kfd/kfd/proc/<pid>/queues/<q>/gpuid)
 *     every process with a hardware queue on the device, library or not;
 *   - every persistent launch reports workgroups that the device's scheduler
 *     moved between compute units while a task ran (the one disturbance its
 *     hand-off protocol does not survive): such an evaluation is
 *     run again (PSOAP_SHARE_RETRIES, 3; bit-identical when clean), then by the
 *     staged path (kernel boundaries only).  Measured clean up to 8 processes per device
 *     (0 wrong in 246,000 evaluations, rounds 4-5); the check sees a workgroup that is
 *     somewhere else at the end of a task than at its start, not one that moved and came back;
 *   - with PSOAP_DEVICE_LOCK=0 and several processes on the device, or more
 *     than PSOAP_SHARE_DAG_MAX (8) of them, evaluations take the staged path
 *     from the start and without the lock (kernel boundaries only: immune, and
 *     the device interleaves the processes' kernels); psoap_stream_open is
 *     refused there.  PSOAP_SHARE_POLICY=dag|staged pins the path.
 *   psoap_share_stats reports what all this cost.
 */
#ifndef PSOAP_GP_H
#define PSOAP_GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psoap_chunk psoap_chunk; /* opaque per-chunk device state */

/* ---- library ---------------------------------------------------------------- */
int psoap_version(void);
const char *psoap_last_error(void);
int psoap_device_count(int *count);

/* What sharing a device with other processes has cost THIS process so far
 * (process-wide counters; out[k], k < min(n, PSOAP_SHARE_N)). */
enum {
    PSOAP_SHARE_PROCS = 0,            /* processes with a slot on the device now (this one included) */
    PSOAP_SHARE_DAG_LAUNCHES = 1,     /* persistent launches issued */
    PSOAP_SHARE_TAINTED = 2,          /* ... that reported a moved workgroup (results withheld) */
    PSOAP_SHARE_RETRIES = 3,          /* evaluations issued again because of that */
    PSOAP_SHARE_STAGED_FALLBACKS = 4, /* evaluations that went to the staged path after the retries */
    PSOAP_SHARE_STAGED_POLICY = 5,    /* evaluations sent down the staged path from the start */
    PSOAP_SHARE_MOVED_TASKS = 6,      /* tasks that ended on another compute unit than they started on */
    PSOAP_SHARE_MOVED_XCD = 7,        /* ... on another XCD */
    PSOAP_SHARE_LOCK_ACQUISITIONS = 8,
    PSOAP_SHARE_LOCK_WAIT_US = 9,
    PSOAP_SHARE_STREAM_RESUBMITS = 10,
    PSOAP_SHARE_LOCK_ENABLED = 11,
    PSOAP_SHARE_N = 12
};
int psoap_share_stats(int device, long long *out, int n);

/* Launches of the persistent kernel per built form so far (process-wide, all
 * devices): out[k], k < min(n, forms); returns the number of forms (24).
 *   likelihood and predict: k = 9*AUG + 3*(C-1) + {0 throughput, 1 LAT, 2 LAT wide}
 *                           (AUG: 0 likelihood, 1 predict)
 *   resident stream:        k = 18 + 2*(C-1) + {0 throughput, 1 LAT}
 * out may be NULL. */
int psoap_dag_form_launches(long long *out, int n);

/* ---- per-chunk handle ---------------------------------------------------------
 * Replaces the per-chunk state of Worker.initialize (psoap/sample_parallel.py:
 * 126-166): fl, sigma and the N x N scratch matrix V11 (:163) live on the device
 * for the life of the handle; max_batch matrices are pre-allocated so that
 * max_batch proposals can be evaluated concurrently. */
int psoap_chunk_create(psoap_chunk **out, int device, int N, const double *fl,
                       const double *sigma, int max_batch);
int psoap_chunk_destroy(psoap_chunk *h);
int psoap_chunk_set_data(psoap_chunk *h, const double *fl, const double *sigma);
/* Observed-frame grid for the device-side Doppler shift
 * (replicate_wls, psoap/data.py:40-63): lwl[N], epoch[N] in [0, n_epochs). */
int psoap_chunk_set_grid(psoap_chunk *h, const double *lwl, const int32_t *epoch,
                         int n_epochs);

/* ---- lnlike -------------------------------------------------------------------
 * lnlike_f / lnlike_f_g / lnlike_f_g_h (psoap/covariance.py:299-376), c = 1,2,3.
 *   lwl : (c, N) rest-frame ln-wavelengths (the *lwls splat of
 *         sample_parallel.py:193); gp : (amp_0, l_0, amp_1, l_1, ...).
 *   out : -0.5 * (r^T K^-1 r + logdet K), r = fl - mu_GP; -inf conventions above. */
int psoap_lnlike(psoap_chunk *h, int c, const double *lwl, const double *gp,
                 double mu_GP, double *out);
/* B proposals at once: lwl (B, c, N), gp (B, 2c), out (B).  B <= max_batch. */
int psoap_lnlike_batch(psoap_chunk *h, int B, int c, const double *lwl,
                       const double *gp, double mu_GP, double *out);

/* ---- gradient of lnlike -------------------------------------------------------
 * Value and analytic gradient for B proposals: lwl (B, c, N), gp (B, 2c) as for
 * psoap_lnlike_batch; B is NOT bound by max_batch.
 *   lnp      (B)       the value, summed in the order of the staged path (a few ulp
 *                      from psoap_lnlike, which may run another scheme);
 *   grad_gp  (B, 2c)   d lnp / d (amp_0, l_0, amp_1, l_1, ...);
 *   grad_lwl (B, c, N) d lnp / d lwl[c][i]; may be NULL;
 *   grad_mu  (B)       d lnp / d mu_GP; may be NULL.
 * With alpha = K^-1 r and Q = alpha alpha^T - K^-1 the gradient is 1/2 sum_ij Q_ij
 * dK_ij; the staged factorisation runs on [K | I], which leaves W = U^-T beside the
 * factor (K^-1 = W^T W), and one fused kernel contracts the tiles of Q with the
 * covariance derivatives without ever storing K^-1 (csrc/grad_kernels.hpp; N^3
 * flops in all).  No atomics: the same arguments give the same bits, alone or in
 * any batch.
 * Conventions: a negative hyper-parameter or a matrix that is not positive
 * definite gives lnp = -inf and NaN in every gradient entry of that proposal; the
 * status is non-zero for runtime errors only.
 * Workspace: 16 Npad^2 bytes per matrix (Npad = N rounded up to 128), allocated by
 * the first call, kept with the handle and freed by psoap_chunk_grad_release or
 * psoap_chunk_destroy.  The proposals are walked in groups of at most 8 matrices
 * and at most 1 GiB of that storage (never less than one matrix), so the
 * workspace does not grow with B.  The handle's uploaded batches, their results
 * and the likelihood workspaces are left as they are. */
int psoap_chunk_lnlike_grad(psoap_chunk *h, int B, int c, const double *lwl,
                            const double *gp, double mu_GP, double *lnp,
                            double *grad_gp, double *grad_lwl, double *grad_mu);
int psoap_chunk_grad_release(psoap_chunk *h);

/* ---- time-variable component spectra: a temporal factor in the GP kernel -------------
 * Model: each component's squared exponential in ln-wavelength times one in observation
 * time, with a time scale tau_c (days) per component:
 *   K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2) + sigma_i^2 delta_ij
 *   d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2
 *   dt_ij = t[j] - t[i],      q_c = -1/2 / tau_c^2
 * tau_c = +inf is the static model of psoap_chunk_lnlike_grad; a finite tau_c lets that
 * component's spectrum drift from epoch to epoch.
 *
 * psoap_chunk_set_times: t (N), the observation time of every pixel in days, copied to
 * the device and kept with the handle as fl and sigma are.  Any order: a pixel-permuted
 * chunk is legal.  Pass times from which a constant (their minimum) has been taken, so
 * that the differences are formed from small numbers.  Refused on an open stream.
 *
 * psoap_chunk_lnlike_tv_grad: lwl (B, c, N), gp (B, 2c) and the outputs lnp, grad_gp,
 * grad_lwl (may be NULL), grad_mu (may be NULL) as for psoap_chunk_lnlike_grad; tau (B, c)
 * and grad_tau (B, c) = d lnp / d tau_c.  With Q = alpha alpha^T - K^-1 and
 * e_cij = exp(p_c d_cij^2 + q_c dt_ij^2) the formulas of psoap_chunk_lnlike_grad hold
 * with that e, and
 *   d lnp / d tau_c = 1/2 a_c^2 / tau_c^3 sum_ij Q_ij e_cij dt_ij^2
 * One exp per element and component: the argument is evaluated as a = p * d * d, then
 * a = a + q * dt * dt, without contraction, and the underflow shortcut works on the sum
 * (csrc/fill_kernels.hpp, TV).  The factorisation, alpha and the product are those of
 * psoap_chunk_lnlike_grad; no atomics, the same arguments give the same bits alone or in
 * any batch.
 * Bit-identity at tau = inf: q = -0, the added term is -0 and a keeps its bits, so with
 * every tau_c = +inf lnp, grad_gp, grad_lwl and grad_mu have the bits
 * psoap_chunk_lnlike_grad returns on the same handle, and grad_tau is exactly 0.
 * grad_gp == NULL asks for the value only: grad_tau, grad_lwl and grad_mu must then be
 * NULL too, the contraction is skipped, and lnp has the bits of a call that asks for the
 * gradient.  With grad_gp, grad_tau is required.
 * Conventions: tau_c <= 0 or NaN, a negative hyper-parameter or a matrix that is not
 * positive definite gives lnp = -inf and NaN in every gradient entry of that proposal;
 * the other proposals keep their bits; tau_c = +inf is valid.  The status is non-zero
 * for runtime and argument errors only: a call before psoap_chunk_set_times, on a handle
 * with an open stream, or on a handle with a baseline (psoap_chunk_set_baseline: the
 * combination with the marginalised continuum is not built) is refused with a message.
 * Workspace: that of psoap_chunk_lnlike_grad, walked in the same groups (at most 8
 * matrices and 1 GiB), plus 3 doubles per matrix of a group for tau and for grad_tau and
 * one double more per tile record; psoap_chunk_grad_release frees all of it, the times
 * stay with the handle. */
int psoap_chunk_set_times(psoap_chunk *h, const double *t);
int psoap_chunk_lnlike_tv_grad(psoap_chunk *h, int B, int c, const double *lwl,
                               const double *gp, const double *tau, double mu_GP,
                               double *lnp, double *grad_gp, double *grad_tau,
                               double *grad_lwl, double *grad_mu);

/* ---- quasi-periodic temporal factor: value and gradient ------------------------------
 * (not in the reference.)  The time-variable kernel forgets; the line-profile variability
 * of a spotted, rotating star repeats with the rotation period and decays over the spot
 * lifetime.  The decaying factor is multiplied by a periodic one:
 *   K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2 - Gamma_c sin^2(pi dt_ij / P_c))
 *          + sigma_i^2 delta_ij
 * over the times of psoap_chunk_set_times; Gamma_c >= 0 is dimensionless, P_c > 0 in days.
 * Gamma_c = 0 is the time-variable model of psoap_chunk_lnlike_tv_grad, and with
 * tau_c = +inf as well the static one; tau_c = +inf with Gamma_c > 0 is purely periodic.
 *
 * psoap_chunk_lnlike_qp_grad: lwl, gp, tau, lnp, grad_gp, grad_tau, grad_lwl (may be NULL),
 * grad_mu (may be NULL) as for psoap_chunk_lnlike_tv_grad; gamma, period (B, c) and
 * grad_gamma, grad_period (B, c).  With e_cij the exponential above the formulas of
 * psoap_chunk_lnlike_tv_grad hold with that e, and
 *   d lnp / d Gamma_c = -1/2 a_c^2 sum_ij Q_ij e_cij sin^2(pi dt_ij / P_c)
 *   d lnp / d P_c     =  1/2 a_c^2 Gamma_c pi / P_c^2 sum_ij Q_ij e_cij dt_ij sin(2 pi dt_ij / P_c)
 * Still one exp per element and component: the argument is a = p * d * d, a = a + q * dt * dt,
 * u = dt * rP with rP = 1 / P rounded once, sincospi(u, &s, &co), a = a + ng * s * s with
 * ng = -Gamma, without contraction (csrc/fill_kernels.hpp, QP); the contraction rebuilds it
 * the same way and takes sin(2 pi dt / P) = 2 s co from sincospi of the same rounded u.  No atomics: the same
 * arguments give the same bits alone or in any batch.
 * Bit-identity.  At Gamma_c = 0 the added term is -0 for every finite s: whatever P, lnp,
 * grad_gp, grad_tau, grad_lwl and grad_mu have the bits psoap_chunk_lnlike_tv_grad returns
 * on the same handle, grad_period is exactly 0, and grad_gamma is the score of a test for
 * periodicity.  At dt = 0, s = +0 exactly: pixels of one epoch see the static kernel.
 * grad_gp == NULL asks for the value only: every other gradient must then be NULL, and lnp
 * has the bits of a call that asks for the gradient.  With grad_gp, grad_tau, grad_gamma
 * and grad_period are required.
 * Conventions: Gamma_c < 0, NaN or inf, P_c <= 0, NaN, inf or with 1 / P_c not finite, tau_c <= 0 or NaN, a negative
 * hyper-parameter or a matrix that is not positive definite gives lnp = -inf and NaN in
 * every gradient entry of that proposal; the other proposals keep their bits.  A call
 * before psoap_chunk_set_times, on a handle with an open stream or on a handle with a
 * baseline is refused with a message.  Not built under this kernel: the batch / lnprob(p)
 * route, Fisher, leave-one-out, predict, draws, the mixture, the marginalised continuum and
 * the persistent kernel.
 * Workspace: that of psoap_chunk_lnlike_tv_grad plus 3 doubles per matrix of a group for
 * each of gamma, period and their gradients and two doubles more per component in a tile
 * record; psoap_chunk_grad_release frees all of it. */
int psoap_chunk_lnlike_qp_grad(psoap_chunk *h, int B, int c, const double *lwl,
                               const double *gp, const double *tau, const double *gamma,
                               const double *period, double mu_GP, double *lnp,
                               double *grad_gp, double *grad_tau, double *grad_gamma,
                               double *grad_period, double *grad_lwl, double *grad_mu);

/* ---- gradient of lnprob(p): through the Kepler solve and the Doppler shift ----------
 * B proposals as for psoap_batch_upload_orbits (needs set_grid + set_dates); B is NOT
 * bound by max_batch.
 *   lnp      (B)               the value psoap_chunk_lnlike_grad gives on the grids
 *                              that psoap_orbit_velocities and the Doppler shift make;
 *   grad_orb (B, n_orb)        d lnp / d p_orb, registered order up to gamma;
 *   grad_gp  (B, 2c)           as for psoap_chunk_lnlike_grad;
 *   grad_vel (B, c, n_epochs)  d lnp / d v[c][epoch]; may be NULL;
 *   grad_mu  (B)               may be NULL.
 * Per group of matrices one kernel evaluates the velocities (the arithmetic and the
 * bits of psoap_orbit_velocities) and their Jacobian at the same converged E, by
 * implicit differentiation of Kepler's equation (csrc/orbit_grad_kernels.hpp); the
 * grids are shifted on the device, the gradient above runs untouched, and two small
 * kernels fold d lnp / d lwl over the pixels of every epoch
 * (grad_vel = -1/c_kms * the sum over the epoch's pixels; 0.0 for an epoch with no
 * pixel) and contract it with the Jacobian.  The (B, c, N) wavelength gradient never
 * leaves the device: the host ships n_orb + 2c doubles per proposal and receives
 * 1 + n_orb + 2c + 1.  No atomics in any sum: the order is fixed by the chunk alone.
 * Conventions: a proposal with some |v| >= c_kms, a negative hyper-parameter or a
 * matrix that is not positive definite gives lnp = -inf and NaN in every gradient
 * entry of that proposal; the other proposals of the batch keep the bits they have
 * alone; the status is non-zero for runtime errors only (an eccentricity outside
 * [0, 1) is one, as for psoap_batch_upload_orbits).  An open stream on the handle is
 * refused.  The workspace is that of psoap_chunk_lnlike_grad plus a few KB per
 * matrix (psoap_chunk_grad_release frees both), walked in the same groups.  The
 * handle's uploaded batches, their results and the likelihood workspaces are left
 * as they are. */
int psoap_chunk_lnprob_grad(psoap_chunk *h, int B, int model, const double *p_orb,
                            const double *gp, double mu_GP, double *lnp,
                            double *grad_orb, double *grad_gp, double *grad_vel,
                            double *grad_mu);
/* stand-alone, beside psoap_orbit_velocities: vel_out (B, c, n_dates) with the bits of
 * psoap_orbit_velocities, jac_out (B, c, n_dates, n_orb) = d v / d p_orb; entries of
 * parameters a component does not depend on are exact zeros. */
int psoap_orbit_velocity_jacobian(int device, int model, int B, const double *p_orb,
                                  int n_dates, const double *dates, double *vel_out,
                                  double *jac_out);

/* ---- Fisher information of the likelihood ----------------------------------------
 * For one matrix (lwl (c, N), gp (2c)) and T tangents in (grid, hyper-parameter)
 * space -- tan_lwl (T, c, N), or NULL for zeros, and tan_gp (T, 2c), a tangent's
 * covariance derivative being, with d = lwl[c][n] - lwl[c][m] and e = exp(p_c d^2),
 *   K_t[m][n] = sum_c e (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc
 *                        + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m])) --
 *   fisher    (T, T)  F_st = 1/2 tr(K^-1 K_s K^-1 K_t), both triangles, F == F^T bit
 *                     for bit;
 *   fisher_mu (1)     1^T K^-1 1, the information of mu_GP (its cross terms with the
 *                     other parameters are zero in expectation); may be NULL.
 * F does not depend on the data.  The factorisation of [K | I] runs as for the
 * gradient, in the gradient's workspace for one matrix; K^-1 = W^T W is stored, and
 * per tangent K_t, Z = K_t K^-1 and the upper tiles of G_t = 1/2 (K^-1 Z + Z^T K^-1)
 * follow, G_t contracted in the accumulators with the derivative of K in every
 * parameter (csrc/fisher_kernels.hpp; (1 + 4 T) N^3 flops).  No atomics, every sum in an order
 * fixed by (N, c, T): the same arguments give the same bits, and a subsequence of
 * the tangents gives the bits of the entries it shares.
 * Conventions: a negative hyper-parameter or a matrix that is not positive definite
 * gives NaN in every output and status 0; T < 1 or T > 32 and an open stream on the
 * handle are refused (non-zero status, psoap_last_error).
 * Workspace: 24 Npad^2 bytes (K^-1, K_t, Z) beyond the gradient's 16 Npad^2 for one
 * matrix, whatever T is, allocated by the first call, kept with the handle and freed
 * by psoap_chunk_fisher_release (the gradient's by psoap_chunk_grad_release) or
 * psoap_chunk_destroy.  The handle's uploaded batches, their results and the
 * likelihood workspaces are left as they are. */
int psoap_chunk_fisher(psoap_chunk *h, int c, const double *lwl, const double *gp,
                       int T, const double *tan_lwl, const double *tan_gp,
                       double *fisher, double *fisher_mu);
int psoap_chunk_fisher_release(psoap_chunk *h);

/* ---- Fisher information of the per-epoch radial velocities -------------------------
 * For one matrix (lwl (c, N), gp (2c), as for psoap_chunk_fisher) and the epoch of
 * every pixel (epoch (N), values in [0, n_epochs), any pixel order, an epoch may have no
 * pixel): the information of the c n_epochs velocities v[k][e] behind the grids
 * lwl[k][n] = lwl0[n] - v[k][epoch[n]] / c_kms, AT FIXED hyper-parameters,
 *   fisher (c E, c E)  F[(k, e), (j, f)] = 1/2 tr(K^-1 K_(k,e) K^-1 K_(j,f)), row
 *                      k * n_epochs + e (grad_vel's order), both triangles, F == F^T
 *                      bit for bit --
 * what psoap_chunk_fisher gives for the c E tangents dx = -1 / c_kms on component k,
 * epoch e, without its limit of 32 and at c + c (c + 1) / 2 dense products whatever
 * n_epochs is: a velocity tangent touches only the rows and columns of one epoch
 * (csrc/vel_fisher_kernels.hpp; (2 c + c (c + 1)) N^3 flops beyond the factorisation
 * of [K | I] and K^-1).  F has c null directions, the constant shift of each component
 * (the kernel is stationary): velocities are determined up to one offset per
 * component.  An epoch without pixels gives an exactly-zero row and column.  The cross
 * terms with the hyper-parameters stay with psoap_chunk_fisher.
 * No atomics, every sum in an order fixed by (N, c, epoch): the same arguments give the
 * same bits.
 * Conventions: a negative hyper-parameter or a matrix that is not positive definite
 * gives NaN in every entry and status 0; n_epochs < 1 or > 2048, an epoch index out of
 * range and an open stream on the handle are refused (non-zero status,
 * psoap_last_error).
 * Workspace: K^-1 in the Fisher workspace (8 Npad^2 bytes, psoap_chunk_fisher_release)
 * and, of its own, 16 c Npad^2 bytes (Dv_k, Z_k) + 4 c (c + 1) S^2 + 8 (c E)^2 bytes
 * (S: the slots of psoap_vel_fisher_plan), allocated by the first call, kept with the
 * handle and freed by psoap_chunk_fisher_vel_release or psoap_chunk_destroy.  S is
 * about Npad / 128 + n_epochs for an epoch-major chunk; for pixels in no epoch order it
 * is at most min(Npad, Npad / 128 * n_epochs), the bin sums then reach 4 c (c + 1) Npad^2
 * bytes and the binning epilogue up to 128 x 128 passes per tile (estimated at tenths of
 * a second to a second per call at N = 6000 .. 8192; csrc/vel_fisher_kernels.hpp): sort
 * the pixels by epoch.  n_epochs is capped at 2048 because fisher grows as (c E)^2
 * (302 MB at c = 3 there).  The
 * handle's uploaded batches, their results and the likelihood workspaces are left as
 * they are.  Launches are booked under PSOAP_K_FILL (Dv_k), GRAD (K^-1 and the
 * products), MISC (the rest) and the factorisation's own classes. */
int psoap_chunk_fisher_vel(psoap_chunk *h, int c, const double *lwl, const double *gp,
                           int n_epochs, const int32_t *epoch, double *fisher);
int psoap_chunk_fisher_vel_release(psoap_chunk *h);

/* ---- observed information of the per-epoch radial velocities ------------------------
 * Value, gradient, expected and OBSERVED information of the velocities of
 * psoap_chunk_fisher_vel (same lwl, gp, epoch, n_epochs, same order of rows) at the
 * handle's flux, from one factorisation:
 *   lnp                the likelihood, as psoap_lnlike returns it (marg: psoap_chunk_lnlike_marg)
 *   grad (c E)         dlnL/dv[k][e]
 *   fisher (c E, c E)  F; with marg = 0 the bits of psoap_chunk_fisher_vel
 *   observed (c E, c E)  J = -d2 lnL / dv dv = -F + U^T G U + T at the data, E[J] = F;
 *                      both triangles, J == J^T bit for bit
 * (csrc/vel_newton_kernels.hpp: one pass over the pixel pairs, c N^2 exponentials, and
 * 2 N^2 Tpad + N Tpad^2 flops of dense products, Tpad = c E rounded up to 128, beyond the
 * work of psoap_chunk_fisher_vel).  J has the c null directions of F; it need not be
 * positive semi-definite away from the optimum.  An epoch without pixels gives
 * exactly-zero rows, columns and gradient entries.
 * marg != 0: everything under the baseline of psoap_chunk_set_baseline, K + H Lambda H^T
 * in place of K and alpha_m in place of alpha (H does not depend on the velocities);
 * refused without a baseline.
 * No atomics, every sum in an order fixed by (N, c, epoch): the same arguments give the
 * same bits.
 * Conventions: a negative hyper-parameter or a matrix that is not positive definite
 * gives lnp = -inf, NaN in grad, fisher and observed and status 0; the refusals are
 * those of psoap_chunk_fisher_vel.
 * Workspace: that of psoap_chunk_fisher_vel (and under marg of the marginal gradient
 * for one matrix) and, of its own, 8 (c S Npad + 2 c S^2 + 2 Npad Tpad + Tpad^2 +
 * (c E)^2 + c E) bytes, freed by psoap_chunk_fisher_vel_release as well.  Launches are
 * booked under PSOAP_K_FILL (the pair pass), GRAD (the products) and MISC. */
int psoap_chunk_info_vel(psoap_chunk *h, int marg, int c, const double *lwl,
                         const double *gp, double mu_GP, int n_epochs, const int32_t *epoch,
                         double *lnp, double *grad, double *fisher, double *observed);
/* host twin of the plan of psoap_chunk_fisher_vel, which psoap_chunk_info_vel shares
 * (pure host): a slot is one of the distinct epochs of a
 * 128-row tile row, in ascending epoch id, numbered through the tile rows.  n_slots;
 * slot_of_out (N) the slot of every pixel; slot_first_out (ceil(N / 128) + 1);
 * slot_epoch_out (min(max_slots, n_slots)) the epoch of a slot; the tiles of a cross
 * product (all) and of a symmetrised one (upper); the bytes of every device buffer
 * beyond [K | I].  Any output may be NULL.  Returns 2 where psoap_chunk_fisher_vel
 * refuses c, n_epochs or epoch, and for N < 1. */
int psoap_vel_fisher_plan(int c, int N, int n_epochs, const int32_t *epoch, int *n_slots,
                          int *slot_of_out, int *slot_first_out, int *slot_epoch_out,
                          int max_slots, int *n_tiles_all, int *n_tiles_upper,
                          long long *bytes);

/* ---- leave-one-out cross-validation of the likelihood -----------------------------
 * For one matrix (lwl (c, N), gp (2c), as for psoap_chunk_fisher), with r = fl - mu_GP,
 * A = K^-1 and alpha = A r (K as psoap_lnlike builds it, noise on the diagonal: pix_var
 * is the predictive variance of the observed flux, not of the latent spectrum):
 *   lnp      (1)  the likelihood, with the bits of psoap_chunk_lnlike_grad;
 *   loo_logp (1)  sum_i pix_logp[i], summed in pixel order;
 *   pix_mean (N)  fl[i] - alpha[i] / A[i][i]: pixel i predicted from all the others;
 *   pix_var  (N)  1 / A[i][i];
 *   pix_logp (N)  1/2 log A[i][i] - alpha[i]^2 / (2 A[i][i]) - 1/2 log(2 pi);
 * and per epoch e with the n_e pixels I_e, s_e = A[I_e,I_e]^-1 alpha[I_e]:
 *   ep_resid (N)         s_e on the pixels of epoch e: fl[I_e] minus the prediction
 *                        of the epoch from all other epochs;
 *   ep_chi2  (n_epochs)  alpha[I_e] . s_e, chi-squared with n_e degrees of freedom
 *                        under the model;
 *   ep_logp  (n_epochs)  -1/2 ep_chi2 + 1/2 log det A[I_e,I_e] - n_e/2 log(2 pi);
 *   ep_npix  (n_epochs)  n_e; an epoch without pixels gives 0.0, 0.0, 0.
 * epoch == NULL: pixel outputs only; the ep_* pointers and n_epochs are ignored.
 * epoch (N) given: values in [0, n_epochs), every epoch's pixels one contiguous run
 * (the flattened, epoch-major order of Chunk.apply_mask; the runs in any order).
 * Any output pointer may be NULL.
 * The factorisation of [K | I] and alpha run as for the gradient, in the gradient's
 * workspace for one matrix.  Then one workgroup per tile of the band of W^T W that
 * meets an epoch's diagonal block scatters it into that epoch's packed block (square,
 * side n_e rounded up to 128, the identity on the padding); the packed blocks go
 * through the staged potrf / trsm / panel-update kernels as a batch, in groups of
 * equal padded side; one kernel finishes (csrc/loo_kernels.hpp).  diag(A) is read off
 * the packed blocks: pixel and epoch outputs rest on the same numbers, and the pixel
 * outputs have the same bits with and without an epoch index.  No atomics, every sum
 * in an order fixed by (N, c, epoch layout): the same arguments give the same bits.
 * Conventions: a negative hyper-parameter or a matrix that is not positive definite
 * gives lnp = -inf, NaN in every other floating output and status 0; a packed block
 * that fails to factor (impossible for a positive definite K in exact arithmetic)
 * gives NaN in that epoch's ep_resid, ep_chi2 and ep_logp only.  An epoch whose pixels
 * are not contiguous, an epoch index outside [0, n_epochs), n_epochs < 1 with an epoch
 * index and an open stream on the handle are refused (non-zero status,
 * psoap_last_error).
 * Workspace: the gradient's 16 Npad^2 bytes for one matrix (shared with it, freed by
 * psoap_chunk_grad_release), plus the packed blocks (8 sum side_e^2 bytes), one
 * 128 x 128 inverse per block row of every block and a few N-vectors, allocated by the
 * first call, kept with the handle and freed by psoap_chunk_loo_release or
 * psoap_chunk_destroy.  The handle's uploaded batches, their results and the
 * likelihood workspaces are left as they are. */
int psoap_chunk_loo(psoap_chunk *h, int c, const double *lwl, const double *gp, double mu_GP,
                    const int32_t *epoch, int n_epochs,
                    double *lnp, double *loo_logp,
                    double *pix_mean, double *pix_var, double *pix_logp,
                    double *ep_resid,
                    double *ep_chi2, double *ep_logp, int32_t *ep_npix);
int psoap_chunk_loo_release(psoap_chunk *h);

/* ---- likelihood with a per-epoch continuum polynomial integrated out ----------------
 * psoap_lnlike takes the continuum of every epoch as known: it subtracts the scalar
 * mu_GP.  Here every epoch e carries a Chebyshev polynomial of degree `order` with a
 * Gaussian prior, integrated out in closed form (Rasmussen & Williams 2.7).  With
 * r = fl - mu_GP and K as psoap_lnlike builds it:
 *   H[i][e (order+1) + k] = w[i] T_k(u_i) for the pixels i of epoch e, else 0, where u_i
 *       is x[i] mapped so that the smallest and the largest abscissa of the epoch go
 *       to -1 and +1 (numpy.polynomial.Chebyshev(domain=[a, b]); u = 0 for an epoch
 *       with one pixel or equal abscissae); q = n_epochs (order+1) columns;
 *   r = H beta + f + eps,  beta ~ N(0, Lambda),  Lambda = diag(prior_sd[k]^2), the same
 *       for every epoch;
 *   Ht = H Lambda^1/2,  W = U^-T Ht,  z = U^-T r  (K = U^T U),  M = I + W^T W,  bt = W^T z;
 *   lnp  = -1/2 (z^T z - bt^T M^-1 bt + log det K + log det M): the likelihood of r under
 *          K + H Lambda H^T, without N/2 log 2 pi as everywhere in this library;
 *   parts (B, 4)     z^T z, log det K, the gain bt^T M^-1 bt, log det M;
 *   beta (B, q)      E[beta] = Lambda^1/2 M^-1 bt;
 *   beta_cov (B, q, q)  Cov[beta] = Lambda^1/2 M^-1 Lambda^1/2, symmetric bit for bit;
 *   fl_cor (B, N)    fl - H E[beta].
 * weight == NULL is w = 1 (an additive offset); w = fl is the first-order form of a
 * multiplicative correction.  An epoch without pixels keeps its columns: mean 0,
 * covariance Lambda, nothing added to lnp.  parts, beta, beta_cov and fl_cor may be NULL;
 * the covariance and the solve for beta run only when asked for.
 * psoap_chunk_set_baseline checks and keeps the baseline (H does not depend on the
 * proposal: Ht is built once, by the next psoap_chunk_lnlike_marg, into a buffer of the
 * handle).  psoap_chunk_lnlike_marg walks B proposals (lwl (B, c, N), gp (B, 2c)) in
 * groups through the staged factorisation of [K | Ht] -- block row p updates and solves
 * only the appended tile columns that can be non-zero there -- forms M tile by tile in
 * the MFMA accumulators, factors it with the same staged kernels and finishes in one
 * workgroup per matrix (csrc/marg_kernels.hpp, csrc/marg_plan.hpp).  No atomics, every
 * sum in an order fixed by (N, c, epoch layout, order): the same arguments give the
 * same bits, whatever the batch around a matrix and whichever outputs are asked for.
 * Conventions: a negative hyper-parameter, a K that is not positive definite or an M
 * that fails to factor (impossible in exact arithmetic: its eigenvalues are >= 1) gives
 * lnp = -inf, NaN in every other output and status 0.  Refused (non-zero status,
 * psoap_last_error): order < 0 or > 15; (order+1) n_epochs > 1024; a prior_sd that is
 * not finite and positive; an epoch index outside [0, n_epochs); an epoch whose pixels
 * are not one contiguous run (the runs may come in any order); a non-finite abscissa
 * or weight; psoap_chunk_lnlike_marg before psoap_chunk_set_baseline, or after a
 * psoap_chunk_set_data that followed a baseline WITH weights (they described the old
 * data: set the baseline again); B < 1 or B > max_batch; an open stream on the handle.
 * Workspace: the gradient's buffer (shared with it as leave-one-out shares it, freed by
 * psoap_chunk_grad_release), 8 Npad (Npad + 128 Q) bytes per matrix of a group,
 * Q = ceil(q / 128); plus Ht (8 Npad 128 Q bytes), per matrix of a group M (16 (128 Q)^2
 * bytes; M^-1 and the covariance when asked for) and a few vectors, allocated by the
 * first call and freed by psoap_chunk_marg_release or psoap_chunk_destroy.  After a
 * release the baseline stays set: the next call builds Ht again.  The handle's
 * uploaded batches, their results and the likelihood workspaces are left as they are. */
int psoap_chunk_set_baseline(psoap_chunk *h, int order, const double *x, const int32_t *epoch, int n_epochs,
                             const double *weight, const double *prior_sd);
int psoap_chunk_lnlike_marg(psoap_chunk *h, int B, int c, const double *lwl, const double *gp, double mu_GP,
                            double *lnp, double *parts, double *beta, double *beta_cov, double *fl_cor);
int psoap_chunk_marg_release(psoap_chunk *h);

/* ---- gradient of the continuum-marginalised likelihood ----------------------------------
 * psoap_chunk_lnlike_marg_grad: the value psoap_chunk_lnlike_marg returns (lnp and parts
 * bit for bit) and its analytic gradient, with the outputs of psoap_chunk_lnlike_grad:
 *   grad_gp (B, 2c); grad_lwl (B, c, N), may be NULL; grad_mu (B), may be NULL; parts
 *   (B, 4), may be NULL.
 * H does not depend on the hyper-parameters, the rest-frame grids or mu_GP, so every
 * derivative is that of psoap_chunk_lnlike_grad with K^-1 -> (K + Ht Ht^T)^-1 =
 * Wi^T Wi - V V^T and alpha -> (K + Ht Ht^T)^-1 r: the staged factorisation runs on
 * [K | I | Ht], the Gram matrix is factored with Xt = Wh^T Wi appended so that
 * Vt = U_M^-T Xt falls out of it, and the fused contraction runs a second K loop of depth
 * 128 Q over Vt (csrc/marg_grad_kernels.hpp, csrc/marg_grad_plan.hpp).  The derivative
 * with respect to prior_sd is not provided.  No atomics, every sum in an order fixed by
 * (N, c, baseline layout): a proposal's bits do not depend on the batch around it nor on
 * which outputs are asked for; psoap_chunk_lnlike_grad keeps its bits.
 * psoap_chunk_lnprob_marg_grad: psoap_chunk_lnprob_grad with that gradient in the middle
 * (needs psoap_chunk_set_grid and psoap_chunk_set_dates); NOTE the order of its last two
 * arguments: grad_mu (B, may be NULL), then grad_vel (B, c, n_epochs; may be NULL).
 * Both take any B >= 1 (groups of at most 8 matrices and 1 GiB, as the gradient) and
 * need psoap_chunk_set_baseline: without one, or after a psoap_chunk_set_data that
 * followed a baseline with weights, they refuse with psoap_chunk_lnlike_marg's message.
 * A negative hyper-parameter, a K or an M that does not factor, or a faster-than-light
 * orbit gives lnp = -inf and NaN in every other output of that proposal, status 0.
 * Workspace: the gradient's buffer with 8 Npad (2 Npad + 128 Q) bytes per matrix of a
 * group (psoap_chunk_grad_release), and per matrix 8 * 128 Q (128 Q + Npad) bytes of
 * [M | Xt] beside the baseline's device side (psoap_chunk_marg_release). */
int psoap_chunk_lnlike_marg_grad(psoap_chunk *h, int B, int c, const double *lwl, const double *gp, double mu_GP,
                                 double *lnp, double *parts, double *grad_gp, double *grad_lwl, double *grad_mu);
int psoap_chunk_lnprob_marg_grad(psoap_chunk *h, int B, int model, const double *p_orb, const double *gp, double mu_GP,
                                 double *lnp, double *grad_orb, double *grad_gp, double *grad_mu, double *grad_vel);

/* ---- Fisher information and leave-one-out under the marginalised continuum ---------------
 * psoap_chunk_fisher_marg and psoap_chunk_loo_marg are psoap_chunk_fisher and
 * psoap_chunk_loo with Kt = K + Ht Ht^T (the baseline of psoap_chunk_set_baseline) in the
 * place of K: arguments, outputs, shapes and NULL rules are their plain twins'.
 *   fisher    F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t), both triangles, F == F^T bit for bit;
 *   fisher_mu 1^T Kt^-1 1 = |Wi 1|^2 - |Vt 1|^2;
 *   leave-one-out: A = Kt^-1 and alpha = Kt^-1 r in every formula of psoap_chunk_loo;
 *             lnp is the marginal likelihood, with the bits of psoap_chunk_lnlike_marg.
 * H does not depend on the hyper-parameters, the rest-frame grids or mu_GP, so a
 * tangent's covariance derivative K_t is the plain one.  The staged factorisation of
 * [K | I | Ht] and of [M | Xt] runs as psoap_chunk_lnlike_marg_grad runs it for one matrix
 * and leaves Wi = U^-T, Vt = U_M^-T Wh^T Wi and alpha_m; Kt^-1 = Wi^T Wi - Vt^T Vt is formed
 * tile by tile with a second K loop of depth 128 Q over Vt on the same accumulators, into
 * the Fisher workspace's K^-1 slot or, for the band tiles, into the packed epoch blocks
 * (csrc/marg_fisher_kernels.hpp); everything after that is the plain entry's launches.
 * About 3 N^2 128 Q flops beyond the plain entries, nothing more per tangent.  No atomics,
 * every sum in an order fixed by (N, c, baseline layout, T): the same arguments give the
 * same bits, a subsequence of the tangents gives the bits of the entries it shares, and
 * the plain entries keep their bits, also on a handle with a baseline.
 * The epoch index of psoap_chunk_loo_marg is that of its own outputs (contiguous runs in
 * any order, as for psoap_chunk_loo); it need not be the baseline's.
 * Conventions: a negative hyper-parameter, a K that is not positive definite or an M that
 * does not factor gives NaN in every output (lnp = -inf) and status 0.  Refused: what the
 * plain twins refuse (T < 1 or T > 32, a bad epoch layout, an open stream), and a handle
 * without a baseline or with a stale one, with psoap_chunk_lnlike_marg's messages.  The
 * derivative with respect to prior_sd is not provided.
 * Workspace: that of psoap_chunk_lnlike_marg_grad for one matrix (psoap_chunk_grad_release,
 * psoap_chunk_marg_release) plus the three Npad^2 matrices of psoap_chunk_fisher
 * (psoap_chunk_fisher_release) or the packed blocks of psoap_chunk_loo
 * (psoap_chunk_loo_release): the workspaces of the plain twins, shared with them. */
int psoap_chunk_fisher_marg(psoap_chunk *h, int c, const double *lwl, const double *gp,
                            int T, const double *tan_lwl, const double *tan_gp,
                            double *fisher, double *fisher_mu);
int psoap_chunk_loo_marg(psoap_chunk *h, int c, const double *lwl, const double *gp, double mu_GP,
                         const int32_t *epoch, int n_epochs,
                         double *lnp, double *loo_logp,
                         double *pix_mean, double *pix_var, double *pix_logp,
                         double *ep_resid,
                         double *ep_chi2, double *ep_logp, int32_t *ep_npix);

/* ---- Fisher information and leave-one-out under the time-variable kernel -----------------
 * psoap_chunk_fisher_tv and psoap_chunk_loo_tv are psoap_chunk_fisher and psoap_chunk_loo
 * with the time-variable kernel of psoap_chunk_lnlike_tv_grad over the handle's times
 * (psoap_chunk_set_times) in the place of K: tau (c) as there, the other arguments,
 * outputs, shapes and NULL rules are their plain twins'.
 * A tangent is t = (dx_t (c, N), da_tc, dl_tc, dtau_tc): tan_lwl (T, c, N; NULL: zeros),
 * tan_gp (T, 2c), tan_tau (T, c; NULL: zeros), 1 <= T <= 32.  With d = x_c[n] - x_c[m],
 * dt = t[n] - t[m] and e = exp(p_c d^2 + q_c dt^2), formed as psoap_chunk_lnlike_tv_grad
 * forms it (a = p * d * d, then a = a + q * dt * dt, without contraction, one exp),
 *   K_t[m,n] = sum_c e (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc
 *                       + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m]) + a_c^2 / tau_c^3 dt^2 dtau_tc)
 *   fisher    F_st = 1/2 tr(K^-1 K_s K^-1 K_t), both triangles, F == F^T bit for bit;
 *   fisher_mu 1^T K^-1 1 (may be NULL);
 *   leave-one-out: A = K^-1 and alpha = K^-1 r of that K in every formula of
 *             psoap_chunk_loo; lnp has the bits of psoap_chunk_lnlike_tv_grad.
 * The launches are the plain entries' with [K | I] factored under the time-variable fill;
 * the Fisher information takes the time-variable forms of its tangent fill, contraction and
 * finishing sums and a dot with time-scale terms (csrc/fisher_kernels.hpp), the
 * leave-one-out nothing: behind the factorisation
 * it reads K through W and alpha alone.  One multiply-add more per element in one fill and
 * one epilogue per tangent; the flops are psoap_chunk_fisher's, (1 + 4 T) N^3.  No
 * atomics, every sum in an order fixed by (N, c, T): the same arguments give the same
 * bits, a subsequence of the tangents gives the bits of the entries it shares.
 * Bit-identity at tau = inf: with every tau_c = +inf, F has the bits of psoap_chunk_fisher
 * in every entry -- whatever tan_tau holds: its coefficient a^2 / tau^3 dtau is 0, added
 * last -- and an entry whose tangent has nothing but dtau is exactly 0; fisher_mu and
 * every field of the leave-one-out have the bits of the plain entries.
 * Conventions: tau_c <= 0 or NaN, a negative hyper-parameter or a matrix that is not
 * positive definite gives NaN in every entry of fisher and in fisher_mu, and for the
 * leave-one-out lnp = -inf and NaN in every other floating output; status 0.  Refused
 * with a message: what the plain twins refuse, a call before psoap_chunk_set_times, on a
 * handle with an open stream, or on a handle with a baseline (the combination with the
 * marginalised continuum is not built).
 * Workspace: that of the plain twins, shared with them, plus 3 doubles for tau,
 * 2 T c doubles of time-scale tangents and contractions and one double more per tile
 * record; psoap_chunk_fisher_release, psoap_chunk_loo_release and
 * psoap_chunk_grad_release free all of it, the times stay with the handle. */
int psoap_chunk_fisher_tv(psoap_chunk *h, int c, const double *lwl, const double *gp,
                          const double *tau, int T, const double *tan_lwl,
                          const double *tan_gp, const double *tan_tau,
                          double *fisher, double *fisher_mu);
int psoap_chunk_loo_tv(psoap_chunk *h, int c, const double *lwl, const double *gp,
                       const double *tau, double mu_GP,
                       const int32_t *epoch, int n_epochs,
                       double *lnp, double *loo_logp,
                       double *pix_mean, double *pix_var, double *pix_logp,
                       double *ep_resid,
                       double *ep_chi2, double *ep_logp, int32_t *ep_npix);

/* ---- Fisher information and leave-one-out under the quasi-periodic kernel ------------------
 * psoap_chunk_fisher_qp and psoap_chunk_loo_qp are psoap_chunk_fisher_tv and
 * psoap_chunk_loo_tv with the quasi-periodic kernel of psoap_chunk_lnlike_qp_grad in the
 * place of K: gamma (c) and period (c) behind tau as there, the other arguments, outputs,
 * shapes and NULL rules are the time-variable twins'.
 * A tangent is t = (dx_t (c, N), da_tc, dl_tc, dtau_tc, dGamma_tc, dP_tc): tan_gamma and
 * tan_period (T, c; NULL: zeros) behind tan_tau.  With s, co = sincospi(dt / P_c) and
 * e = exp(p_c d^2 + q_c dt^2 - Gamma_c s^2), formed as psoap_chunk_lnlike_qp_grad forms it,
 *   K_t[m,n] = sum_c e (the time-variable terms - a_c^2 s^2 dGamma_tc
 *                       + a_c^2 Gamma_c pi / P_c^2 dt (2 s co) dP_tc)
 * and F_st, fisher_mu and the leave-one-out are the time-variable twins' formulas on that K.
 * New device code per tangent: k_qp_fisher_tangent_fill, k_qp_fisher_contract (the two K
 * loops of the time-variable contraction, the quasi-periodic epilogue), then
 * k_qp_grad_finish as it is and k_qp_fisher_dot; the leave-one-out has none.  No atomics,
 * every sum in an order fixed by (N, c, T): F == F^T bit for bit, a subsequence of the
 * tangents gives the bits of the entries it shares.
 * Bit-identity at Gamma = 0: with every Gamma_c = 0 and tan_gamma = 0, fisher and
 * fisher_mu have the bits of psoap_chunk_fisher_tv whatever period and tan_period hold, and
 * every field of the leave-one-out has the bits of psoap_chunk_loo_tv (lnp those of
 * psoap_chunk_lnlike_qp_grad).  A tangent with nothing but dP_c of a component with
 * Gamma_c = 0 has an exactly-zero row and column.
 * Conventions: those of the time-variable twins, and a Gamma_c < 0, NaN or inf or a
 * P_c <= 0, NaN or inf likewise.  Refused with a message: what the twins refuse.
 * Workspace: that of the twins, shared with them, plus 6 doubles for Gamma and P, 4 T c
 * doubles of tangents and contractions and two doubles more per component in a tile record;
 * the same releases free all of it. */
int psoap_chunk_fisher_qp(psoap_chunk *h, int c, const double *lwl, const double *gp,
                          const double *tau, const double *gamma, const double *period,
                          int T, const double *tan_lwl, const double *tan_gp,
                          const double *tan_tau, const double *tan_gamma,
                          const double *tan_period, double *fisher, double *fisher_mu);
int psoap_chunk_loo_qp(psoap_chunk *h, int c, const double *lwl, const double *gp,
                       const double *tau, const double *gamma, const double *period,
                       double mu_GP, const int32_t *epoch, int n_epochs,
                       double *lnp, double *loo_logp,
                       double *pix_mean, double *pix_var, double *pix_logp,
                       double *ep_resid,
                       double *ep_chi2, double *ep_logp, int32_t *ep_npix);

/* ---- the time-variable kernel under the marginalised continuum ------------------------------
 * Kt = K_tv + Ht Ht^T: K_tv the time-variable kernel of psoap_chunk_lnlike_tv_grad over the
 * handle's times (psoap_chunk_set_times), Ht from the handle's baseline
 * (psoap_chunk_set_baseline).  Three entries, each its marginal twin with tau:
 *   psoap_chunk_lnlike_marg_tv       psoap_chunk_lnlike_marg with tau (B, c): lnp, parts, beta,
 *                                    beta_cov, fl_cor with its shapes and NULL rules,
 *                                    B <= max_batch;
 *   psoap_chunk_lnlike_marg_tv_grad  psoap_chunk_lnlike_marg_grad with tau (B, c) and grad_tau
 *                                    (B, c), any B >= 1; lnp and parts have the bits of the
 *                                    value entry above; grad_gp == NULL asks for the value
 *                                    only, with the NULL rules of psoap_chunk_lnlike_tv_grad
 *                                    (grad_tau, grad_lwl and grad_mu NULL too; with grad_gp,
 *                                    grad_tau is required), and the same bits;
 *   psoap_chunk_fisher_marg_tv       psoap_chunk_fisher_tv under Kt: tau (c), tangents
 *                                    (tan_lwl, tan_gp, tan_tau), 1 <= T <= 32.
 * H does not depend on tau, so every derivative is the time-variable one with
 * K^-1 -> Kt^-1 = Wi^T Wi - Vt^T Vt and alpha -> alpha_m = Kt^-1 r; in particular, with
 * Q_m = alpha_m alpha_m^T - Kt^-1,
 *   d lnp / d tau_c = 1/2 a_c^2 / tau_c^3 sum_ij Q_m,ij e_cij dt_ij^2.
 * The launches are the marginal entries' with K filled by the time-variable fill; the
 * gradient's contraction is k_marg_tv_grad_contract (csrc/marg_grad_kernels.hpp: the two K
 * loops of the marginal contraction, the epilogue of the time-variable one) and its
 * finishing sums the time-variable ones; the Fisher information forms Kt^-1 as
 * psoap_chunk_fisher_marg does and then runs the tangent fill, product, contraction,
 * finishing sums and dot of psoap_chunk_fisher_tv.  One multiply-add more per element in
 * the fill and the epilogues; the flops are the marginal entries'.  No atomics, every sum
 * in an order fixed by (N, c, baseline layout, T): a proposal's bits do not depend on the
 * batch around it, on the grouping or on which optional outputs are asked for; a
 * subsequence of the tangents gives the bits of the entries it shares.
 * Bit-identity at tau = inf: with every tau_c = +inf, lnp, parts, beta, beta_cov, fl_cor,
 * grad_gp, grad_lwl, grad_mu, every entry of fisher and fisher_mu have the bits of
 * psoap_chunk_lnlike_marg, psoap_chunk_lnlike_marg_grad and psoap_chunk_fisher_marg on the
 * same handle; grad_tau is exactly 0, and so is a Fisher entry whose tangent has nothing
 * but dtau.
 * Conventions: tau_c <= 0 or NaN, a negative hyper-parameter, or a K or an M that does not
 * factor gives lnp = -inf and NaN in every other output of that proposal (NaN in every
 * entry of fisher and in fisher_mu), status 0; the other proposals keep their bits.
 * Refused with a message, in this order: missing arrays; the NULL rules above; c outside
 * 1 .. 3; B < 1 (the value entry: B outside [1, max_batch]) or T outside 1 .. 32; a call
 * before psoap_chunk_set_times; an open stream; a handle without a baseline or with a
 * stale one (psoap_chunk_lnlike_marg's messages).  The plain, _tv and _marg entries keep
 * their bits, and the _tv entries and psoap_chunk_predict_tv go on refusing a handle with
 * a baseline: the combination is reached through these three entries only.  Not built
 * under it: leave-one-out, predict, draws and the mixture; the derivative with respect to
 * prior_sd is not provided.
 * Workspace: that of psoap_chunk_lnlike_marg / _marg_grad / _fisher_marg in the same groups
 * (at most 8 matrices and 1 GiB), plus 3 doubles per matrix of a group for tau and for
 * grad_tau, one double more per tile record and 2 T c doubles of time-scale tangents and
 * contractions; psoap_chunk_grad_release, psoap_chunk_marg_release and
 * psoap_chunk_fisher_release free all of it, the times and the baseline stay with the
 * handle. */
int psoap_chunk_lnlike_marg_tv(psoap_chunk *h, int B, int c, const double *lwl, const double *gp,
                               const double *tau, double mu_GP,
                               double *lnp, double *parts, double *beta, double *beta_cov, double *fl_cor);
int psoap_chunk_lnlike_marg_tv_grad(psoap_chunk *h, int B, int c, const double *lwl, const double *gp,
                                    const double *tau, double mu_GP,
                                    double *lnp, double *parts, double *grad_gp, double *grad_tau,
                                    double *grad_lwl, double *grad_mu);
int psoap_chunk_fisher_marg_tv(psoap_chunk *h, int c, const double *lwl, const double *gp,
                               const double *tau, int T, const double *tan_lwl,
                               const double *tan_gp, const double *tan_tau,
                               double *fisher, double *fisher_mu);

/* ---- lnprob(p) under the time-variable kernel ---------------------------------------------------
 * psoap_chunk_lnprob_grad and psoap_chunk_lnprob_marg_grad with tau (B, c) after gp and
 * grad_tau (B, c) after grad_gp: the same orbit front end (Kepler solve, Jacobian, Doppler shift
 * on the device), the gradient run of psoap_chunk_lnlike_tv_grad / _marg_tv_grad, the epoch fold
 * and the Jacobian contraction.  Needs psoap_chunk_set_grid, _set_dates and _set_times; the
 * _marg_ entry a baseline, which the plain entry refuses.  NULL rules as
 * psoap_chunk_lnlike_tv_grad: grad_gp == NULL asks for the value only (every other gradient
 * NULL too); grad_orb and grad_tau go with grad_gp; grad_vel and grad_mu are optional.
 * A faster-than-light orbit, a negative hyper-parameter, a tau that is no time scale or a
 * matrix that does not factor gives -inf and NaN gradients for that proposal.  With every
 * tau = +inf the outputs have the bits of the entries without tau and grad_tau is exactly 0. */
int psoap_chunk_lnprob_tv_grad(psoap_chunk *h, int B, int model, const double *p_orb, const double *gp,
                               const double *tau, double mu_GP, double *lnp, double *grad_orb,
                               double *grad_gp, double *grad_tau, double *grad_vel, double *grad_mu);
int psoap_chunk_lnprob_marg_tv_grad(psoap_chunk *h, int B, int model, const double *p_orb, const double *gp,
                                    const double *tau, double mu_GP, double *lnp, double *grad_orb,
                                    double *grad_gp, double *grad_tau, double *grad_mu, double *grad_vel);

/* ---- component spectra under the marginalised continuum ------------------------------------------
 * psoap_chunk_predict_marg and psoap_chunk_predict_marg_var are psoap_chunk_predict and psoap_chunk_predict_var with
 * Kt = K + Ht Ht^T (the baseline of psoap_chunk_set_baseline) in the place of the data covariance K: arguments, output
 * shapes and the NULL rule of Sigma_out are their plain twins'.  The continuum itself is not predicted (beta and fl_cor of
 * psoap_chunk_lnlike_marg give it); it enters through the data covariance only, so the component spectra carry its
 * uncertainty instead of a continuum frozen at its posterior mean.  With r = fl - offset, Cx (R x N), A and m0 exactly as
 * the plain mode builds them (psoap_predict above):
 *   mu = m0 + Cx Kt^-1 r,   Sigma = A - Cx Kt^-1 Cx^T;
 *   Wc = U^-T Cx^T, Wh = U^-T Ht, z = U^-T r  (K = U^T U);  M = I + Wh^T Wh = U_M^T U_M,  G = Wh^T Wc (S x R, S = 128 Q),
 *   bt = Wh^T z,  Y = U_M^-T G,  y = U_M^-T bt;
 *   mu = m0 + Wc^T z - Y^T y,   Sigma = A - Wc^T Wc + Y^T Y,   var = prior - colnorm^2(Wc) + colnorm^2(Y):
 * the plain Sigma plus a positive semi-definite term of rank <= q.  The staged factorisation runs on [K | Cx^T | Ht]
 * (ld = Npad + Rpad + 128 Q; block row p updates and solves K's own columns, all of Cx^T and the slots of Ht that can be
 * non-zero there), one launch forms [M | G] tile by tile in the MFMA accumulators, the same staged kernels factor it
 * with bt as right-hand side, which leaves Y and y, and one workgroup per upper tile of Sigma runs two K loops (depth
 * Npad over Wc, depth S over Y) on one accumulator set and mirrors the tile (csrc/marg_predict_kernels.hpp,
 * csrc/marg_predict_plan.hpp).  No explicit inverse.  No atomics, every sum in an order fixed by (N, c, M, mode,
 * baseline layout): the same arguments give the same bits, mu has the same bits whether Sigma, the variances or neither
 * is asked for, Sigma == Sigma^T bit for bit, and psoap_chunk_predict keeps its bits on a handle with a baseline.
 * Modes: 0 with c = 2 or 3, 1 with c = 2, 2 with c = 1.  Mode 1 with c = 3 (the transposed mean of predict_f_g_h_sum,
 * covariance.py:294) is refused, as are an open stream and a handle without a baseline or with a stale one -- the
 * baseline's with psoap_chunk_lnlike_marg's messages.
 * status_out: 0 ok; 1 K is not positive definite or M does not factor -- every output is then NaN and the call itself returns 0.
 * Workspace: 8 Npad (Npad + Rpad + 128 Q) bytes of [K | Cx^T | Ht] and, with Sigma, 8 Rpad^2 in the handle's predict
 * workspace (grown, shared with psoap_chunk_predict; psoap_chunk_predict_release); 8 * 128 Q (128 Q + Rpad) bytes of
 * [M | G] and a few vectors beside the baseline's device side (psoap_chunk_marg_release).  Rpad = R rounded up to 128.
 * psoap_chunk_predict_timings reports the call: factor_ms = fill, both staged factorisations and the Gram launch,
 * sigma_ms = mean + prior fill + Sigma (or the variances); flops = the plain F_pred + N S (S + R) + S^3 / 3 + S^2 R
 * + S R^2 on padded sizes (S R^2, like N R^2, only when Sigma is formed; 2 S R for the variances). */
int psoap_chunk_predict_marg(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                             const double *lwl_pred, const double *mu_c, const double *gp,
                             double *mu_out, double *Sigma_out /* may be NULL */, int *status_out);
int psoap_chunk_predict_marg_var(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                                 const double *lwl_pred, const double *mu_c, const double *gp,
                                 double *mu_out, double *var_out, int *status_out);

/* ---- component spectra under the time-variable kernel: the spectrum at a date ----------------------
 * psoap_chunk_predict_tv and psoap_chunk_predict_tv_var are psoap_chunk_predict and psoap_chunk_predict_var under the
 * kernel of psoap_chunk_lnlike_tv_grad, K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2) + sigma_i^2 delta_ij with
 * q_c = -1/2 / tau_c^2 over the times of psoap_chunk_set_times.  A prediction point is a pair: ln-wavelength
 * lwl_pred[k][m] and date t_pred[m] -- t_pred (M) is shared by the components, in days, with the constant removed that
 * was removed from the handle's times.  With tau (c):
 *   cross-covariance of component k with pixel i:  a_k^2 exp(p_k (lwl_pred[k][m] - lwl[k][i])^2 + q_k (t_pred[m] - t[i])^2)
 *   prior covariance of points m and n:            a_k^2 exp(p_k d^2 + q_k (t_pred[n] - t_pred[m])^2)
 * (the diagonal: a_k^2, with the nugget where the static mode has one); modes, offsets, m0, the block layout and the
 * NULL rule of Sigma_out are psoap_predict's.  Several dates in one call are several runs of t_pred (with lwl_pred
 * repeated): Sigma then holds the covariance between the dates as well.
 * Mode 0 with c = 2 or 3, mode 1 with c = 2, mode 2 with c = 1; refused with a message: mode 1 with c = 3, a call before
 * psoap_chunk_set_times, an open stream, a handle with a baseline (that combination is not built), a tau_c that is <= 0 or
 * NaN (+inf is valid: that component is static) and a t_pred that is not finite.
 * status_out: 0 ok; 1 K is not positive definite -- every output is then NaN and the call itself returns 0.
 * The factorisation is always the staged sweep (the persistent launch evaluates the static covariance): with every
 * tau_c = +inf the outputs have the bits of psoap_chunk_predict / _var on that route (PSOAP_SHARE_POLICY=staged).  A
 * component with finite tau_c whose every q_c (t_pred[m] - t[i])^2 is <= -746 gets its prior back exactly: m0, its block
 * of A, variances a_c^2.  No atomics: every sum runs in an order fixed by (N, c, M, mode).
 * With Sigma_out the handle keeps mean and Sigma for psoap_chunk_predict_draw, as after psoap_chunk_predict.
 * Workspace: the handle's predict workspace (psoap_chunk_predict_release); psoap_chunk_predict_timings and, with
 * profiling on, psoap_chunk_get_timings report the call (flops: those of the plain call). */
int psoap_chunk_predict_tv(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                           const double *lwl_pred, const double *t_pred, const double *mu_c,
                           const double *gp, const double *tau,
                           double *mu_out, double *Sigma_out /* may be NULL */, int *status_out);
int psoap_chunk_predict_tv_var(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                               const double *lwl_pred, const double *t_pred, const double *mu_c,
                               const double *gp, const double *tau,
                               double *mu_out, double *var_out, int *status_out);

/* Split-phase form of psoap_lnlike_batch: upload (H2D, async, on a copy stream of
 * its own), eval (kernels only, async), fetch (sync + D2H of B doubles).
 * A handle holds TWO proposal batches: an upload always goes to the one that is
 * not being evaluated, and eval consumes the most recent upload (or re-evaluates
 * the current batch when nothing new was uploaded).  So
 *     upload(0); loop { eval(); upload(k+1); fetch() -> results of k }
 * moves the proposals of step k+1 over PCIe while step k is being factored
 * (bench.py's timed step: one upload, one eval, one fetch), and the plain
 * upload / eval / fetch sequence keeps working unchanged. */
int psoap_batch_upload(psoap_chunk *h, int B, int c, const double *lwl,
                       const double *gp, double mu_GP);
/* Same, but the Doppler shift runs on the device: vel (B, c, n_epochs) km/s,
 * lwl_c = lwl - vel[c, epoch]/c_kms (psoap/data.py:37,61).  Needs set_grid. */
int psoap_batch_upload_velocities(psoap_chunk *h, int B, int c, const double *vel,
                                  const double *gp, double mu_GP);
/* Orbit proposals: the batched Kepler solve, the Doppler shift and the
 * |v| >= c_kms -> -inf rule of Worker.lnprob (psoap/sample_parallel.py:183-193) run on the device.
 * model: 0 SB1, 1 SB2, 2 ST1, 3 ST2, 4 ST3; p_orb (B, n_orb) in the order of utils.registered_params
 * up to and including gamma (psoap/utils.py:4-14): n_orb = 6, 7, 11, 12, 13.  Needs set_grid + set_dates. */
int psoap_chunk_set_dates(psoap_chunk *h, const double *dates, int n_epochs);
int psoap_batch_upload_orbits(psoap_chunk *h, int B, int model, const double *p_orb, const double *gp,
                              double mu_GP);
/* orbit.models[model](*p_orb, dates).get_velocities() for B parameter vectors at once
 * (psoap/orbit.py:95-115,148-170,301-320,394-417,463-487): vel_out (B, c, n_dates) km/s. */
int psoap_orbit_velocities(int device, int model, int B, const double *p_orb, int n_dates, const double *dates,
                           double *vel_out);
/* Time scales for the PENDING upload (whichever of the three uploads made it): tau (B, c) in days, the
 * tau_c of psoap_chunk_lnlike_tv_grad, over the times of psoap_chunk_set_times.  B and c must be the
 * upload's.  The copy is queued on the upload's stream behind it (no host round trip: the upload stays
 * asynchronous); the next upload to that slot clears the time scales.  psoap_batch_eval on a slot that
 * carries them always takes the staged path, whatever psoap_chunk_set_mode says -- the persistent kernel
 * has no temporal factor -- with the time-variable fill; it is not counted as a staged_policy event.
 * tau_c <= 0 or NaN gives -inf for that proposal alone, flagged on the device with the fill (the others
 * keep their bits); tau_c = +inf is the static model, and with every tau = +inf the results have the bits
 * of the same upload evaluated without this call under psoap_chunk_set_mode(h, 0).  A proposal's bits
 * depend neither on B nor on its position in the batch nor on the number of stream groups.
 * Refused: no pending upload, another B or c, no times, an open stream, a handle with a baseline (the
 * value under a baseline goes through psoap_chunk_lnlike_marg_tv).  psoap_group_eval and
 * psoap_stream_open refuse a handle while the slot its next evaluation would read -- the pending one
 * if there is one, else the active one -- carries time scales. */
int psoap_batch_set_tau(psoap_chunk *h, int B, int c, const double *tau);
int psoap_batch_eval(psoap_chunk *h);
int psoap_batch_fetch(psoap_chunk *h, double *out);
int psoap_chunk_sync(psoap_chunk *h);

/* ---- kernel-matrix fills --------------------------------------------------------
 * fill_V11_f / fill_V11_f_g / fill_V11_f_g_h (psoap/matrix_functions.pyx:19-59,
 * 99-146,149-201): full symmetric (N,N) matrix written IN PLACE into the
 * caller's host array; sigma == NULL -> no noise term (the pyx contract);
 * sigma != NULL fuses V11[diag] += sigma**2 (covariance.py:322). */
int psoap_fill_sym(int device, int c, int N, const double *lwl, const double *gp,
                   const double *sigma, double *out);
/* psoap_fill_sym under the time-variable kernel (psoap_chunk_lnlike_tv_grad above):
 * t (N) the pixels' times, tau (c) the time scales,
 *   out[i,j] = sum_c amp_c^2 exp(p_c (lwl_c[j]-lwl_c[i])^2 + q_c (t[j]-t[i])^2),
 * the argument formed as p * d * d, then + q * dt * dt, without contraction; diagonal,
 * sigma and everything else as psoap_fill_sym.  With every tau_c = +inf the matrix is
 * bit-identical to psoap_fill_sym's.  Stand-alone (no handle): it exists so that the
 * matrix of the time-variable likelihood can be checked element by element. */
int psoap_fill_sym_tv(int device, int c, int N, const double *lwl, const double *t,
                      const double *gp, const double *tau, const double *sigma,
                      double *out);
/* psoap_fill_sym under the quasi-periodic kernel (psoap_chunk_lnlike_qp_grad above):
 * gamma, period (c) beside tau,
 *   out[i,j] = sum_c amp_c^2 exp(p_c d^2 + q_c dt^2 - gamma_c sin^2(pi dt / period_c)),
 * the argument formed as that entry describes; everything else as psoap_fill_sym_tv.
 * With every gamma_c = 0 the matrix is bit-identical to psoap_fill_sym_tv's. */
int psoap_fill_sym_qp(int device, int c, int N, const double *lwl, const double *t,
                      const double *gp, const double *tau, const double *gamma,
                      const double *period, const double *sigma, double *out);
/* fill_V12_f(psoap/matrix_functions.pyx:61-96): out (M,N),
 * out[i,j] = amp^2 exp(p (lwl_col[j]-lwl_row[i])^2), M = len(lwl_row). */
int psoap_fill_cross(int device, int M, int N, const double *lwl_row,
                     const double *lwl_col, double amp, double l, double *out);

/* ---- predict --------------------------------------------------------------------
 * mode 0: joint conditional of the c components -- predict_f_g
 *         (covariance.py:81-148), predict_f_g_h (:190-251):
 *         mu (c*M), Sigma (c*M, c*M); mean offset fl - 1.0 (:140,:248).
 * mode 1: conditional of the sum -- predict_f_g_sum (:151-187; 1e-8 nugget,
 *         offset fl - 1.0), predict_f_g_h_sum (:253-297; offset fl - mu_c[0],
 *         M == N): mu (M), Sigma (M, M).  mu_c[0] is mu_fg / mu_fgh.
 * mode 2: single component predict_f (:25-54) with the evidently intended
 *         N = len(lwl_predict) (the reference raises NameError at :38):
 *         offset fl - mu_c[0].
 * lwl (c,N), lwl_pred (c,M); Sigma_out may be NULL (get_Sigma=False, :145-148).
 * status_out: 0 ok, 1 data covariance not positive definite (the reference
 * raises LinAlgError there; outputs are then NaN). */
int psoap_predict(int device, int mode, int c, int N, int M, const double *lwl,
                  const double *fl, const double *sigma, const double *lwl_pred,
                  const double *mu_c, const double *gp, double *mu_out,
                  double *Sigma_out, int *status_out);
/* The same on a chunk handle (fl, sigma and N are the handle's): every device
 * buffer lives in a grow-only workspace owned by the handle, so the retrieve loop
 * (scripts/psoap_retrieve_ST3.py:148, one predict per chunk) allocates once.
 * psoap_chunk_predict_release frees that workspace early (destroy frees it too). */
int psoap_chunk_predict(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                        const double *lwl_pred, const double *mu_c, const double *gp,
                        double *mu_out, double *Sigma_out, int *status_out);
/* Mean and diag(Sigma) only (R doubles instead of R^2, no N R^2 product, no 75 MB download):
 * what the retrieve scripts use of Sigma -- sigma_f = sqrt(diag(Sigma))[0:M]
 * (scripts/psoap_retrieve_ST3.py:111-119, psoap_retrieve_SB2.py:107-113). */
int psoap_chunk_predict_var(psoap_chunk *h, int mode, int c, int M, const double *lwl,
                            const double *lwl_pred, const double *mu_c, const double *gp,
                            double *mu_out, double *var_out, int *status_out);
int psoap_chunk_predict_release(psoap_chunk *h);
/* Posterior draws of the component spectra (csrc/draw_kernels.hpp, draw_plan.hpp, draw_rng.hpp): what the reference's
 * scripts/psoap_retrieve_SB2_draw.py, psoap_retrieve_ST3_draw.py and psoap_predict_SB2.py / _ST3.py --draws make with
 * np.random.multivariate_normal(mu, Sigma, size=n_draws), from the mean and Sigma the handle's predict workspace holds:
 *     X[d, :] = mu + U^T z_d,   U^T U = Sigma + nugget I (U upper),   z_d ~ N(0, I_R),   d = 0 .. D-1
 * with R the prediction rows of the handle's last successful psoap_chunk_predict or psoap_chunk_predict_marg call that
 * formed Sigma (Sigma_out != NULL, status 0; any mode).  The draws are from N(mu, Sigma + nugget I), NOT N(mu, Sigma):
 * nugget is an absolute variance (flux^2, >= 0) and is needed -- Sigma = A - W^T W on a prediction grid finer than the
 * kernel's length scale is numerically rank deficient with small negative eigenvalues from rounding, which NumPy's SVD
 * route hides and a Cholesky factorisation does not (the reference itself adds 1e-8 in predict_f_g_sum,
 * covariance.py:165; the Python layers default to that).  Sigma and mu are only read: further calls with another seed,
 * D or nugget need no new predict.
 * z == NULL: the normals come from seed -- Philox4x32-10 with key (seed low word, seed high word) and counter
 * (i >> 1, d, 0, 0) for element i of draw d, two 53-bit uniforms per block, Box-Muller (even element the cosine, odd the
 * sine): element i of draw d depends on (seed, d, i) alone, not on D, the padding, the grid or the device.
 * z != NULL: z (D, R) is used and seed ignored.  out (D, R).
 * status_out: 0 ok, 1 Sigma + nugget I does not factor (out is NaN, the call returns 0).
 * Returns 2 (psoap_last_error): no such predict call since the handle's creation, psoap_chunk_predict_release,
 * psoap_chunk_set_data or psoap_chunk_set_baseline (the variance-only calls, Sigma_out == NULL and a predict call with
 * status 1 clear the record too); D < 1 or D > 1048576; nugget < 0 or not finite; an open stream.
 * Work: the copy, the staged factorisation of the copy (Rpad^3 / 3), the normals, and one fp64 MFMA launch for the
 * triangular product, tile (td, tj) running block rows 0 .. tj of U with the diagonal tile masked to its upper half
 * (D R^2 flops).  No atomics, every sum in an order fixed by (R, D).  Memory: 8 Rpad (Rpad + Dpad) + 8 Dpad Rpad bytes
 * beside the predict workspace, grown as needed and freed by psoap_chunk_predict_release.  Launches are booked under
 * PSOAP_K_FILL (copy), PANEL_UPDATE / POTRF / TRSM (factorisation), MISC (normals), GRAD (product). */
int psoap_chunk_predict_draw(psoap_chunk *h, int D, unsigned long long seed, const double *z,
                             double nugget, double *out, int *status_out);
/* the generator alone: out[d * n + i] for d < D, i < n -- what the call above uses as z for the same seed */
int psoap_draw_normals(int device, unsigned long long seed, int D, int n, double *out);
/* host twin of the generator's integer core (pure host): the Philox4x32-10 block of key seed, counter (c0, c1, 0, 0) */
int psoap_draw_philox(unsigned long long seed, unsigned int c0, unsigned int c1, unsigned int out[4]);
/* Component spectra marginalised over the chain: mixture moments on the device (csrc/mix_kernels.hpp, mix_plan.hpp).
 * Over samples s = 1 .. S of the orbit and the hyper-parameters with weights w_s, W = sum_s w_s, and the conditional
 * (mu_s, Sigma_s) of each sample as psoap_chunk_predict (marg = 0) or psoap_chunk_predict_marg (marg = 1) computes it:
 *     mu_mix    = sum_s w_s mu_s / W
 *     Sigma_mix = sum_s w_s Sigma_s / W  +  sum_s w_s (mu_s - mu_mix)(mu_s - mu_mix)^T / W      (within + between)
 * Every sample is folded on the device; one mu and one Sigma travel to the host at the end.
 * psoap_chunk_mix_begin fixes what the samples share -- marg, mode, c, M and lwl_pred (c, M) as the twins take them (marg = 1
 * needs a current baseline), the prior means mu_c (c values in mode 0, else one), S_max (1 .. 4096) and whether full Sigma
 * (want_sigma = 1) or the variances only (0) are accumulated -- and zeroes the accumulators.  Memory, beside the predict
 * workspace and untouched by psoap_chunk_predict_release: 2 x 8 Rpad^2 (Sbar, Sigma_mix; 8 Rpad in the variance-only mode)
 * + 2 x 8 Spad Rpad (the stacked means and their centred copy), Rpad = R rounded up to 128, Spad = S_max rounded up to 16.
 * psoap_chunk_mix_add runs exactly the predict call of the twins (their _var forms with want_sigma = 0) for (lwl (c, N),
 * gp (2c)) with the outputs staying on the device -- no Sigma download -- and folds the result with `weight` (finite, > 0):
 * Sbar += weight Sigma_s without FMA contraction (weight 1 adds exactly), mu_s into row s of the stacked means.  With
 * want_sigma = 1 the handle's draw record is left as by a predict call with Sigma_out: psoap_chunk_predict_draw then draws
 * from that sample's posterior.  status_out: 0 folded; 1 not positive definite -- the sample is NOT folded, the accumulators
 * are untouched, the call returns 0.
 * psoap_chunk_mix_finish only reads the accumulators: it may be called repeatedly and between adds.  mu_out (R), Sigma_out
 * (R, R; symmetric bit for bit; must be NULL in the variance-only mode, may be NULL otherwise), var_within_out and
 * var_between_out (R): diag of the two terms, diag(Sigma_mix) = var_within + var_between.  n_folded_out, W_out: optional.
 * W and the weighted means are summed in ascending order of the adds, one lane per column; the between term is one fp64
 * MFMA launch over all upper tiles (K loop over the samples in that order); no atomics: the result is fixed by
 * (R, the samples, the order of the adds).
 * Each returns 2 (psoap_last_error): an open stream; weight not finite or <= 0; more than S_max folded samples; S_max < 1 or
 * > 4096; add or finish without begin, or after psoap_chunk_set_data, psoap_chunk_set_baseline or psoap_chunk_mix_release
 * ended the mixture; finish with nothing folded; Sigma_out in the variance-only mode.
 * Launches are booked under PSOAP_K_FILL (fold), GRAD (the rank-S product), MISC (the rest). */
int psoap_chunk_mix_begin(psoap_chunk *h, int marg, int mode, int c, int M, const double *lwl_pred,
                          const double *mu_c, int S_max, int want_sigma);
int psoap_chunk_mix_add(psoap_chunk *h, const double *lwl, const double *gp, double weight, int *status_out);
int psoap_chunk_mix_finish(psoap_chunk *h, double *mu_out, double *Sigma_out, double *var_within_out,
                           double *var_between_out, int *n_folded_out, double *W_out);
int psoap_chunk_mix_release(psoap_chunk *h);
/* host twin of the mixture's plan (pure host): Rpad, Spad, the upper tiles of the rank-S product in launch order
 * (tiles_out: min(max_tiles, n_tiles) pairs (ti, tj)) and the bytes of all its device buffers; any output may be NULL.
 * Returns 2: R < 1 or > 32768, S_max < 1 or > 4096, want_sigma not 0 or 1. */
int psoap_mix_plan(int R, int S_max, int want_sigma, int *Rpad, int *Spad, int *n_tiles, int *tiles_out,
                   int max_tiles, long long *bytes);
/* Timings of the handle's last predict call, in ms: device_ms = first upload ->
 * mu and Sigma complete on the device (HIP events), factor_ms = the persistent
 * launch over [B | Cx^T], sigma_ms = mean + prior fill + Sigma = A - W^T W,
 * download_ms = what the Sigma download adds to the call beyond the device work (it
 * travels in groups of tile rows while later groups are computed), total_ms = the whole call
 * (host clock); flops = N^3/3 + N^2 R + N R^2 + 2 N R (SURVEY.md 8(d) F_pred,
 * padded sizes, R = prediction columns). */
typedef struct {
    double device_ms, factor_ms, sigma_ms, download_ms, total_ms, flops;
} psoap_predict_timings;
int psoap_chunk_predict_timings(psoap_chunk *h, psoap_predict_timings *t);
/* A reusable predict workspace that is not tied to a chunk: fl and sigma travel with
 * every call (2 N doubles), all N^2-sized buffers are kept and only grow.  One
 * predictor serves the whole retrieve loop (chunk after chunk); psoap_predict is
 * this with a workspace created and destroyed inside the call. */
typedef struct psoap_predictor psoap_predictor;
int psoap_predictor_create(psoap_predictor **out, int device);
int psoap_predictor_run(psoap_predictor *p, int mode, int c, int N, int M,
                        const double *lwl, const double *fl, const double *sigma,
                        const double *lwl_pred, const double *mu_c, const double *gp,
                        double *mu_out, double *Sigma_out, int *status_out);
int psoap_predictor_run_var(psoap_predictor *p, int mode, int c, int N, int M,
                            const double *lwl, const double *fl, const double *sigma,
                            const double *lwl_pred, const double *mu_c, const double *gp,
                            double *mu_out, double *var_out, int *status_out);
int psoap_predictor_timings(psoap_predictor *p, psoap_predict_timings *t);
int psoap_predictor_destroy(psoap_predictor *p);

/* ---- calibration ---------------------------------------------
 * Chebyshev re-normalisation of one epoch's flux against reference epochs:
 *   fl' = mu + C B^-1 (fl_fixed - mu),  C' = A - C B^-1 C^T,  D = fl_cal * T_k(lwl_cal),
 *   X = (D^T C'^-1 D)^-1 D^T C'^-1 fl',  fl_cor = D X.
 * psoap_calibrate_explicit replaces optimize_calibration (covariance.py:560-624):
 *   caller-filled A (M,M) with sigma_cal^2 on the diagonal, B (N,N) with
 *   sigma_fixed^2, C (M,N); row-major host arrays.
 * psoap_calibrate evaluates the three matrices on the device from c-component
 *   rest-frame grids: optimize_calibration_static (covariance.py:628-707, c = 1,
 *   lwls_cal == lwl_cal) and the per-epoch body of
 *   scripts/psoap_process_calibration_ST3.py:147-183 (c = 3).  lwls_cal (c,M),
 *   lwls_fixed (c,N), gp (2c); lwl_cal (M) is the Chebyshev abscissa, mapped from
 *   [lwl0, lwl1] onto [-1, 1] as numpy's Chebyshev(domain=...) does.
 * Outputs: fl_cor (M), X (order+1).  order <= 15.
 * status_out: 0 ok; 1 B, 2 C', 3 the normal equations not positive definite (the
 * reference raises LinAlgError there; outputs are then unspecified). */
int psoap_calibrate(int device, int c, int M, int N, int order, double lwl0,
                    double lwl1, const double *lwl_cal, const double *lwls_cal,
                    const double *fl_cal, const double *sigma_cal,
                    const double *lwls_fixed, const double *fl_fixed,
                    const double *sigma_fixed, const double *gp, double mu_GP,
                    double *fl_cor, double *X, int *status_out);
int psoap_calibrate_explicit(int device, int M, int N, int order, double lwl0,
                             double lwl1, const double *lwl_cal,
                             const double *fl_cal, const double *fl_fixed,
                             const double *A, const double *B, const double *C,
                             double mu_GP, double *fl_cor, double *X,
                             int *status_out);

/* ---- several chunks, one launch ---------------------------------------------------
 * A group evaluates the uploaded batches of several chunk handles (one device, one
 * component count, sizes may differ) in ONE launch of the persistent kernel over the
 * heterogeneous batch, so that the matrices of all chunks hide each other's dependency
 * chains.  The reference evaluates its chunks in separate worker processes
 * (sample_parallel.py:258-278, :378-387); this is the one-GPU form of that fan-out.
 * Usage: psoap_batch_upload* on every member, psoap_group_eval, psoap_batch_fetch on
 * every member (each handle's stream waits for the group launch). */
typedef struct psoap_group psoap_group;
int psoap_group_create(psoap_group **out, psoap_chunk *const *handles, int n);
int psoap_group_eval(psoap_group *g);
int psoap_group_destroy(psoap_group *g);
/* How often the group rebuilt its task list (batch sizes changed) and refreshed its matrix
 * records (a member moved to its other proposal slot: device-to-device, no host sync). */
int psoap_group_stats(psoap_group *g, long long *plan_builds, long long *record_refreshes);

/* ---- measurement ----------------------------------------------------------------
 * With profiling on, every kernel launch of psoap_batch_eval is bracketed by
 * hipEvents on its own stream (single stream group, so launches serialise);
 * get_timings returns per-kernel-class totals of the LAST eval. */
enum {
    PSOAP_K_FILL = 0,
    PSOAP_K_PANEL_UPDATE = 1, /* MFMA f64 left-looking panel update (dominant) */
    PSOAP_K_POTRF = 2,
    PSOAP_K_TRSM = 3,
    PSOAP_K_MISC = 4,
    PSOAP_K_DAG = 5,          /* the persistent dependency-graph kernel (whole factorisation) */
    PSOAP_K_GRAD = 6,         /* the fused contraction of psoap_chunk_lnlike_grad */
    PSOAP_K_CLASSES = 7
};
typedef struct {
    double ms[PSOAP_K_CLASSES];      /* summed device time per class */
    int64_t launches[PSOAP_K_CLASSES];
    double flops[PSOAP_K_CLASSES];   /* executed flops per class (MFMA classes) */
    double bytes[PSOAP_K_CLASSES];   /* algorithmic HBM bytes per class (fill) */
    double total_ms;                 /* first launch -> last launch, event time */
} psoap_timings;
int psoap_chunk_set_profiling(psoap_chunk *h, int enabled);
int psoap_chunk_get_timings(psoap_chunk *h, psoap_timings *t);
/* Number of concurrent stream groups a batch is split into (staged mode; default 2). */
int psoap_chunk_set_stream_groups(psoap_chunk *h, int groups);
/* Execution mode of psoap_batch_eval: 1 (default) = one persistent dependency-graph kernel
 * for the whole batched factorisation; 0 = staged, three kernels per 128-row panel.
 * Inside mode 1 the tile updates are cut by one of two schemes chosen from the batch size (latency
 * for small batches, throughput for large ones); the environment variable
 * PSOAP_DAG_SCHEME=0|1, read when a task list is built, pins one for experiments. */
int psoap_chunk_set_mode(psoap_chunk *h, int mode);

/* Debug aid for the persistent kernel: the first call allocates a per-task timestamp log, later
 * calls copy it out (4 x 100 MHz stamps per task, indexed by ticket). */
int psoap_chunk_dag_tasklog(psoap_chunk *h, unsigned long long *out, long long max_tasks);
/* ---- Streamed evaluation (round 4): consecutive ensemble steps through ONE resident launch ----------------
 * Replaces: the back-to-back iterations of the sampler's loop, /root/reference/psoap/sample_parallel.py:434-438 (every
 * iteration calls lnprob -> Worker.lnprob -> covariance.lnlike[...] at :193, and the master gathers at :378-387).
 * A plain psoap_batch_eval is one launch of the persistent kernel per step, which ramps up and drains every time;
 * a stream keeps the launch resident and lets the MATRICES come and go: `lanes` matrix workspaces of the handle
 * (lanes <= max_batch, <= 64) each run the same single-matrix task list, a dispatcher workgroup inside the launch pulls
 * submitted proposals from pinned host memory and opens lanes, and the workgroup that finishes a matrix writes its
 * lnprob straight into pinned host memory.  A proposal's result does not depend on what else is in flight: it is
 * bit-identical for every batch size, submission order and number of GPUs.
 * Typical use -- two half-ensembles in flight (neither half's proposals depend on the other's accept / reject):
 *     open; tA = submit(A0); tB = submit(B0); loop { fetch(tA); tA = submit(A_next); fetch(tB); tB = submit(B_next); }
 * While a stream is open the handle's batch entry points (psoap_batch_*, psoap_lnlike*) are refused -- the matrix
 * workspaces belong to the resident launch -- and other launches on the device wait until it leaves (it does so by
 * itself once nothing has been in flight for PSOAP_STREAM_IDLE_MS, default 20 ms, and comes back on the next submit). */
/* c: number of components of every submission; scheme: -1 automatic (by lanes and N, as for a batch of `lanes` matrices),
 * 0 throughput, 1 latency, 2 following (refused in late round 5 for a rare wrong value; round 6 removed its cause --
 * LABNOTES 14 -- and all three run here). */
int psoap_stream_open(psoap_chunk *h, int c, int lanes, int scheme);
/* n proposals -- lwl (n, c, N), gp (n, 2c) as psoap_batch_upload -- into n free lanes; tickets[n] identify them.
 * Fails when fewer than n lanes are free. */
int psoap_stream_submit(psoap_chunk *h, int n, const double *lwl, const double *gp, double mu_GP, long long *tickets);
/* The same with radial velocities (n, c, n_epochs) -- the resident launch shifts the chunk's grid itself (as
 * psoap_batch_upload_velocities: replicate_wls + lredshift, psoap/data.py:37,61) -- or with orbital parameters
 * (n, n_orb(model)): Kepler solve per epoch, the |v| >= c_kms -> -inf rule (sample_parallel.py:183-187) and the shift
 * inside the launch (as psoap_batch_upload_orbits).  psoap_chunk_set_grid / _set_dates BEFORE psoap_stream_open. */
int psoap_stream_submit_velocities(psoap_chunk *h, int n, const double *vel, const double *gp, double mu_GP, long long *tickets);
int psoap_stream_submit_orbits(psoap_chunk *h, int n, int model, const double *p_orb, const double *gp, double mu_GP,
                               long long *tickets);
/* blocks until the n results are there (any order of tickets); frees their lanes.  -inf for a negative hyper-parameter
 * (covariance.py:317) or a matrix that is not positive definite. */
int psoap_stream_fetch(psoap_chunk *h, int n, const long long *tickets, double *out);
/* blocks until one of the n tickets has its result: *which = its index (then psoap_stream_fetch of that one returns at
 * once) -- independent chains resubmit each walker the moment it completes instead of waiting for a whole group */
int psoap_stream_wait_any(psoap_chunk *h, int n, const long long *tickets, int *which);
/* *ready = 1 when the result of `ticket` has arrived (never blocks) */
int psoap_stream_ready(psoap_chunk *h, long long ticket, int *ready);
/* the resident launch leaves as soon as what is in flight is done (instead of after the idle time-out) and the call
 * returns when it has; the stream stays open and the next submit relaunches.  Call before a device-wide synchronise. */
int psoap_stream_pause(psoap_chunk *h);
/* duration (HIP events around it) of the resident launch that psoap_stream_pause ended last, and the matrices it completed */
int psoap_stream_last_launch(psoap_chunk *h, double *ms, long long *matrices);
/* waits for what is in flight, ends the resident launch, frees the stream */
int psoap_stream_close(psoap_chunk *h);
/* counters: launches of the resident kernel so far (> 1 after an idle time-out), submissions, completed results, the
 * scheme of the lanes' task list and its length; any pointer may be NULL */
int psoap_stream_stats(psoap_chunk *h, long long *launches, long long *submitted, long long *completed, int *scheme,
                       long long *tasks_per_matrix);
/* Pure host function (touches no device): the task list every lane of a stream of `lanes` lanes runs for matrices of
 * P block rows on `workers` workgroups (record format of psoap_chunk_dag_tasks; the field `b` carries the burst marks:
 * 0x8000 = the last ticket of a burst, i.e. of a block row).  scheme -1: automatic; *scheme_out the one taken. */
int psoap_stream_plan(int P, int lanes, int workers, int scheme, void *out, long long max_tasks, long long *n_tasks,
                      long long *n_slots, long long *n_ctrs, int *scheme_out);
/* Debug aids: per-task time stamps of the last `cap` submissions (allocate with out == NULL before the first submit;
 * read with nothing in flight), and the task list every lane runs (record format of psoap_chunk_dag_tasks). */
int psoap_stream_tasklog(psoap_chunk *h, int cap, unsigned long long *out, long long max_words);
int psoap_stream_tasks(psoap_chunk *h, void *out, long long max_tasks, long long *n_tasks);

/* Debug aid: the persistent kernel's task list (16-byte records: type, q, j, S, b(u16), pa, pb,
 * slot(u32), ctr(u32)) in ticket order; *n_tasks receives the list length. */
int psoap_chunk_dag_tasks(psoap_chunk *h, void *out, long long max_tasks, long long *n_tasks);

/* Pure host function (touches no device): the task list of the persistent kernel for B matrices of
 * P block rows on `workers` workgroups, same record format as psoap_chunk_dag_tasks. */
int psoap_dag_plan(int B, int P, int workers, void *out, long long max_tasks, long long *n_tasks,
                   long long *n_slots, long long *n_ctrs, unsigned int *queue_first /* 9 entries or NULL */);
/* Skyline: a handle keeps every proposal slot in ascending ln-wavelength order and evaluates the throughput
 * scheme of a batch only over the tiles that are not provably zero.  PSOAP_SKYLINE=0 in the environment when a handle is
 * created: input order and dense lists, as before.
 * psoap_dag_plan_sky: the throughput list inside the skyline first[0 .. P) (tile (q, j) exists iff q >= first[j]; first
 *   non-decreasing, first[j] <= max(j - 1, 0)); the ctr field of a final carries in bits 24.. how many tiles its block row
 *   is short of P - q.  first all zero: the list of psoap_dag_plan, byte for byte.  Inside a skyline the tiles of a block
 *   row are emitted column by column over a queue's matrices and a diagonal tile's pre-accumulation is cut by its clipped
 *   length (dag_plan.hpp); PSOAP_SKY_SPLIT=0 -- at handle creation, or when this function is called -- keeps the dense order and split rules.
 * The row order is chosen behind every upload from the slot's contents: among convex blends of the first walker's component
 * grids (1, 9, 15 candidates for 1, 2, 3 components; candidate 0 is the first component alone) the one whose union skyline
 * costs the fewest tile-GEMM units, ties to the lowest candidate.  PSOAP_SKY_ORDER=0 at handle creation: always candidate 0.
 * psoap_sky_first: host twin of the upload-side kernels pinned to candidate 0 -- the permutation perm_out (N) and the union
 *   skyline first_out (ceil(N / 128)) of a batch lwl (B, c, N), gp (B, 2c); either output may be NULL.
 * psoap_sky_order: host twin of the upload-side kernels with the choice -- the same outputs for the winning candidate, and
 *   its index in *cand_out; any output may be NULL.
 * The list is the union's over the batch; inside it the kernel clips every matrix's updates to that matrix's own skyline
 * (block rows above it are exact zeros of its factor: only products with zero are skipped, the results keep their bits).
 * PSOAP_SKY_CLIP=0 at handle creation: every matrix runs the union's ranges.
 * psoap_sky_clip: host twin of what the clip reads -- the winning candidate's per-matrix skylines first_b_out (B, ceil(N /
 *   128)), row b that of matrix b (all zero for a matrix with an unusable hyper-parameter), and in *units_out the tile-GEMM
 *   units they leave, summed over the batch; any output may be NULL.
 * The clip starts at a row, not a panel: the K-loop of an update streams 16 rows per stage, and behind every upload the
 * device also computes, per matrix and column tile, the first 16-row group that is not provably zero (same test, the row
 * interval taken over 16 rows; clamped to 8 max(j - 1, 0), non-decreasing, never above 8 times the tile-level row).  An
 * update's panels before its last start at that row; its last panel runs whole, or not at all when the row lies beyond it.
 * PSOAP_SKY_FINE=0 at handle creation: that kernel is not queued and every update starts at a whole panel.
 * psoap_sky_clip16: host twin of it -- the winning candidate's rows by 16-row groups first16_b_out (B, ceil(N / 128)) and in
 *   *stages_out the 16-row stages the updates of the union's list then run, summed over the batch and counted per tile (a
 *   tile whose update the list splits into parts runs the last panel of each part whole); any output may be NULL.
 * psoap_chunk_sky_stats: out[0 .. n) of { tiles planned, tiles dense, tile-GEMM units planned, units dense, plan builds,
 *   plan-cache hits, skyline read (0 / 1), units executed after the clip (== units planned where nothing is clipped),
 *   16-row stages of those units that run from each matrix's own first row group on (psoap_sky_clip16's figure; 8 per
 *   unit where no stage is skipped) } for the handle's last evaluation; returns the number of fields (9). */
int psoap_dag_plan_sky(int B, int P, const int *first, int workers, void *out, long long max_tasks, long long *n_tasks,
                       long long *n_slots, long long *n_ctrs, unsigned int *queue_first /* 9 entries or NULL */);
int psoap_sky_first(int c, int N, int B, const double *lwl, const double *gp, int *first_out, int *perm_out);
int psoap_sky_order(int c, int N, int B, const double *lwl, const double *gp, int *first_out, int *perm_out, int *cand_out);
int psoap_sky_clip(int c, int N, int B, const double *lwl, const double *gp, int *first_b_out, long long *units_out,
                   int *cand_out);
int psoap_sky_clip16(int c, int N, int B, const double *lwl, const double *gp, int *first16_b_out, long long *stages_out,
                     int *cand_out);
int psoap_chunk_sky_stats(psoap_chunk *h, long long *out, int n);
/* The same for a heterogeneous batch (matrices of several chunks in one launch): matrix b has Ps[b]
 * block rows. */
int psoap_dag_plan_multi(int B, const int *Ps, int workers, void *out, long long max_tasks,
                         long long *n_tasks, long long *n_slots, long long *n_ctrs,
                         unsigned int *queue_first);
/* One matrix of P block rows with Mt appended column tiles (the predict launch) and, when
 * Ms > 0, the Ms x Ms upper tiles of their Schur complement (Sigma = A - W^T W) as tasks of
 * the same launch; scheme -1 automatic, 0 throughput, 1 latency. */
int psoap_dag_plan_aug(int P, int Mt, int Ms, int workers, int scheme, void *tasks_out,
                       long long max_tasks, long long *n_tasks, long long *n_slots,
                       long long *n_ctrs, unsigned int *queue_first);

/* Pure host function: the number of persistent workgroups a batch gets -- all the device admits (two per
 * compute unit), or one per compute unit when the batch is bound by the row-to-row chains of its matrices
 * (algorithmic flops <= 3.3e9 x block rows of the largest matrix).  Ps[b]: block rows of
 * matrix b, Mt: appended column tiles (predict). */
int psoap_dag_pick_workers(int B, const int *Ps, int Mt, int compute_units, int max_workers, int *workers);

#ifdef __cplusplus
}
#endif
#endif /* PSOAP_GP_H */
