/*
 * piadmm.h -- C-ABI of the MI355X PI-ADMM consensus solver (libpiadmm.so).
 *
 * Drop-in boundary for the reference's per-MPC-step inner loop
 * (casadi/main.py:43-201 with the PI anti-windup dual update of
 * matlab_old_files/ADMM_CVX_two_veh_intesection_PI_antiwindup.m:152-188).
 *
 * The reference has no plugin API: its only solver seam is CasADi,
 *   F = ca.qpsol("solver", "osqp", {"x": u, "f": J(u), "g": g(u)}, opts); sol = F(lbg=0)
 * called once per agent per outer iteration (casadi/main.py:96,101) and once
 * per colliding pair (casadi/main.py:146,151), with the loop, collision test,
 * dual update, residuals and propagation in Python around it.  This library
 * replaces that whole loop for all agents at once: one call = one MPC step
 * (every outer ADMM iteration of every agent and pair), so the per-call
 * CasADi graph build + OSQP setup of the reference disappears.
 *
 * Conventions
 *   - return value: 0 on success, a negative PIADMM_E* code on failure;
 *     piadmm_last_error() gives the message.  Per-agent / per-pair QP status
 *     comes back in status_out (never silent, unlike the reference's
 *     error_on_fail=False at casadi/main.py:145).
 *   - all arrays are row-major fp64 (int32 for indices); the caller owns host
 *     arrays, the library copies them; the library owns all device memory.
 *   - a handle is bound to one HIP device and is not thread-safe.
 *   - multi-GPU = one process per GPU, each with its own handle over its shard of
 *     agents.  Whole components per rank need no data-path collective (global
 *     termination all-reduces 5 scalars per outer iteration); pairs across ranks add
 *     one all-reduce of the boundary exchange buffer per outer iteration
 *     (piadmm_set_scenario_shard).
 */
#ifndef PIADMM_H
#define PIADMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIADMM_ABI_VERSION 7

enum {
  PIADMM_OK = 0,
  PIADMM_E_ARG = -1,       /* bad argument / unsupported size */
  PIADMM_E_HIP = -2,       /* HIP runtime error */
  PIADMM_E_STATE = -3,     /* call out of order (e.g. step before set_scenario) */
  PIADMM_E_NODEV = -4      /* no HIP device */
};

/* dual_mode */
#define PIADMM_DUAL_PLAIN 0  /* lam += rho (p - hat)            casadi/main.py:161-162 */
#define PIADMM_DUAL_PI 1     /* per-edge PI + back-calculation  ADMM_CVX_..._PI_antiwindup.m:156-188 */
#define PIADMM_DUAL_PI_GLOBAL 2  /* PI with adaptive rho and K_P   casadi_old_PI_ADMM/main.py:133-151;
                                    with ki_adapt / d_gain / dual_init (ABI 7) the adaptive-gain
                                    variant ADMM_CVX_two_veh_intesection_adp_PI_antiwindup1.m:121-147 */

/* status_out codes per agent / pair (bit flags accumulated over one MPC step) */
#define PIADMM_QP_OK 0
#define PIADMM_QP_INEXACT 1  /* a QP hit max_inner without a certified polish */
#define PIADMM_QP_NAN 2      /* a non-finite value was produced */

/* Mirror of the reference parameters: casadi/PI_ADMM_class.py:15-28 (Bunch),
 * casadi/main.py:26-27, ADMM_CVX_..._PI_antiwindup.m:6-25,43.  Field order is
 * ABI: the Python dataclass piadmm.config.PIADMMConfig has the same fields. */
typedef struct piadmm_config {
  int32_t n_agents;
  int32_t H;                 /* num_ho, 3 <= H <= 63 (H > 32: matrices in HBM / L2) */
  int32_t max_outer;         /* iter_num */
  int32_t dual_mode;
  double dt, L, dis_thres, beta, Pnorm, Pcost, rho, eps_pri, eps_dual, u_max, du_max;
  double kP, kI, theta1, theta2, windup_sat;
  int32_t windup;            /* 1: saturation + back-calculation */
  int32_t round_decimals;    /* 4 (reference np.around) or -1 */
  int32_t collide_sq_thres;  /* 0: d^2 < dis_thres (Python), 1: d^2 < dis_thres^2 (MATLAB) */
  int32_t alias_dual_residual; /* 1: Python last_iter_hat_pos aliasing (quirk B4) */
  int32_t pos_model;         /* 0: linearised pos_old (Python), 1: nonlinear (MATLAB numeric) */
  int32_t term_dist_check;   /* 1: MATLAB extra stop condition dis_vec(2) > dis_thres */
  int32_t fixed_iters;       /* 1: run exactly max_outer iterations (throughput runs) */
  int32_t max_inner;         /* ADMM iteration cap per QP */
  double admm_rho, admm_sigma, admm_alpha, qp_tol;
  int32_t polish_every;      /* PDAS polish attempt period (ADMM iterations) */
  int32_t device;            /* HIP device ordinal */
  /* ABI 2: N-agent semantics and the hot path's remaining rows */
  int32_t term_global;       /* 1: flag / termination over ALL agents of all ranks (casadi/main.py:
                                115-118,174; one RCCL all-reduce per outer iteration when sharded);
                                0: per connected component */
  int32_t warm_duals;        /* 1: hat, lam, S, D shifted one slot into the next MPC step
                                (iterate_next_state, Distributed_planner/decentralized/optimizer.py:337-344) */
  int32_t tighten;           /* 1: delay-tightened safety distance d_eff = dis_thres + |delta_i| + |delta_j|
                                (compute_square_halfspaces_ca_prob, decentralized/util.py:70-101) */
  int32_t precision;         /* 0: fp64; 1: ADMM iteration matrices K_s^-1 stored fp32 (half the LDS),
                                polish and certificate fp64 -- answers unchanged; 2 (ABI 6): the x-step's
                                parametric tables G, X' read in fp32 where they live in HBM (H > 32, or
                                the graph kernel), fp64 accumulation and ONE fp64 refinement step
                                against the exact KKT residual, then the same certificate -- answers
                                move at the 1e-7..1e-9 level (configs[4] fp32 tolerance study) */
  double tight_p, avg_delay, var_delay;   /* VehicleConfig prob / avg_delay / var_delay (veh_config.py:25-27) */
  /* ABI 3: PIADMM_DUAL_PI_GLOBAL (casadi_old_PI_ADMM/main.py:133-151), per pair from the minimum
   * distance d of the x-step plans (nonlinear rollouts): rho = clamp(rho_num / d, rho_min, rho_max)
   * (penalty of the next x-steps and pair QPs, kept across MPC steps), K_P = min(theta1 / d,
   * theta2), lam = S + K_P e, S += kI e + 2 D, saturation +-windup_sat with back-calculation D */
  double rho_num, rho_min, rho_max;
  int32_t no_collision_gate; /* 1: every candidate pair runs its pair QP every iteration (the
                                global-PI script solves the edge problem unconditionally) */
  int32_t pi_trad;           /* ABI 7 (was reserved0), PIADMM_DUAL_PI_GLOBAL: the scripts' `trad == 1`
                                branch, lam += rho e + D then the same saturation / back-calculation
                                (casadi_old_PI_ADMM/main.py:138-139, ADMM_CVX_..._adp_PI_antiwindup1.m:131-132) */
  /* ABI 7: the adaptive-gain global PI (ADMM_CVX_two_veh_intesection_adp_PI_antiwindup1.m:121-147) */
  int32_t ki_adapt;          /* 1: K_I = kI / d_min (K_I_coeff / dis_min, :127); 0: K_I = kI (casadi_old :135) */
  int32_t reserved1;
  double d_gain;             /* S += K_I e + d_gain D: 2 (casadi_old_PI_ADMM/main.py:142), 1 (adp :135).
                                Set it to 2.0 to keep ABI 6's dual_mode 2 behaviour; with dual_mode 2 a
                                zero (e.g. a zero-initialised struct) is refused with PIADMM_E_ARG */
  double dual_init;          /* hat, lam and last_hat at every MPC step's start: 0 (casadi/main.py:56-63,
                                casadi_old :49-51) or 1e-4 (adp :59-61); nonzero excludes warm_duals */
} piadmm_config_t;

typedef struct piadmm_ctx* piadmm_handle_t;

/* Library / device queries (no handle). */
int32_t piadmm_abi_version(void);
const char* piadmm_build_info(void);           /* e.g. "gfx950 hip 7.2 ..." */
int32_t piadmm_device_count(void);
int32_t piadmm_config_size(void);              /* sizeof(piadmm_config_t), for binding checks */

/* Create / destroy.  Replaces PI_ADMM_CASADI.__init__ (casadi/PI_ADMM_class.py:13-37).
 * The configuration is checked before any device call: one without a valid solve (u_max, du_max
 * or dis_thres <= 0 or non-finite, non-finite eps_pri / eps_dual, windup with windup_sat <= 0,
 * round_decimals outside [-1, 12], ...) is refused with PIADMM_E_ARG, with or without a GPU. */
int32_t piadmm_create(const piadmm_config_t* cfg, piadmm_handle_t* out);
int32_t piadmm_destroy(piadmm_handle_t h);
const char* piadmm_last_error(piadmm_handle_t h);

/* Scenario: speeds (N), initial states (N x 3: x, y, theta), reference positions
 * (N x 2 x T, ref[i][0][t] = x, ref[i][1][t] = y; casadi/PI_ADMM_class.py:33-37)
 * and candidate pairs (E x 2, v1 < v2; any static graph: an agent's x-step sums the
 * consensus term over all its candidate neighbours, PI_ADMM_class.py:126-129, and every
 * candidate pair is collision-tested, casadi/main.py:110-113).  Resets xt to xt0. */
int32_t piadmm_set_scenario(piadmm_handle_t h, const double* spd, const double* xt0,
                            const double* ref, int32_t T, const int32_t* edges, int32_t n_edges);

/* One rank's part of a sharded job whose candidate pairs may cross ranks.
 * The arrays describe the rank's LOCAL scenario: its own agents plus a ghost copy of every
 * neighbour owned by another rank, and every pair with at least one own agent (the host
 * side, piadmm.dist.shard_graph, builds it).
 *   owned   N   1: this rank solves the agent's x-step; 0: ghost (another rank's agent)
 *   slot    N   the agent's slot in the job-wide boundary exchange buffer, -1 if none; every
 *               ghost has one, and so has every own agent with a neighbour on another rank
 *   n_slots     slots in the job (the same on every rank; 0: nothing crosses ranks)
 *   counted E   1: this rank counts the pair's residuals and termination terms (a cross-rank
 *               pair on exactly one of its ranks, e.g. the owner of v1)
 * With n_slots > 0 every outer iteration all-reduces n_slots x 3(H+1) doubles (positions and
 * controls of the boundary agents, each slot written by its owner and 0 elsewhere) between
 * the x-steps and the pair step; a cross-rank pair is solved on both of its ranks, bit-
 * identically.  Requires term_global (the job stops as one).  Transport: the RCCL
 * communicator (piadmm_comm_init) or the host callback (piadmm_set_allreduce). */
int32_t piadmm_set_scenario_shard(piadmm_handle_t h, const double* spd, const double* xt0,
                                  const double* ref, int32_t T, const int32_t* edges, int32_t n_edges,
                                  const uint8_t* owned, const int32_t* slot, int32_t n_slots,
                                  const uint8_t* counted);

/* Host all-reduce transport for jobs without RCCL (e.g. ranks sharing one GPU, or a gloo /
 * MPI host fabric): fn(ctx, buf, n) must replace buf[0..n) by its sum over all ranks of the
 * job and return 0 (non-zero aborts the step).  Used for the exchange buffer, termination
 * partials and residual histories; fn = NULL removes it. */
typedef int32_t (*piadmm_allreduce_fn)(void* ctx, double* buf, int64_t n);
int32_t piadmm_set_allreduce(piadmm_handle_t h, piadmm_allreduce_fn fn, void* ctx);

/* Overwrite the current agent states (N x 3). */
int32_t piadmm_set_xt(piadmm_handle_t h, const double* xt);

/* One MPC step at reference time index t (casadi/main.py:43-201): seeds,
 * outer ADMM loop (x-step QPs, collision graph, z-step QPs, dual update,
 * residuals, termination) and propagation of xt.  Outputs may be NULL:
 *   xt_out     N x 3        state after propagation
 *   u_out      N x H        primal_u used for propagation
 *   resid_out  C x max_outer x 2   (rk, sk) per executed iteration, NaN after
 *   iters_out  C            outer iterations executed per component
 *   status_out N + E        PIADMM_QP_* flags per agent then per pair
 * Blocking: returns after the step and the copies have finished. */
int32_t piadmm_mpc_step(piadmm_handle_t h, int32_t t, double* xt_out, double* u_out,
                        double* resid_out, int32_t* iters_out, int32_t* status_out);

/* Enqueue n_steps consecutive MPC steps starting at t0 on the handle's stream
 * without host copies or synchronisation (device-resident MPC loop: the reference's
 * `for num_step` loop, casadi/main.py:43-201).  Unless global termination with the
 * stopping test is on, up to piadmm_steps_per_launch() steps run in ONE persistent
 * launch, each component stepping through them on its own. */
int32_t piadmm_mpc_steps_async(piadmm_handle_t h, int32_t t0, int32_t n_steps);
int32_t piadmm_sync(piadmm_handle_t h);

/* Device time (ms, hipEvent on the handle's stream) of n_steps MPC steps from t0. */
int32_t piadmm_time_steps(piadmm_handle_t h, int32_t t0, int32_t n_steps, float* ms_out);

/* State of the last step, or of the last outer iteration of a host-stepped step (any pointer
 * may be NULL):
 *   xt N x 3, u N x H, pos_old N x 2 x (H+1), hat / lam / S / D E x 2 x 2 x (H+1)
 *   (direction 0 = hat_{v1 v2}, 1 = hat_{v2 v1}; S, D: the PI integral and back-calculation
 *   term of ADMM_CVX_..._PI_antiwindup.m:160-188), edge_active E, iters C.  (ABI 4: S, D added.) */
int32_t piadmm_get_state(piadmm_handle_t h, double* xt, double* u, double* pos_old,
                         double* hat, double* lam, double* S, double* D, uint8_t* edge_active, int32_t* iters);

/* Host stepping of ONE outer ADMM iteration of MPC step t (the body of
 * `for i_iter in range(iter_num)`, casadi/main.py:78-181): it = 0 starts the step (seeds, the
 * per-step reset of :52-63), it = 1, 2, ... continue it in order.  After each call
 * piadmm_get_state shows pos_old, hat, lam, S, D of that iteration.  *stop_out (may be NULL) = 1
 * when the reference's stop rules end the step at this iteration (casadi/main.py:115-118,174-178:
 * over all agents with term_global, else once every component has stopped -- a stopped
 * component keeps its state while the others continue).  Calling on after a stop, or out of
 * order, is PIADMM_E_STATE.  piadmm_step_finish then propagates (casadi/main.py:185-192); no
 * other step call is accepted while a host-stepped step is open.  (ABI 6: also a sharded graph --
 * every rank steps, the exchange all-reduce inside each call -- and a component split over
 * workgroups.) */
int32_t piadmm_outer_iter(piadmm_handle_t h, int32_t t, int32_t it, int32_t* stop_out);
int32_t piadmm_step_finish(piadmm_handle_t h, double* xt_out /* N x 3 */, double* u_out /* N x H */);

int32_t piadmm_n_components(piadmm_handle_t h);
/* MPC steps per persistent launch (after set_scenario; 1 under global natural termination). */
int32_t piadmm_steps_per_launch(piadmm_handle_t h);

/* Work counters accumulated over all steps since the last reset, summed over
 * components: [0] outer iterations executed (per component), [1] x-step QPs,
 * [2] z-step (pair) QPs, [3] ADMM iterations in x-step QPs, [4] ADMM iterations
 * in pair QPs, [5] PDAS reduced KKT solves (x), [6] PDAS reduced solves (pair),
 * [7] QPs that ended without a certified polish (PIADMM_QP_INEXACT). */
int32_t piadmm_get_counters(piadmm_handle_t h, uint64_t* out8);
int32_t piadmm_reset_counters(piadmm_handle_t h);
/* The same counters per component (C x 8 uint64, n >= 8*C). */
int32_t piadmm_get_component_counters(piadmm_handle_t h, uint64_t* out, int32_t n);

/* ABI 6: near-tie log.  The reference's loop takes discrete decisions --
 * rounding to round_decimals (casadi/main.py:48-49,103,153), the collision test d^2 < thr
 * (:112-113), the stop test rk <= eps_pri, sk <= eps_dual (:174) and MATLAB's distance check
 * dis_vec(2) > dis_thres (ADMM_CVX_..._PI_antiwindup.m:202).  Two exact implementations (this
 * library, a CPU port, the reference) agree on every continuous value to rounding, so their
 * trajectories can part only where such a decision falls within rounding of its threshold.  The
 * library records, once piadmm_set_tie_tolerance(h, tol > 0) has turned the log on, every decision
 * taken within `tol` of its threshold (1e-9 is a good choice; tol = 0, the default, turns it off:
 * the kernels then run an instantiation without the checks -- the log costs 3-10 % of a step):
 *   PIADMM_TIE_ROUND_U     an x-step control        id = agent, index = horizon slot k
 *   PIADMM_TIE_ROUND_UHAT  a pair (edge) control    id = pair,  index = side * H + k
 *   PIADMM_TIE_ROUND_SEED  a seed                   id = agent, index = 0 (x) / 1 (y)
 *     margin = value - nearest rounding boundary (k + 1/2) 10^-d, absolute, |margin| <= tol
 *   PIADMM_TIE_COLLIDE     the collision test       id = pair, index = closest slot k,
 *     margin = (min_k d_k^2 - thr) / thr (relative)
 *   PIADMM_TIE_STOP        the stop test            id = component (-1: the job under term_global),
 *     index 0: rk vs eps_pri, 1: sk vs eps_dual, margin = (r - eps) / eps (relative)
 *   PIADMM_TIE_DIST        the distance check       id = pair (-1: unknown), margin = (d - d_eff) / d_eff
 * Each event carries the reference time index of the MPC step and the outer iteration (-1: the
 * step's seeds).  Counts and events accumulate until piadmm_reset_counters; the counts are the
 * totals, and at most PIADMM_TIE_CAP device events (the kernels' decisions) plus PIADMM_TIE_CAP host
 * events (the host's stop decisions) are kept.  *n_events = the number of events written to
 * `events` (<= max_events). */
#define PIADMM_TIE_ROUND_U 0
#define PIADMM_TIE_ROUND_UHAT 1
#define PIADMM_TIE_ROUND_SEED 2
#define PIADMM_TIE_COLLIDE 3
#define PIADMM_TIE_STOP 4
#define PIADMM_TIE_DIST 5
#define PIADMM_TIE_KINDS 6
#define PIADMM_TIE_CAP 4096
typedef struct piadmm_near_tie {
  int32_t step, iter, kind, id, index, reserved;
  double margin;
} piadmm_near_tie_t;
int32_t piadmm_set_tie_tolerance(piadmm_handle_t h, double tol);
int32_t piadmm_get_near_ties(piadmm_handle_t h, uint64_t* counts /* PIADMM_TIE_KINDS, may be NULL */,
                             piadmm_near_tie_t* events /* may be NULL */, int32_t max_events, int32_t* n_events);

/* ABI 6: checkpoint / resume.  The state that carries from one MPC step to the
 * next: xt (N x 3) and, for warm_duals (a12) and the global-PI law, hat / lam / S / D / last_hat
 * (E x 2 x 2 x (H+1), the layout of piadmm_get_state; last_hat = last_iter_hat_pos,
 * casadi/main.py:180) and the global-PI pair penalties rho_pi (E).  piadmm_get_step_state reads it
 * after a step; piadmm_set_state writes it before the next (any pointer but xt may be NULL: that
 * part is zeroed, as at the reference's per-step reset, casadi/main.py:52-63; rho_pi NULL: the
 * configured rho).  A run resumed from a checkpoint continues like the uninterrupted one, to
 * rounding: the QP solvers' warm starts (active sets, labels) are not part of the checkpoint, and
 * they are guesses only -- every answer is the certified minimiser of the same QP. */
int32_t piadmm_get_step_state(piadmm_handle_t h, double* xt, double* hat, double* lam, double* S, double* D,
                              double* last_hat, double* rho_pi);
int32_t piadmm_set_state(piadmm_handle_t h, const double* xt, const double* hat, const double* lam,
                         const double* S, const double* D, const double* last_hat, const double* rho_pi);

/* Multi-GPU (term_global): one process per GPU, one handle each, joined by an RCCL
 * communicator over xGMI.  Rank 0 calls piadmm_comm_unique_id and ships the 128 bytes to
 * the other ranks (any out-of-band channel); every rank then calls piadmm_comm_init.
 * mpc_step then all-reduces the termination partials (rk, sk, active pairs, distance
 * checks) once per outer iteration, or, with fixed_iters, the residual history once per
 * MPC step, and, for a sharded graph (piadmm_set_scenario_shard), the boundary exchange
 * buffer once per outer iteration.  Without a communicator (or host transport) the
 * handle is a single-rank job. */
int32_t piadmm_comm_unique_id(uint8_t* id_out /* 128 bytes */);
int32_t piadmm_comm_init(piadmm_handle_t h, const uint8_t* id /* 128 bytes */, int32_t nranks, int32_t rank);

/* Global residual history of the last step (term_global): max_outer x 2 (rk, sk summed over
 * every active pair of every rank, NaN after the last executed iteration) and the number of
 * executed outer iterations (equal on every rank). */
int32_t piadmm_global_resid(piadmm_handle_t h, double* resid_out, int32_t* iters_out);

/* Candidate pairs for large N: all pairs i < j of the n points
 * xy (n x 2) with |xy_i - xy_j| <= radius_i + radius_j, in increasing (i, j) order, found on a
 * uniform grid hash in O(n) on the handle's device (replaces the O(N^2) pair loop of
 * casadi/main.py:110-113 as the source of the candidate graph).  With radius_i the reach bound
 * of piadmm.candidates.reach_radii no other pair can collide within the horizon: for the
 * linearised position model (pos_model 0) it is sum_k dt s sqrt(1 + (k dt s u_max / L)^2) plus half
 * the collision distance (and the delay offset with tighten) -- NOT the constant-speed s H dt,
 * which the linearised rollout can exceed.
 * Writes min(total, max_pairs) pairs to pairs_out (max_pairs x 2) and the total to
 * *n_pairs_out (call again with a larger buffer when total > max_pairs); ms_out (may be NULL):
 * device time of the detection kernels, inputs resident. */
int32_t piadmm_candidate_pairs(piadmm_handle_t h, const double* xy, const double* radius, int32_t n,
                               int32_t* pairs_out, int32_t max_pairs, int32_t* n_pairs_out, float* ms_out);

/* Diagnostic builds (-DPIADMM_STAMPS, libpiadmm_stamps.so) only: per-component
 * cycle sums of the kernel phases (C x 32 uint64); PIADMM_E_STATE otherwise. */
int32_t piadmm_debug_stamps(piadmm_handle_t h, uint64_t* out, int32_t n);

/* ---- OBCA local subproblem ------------------------------------------
 * Replaces the vehicle side of the OBCA-ADMM planner: OBCAOptimizer.local_initialize,
 * local_build_model, local_generate_constrain, local_generate_variable, local_generate_object and
 * local_solve (Distributed_planner/decentralized/optimizer.py:40-201) -- one CasADi/IPOPT NLP per
 * vehicle per ADMM iterate (decentralized_overtaking_ADMM.py:49-63) -- with a batched SQP on the
 * device: n independent local NLPs (kinematic bicycle, N_horz 8, OBCA dual-distance constraints
 * against the other vehicle's exchanged halfspaces), one wavefront each, one launch.
 *
 * recs: n x PIADMM_OBCA_REC fp64 records, each
 *   init[5] | ref[8][5] (ref_traj[veh][t_step + k]) | A_o[7][4][2] | b_o[7][4] | lamb_ij_o[7][4]
 *   (bar_state.A/b/lamb_ij of the OTHER vehicle) | lamb_bar[7][9] | Z_bar[7][9] (this vehicle's) |
 *   rho, min_dis, max_x, max_y, r, q, prob (0/1: util.py:48-68 or :70-101 halfspaces),
 *   max_sqp_iters | pad.
 * out: n x PIADMM_OBCA_OUT fp64: X[8][5] | U[7][2] | Lambda[7][4] (local_solve's x_opt..steer_opt,
 *   a_opt, steerate_opt, lambda_loc, :183-201) | multipliers y_a[7] y_b[7][2] y_n[7] y_x[7][5]
 *   pi[7][5] y_u[14] y_l[28] | cost | pad.
 * status3: n x 3 int32: PIADMM_OBCA_* status, SQP iterations, QP active-set steps.
 * The NLP is the reference's as written; the solver is not IPOPT. */
#define PIADMM_OBCA_REC 296
#define PIADMM_OBCA_OUT 224
#define PIADMM_OBCA_CONVERGED 0
#define PIADMM_OBCA_MAX_ITER 1
#define PIADMM_OBCA_QP_INFEASIBLE 2
#define PIADMM_OBCA_LINESEARCH_FAIL 3
#define PIADMM_OBCA_HESSIAN_FAIL 4

typedef struct piadmm_obca_s* piadmm_obca_t;
int32_t piadmm_obca_create(int32_t device, piadmm_obca_t* out);
int32_t piadmm_obca_destroy(piadmm_obca_t h);
const char* piadmm_obca_last_error(piadmm_obca_t h);
/* upload + one launch + download (synchronous) */
int32_t piadmm_obca_solve(piadmm_obca_t h, const double* recs, int32_t n, double* out, int32_t* status3);
/* resident batch: upload once, launch, time, download.  Block b of a launch solves problem
 * order[b]: longest first by the QP steps each problem took in the previous run of the SAME upload
 * (index order on the first run after an upload), so the longest problems start in the first
 * dispatch wave; the answers do not depend on the order.  piadmm_obca_run blocks: it reads the
 * previous run's per-problem work back to the host (a device-to-host copy and stream syncs) and
 * uploads the order before it enqueues its launches, which then run asynchronously on the handle's
 * stream (piadmm_obca_download / _time synchronise). */
int32_t piadmm_obca_upload(piadmm_obca_t h, const double* recs, int32_t n);
int32_t piadmm_obca_run(piadmm_obca_t h, int32_t repeats);
int32_t piadmm_obca_time(piadmm_obca_t h, int32_t repeats, float* ms_per_launch);
int32_t piadmm_obca_download(piadmm_obca_t h, double* out, int32_t* status3, int32_t n);
/* Diagnostic builds (-DPIADMM_STAMPS) only: per-problem cycle sums of the SQP phases and event
 * counts of the last launch (n = 16 x batch uint64); PIADMM_E_STATE otherwise. */
int32_t piadmm_obca_debug_stamps(piadmm_obca_t h, uint64_t* out, int32_t n);

/* ---- OBCA-ADMM edge (RSU) step -------------------------------------------------------------
 * The coordinator half of an ADMM iterate: the edge NLP on the consensus variable Z
 * (optimizer.py:239-328) and lambda_update (:330-335) fused behind it.  The NLP is separable over
 * the 7 horizon slots: one vehicle pair is 7 slot problems in
 * z = [s_0 (5), mu_0 (4), s_1 (5), mu_1 (4)],
 *   min  -z.lamb_bar + rho/2 |w - z|^2,  w = [local_x, lamb_ij]
 *   s.t. A(s_0)' mu_0 + A(s_1)' mu_1 = 0,  min_dis <= -b(s_0)' mu_0 - b(s_1)' mu_1 <= g_max,
 *        |s| <= x_bound, 0 <= mu <= mu_max,
 * one wavefront each, n_pairs x 7 per launch; the same wave then writes Z_bar (Z rounded to
 * round_decimals, -1 = off), lamb_bar_new = lamb_bar + rho (w - Z_bar) and the slot's
 * sum |lamb_bar_new - lamb_bar| partial (dres; the host adds the 7 in index order).  A slot whose
 * status wrote no iterate (QP_INFEASIBLE, HESSIAN_FAIL) leaves lamb_bar unchanged, dres = 0.
 *
 * recs: n_pairs x PIADMM_OBCA_EDGE_REC fp64: local_x[2][7][5] | lamb_ij[2][7][4] | lamb_bar[2][7][9] |
 *   rho, min_dis, prob, max_iter, round_decimals, start (0: zeros, 1: w clipped into the bounds),
 *   x_bound, mu_max, g_max | pad.
 * out: n_pairs x PIADMM_OBCA_EDGE_OUT fp64: Z[2][7][9] unrounded | Z_bar[2][7][9] |
 *   lamb_bar_new[2][7][9] | y_eq[7][2] | y_in[7] | y_bnd[7][18] | cost[7] | dres[7] | pad.
 * status3: n_pairs x 7 x 3 int32: PIADMM_OBCA_* status, SQP iterations, QP active-set steps.
 * Records with rho <= 0, prob not 0/1, max_iter outside [1, 1000], start not 0/1, round_decimals
 * outside [-1, 15], or x_bound or mu_max <= 0 are refused before any launch
 * ("record k: bad parameters").  The edge buffers are the handle's own: a call between
 * piadmm_obca_upload and piadmm_obca_download leaves the resident local batch as it was. */
#define PIADMM_OBCA_EDGE_REC 264
#define PIADMM_OBCA_EDGE_OUT 544
int32_t piadmm_obca_edge_solve(piadmm_obca_t h, const double* recs, int32_t n_pairs, double* out,
                               int32_t* status3);
/* upload + `repeats` launches between two events; ms per launch */
int32_t piadmm_obca_edge_time(piadmm_obca_t h, const double* recs, int32_t n_pairs, int32_t repeats,
                              float* ms_per_launch);

/* ---- OBCA-ADMM consensus loop, device-resident ---------------------------------------------
 * The loop of decentralized_overtaking_ADMM.py:31-102 for n_scenarios vehicle pairs at once, the
 * planner state resident on the device: per ADMM iterate one launch each of pack-local, the local
 * SQP (scenarios x 2), exchange (bar_state_update, check_converge and the edge record), the edge
 * SQP with the fused lambda_update, residual (the stop rule of :82-86) and an order-keeping
 * compaction of the scenarios still active; the host reads back 4 bytes per iterate (their count).
 * A stopped scenario is not resubmitted; on termination the horizon shift takes the PREVIOUS
 * iterate's state (:87) and init_state = X[1] (:99).
 *
 * State of one scenario (PIADMM_OBCA_PLAN_STATE fp64):
 *   Z_bar[2][7][9] | A[2][7][4][2] | b[2][7][4] | lamb_bar[2][7][9] | lamb_ij[2][7][4] |
 *   local_x[2][7][5] | init_state[2][5]
 *
 * piadmm_obca_plan_begin checks the configuration before any launch (rho, r, q, max_x, max_y,
 * x_bound, mu_max > 0; prob[k] 0/1; 1 <= max_sqp_iter <= 1000; start and update_lamb_ij 0/1;
 * -1 <= round_decimals <= 15; n_scenarios >= 1; max_admm_iter >= 0; 0 <= t_step0 and
 * t_step0 + 8 <= n_ref), copies prob, the thresholds (one per scenario), ref_traj and the state
 * (which becomes both the current and the previous iterate's), and opens MPC step t_step0.
 * It takes the handle's local and edge device buffers over: afterwards piadmm_obca_run, _time and
 * _download return PIADMM_E_STATE until the next piadmm_obca_upload.  Any upload into those buffers
 * (piadmm_obca_upload / _solve / _edge_solve / _edge_time) ends the plan as piadmm_obca_plan_end does.
 *
 * piadmm_obca_plan_iterate runs one ADMM iterate of the open MPC step on the scenarios still
 * active and returns how many remain active; PIADMM_E_STATE without an open plan, with no active
 * scenario left (call piadmm_obca_plan_shift) or when t_step + 8 > n_ref ("reference exhausted").
 * piadmm_obca_plan_shift closes the step (iterate_next_state of the frozen previous state into both
 * states, init_state = X[1], t_step += 1, every scenario active again); PIADMM_E_STATE while
 * scenarios are active.  piadmm_obca_plan_step = iterate until none is active (at most
 * max_admm_iter + 1 iterates), then shift; iters_out: the iterate each scenario stopped at.
 *
 * piadmm_obca_plan_get copies one item to the host; `bytes` must be the item's size exactly
 * (PIADMM_E_ARG otherwise).  n = n_scenarios, m = the number of scenarios submitted to the last
 * iterate (0 before the first iterate of a step):
 *   STATE, STATE_PREV   n x 556 fp64     the current / the previous iterate's state
 *   CTRL, CTRL_PREV     n x 2 x 14 fp64  [U[:,0], U[:,1]] per vehicle (CTRL_PREV: zeros at a step's start)
 *   X                   n x 2 x 8 x 5 fp64   the last local solution of each scenario
 *   ITERS               n int32          the iterate each scenario stopped at (0: still active)
 *   ACTIVE              m int32          the scenarios submitted to the last iterate, ascending
 *                       (longest first with piadmm_obca_order_plan attached, below)
 *   PRIMAL, DUAL        n fp64           the residuals of each scenario's last iterate
 *   STOP, CONVERGE      n int32          the stop decision / check_converge of its last iterate
 *   LOCAL_REC / _OUT / _IST   2m x PIADMM_OBCA_REC / 2m x PIADMM_OBCA_OUT fp64 / 2m x 3 int32
 *                       record 2k + v: vehicle v of scenario ACTIVE[k]
 *   EDGE_REC / _OUT / _IST    m x PIADMM_OBCA_EDGE_REC / m x PIADMM_OBCA_EDGE_OUT fp64 / m x 7 x 3 int32
 *   T_STEP              1 int32          the open MPC step
 *   LAMBDA              n x 2 x 7 x 9 fp64   lamb_bar of each scenario's last iterate in the step
 *                       closed last (what the script's lambda_record keeps, :103)
 *   COUNTS              3 int32          m, the number still active, the iterates run in the open step
 *   STATUS_MASK         n x 2 int32      OR of (1 << status) over the local / the edge solves of the
 *                       scenario in the step closed last (in the open step before the shift)
 *   REF                 rows x 2 x n_ref x 5 fp64   the references as uploaded
 *   PAR                 rows x PIADMM_OBCA_FLEET_PAR fp64   the parameter rows as uploaded
 *                       rows = 1 (the shared row) after piadmm_obca_plan_begin, n after piadmm_obca_fleet_begin
 *
 * piadmm_obca_fleet_begin opens the same plan with a reference and a parameter row per scenario
 * (a fleet, a Monte-Carlo study over speeds and gaps, a sweep over rho and min_dis in one batch);
 * piadmm_obca_plan_iterate / _shift / _step / _get / _end, the buffer takeover and the "an upload
 * ends the plan" rule apply to it unchanged.  A row of `par` holds, in order,
 *   rho, min_dis, conv_thres, max_x, max_y, r, q, x_bound, mu_max, g_max,
 *   max_admm_iter, max_sqp_iter, round_decimals, start, 0, 0
 * the integers stored as doubles, as the records store them.  cfg carries what stays shared
 * (n_scenarios, t_step0, n_ref, update_lamb_ij); its other fields are the row of every scenario
 * when par is NULL.  Every row passes the checks of piadmm_obca_plan_begin and its integers must be
 * integral, before any device call: a bad row is PIADMM_E_ARG with "obca_fleet_begin: row k: ..."
 * and an open plan stays as it was.  A scenario stops at i_iter > its own max_admm_iter;
 * piadmm_obca_plan_step runs at most the largest max_admm_iter of the rows, plus one, iterates.
 * The vehicle geometry and the delay statistics are constants of the solver kernels and n_ref is
 * the plan's: none of them is per scenario.  t_step is the plan's too unless a clock is attached
 * (piadmm_obca_clock_plan, below): then every scenario reads its reference at its own step and
 * over its own length. */
#define PIADMM_OBCA_PLAN_STATE 556
#define PIADMM_OBCA_PLAN_GET_STATE 0
#define PIADMM_OBCA_PLAN_GET_STATE_PREV 1
#define PIADMM_OBCA_PLAN_GET_CTRL 2
#define PIADMM_OBCA_PLAN_GET_CTRL_PREV 3
#define PIADMM_OBCA_PLAN_GET_X 4
#define PIADMM_OBCA_PLAN_GET_ITERS 5
#define PIADMM_OBCA_PLAN_GET_ACTIVE 6
#define PIADMM_OBCA_PLAN_GET_PRIMAL 7
#define PIADMM_OBCA_PLAN_GET_DUAL 8
#define PIADMM_OBCA_PLAN_GET_STOP 9
#define PIADMM_OBCA_PLAN_GET_CONVERGE 10
#define PIADMM_OBCA_PLAN_GET_LOCAL_REC 11
#define PIADMM_OBCA_PLAN_GET_LOCAL_OUT 12
#define PIADMM_OBCA_PLAN_GET_LOCAL_IST 13
#define PIADMM_OBCA_PLAN_GET_EDGE_REC 14
#define PIADMM_OBCA_PLAN_GET_EDGE_OUT 15
#define PIADMM_OBCA_PLAN_GET_EDGE_IST 16
#define PIADMM_OBCA_PLAN_GET_T_STEP 17
#define PIADMM_OBCA_PLAN_GET_LAMBDA 18
#define PIADMM_OBCA_PLAN_GET_COUNTS 19
#define PIADMM_OBCA_PLAN_GET_STATUS_MASK 20
#define PIADMM_OBCA_PLAN_GET_REF 21
#define PIADMM_OBCA_PLAN_GET_PAR 22
#define PIADMM_OBCA_PLAN_GET_DUAL_S 23
#define PIADMM_OBCA_PLAN_GET_DUAL_D 24
#define PIADMM_OBCA_PLAN_GET_DUAL_PAR 25
#define PIADMM_OBCA_PLAN_GET_WORK 26
#define PIADMM_OBCA_PLAN_GET_CLOCK 27
#define PIADMM_OBCA_PLAN_GET_WINDOW 28
#define PIADMM_OBCA_FLEET_PAR 16
typedef struct {
  int32_t n_scenarios, t_step0, max_admm_iter, round_decimals, start, update_lamb_ij, max_sqp_iter, n_ref;
  double rho, min_dis, conv_thres, max_x, max_y, r, q, x_bound, mu_max, g_max;
} piadmm_obca_plan_cfg_t;
int32_t piadmm_obca_plan_cfg_size(void);
int32_t piadmm_obca_plan_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                               const double* primal_thres, const double* dual_thres,
                               const double* ref_traj /* 2 x n_ref x 5 */, const double* state /* n x 556 */);
int32_t piadmm_obca_plan_iterate(piadmm_obca_t h, int32_t* n_active_after);
int32_t piadmm_obca_plan_shift(piadmm_obca_t h);
int32_t piadmm_obca_plan_step(piadmm_obca_t h, int32_t* iters_out /* n, may be NULL */);
int32_t piadmm_obca_plan_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes);
int32_t piadmm_obca_plan_end(piadmm_obca_t h);
int32_t piadmm_obca_fleet_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                                const double* primal_thres, const double* dual_thres,
                                const double* ref_traj /* n x 2 x n_ref x 5 */,
                                const double* par      /* n x PIADMM_OBCA_FLEET_PAR, may be NULL */,
                                const double* state    /* n x 556 */);

/* ---- the run record ("trace") of an open plan, and the clearance of a state pair -----------
 * piadmm_obca_clearance: the exact minimum Euclidean distance between the two vehicles'
 * rectangles (generate_vehicle_vertices, util.py:34-42: centre x, y, heading state[3], 3.5 x 2.0)
 * at each of n state pairs, out[k] = {plain, tight}: `plain` for those rectangles, `tight` for the
 * delay-tightened ones the planner constrains (compute_square_halfspaces_ca_prob, util.py:70-101:
 * each centre moved by delta_avg + sqrt(p / (1 - p)) delta_var); prob[k] = 0 gives the plain value
 * twice.  The distance is 0 when no edge normal of either rectangle separates them, else the
 * minimum of the 32 vertex-to-edge distances.  The call has its own device buffers: the handle's
 * local and edge buffers and an open plan stay as they are.  Before any device call: 1 <= n <= 2^20,
 * non-null pointers, prob 0 or 1, every state finite (PIADMM_E_ARG otherwise).
 *
 * piadmm_obca_trace_begin attaches a record of capacity cap_steps MPC steps to the open plan
 * (device arrays; a second call replaces the first) and writes its row 0: every scenario's current
 * init_state and its clearances.  Only at a step boundary (no iterate of the open step has run):
 * PIADMM_E_STATE otherwise; cap_steps < 1 (or > 2^20) or unknown flag bits are PIADMM_E_ARG.
 * flags: PIADMM_OBCA_TRACE_LAMBDA also keeps each step's lamb_bar (126 fp64 per scenario and step).
 * While a trace is attached piadmm_obca_plan_shift -- called directly, by piadmm_obca_plan_step or
 * by piadmm_obca_trace_run -- appends one row for the step it closes, on the device: the new
 * init_state and its clearances, the stop iterate, both status masks, the stopping iterate's
 * residuals and, with the flag, the step's lamb_bar; each scenario's running minimum clearances are
 * kept with the row the plain minimum was first reached at.  Nothing is read back for it.  With the
 * trace full, piadmm_obca_plan_shift and piadmm_obca_plan_step return PIADMM_E_STATE ("trace
 * full") before any launch and the plan stays as it was.  Without a trace the plan calls are as before.
 *
 * piadmm_obca_trace_run runs n_steps MPC steps (piadmm_obca_plan_step each; steps_done, may be
 * NULL, counts the completed ones).  PIADMM_E_STATE with nothing run when the steps do not fit the
 * trace (rows + n_steps > cap_steps) or the reference (t_step + n_steps - 1 + 8 > n_ref).
 *
 * piadmm_obca_trace_get copies one item; `bytes` must be exact.  R = the steps recorded, n = n_scenarios:
 *   STATES        (R + 1) x n x 2 x 5 fp64   row 0: where the trace was attached; row r: init_state after step r
 *   CLEARANCE     (R + 1) x n x 2 fp64       {plain, tight} of the same rows
 *   ITERS         R x n int32                the iterate each scenario stopped at
 *   STATUS_MASK   R x n x 2 int32            as PIADMM_OBCA_PLAN_GET_STATUS_MASK, per step
 *   PRIMAL, DUAL  R x n fp64                 the residuals of each scenario's stopping iterate
 *   LAMBDA        R x n x 2 x 7 x 9 fp64     as PIADMM_OBCA_PLAN_GET_LAMBDA, per step (PIADMM_E_STATE without the flag)
 *   SUMMARY       n x 4 fp64                 min plain clearance over the rows, its row (the first such),
 *                                            min tightened clearance, sum of the stop iterates
 *   ROWS          1 int32                    R
 * piadmm_obca_trace_end frees the trace alone; piadmm_obca_plan_end, a new piadmm_obca_plan_begin /
 * _fleet_begin and any upload that ends the plan free it too.  Every trace call without an open plan
 * or an attached trace is PIADMM_E_STATE (piadmm_obca_trace_end: 0). */
#define PIADMM_OBCA_TRACE_LAMBDA 1
#define PIADMM_OBCA_TRACE_GET_STATES 0
#define PIADMM_OBCA_TRACE_GET_CLEARANCE 1
#define PIADMM_OBCA_TRACE_GET_ITERS 2
#define PIADMM_OBCA_TRACE_GET_STATUS_MASK 3
#define PIADMM_OBCA_TRACE_GET_PRIMAL 4
#define PIADMM_OBCA_TRACE_GET_DUAL 5
#define PIADMM_OBCA_TRACE_GET_LAMBDA 6
#define PIADMM_OBCA_TRACE_GET_SUMMARY 7
#define PIADMM_OBCA_TRACE_GET_ROWS 8
int32_t piadmm_obca_clearance(piadmm_obca_t h, int32_t n, const double* states /* n x 2 x 5 */,
                              const int32_t* prob /* n */, double* out /* n x 2: plain, tight */);
int32_t piadmm_obca_trace_begin(piadmm_obca_t h, int32_t cap_steps, int32_t flags);
int32_t piadmm_obca_trace_run(piadmm_obca_t h, int32_t n_steps, int32_t* steps_done);
int32_t piadmm_obca_trace_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes);
int32_t piadmm_obca_trace_end(piadmm_obca_t h);

/* ---- the PI anti-windup dual law of an open plan --------------------------------------------
 * The plan's dual update is lamb_bar += rho (w - Z_bar) (optimizer.py:330-335), fused behind the
 * edge solve.  piadmm_obca_dual_plan attaches a second law to the open plan, the per-edge PI with
 * back-calculation of ADMM_CVX_two_veh_intesection_PI_antiwindup.m:156-188 with a constant
 * proportional gain, on the plan's consensus error.  For every entry i of [vehicle 2][slot 7][9]
 * in a slot whose edge solve wrote an answer (status CONVERGED, MAX_ITER or LINESEARCH_FAIL):
 *   e    = w[i] - Zb[i]              w = [local_x, lamb_ij] of the edge record, Zb the rounded Z
 *   S'   = S[i] + kI e + d_gain D[i]
 *   raw  = S' + kP e
 *   lam' = windup ? min(sat, max(raw, -sat)) : raw
 *   D'   = windup ? lam' - raw : 0
 * products and sums uncontracted; every other slot (any other status value) keeps lamb_bar, S and D
 * and adds 0 to the dual residual, which is sum |lam' - lam| in the order of the plain path.
 * A gains row is PIADMM_OBCA_DUAL_PAR doubles: kP, kI, windup_sat, d_gain, windup (0 / 1), 0, 0, 0.
 * rows = 1 (every scenario reads the one row) or n (one row per scenario).  Checked before any
 * device call: every entry finite, windup 0 or 1, windup_sat > 0 with windup set, the trailing
 * entries 0; a bad row is PIADMM_E_ARG with "obca_dual_plan: row k: ..." and the plan, with a law
 * attached before, stays as it was.  gains NULL or rows 0 detaches the law: the plan is plain again.
 * Only at a step boundary (no iterate of the open step has run): PIADMM_E_STATE otherwise, as for
 * piadmm_obca_trace_begin; for a plan of piadmm_obca_plan_begin or of piadmm_obca_fleet_begin alike.
 * Attaching sets S = lamb_bar of the current state and D = 0, so kP = 0, kI = rho, windup = 0 is
 * the plain update to rounding.  While attached, every iterate runs one more launch between the
 * edge solve and the residual, which overwrites lamb_bar_new and the 7 dres partials of the edge
 * output in place: PIADMM_OBCA_PLAN_GET_EDGE_OUT then shows the law's values in those two fields,
 * and the state, the dual residual, the stop rule, LAMBDA and the trace follow them.  The horizon
 * shift takes, as it does for the state (B16), the integrator of the iterate before the stopping
 * one, one slot on with the last slot repeated.  piadmm_obca_plan_get gains
 *   DUAL_S, DUAL_D      n x 2 x 7 x 9 fp64   the integrator and the back-calculation term
 *   DUAL_PAR            rows x PIADMM_OBCA_DUAL_PAR fp64   the gains rows as uploaded
 * (PIADMM_E_STATE without a law).  piadmm_obca_plan_end, a new piadmm_obca_plan_begin /
 * _fleet_begin and any upload that ends the plan free the law.  Without a law the plan runs the
 * launches it ran before.
 *
 * piadmm_obca_dual_pi applies the law once to the caller's arrays (w, zb, lamb, S, D and lamb_out
 * n x 126 in the layout above, status and dres_out n x 7; S and D in / out), one launch of the same
 * kernel on the call's own device buffers: the handle's buffers and an open plan stay as they are.
 * Before any device call: 1 <= n <= 2^20, non-null pointers, rows 1 or n, the gains rows as above
 * ("obca_dual_pi: row k: ..."), every input finite (PIADMM_E_ARG otherwise). */
#define PIADMM_OBCA_DUAL_PAR 8
int32_t piadmm_obca_dual_plan(piadmm_obca_t h, const double* gains /* rows x PIADMM_OBCA_DUAL_PAR, may be NULL */,
                              int32_t rows);
int32_t piadmm_obca_dual_pi(piadmm_obca_t h, int32_t n, const double* w, const double* zb, const double* lamb,
                            const int32_t* status /* n x 7 */, const double* gains, int32_t rows,
                            double* S, double* D, double* lamb_out, double* dres_out /* n x 7 */);

/* ---- longest-first scenario order inside an open plan ----------------------------------------
 * Both solves of an iterate run one wavefront per problem in the order of the active list, and a
 * launch lasts as long as its longest wave: a solve that runs to the SQP cap and starts last adds
 * its whole length to the launch, started first it hides behind the rest.  Every scenario's answer
 * is independent of its place in the list (bit for bit), so the list may be put in any order.
 *
 * piadmm_obca_order_plan, mode 1, attaches the order to the open plan: a record work[s] = (Q, I)
 * per scenario, Q the largest QP step count and I the largest SQP iteration count (ist[.][2] and
 * ist[.][1]) over the scenario's 2 local and 7 edge solves of the last iterate it was active in,
 * kept on the device by one more launch per iterate; a scenario that did not run keeps its pair.
 * The record starts at 0, or at work_init (n x 2: what an earlier run of the same fleet left in
 * PIADMM_OBCA_PLAN_GET_WORK schedules the first step).  While attached, every active list -- the
 * one the compaction leaves for the next iterate and the full one piadmm_obca_plan_shift leaves
 * for the next step -- is sorted on the device by
 *   Q descending, then I descending, then scenario ascending
 * (Q and I compared after clamping to 2^21 - 1), a strict total order: the list is a function of
 * the set of scenarios in it and of the record alone, the same on every run.  No position is
 * decided by an atomic; no kernel waits for another workgroup.  PIADMM_OBCA_PLAN_GET_ACTIVE and
 * the LOCAL_ / EDGE_ items then follow that order instead of the ascending one; every per-scenario
 * item, the trace and the dual law are unchanged, bit for bit.  The 4 bytes read back per iterate
 * stay the only ones.  Attaching sorts the current list at once (zero work: ascending, no change).
 * mode 0 detaches: the list is ascending again, the record is freed and the plan runs the launches
 * it ran before.  Checked before any device call: an open plan (PIADMM_E_STATE), mode 0 or 1,
 * work_init >= 0 ("obca_order_plan: row k: ..."), n_scenarios < 2^21 (PIADMM_E_ARG), and a step
 * boundary (no iterate of the open step has run: PIADMM_E_STATE); a refused call leaves the plan as
 * it was.  piadmm_obca_plan_get gains
 *   WORK                n x 2 int32      the record (Q, I) per scenario (PIADMM_E_STATE without the order)
 * piadmm_obca_plan_end, a new piadmm_obca_plan_begin / _fleet_begin and any upload that ends the
 * plan free the record.
 *
 * piadmm_obca_order sorts the caller's list (m distinct scenarios below n) by the caller's work
 * (n x 2) into out (m), one launch of the same kernel on the call's own device buffers: the
 * handle's buffers and an open plan stay as they are.  Before any device call: 1 <= m <= n < 2^21,
 * non-null pointers, every list entry a scenario below n and listed once, work >= 0 (PIADMM_E_ARG). */
int32_t piadmm_obca_order_plan(piadmm_obca_t h, int32_t mode, const int32_t* work_init /* n x 2, may be NULL */);
int32_t piadmm_obca_order(piadmm_obca_t h, const int32_t* list /* m */, int32_t m, const int32_t* work /* n x 2 */,
                          int32_t n, int32_t* out /* m */);

/* ---- per-scenario clocks inside an open plan: mixed phases, retiring, admission ---------------
 * A plan has one clock: every scenario reads its reference at the plan's t_step, and the plan ends
 * for all of them when t_step + 8 > n_ref.  piadmm_obca_clock_plan, mode 1, attaches a record
 *   clock[s] = (c, len, alive), three int32
 * per scenario: c the row of its own reference that slot 0 of its horizon reads (its own MPC step),
 * len the number of valid rows of its reference (8 <= len <= n_ref), alive = (c + 8 <= len).
 * clock_init holds (c0, len) per scenario; NULL is c0 = t_step, len = n_ref for everyone, and the
 * plan then computes what it computed without the clock, bit for bit.  Rows are checked before any
 * device call (c0 >= 0, 8 <= len <= n_ref, c0 + 8 <= len): a bad row is PIADMM_E_ARG with
 * "obca_clock_plan: row k: ...".  Only at a step boundary (PIADMM_E_STATE otherwise, as for
 * piadmm_obca_trace_begin); for a plan of piadmm_obca_plan_begin (one shared reference read at
 * different phases) or of piadmm_obca_fleet_begin alike; a second attach replaces the record.
 * mode 0 detaches, only while every scenario is alive, all c are equal and every len == n_ref
 * (PIADMM_E_STATE otherwise): the plan's t_step becomes that common c and the plan is plain again,
 * running the launches it ran before.  A refused call leaves the plan as it was.
 *
 * While attached the device keeps a window ref_s[v][c .. c + 7] per scenario (n x 2 x 8 x 5 fp64,
 * exact copies) and the local records are packed from it, so they are bit-equal to what the plain
 * plan packs at t_step = c.  A step runs the scenarios that were alive when it opened;
 * piadmm_obca_plan_shift closes it for exactly those (the state shift, init_state = X[1], the
 * CTRL_PREV reset, LAMBDA and, with a dual law, the integrator shift), then c += 1 for them, alive
 * is recomputed, the windows of the alive scenarios are refreshed and the next list is the alive
 * scenarios ascending (longest first with piadmm_obca_order_plan attached).  The record evolves
 * deterministically and the host keeps a mirror of it: nothing more is read back per iterate or per
 * step.  A retired scenario (alive = 0) is frozen: its STATE, STATE_PREV, X, CTRL, LAMBDA, DUAL_S,
 * DUAL_D, WORK and WINDOW stay as its last shift left them, its ITERS and STATUS_MASK are 0 in
 * every later step, and its PRIMAL / DUAL (and STOP / CONVERGE) keep the values of its last iterate.
 * With no scenario alive piadmm_obca_plan_iterate, piadmm_obca_plan_step and piadmm_obca_trace_run
 * return PIADMM_E_STATE ("no scenario alive") before any launch; this replaces "reference
 * exhausted".  T_STEP keeps counting the plan's steps and may pass n_ref - 8.  A trace keeps one row
 * per plan step for all n: a retired scenario's row repeats its frozen init_state and clearance, has
 * iterate 0 and masks 0 (its PRIMAL / DUAL / LAMBDA entries repeat the frozen values), adds 0 to the
 * summary's sum and cannot move the running minimum's row (the comparison is strict).
 * piadmm_obca_trace_run refuses n_steps larger than the steps the longest-lived scenario has left,
 * max over the alive of len - 8 - c + 1.  piadmm_obca_plan_get gains
 *   CLOCK               n x 3 int32          (c, len, alive) per scenario
 *   WINDOW              n x 2 x 8 x 5 fp64   the reference window of each scenario (a retired one's: its last)
 * (PIADMM_E_STATE without a clock).  piadmm_obca_plan_end, a new piadmm_obca_plan_begin /
 * _fleet_begin and any upload that ends the plan free the record.
 *
 * piadmm_obca_clock_admit puts m new tenants into the slots `slots` (distinct, below n; a slot need
 * not be retired) of the open plan.  Only at a step boundary, with a clock and without a trace
 * attached (a trace's running minima would mix two tenants): PIADMM_E_STATE otherwise.  clock holds
 * (c0, len) per tenant and is required; every other array may be NULL, which keeps what the slot
 * has.  A non-NULL ref or par needs a plan with n rows of that kind (piadmm_obca_fleet_begin):
 * PIADMM_E_STATE otherwise.  Before any device call the par rows pass the checks of
 * piadmm_obca_fleet_begin, prob is 0 or 1 and the clock rows pass the checks above: a bad row is
 * PIADMM_E_ARG with "obca_clock_admit: row k: ..." and the plan is unchanged.  Of every admitted
 * slot both state copies are set to `state`, CTRL, CTRL_PREV, X, LAMBDA, ITERS and STATUS_MASK are
 * zeroed, with a dual law S = S_prev = lamb_bar of the slot's state and D = D_prev = 0, with the
 * order WORK = (0, 0); then the largest max_admm_iter is taken over the current rows and the
 * windows, the alive flags and the active list are rebuilt.  The admitted tenant then computes what
 * a fresh plan opened at t_step0 = c0 on the same state, reference and row computes.
 *
 * piadmm_obca_clock_tick runs the tick, window and compaction kernels alone on the call's own
 * device buffers (the handle's buffers and an open plan stay as they are): clock_out[s] =
 * (c + ran[s], len, alive), window_out[s] = ref_s[v][c' .. c' + 7] of an alive scenario (zeros
 * otherwise), list_out = the alive scenarios ascending (count_out[0] of them, zeros behind).
 * ref_rows = 1 (one reference for all) or n.  Before any device call: 1 <= n <= 2^20, non-null
 * pointers, ref_rows 1 or n, 8 <= n_ref <= 2^20, 0 <= c <= 2^30, 8 <= len <= n_ref, ran 0 or 1
 * ("obca_clock_tick: row k: ...", PIADMM_E_ARG). */
int32_t piadmm_obca_clock_plan(piadmm_obca_t h, int32_t mode, const int32_t* clock_init /* n x 2: c0, len; may be NULL */);
int32_t piadmm_obca_clock_admit(piadmm_obca_t h, int32_t m, const int32_t* slots /* m */,
                                const int32_t* clock /* m x 2: c0, len */,
                                const double* state /* m x 556 or NULL */,
                                const double* ref /* m x 2 x n_ref x 5 or NULL */,
                                const double* par /* m x PIADMM_OBCA_FLEET_PAR or NULL */,
                                const int32_t* prob /* m or NULL */, const double* primal_thres /* m or NULL */,
                                const double* dual_thres /* m or NULL */);
int32_t piadmm_obca_clock_tick(piadmm_obca_t h, int32_t n, const int32_t* clock_in /* n x 3 */,
                               const int32_t* ran /* n, 0 / 1 */, const double* ref, int32_t ref_rows /* 1 or n */,
                               int32_t n_ref, int32_t* clock_out /* n x 3 */, double* window_out /* n x 2 x 8 x 5 */,
                               int32_t* list_out /* n */, int32_t* count_out /* 1 */);

/* ---- export and import of running tenants: checkpoint, migration, compaction ------------------
 * piadmm_obca_clock_admit starts a fresh tenant.  A RUNNING tenant leaves a plan, or enters one,
 * as a record that holds every per-scenario array of the plan; a scenario's answers do not depend
 * on its place in a batch, so a tenant exported at a step boundary and imported into any slot of any
 * plan continues bit for bit.  A blob is a header followed by m records, little endian as the
 * device writes them.
 *
 * Header, PIADMM_OBCA_TENANT_HEADER = 64 bytes, sixteen int32:
 *   0 magic PIADMM_OBCA_TENANT_MAGIC | 1 PIADMM_ABI_VERSION | 2 m | 3 n_ref | 4 update_lamb_ij |
 *   5 law present (0 / 1) | 6 order present (0 / 1) | 7 F, the fp64 words of a record |
 *   8 PIADMM_OBCA_TENANT_INTS, its int32 words | 9 the bytes of a record, 8 F + 48 |
 *   10 the bytes of the header | 11 the loop's flags (0 without the loop; piadmm_obca_loop_plan:
 *   1 present, + 2 noise rows, + 4 delay rows) | 12, 13 its seed (low, high) | 14 its k0 | 15 zero
 * Record k starts at byte 64 + k (8 F + 48).  Its fp64 section, offsets in doubles (R = 10 n_ref):
 *   0 STATE 556 | 556 STATE_PREV 556 | 1112 CTRL 28 | 1140 CTRL_PREV 28 | 1168 X 80 |
 *   1248 LAMBDA 126 | 1374 PRIMAL | 1375 DUAL | 1376 primal_thres | 1377 dual_thres |
 *   1378 the parameter row 16 | 1394 the tenant's reference 2 x n_ref x 5 |
 *   1394 + R WINDOW 80 (with a clock the window the plan holds; without one the 8 rows at t_step,
 *   zeros when t_step + 8 > n_ref)
 * and, only with a law, from L = 1474 + R:
 *   L S 126 | L + 126 D 126 | L + 252 S_prev 126 | L + 378 D_prev 126 | L + 504 the gains row 8
 * and, only with the loop, PIADMM_OBCA_TENANT_F64_LOOP = 50 words behind the law's section (or the
 * window), from Q:
 *   Q the plant row 16 | Q + 16 the noise row 22 (zeros if absent) | Q + 38 the delay row 8 (zeros if
 *   absent) | Q + 46 the open step's latencies 2 (zeros without delay rows) | Q + 48 the stream id
 *   (the int64's bits) | Q + 49 zero
 * so F = 1474 + R without a law and 1986 + R with one, 50 more with the loop.  Every segment but the four scalars starts
 * on an even word and has an even length, and a record is a multiple of 16 bytes.  Its int32
 * section, at byte 8 F of the record:
 *   0 ITERS | 1 STOP | 2 CONVERGE | 3 prob | 4-5 STATUS_MASK | 6-7 WORK (zeros without the order) |
 *   8-10 CLOCK (c, len, alive; (t_step, n_ref, 1) without a clock) | 11 zero
 * piadmm.obca.tenant_pack / tenant_unpack are the same statement in NumPy.
 *
 * piadmm_obca_tenant_export_bytes returns the size of a blob of m tenants of the open plan.
 * piadmm_obca_tenant_export writes the tenants in `slots` (m distinct scenarios below n, any order;
 * record k is scenario slots[k]) of any open plan -- shared or fleet, with or without clock, law,
 * order or trace; a shared plan writes its one row, its one reference and its one gains row into
 * every record; a retired tenant exports like any other.  `bytes` must be exact (PIADMM_E_ARG); only
 * at a step boundary (PIADMM_E_STATE).  The plan is not changed.  The m slot numbers go to the device,
 * one launch of k_plan_export (one wave per tenant) fills a staging buffer there, and one copy
 * brings the records to the host.
 *
 * piadmm_obca_tenant_import puts the m tenants of a blob into `slots` of the open plan; nothing is
 * zeroed, the slot holds what the tenant had.  Checked before any device call, PIADMM_E_ARG: the
 * slots; the header (magic, ABI, m, the section sizes against its own n_ref and flags, `bytes`);
 * n_ref and update_lamb_ij equal to the plan's; then per record, "obca_tenant_import: row k: ...":
 * the parameter row as piadmm_obca_fleet_begin checks it, prob 0 or 1, the clock c >= 0 and
 * 8 <= len <= n_ref.  Then, PIADMM_E_STATE: a clock is attached, no trace is, the plan is at a step
 * boundary, it has n references and n parameter rows (piadmm_obca_fleet_begin), and the law and the
 * order are attached exactly when the blob carries them.  A plan with one shared gains row takes
 * only tenants whose gains row equals it bit for bit (PIADMM_E_ARG; the row is read back for this);
 * with n gains rows the row travels.  A refused call leaves every piadmm_obca_plan_get item as it
 * was.  One copy of the records to the device (and the m slot numbers) and one launch of
 * k_plan_import; alive is recomputed
 * as c + 8 <= len, so a retired tenant stays retired and frozen; then, as an admission does, the
 * largest max_admm_iter is taken over the current rows and the windows of the alive, the alive flags
 * and the active list are rebuilt (re-sorted, with the order attached).
 *
 * piadmm_obca_plan_get gains, for the arrays a record holds and no item showed,
 *   PRIMAL_THRES, DUAL_THRES   n fp64    the stop thresholds as uploaded
 *   PROB                       n int32
 *   DUAL_S_PREV, DUAL_D_PREV   n x 2 x 7 x 9 fp64   the previous iterate's integrator (PIADMM_E_STATE without a law) */
#define PIADMM_OBCA_TENANT_MAGIC 0x314E5454 /* "TTN1" */
#define PIADMM_OBCA_TENANT_HEADER 64
#define PIADMM_OBCA_TENANT_INTS 12
#define PIADMM_OBCA_TENANT_F64 1474       /* + 10 n_ref, + PIADMM_OBCA_TENANT_F64_LAW with a law */
#define PIADMM_OBCA_TENANT_F64_LAW 512
#define PIADMM_OBCA_TENANT_F64_LOOP 50    /* + this with the loop (piadmm_obca_loop_plan) */
#define PIADMM_OBCA_PLAN_GET_PRIMAL_THRES 29
#define PIADMM_OBCA_PLAN_GET_DUAL_THRES 30
#define PIADMM_OBCA_PLAN_GET_PROB 31
#define PIADMM_OBCA_PLAN_GET_DUAL_S_PREV 32
#define PIADMM_OBCA_PLAN_GET_DUAL_D_PREV 33
int32_t piadmm_obca_tenant_export_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes);
int32_t piadmm_obca_tenant_export(piadmm_obca_t h, int32_t m, const int32_t* slots /* m */, void* blob, int64_t bytes);
int32_t piadmm_obca_tenant_import(piadmm_obca_t h, int32_t m, const int32_t* slots /* m */, const void* blob,
                                int64_t bytes);

/* ---- closed-loop feedback for an open plan: plant, disturbance, measurement -------------------
 * piadmm_obca_plan_shift closes an MPC step with init_state = X[1]: the next step starts from the
 * planner's own Euler prediction (decentralized_overtaking_ADMM.py:99).  The calls below put a
 * vehicle between two steps instead: a plant model that need not be the NLP's, an additive
 * disturbance, or a state measured outside.  Opt-in: without the attachment the plan issues exactly
 * the launches it issued before.
 *
 * The plant step.  State (x, y, v, theta, delta), held control (a, omega), one step of length
 * DT = 0.1 of the reference's right-hand side (decentralized/optimizer.py:75-77)
 *   beta = atan(lr tan(delta) / (lr + lf))
 *   rhs  = (v cos(theta + beta), v sin(theta + beta), a_eff, v / lr sin(beta), w_eff)
 * with a_eff = clip(gain_a a, +-a_max) and w_eff = clip(gain_w omega, +-w_max), in n_sub substeps of
 * DT / n_sub, explicit Euler (method 0) or classical RK4 (method 1); after every substep delta is
 * clipped to +-0.6 (max_front_wheel_angle), after the last one the disturbance row is added:
 * x_next = F(x0, u) + w.  A parameter row is PIADMM_OBCA_FEEDBACK_PAR = 16 doubles, 8 per vehicle,
 * vehicle 0 first, the integers stored as doubles:
 *   method (0 / 1), n_sub (1..64), lr, lf (> 0), gain_a, gain_w (finite), a_max, w_max (> 0)
 * The nominal row (Euler, 1, 1.0, 1.5, 1, 1, 5, 20) with w = 0 is the NLP's own transition
 * st + dt f(st, con) (optimizer.py:92-96).  piadmm.obca.propagate is the same statement in NumPy.
 *
 * piadmm_obca_propagate runs k_plan_propagate (one lane per vehicle) alone on the call's own device
 * buffers; the handle's buffers and an open plan stay as they are.  Before any device call:
 * 1 <= n <= 2^20, non-null pointers (w may be NULL: no disturbance), every input finite, every row
 * valid -- a bad row is PIADMM_E_ARG with "obca_propagate: row k: ...".
 *
 * piadmm_obca_feedback_plan, mode 1, attaches the plant to the open plan: par holds `rows` = 1 (every
 * scenario) or n parameter rows, NULL is the nominal row; tape holds `cap` disturbance rows per
 * scenario (n x cap x 2 x 5, 0 <= cap <= 2^20), NULL is no disturbance.  A second call replaces the
 * first; mode 0 detaches.  Rows and tape (every value finite) are checked on the host before any
 * device call: PIADMM_E_ARG, a bad row with "obca_feedback_plan: row k: ...".  Then, PIADMM_E_STATE:
 * only at a step boundary (no iterate of the open step has run), and not while a clock is attached.
 * A refused call leaves the plan and an earlier attachment as they were.
 *
 * While attached, piadmm_obca_plan_shift (called directly, by piadmm_obca_plan_step or by
 * piadmm_obca_trace_run) computes for every scenario
 *   next = propagate(x0, u0, par[s], tape[s][k])
 * with x0 the closing step's init_state bit for bit (not X[0], which equals it only to the solver's
 * tolerance), u0 = (U[0, 0], U[0, 1]) of the local solution whose X[1] the shift would take (the
 * CTRL item holds it) and k the steps consumed since the attachment; then it runs the unchanged
 * shift and writes `next` over init_state of STATE and STATE_PREV.  Everything else the shift
 * produces -- the shifted duals and halfspaces, LAMBDA, CTRL_PREV = 0, the order's list, the dual
 * law's integrators -- is unchanged bit for bit.  It runs before the trace's row is appended: the
 * row's STATES and clearances are those of the state the vehicle reached.  With a tape, at k >= cap
 * the shift, piadmm_obca_plan_step and piadmm_obca_trace_run (whose n_steps must fit what is left)
 * return PIADMM_E_STATE ("disturbance tape exhausted") before any launch and the plan stays as it
 * was, as "trace full" does.  piadmm_obca_plan_get gains
 *   FEEDBACK_PAR        rows x PIADMM_OBCA_FEEDBACK_PAR fp64   the rows as attached (1 nominal row for NULL)
 *   FEEDBACK_STEPS      1 int32                                the steps consumed since the attachment
 * (PIADMM_E_STATE without the attachment).  piadmm_obca_plan_end, a new piadmm_obca_plan_begin /
 * _fleet_begin and any upload that ends the plan free the attachment.
 *
 * piadmm_obca_feedback_measure writes m measured states over init_state of both state copies of the
 * scenarios `slots` (ascending, distinct, below n) of any open plan, attached or not, in one scatter
 * launch; nothing else changes.  PIADMM_E_ARG before any device call for bad slots or a state that is
 * not finite; PIADMM_E_STATE while an MPC step is open, and while a trace is attached (its last row
 * and running minima were computed from the state being replaced).
 *
 * Out of scope, PIADMM_E_STATE before any device call: piadmm_obca_feedback_plan(mode 1) while a
 * clock is attached, piadmm_obca_clock_plan(mode 1) while feedback is attached, and
 * piadmm_obca_tenant_export / _import while feedback is attached (the tenant record's layout is
 * fixed and has no room for the tape). */
#define PIADMM_OBCA_FEEDBACK_PAR 16
#define PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR 34
#define PIADMM_OBCA_PLAN_GET_FEEDBACK_STEPS 35
int32_t piadmm_obca_propagate(piadmm_obca_t h, int32_t n, const double* states /* n x 2 x 5 */,
                              const double* ctrl /* n x 2 x 2: a, omega */,
                              const double* par /* n x PIADMM_OBCA_FEEDBACK_PAR */,
                              const double* w /* n x 2 x 5 or NULL */, double* out /* n x 2 x 5 */);
int32_t piadmm_obca_feedback_plan(piadmm_obca_t h, int32_t mode,
                                  const double* par /* rows x PIADMM_OBCA_FEEDBACK_PAR, may be NULL */,
                                  int32_t rows /* 1 or n */, const double* tape /* n x cap x 2 x 5, may be NULL */,
                                  int32_t cap);
int32_t piadmm_obca_feedback_measure(piadmm_obca_t h, int32_t m, const int32_t* slots /* m, ascending */,
                                     const double* states /* m x 2 x 5 */);

/* ---- device-side disturbance noise for the closed-loop plan -------------------------------------
 * The tape of piadmm_obca_feedback_plan is the caller's: n x cap x 80 bytes generated, checked and
 * uploaded, and a scenario's disturbance is a function of nothing the library knows.  The calls below
 * draw it on the device from a counter-based generator: the disturbance row of a scenario at a step
 * is a pure function of (seed, stream id, step index), the same in NumPy (piadmm.obca.noise_tape)
 * and on the device, so a scenario can be re-run alone -- in another plan, handle or process -- from
 * three integers.  Opt-in: without the attachment the plan issues exactly the launches it issued
 * before.
 *
 * The statement.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as
 * 1, 2, 3", SC'11): multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85,
 * ten rounds.  For vehicle v (0 / 1) of stream t (int64, 0 <= t < 2^63), step index k
 * (0 <= k < 2^31) and call j (0, 1, 2):
 *   counter = (k, 4 v + j, t & 0xffffffff, t >> 32),  key = (seed & 0xffffffff, seed >> 32)
 *   (r0, r1, r2, r3) = philox4x32_10(counter, key)
 *   u1 = (((r0 << 32 | r1) >> 12) + 0.5) 2^-52,  u2 = (((r2 << 32 | r3) >> 12) + 0.5) 2^-52    in (0, 1), exact
 *   rad = sqrt(-2 log(u1)),  z[2 j] = rad cos(2 pi u2),  z[2 j + 1] = rad sin(2 pi u2)
 * z[0 .. 4] are the vehicle's normals for (x, y, v, theta, delta), z[5] is discarded.  A noise row is
 * PIADMM_OBCA_NOISE_PAR = 22 doubles:
 *   sigma[2][5] (finite, >= 0), bias[2][5] (finite), trunc (0: none, else > 0: z is clipped to
 *   +-trunc before it is scaled), one reserved zero
 * and the disturbance is w[v][i] = bias[v][i] + sigma[v][i] z[i], product and sum kept apart (no
 * contraction): sigma = 0 gives the bias bit for bit.  The integer part is exact everywhere; log, sqrt,
 * cos and sin are the device's, so a device row equals the NumPy one to a few ulp, not bit for bit,
 * and two device rows of the same (seed, t, k) are equal bit for bit.
 *
 * piadmm_obca_noise_tape runs k_plan_noise (one lane per vehicle, one grid row per step index) alone
 * on the call's own device buffers; the handle's buffers and an open plan stay as they are.  It
 * fills tape_out[s][i] (n x cap x 2 x 5) with the row of stream streams[s] (NULL: s) at step index
 * k0 + i under par (`rows` = 1 row for every scenario, or n), and raw_out (n x cap x 2 x 3 x 4, may
 * be NULL) with the generator's words.  Before any device call, PIADMM_E_ARG: 1 <= n <= 2^20,
 * 0 <= cap <= 2^20, n x cap x 80 bytes below 2 GiB, rows 1 or n, every row valid ("obca_noise_tape:
 * row k: ..."), streams >= 0, k0 >= 0 and k0 + cap <= 2^31.
 *
 * piadmm_obca_noise_plan, mode 1, attaches the generator to an open plan that has feedback attached:
 * from then on piadmm_obca_plan_shift launches k_plan_noise in front of the unchanged
 * k_plan_propagate, which reads the step's rows in the tape's place:
 *   next = propagate(x0, u0, par[s], tape[s][k] + noise(seed, streams[s], k0 + k))
 * with k the feedback's FEEDBACK_STEPS; the tape term comes first and is absent without a tape.  One
 * more launch per MPC step and nothing else.  A second call replaces the first; mode 0 detaches (the
 * other arguments are then ignored).  The same host checks as above (PIADMM_E_ARG, "obca_noise_plan:
 * row k: ..."), then PIADMM_E_STATE: no open plan, no feedback attached, an MPC step open.  A refused
 * call leaves the plan and an earlier noise attachment as they were.  The noise counts its steps by
 * the feedback's: piadmm_obca_feedback_plan mode 0 detaches the noise too, and so does mode 1 (a new
 * feedback attachment restarts FEEDBACK_STEPS) -- attach the noise again after it.  Without a tape
 * nothing is ever "exhausted" (only the step index: k0 + k stays below 2^31, else PIADMM_E_STATE
 * "noise step index exhausted"); with a tape its cap applies unchanged.
 * piadmm_obca_plan_get gains the items
 *   PIADMM_OBCA_NOISE_GET_PAR       rows x PIADMM_OBCA_NOISE_PAR fp64   the rows as attached
 *   PIADMM_OBCA_NOISE_GET_STREAMS   n int64                             the stream ids (0 .. n-1 for NULL)
 *   PIADMM_OBCA_NOISE_GET_SEED      2 uint64                            seed, k0
 * (PIADMM_E_STATE without the attachment).  Out of scope: noise with a clock or the tenant calls
 * (feedback refuses both), noise in piadmm_obca_feedback_measure, time-correlated noise. */
#define PIADMM_OBCA_NOISE_PAR 22
#define PIADMM_OBCA_NOISE_GET_PAR 36
#define PIADMM_OBCA_NOISE_GET_STREAMS 37
#define PIADMM_OBCA_NOISE_GET_SEED 38
int32_t piadmm_obca_noise_tape(piadmm_obca_t h, int32_t n, int32_t cap,
                               const double* par /* rows x PIADMM_OBCA_NOISE_PAR */, int32_t rows /* 1 or n */,
                               const int64_t* streams /* n, may be NULL: 0 .. n-1 */, uint64_t seed, int32_t k0,
                               double* tape_out /* n x cap x 2 x 5 */,
                               uint32_t* raw_out /* n x cap x 2 x 3 x 4, may be NULL */);
int32_t piadmm_obca_noise_plan(piadmm_obca_t h, int32_t mode, const double* par /* rows x PIADMM_OBCA_NOISE_PAR */,
                               int32_t rows /* 1 or n */, const int64_t* streams /* n, may be NULL: 0 .. n-1 */,
                               uint64_t seed, int32_t k0);

/* ---- communication delay in the plan's exchange: stale exchanged plans --------------------------
 * The delay tightening of the halfspaces (prob = 1: the box moved forward by AVG_DELAY v (cos, sin)
 * plus a variance term) exists to cover communication delay, yet the plan's exchange is never stale:
 * every vehicle sends the halfspaces of its current local solution.  The calls below attach a
 * communication-delay model to the exchange of an open plan.  Opt-in: without the attachment the
 * plan issues exactly the launches it issued before and gives the same bits.
 *
 * The latency.  One value per vehicle and MPC step, held over all ADMM iterates of that step.  A
 * delay row is PIADMM_OBCA_DELAY_PAR = 8 doubles:
 *   avg[2] (finite, >= 0), std[2] (finite, >= 0), tau_max[2] (0 <= tau_max <= DT = 0.1),
 *   trunc (0: none, else > 0: z is clipped to +-trunc first), one reserved zero
 * For vehicle v of stream t (int64, 0 <= t < 2^63) at step index k (0 <= k < 2^31) under `seed`:
 *   counter = (k, 4 v + 3, t & 0xffffffff, t >> 32),  key = (seed & 0xffffffff, seed >> 32)
 * -- the call the noise leaves free (its calls are 4 v + 0, 1, 2), so noise and delay under one seed
 * and the same streams draw independently -- u1, u2 from the four words as the noise forms them,
 *   z = sqrt(-2 log(u1)) cos(2 pi u2)                      (the second normal is discarded)
 *   x = tape + (avg[v] + std[v] z)                         tape: the latency tape's entry, or 0
 *   tau = min(tau_max[v], max(0, x))                       (x > 0 ? x : 0, then < tau_max ? . : tau_max)
 * products and sums kept apart; std = 0 without a tape gives min(tau_max, avg) bit for bit.  The
 * words are exact; log, sqrt and cos are the device's, so a device tau equals the NumPy one
 * (piadmm.obca.delay_tau) to a few ulp and two device values of the same (seed, t, k) bit for bit.
 *
 * The stale message.  With the local solve's states X[0 .. 7] (X[0] is init_state), slot t = 0 .. 6:
 *   st' = X[t+1]                                      if tau == 0  (the plain exchange, bit for bit)
 *   st' = X[t+1] + (tau / DT) (X[t] - X[t+1])         otherwise: all five entries, theta linearly
 * and everything the vehicle sends is computed from st' in place of X[t+1]: local_x of the state and
 * of the edge record, A and b through the unchanged halfspaces, and with them check_converge.  What
 * the vehicle keeps for itself (CTRL, X, later init_state) is unchanged: the vehicles move truly,
 * the other vehicle and the coordinator see stale plans, and a trace's clearances stay the truth.
 *
 * piadmm_obca_delay_tau runs k_plan_delay (one lane per vehicle, one grid row per step index) alone
 * on the call's own device buffers: tau_out[s][i][v] (n x cap x 2) is the latency of stream
 * streams[s] (NULL: s) at step index k0 + i under par (`rows` = 1 or n), tape (n x cap x 2, may be
 * NULL) added as above, raw_out (n x cap x 2 x 4, may be NULL) the call's words.  Before any device
 * call, PIADMM_E_ARG: 1 <= n <= 2^20, 0 <= cap <= 2^20, n x cap x 16 bytes below 2 GiB, rows 1 or n,
 * every row valid ("obca_delay_tau: row k: ..."), streams >= 0, k0 >= 0 and k0 + cap <= 2^31, the
 * tape finite.
 *
 * piadmm_obca_delay_exchange computes the stale message alone from given latencies (tau n x 2, each
 * in [0, DT]), one wave per scenario, by the device function the plan's kernel runs: lx_out = st',
 * (A_out, b_out) = halfspaces(st', prob[s]).  PIADMM_E_ARG before any device call: 1 <= n <= 2^20,
 * non-null pointers, prob 0 or 1, X finite, tau in [0, DT].
 *
 * piadmm_obca_delay_plan, mode 1, attaches the model to an open plan: tau of step index k0 is drawn
 * at once, from then on every iterate launches the stale exchange in the plain one's place, and
 * piadmm_obca_plan_shift draws the next step's tau after the shift (one launch more per MPC step).
 * The delay counts its own steps since the attachment; it works with or without feedback and noise.
 * tape (n x cap x 2, may be NULL; cap is ignored without one) adds recorded latencies: step k since
 * the attachment reads tape[s][k][v], and once cap steps are closed piadmm_obca_plan_iterate,
 * _plan_step, _plan_shift and piadmm_obca_trace_run (whose n_steps must fit what is left) return
 * PIADMM_E_STATE ("latency tape exhausted") before any launch, as "trace full" does; a step index
 * reaching 2^31 is refused the same way ("delay step index exhausted").  A second call replaces the
 * first once the new attachment is complete; mode 0 detaches (the other arguments are ignored).  The
 * host checks above (PIADMM_E_ARG, "obca_delay_plan: row k: ..."), then PIADMM_E_STATE: no open
 * plan, a clock attached, an MPC step open.  A refused call leaves everything as it was.  While the
 * delay is attached piadmm_obca_clock_plan (mode 1) and piadmm_obca_tenant_export / _import return
 * PIADMM_E_STATE (the record has no room for it).  piadmm_obca_plan_get gains the items
 *   PIADMM_OBCA_DELAY_GET_PAR       rows x PIADMM_OBCA_DELAY_PAR fp64   the rows as attached
 *   PIADMM_OBCA_DELAY_GET_TAU       n x 2 fp64                          the open step's latencies
 *   PIADMM_OBCA_DELAY_GET_STREAMS   n int64                             the stream ids (0 .. n-1 for NULL)
 *   PIADMM_OBCA_DELAY_GET_SEED      3 uint64                            seed, k0, the steps closed since
 * (PIADMM_E_STATE without the attachment).  Out of scope: a latency per iterate or per direction,
 * delays beyond one step, staleness of the coordinator's answer, angle wrapping in the interpolation. */
#define PIADMM_OBCA_DELAY_PAR 8
#define PIADMM_OBCA_DELAY_GET_PAR 39
#define PIADMM_OBCA_DELAY_GET_TAU 40
#define PIADMM_OBCA_DELAY_GET_STREAMS 41
#define PIADMM_OBCA_DELAY_GET_SEED 42
int32_t piadmm_obca_delay_tau(piadmm_obca_t h, int32_t n, int32_t cap,
                              const double* par /* rows x PIADMM_OBCA_DELAY_PAR */, int32_t rows /* 1 or n */,
                              const int64_t* streams /* n, may be NULL: 0 .. n-1 */, uint64_t seed, int32_t k0,
                              const double* tape /* n x cap x 2, may be NULL */, double* tau_out /* n x cap x 2 */,
                              uint32_t* raw_out /* n x cap x 2 x 4, may be NULL */);
int32_t piadmm_obca_delay_exchange(piadmm_obca_t h, int32_t n, const double* X /* n x 2 x 8 x 5 */,
                                   const int32_t* prob /* n */, const double* tau /* n x 2 */,
                                   double* lx_out /* n x 2 x 7 x 5 */, double* A_out /* n x 2 x 7 x 4 x 2 */,
                                   double* b_out /* n x 2 x 7 x 4 */);
int32_t piadmm_obca_delay_plan(piadmm_obca_t h, int32_t mode, const double* par /* rows x PIADMM_OBCA_DELAY_PAR */,
                               int32_t rows /* 1 or n */, const int64_t* streams /* n, may be NULL: 0 .. n-1 */,
                               uint64_t seed, int32_t k0, const double* tape /* n x cap x 2, may be NULL */,
                               int32_t cap);

/* ---- the loop: closed loop under per-scenario clocks (plant, noise, delay, tenants) -------------
 * piadmm_obca_feedback_plan, _noise_plan and _delay_plan count the plan's steps and therefore refuse a
 * clocked plan, and the tenant calls refuse them.  The loop is the same closed loop for a clocked
 * plan: its step index is each tenant's own clock.  With c the tenant's clock as
 * PIADMM_OBCA_PLAN_GET_CLOCK shows it, the disturbance row and the latency of scenario s are the pure
 * functions of (seed, streams[s], k0 + c) the noise and the delay sections define (one seed, one
 * stream id and one k0 serve both draws: the noise's counter calls are 4 v + 0, 1, 2, the delay's is
 * 4 v + 3), so a tenant re-run alone, admitted late, retired, exported or imported computes the same
 * bits.  Opt-in: without the attachment the plan issues exactly the launches it issued before.
 *
 * piadmm_obca_loop_plan, mode 1, attaches it; a second call replaces the first once the new
 * attachment is complete; mode 0 detaches (the other arguments are ignored).  plant: plant rows
 * (NULL: the nominal row), noise: noise rows (NULL: no noise), delay: delay rows (NULL: no delay, the
 * plain exchange runs), each `rows` = 1 (shared) or n and each row checked as its own attachment
 * checks it (PIADMM_E_ARG, "obca_loop_plan: <kind> row k: ..."); streams >= 0 (NULL: 0 .. n-1),
 * k0 >= 0.  Then PIADMM_E_STATE: no open plan, feedback or the delay attached, no clock attached, an
 * MPC step open, a step index k0 + c of an alive tenant at 2^31.  A refused call leaves every
 * piadmm_obca_plan_get item and an earlier loop as they were.  While attached:
 *   closing a step   piadmm_obca_plan_shift computes, for exactly the scenarios the step ran and before
 *                    the shift overwrites what it reads, next = propagate(init_state, u0, plant[s]) +
 *                    (the noise row at k0 + c, if any) with x0, u0 and the order of operations of
 *                    piadmm_obca_feedback_plan (k_loop_close); after the unchanged shift next goes
 *                    over init_state of both state copies (k_plan_set_init), before the tick and
 *                    before a trace row is appended
 *   opening a step   with delay rows the open step's latency of an alive tenant is tau(seed,
 *                    streams[s], k0 + c) at its clock after the tick: drawn at the attachment, after
 *                    every shift and after every admission or import (k_loop_open over the alive
 *                    scenarios); every iterate launches k_plan_exchange_stale on them
 *   retired tenants  frozen as the clock section says; their latency and stream id stay as well
 *   the limit        a shift, step or piadmm_obca_trace_run that would take an alive tenant's k0 + c to
 *                    2^31 is PIADMM_E_STATE ("loop step index exhausted") before any launch
 * piadmm_obca_clock_plan (either mode) returns PIADMM_E_STATE ("obca_clock_plan: the loop is
 * attached"): detach the loop first.  piadmm_obca_feedback_measure, the trace, the order and the dual
 * law work as before.  piadmm_obca_clock_admit keeps the slot's loop rows and stream id and redraws
 * its latency at the new c0.
 *
 * piadmm_obca_loop_admit sets the loop rows and stream ids of the m slots (distinct, below n): a
 * non-NULL row array holds m rows of that kind and needs a loop with n rows of it (PIADMM_E_STATE
 * otherwise); NULL keeps what the slot has.  Only at a step boundary, without a trace; the latencies
 * of the alive scenarios are drawn again.
 *
 * piadmm_obca_loop_draw runs the per-tenant draw alone on the call's own device buffers (k_loop_draw):
 * w_out[s] and tau_out[s] are the disturbance row and the latency of stream streams[s] at step index
 * k0 + clock[s][0] (clock n x 3 as the CLOCK item; only c is read); NULL noise gives zeros in w_out,
 * NULL delay zeros in tau_out.  PIADMM_E_ARG before any device call: 1 <= n <= 2^20, the rows, the
 * streams, k0 >= 0, c >= 0 and k0 + c < 2^31.
 *
 * The tenant record carries the loop (the layout above): piadmm_obca_tenant_export of a plan with the
 * loop writes the section, a shared row into every record.  piadmm_obca_tenant_import checks, before
 * any device call: the header's flags, seed and k0 against the plan's loop (PIADMM_E_ARG; the loop
 * present in one and absent in the other is PIADMM_E_STATE, as the law), per record ("obca_tenant_import:
 * row k: ...") the three rows, tau in [0, DT], the stream id >= 0, and a row that differs from the
 * plan's shared row of its kind.  Rows, tau and stream id travel; an alive tenant's latency is then
 * drawn again at its clock (the value a consistent record holds), a retired tenant keeps the
 * record's: the tenant continues bit for bit.
 *
 * piadmm_obca_plan_get gains (PIADMM_E_STATE without the loop; NOISE / DELAY also without that kind)
 *   PIADMM_OBCA_LOOP_GET_PLANT     rows x PIADMM_OBCA_FEEDBACK_PAR fp64
 *   PIADMM_OBCA_LOOP_GET_NOISE     rows x PIADMM_OBCA_NOISE_PAR fp64
 *   PIADMM_OBCA_LOOP_GET_DELAY     rows x PIADMM_OBCA_DELAY_PAR fp64
 *   PIADMM_OBCA_LOOP_GET_TAU       n x 2 fp64    the open step's latencies (zeros without delay rows)
 *   PIADMM_OBCA_LOOP_GET_STREAMS   n int64
 *   PIADMM_OBCA_LOOP_GET_SEED      3 uint64      seed, k0, flags
 * Out of scope: tapes (a tape has no per-tenant clock), AR(1) noise, delays beyond one step, admission
 * under a trace. */
#define PIADMM_OBCA_LOOP_GET_PLANT 43
#define PIADMM_OBCA_LOOP_GET_NOISE 44
#define PIADMM_OBCA_LOOP_GET_DELAY 45
#define PIADMM_OBCA_LOOP_GET_TAU 46
#define PIADMM_OBCA_LOOP_GET_STREAMS 47
#define PIADMM_OBCA_LOOP_GET_SEED 48
int32_t piadmm_obca_loop_plan(piadmm_obca_t h, int32_t mode,
                              const double* plant /* rows x PIADMM_OBCA_FEEDBACK_PAR, may be NULL */, int32_t plant_rows,
                              const double* noise /* rows x PIADMM_OBCA_NOISE_PAR, may be NULL */, int32_t noise_rows,
                              const double* delay /* rows x PIADMM_OBCA_DELAY_PAR, may be NULL */, int32_t delay_rows,
                              const int64_t* streams /* n, may be NULL: 0 .. n-1 */, uint64_t seed, int32_t k0);
int32_t piadmm_obca_loop_admit(piadmm_obca_t h, int32_t m, const int32_t* slots /* m */,
                               const double* plant, const double* noise, const double* delay /* m rows each, may be NULL */,
                               const int64_t* streams /* m, may be NULL */);
int32_t piadmm_obca_loop_draw(piadmm_obca_t h, int32_t n, const int32_t* clock /* n x 3 */,
                              const double* noise, int32_t noise_rows, const double* delay, int32_t delay_rows,
                              const int64_t* streams /* n, may be NULL */, uint64_t seed, int32_t k0,
                              double* w_out /* n x 2 x 5 */, double* tau_out /* n x 2 */);

/* ---- fleet risk statistics and the worst-case gather of a run record ---------------------------
 * A Monte-Carlo study over a traced fleet asks how many runs came closer than d, at which step the
 * fleet is most at risk, and which runs were the worst.  piadmm_obca_trace_get can only copy the
 * whole record, O(R n) bytes; the calls below reduce it on the device and bring back the counts, the
 * minima and the record of a chosen few scenarios, O(R B + R m) bytes.
 *
 * The ordering key.  Values are ordered by (value ascending, then scenario ascending); a value that
 * is not finite (NaN, +inf, -inf) orders after every finite one, again by scenario: a strict total
 * order, as the one of piadmm_obca_order.  Equal values are compared with ==, so -0.0 ties with 0.0.
 *
 * With ascending edges e_0 < ... < e_(B-1), R recorded steps and n scenarios, over a summary (n x 4:
 * min plain clearance, its row, min tightened clearance, sum of the stop iterates -- the SUMMARY item),
 * the clearances ((R + 1) x n x 2), the stop iterates (R x n) and the status masks (R x n x 2):
 *   piadmm_obca_stats_t  nonfinite[k]   the scenarios whose minimum k (0 plain, 1 tightened) is not finite
 *                        iter_sum       the sum of the summary's iterate sums, each converted to an integer
 *                        flagged        the scenarios whose OR over the rows, of either mask, has a bit other
 *                                       than 1 << PIADMM_OBCA_CONVERGED
 *                        fleet_min[k], fleet_arg[k]   the first finite minimum k under the key and its
 *                                       scenario; +inf and -1 when none is finite
 *                        iter_max       the largest stop iterate (0 for R = 0)
 *                        mask_or[j]     the OR of the local (0) / the edge (1) mask over rows and scenarios
 *   hist       2 x (B + 1) int64        of the plain / the tightened minima: bin 0 counts x < e_0, bin b
 *                                       e_(b-1) <= x < e_b, bin B x >= e_(B-1); a minimum that is not finite
 *                                       is in no bin
 *   row_min    (R + 1) x 2 fp64         per row the first finite clearance under the key ...
 *   row_arg    (R + 1) x 2 int32        ... and its scenario; +inf and -1 when the row has none
 *   row_below  (R + 1) x 2 x B int32    the scenarios of the row with a finite clearance < e_b (cumulative in b)
 *   worst      K int32                  the K scenarios that come first under the key on the plain minimum,
 *                                       in that order (the ones that are not finite last)
 * Every result is an integer count, a minimum of doubles or a comparison: exact, a function of the
 * inputs alone, the same on every run.  k_stats_fleet, k_stats_rows and k_stats_worst reduce 128
 * scenarios per workgroup with wave reductions and LDS partials and write one partial record each; a
 * second, small launch (several for `worst` on a large fleet) reduces the records.  No atomic decides
 * a value or a position and no kernel waits for another workgroup.  piadmm.obca.fleet_stats_host is
 * the same statement in NumPy.
 *
 * piadmm_obca_fleet_stats runs the reductions on the caller's arrays, on the call's own device
 * buffers: the handle's buffers and an open plan stay as they are.  rows_R may be 0; iters and mask
 * may then be NULL.  piadmm_obca_stats_trace runs them on the attached trace in place (R = the steps
 * recorded, PIADMM_OBCA_TRACE_GET_ROWS): nothing but the results is copied, the plan and the trace
 * are not changed, and it works with a dual law, an order, a clock or feedback attached.  Under a
 * clock a retired scenario's rows hold its frozen values and are counted as they stand.
 * Before any device call, PIADMM_E_ARG: non-null pointers, 1 <= n <= 2^20, 0 <= rows_R <= 2^20,
 * 1 <= B <= PIADMM_OBCA_STATS_EDGES, every edge finite and above the one before it ("obca_fleet_stats:
 * edge k: ..."), 1 <= K <= min(PIADMM_OBCA_STATS_WORST, n) and, for piadmm_obca_fleet_stats, every
 * iterate sum of the summary an integer in [0, 2^40] ("obca_fleet_stats: row k: ...").
 * piadmm_obca_stats_trace without an open plan or an attached trace is PIADMM_E_STATE.  A refused
 * call writes nothing.
 *
 * piadmm_obca_gather_trace copies every row of the m scenarios `slots` (distinct, below n, any order)
 * out of the attached trace: the slot numbers go to the device, one launch of k_trace_gather (one wave
 * per row and column) fills a staging buffer there and one copy brings it to the host.  Column k is
 * scenario slots[k]; every value is an exact copy.  The blob, offsets in bytes with R = the steps
 * recorded and P = R m:
 *   0                       STATES       (R + 1) x m x 2 x 5 fp64
 *   80 (R + 1) m            CLEARANCE    (R + 1) x m x 2 fp64
 *   96 (R + 1) m            PRIMAL       R x m fp64
 *   96 (R + 1) m + 8 P      DUAL         R x m fp64
 *   96 (R + 1) m + 16 P     SUMMARY      m x 4 fp64
 *   I = 96 (R + 1) m + 16 P + 32 m       ITERS        R x m int32
 *   I + 4 P                 STATUS_MASK  R x m x 2 int32
 *   L = I + 12 P + (4 if P is odd)       LAMBDA       R x m x 2 x 7 x 9 fp64, only with PIADMM_OBCA_TRACE_LAMBDA
 * The blob is L bytes without the flag and L + 1008 P with it; piadmm_obca_gather_trace_bytes returns
 * that number, and `bytes` must equal it.  piadmm.obca.trace_gather_unpack is the same statement in
 * NumPy.  PIADMM_E_ARG before any device call: 1 <= m <= n, non-null pointers, the slots, `bytes`;
 * PIADMM_E_STATE without an open plan or an attached trace.  Neither the plan nor the trace changes. */
#define PIADMM_OBCA_STATS_EDGES 64
#define PIADMM_OBCA_STATS_WORST 64
typedef struct {
  int64_t nonfinite[2];
  int64_t iter_sum, flagged;
  double fleet_min[2];
  int32_t fleet_arg[2];
  int32_t iter_max;
  int32_t mask_or[2];
  int32_t reserved;
} piadmm_obca_stats_t;
int32_t piadmm_obca_stats_size(void);
int32_t piadmm_obca_fleet_stats(piadmm_obca_t h, int32_t rows_R, int32_t n, const double* clear /* (R + 1) x n x 2 */,
                                const double* summary /* n x 4 */, const int32_t* iters /* R x n */,
                                const int32_t* mask /* R x n x 2 */, const double* edges /* B */, int32_t B, int32_t K,
                                piadmm_obca_stats_t* stats, int64_t* hist /* 2 x (B + 1) */,
                                double* row_min /* (R + 1) x 2 */, int32_t* row_arg /* (R + 1) x 2 */,
                                int32_t* row_below /* (R + 1) x 2 x B */, int32_t* worst /* K */);
int32_t piadmm_obca_stats_trace(piadmm_obca_t h, const double* edges /* B */, int32_t B, int32_t K,
                                piadmm_obca_stats_t* stats, int64_t* hist, double* row_min, int32_t* row_arg,
                                int32_t* row_below, int32_t* worst);
int32_t piadmm_obca_gather_trace_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes);
int32_t piadmm_obca_gather_trace(piadmm_obca_t h, int32_t m, const int32_t* slots /* m */, void* blob, int64_t bytes);

/* ---- the tenant ledger: risk records that survive retirement and admission ----------------------
 * A trace is indexed by plan step and slot: it costs O(steps x n) device memory, ends at cap_steps and
 * would mix two tenants of one slot, so admission and import refuse it.  The ledger is the record a
 * service keeps instead: one small record per tenant, kept on the device while the tenant runs,
 * appended when the tenant leaves its slot, and reducible by the statistics above.  Opt-in, the fifth
 * attachment of a clocked plan (with or without the loop, the dual law and the order): without it
 * every call issues exactly the launches it issued before and computes the same bits.
 *
 * A record is PIADMM_OBCA_LEDGER_REC = 176 bytes, 22 words of 8 bytes; of two int32 in a word the
 * first is the low half:
 *   word 0        int64   the tenant's id
 *   word 1        int64   the stream id of the loop it ran under (-1 without the loop)
 *   word 2        int32   the slot; int32 the reason: 1 retired by its clock, 2 replaced by an admission,
 *                         3 replaced by an import (0 in an open record)
 *   word 3        int32   c_first, the tenant's clock when its record was opened; int32 steps closed since
 *   word 4        fp64    the minimum plain clearance over the entry state and every state a closed step left
 *   word 5        fp64    the minimum tightened clearance over the same states
 *   word 6        int32   c_min, the tenant's clock at the state where the plain minimum was first reached
 *                         (strict <, as the trace's summary); int32 the largest stop iterate
 *   word 7        int64   the sum of the stop iterates
 *   word 8        int32   the OR of the local status masks; int32 the OR of the edge status masks
 *   words 9, 10   fp64    the primal and the dual residual of the last closed step's stopping iterate
 *                         (0 with steps = 0)
 *   word 11       int32   the plan's T_STEP (PIADMM_OBCA_PLAN_GET_T_STEP) when the call that appended the
 *                         record was made (-1 in an open record); int32 0
 *   words 12-21   fp64    init_state[2][5] after the last closed step (the entry state with steps = 0)
 * The clearances are those of piadmm_obca_clearance at the plan's prob[slot] (clearance_pair,
 * csrc/piadmm_obca_plan.h: the statements k_plan_clearance runs, the same bits).
 *
 * piadmm_obca_ledger_begin attaches a ledger of cap_tenants records; a second call replaces the first.
 * PIADMM_E_ARG before any device call: 1 <= cap_tenants <= 2^20, flags = 0.  PIADMM_E_STATE: no open
 * plan, no clock attached, a trace attached (piadmm_obca_trace_begin refuses a plan with a ledger
 * likewise), an MPC step open.  It opens a record for every alive slot (k_ledger_open): id = the slot
 * number, c_first = the slot's clock, the clearances of its init_state start the minima.  A slot that
 * is not alive holds no tenant: id -1, never appended.  The id counter starts at n.  While attached:
 *   closing a step   piadmm_obca_plan_shift (called directly, by piadmm_obca_plan_step or by a run)
 *                    updates the open record of every scenario the step ran (k_ledger_step, one launch,
 *                    after the shift -- under the loop after `next` has gone over init_state -- and
 *                    before the tick): the new init_state, its two clearances, the stop iterate, both
 *                    masks, the residuals, the stream id.  A scenario this shift retires is appended
 *                    with reason 1; the retirees of one shift are appended ascending by slot at
 *                    positions count, count + 1, ...: a position is the host's count plus the number of
 *                    retirees before the scenario in the list the step ran, counted on the device as
 *                    k_plan_order counts a rank.  No atomic decides a position and nothing is read back.
 *   the limit        the host mirrors count from its mirror of the clocks; a shift, step or run that
 *                    would take count above cap_tenants is PIADMM_E_STATE ("ledger full") before any launch
 *   admission        piadmm_obca_clock_admit and piadmm_obca_tenant_import append, before a slot is
 *                    overwritten, the open record of its alive tenant (k_ledger_close; reason 2 / 3,
 *                    in the order of `slots`, with the stream id it ran under); a retired tenant was
 *                    appended already.  Each new alive tenant then takes the next id, in the order of
 *                    `slots`, and a fresh record opens at its clock and entry state (k_ledger_open); an
 *                    imported tenant that is retired holds no record.  "ledger full" as above, before
 *                    any device call.  piadmm_obca_loop_admit does the same to a tenant that has closed
 *                    a step; one that has not -- the slot was just admitted -- keeps its id and its
 *                    record is opened again under the new stream id.
 * piadmm_obca_clock_plan (either mode) is PIADMM_E_STATE while a ledger is attached: end it first.
 * piadmm_obca_tenant_export and a blob do not change: an imported tenant starts a fresh record.
 *
 * piadmm_obca_ledger_get copies one item; `bytes` must be exact:
 *   PIADMM_OBCA_LEDGER_GET_COUNT     1 int32              the appended records
 *   PIADMM_OBCA_LEDGER_GET_RECORDS   count x 176 bytes    the appended records, in the order of appending
 *   PIADMM_OBCA_LEDGER_GET_RUNNING   n x 176 bytes        the open record of every slot: reason 0; a slot
 *                                                         without a tenant has id -1
 *   PIADMM_OBCA_LEDGER_GET_NEXT_ID   1 int64              the id the next admitted tenant takes
 * piadmm_obca_ledger_clear sets count to 0, so that a service drains the records and goes on; ids
 * keep counting.  piadmm_obca_ledger_end frees the ledger alone; whatever ends the plan frees it too.
 *
 * piadmm_obca_ledger_stats reduces the appended records on the device in place: k_ledger_view builds,
 * in the ledger's own scratch, the view of a run record with R = 1 and n = count -- summary (min
 * plain, c_min, min tight, the iterate sum), clearances (both rows the minima), iterates (the largest
 * stop iterate), masks (the two ORs) -- and the kernels of piadmm_obca_stats_trace run on it.  stats,
 * hist and worst are those of the statistics section with a record's position in the ledger as the
 * scenario.  The checks of edges, B and K are those of piadmm_obca_fleet_stats with n = count;
 * count = 0 is PIADMM_E_STATE.  piadmm.obca.ledger_stats_host is the same statement in NumPy.
 * Out of scope: an open record inside a tenant blob, a record per step (the trace), quantiles, a
 * ledger on a plan without a clock; piadmm_obca_feedback_measure does not enter a record. */
#define PIADMM_OBCA_LEDGER_REC 176
#define PIADMM_OBCA_LEDGER_GET_COUNT 0
#define PIADMM_OBCA_LEDGER_GET_RECORDS 1
#define PIADMM_OBCA_LEDGER_GET_RUNNING 2
#define PIADMM_OBCA_LEDGER_GET_NEXT_ID 3
int32_t piadmm_obca_ledger_begin(piadmm_obca_t h, int32_t cap_tenants, int32_t flags);
int32_t piadmm_obca_ledger_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes);
int32_t piadmm_obca_ledger_clear(piadmm_obca_t h);
int32_t piadmm_obca_ledger_stats(piadmm_obca_t h, const double* edges /* B */, int32_t B, int32_t K,
                                 piadmm_obca_stats_t* stats, int64_t* hist /* 2 x (B + 1) */, int32_t* worst /* K */);
int32_t piadmm_obca_ledger_end(piadmm_obca_t h);

#ifdef __cplusplus
}
#endif

#endif /* PIADMM_H */
