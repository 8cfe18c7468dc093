/*
 * sdeng.h -- C ABI of the MI355X-native SDE sampling engine (libsdeng.so).
 *
 * The reference (vanilladucky/sde_sampler_lrds) has no FFI: its seam for this path is the
 * Python callable protocol of sde_sampler/losses/oc.py (`loss.simulate(ts, x, ...)`,
 * SURVEY.md section 8b).  This header is the binding a maintainer would add below that seam:
 * one call per `simulate()` loop, plain pointers and sizes, no torch types.  Every entry point
 * names the reference code it replaces (paths relative to /root/reference/sde_sampler).
 *
 * Conventions
 *   - all arrays are fp32, row-major, contiguous, in DEVICE memory unless noted;
 *   - the callee borrows every pointer for the duration of the stream-ordered work and never
 *     frees or allocates: outputs and the workspace are caller-allocated;
 *   - every function enqueues on `stream` (a hipStream_t) and returns without synchronising;
 *   - return value 0 = ok, negative = error (see SDENG_E_*); the message for the calling
 *     thread's last error is available from sdeng_last_error(); nothing ever throws;
 *   - re-entrant per stream; the only global state is the thread-local error string.
 */
#ifndef SDENG_H
#define SDENG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDENG_ABI_VERSION 4

/* error codes */
#define SDENG_OK 0
#define SDENG_E_INVALID (-1)     /* malformed descriptor (null pointer, bad size)          */
#define SDENG_E_UNSUPPORTED (-2) /* valid, but no kernel is built for this combination      */
#define SDENG_E_WORKSPACE (-3)   /* workspace too small (see sdeng_workspace_bytes)          */
#define SDENG_E_HIP (-4)         /* a HIP runtime call failed                                */

/* ---- which simulate() loop -------------------------------------------------------------
 * SDENG_FORM_LIN   x' = (c1*x + c2*(u [+ ref])) + c3*z ;  rnd += c4*<u,u> + c5*<u,z> + c6
 *                  EIReferenceSDELoss.simulate        losses/oc.py:444-510  (+ eq/sdes.py:532-539, 658-666)
 *                  DDPMLikeReferenceSDELoss.simulate  losses/oc.py:584-651  (+ eq/sdes.py:541-555, 668-678)
 *                  DiscreteTimeReversalLossEI.simulate losses/oc.py:906-978
 *                  ExponentialIntegratorSDELoss.simulate losses/oc.py:1319-1397 (DDS)
 * SDENG_FORM_EM    x' = x + ((c1*x [+ c3*ref]) + c2*u)*c4 + c2*(c5*z) ; rnd += 0.5*<u,u>*c4 + <u,c5*z> + c6
 *                  EMReferenceSDELoss.simulate        losses/oc.py:218-296  (PIS: no reference)
 *                  TimeReversalLoss.simulate          losses/oc.py:1133-1238 (no inference control)
 * SDENG_FORM_CMCD  ControlledLangevinSDELoss.simulate losses/oc.py:666-755 (+ eq/sdes.py:101-110)
 * SDENG_FORM_EUBO  the noising loops (x_in = samples of the target; coef rows in ITERATION order, i.e. times T - s run backwards):
 *                  x' = x*c1 + c3*z ; u = c2*ctrl(t_net, x') ; rnd -= c4*<u, ref(x') + u/2> ; rnd += c6*<u, x'> ; rnd -= c5*<u, z>
 *                  EIReferenceSDELoss.compute_eubo    losses/oc.py:512-568  (c2 = 1, c6 = 0)
 *                  EMReferenceSDELoss.compute_eubo    losses/oc.py:298-362  (also DDPMLikeReferenceSDELoss)
 *                  FLAG_TERM_REF / FLAG_TERM_TARGET here mean the INITIAL cost rnd0 = log p_ref(x_in) - log pi~(x_in) (:322, :536);
 *                  DiscreteTimeReversalLossEI.compute_eubo losses/oc.py:980-1036 (no reference, Score/LerpCtrl, c2 = 1, c6 = 0;
 *                  FLAG_INIT_LOGP here adds log p_prior of the NOISED samples at the end, :1032)
 *                  needs either a reference with a ClippedCtrl or no reference with a Score/LerpCtrl.
 */
#define SDENG_FORM_LIN 0
#define SDENG_FORM_EM 1
#define SDENG_FORM_CMCD 2
#define SDENG_FORM_EUBO 3
#define SDENG_FORM_CMCD_EUBO 4 /* ControlledLangevinSDELoss.compute_eubo losses/oc.py:757-828: the CMCD loop run from target samples
                                  with -u; coef rows in iteration order ([0] = ts[N-k], [2],[3] = dt, sqrt(dt) of iteration k,
                                  [4..7] = annealing weights of that time); rnd0 = -log pi~(x_in), + log p_prior(x_out) at the end */

/* Per-step coefficient table: coef[N][SDENG_NCOEF], filled by the host with the reference's own
 * fp32 scalar formulas (eq/sdes.py:456-555, 609-678; losses/oc.py:1369-1371).  Column meaning:
 *            LIN              EM                 CMCD
 *   [0]  t_net            t_net              s            time fed to the drift net
 *   [1]  c1 (x gain)      c1 (+-drift coef)  t            (CMCD: time of the second evaluation)
 *   [2]  c2 (ctrl gain)   c2 = g             dt
 *   [3]  c3 (noise gain)  c3 = g^2           sqrt(dt)
 *   [4]  c4 (0.5*omega)   c4 = dt            s/T
 *   [5]  c5 (sqrt omega)  c5 = sqrt(dt)      1 - s/T
 *   [6]  c6 (rnd const)   c6 (rnd const)     t/T
 *   [7]  score gain       score gain         1 - t/T      LerpCtrl: g(t); ScoreCtrl: 1
 *   [8]  lerp weight t/T  lerp weight        (unused)     LerpCtrl only
 *   [9]  s(tau)   [10] s(tau)^2*sigma_sq(tau)   [11] s(tau)^2   reference marginal (eq/sdes.py:228-229,247)
 *   [12] sigma = sde_ctrl_noise   [13] p = sde_ctrl_dropout   [14] a_k = drift_coeff_t(tau_k)   [15] g_k = diff_coeff_t(tau_k)
 *        LIN / EM with SDENG_FLAG_CTRL_NOISE / _DROPOUT only (else 0); tau_k = the time the loss hands its control (T - s for the RDS
 *        losses and DIS-EI, s for DDS and TimeReversalLoss), with the reference's fp32 formulas of the loss's SDE (eq/sdes.py:143-148)
 * SDENG_FORM_EUBO (rows in iteration order): [0] t_net = T - s, [1] mean factor, [2] control gain (1, or 1/g with
 *   use_rescaling), [3] std factor, [4] running-cost weight (omega | dt g^2), [5] Ito weight (sqrt omega | std/mean),
 *   [6] <u,x> weight (0 | 1/mean - 1 + drift_coeff dt), [9..11] reference marginal at t_net.
 */
#define SDENG_NCOEF 16

/* flags */
#define SDENG_FLAG_ITO 1u          /* accumulate the stochastic integral <u,z> (compute_ito_int)     */
#define SDENG_FLAG_INIT_LOGP 2u    /* rnd0 = log p_prior(x0)  (losses/oc.py:695-699, 935-939, 1164-1168) */
#define SDENG_FLAG_TERM_REF 4u     /* terminal: rnd += log p_ref(x_N)  (losses/oc.py:290, 505, 645, 1390) */
#define SDENG_FLAG_TERM_TARGET 8u  /* terminal: rnd -= log pi~(x_N)                                 */
#define SDENG_FLAG_SPLIT_TILES 16u /* hint for small batches (B <= 8 192 = two tiles per CU; the reference's default evaluation batch is 6 000,
                                      conf/solver/basic_oc_base.yaml:28-30): work on every 16-particle tile with four waves (one per SIMD,
                                      a quarter of the features each) instead of one -- ~2x lower latency when the batch cannot fill the
                                      chip.  Same noise counters; sums are formed in another order, so results equal the default path's
                                      to fp32 round-off, not bit for bit.  Honoured for ClippedCtrl, LIN / EM forms, no / Gaussian /
                                      small-mixture reference, d > 64, no noise_in (xs_out is written); ignored otherwise. */

#define SDENG_FLAG_REMOVE_REF 32u  /* RemoveReferenceCtrl(score, ref_score, use_rescaling=False) (models/reparam.py:46-64): the control the loss sees is
                                      ctrl(t, x) - ref_score(t, x), ref_score = the reference drift of `ref`.  Forward forms (LIN / EM) with a
                                      Score / Lerp / CancelDrift control and a diagonal reference; SDENG_E_UNSUPPORTED otherwise. */

/* sde_ctrl_noise / sde_ctrl_dropout of log-variance training (BaseOCLoss.generative_and_sde_ctrl, losses/oc.py:97-102): the control that drives
 * the step -- after the clip, the score / lerp terms and the FLAG_REMOVE_REF subtraction -- is perturbed before anything consumes it (running
 * cost, update, Ito term; the reference writes it in place through the detached alias, so its value is the control of every term):
 *   CTRL_NOISE    u += coef[12] * eps, eps = the Philox normals of stream 4 with the step noise's counter layout (particle0+p, feature/4, step, 4);
 *   CTRL_DROPOUT  then u = -(coef[14] * x) / coef[15] wherever U > coef[13] (x: the state of the step), U = output word feature % 4 of
 *                 Philox4x32-10 with counter (particle0+p, feature/4, step, 5), as ((bits>>9)+0.5)*2^-23.  `U > p` is the reference's
 *                 convention (`rand_like > sde_ctrl_dropout`): an element is REPLACED with probability 1 - p.
 * (Streams 2 and 3 belong to sdeng_langevin_moves, 6 and 7 to sdeng_rwmh_moves: 0-7 are taken.)  FORM_LIN / FORM_EM with a drift net; SDENG_E_UNSUPPORTED otherwise (CMCD, EUBO, Euler). */
#define SDENG_FLAG_CTRL_NOISE 128u
#define SDENG_FLAG_CTRL_DROPOUT 256u

#define SDENG_FLAG_REUSE_PACK 64u  /* sdeng_ctrl_vjp only: the packed weight images of an earlier call with the same net are still in the
                                      workspace -- skip re-packing (a caller that walks the times one by one, e.g. an adjoint recursion) */

/* ---- distributions (the distr package): log-density and score by hand-coded formulas ------------ */
#define SDENG_DIST_NONE 0
#define SDENG_DIST_GMM_DIAG 1   /* distr/gauss.py:138-244  GMM / TwoModes / ManyModes (MixtureSameFamily)   */
#define SDENG_DIST_GAUSS_DIAG 2 /* distr/gauss.py:597-629  Gauss, Delta (one component, no mixture weights) */
#define SDENG_DIST_ISO_GAUSS 3  /* distr/gauss.py:720-787  IsotropicGauss                                   */
#define SDENG_DIST_PHI4 4       /* distr/phi_four.py:8-96  1-D lattice, Dirichlet-0 boundary                */
#define SDENG_DIST_LOGREG 5     /* distr/logistic_regression.py:11-92 + autograd score distr/base.py:146-154 */
#define SDENG_DIST_GAUSS_FULL 6 /* distr/gauss.py:632-717  GaussFull (MultivariateNormal)                   */
#define SDENG_DIST_RINGS 7      /* distr/rings.py:38-109   2-D rings: radial Gaussian mixture x uniform angle     */
#define SDENG_DIST_GMM_FULL 8   /* distr/gauss.py:310-520  GMMFull / TwoModesFull (full covariances), as the TARGET of a Score / Lerp /
                                   CancelDrift control only (score_mog_full :110-121 inside the step loop): loc [k,d], scale = eigenvalues
                                   [k,d] and aux = eigenvectors [k,d,d] (row-major, columns = vectors) of each covariance, w [k].  Forward
                                   forms without a reference drift (PIS / DDS / DIS); its log-density is not evaluated here (no
                                   FLAG_TERM_TARGET with it): SDENG_E_UNSUPPORTED otherwise. */
#define SDENG_DIST_CHECKERBOARD 9 /* distr/checkerboard.py:6-94  2-D checkerboard: a mixture of uniform squares (d must be 2).  k squares,
                                     loc = lower corners [k,2], scale = upper corners [k,2], w = the log-density inside each square [k]
                                     (the caller evaluates the reference's own expression at the square's centre).  Square c holds x
                                     when loc[c] <= x < scale[c] in both coordinates (Uniform.log_prob is half-open); the squares must be
                                     disjoint.  log pi~(x) = w[c] inside square c, -inf outside every square and for NaN input; score = 0
                                     (the reference returns zeros, no autograd).  Particles that end outside every square get rnd = +inf.
                                     No sdeng_langevin_moves or sdeng_kl_adjoint with it (SDENG_E_UNSUPPORTED). */

typedef struct sdeng_dist {
  int32_t kind;      /* SDENG_DIST_*                                                              */
  int32_t k;         /* GMM: number of components; LOGREG: number of data rows                    */
  const float* loc;  /* GMM [k,d]; GAUSS_DIAG/GAUSS_FULL [d]; LOGREG: X [k,d-1]; RINGS: radii [k <= 8]; CHECKERBOARD: low [k,2] */
  const float* scale;/* GMM [k,d]; GAUSS_DIAG [d] (std-dev); GAUSS_FULL: precision [d,d]; LOGREG: y [k]; CHECKERBOARD: high [k,2] */
  const float* w;    /* GMM, RINGS: unnormalised mixture weights [k]; GAUSS_FULL: inverse Cholesky factor L^-1 [d,d];
                        CHECKERBOARD: log-density inside each square [k] */
  float p0, p1, p2, p3; /* ISO_GAUSS: loc, scale, norm_const = -0.5*d*log(2*pi*scale^2), scale^2 (both as the
                           reference computes them in fp32, distr/gauss.py:759-760); PHI4: a, b, beta;
                           LOGREG: weight_scale, intercept_mean, intercept_scale, threshold;
                           GAUSS_FULL: p0 = sum(log diag L); RINGS: p0 = radial std-dev (d must be 2) */
  float clip;        /* clip applied to the log-density (solver/oc.py:80-87 clip_target); <=0: none */
  const float* aux;  /* GAUSS_FULL as x0_dist: Cholesky factor L [d,d] (row-major, lower) of the covariance; else NULL */
} sdeng_dist;

/* ---- drift net: models/mlp.py:99-143 FourierMLP(num_layers=4, channels=64, GELU) wrapped by
 *      models/reparam.py:18-43 ClippedCtrl / :63-117 ScoreCtrl / :148-199 LerpCtrl ------------ */
#define SDENG_CTRL_CLIPPED 0
#define SDENG_CTRL_SCORE 1
#define SDENG_CTRL_LERP 2
/* no drift net: EulerIntegrator.integrate (eq/integrator.py:93-129) of an uncontrolled linear SDE (OU.drift/diff,
 * eq/sdes.py:143-148; the inference process of solver/oc.py:162-180) or of the classic Langevin SDE (LangevinSDE,
 * eq/sdes.py:46-76; solver/langevin.py:36-66).  form = SDENG_FORM_EM, no reference; per step
 *   x' = x + (coef[1] x + clip(coef[7] score_target(x), net.clip_score)) coef[4] + coef[2] (z coef[5])
 * (target.kind NONE: no score term).  rnd_out is zero-filled; xs_out carries the N+1 states. */
#define SDENG_CTRL_NONE 3
/* CancelDriftCtrl (models/reparam.py:120-145, conf/model/langevin_init.yaml): a ScoreCtrl that also cancels the SDE's drift,
 *   u = clip(net) + coef[8] x + coef[7] (scale clip(score_target(x)) s_theta(t))
 * with coef[8] = drift_coeff(t)/g(t), coef[7] = g(t)/2 at the net's time (use_rescaling; else drift_coeff/g^2 and 1/2). */
#define SDENG_CTRL_CANCEL_DRIFT 4
#define SDENG_HIDDEN 64

typedef struct sdeng_time_embed { /* models/mlp.py:57-96 TimeEmbed */
  const float* coeff;             /* timestep_coeff [64] (linspace(0.1,100,64))          */
  const float* phase;             /* timestep_phase [64]                                  */
  const float* w[4];              /* hidden_layer[i].weight: [64,128] for i=0, [64,64] after */
  const float* b[4];              /* hidden_layer[i].bias [64]                            */
  int32_t n_hidden;               /* num_layers - 1 (1 for the MLP's embed, 3 for score_model) */
  int32_t dim_out;                /* 64 (MLP embed) or 1 (score_model)                    */
  const float* w_out;             /* out_layer.weight [dim_out,64]                        */
  const float* b_out;             /* out_layer.bias [dim_out]                             */
} sdeng_time_embed;

typedef struct sdeng_net {
  int32_t ctrl_kind;              /* SDENG_CTRL_*                                         */
  int32_t reserved;
  const float *w_in, *b_in;       /* input_embed  [64,d], [64]                            */
  const float *w_h1, *b_h1;       /* hidden_layer.0 [64,64], [64]                         */
  const float *w_h2, *b_h2;       /* hidden_layer.1 [64,64], [64]                         */
  const float *w_out, *b_out;     /* out_layer [d,64], [d]                                */
  sdeng_time_embed t_embed;       /* base_model.timestep_embed (dim_out 64)               */
  sdeng_time_embed score_model;   /* ScoreCtrl/LerpCtrl score_model (dim_out 1); n_hidden=0: absent */
  float clip_model;               /* reparam.py:33-40; <=0: no clipping                   */
  float clip_score;               /* reparam.py:91-100; <=0: none                         */
  float scale_score;              /* reparam.py:114                                       */
  float reserved_f;
} sdeng_net;

/* ---- reference drift (solver/oc.py:535-576 change_reference_type -> eq/sdes.py:265-345) ---- */
#define SDENG_REF_NONE 0
#define SDENG_REF_GAUSS_DIAG 1 /* marginal_score, diagonal var_init            eq/sdes.py:265-279 */
#define SDENG_REF_GMM_DIAG 2   /* marginal_gmm_score, diagonal variances_init  eq/sdes.py:329-345 */

/* marginal_gmm_score with full covariance matrices, score_mog_full (distr/gauss.py:110-121, eq/sdes.py:329-345), in the
 * eigen form the reference itself accepts (eq/sdes.py:228-238: variances_init = (D, P), covariance_c = P_c diag(D_c) P_c^T):
 * vars_init holds the eigenvalues D [k,d], eigvecs the eigenvectors P [k,d,d] row-major (P[c][i][j] = i-th coordinate of
 * the j-th eigenvector).  A caller holding covariance matrices passes their symmetric eigendecomposition. */
#define SDENG_REF_GMM_FULL 3

typedef struct sdeng_ref {
  int32_t kind;
  int32_t k;               /* GMM components (1 for GAUSS_DIAG)                      */
  const float* means_init; /* [k,d]                                                   */
  const float* vars_init;  /* [k,d]  (GMM_FULL: eigenvalues of the covariances)      */
  const float* weights;    /* [k] unnormalised (normalised like distr/gauss.py:100)   */
  const float* eigvecs;    /* [k,d,d] GMM_FULL only, else NULL                        */
  int32_t shared_var;      /* GMM_DIAG: 1 = the caller guarantees that all k rows of vars_init are equal (the reference's default
                              initialisation, variances_init = v * ones): mixtures with 4 < k <= 64 then run on the matrix pipe.
                              The promise is checked on the device: if the rows differ, x_out and rnd_out come back NaN. */
  int32_t reserved;
} sdeng_ref;

/* ---- noise ---------------------------------------------------------------------------------
 * noise_in != NULL : injected, z[k] = noise_in[k*B*d ...] -- replays the reference's one
 *                    randn_like(x) per step (losses/oc.py:277, eq/sdes.py:537, losses/oc.py:722, 1372, 1222);
 * noise_in == NULL : counter-based Philox4x32-10, counter (particle0+p, feature/4, step, stream), key = seed,
 *                    two Box-Muller pairs on u = ((bits>>9)+0.5)*2^-23; independent of sharding.
 */
/* ---- initial particles -------------------------------------------------------------------------
 * x_in != NULL : the caller's x0 [B,d] (e.g. prior.sample((B,)) as solver/oc.py:132 does).
 * x_in == NULL : x0 is drawn by the engine from `x0_dist`, z = the Philox normals of stream 1 at step 0 (same counter layout as
 *                the step noise, so x0 of global particle p does not depend on the sharding):
 *     ISO_GAUSS   x0 = p0 + p1 * z                IsotropicGauss.sample   distr/gauss.py:772-787 (no truncation)
 *     GAUSS_DIAG  x0 = loc + scale * z            Gauss.sample distr/gauss.py:235-239;  scale == NULL: x0 = loc  (Delta.sample, distr/delta.py:27-31)
 *     GAUSS_FULL  x0 = loc + L z  (L = aux)       GaussFull.sample        distr/gauss.py:709-713 (MultivariateNormal)
 *   A sampler kernel writes x0 into the workspace -- or into x0_out ([B,d], optional) -- ahead of the step loop: one launch,
 *   0.2 % of a cfg-2 pass.  (A step-loop variant that drew x0 in registers was measured 1-4 % slower and dropped)
 */
typedef struct sdeng_desc {
  int32_t abi_version;   /* SDENG_ABI_VERSION                                              */
  int32_t form;          /* SDENG_FORM_*                                                   */
  uint32_t flags;        /* SDENG_FLAG_*                                                   */
  int32_t B, d, N;       /* particles (this shard), dimension (<=128), steps               */
  int64_t particle0;     /* global index of this shard's first particle (Philox counter)   */
  uint64_t seed;         /* Philox key                                                     */
  const float* coef;     /* [N][SDENG_NCOEF], device                                        */
  const float* x_in;     /* [B,d], or NULL: draw x0 from x0_dist                             */
  float* x_out;          /* [B,d]                                                           */
  float* rnd_out;        /* [B]  (the reference's rnd[B,1])                                 */
  float* xs_out;         /* optional trajectory [N+1,B,d] (return_traj=True), or NULL       */
  const float* noise_in; /* optional [N,B,d], or NULL                                       */
  sdeng_net net;
  sdeng_ref ref;
  sdeng_dist target;     /* terminal cost + (ScoreCtrl/LerpCtrl/CMCD) target score          */
  sdeng_dist ref_dist;   /* terminal reference log-density (FLAG_TERM_REF)                  */
  sdeng_dist prior;      /* initial log-density (FLAG_INIT_LOGP); LerpCtrl/CMCD prior score  */
  float cmcd_g;          /* ControlledLangevinSDE.diff_coeff          eq/sdes.py:93-95     */
  float cmcd_clip;       /* ControlledLangevinSDE.clip_score (<=0: none) eq/sdes.py:105-110 */
  void* workspace;       /* device scratch, >= sdeng_workspace_bytes(desc)                  */
  size_t workspace_bytes;
  void* ev_start;        /* optional hipEvent_t recorded on `stream` right before the step-loop kernel */
  void* ev_stop;         /* optional hipEvent_t recorded right after it (roofline timing)            */
  sdeng_dist x0_dist;    /* distribution of x0 when x_in == NULL (see above)                 */
  float* x0_out;         /* optional [B,d]: the x0 that was drawn                             */
} sdeng_desc;

/* Version of this ABI compiled into the library. */
int sdeng_abi_version(void);

/* Message of the calling thread's most recent error ("" if none). */
const char* sdeng_last_error(void);

/* Device scratch needed by sdeng_simulate for this descriptor (packed MFMA weight image,
 * per-step embedding and reference tables).  Pure host arithmetic; 0 on a malformed descriptor. */
size_t sdeng_workspace_bytes(const sdeng_desc* desc);

/* Run one whole simulate() loop (all N steps, initial and terminal cost) on `stream`.
 * Replaces the Python step loops listed under SDENG_FORM_*. */
int sdeng_simulate(const sdeng_desc* desc, void* stream);

/* Estimators of BaseOCLoss.compute_results (losses/oc.py:150-161) and the normalised ESS of
 * eval/metrics.py:135-140 from rnd[B]:
 *   stats[0] = mean(-rnd) (elbo)      stats[1] = logsumexp(-rnd) - log(B) (log_norm_const_is)
 *   stats[2] = var(rnd) (unbiased)    stats[3] = (sum w)^2 / sum w^2 / B  with w = softmax(-rnd)
 *   stats[4] = max(-rnd)              stats[5] = sum exp(-rnd - max)      stats[6] = sum exp(2(-rnd - max))
 *   stats[7] = sum(-rnd)              (4..7: partials for the multi-GPU combine)
 * weights_out (optional, [B]) receives softmax(-rnd, 0).  stats is device memory, 8 floats. */
int sdeng_logz(const float* rnd, int64_t B, float* stats, float* weights_out, void* workspace, size_t workspace_bytes,
               void* stream);
size_t sdeng_logz_workspace_bytes(void);

/* Standalone pieces, exported for unit parity tests against the oracle:
 * FourierMLP (+ctrl wrapper) forward at one time, u[B,d] (models/mlp.py:135-143, reparam.py:42,112-117,186-199) */
int sdeng_ctrl_forward(const sdeng_desc* desc, float t_net, float score_gain, float lerp_w, const float* x, float* u_out,
                       void* stream);
/* distribution log-density [B] and score [B,d] (either output may be NULL) */
int sdeng_dist_eval(const sdeng_dist* dist, int32_t B, int32_t d, const float* x, float* logp_out, float* score_out,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t sdeng_dist_workspace_bytes(const sdeng_dist* dist, int32_t d);
/* Counter-based normals exactly as the step loop draws them: out[B,d] for one step. */
int sdeng_philox_normal(uint64_t seed, int32_t step, int64_t particle0, int32_t B, int32_t d, uint32_t stream_id,
                        float* out, void* stream);
/* The same for n_steps consecutive steps in one launch: out[n_steps,B,d] (the noise a training call keeps, losses/oc.py:277, :537). */
int sdeng_philox_normal_steps(uint64_t seed, int32_t step0, int32_t n_steps, int64_t particle0, int32_t B, int32_t d,
                              uint32_t stream_id, float* out, void* stream);

/* Training direction: fused forward + backward of the drift net -- FourierMLP under ClippedCtrl -- over
 * M = n_times * rows_per_time rows; row r = k * rows_per_time + b is the state x[r] at time desc->coef[k][0].  Replaces the autograd
 * graph that losses/oc.py:83-103 (generative_and_sde_ctrl) builds per step and loss.backward() walks (models/mlp.py:135-143,
 * models/reparam.py:33-43).  Reads desc->{abi_version, d, coef, net, workspace}.  `cot` [M,d] is the cotangent of the control u.
 * Per-row outputs, all [M,64] unless noted:  a0, a1, a2 = gelu of the three hidden pre-activations;  d0, d1, d2 = cotangents of those
 * pre-activations;  dout [M,d] = cot under ClippedCtrl's clip mask;  gx [M,d] (optional) = gradient w.r.t. the state;  u_out [M,d]
 * (optional) = the control itself.  cot == NULL: forward only (u_out required, the other outputs may be NULL).  The
 * parameter gradients are the caller's six products over the rows: dW_out = dout^T a2, dW_2 = d2^T a1, dW_1 = d1^T a0,
 * dW_in = d0^T x, bias gradients = column sums, cotangent of the time embedding of time k = sum over its rows of d0. */
int sdeng_ctrl_vjp(const sdeng_desc* desc, int32_t n_times, int32_t rows_per_time, const float* x, const float* cot, float* a0, float* a1,
                   float* a2, float* d0, float* d1, float* d2, float* dout, float* gx, float* u_out, void* stream);
size_t sdeng_ctrl_vjp_workspace_bytes(int32_t d, int32_t n_times);

/* KL-method training (BaseOCLoss.compute_loss kl branch, losses/oc.py:105-131): the gradient of the mean log-weight through the
 * trajectory -- what loss.backward() computes by walking the autograd graph of simulate() (losses/oc.py:258-284 EM, :478-502 EI) -- as the
 * discrete adjoint of the recursion sdeng_simulate integrates, in ONE launch.  The states xs[k] (k = 0 .. N-1, from sdeng_simulate's xs_out)
 * are constants; per 16 particles the kernel walks k = N-1 .. 0 with the adjoint state lambda in registers:
 *     cot_k  = alpha_k lambda + w_b (beta_k u_k + gamma_k z_k)        u_k = the control at (coef[k][0], xs[k]), recomputed
 *     lambda = A_k lambda + C_k H_ref(xs[k]) lambda + J_u^T cot_k     H_ref: Jacobian of the noised reference's score (eq/sdes.py:265-279, 329-345)
 * (FORM_LIN: alpha = c2, beta = 2 c4, gamma = c5, A = c1, C = c2;  FORM_EM: alpha = c2 c4, beta = c4, gamma = c5, A = 1 + c4 c1, C = c4 c3;
 * gamma = 0 without SDENG_FLAG_ITO) and writes the per-row arrays of sdeng_ctrl_vjp at row k * B + b: the parameter gradients are the same
 * six products.  Reads desc->{abi_version, B, d, N, form, flags & ITO, coef, net, ref (NONE / GAUSS_DIAG / GMM_DIAG), target, workspace}.
 * Controls: ClippedCtrl, and ScoreCtrl / LerpCtrl / CancelDriftCtrl (models/reparam.py:63-199; the latter two with the per-step gains of
 * coef[7], coef[8] and, for LerpCtrl, desc->prior = the IsotropicGauss whose score is interpolated: d lerp/dx = (1 - t/T)(-1/var) + (t/T) H_pi)
 * -- written out for ScoreCtrl (BASELINE configs 1 and 3: DDS, PIS) -- on a diagonal mixture or phi^4 target
 * (desc->target of kind GMM_DIAG / PHI4): u = clip(net) + scale clip(score_pi(x)) s_theta(t); the state gradient gains
 * scale s_theta H_pi(x) (mask cot) (closed-form Hessian-vector product: mixture, or the lattice's tridiagonal Hessian; skipped with detach_score), and `dst` receives the cotangent of s_theta(t_k) per particle -- the caller sums
 * it over the particles and back-propagates the N values through the small score model. */
typedef struct sdeng_adjoint {
  const float* xs;      /* [N][B][d] states x_0 .. x_{N-1}                                                   */
  const float* noise;   /* [N][B][d] the normals of the trajectory (sdeng_philox_normal_steps of its seed); required with FLAG_ITO */
  const float* w;       /* [B] d loss / d rnd_b (1/B on the particles that pass the loss's filter, else 0)   */
  const float* lam_in;  /* [B][d] lambda_N = d (sum_b w_b terminal(x_N,b)) / d x_N                           */
  float* lam_out;       /* [B][d] lambda_0, or NULL                                                          */
  float *a0, *a1, *a2, *d0, *d1, *d2; /* [N*B][64] each, as sdeng_ctrl_vjp                                    */
  float* dout;          /* [N*B][d]                                                                          */
  float* dst;           /* [N*B] ScoreCtrl: <cot, scale clip(score_pi)>, the cotangent of s_theta(t_k) per particle; else NULL */
  int32_t detach_score; /* ScoreCtrl(detach_score=True): the target score is treated as a constant of x     */
  const float* score;   /* [N*B][d] or NULL.  Given: the target score of every row, evaluated by the caller (sdeng_dist_eval) and treated as
                           a constant of x -- for targets whose score the reference makes by autograd without a graph (distr/base.py:146-154:
                           LogisticRegression), desc->target is then ignored */
} sdeng_adjoint;
int sdeng_kl_adjoint(const sdeng_desc* desc, const sdeng_adjoint* adj, void* stream);
size_t sdeng_kl_adjoint_workspace_bytes(const sdeng_desc* desc);

/* KL-method training of CMCD (ControlledLangevinSDELoss with method 'kl' / 'kl_ito': back-propagation through simulate(train=True),
 * losses/oc.py:666-755, rnd0 = 0 :695-699, with the annealed drift of eq/sdes.py:101-110 whose clip is per element, utils/common.py:109-112)
 * as ONE launch.  Step j of that loop reads the control and the drift at BOTH of its ends,
 *     x_{j+1} = x_j + (b_j + g u_j) dt_j + g db_j ;   cost_j = (b_j + b_{j+1})/g + u_j - u_{j+1} ;   rnd += 0.5 |cost_j|^2 dt_j + <cost_j, db_j>
 * (:722-742; u_j = ctrl(t_j, x_j) at FORWARD time, b_j = clip(0.5 g^2 (tau_j s_pi(x_j) + (1 - tau_j) s_prior(x_j)), +-cmcd_clip), tau_j = t_j/T,
 * db_j = sqrt(dt_j) z_j), so evaluation point j = 0 .. N receives cotangents from steps j - 1 and j.  The states xs[j] (sdeng_simulate's
 * xs_out, all N + 1 of them) are constants; the caller evaluates the costs in one batched forward pass and passes
 *     cbar[j] = cost_j dt_j + db_j          (0 <= j < N; per unit weight)
 * and per 16 particles the kernel walks j = N .. 0 with the adjoint state Lambda in registers (c_j = w_b cbar[j], c_{-1} = c_N = 0, dt_N = 0):
 *     ubar_j   = g dt_j Lambda + c_j - c_{j-1}                     cotangent of u_j
 *     v_j      = dt_j Lambda + (c_j + c_{j-1}) / g                 cotangent of b_j
 *     Lambda  += J_u(t_j, xs[j])^T ubar_j + 0.5 g^2 (tau_j H_pi(xs[j]) + (1 - tau_j) H_prior) (mask_j * v_j)
 * starting from lam_in = d (sum_b w_b (-log pi~(x_N,b))) / d x_N.  mask_j = 1 where the unclipped drift lies in [-cmcd_clip, cmcd_clip] (torch.clip's
 * backward); H_prior = -1/var on the diagonal; H_pi = the closed-form Hessian-vector product of a diagonal mixture / Gaussian or of the phi^4
 * lattice.  For a target whose score the reference makes by autograd WITHOUT a graph (distr/base.py:146-154: LogisticRegression) backward()
 * sees the score as a constant of x: the caller passes the target score of every row in `score` (sdeng_dist_eval), it feeds the drift's clip
 * mask and a ScoreCtrl's score term, and H_pi = 0.  J_u^T and the per-row outputs are those of sdeng_kl_adjoint over the (N + 1) * B rows
 * (row = j * B + b): ClippedCtrl, or ScoreCtrl (models/reparam.py:63-117: + scale s_theta(t_j) H_pi under the score clip's mask unless
 * detach_score, and `dst`).  A particle with w_b = 0 (filtered by the loss) contributes exactly zero, whatever its costs hold.
 * Reads desc->{abi_version, B, d, N (steps), coef ([N + 1][SDENG_NCOEF], the SDENG_FORM_CMCD table sdeng_simulate was given), net, target, prior,
 * cmcd_g, cmcd_clip, workspace}.  SDENG_E_UNSUPPORTED, each with its reason in sdeng_last_error(): a full-covariance prior (GAUSS_FULL), a
 * full-covariance target (GAUSS_FULL / GMM_FULL), a RINGS target, a CHECKERBOARD target, d > 128, a control other than ClippedCtrl / ScoreCtrl
 * (KL training of those runs the adjoint step by step on the host). */
typedef struct sdeng_cmcd_adjoint {
  const float* xs;      /* [N+1][B][d] states x_0 .. x_N                                                      */
  const float* cbar;    /* [N][B][d] cost_j dt_j + db_j                                                        */
  const float* w;       /* [B] d loss / d rnd_b                                                                */
  const float* lam_in;  /* [B][d]                                                                              */
  float* lam_out;       /* [B][d] Lambda_0, or NULL                                                            */
  float *a0, *a1, *a2, *d0, *d1, *d2; /* [(N+1)*B][64] each, as sdeng_ctrl_vjp                                 */
  float* dout;          /* [(N+1)*B][d]                                                                        */
  float* dst;           /* [(N+1)*B] ScoreCtrl: <ubar, scale clip(score_pi)>, the cotangent of s_theta(t_j) per particle; else NULL */
  int32_t detach_score; /* ScoreCtrl(detach_score=True)                                                        */
  const float* score;   /* [(N+1)*B][d]: the target score of every row; required for a LOGREG target (graph-less score), else NULL */
} sdeng_cmcd_adjoint;
int sdeng_cmcd_kl_adjoint(const sdeng_desc* desc, const sdeng_cmcd_adjoint* adj, void* stream);
size_t sdeng_cmcd_kl_adjoint_workspace_bytes(const sdeng_desc* desc);

/* Annealed samplers: n_moves Langevin moves of B chains in ONE launch -- mala_step / ula_step of additions/mcmc.py:77-135,
 * 189-221 with the per-chain step-size heuristic of :55-74 (target_acceptance > 0), as smc_sampler / re_sampler / mcmc_sample apply
 * them move after move (additions/ebm_mle.py:120-160, 340-380; experiments/benchmark_utils.py:300-330).  Density: the geometric path
 * log pi_t = (1 - t[b]) log p_prior + t[b] log pi~ (prior == NULL or kind NONE: the target alone; t == NULL: 1).  State in / out:
 * x [B,d], lp [B] = log pi_t(x), grad [B,d], step [B].  Noise: injected normals z [n_moves,B,d] and uniforms u [n_moves,B] (u unused
 * by the unadjusted move) -- e.g. drawn from the host framework's generator in the reference's order -- or NULL: Philox streams 2 / 3
 * keyed by (seed, chain0 + chain, move).  samples (optional) [n_moves - keep_from, B, d]: the states after moves keep_from..;
 * acc_sum (optional) [B]: sum over those moves of min(1, acceptance ratio); acc_last (optional) [B]: that of the last move. */
int sdeng_langevin_moves(const sdeng_dist* prior, const sdeng_dist* target, int32_t B, int32_t d, int32_t n_moves, int32_t keep_from,
                         int32_t unadjusted, float target_acceptance, const float* t, float* x, float* lp, float* grad, float* step,
                         const float* z, const float* u, uint64_t seed, int64_t chain0, float* samples, float* acc_sum, float* acc_last,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t sdeng_langevin_moves_workspace_bytes(const sdeng_dist* prior, const sdeng_dist* target, int32_t d);

/* Learned-reference data set: n_moves random-walk Metropolis moves of B chains in ONE launch -- rwmh_step of additions/mcmc.py:256-293 with
 * the per-chain step-size heuristic of :54-72 (target_acceptance > 0), as mcmc_sample(mcmc_type='rwmh') applies them move after move
 * (experiments/benchmark_utils.py:299-327; the checkerboard's data set, experiments/sample_toy_gmm_mcmc.py:112-115).  Proposal
 * x + step[b] * z (the standard deviation is the step itself), log_acc = log pi~(prop) - lp[b], accepted iff log(u) < log_acc.  Every
 * distribution kind sdeng_dist_eval has a log-density for, SDENG_DIST_CHECKERBOARD included: non-finite log-densities keep their IEEE
 * meaning (-inf: rejected, the step shrinks; +inf from a start outside every square: accepted, the step grows; NaN: rejected, the step
 * stays).  No tempering (the reference has no tempered random-walk move).  State in / out: x [B,d], lp [B] = log pi~(x), step [B].
 * Noise: injected normals z [n_moves,B,d] and uniforms u [n_moves,B], both or neither; NULL: Philox stream 6 for the normals (the
 * counter layout of the step noise, keyed by (seed, chain0 + chain, move): sdeng_philox_normal_steps(..., stream_id = 6) replays them)
 * and stream 7 for the uniforms (counter (chain0 + chain, 0, move, 7), output word 0).  samples / acc_sum / acc_last: as
 * sdeng_langevin_moves.  d <= 255 (SDENG_E_UNSUPPORTED above); keep_from <= n_moves. */
int sdeng_rwmh_moves(const sdeng_dist* target, int32_t B, int32_t d, int32_t n_moves, int32_t keep_from, float target_acceptance,
                     float* x, float* lp, float* step, const float* z, const float* u, uint64_t seed, int64_t chain0,
                     float* samples, float* acc_sum, float* acc_last, void* workspace, size_t workspace_bytes, void* stream);
size_t sdeng_rwmh_moves_workspace_bytes(const sdeng_dist* target, int32_t d);

/* prior.sample((B,)) on the device, out[B,d]: exactly the x0 that sdeng_simulate draws for x_in == NULL with the same
 * (dist, seed, particle0).  Replaces IsotropicGauss.sample / Gauss.sample / Delta.sample / GaussFull.sample (distr/gauss.py:772-787,
 * 235-239, 709-713; distr/delta.py:27-31). */
int sdeng_sample_x0(const sdeng_dist* dist, uint64_t seed, int64_t particle0, int32_t B, int32_t d, float* out, void* stream);

/* Sample-quality metrics of the reference's evaluation layer (eval/metrics.py:173-191 applies them to the samples of every model).
 *
 * sdeng_sinkhorn: the entropy-regularised p-Wasserstein distance of Sinkhorn.compute (eval/sinkhorn.py:64-177, written there on pykeops
 * lazy tensors) between x [n,d] and y [m,d]:  M_ij = (sum_k |x_ik - y_jk|^p)^(1/p), p in {1, 2} (else SDENG_E_UNSUPPORTED);
 * w_x [n], w_y [m] or both NULL = uniform 1/n and (1/m)(n/m) (:123-126);  u = 0, v = eps log w_y;  per iteration
 *     u_i = eps (log w_x,i - LSE_j((v_j - M_ij) / eps)),   v_j = eps (log w_y,j - LSE_i((u_i - M_ij) / eps))  with the new u,
 * until max|du| < stop_thresh and max|dv| < stop_thresh or max_iters iterations (:143-160); then
 * distance = sum_ij P_ij M_ij with P_ij = exp((u_i + v_j - M_ij) / eps), corr_x_to_y[i] = argmax_j P_ij, corr_y_to_x[j] = argmax_i P_ij
 * (:162-171).  M is built once from differences accumulated in double and kept as fp32 in the workspace when the workspace has room for
 * it (sdeng_sinkhorn_workspace_bytes(n, m, d, 1)) and n m 4 <= SDENG_SINKHORN_MATRIX_MAX_BYTES: each half-iteration is then one
 * streaming pass over it.  With the smaller workspace (..., 0), or beyond that size, every pass recomputes the costs from x and y --
 * same arithmetic, same result, O(n + m) memory.  u, v and the exponents are double inside; u_out [n], v_out [m] (optional) are fp32.
 * One 16-byte read-back per iteration (the stop test): the call returns with the stream synchronised and `result` (host memory) filled.
 * Reductions run in a fixed order: two calls on the same input agree bit for bit. */
#define SDENG_SINKHORN_MATRIX_MAX_BYTES (1ull << 30)
typedef struct sdeng_sinkhorn_result {
  double distance;
  double max_err_u, max_err_v; /* max |change| of u and v in the last iteration        */
  int32_t iters;               /* iterations run                                        */
  int32_t materialised;        /* 1: the cost matrix was kept in the workspace          */
} sdeng_sinkhorn_result;
int sdeng_sinkhorn(const float* x, const float* y, int32_t n, int32_t m, int32_t d, int32_t p, double eps, int32_t max_iters,
                   double stop_thresh, const float* w_x, const float* w_y, float* u_out, float* v_out, int32_t* corr_x_to_y,
                   int32_t* corr_y_to_x, sdeng_sinkhorn_result* result, void* workspace, size_t workspace_bytes, void* stream);
size_t sdeng_sinkhorn_workspace_bytes(int32_t n, int32_t m, int32_t d, int32_t materialise);

/* sdeng_mmd_median: mmd_median(X, Y) of additions/mmd.py:30-59 for X, Y [n,d] (n == m >= 2 as asserted there) without its n x n
 * matrices.  The bandwidth is the lower median (torch.median: rank (N - 1) / 2) of the N = n (2n - 1) squared distances
 * {XX, i < j} + {YY, i < j} + {XY, all} -- the pairs i < j of the pooled sample -- found exactly by a three-pass radix selection over the
 * bit patterns of the fp32 distances (each pass recomputes them); then the Gaussian-kernel sums of :47-56 in double and
 * out[0] = sqrt(max(1e-20, mmd^2)), out[1] = bandwidth_sq (device memory, 2 floats).  Workspace: O(n) (48 KB of counters and
 * 6 KB of partial sums per 1024 rows).  No read-back; integer counters are the only atomics, so reruns agree bit for bit. */
int sdeng_mmd_median(const float* X, const float* Y, int32_t n, int32_t m, int32_t d, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t sdeng_mmd_median_workspace_bytes(int32_t n, int32_t d);

/* Energy-based (tilted-potential) references: log-density and score of GMMTitledPotential / GaussTiltedPotential (models/reparam.py:277-520
 * and :485-606; what net.unnorm_log_prob, net.unnorm_log_prob_and_grad and net(t, x) compute: models/reparam.py:354-482) around
 * FourierMLP(num_layers=6, channels=128, GELU) (models/mlp.py:57-143), in ONE launch over M = n_times * rows_per_time rows; row r is the
 * state x[r] at time r / rows_per_time -- the layout of sdeng_ctrl_vjp, and of replica exchange's levels x chains
 * (additions/ebm_mle.py:440-446).  Per row, with s = sde.s(t), sigma^2 = sde.sigma_sq(t) and (s', sigma'^2) the same at t' = max(t, t_limit):
 *     xs = (x - s mean_gauss) / c_i,  c_i = s sqrt(var_gauss + sigma^2)                                   scaling_input   reparam.py:420-424
 *     v  = FourierMLP(t, xs):  h0 = W_in xs + b_in + TimeEmbed(t);  h_l = W_l gelu(h_{l-1}) + b_l (l = 1..4);  v = W_out gelu(h4) + b_out
 *     base_lp = -<v, xs>  (tilt 'dot', :428-430);   base_grad = -(v + J^T xs) / c_i,  J = dv/dxs: one backward pass with cotangent xs
 *     prior: log-density and score of the mixture noised to t' (sde.marginal_gmm_params, eq/sdes.py:208-307; weights renormalised,
 *            reparam.py:376-418): diagonal variances [k,d], or full covariances in eigen form, covariance_c = P_c diag(D_c) P_c^T, noised
 *            precision P_c diag(1 / (s'^2 (D_c + sigma'^2))) P_c^T (eq/sdes.py:232-239); k = 1 is GaussTiltedPotential (:571-606)
 *     log_prob = prior_lp + f base_lp;   grad = prior_grad + f base_grad;   f = s(t) with use_s_t_scaling, else 1                  :457-476
 * tinfo [n_times][5] = (t, s, sigma^2, s', sigma'^2), computed by the caller with the SDE object in fp32 as the reference does: the
 * kernel knows no SDE kinds.  log_prob [M] and grad [M,d] are each optional (not both NULL); without grad the backward pass is skipped.
 * SDENG_E_INVALID: null pointers, d outside [1,128], k outside [1,16], M != n_times * rows_per_time, wrong abi_version.
 * SDENG_E_UNSUPPORTED (reason in sdeng_last_error): a net other than 6 layers x 128 channels, a tilt other than 'dot', use_scaling_factor.
 * Workspace: the packed weight images first (SDENG_FLAG_REUSE_PACK in flags: those of an earlier call with the same parameters are still
 * there), then the per-wave pre-activations of the backward pass.  States or activations beyond 65 504 are not guarded (NaN). */
#define SDENG_TILT_DOT 0
#define SDENG_TILT_SQ_NORM 1
#define SDENG_TILT_SUM 2
typedef struct sdeng_tilted {
  int32_t abi_version;      /* SDENG_ABI_VERSION                                                    */
  uint32_t flags;           /* SDENG_FLAG_REUSE_PACK or 0                                           */
  int32_t M, n_times, rows_per_time, d;
  int32_t k;                /* mixture components, 1..16                                            */
  int32_t full_cov;         /* 0: vars = variances [k,d];  1: vars = eigenvalues D [k,d], eigvecs = P [k,d,d] (row-major, columns = vectors) */
  int32_t num_layers, channels;       /* of the FourierMLP: 6 and 128                               */
  int32_t tilt_type;        /* SDENG_TILT_*                                                         */
  int32_t use_scaling_factor, use_s_t_scaling;
  int32_t reserved;
  const float* x;           /* [M,d]                                                                */
  const float* tinfo;       /* [n_times][5]                                                         */
  const float *w_in, *b_in; /* input_embed [128,d], [128]                                           */
  const float* w_h[4];      /* hidden_layer.0..3 [128,128]                                          */
  const float* b_h[4];      /* [128]                                                                */
  const float *w_out, *b_out;         /* out_layer [d,128], [d]                                     */
  const float *te_coeff, *te_phase;   /* timestep_embed.timestep_coeff / _phase [128]               */
  const float *te_w1, *te_b1;         /* timestep_embed.hidden_layer.0 [128,256], [128]             */
  const float *te_w2, *te_b2;         /* timestep_embed.out_layer [128,128], [128]                  */
  const float *mean_gauss, *var_gauss; /* [d] moments of the un-noised prior (scaling_input)         */
  const float* weights;     /* [k] unnormalised                                                     */
  const float* means;       /* [k,d]                                                                */
  const float* vars;        /* [k,d]                                                                */
  const float* eigvecs;     /* [k,d,d] with full_cov, else NULL                                     */
  float* log_prob;          /* [M] or NULL                                                          */
  float* grad;              /* [M,d] or NULL                                                        */
  void* workspace;
  size_t workspace_bytes;
} sdeng_tilted;
int sdeng_tilted_eval(const sdeng_tilted* desc, void* stream);
size_t sdeng_tilted_eval_workspace_bytes(const sdeng_tilted* desc);

/* Training an energy-based reference: everything the gradient of the energy with respect to the net's parameters needs, in ONE launch --
 * the training instantiation of the kernel behind sdeng_tilted_eval, same walk, same numbers.  The trainer's loss (MaximumLikelihoodEBM.train,
 * additions/ebm_mle.py:735-771) is a function of E_r = net.energy(t_r, x_r) over detached rows; the prior has no parameters, so with the
 * quantities of sdeng_tilted_eval (models/reparam.py:426-451)
 *     E_r = -prior_lp_r + f_r <v_r, xs_r>,   dE_r/dtheta = f_r (backward pass of the net with cotangent xs_r)
 * -- the backward pass J^T xs of sdeng_tilted_eval, whose pre-activation cotangents dh_4 .. dh_0 are written out here instead of dropped.
 * Per row (row-major arrays, row r as in sdeng_tilted):
 *     a[l]  [M,128]  gelu(h_l), l = 0..4            d[l]  [M,128]  f_r dh_l,  dh_4 = (W_out^T xs) . gelu'(h_4),  dh_l = (W_{l+1}^T dh_{l+1}) . gelu'(h_l)
 *     xs    [M,d]    the scaled state               dv    [M,d]    f_r xs, the cotangent of v
 * With c_r = dL/dE_r (the caller's: the kernel knows no loss) the gradients are outer products over the rows, left to the caller as for
 * sdeng_ctrl_vjp:  dW_out = (c dv)^T a[4],  dW_l = (c d[l])^T a[l-1] (l = 1..4),  dW_in = (c d[0])^T xs,  biases the column sums, and the
 * time embedding takes sum_b c d[0] per time as the cotangent of TimeEmbed(t).
 * desc->log_prob and desc->grad are written as by sdeng_tilted_eval and are each optional here (both may be NULL).  Errors: those of
 * sdeng_tilted_eval, and SDENG_E_INVALID for a null `rows` or a null pointer in it (sdeng_last_error names the array).  Workspace: that of
 * an evaluation with grad (the pre-activations are always kept); SDENG_FLAG_REUSE_PACK as for sdeng_tilted_eval -- the packed images of
 * the two entry points are the same. */
typedef struct sdeng_tilted_rows { float *a[5], *d[5]; float *xs, *dv; } sdeng_tilted_rows;
int sdeng_tilted_vjp(const sdeng_tilted* desc, const sdeng_tilted_rows* rows, void* stream);
size_t sdeng_tilted_vjp_workspace_bytes(const sdeng_tilted* desc);

/* Annealed samplers over an energy-based reference: n_moves Langevin moves of M chains in ONE launch -- mala_step / ula_step of
 * additions/mcmc.py:77-135, 189-221 with the per-chain step-size heuristic of :55-74 (target_acceptance > 0), exactly the moves of
 * sdeng_langevin_moves, with the density of sdeng_tilted_eval at every proposal: what re_sampler does swap_frequency - 1 times between two
 * swap steps, smc_sampler n_warmup + n_mcmc times per level and MaximumLikelihoodEBM.cd_sampling from the positives
 * (additions/ebm_mle.py:120-160, 340-380, 440-446, 505-540), one sdeng_tilted_eval launch and a dozen small host kernels per move.
 * `desc` carries the net, the prior and the row-to-time layout (M, n_times, rows_per_time, tinfo: chain r moves at time r / rows_per_time;
 * n_times = M, rows_per_time = 1 gives every chain its own time), the workspace and SDENG_FLAG_REUSE_PACK; its x, log_prob and grad are
 * ignored.  State in / out: x [M,d], lp [M] = log_prob at x, grad [M,d] = its score, step [M].  Per move and chain:
 *     prop = sqrt(2 step) z + (x + step grad);   (lp', grad') = sdeng_tilted_eval at (t, prop);
 *     log_acc = (lp' + |prop - x - step grad|^2 / (4 step)) - (lp + |x - prop - step grad'|^2 / (4 step));  accepted iff log(u) < log_acc
 * (a NaN lp' is a rejection: the chain keeps its state; the unadjusted move accepts always and reads no u), then the step heuristic.
 * The time embedding of the net depends on the chain's time alone and is computed once per launch, not per move.
 * Noise: injected normals z [n_moves,M,d] and uniforms u [n_moves,M], both or neither (unadjusted: z alone) -- or NULL: Philox stream 8
 * for the normals (the counter layout of the step noise, keyed by (seed, chain0 + chain, move): sdeng_philox_normal_steps(...,
 * stream_id = 8) replays them) and stream 9 for the uniforms (counter (chain0 + chain, 0, move, 9), output word 0).  Streams 0-7 are taken.
 * samples (optional) [n_moves - keep_from, M, d], acc_sum (optional) [M], acc_last (optional) [M]: as sdeng_langevin_moves.
 * Errors, all before any launch: SDENG_E_INVALID for what sdeng_tilted_eval rejects in the descriptor (but its three ignored pointers), a
 * null `mv` or state pointer, n_moves < 0, keep_from outside [0, n_moves], exactly one of z / u for an adjusted move; SDENG_E_UNSUPPORTED
 * as sdeng_tilted_eval; SDENG_E_WORKSPACE.  Workspace (sdeng_tilted_moves_workspace_bytes): the packed images where sdeng_tilted_eval
 * keeps them (every tilted entry point shares them), per-wave slots of six layers (the five pre-activations and the time embedding), then
 * the proposal and proposal-score rows, 2 x [M,d]. */
typedef struct sdeng_tilted_moves_state {
  int32_t n_moves, keep_from, unadjusted, reserved;
  float target_acceptance;          /* <= 0: steps stay fixed */
  float *x, *lp, *grad, *step;      /* [M,d], [M], [M,d], [M]: in and out */
  const float *z, *u;               /* injected noise or NULL (Philox 8 / 9) */
  uint64_t seed; int64_t chain0;
  float *samples, *acc_sum, *acc_last;   /* optional, as sdeng_langevin_moves */
} sdeng_tilted_moves_state;
int sdeng_tilted_moves(const sdeng_tilted* desc, const sdeng_tilted_moves_state* mv, void* stream);
size_t sdeng_tilted_moves_workspace_bytes(const sdeng_tilted* desc);

/* RDS over an energy-based reference (ref_type 'nn', solver/oc.py:577-592): one whole simulate() loop of EIReferenceSDELoss /
 * DDPMLikeReferenceSDELoss (SDENG_FORM_LIN; losses/oc.py:444-510, :584-651, eq/sdes.py:532-555) or EMReferenceSDELoss (SDENG_FORM_EM;
 * losses/oc.py:218-296) whose reference_ctrl is the score net(t, x) of a tilted potential (models/reparam.py:478-482) -- in the reference one
 * autograd pass through the 6 x 128 net per step, here all N steps in ONE launch (and one small launch ahead of it for the time embeddings
 * of the N step times).  Per step k, with the row coef[k] of the table above and the density of sdeng_tilted_eval:
 *     ref = grad log p_ref(t_k, x_k)      t_k = tinfo[k][0] (the caller passes the times of coef[k][0]); the score of sdeng_tilted_eval at that
 *                                         row, bit for bit (the kernel calls the same walk)
 *     u   = clip(FourierMLP(t_k, x_k), clip_model)      ClippedCtrl, models/reparam.py:33-43, models/mlp.py:99-143
 *     z   = noise_in[k], or the Philox normals of stream 0 with counter (particle0 + p, feature/4, k, 0): sdeng_philox_normal_steps replays them
 *     then the update and the running cost of SDENG_FORM_LIN / SDENG_FORM_EM exactly as sdeng_simulate forms them (the Ito term with SDENG_FLAG_ITO).
 * `ref` carries the net, the prior, d, M = the B particles of this shard, n_times = N, tinfo [N][5] at the step times, the workspace and
 * SDENG_FLAG_REUSE_PACK; its rows_per_time, x, log_prob and grad are ignored.  Terminal costs are NOT added: the caller adds log p_ref(x_N)
 * (sdeng_tilted_eval at eps: WrapperDistrNN.log_prob, distr/base.py:186-198) and -log pi~(x_N) (sdeng_dist_eval) to rnd_out
 * (losses/oc.py:290, :505, :645).  No Philox stream is taken beyond stream 0.
 * Errors, all before any launch: SDENG_E_INVALID for what sdeng_tilted_eval rejects in `ref` (but its ignored fields), a null `run`, a
 * null coef / x_in / x_out / rnd_out, N < 1 or N != ref->n_times, a malformed drift net; SDENG_E_UNSUPPORTED (reason in
 * sdeng_last_error) as sdeng_tilted_eval, for a control other than ClippedCtrl, a form other than LIN / EM and any flag but
 * SDENG_FLAG_ITO (REMOVE_REF, CTRL_NOISE, CTRL_DROPOUT and SPLIT_TILES are named); SDENG_E_WORKSPACE.
 * Workspace (sdeng_tilted_simulate_workspace_bytes): the packed images where sdeng_tilted_eval keeps them (the four entry points share
 * them), the per-wave pre-activations, the packed drift net and its N time embeddings, the EBM's N time embeddings [N][128], the score
 * rows [B,d] and two state rows [B,d] (used without xs_out). */
typedef struct sdeng_tilted_rds {
  int32_t form;             /* SDENG_FORM_LIN or SDENG_FORM_EM                                       */
  uint32_t flags;           /* SDENG_FLAG_ITO or 0                                                   */
  int32_t N;                /* steps (= ref->n_times)                                                */
  int32_t reserved;
  const float* coef;        /* [N][SDENG_NCOEF]                                                      */
  sdeng_net net;            /* the drift net, ctrl_kind SDENG_CTRL_CLIPPED                           */
  uint64_t seed;            /* Philox key                                                            */
  int64_t particle0;        /* global index of this shard's first particle                           */
  const float* x_in;        /* [B,d]                                                                 */
  const float* noise_in;    /* [N,B,d] or NULL                                                       */
  float *x_out, *rnd_out;   /* [B,d], [B]                                                            */
  float* xs_out;            /* [N+1,B,d] or NULL                                                     */
  float* ref_out;           /* [N,B,d] or NULL: the reference score the kernel used at every step (for tests) */
} sdeng_tilted_rds;
int sdeng_tilted_simulate(const sdeng_tilted* ref, const sdeng_tilted_rds* run, void* stream);
size_t sdeng_tilted_simulate_workspace_bytes(const sdeng_tilted* ref, const sdeng_tilted_rds* run);

#ifdef __cplusplus
}
#endif
#endif /* SDENG_H */
