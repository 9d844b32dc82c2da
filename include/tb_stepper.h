/*
 * tb_stepper.h -- C ABI of the MI355X-native batched physics stepper for the
 * SwingRacket-v0 / Tennisbot-v0 environments of youliangtan/tennisbot-rl.
 *
 * This is the drop-in boundary. The reference has no FFI of its
 * own: its envs call the third-party `pybullet` C-API from Python. Each entry point
 * below therefore cites the reference call sites (file:line under the reference root)
 * whose work it replaces for a whole batch of N independent worlds.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature. `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream); every call is
 *     asynchronous on that stream unless stated otherwise.
 *   - all `*_dev` pointers are DEVICE pointers owned by the caller (for example
 *     torch tensors' data_ptr()). Layouts are row-major: actions [N][A], obs [N][O].
 *   - return value: 0 = OK, negative = TB_E_* below, positive = a hipError_t.
 *     Nothing throws across this boundary. tb_last_error() gives a thread-local
 *     message for the last non-zero return on the calling thread.
 *   - a handle is bound to one device and is not re-entrant.
 *   - there is NO CPU fallback in this library: without a usable HIP device
 *     tb_create fails.
 */
#ifndef TB_STEPPER_H
#define TB_STEPPER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TB_ABI_VERSION 4

/* library error codes (negative); positive return values are hipError_t */
#define TB_OK 0
#define TB_E_INVAL (-1)    /* bad argument (null pointer, n_envs <= 0, unknown env kind, ...) */
#define TB_E_NODEVICE (-2) /* no usable HIP device / device index out of range */
#define TB_E_PARAMS (-3)   /* TbParams failed validation (n_hull, dt, masses, ...) */
#define TB_E_UNSUPPORTED (-4)
#define TB_E_TIMEOUT (-5)    /* tb_mark_host_wait: the mark did not fire in time */

/* env kinds: tennisbot/__init__.py:3-11 registers exactly these two ids */
#define TB_ENV_SWING 0  /* SwingRacket-v0 -> tennisbot/envs/swingracket_env.py */
#define TB_ENV_TENNIS 1 /* Tennisbot-v0   -> tennisbot/envs/tennisbot_env.py   */

#define TB_SWING_ACT_DIM 6  /* swingracket_env.py:29-31 */
#define TB_SWING_OBS_DIM 6  /* swingracket_env.py:34-39,143-144 */
#define TB_TENNIS_ACT_DIM 2 /* tennisbot_env.py:43-44 */
#define TB_TENNIS_OBS_DIM 12 /* tennisbot_env.py:52-55,134-136 */

/* persistent state, structure-of-arrays: 32-bit words [TB_*_WORDS][N] + one byte [N] */
#define TB_SWING_WORDS 30
#define TB_TENNIS_WORDS 28
/* rows shared by both envs */
#define TB_W_RP 0   /* racket COM position (3)  racket.py:131 returns the COM frame */
#define TB_W_RQ 3   /* racket orientation quaternion x,y,z,w (4) */
#define TB_W_RV 7   /* racket linear velocity (3)  racket.py:142 */
#define TB_W_RW 10  /* racket angular velocity, world frame (3) */
#define TB_W_BP 13  /* ball position (3)  objects.py:57 */
#define TB_W_BV 16  /* ball linear velocity (3)  objects.py:64 */
#define TB_W_BW 19  /* ball angular velocity (3) */
/* SwingRacket-v0 rows */
#define TB_W_SW_GOAL 22   /* goal x,y (2)             swingracket_env.py:173 */
#define TB_W_SW_SPAWN 24  /* racket LINK spawn pos (3) swingracket_env.py:168 */
#define TB_W_SW_D0 27     /* initial_dist_to_goal      swingracket_env.py:174-175 */
#define TB_W_SW_STEP 28   /* step_count (int32)        swingracket_env.py:83,108 */
#define TB_W_SW_EPISODE 29 /* episode index (uint32), keys the reset RNG */
/* Tennisbot-v0 rows */
#define TB_W_TN_SHOOT 22  /* ball_shoot_force (3)      tennisbot_env.py:237-241 */
#define TB_W_TN_SCALE 25  /* racket globalScaling this episode was built with  tennisbot_env.py:230-234 */
#define TB_W_TN_STEP 26   /* step_count (int32)        tennisbot_env.py:122 */
#define TB_W_TN_EPISODE 27

/* done byte: 0 running; 1 done, and (Swing) the restoring force issued at the end
 * of the last fast-forward substep (swingracket_env.py:135-141) is still pending in
 * the engine's force accumulator; 2 done, nothing pending. */
#define TB_DONE_NO 0
#define TB_DONE_PENDING_FORCE 1
#define TB_DONE_YES 2

/* TbParams.flags */
#define TB_F_AUTO_RESET 0x1u          /* VecEnv semantics: a done env is reset inside the step */
#define TB_F_NET 0x2u                 /* court.urdf:43-47 second collision box */
#define TB_F_RACKET_BALL 0x4u         /* racket<->ball narrowphase + impulse; clear = BASELINE configs[1] "no ball contact" bench mode */
#define TB_F_RACKET_GROUND 0x8u       /* racket<->court-ground contact (court.urdf:19-24): a persistent manifold of
                                       * up to 4 hull vertices per env, one support point added per substep, warm-started rows
                                       * (DESIGN.md section 3). Opt-in. The reference's court does collide with the racket, and in
                                       * the SwingRacket fast-forward the racket is not gravity-compensated: it lands. What keeps
                                       * the flag out of the default is not the contact's own cost any more but the episodes it
                                       * creates: 0.08 % of random-action envs end with the ball at rest on the grounded racket and
                                       * run to the 800-substep limit (776 substeps of stacked resting contact, >= 6 us each, one
                                       * lane) -- at 4096 envs that is nearly every episode end of the batch, i.e. >= 4 ms behind
                                       * every rollout's join (the rollout itself takes 6.5 ms); rewards are not affected
                                       * (DESIGN.md section 3 has the measured distributions) */
#define TB_F_DEFAULT (TB_F_NET | TB_F_RACKET_BALL)

#define TB_MAX_HULL 64
#define TB_HULL_REC 8 /* floats per hull edge record */

/*
 * Scene + engine parameters. Every engine-semantics value recalled from Bullet
 *  is a named field so a host that has pybullet can calibrate.
 * All derived values (inverses, edge records) are computed once by the host side in
 * float64, rounded to float32 and consumed as given by the kernels.
 */
typedef struct TbParams {
  /* engine (Appendix B.1/B.2) */
  float dt;                 /* 1/240, racket.py:24 */
  float inv_dt;             /* 240 */
  float gravity;            /* 9.81, swingracket_env.py:154 setGravity(0,0,-9.81) */
  float lin_damp;           /* k1 = 0.04 of the damping force -m v (k1 + k2 |v|) */
  float ang_damp;           /* 0.04, the same form on the angular momentum */
  float lin_damp_quad;      /* k2 (ABI v4). Bullet's multibody path uses ONE damping value for both terms (k1 = k2 = 0.04): a field of its
                             * own so that the speed-proportional term can be switched off on its own (profiles/r03_pin_sensitivity.md) */
  float ang_damp_quad;
  float max_ang_step;       /* pi/4 per substep rotation clamp */
  float rest_vel_threshold; /* 0.2 m/s: below it restitution is 0 */
  float erp;                /* contact ERP (Baumgarte): 0.08 = PyBullet's world default (Bullet's library default is 0.2) */
  float contact_threshold;  /* 0.02 * ball radius: manifold keeps points closer than this */
  int32_t solver_iters;     /* sequential-impulse iteration cap (Bullet default 50) */
  float solver_tol;         /* stop early once every impulse update of a sweep is <= tol * |impulse|
                             * (float32 PGS otherwise oscillates by a few ulp and always runs to the cap) */
  uint32_t flags;           /* TB_F_* */
  /* racket: racket.urdf:17-21, racket.py:43-45 */
  float racket_mass, racket_inv_mass;
  float racket_inertia[3], racket_inv_inertia[3]; /* body-frame diagonal at scale 1; default: derived from the collision shape as Bullet does */
  float racket_com[3];       /* inertial origin in the link frame, at scale 1 */
  float racket_half_thick;   /* at scale 1 */
  float hull_margin;         /* URDF convex-hull collision margin, 0.001 (not scaled) */
  float hull_bound_radius;   /* max distance COM -> hull vertex at scale 1, for the cull */
  float racket_scale;        /* tennisbot_env.py:213-215: the globalScaling an env's racket is rebuilt
                              * with at its NEXT reset (tennisbot_env.py:230-234); each Tennisbot env
                              * keeps the scale of its current episode in its own state word */
  /* ball: ball.urdf:11-15,27-32, objects.py:48-50,67-72 */
  float ball_mass, ball_inv_mass, ball_inv_inertia, ball_radius;
  float magnus_k;            /* F = k (w x v); 0 reproduces the reference (BASELINE configs[4] extension) */
  float ball_spin_max;       /* reset: w0 ~ U(-max, max)^3; 0 reproduces the reference */
  /* pair coefficients: product rule, objects.py:16-18,29-31,48-50; goal keeps defaults */
  float rest_racket, rest_court, rest_goal;
  float fric_racket, fric_court, fric_goal;
  /* rolling friction of a ball contact (racket.py:43-45, objects.py:29-31,48-50 set rollingFriction .001):
   * combined coefficient of the pair, Bullet's rule rolling_a * friction_b + rolling_b * friction_a
   * (4e-4 with the racket and the court, 5e-4 with the goal: params.reference_rolling_friction()).
   * > 0 adds two angular rows per ball contact, along the friction directions, each boxed by
   * roll * j_n, solved between the normal and the sliding-friction rows. 0 (default) = no such rows:
   * whether Bullet's multibody solver visits them in PyBullet's default solver mode is not known here */
  float roll_racket, roll_court, roll_goal;
  /* racket <-> court (TB_F_RACKET_GROUND): product rule again (0.81, 0.04); manifold threshold
   * 0.02 * the racket's bounding radius at scale 1 (Bullet: 0.02 * angular motion disc) */
  float rest_racket_court, fric_racket_court, racket_ground_threshold;
  /* statics: court.urdf:19-24,43-47; simplegoal.urdf:17-22 (origins inside <geometry> are ignored) */
  float ground_half[3];
  float net_half[3];
  float goal_radius, goal_half_len;
  /* racket collision outline: CCW convex polygon in the COM frame (y, z), at scale 1.
   * record i = { a.y, a.z, e.y, e.z, 1/|e|^2, 1/|e|, 0, 0 } with e = v[i+1] - v[i] */
  int32_t n_hull;
  float hull_edges[TB_MAX_HULL][TB_HULL_REC];
} TbParams;

typedef struct TbHandle TbHandle;

/*
 * Kernel-selection options (since ABI v3; they replace the TB_BLOCK / TB_TENNIS_REG_ROWS / TB_SWING_REG_ROWS
 * environment variables of v2; v4 names the former `reserved` field and changes the policy blob's fragment order; `ff_seal` was appended
 * within v4: `struct_size` tells the library whether a caller has it, and an older caller gets the automatic choice). Every field: 0 = let the library choose from the batch size. None of
 * them changes any result -- the variants are bit-identical (tests/test_gpu_parity.py runs them all) --
 * only which instantiation of the same arithmetic is launched.
 */
typedef struct TbOptions {
  uint32_t struct_size;     /* sizeof(TbOptions): lets a newer library read an older caller's struct */
  int32_t block;            /* threads per workgroup of the step kernels: 64, 128 or 256 (auto: 64 up to 16384 envs, above that 128; 64 for SwingRacket-v0 between 49152 and 131072 envs) */
  int32_t tennis_reg_rows;  /* accepted and ignored (was: an opt-out, -1, that moved the Tennisbot step kernels' static contact rows from
                             * registers to LDS, which never changed a result and no default chose) */
  int32_t swing_reg_rows;   /* accepted and ignored (was: the same for the pipelined SwingRacket one-step kernel; -1 also turned its
                             * two-wave form off) */
  int32_t ff_lanes_per_wave; /* parked envs per wave in the first fast-forward phase, 1..64 (auto: 64 from 4096 envs on, fewer below) */
  int32_t ff_sort;          /* accepted and ignored (was: an opt-in sort of the parked envs by flight estimate, which never changed a
                             * result and no measured workload won with) */
  int32_t ff_phases;        /* the fast-forward as 1, 2 or 3 kernels: budgeted loop, then its compacted survivors (auto: 3 from 262144 envs on, else 1; from 131072 envs on the first of several also hands over every env whose ball reaches the racket) */
  int32_t ff_defer;         /* deferred fast-forwards (SwingRacket-v0 pipeline, up to 131072 envs). A fast-forward kernel lasts as long as its
                             * slowest env, at most four run at once (one per hardware queue), and every one is a FORK in a replayed graph that
                             * moves the chain of steps to another queue. 2: every episode end is parked straight into a pool (up to 64 episodes
                             * between two joins) and ONE launch runs all of them to their end when the caller joins (tb_flush and every call
                             * that flushes): the rollout is a single chain of step kernels. 1: each episode keeps its own fast-forward kernel,
                             * but an env still running after its ballistic flight estimate (capped at an un-struck ball's) + ff_defer_margin
                             * substeps moves on to the pool. -1: off. 0 = auto: 2 up to 16384 envs (4096 envs: 679 -> 871 M env steps/s; with
                             * racket<->court contact 92 -> 115-127 M), above that 1 with TB_F_RACKET_GROUND, else off (large batches run their
                             * fast-forwards beside the steps, in phases). Results do not change; terminal rewards are complete after the join,
                             * as with every pipelined path. Progress marks (a mark promises final steps): an explicit 2 gives the episodes parked since
                             * the previous mark their launch at tb_mark_record, on a side stream; auto and 1 fall back to one kernel per episode
                             * end while marks are enabled (measured: faster beside the chunks' all-gathers). Neither form is used for steps that
                             * ask for terminal-observation / substep outputs. */
  int32_t ff_defer_margin;  /* substeps beyond the estimate before an env is deferred (auto: 16) */
  int32_t policy_slices;    /* tb_policy_rollout: 16-env slices per workgroup, 1 (three waves per 16 envs) or 3 (seven waves per 48 envs) (auto: 1 up to 4096 envs) */
  int32_t ff_seal;          /* the pool's sealed-fate exit: 1 / 0 on (auto), -1 off. A SwingRacket-v0 flight whose ball has fallen below the court,
                             * out of the racket's reach for good, can only end in the 800-substep timeout with reward 0
                             * (swingracket_env.py:127-128); with auto-reset nothing else of it is ever read, so the pool books the remaining
                             * substeps (counters[6], substeps and timeouts are those of the full flight) instead of running them. Every
                             * result is the one the full flight gives (the oracle has no such exit and the parity tests compare against
                             * it); the pool's waves stop paying ~400 substeps for one such ball (a trained policy's collect: +5-8 %).
                             * Only without the Magnus extension and the extended contact set, with parameters inside the limits the
                             * argument needs (tb_kernels.hpp, fate_sealed), and never for launches that write terminal observations.
                             * tb_sealed_substeps reports how many substeps were booked this way. */
  int32_t step_waves;       /* waves per 64 envs of the pipelined SwingRacket-v0 one-step kernel: 0 = auto (2 up to 16384 envs, where most
                             * SIMDs are idle, else 1), 1, or 2 (the racket's update on one wave, the ball's on the other,
                             * for launches where no env nears a contact or ends its short steps). tb_step_waves reports the choice. (Appended after ABI v4's fields: an older caller's shorter struct reads as auto.) */
} TbOptions;

/* library identity / shape queries (host only, no device touched) */
int tb_abi_version(void);
int tb_obs_dim(int env_kind);
int tb_act_dim(int env_kind);
int tb_state_words(int env_kind);
const char *tb_last_error(void);

/*
 * Create a batch of n_envs independent worlds on `device`.
 * Replaces, per world: p.connect (swingracket_env.py:44-47, tennisbot_env.py:65-68),
 * and the one-time part of every loadURDF/changeDynamics (racket.py:35-45,
 * objects.py:25-36,43-50,102-104). State is NOT initialised: call tb_reset.
 * seed / env_id_base key the counter-based reset RNG: env i draws from
 * (seed, env_id_base + i, episode_index), so results do not depend on how a
 * global batch is sharded over GPUs.
 */
int tb_create(const TbParams *params, const TbOptions *options_or_null, int env_kind, int n_envs, int device,
              uint64_t seed, uint64_t env_id_base, TbHandle **out);

/* Replaces p.disconnect (swingracket_env.py:189, tennisbot_env.py:291). Synchronous. */
int tb_destroy(TbHandle *h);

/* Replace the parameter block. Takes effect for launches ENQUEUED after it on `stream`. The scalar
 * parameters travel in the kernel-argument block of each launch, so a hipGraph captured earlier keeps
 * the values it was captured with: tb_params_generation() goes up by one on every tb_set_params, and a
 * caller that replays captured steps compares it with the value at capture time and recaptures when it
 * differs (tennisbot_rl_amd.stepper.StepGraph does; a stale replay is refused, never silent). A call that
 * fails (e.g. the pool the new block asks for cannot be allocated) leaves the handle as it was: old
 * parameters, old generation. */
int tb_set_params(TbHandle *h, const TbParams *params, void *stream);
int tb_params_generation(TbHandle *h);
/* set_racket_scale (tennisbot_env.py:213-215; the curriculum callback train.py:164-176 calls it at every
 * rollout start): the globalScaling an env's racket is rebuilt with at ITS next reset. Unlike the rest of
 * TbParams this value is read by the reset code from the device-resident parameter block, not from the
 * kernel arguments: the update is one asynchronous 4-byte copy on `stream`, it does not bump
 * tb_params_generation, and REPLAYS OF GRAPHS CAPTURED EARLIER SEE IT (row f2 under hipGraph replay). */
int tb_set_racket_scale(TbHandle *h, float scale, void *stream);

/*
 * reset(): swingracket_env.py:151-186 / tennisbot_env.py:217-261 for every env i with
 * mask_dev == NULL or mask_dev[i] != 0. Starts a new episode (episode index + 1) and
 * writes the initial observation to obs_dev[i] if obs_dev != NULL.
 */
int tb_reset(TbHandle *h, const uint8_t *mask_dev, float *obs_dev, void *stream);

/*
 * step(action): swingracket_env.py:75-145 / tennisbot_env.py:104-207 for all envs,
 * including every p.stepSimulation() (swingracket_env.py:82,107; tennisbot_env.py:121),
 * the p.getContactPoints queries (swingracket_env.py:99,111,119; tennisbot_env.py:170),
 * Racket.apply_target_action (racket.py:92-100), Ball.apply_force (objects.py:67-72)
 * and the pose/velocity reads (racket.py:124-143, objects.py:52-65).
 *   actions_dev  [N][A] float32 in
 *   obs_dev      [N][O] float32 out
 *   reward_dev   [N]    float32 out
 *   done_dev     [N]    uint8   out (0/1)
 *   terminal_obs_dev [N][O] or NULL: with TB_F_AUTO_RESET, the last observation of an
 *                episode that ended in this step (untouched for other envs)
 *   substeps_dev [N] int32 or NULL: physics substeps executed for env i in this call
 */
int tb_step(TbHandle *h, const float *actions_dev, float *obs_dev, float *reward_dev,
            uint8_t *done_dev, float *terminal_obs_dev, int32_t *substeps_dev, void *stream);

/*
 * T consecutive step() calls in ONE launch with the state kept in registers:
 * actions [T][N][A] in; obs [T][N][O], reward [T][N], done [T][N] out; substeps_total
 * [N] int32 or NULL. Requires TB_F_AUTO_RESET. Same results as T calls of tb_step.
 * With the pipeline on (tb_set_pipeline), lockstep episodes and substeps_total_dev == NULL, the T steps
 * are issued as launches that end where the episodes end (<= 26 steps each), each followed by its
 * fast-forward on a side stream; the rewards of those terminal steps are then complete after tb_flush.
 */
int tb_rollout(TbHandle *h, int n_steps, const float *actions_dev, float *obs_dev,
               float *reward_dev, uint8_t *done_dev, int32_t *substeps_total_dev, void *stream);

/*
 * n_steps consecutive tb_step calls issued from one host call: step t reads actions at
 * actions_dev + t * actions_stride (bytes) and writes obs / reward / done at their bases + t * their
 * strides -- e.g. the records of a packed rollout buffer. Same launches, same results and the same
 * pipelining as n_steps calls of tb_step (no terminal_obs / substeps outputs); it only takes the host
 * language's per-call cost out of the loop (a ctypes call costs about as much as the step kernel runs).
 * Strides must keep every row as aligned as tb_step requires.
 */
int tb_step_sequence(TbHandle *h, int n_steps, const float *actions_dev, float *obs_dev, float *reward_dev,
                     uint8_t *done_dev, size_t actions_stride, size_t obs_stride, size_t reward_stride,
                     size_t done_stride, void *stream);

/*
 * step() with the policy inside ("policy inference on device ... so collect never
 * leaves the GPU"): SB3's MlpPolicy as the reference configures it (train_swing.py:80-82: pi = vf =
 * [32, 64, 32], tanh; Tennisbot-v0: SB3's default [64, 64], train.py:104-110), a = mean + exp(log_std)
 * * eps, clipped to the action space before the env sees it, as SB3 does. Per env i:
 *   obs_in_dev [N][O] the observation acted on  ->  actions_dev [N][A] (clipped), raw_actions_dev [N][A],
 *   logp_dev [N] (log-probability of the raw sample), value_dev [N]; then exactly tb_step on those actions.
 * The towers run on the matrix cores in fp32 (v_mfma_f32_16x16x4_f32, 16 envs per wave),
 * one layer's accumulator tile feeding the next layer's operand registers directly; tanh is evaluated
 * as 1 - 2/(exp(2x)+1) on the hardware exp2/rcp units (absolute error < 3e-7).
 * weights_dev: tb_policy_floats(kind) floats, 16-byte aligned, in the fragment order the kernel loads:
 * per tower (pi, then vf) its hidden layers and its head (padded to 16 outputs), each layer as
 *   bias tiles     [ceil(out/16)][4][4]: value (t, g, r) = bias[16t + 4g + r]
 *   weight frags   [ceil(out/16)][chunks][4][16]: value (t, c, g, j) = W[out 16t + j][in k(c, g)]
 * with k(c, g) = 4c + g for the first layer (zero beyond the observation) and k(4u + r, g) = 16u + 4g + r
 * after it (W = torch's nn.Linear.weight, zero beyond `out`); then log_std[A] padded to a multiple of 4.
 * tennisbot_rl_amd/ppo.py pack_policy() is the reference packer. eps is drawn in-kernel from Philox
 * keyed by (noise_seed, global env id, episode, step), so
 * a captured graph draws fresh noise on every replay; deterministic != 0 uses the mean.
 */
int tb_policy_floats(int env_kind);
int tb_policy_step(TbHandle *h, const float *weights_dev, const float *obs_in_dev, float *actions_dev,
                   float *raw_actions_dev, float *logp_dev, float *value_dev, float *obs_dev,
                   float *reward_dev, uint8_t *done_dev, uint64_t noise_seed, int deterministic, void *stream);

/*
 * n_steps of tb_policy_step without a launch boundary between them: whole episodes per launch, the
 * policy's weights resident in registers, the envs' state too; the observation a step produces is the
 * one the next step acts on (obs_in_dev is only read for the first). Output arrays are [n_steps][N][..];
 * step_strides_bytes (or NULL = contiguous) gives the distance in bytes between consecutive steps of
 * {actions, raw_actions, logp, value, obs, reward, done} -- e.g. the record size of a packed rollout
 * buffer; a 0 entry means contiguous for that array. Per env the arithmetic and the noise (keyed by
 * env, episode, step) are those of tb_policy_step: identical results. actions_dev / raw_actions_dev and their
 * step strides must be 8-byte aligned (rows are written two floats at a time). Requires TB_F_AUTO_RESET; on
 * SwingRacket-v0 also tb_set_pipeline(h, 1) and lockstep episodes (the launches end where the episodes
 * end, each followed by its fast-forward on a side stream; terminal rewards complete after tb_flush).
 */
int tb_policy_rollout(TbHandle *h, int n_steps, const float *weights_dev, const float *obs_in_dev,
                      float *actions_dev, float *raw_actions_dev, float *logp_dev, float *value_dev,
                      float *obs_dev, float *reward_dev, uint8_t *done_dev, const size_t *step_strides_bytes,
                      uint64_t noise_seed, int deterministic, void *stream);

/*
 * The network of the fused policy. TB_NET_DEFAULT: the env kind's own (above). TB_NET_TUNED, Tennisbot-v0 only: the
 * reference's `train.py -s tuned_ppo` (train.py:54-67,112-127) -- a ReLU features extractor 12 -> 64 -> A shared by actor and
 * critic (A = 2, the action dimension), then ReLU towers pi = vf = A -> 32 -> 64 -> 32 with the usual heads and a state-independent log_std; ReLU is exact
 * (0 for z <= 0, a NaN kept). The net is an argument of the call, not a state of the handle: calls with either net may follow
 * each other on one handle, and a captured launch keeps the net it was captured with. Any other (kind, net) pair is refused
 * with TB_E_PARAMS before anything is launched.
 * Blob (tb_policy_blob_floats(kind, net) floats; for TB_NET_DEFAULT the layout and the length of tb_policy_floats): the
 * extractor's two layers, the pi tower with its head, the vf tower with its head, log_std padded to 4 -- every layer in the
 * bias-tile / weight-fragment format above. The extractor's second layer and the heads are padded to 16 outputs with zeros;
 * the towers' first layer takes the A-wide feature as a 16-wide input (k(4u + r, g) = 16u + 4g + r, zero for k >= A).
 * tb_policy_step_net / tb_policy_rollout_net: tb_policy_step / tb_policy_rollout with that network; sampling, noise keys,
 * clipping, episode ends and every output are theirs. The un-suffixed names are the TB_NET_DEFAULT calls.
 * TB_NET_MLP64, SwingRacket-v0 only: SB3's MlpPolicy default, pi = vf = [64, 64] tanh (6 -> 64 -> 64 -> 6 and -> 1), what the
 * reference's `train_swing.py -s trpo` trains (train_swing.py:101-102). Blob: 11560 floats in TB_NET_DEFAULT's layout -- pi
 * tower, vf tower, log_std padded to 8; the first layer has two k-chunks (O = 6 padded to 8). On Tennisbot-v0 TB_NET_DEFAULT
 * already is that architecture, so (TB_ENV_TENNIS, TB_NET_MLP64) is refused like every other unbuilt pair.
 */
enum { TB_NET_DEFAULT = 0, TB_NET_TUNED = 1, TB_NET_MLP64 = 2 };
int tb_policy_blob_floats(int env_kind, int net);
int tb_policy_step_net(TbHandle *h, int net, const float *weights_dev, const float *obs_in_dev, float *actions_dev,
                       float *raw_actions_dev, float *logp_dev, float *value_dev, float *obs_dev,
                       float *reward_dev, uint8_t *done_dev, uint64_t noise_seed, int deterministic, void *stream);
int tb_policy_rollout_net(TbHandle *h, int net, int n_steps, const float *weights_dev, const float *obs_in_dev,
                          float *actions_dev, float *raw_actions_dev, float *logp_dev, float *value_dev,
                          float *obs_dev, float *reward_dev, uint8_t *done_dev, const size_t *step_strides_bytes,
                          uint64_t noise_seed, int deterministic, void *stream);

/*
 * Evolution-strategies population evaluation: the reference's fitness_static (tennisbot/ES/fitness_functions.py:17-159,
 * evolution_strategy_static.py:25-44) for every env at once, one launch for every env's whole episode. Each env runs one episode
 * with a fresh float64 observation normaliser and its member's GatedCNN (tennisbot/ES/policies.py:59-130) on the last 8
 * normalised observations; action = clip(net, -1, 1) with NaN kept; the return is the float64 sum of the float32 step rewards in
 * step order through the first done.
 *   weights_dev: n_members rows of tb_es_floats(kind) floats in nn.utils.parameters_to_vector order (conv_0.w [8][O][2], conv_0.b,
 *     conv_gate_0.w/b, conv_1.w [12][8][2], conv_1.b, conv_gate_1.w/b, conv_2.w [A][12][2], conv_2.b), weights_stride_floats apart:
 *     a multiple of 4 and >= tb_es_floats(kind); base 16-byte aligned. Env i uses member i / envs_per_member, and
 *     n_members * envs_per_member must equal n_envs.
 *   return_dev [n_envs] doubles, length_dev [n_envs] agent steps (SwingRacket: always 26; Tennisbot: <= 1001).
 * Every call first resets every env exactly as tb_reset(h, NULL, ...) does: env i evaluates the episode whose index is one past
 * the one it was in (on a fresh handle the k-th call, counted from 0 and with no other reset in between, evaluates episode k),
 * and on return every env holds that episode's freshly reset state again (the episode phase is 0). SwingRacket-v0 requires
 * tb_set_pipeline(h, 1) (TB_E_UNSUPPORTED otherwise): the 26th step's fast-forward runs on the pipeline's kernels, and the
 * return is complete in stream order on `stream` when the call returns -- no tb_flush is needed. The trace never changes a result.
 * Counters: episodes finished and substeps are counted by the kernel (no host share).
 */
typedef struct TbEsTrace {
  size_t struct_size;  /* sizeof(TbEsTrace) */
  int max_steps;       /* rows [max_steps][n_envs]; steps beyond are not recorded; rows after an env's last step are not written */
  float *net_in;       /* [T][N][O] the normalised float32 row the network appended at step t (the newest of the 8 it saw) */
  float *obs;          /* [T][N][O] the observation that row was normalised from: the reset observation at t = 0, else step t-1's */
  float *actions;      /* [T][N][A] the clipped action step t was taken with */
  float *raw;          /* [T][N][A] the network's output before the clip */
  float *reward;       /* [T][N] step t's float32 reward (SwingRacket's step 25: the fast-forward's terminal reward) */
  uint8_t *done;       /* [T][N] */
} TbEsTrace;
int tb_es_floats(int env_kind); /* GatedCNN parameters: 766 (SwingRacket-v0) / 858 (Tennisbot-v0) */
int tb_es_evaluate(TbHandle *h, const float *weights_dev, int n_members, size_t weights_stride_floats, int envs_per_member,
                   double *return_dev, int32_t *length_dev, const TbEsTrace *trace_or_null, void *stream);

/*
 * Whole-episode evaluation of the fused policy: one launch runs every env's whole episode with the network of
 * tb_policy_step_net inside (csrc/tb_kernels.hpp, tb_policy_evaluate_kernel: 16 envs per two-wave workgroup, only the pi tower).
 *   weights_dev: the tb_policy_blob_floats(kind, net) blob of pack_policy, 16-byte aligned.
 *   Sampling, noise keys (noise_seed, global env id, episode, step) and clipping are tb_policy_step_net's; deterministic != 0
 *     acts on the mean. Per env, the actions are bit for bit those tb_policy_step_net would have produced, step after step.
 *   return_dev [n_envs] doubles: the float64 sum of the float32 step rewards in step order through the first done;
 *   length_dev [n_envs]: the episode length in agent steps (SwingRacket: always 26; Tennisbot: <= 1001).
 * Every call first resets every env exactly as tb_reset(h, NULL, ...) does: env i evaluates the episode whose index is one past
 * the one it was in (on a fresh handle the k-th call, counted from 0 and with no other reset in between, evaluates episode k),
 * and on return every env holds that episode's freshly reset state again (the episode phase is 0): no state word is written.
 * SwingRacket-v0 requires tb_set_pipeline(h, 1) (TB_E_UNSUPPORTED otherwise): the 26th step's fast-forward runs on the
 * pipeline's kernels. Both results are complete in stream order on `stream` when the call returns -- no tb_flush is needed.
 * Null arguments: TB_E_INVAL; a (kind, net) pair that is not built: TB_E_PARAMS; nothing is launched on a refusal.
 * Counters: episodes finished and substeps are counted by the kernel (no host share).
 */
int tb_policy_evaluate(TbHandle *h, int net, const float *weights_dev, double *return_dev, int32_t *length_dev,
                       uint64_t noise_seed, int deterministic, void *stream);

/*
 * tb_policy_evaluate for a POPULATION of networks, one launch (csrc/tb_kernels.hpp, tb_policy_evaluate_members_kernel): a
 * checkpoint tournament, or the population of an evolution strategy on the MlpPolicy actor. A workgroup still owns 16 envs; they
 * all belong to one member, whose blob its tower wave keeps in registers -- 16 envs against one weight fragment on the matrix cores.
 *   weights_dev: n_members blobs of tb_policy_blob_floats(kind, net) floats in pack_policy's layout, weights_stride_floats apart:
 *     a multiple of 4 and >= the blob length; the base 16-byte aligned. Floats between the end of a blob and the next row are
 *     never read. Env i uses member i / envs_per_member; n_members * envs_per_member must equal n_envs, and envs_per_member
 *     must be a multiple of tb_policy_member_granule() (16: the envs of a tower wave).
 * Everything else is tb_policy_evaluate's contract: the call resets first (call k is episode k), return_dev [n_envs] is the float64
 * sum of the float32 rewards in step order through the first done, length_dev [n_envs] the episode length in agent steps; no state
 * word is written and the phase is 0 on return; SwingRacket-v0 needs tb_set_pipeline(h, 1) (TB_E_UNSUPPORTED otherwise) and its
 * terminal reward is folded in behind the flush; the kernel counts its counters; results are complete in stream order. Per env, the
 * actions are bit for bit those of tb_policy_step_net with that member's blob, and log_std is that member's -- so row m equals
 * tb_policy_evaluate with blob m on a handle of envs_per_member envs whose env_id_base is this handle's + m * envs_per_member.
 * Null h / weights_dev / return_dev / length_dev, n_members < 1, envs_per_member < 1 or not a multiple of the granule, a
 * product other than n_envs, a stride below the blob length or not a multiple of 4, a misaligned base: TB_E_INVAL; a (kind, net)
 * pair that is not built: TB_E_PARAMS. A refusal launches, resets and writes nothing.
 */
int tb_policy_member_granule(void);
int tb_policy_evaluate_members(TbHandle *h, int net, const float *weights_dev, int n_members, size_t weights_stride_floats,
                               int envs_per_member, double *return_dev, int32_t *length_dev, uint64_t noise_seed,
                               int deterministic, void *stream);

/*
 * tb_policy_rollout_net for a POPULATION of networks (csrc/tb_kernels.hpp, tb_policy_rollout_kernel's members form): the collect of
 * a population of PPO learners, one launch per episode cut whatever the population's size. Everything is tb_policy_rollout_net's:
 * arrays [n_steps][N][..], step strides, alignment, TB_F_AUTO_RESET and, on SwingRacket-v0, the pipeline and lockstep. The weights
 * are tb_policy_evaluate_members': n_members blobs weights_stride_floats apart (a multiple of 4, >= the blob length, base 16-byte
 * aligned; floats between blobs are never read), env i uses member i / envs_per_member, envs_per_member a multiple of
 * tb_policy_member_granule(), n_members * envs_per_member == n_envs. The member belongs to a SLICE of 16 envs: at 48 envs per
 * workgroup the three tower-wave pairs may hold three members' weights. Per env, every output is bit for bit what
 * tb_policy_rollout_net gives with that member's blob on a handle of envs_per_member envs whose env_id_base is this handle's
 * + m * envs_per_member. Refusals: tb_policy_evaluate_members' list and tb_policy_rollout_net's, with the same codes, named after
 * this function; a refusal launches nothing and writes nothing.
 */
int tb_policy_rollout_members(TbHandle *h, int net, int n_steps, const float *weights_dev, int n_members, size_t weights_stride_floats,
                              int envs_per_member, const float *obs_in_dev, float *actions_dev, float *raw_actions_dev, float *logp_dev,
                              float *value_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev, const size_t *step_strides_bytes,
                              uint64_t noise_seed, int deterministic, void *stream);

/*
 * Whole-episode evaluation of a SAC / TQC actor (the two share it): one launch runs every env's whole episode with the
 * 256-wide actor inside (csrc/tb_sac.hpp, tb_sac_evaluate_kernel: 16 envs per four-wave workgroup, weights streamed from L2).
 *   actor_dev: the flat TB_SAC_ACTOR vector, tb_sac_param_floats(kind, TB_SAC_ACTOR) floats, as the learner trains it.
 *   Per step a = tanh(mu + exp(clamp(log_std, -20, 2)) eps) with mu / log_std computed element for element as
 *     tb_sac_actor_forward computes them; eps is tb_policy_step's noise, keyed by (noise_seed, global env id, episode, step);
 *     deterministic != 0 gives eps = 0. A NaN action stays NaN.
 *   return_dev [n_envs] doubles: the float64 sum of the float32 step rewards in step order through the first done;
 *   length_dev [n_envs]: the episode length in agent steps (SwingRacket: always 26; Tennisbot: <= 1001).
 * Every call first resets every env exactly as tb_reset(h, NULL, ...) does: env i evaluates the episode whose index is one past
 * the one it was in (on a fresh handle the k-th call, counted from 0 and with no other reset in between, evaluates episode k),
 * and on return every env holds that episode's freshly reset state again (the episode phase is 0): no state word is written.
 * SwingRacket-v0 requires tb_set_pipeline(h, 1) (TB_E_UNSUPPORTED otherwise): the 26th step's fast-forward runs on the
 * pipeline's kernels. Results are complete in stream order on `stream` when the call returns -- no tb_flush is needed.
 * Null h / actor_dev / return_dev / length_dev, or a trace whose struct_size is not sizeof(TbSacEvalTrace) or with a null
 * array: TB_E_INVAL; nothing is launched on a refusal. The trace never changes a result; rows after an env's last step are
 * not written. Counters: episodes finished and substeps are counted by the kernel (no host share).
 */
typedef struct TbSacEvalTrace {
  size_t struct_size;  /* sizeof(TbSacEvalTrace) */
  int max_steps;       /* rows [max_steps][n_envs]; later steps are not recorded */
  float *obs;          /* [T][N][O] the observation step t acted on (t = 0: the reset's) */
  float *eps;          /* [T][N][A] the noise drawn for step t (0 when deterministic) */
  float *actions;      /* [T][N][A] the squashed action step t was taken with */
  float *reward;       /* [T][N]   (SwingRacket's step 25: the fast-forward's terminal reward) */
  uint8_t *done;       /* [T][N] */
} TbSacEvalTrace;
int tb_sac_evaluate(TbHandle *h, const float *actor_dev, double *return_dev, int32_t *length_dev, uint64_t noise_seed,
                    int deterministic, const TbSacEvalTrace *trace_or_null, void *stream);

/*
 * tb_sac_evaluate for a POPULATION of actors, one launch (csrc/tb_sac.hpp, tb_sac_evaluate_kernel's members form): a tournament of
 * the checkpoints train_sac.py / train_tqc.py write, or the runs of a seed sweep. A workgroup still owns 16 envs; they all belong
 * to one member, whose vector its four waves stream -- 16 envs against one weight fragment on the matrix cores.
 *   actors_dev: n_members flat TB_SAC_ACTOR vectors of tb_sac_param_floats(kind, TB_SAC_ACTOR) floats, actors_stride_floats
 *     apart: a multiple of 4 and >= the vector's length; the base 16-byte aligned. Floats between the end of a vector and the next
 *     row are never read. Env i uses the vector at actors_dev + (i / envs_per_member) * actors_stride_floats;
 *     n_members * envs_per_member must equal n_envs, and envs_per_member must be a multiple of tb_policy_member_granule() (16).
 * Everything else is tb_sac_evaluate's contract: the call resets first (call k is episode k), return_dev / length_dev [n_envs] as
 * there, no state word is written and the phase is 0 on return; SwingRacket-v0 needs tb_set_pipeline(h, 1) (TB_E_UNSUPPORTED
 * otherwise); results are complete in stream order; the optional trace has rows [T][n_envs] and changes no result. Per env, every
 * result and every trace row is bit for bit what tb_sac_evaluate gives with that member's vector on a handle of envs_per_member
 * envs whose env_id_base is this handle's + m * envs_per_member.
 * Null h / actors_dev / return_dev / length_dev, n_members < 1, envs_per_member < 1 or not a multiple of the granule, a product
 * other than n_envs, a stride below the vector's length or not a multiple of 4, a misaligned base, a trace whose struct_size is
 * not sizeof(TbSacEvalTrace) or with a null array: TB_E_INVAL. A refusal launches, resets and writes nothing.
 */
int tb_sac_evaluate_members(TbHandle *h, const float *actors_dev, int n_members, size_t actors_stride_floats, int envs_per_member,
                            double *return_dev, int32_t *length_dev, uint64_t noise_seed, int deterministic,
                            const TbSacEvalTrace *trace_or_null, void *stream);

/*
 * SAC / TQC collect: n_steps agent steps of every env with the 256-wide actor inside, one launch, every transition written as a
 * replay ring stores it (csrc/tb_sac.hpp, tb_sac_collect_kernel: tb_sac_evaluate_kernel's four-wave workgroup and actor stage
 * around tb_policy_rollout's env wave).
 *   Steps and state: every env is stepped n_steps agent steps from the state the handle holds -- no reset. An env that
 *     finishes restarts inside the launch exactly as the step kernels do on done (TB_F_AUTO_RESET is required, TB_E_UNSUPPORTED
 *     otherwise), and the state is written back: on return the handle is where n_steps calls of tb_step with the same actions
 *     would have left it, episode phase included.
 *   mode TB_SAC_COLLECT_ACTOR: a = tanh(mu + exp(clamp(log_std, -20, 2)) eps) with mu / log_std computed element for element
 *     as tb_sac_actor_forward computes them from actor_dev (the flat TB_SAC_ACTOR vector); eps is tb_policy_step's noise, keyed
 *     by (noise_seed, global env id, episode, step). A NaN action stays NaN.
 *   mode TB_SAC_COLLECT_UNIFORM: no actor stage runs and actor_dev may be null. Action k is (float)(w >> 8) * 0x1p-23f - 1.0f,
 *     w being word k % 4 of the Philox block k / 4 that the noise of that (noise_seed, env, episode, step) would have been
 *     made from: exact in float32, range [-1, 1 - 2^-23]. The mode is a kernel argument, the same for the whole grid.
 *   out: rows are plain [S][N] arrays, S = n_steps, no stride and no wrap -- the caller hands in pointers into its ring. All
 *     five arrays are required; eps_or_null is optional and changes no result. obs / next_obs rows must be 16-byte aligned
 *     (SwingRacket-v0: 8), action / eps rows 8-byte aligned.
 *   SwingRacket-v0 needs tb_set_pipeline(h, 1) and episodes in lockstep (TB_E_UNSUPPORTED otherwise, as tb_policy_rollout), and
 *     the launch must stay inside the episode: phase + n_steps <= 26 (TB_E_INVAL otherwise; tb_policy_rollout cuts its launches
 *     there itself, this call leaves the cut to the caller, whose ring rows it writes). A launch that ends the episodes parks
 *     them for the fast-forward, which writes the terminal reward into out->reward's last row itself; the call then flushes on
 *     `stream`: every output, that reward included, is complete in stream order on `stream` when the call returns.
 *   Tennisbot-v0: any n_steps >= 1.
 * Null h / out, a null required array, a struct_size that is not sizeof(TbSacCollectOut), n_steps < 1, an unknown mode, a
 * null actor_dev in actor mode, a misaligned array: TB_E_INVAL. Nothing is launched on a refusal.
 * Counters: as tb_policy_rollout counts them (each step's first substep by the host, the rest and the episodes by the kernel).
 */
enum { TB_SAC_COLLECT_ACTOR = 0, TB_SAC_COLLECT_UNIFORM = 1 };
typedef struct TbSacCollectOut {
  size_t struct_size;   /* sizeof(TbSacCollectOut) */
  float *obs;           /* [S][N][O] the observation step t acted on */
  float *next_obs;      /* [S][N][O] what tb_step would have returned (a done row: the next episode's first observation) */
  float *action;        /* [S][N][A] the action the env was stepped with */
  float *reward;        /* [S][N] */
  float *done;          /* [S][N]   0.0f / 1.0f: the replay ring's type */
  float *eps_or_null;   /* [S][N][A] the noise drawn (0 in uniform mode); optional, changes no result */
} TbSacCollectOut;
int tb_sac_collect(TbHandle *h, const float *actor_dev, int n_steps, int mode, uint64_t noise_seed,
                   const TbSacCollectOut *out, void *stream);

/*
 * The PPO learner (csrc/tb_learner.hpp; tennisbot_rl_amd/learner.py is the caller): GAE, one minibatch's gradient, and the
 * optimiser step, fp32, for the two policy architectures the fused policy kernels are instantiated for. These functions need
 * no env: they take (env_kind, device, stream) instead of a TbHandle, every buffer is caller-owned device memory, and every
 * output is complete in stream order on `stream` when the call returns. Nothing is read or written on the host.
 *
 * Flat parameter order (tb_ppo_param_floats(kind) floats: 9069 SwingRacket-v0, 10181 Tennisbot-v0): the order of
 * build_actor_critic(...).named_parameters() in tennisbot_rl_amd/ppo.py, each tensor row-major as torch holds it
 * (nn.Linear.weight is [out][in]):
 *   log_std [A] | policy_net.{0,2,(4)}.weight, .bias interleaved per layer | value_net_body likewise |
 *   action_net.weight [A][last], .bias [A] | value_net.weight [1][last], .bias [1]
 * The gradient and both Adam moments use the same order. float arrays must be 4-byte aligned, idx_dev and the workspace 8-byte
 * aligned; bad sizes, null or misaligned pointers are refused here (TB_E_INVAL, tb_last_error), before anything is launched.
 *
 * tb_ppo_gae: adv[k] = delta[k] + gamma lambda (1 - done[k]) adv[k+1], delta[k] = r[k] + gamma V[k+1] (1 - done[k]) - V[k],
 * V[T] = last_value; returns = adv + V. One lane per env, one launch. rewards / dones are [T][n] with a distance of
 * *_step_stride_bytes between steps (0 = contiguous; e.g. the record size of a packed rollout buffer); values, adv and returns
 * are contiguous [T][n], last_value [n].
 *
 * tb_ppo_grad: the gradient of the clipped-surrogate loss (advantages normalised with the minibatch's mean and unbiased std,
 * value loss vf_coef * mean squared error; the entropy term is added by tb_ppo_apply) over the rows idx[0 .. batch) of the
 * flat rollout arrays obs [n_rows][O], raw_actions [n_rows][A] (the unclipped samples), old_logp, adv, returns [n_rows].
 * Each workgroup gathers tb_ppo_rows_per_workgroup() consecutive entries of idx itself and leaves partial gradient vectors in
 * the workspace (tb_ppo_workspace_bytes(kind, batch) bytes; its content is only meaningful to tb_ppo_apply). No float atomics:
 * the same inputs give the same bits. batch >= 2; idx values outside [0, n_rows) are clamped.
 *
 * tb_ppo_apply, phases = TB_PPO_REDUCE: grad_dev = the partials summed in a fixed order, minus ent_coef on log_std; stats_dev
 * [3] = policy loss, value loss, entropy of the minibatch. phases = TB_PPO_STEP: grad_dev /= world, then times torch's clip
 * factor min(1, max_grad_norm / (norm + 1e-6)); Adam (bias correction from `step`, the 1-based count of this step) updates
 * params_dev, exp_avg_dev and exp_avg_sq_dev in place. Both bits: the two in turn. With several ranks the caller all-reduces
 * (sums) grad_dev between the two phases; identical grad_dev, parameters and moments give identical bits on every rank.
 * NON-FINITE GRADIENTS: the factor is torch's clamp(r, max = 1) of r = max_grad_norm / (norm + 1e-6), which KEEPS a NaN (r < 1 ?
 * r : (r is NaN ? r : 1); not fminf, which drops it). A norm that is NaN, or inf under an infinite bound (inf / inf), therefore
 * makes every participating slot of grad_dev, of both moments and of the parameters NaN, and an inf norm under a finite bound
 * gives the factor 0 (the inf slot itself: inf * 0 = NaN) -- slot for slot what torch.nn.utils.clip_grad_norm_ followed by
 * torch.optim.Adam leaves. The norm is the float32 rounding of the root of a float64 sum: a root beyond float32's range is inf,
 * although the sum itself is finite. Slots outside the participating ranges (TB_PPO_VALUE_ONLY below) and other members' rows
 * (tb_ppo_apply_members) are untouched, whatever the norm is.
 * TB_PPO_VALUE_ONLY, added to either phase: the critic alone. TB_PPO_REDUCE then writes only the value slots of grad_dev
 * (value_net_body, value_net); TB_PPO_STEP takes its norm over, clips and updates only those slots. The policy slots of the
 * parameters, the gradient and both moments are not written.
 */
#define TB_PPO_REDUCE 1
#define TB_PPO_STEP 2
#define TB_PPO_VALUE_ONLY 4
int tb_ppo_param_floats(int env_kind);
int tb_ppo_rows_per_workgroup(void);
long long tb_ppo_workspace_bytes(int env_kind, int batch);
int tb_ppo_gae(int env_kind, int device, void *stream, int n_steps, int n_envs, const float *rewards_dev,
               size_t reward_step_stride_bytes, const uint8_t *dones_dev, size_t done_step_stride_bytes, const float *values_dev,
               const float *last_value_dev, double gamma, double gae_lambda, float *adv_dev, float *returns_dev);
int tb_ppo_grad(int env_kind, int device, void *stream, const float *obs_dev, const float *raw_actions_dev,
                const float *old_logp_dev, const float *adv_dev, const float *returns_dev, long long n_rows,
                const int64_t *idx_dev, int batch, const float *params_dev, int n_params, float clip_range, float vf_coef,
                void *workspace_dev, size_t workspace_bytes);
int tb_ppo_apply(int env_kind, int device, void *stream, int phases, const void *workspace_dev, size_t workspace_bytes, int batch,
                 float *params_dev, float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev, int n_params, float *stats_dev,
                 float ent_coef, float max_grad_norm, int world, float lr, float beta1, float beta2, float eps, long long step);
/*
 * The same learner for a network given by name (TB_NET_*; the names above are the TB_NET_DEFAULT calls). TB_NET_TUNED
 * (Tennisbot-v0): tb_ppo_param_floats_net = 9639 floats in the order log_std [2] | features extractor W0 [64][12] b0 W1 [2][64]
 * b1 | policy_net W0 [32][2] b0 W1 [64][32] b1 W2 [32][64] b2 | value_net_body, the same | action_net W [2][32] b | value_net
 * W [1][32] b -- named_parameters() of ppo.build_tuned_actor_critic. ReLU' = 0 at z <= 0. Each tower wave differentiates the shared
 * extractor too: a partial vector holds the pi wave's extractor share in the extractor's slots and the vf wave's in a second
 * region, and TB_PPO_REDUCE adds the two float64 sums (pi's first), so the result is as reproducible as the default nets'.
 * TB_PPO_VALUE_ONLY is refused for it (TB_E_UNSUPPORTED): the extractor is shared, there is no critic-only slot range.
 * TB_NET_MLP64 (SwingRacket-v0): 9677 floats in the order of the default nets, log_std [6] | policy_net W0 [64][6] b0 W1 [64][64]
 * b1 | value_net_body, the same | action_net W [6][64] b | value_net W [1][64] b -- named_parameters() of
 * ppo.build_actor_critic(6, 6, (64, 64)). The towers are separate: TB_PPO_VALUE_ONLY is offered.
 * tb_ppo_gae does not depend on the network. Other (kind, net) pairs: TB_E_PARAMS.
 */
int tb_ppo_param_floats_net(int env_kind, int net);
long long tb_ppo_workspace_bytes_net(int env_kind, int net, int batch);
int tb_ppo_grad_net(int env_kind, int net, int device, void *stream, const float *obs_dev, const float *raw_actions_dev,
                    const float *old_logp_dev, const float *adv_dev, const float *returns_dev, long long n_rows,
                    const int64_t *idx_dev, int batch, const float *params_dev, int n_params, float clip_range, float vf_coef,
                    void *workspace_dev, size_t workspace_bytes);
int tb_ppo_apply_net(int env_kind, int net, int device, void *stream, int phases, const void *workspace_dev, size_t workspace_bytes,
                     int batch, float *params_dev, float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev, int n_params,
                     float *stats_dev, float ent_coef, float max_grad_norm, int world, float lr, float beta1, float beta2, float eps,
                     long long step);

/*
 * One minibatch step of a POPULATION of n_members learners in three launches (advantage sums + gradient, reduction, step), whatever
 * n_members is: the kernels above with the member as a second grid axis. The flat rollout arrays are shared; member m reads the
 * index row idx_dev + m * idx_stride (idx_stride >= batch), its parameter row params_dev + m * param_stride_floats
 * (param_stride_floats >= n_params; grad and both moments use the same stride), hp_dev[m] (clip_range and vf_coef in the gradient,
 * ent_coef in the reduction, lr in the step) and its workspace region, tb_ppo_members_workspace_stride_bytes(kind, net, batch)
 * apart (a multiple of 8, >= tb_ppo_workspace_bytes_net). tb_ppo_apply_members always reduces and then steps: no world, no
 * TB_PPO_VALUE_ONLY, no phases. After the pair, member m's grad, params, exp_avg, exp_avg_sq and stats [3] rows are bit for bit what
 * tb_ppo_grad_net + tb_ppo_apply_net(TB_PPO_REDUCE | TB_PPO_STEP, world = 1) leave, given that member's row of each and its four
 * scalars. Floats between rows are neither read nor written. Refused before the device is looked up: n_members outside
 * [1, 65535], batch < 2, a null pointer, a float array not 4-byte aligned, idx / workspace / hp not 8-byte aligned, a stride that is
 * too short, workspace_bytes < n_members * the stride, n_params other than tb_ppo_param_floats_net: TB_E_INVAL; a (kind, net) pair
 * that is not built: TB_E_PARAMS.
 */
typedef struct TbPpoMemberHp { float clip_range, vf_coef, ent_coef, lr; } TbPpoMemberHp;   /* 16 bytes, device array [M] */
long long tb_ppo_members_workspace_stride_bytes(int env_kind, int net, int batch);
int tb_ppo_grad_members(int env_kind, int net, int device, void *stream, const float *obs_dev, const float *raw_actions_dev,
                        const float *old_logp_dev, const float *adv_dev, const float *returns_dev, long long n_rows,
                        const int64_t *idx_dev, size_t idx_stride, int batch, int n_members, const float *params_dev,
                        size_t param_stride_floats, int n_params, const TbPpoMemberHp *hp_dev, void *workspace_dev, size_t workspace_bytes);
int tb_ppo_apply_members(int env_kind, int net, int device, void *stream, const void *workspace_dev, size_t workspace_bytes,
                         int batch, int n_members, float *params_dev, float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                         size_t param_stride_floats, int n_params, float *stats_dev /* [M][3] */, const TbPpoMemberHp *hp_dev,
                         float max_grad_norm, float beta1, float beta2, float eps, long long step);

/*
 * The TRPO learner's policy step (csrc/tb_trpo.hpp; tennisbot_rl_amd/trpo.py is the caller), in the conventions of the tb_ppo_*
 * block above: (env_kind, device, stream), caller-owned device buffers, host-only workspace-size queries, refusals before any
 * launch. Vectors over the parameters (vec, out, direction) are full flat vectors of tb_ppo_param_floats(kind) floats; only
 * their policy slots (log_std, policy_net, action_net) are read, and the value slots of `out` are written as 0.
 *
 * tb_trpo_fvp: out = F vec + damping vec, F the Fisher matrix of the diagonal-Gaussian policy over the rows idx[0 .. n_idx) of
 * obs [n_rows][O]: (1/n_idx) sum_rows J^T diag(sigma^-2) J on the network's slots (J = d mean / d theta), 2 on log_std. Each
 * workgroup takes tb_trpo_rows_per_workgroup() entries of idx; per-wave partial vectors in the workspace
 * (tb_trpo_fvp_workspace_bytes(kind, n_idx)), then a fixed-order float64 reduction: the same inputs give the same bits. The
 * damping term is added in float32 after the sum is rounded: fvp(d) == fvp(0) + fl(d vec) bit for bit. out must not be vec.
 *
 * tb_trpo_search: for each candidate k < n_candidates (<= 64), theta_k = params + steps[k] * direction, over the rows
 * idx[0 .. batch): out[2 k] = mean(ratio_k * A_hat) (ratio_k = exp(logp_k - old_logp); A_hat = adv normalised over those rows
 * with mean and unbiased std + 1e-8, as tb_ppo_grad does) and out[2 k + 1] = mean KL(theta || theta_k). One launch over
 * candidates x tb_trpo_search_rows_per_workgroup()-row shares, float64 partial sums, a fixed-order reduction. A zero step gives
 * KL == 0.0 exactly. Workspace: tb_trpo_search_workspace_bytes(kind, batch, n_candidates). idx values outside [0, n_rows) are
 * clamped in both functions.
 */
int tb_trpo_rows_per_workgroup(void);
int tb_trpo_search_rows_per_workgroup(void);
long long tb_trpo_fvp_workspace_bytes(int env_kind, int n_idx);
long long tb_trpo_search_workspace_bytes(int env_kind, int batch, int n_candidates);
int tb_trpo_fvp(int env_kind, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev, int n_idx,
                const float *params_dev, const float *vec_dev, int n_params, float damping, float *out_dev, void *workspace_dev,
                size_t workspace_bytes);
int tb_trpo_search(int env_kind, int device, void *stream, const float *obs_dev, const float *raw_actions_dev,
                   const float *old_logp_dev, const float *adv_dev, long long n_rows, const int64_t *idx_dev, int batch,
                   const float *params_dev, const float *direction_dev, int n_params, const float *steps_dev, int n_candidates,
                   double *out_dev, void *workspace_dev, size_t workspace_bytes);
/*
 * The same two calls and their workspace queries for a network given by name (the names above are the TB_NET_DEFAULT calls):
 * TB_NET_MLP64 on SwingRacket-v0, vectors of tb_ppo_param_floats_net(kind, net) floats. TB_NET_TUNED is refused (TB_E_PARAMS): the
 * tuned network's shared extractor has no instantiation of these kernels.
 */
long long tb_trpo_fvp_workspace_bytes_net(int env_kind, int net, int n_idx);
long long tb_trpo_search_workspace_bytes_net(int env_kind, int net, int batch, int n_candidates);
int tb_trpo_fvp_net(int env_kind, int net, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev,
                    int n_idx, const float *params_dev, const float *vec_dev, int n_params, float damping, float *out_dev,
                    void *workspace_dev, size_t workspace_bytes);
int tb_trpo_search_net(int env_kind, int net, int device, void *stream, const float *obs_dev, const float *raw_actions_dev,
                       const float *old_logp_dev, const float *adv_dev, long long n_rows, const int64_t *idx_dev, int batch,
                       const float *params_dev, const float *direction_dev, int n_params, const float *steps_dev, int n_candidates,
                       double *out_dev, void *workspace_dev, size_t workspace_bytes);
/*
 * tb_trpo_returns: agent.py's critic-free estimator (agent.py:193-230, 264-268), the discounted return-to-go of the episodes that
 * ended inside the rollout. rewards / dones are [T][n] with tb_ppo_gae's step strides (0 = contiguous) and its refusals. With L_e the
 * last step of env e whose done != 0 (-1: none), row (t, e) -- flat index t n + e -- is FINISHED iff t <= L_e. On finished rows
 * R[t] = r[t] where done[t], else r[t] + discount R[t + 1]: carried in float64, the product and the sum rounded separately, rounded
 * to float32 once at the store (a plain numpy float64 loop gives the same bits). Unfinished rows hold 0.0f. returns is contiguous
 * [T][n]; idx[0 .. *count) holds the flat indices of the finished rows in ascending order, entries from *count on are not written
 * (idx needs room for T n entries); count is ONE int64 on the device. Four launches, no atomics: the same inputs give the same
 * bits. Workspace: tb_trpo_returns_workspace_bytes(n_steps, n_envs), 8-byte aligned. The network plays no part.
 */
long long tb_trpo_returns_workspace_bytes(int n_steps, int n_envs);
int tb_trpo_returns(int env_kind, int device, void *stream, int n_steps, int n_envs, const float *rewards_dev,
                    size_t reward_step_stride_bytes, const uint8_t *dones_dev, size_t done_step_stride_bytes, double discount,
                    float *returns_dev, int64_t *idx_dev, int64_t *count_dev, void *workspace_dev, size_t workspace_bytes);

/*
 * The SAC learner (csrc/tb_sac.hpp; tennisbot_rl_amd/sac.py is the caller): SB3 1.8.0's SAC with MlpPolicy, [256, 256] ReLU nets,
 * in the conventions of the tb_ppo_* / tb_trpo_* blocks: (env_kind, device, stream), caller-owned device buffers, a host-only
 * workspace query, refusals before any device is looked for. fp32 on the f32-input MFMA; losses and statistics are float64 sums
 * in a fixed order; no float atomics: the same inputs give the same bits.
 *
 * Flat parameter vectors, named_parameters() order. TB_SAC_ACTOR (70668 floats SwingRacket-v0, 70148 Tennisbot-v0): latent_pi.0
 * W [256][O] b | latent_pi.2 W [256][256] b | mu W [A][256] b | log_std W [A][256] b. TB_SAC_CRITIC (138754 / 139778; the target
 * has the same shape): qf0 then qf1, each W [256][O + A] b | W [256][256] b | W [1][256] b on cat(obs, action).
 *
 * The replay arrays are obs / next_obs [n_rows][O], action [n_rows][A], reward [n_rows], done [n_rows] (float32, 0 or 1); the
 * batch is the rows idx[0 .. batch) (int64; values outside [0, n_rows) are clamped), gathered by the kernels. eps is the
 * standard-normal noise [batch][A], an input. The workspace (tb_sac_workspace_bytes(kind, batch), 8-byte aligned) carries the
 * activations from one stage to the next: the stages of one gradient step use ONE workspace and ONE batch, in this order:
 *
 * tb_sac_actor_forward: a~ = tanh(mu + exp(clamp(log_std, -20, 2)) eps), logp = sum(-eps^2 / 2 - log_std - ln sqrt(2 pi)) -
 *   sum log(1 - a~^2 + 1e-6) on obs; act_out [batch][A], logp_out [batch]. Keeps the actor's activations for tb_sac_actor_grad.
 * tb_sac_targets: y = r + (1 - d) gamma (min(Q1t, Q2t)(s', a') - alpha logp'), (a', logp') the actor on next_obs with eps_next,
 *   alpha = exp(*log_ent_coef_dev). The envs carry no time limit: done is a true terminal, and y == r bit for bit there.
 * tb_sac_critic_grad: grad_dev = the gradient of 0.5 (mean (Q1(s, a) - y)^2 + mean (Q2(s, a) - y)^2); stats_dev[0] = that loss.
 * tb_sac_actor_grad: the gradient of mean(alpha logp - min(Q1, Q2)(s, a~)) with respect to the actor alone, with critic_dev as it
 *   is NOW (the caller has stepped it), through both critics' input gradients, the min, tanh and the log(1 - a~^2 + 1e-6) term;
 *   *ent_grad_dev = -mean(logp - A), the gradient of log_ent_coef; stats_dev[1] = the loss, [2] = mean logp, [3] = the entropy
 *   coefficient's gradient. Needs tb_sac_actor_forward's workspace content of the same batch. Writes no critic gradient.
 * tb_sac_adam: plain Adam (torch's: eps added to sqrt(v_hat)) on params[0 .. n); step is the 1-based count of this step. With
 *   target_dev the Polyak update target = (1 - tau) target + tau params (SB3's two roundings) follows on the NEW parameters in the
 *   same launch; with params-only pointers null (grad, moments) and target_dev set it is the Polyak update alone.
 * stats_dev: 4 doubles. tb_sac_rows_per_workgroup(): the rows one workgroup of the tile kernels takes.
 */
#define TB_SAC_ACTOR 0
#define TB_SAC_CRITIC 1
int tb_sac_param_floats(int env_kind, int which);
int tb_sac_rows_per_workgroup(void);
long long tb_sac_workspace_bytes(int env_kind, int batch);
int tb_sac_actor_forward(int env_kind, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev,
                         int batch, const float *actor_dev, const float *eps_dev, float *act_out_dev, float *logp_out_dev,
                         void *workspace_dev, size_t workspace_bytes);
int tb_sac_targets(int env_kind, int device, void *stream, const float *next_obs_dev, const float *reward_dev, const float *done_dev,
                   long long n_rows, const int64_t *idx_dev, int batch, const float *actor_dev, const float *target_dev,
                   const float *log_ent_coef_dev, const float *eps_next_dev, float gamma, float *y_dev, void *workspace_dev,
                   size_t workspace_bytes);
int tb_sac_critic_grad(int env_kind, int device, void *stream, const float *obs_dev, const float *action_dev, long long n_rows,
                       const int64_t *idx_dev, int batch, const float *critic_dev, const float *y_dev, float *grad_dev,
                       double *stats_dev, void *workspace_dev, size_t workspace_bytes);
int tb_sac_actor_grad(int env_kind, int device, void *stream, int batch, const float *actor_dev, const float *critic_dev,
                      const float *log_ent_coef_dev, const float *eps_dev, float *actor_grad_dev, float *ent_grad_dev,
                      double *stats_dev, void *workspace_dev, size_t workspace_bytes);
int tb_sac_adam(int device, void *stream, float *params_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                long long n, float lr, float beta1, float beta2, float eps, long long step, float *target_dev, float tau);

/*
 * The TQC learner (csrc/tb_tqc.hpp; tennisbot_rl_amd/tqc.py is the caller): sb3_contrib 1.8.0's TQC with MlpPolicy at its
 * defaults, in the conventions of the tb_sac_* block above, whose actor, replay arrays, index vector, noise, stats_dev and
 * tb_sac_adam (Adam and Polyak, unchanged) it shares. Each of the two critics ends in TB_TQC_QUANTILES outputs; the top
 * TB_TQC_DROP_PER_NET per net of the sorted target quantiles are dropped, TB_TQC_TARGETS are kept.
 *
 * Flat parameter vectors, named_parameters() order. TB_SAC_ACTOR: SAC's (70668 / 70148). TB_SAC_CRITIC (151090 floats
 * SwingRacket-v0, 152114 Tennisbot-v0; the target has the same shape): qf0 then qf1, each W [256][O + A] b | W [256][256] b |
 * W [25][256] b on cat(obs, action). The workspace is tb_tqc_workspace_bytes(kind, batch), 8-byte aligned: ONE workspace and
 * ONE batch for the stages of a gradient step, in this order:
 *
 * tb_tqc_actor_forward: as tb_sac_actor_forward. Keeps the actor's activations for tb_tqc_actor_grad.
 * tb_tqc_targets: z = the 50 quantiles of both targets on (s', a'), sorted ascending (equal values keep one slot each; a NaN
 *   orders last, as torch.sort has it); y_dev [batch][46], y[b][j] = r + (1 - d) gamma (z[j] - alpha logp'), j < 46,
 *   alpha = exp(*log_ent_coef_dev). A terminal row's 46 entries are r bit for bit.
 * tb_tqc_critic_grad: grad_dev = the gradient of the quantile Huber loss, the mean over rows b, critics n, quantiles i and
 *   targets j of |tau_i - [delta < 0]| H(delta), delta = y[b][j] - Q_n(s, a)[i], tau_i = (i + 0.5) / 25, H(delta) = |delta| - 0.5
 *   where |delta| > 1 and delta^2 / 2 elsewhere; stats_dev[0] = that loss.
 * tb_tqc_actor_grad: the gradient of mean(alpha logp - Qbar(s, a~)), Qbar the mean over the 25 quantiles and the 2 critics, with
 *   respect to the actor alone, with critic_dev as it is NOW; *ent_grad_dev and stats_dev[1 .. 3] as tb_sac_actor_grad. Needs
 *   tb_tqc_actor_forward's workspace content of the same batch. Writes no critic gradient.
 */
#define TB_TQC_QUANTILES 25
#define TB_TQC_DROP_PER_NET 2
#define TB_TQC_TARGETS 46
int tb_tqc_param_floats(int env_kind, int which);
long long tb_tqc_workspace_bytes(int env_kind, int batch);
int tb_tqc_actor_forward(int env_kind, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev,
                         int batch, const float *actor_dev, const float *eps_dev, float *act_out_dev, float *logp_out_dev,
                         void *workspace_dev, size_t workspace_bytes);
int tb_tqc_targets(int env_kind, int device, void *stream, const float *next_obs_dev, const float *reward_dev, const float *done_dev,
                   long long n_rows, const int64_t *idx_dev, int batch, const float *actor_dev, const float *target_dev,
                   const float *log_ent_coef_dev, const float *eps_next_dev, float gamma, float *y_dev, void *workspace_dev,
                   size_t workspace_bytes);
int tb_tqc_critic_grad(int env_kind, int device, void *stream, const float *obs_dev, const float *action_dev, long long n_rows,
                       const int64_t *idx_dev, int batch, const float *critic_dev, const float *y_dev, float *grad_dev,
                       double *stats_dev, void *workspace_dev, size_t workspace_bytes);
int tb_tqc_actor_grad(int env_kind, int device, void *stream, int batch, const float *actor_dev, const float *critic_dev,
                      const float *log_ent_coef_dev, const float *eps_dev, float *actor_grad_dev, float *ent_grad_dev,
                      double *stats_dev, void *workspace_dev, size_t workspace_bytes);

/*
 * One gradient step of a POPULATION of n_members SAC (or TQC) learners in the launches of ONE learner's step, whatever n_members
 * is: the kernels of the tb_sac_* / tb_tqc_* stages above with the member as one more grid axis (csrc/tb_sac.hpp, "THE MEMBER
 * AXIS"). The replay arrays obs / next_obs / action / reward / done of n_rows rows are SHARED. Everything else is per member, in
 * rows a stride apart; member m reads and writes
 *   its index row idx_dev + m * idx_stride (entries; idx_stride >= batch; values outside [0, n_rows) are clamped),
 *   its parameter rows actor_dev + m * actor_stride_floats and critic_dev / target_dev + m * critic_stride_floats (each stride >=
 *     tb_sac_param_floats / tb_tqc_param_floats of that vector; a gradient and both moments use their parameter's stride, the
 *     target the critic's),
 *   its noise row eps_dev + m * eps_stride_floats (>= batch * A), act_out_dev + m * act_stride_floats (>= batch * A), logp_out_dev
 *     + m * logp_stride_floats (>= batch), y_dev + m * y_stride_floats (>= batch for SAC, batch * 46 for TQC),
 *   log_ent_coef_dev[m], ent_grad_dev[m], its statistics row stats_dev + 4 m (doubles), its hyper-parameter row hp_dev[m],
 *   its workspace region, tb_sac_members_workspace_stride_bytes(kind, batch) apart (tb_tqc_... for TQC): a multiple of 8, at least
 *     the single-member query; workspace_bytes >= n_members * that stride.
 * After a stage, member m's outputs are bit for bit what the single-member stage leaves, given that member's row of each array
 * and its scalars (gamma in the targets; lr and tau in tb_sac_adam_members). Floats between rows are neither read nor written.
 * tb_sac_adam_members is tb_sac_adam over [n_members] rows of n floats `stride_floats` apart (grad, both moments and the target
 * included): lr is hp_dev[m]'s lr_actor, lr_critic or lr_ent as which_lr (TB_SAC_LR_*) names it, tau hp_dev[m].tau with 1 - tau
 * formed as tb_sac_adam forms it; betas, eps and the step count are shared. target_dev may be null (no Polyak update); with
 * grad and both moments null and target_dev set it is every member's Polyak update alone, as in tb_sac_adam. log_ent_coef's step is
 * the call with n = 1 and stride_floats = 1. TQC uses it as it is.
 * Refused before the device is looked up, with the entry point's name in tb_last_error: n_members outside [1, TB_SAC_MAX_MEMBERS]
 * (the (member, net) pair is the grid's z axis: 2 * n_members <= 65535), batch < 1, a null pointer, a float array not 4-byte
 * aligned, idx / stats / hp / the workspace not 8-byte aligned, a stride that is too short, a gradient row range that overlaps its
 * parameter rows, an unknown env kind: TB_E_INVAL; workspace_bytes < n_members * the stride: TB_E_PARAMS.
 */
#define TB_SAC_MAX_MEMBERS 32767
#define TB_SAC_LR_ACTOR 0
#define TB_SAC_LR_CRITIC 1
#define TB_SAC_LR_ENT 2
typedef struct TbSacMemberHp { float lr_actor, lr_critic, lr_ent, gamma, tau, reserved[3]; } TbSacMemberHp;   /* 32 bytes, device array [M] */
long long tb_sac_members_workspace_stride_bytes(int env_kind, int batch);
long long tb_tqc_members_workspace_stride_bytes(int env_kind, int batch);
int tb_sac_actor_forward_members(int env_kind, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev,
                                 size_t idx_stride, int batch, int n_members, const float *actor_dev, size_t actor_stride_floats,
                                 const float *eps_dev, size_t eps_stride_floats, float *act_out_dev, size_t act_stride_floats,
                                 float *logp_out_dev, size_t logp_stride_floats, void *workspace_dev, size_t workspace_bytes);
int tb_sac_targets_members(int env_kind, int device, void *stream, const float *next_obs_dev, const float *reward_dev,
                           const float *done_dev, long long n_rows, const int64_t *idx_dev, size_t idx_stride, int batch, int n_members,
                           const float *actor_dev, size_t actor_stride_floats, const float *target_dev, size_t critic_stride_floats,
                           const float *log_ent_coef_dev /* [M] */, const float *eps_next_dev, size_t eps_stride_floats,
                           const TbSacMemberHp *hp_dev, float *y_dev, size_t y_stride_floats, void *workspace_dev, size_t workspace_bytes);
int tb_sac_critic_grad_members(int env_kind, int device, void *stream, const float *obs_dev, const float *action_dev, long long n_rows,
                               const int64_t *idx_dev, size_t idx_stride, int batch, int n_members, const float *critic_dev,
                               size_t critic_stride_floats, const float *y_dev, size_t y_stride_floats, float *grad_dev,
                               double *stats_dev /* [M][4] */, void *workspace_dev, size_t workspace_bytes);
int tb_sac_actor_grad_members(int env_kind, int device, void *stream, int batch, int n_members, const float *actor_dev,
                              size_t actor_stride_floats, const float *critic_dev, size_t critic_stride_floats,
                              const float *log_ent_coef_dev /* [M] */, const float *eps_dev, size_t eps_stride_floats,
                              float *actor_grad_dev, float *ent_grad_dev /* [M] */, double *stats_dev /* [M][4] */, void *workspace_dev,
                              size_t workspace_bytes);
int tb_tqc_actor_forward_members(int env_kind, int device, void *stream, const float *obs_dev, long long n_rows, const int64_t *idx_dev,
                                 size_t idx_stride, int batch, int n_members, const float *actor_dev, size_t actor_stride_floats,
                                 const float *eps_dev, size_t eps_stride_floats, float *act_out_dev, size_t act_stride_floats,
                                 float *logp_out_dev, size_t logp_stride_floats, void *workspace_dev, size_t workspace_bytes);
int tb_tqc_targets_members(int env_kind, int device, void *stream, const float *next_obs_dev, const float *reward_dev,
                           const float *done_dev, long long n_rows, const int64_t *idx_dev, size_t idx_stride, int batch, int n_members,
                           const float *actor_dev, size_t actor_stride_floats, const float *target_dev, size_t critic_stride_floats,
                           const float *log_ent_coef_dev /* [M] */, const float *eps_next_dev, size_t eps_stride_floats,
                           const TbSacMemberHp *hp_dev, float *y_dev, size_t y_stride_floats, void *workspace_dev, size_t workspace_bytes);
int tb_tqc_critic_grad_members(int env_kind, int device, void *stream, const float *obs_dev, const float *action_dev, long long n_rows,
                               const int64_t *idx_dev, size_t idx_stride, int batch, int n_members, const float *critic_dev,
                               size_t critic_stride_floats, const float *y_dev, size_t y_stride_floats, float *grad_dev,
                               double *stats_dev /* [M][4] */, void *workspace_dev, size_t workspace_bytes);
int tb_tqc_actor_grad_members(int env_kind, int device, void *stream, int batch, int n_members, const float *actor_dev,
                              size_t actor_stride_floats, const float *critic_dev, size_t critic_stride_floats,
                              const float *log_ent_coef_dev /* [M] */, const float *eps_dev, size_t eps_stride_floats,
                              float *actor_grad_dev, float *ent_grad_dev /* [M] */, double *stats_dev /* [M][4] */, void *workspace_dev,
                              size_t workspace_bytes);
int tb_sac_adam_members(int device, void *stream, float *params_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                        long long n, size_t stride_floats, int n_members, const TbSacMemberHp *hp_dev, int which_lr, float beta1,
                        float beta2, float eps, long long step, float *target_dev);

/*
 * rgb_array frames of env states (csrc/tb_render.hpp states the whole rule: camera, primitives, shading, exceptional values): what
 * the reference's render() set out to do (tennisbot_env.py:263-288 builds a camera at the racket and leaves getCameraImage
 * commented out; validate.py / validate_swing.py open PyBullet's GUI). One launch casts one primary ray per pixel of every image
 * against the ground and net boxes, the SwingRacket-v0 goal cylinder, the ball and the racket's extruded hull (hull_margin, court
 * lines and textures, and a racket shadow are not drawn), in the conventions of the tb_ppo_* block: no handle, caller-owned device
 * buffers, refusals before any launch, complete in stream order on `stream`.
 *   words_dev: [tb_state_words(kind)][n_envs] in tb_get_state's layout; only read. Image k shows env env_idx[k] (any order,
 *     repeats allowed, values outside [0, n_envs) clamped), or env k when env_idx is null (then n_images <= n_envs).
 *   params: the scene (ground_half, net_half and TB_F_NET, goal_*, ball_radius, racket_half_thick, hull_bound_radius, hull_edges)
 *     and, on SwingRacket-v0, racket_scale; a Tennisbot-v0 env is drawn at the scale in its own TB_W_TN_SCALE word.
 *   camera: origin top-left, x to the right; the ray of pixel (i, j) passes through its centre (i + 0.5, j + 0.5).
 *   rgb_dev uint8 [n_images][H][W][3]; id_dev_or_null uint8 [n_images][H][W]: 0 sky, 1 ground, 2 net, 3 goal, 4 ball, 5 racket;
 *   depth_dev_or_null float32 [n_images][H][W]: the ray parameter along the unit direction, +inf for sky.
 * A primitive whose state is not finite is not drawn; no output is ever NaN, out of 0..5, or a negative depth.
 * TB_E_INVAL (and a tb_last_error text): null params / words / camera / rgb, n_hull outside [3, TB_MAX_HULL], a size < 1 (or a
 * side > 16384), struct_size != sizeof(TbCamera), a camera vector that is not finite, eye == target, up zero or parallel to the
 * view direction, light_dir zero, fov_y_deg outside (0, 180), follow not 0 or 1, a misaligned words / env_idx / depth pointer.
 */
typedef struct TbCamera {
  uint32_t struct_size;             /* sizeof(TbCamera) */
  float eye[3], target[3], up[3];   /* up need not be orthogonal to the view direction */
  float fov_y_deg;                  /* vertical field of view, (0, 180) */
  int32_t follow;                   /* 1: eye and target are offsets from EACH env's racket COM */
  float light_dir[3];               /* towards the light; normalised by the library */
} TbCamera;
int tb_render(int env_kind, int device, void *stream, const TbParams *params,
              const uint32_t *words_dev /* [tb_state_words][n_envs], tb_get_state's layout */, int n_envs,
              const int32_t *env_idx_dev_or_null, int n_images, const TbCamera *camera, int width, int height,
              uint8_t *rgb_dev, uint8_t *id_dev_or_null, float *depth_dev_or_null);

/*
 * The flight of a SwingRacket-v0 ball, substep by substep (csrc/tb_trace.hpp): ONE agent step of caller-owned states, with the states it
 * passes through stored as frames. The reference shows the flight in PyBullet's GUI (validate_swing.py); the fast-forward of
 * swingracket_env.py:105-141 runs up to 775 substeps inside env.step(), of which tb_step returns the reward, the terminal observation
 * and a count.
 *   words_dev [tb_state_words][n_rows] and done_dev [n_rows]: the states, in tb_get_state's layout; only read. actions_dev [n_rows][6].
 *   For every row, reward / substeps / done_out / obs (the observation of the final state; optional) are what this sequence gives, bit
 *   for bit: tb_set_state(words, done), then tb_step(actions), on a handle with the same parameters and no TB_F_AUTO_RESET. A restored
 *   state starts with empty racket<->court caches, and so does the trace. The frames are the states that step passed through.
 * Which substeps become frames. Number the substeps of the call s = 1 .. ns: s = 1 is the agent's substep, ns what tb_step reports in
 * substeps_dev (1 .. 776; 1 for a row that starts no flight: step count below 25, or a non-zero done byte). The sampled set is
 * {1 + j stride : j >= 0, 1 + j stride <= ns} plus ns itself, in increasing order: m = 1 + (ns - 1) / stride + ((ns - 1) % stride != 0).
 *   m <= max_frames: row k < m holds the state after the k-th sampled substep, rows m .. max_frames - 1 copies of the final state.
 *   m >  max_frames: rows 0 .. max_frames - 2 hold the first max_frames - 1 samples, row max_frames - 1 the state after substep ns.
 *   The last stored row is always the final state and no byte of frames_dev stays unwritten; n_frames_dev[i] = m in both cases (as
 *   snprintf reports the length it needed). A row's step-count word is the input step count + s; the episode word is unchanged: the
 *   trace never resets an env, whatever TB_F_AUTO_RESET says.
 *   frames_dev is [max_frames][tb_state_words][n_rows]: frames_dev + row * tb_state_words * n_rows is a words_dev for tb_render.
 * The handle supplies the parameters, the outline table and the device, and nothing else: the call does not touch its env state,
 * caches, counters, episode phase, pipeline slots or pool, and it does not flush. n_rows is independent of the handle's n_envs. The
 * call is complete in stream order on `stream`.
 * TB_E_INVAL before any launch, with "tb_swing_trace" in tb_last_error: a null handle or a null pointer other than obs, a Tennisbot-v0
 * handle (there every agent step is one substep and is visible as it is), n_rows < 1 (or > 2^25), stride < 1, max_frames < 1, a
 * pointer that is not 4-byte aligned (actions and obs: 8-byte, rows are accessed two floats at a time).
 */
int tb_swing_trace(TbHandle *h, const uint32_t *words_dev, const uint8_t *done_dev, int n_rows,
                   const float *actions_dev /* [n_rows][6] */, int stride, int max_frames,
                   uint32_t *frames_dev /* [max_frames][tb_state_words][n_rows] */, int32_t *n_frames_dev,
                   float *reward_dev, int32_t *substeps_dev, uint8_t *done_out_dev,
                   float *obs_dev_or_null /* [n_rows][6]: the observation of the final state */, void *stream);

/*
 * Pipelined fast-forward (SwingRacket-v0 with TB_F_AUTO_RESET; HIP streams, no reference
 * counterpart). The <= 775-substep fast-forward of swingracket_env.py:105-141 takes no
 * agent input, and the next episode does not depend on its outcome. With the pipeline
 * enabled, the 26th tb_step after a full tb_reset parks each env's pre-loop state, resets
 * the env and returns at once with obs (first observation of the new episode) and done = 1;
 * the loop itself runs on a stream owned by the handle, overlapping the following steps, and
 * then writes THAT step's reward, terminal observation and substep count into the buffers
 * that were passed to that tb_step call. Those buffers must therefore stay valid and must not
 * be reused until tb_flush; results are bit-identical to the unpipelined path.
 * tb_flush makes `stream` wait for all outstanding fast-forwards (tb_get_state, tb_set_state,
 * tb_counters, tb_reset, tb_set_params and tb_destroy do so themselves).
 * Replays of captured graphs are launched by the caller, not by this library: a caller that mixes eager
 * pipelined steps with graph replays calls tb_flush on the replaying stream first (the graph's launches bake in
 * slot indices and cannot wait for an eager fast-forward still reading its slot; stepper.StepGraph.replay does).
 * At most 2^24 envs per handle with the pipeline on. Device memory per env: 8 slots of parked records (192 B) and flags, with
 * ff_phases > 1 also up to two survivor lists per slot: 1.5-4.6 KB; handles that use the pool (TbOptions.ff_defer: on request, by
 * default up to 16384 envs, above that -- to 131072 -- only with TB_F_RACKET_GROUND, then allocated by the tb_set_params call that
 * turns it on) another 72 records + destination pointers: 14 KB.
 */
int tb_set_pipeline(TbHandle *h, int enable);
int tb_flush(TbHandle *h, void *stream);
/*
 * Progress marks (for callers that ship a rollout in chunks while ONE hipGraph is still producing it). A mark
 * tells the HOST that everything tb_step was asked to do before it is final in the caller's buffers -- the steps
 * themselves AND the late fast-forward writes they are still owed -- without making any stream wait for
 * anything: nothing is forked or joined, the graph keeps the shape it has without marks.
 * tb_mark_enable(h, 1): from now on every fast-forward kernel is followed on its side stream by a one-thread
 * kernel that counts it as finished in pinned host memory (off by default: plain graphs carry nothing extra);
 * call it before issuing -- or capturing -- the steps that marks will cover.
 * tb_mark_record(h, k, stream): the same one-thread kernel on `stream`, incrementing counter k; the library
 * remembers how many fast-forwards were enqueued before the mark (with TbOptions.ff_defer form 2 it first enqueues, on a side
 * stream, the ONE fast-forward launch of the episodes parked since the previous mark). Captured into a graph these are ordinary kernel nodes: every replay fires them again.
 * tb_mark_begin(h): snapshot of the counters; call it right before launching the work that contains the marks,
 * with nothing of this handle in flight (e.g. after a stream synchronize).
 * tb_mark_host_wait(h, k, timeout_ms): spin on the host until mark k has fired since tb_mark_begin and the
 * fast-forwards enqueued before it have finished; TB_E_TIMEOUT otherwise. The host waits, never a stream: a
 * stream-side wait queued on a hardware queue that the graph's own later kernels share would stall the very work
 * it waits for. One marked graph per handle at a time; 0 <= k < TB_MAX_MARKS.
 * tb_mark_count(h, k): how often mark k has fired since tb_create (a host read, no HIP call).
 */
#define TB_MAX_MARKS 64
int tb_mark_enable(TbHandle *h, int on);
int tb_mark_record(TbHandle *h, int k, void *stream);
int tb_mark_begin(TbHandle *h);
int tb_mark_host_wait(TbHandle *h, int k, int timeout_ms);
long long tb_mark_count(TbHandle *h, int k);
/* Stream-capture support (hipGraph): events recorded inside a capture are meaningless outside
 * it and vice versa. Call with host_wait = 1 right BEFORE beginning a capture that will contain
 * tb_step calls (drains the side streams on the host and forgets their events), capture
 * ... tb_step x K ... tb_flush on the capturing stream, end the capture, then call with
 * host_wait = 0 (forget the capture-local events). */
int tb_pipeline_sync(TbHandle *h, int host_wait);
/* The host-side episode phase of a SwingRacket handle: agent steps since the last common reset, modulo 26
 * (every episode is exactly 26 steps, swingracket_env.py:105-129), or -1 when the envs are not known to be
 * in lockstep (masked reset, injected state whose step counters differ). The pipelined kernels use it to
 * know which launch ends the episodes. A capture advances it by the captured steps although nothing ran:
 * tb_pipeline_sync(h, 0) therefore puts it back to the value of the matching tb_pipeline_sync(h, 1), and
 * whoever replays the captured steps calls tb_phase_advance(h, K) per replay -- after checking that
 * tb_phase(h) is the phase the steps were captured at (a graph bakes in WHICH of its steps end an episode).
 * tb_set_state re-derives the phase from the step-count row when every env agrees.
 * tb_phase_advance(h, K) is also how replayed steps reach the substep counter: every agent step runs at least one substep of
 * every env, and that share (n_envs x steps) is counted by the host -- per launch when a launch is enqueued to run, not at all
 * while it is only being captured, and per replay through this call. (One atomic per launch from one lane was 2.7 % of the
 * 4096-env rate.) */
int tb_phase(TbHandle *h);
int tb_phase_advance(TbHandle *h, int n_steps);
/* Which form the SwingRacket pipeline takes on this handle as it stands (TbOptions.ff_defer, the batch size, the contact flags,
 * progress marks on or off) for steps that ask for no terminal-observation / substep outputs: 0 = no pipeline (the fast-forward runs
 * inside the 26th step's kernel), 1 = one fast-forward kernel per episode end on a side stream, 2 = the same, its stragglers moving on
 * to the pool, 3 = every episode end parked into the pool, one fast-forward launch at the join (and at each progress mark). For
 * reports (bench.py names it). */
int tb_pipeline_form(TbHandle *h);
/* waves per 64 envs of the pipelined SwingRacket-v0 one-step kernel (TbOptions.step_waves): 2 or 1; 0 for a handle without that kernel */
int tb_step_waves(TbHandle *h);
/* which form of that kernel the next tb_step would launch: 0 = one-wave (also the episodes' last step while the library knows the episode
 * phase: every env parks there), 1 = two-wave with the early gate and full loads (phase unknown: after a masked reset or an injected
 * state out of lockstep), 2 = two-wave short (phase known, not the last step: each wave loads its own side only); -1 for a handle
 * without that kernel. A captured launch keeps the form of the phase it was captured at. */
int tb_step_form(TbHandle *h);
/* After a capture that contained tb_step calls was ABANDONED (it failed, e.g. because something else
 * in it was not capturable): the handle's side streams were forked into that capture and stay
 * invalidated, and the host's episode-phase hint ran ahead of the device. Replaces the side streams
 * and their events, restores the phase of the last tb_pipeline_sync(h, 1), clears the sticky HIP
 * error. The env state itself is untouched (nothing captured ever ran). */
int tb_pipeline_recover(TbHandle *h);

/* Snapshot / restore the persistent state (the reference never checkpoints env state;
 * SURVEY.md section 5). words: [tb_state_words][N] uint32 bit patterns, done: [N] bytes.
 * `on_device` != 0: the buffers are device memory (async on stream); 0: host memory
 * (the call synchronises the stream before returning). tb_set_state on a SwingRacket handle
 * with the pipeline ON also synchronises the stream in the on_device case (it reads the
 * step-count row back to re-derive the episode phase, see tb_phase) and so cannot be captured
 * into a graph; with the pipeline off an on_device restore is fully asynchronous. The racket<->court
 * contact caches are not part of the state words: a restored state starts with empty caches. */
int tb_get_state(TbHandle *h, uint32_t *words, uint8_t *done, int on_device, void *stream);
int tb_set_state(TbHandle *h, const uint32_t *words, const uint8_t *done, int on_device, void *stream);

/* per-handle event counters since create or the last tb_counters_reset: the batched
 * stand-in for the reference's per-step prints (swingracket_env.py:102,115,124,129;
 * tennisbot_env.py:172,191,202). out[0] racket-ball contact substeps, [1] ball-court
 * terminations, [2] goal hits, [3] timeouts, [4] pass-racket terminations, [5] episodes
 * finished, [6] substeps, [7] non-finite state detections, [8] lockstep violations: lanes that reached
 * an episode end in a launch the host had not given a fast-forward slot (only possible when a captured
 * graph is replayed at another phase than it was captured at; their terminal reward is lost). Synchronises
 * the stream.
 * CONTRACT for callers that replay captured graphs themselves: out[6] counts the first substep of every agent step on the HOST,
 * when tb_step / tb_rollout / tb_policy_* ENQUEUE work that runs (n_envs x steps per call; nothing during stream capture, where
 * nothing runs). Each replay of a graph holding K captured steps must therefore be reported with tb_phase_advance(h, K) -- the
 * call the episode phase needs anyway -- or out[6] under-reports by n_envs x K per replay (every other counter is device-side
 * and needs nothing). */
#define TB_N_COUNTERS 9
int tb_counters(TbHandle *h, uint64_t *out, void *stream);
int tb_counters_reset(TbHandle *h, void *stream);
/* how many of counters[6]'s substeps the pool's sealed-fate exit (TbOptions.ff_seal) booked without running them, since create or
 * the last tb_counters_reset. Joins the pipeline and synchronises the stream like tb_counters. */
int tb_sealed_substeps(TbHandle *h, uint64_t *out, void *stream);

/* Diagnostics (not part of the env surface): copies `rows` SoA rows of n 32-bit words,
 * src[r*n + i] -> dst[r*n + i], one dword per lane exactly like the step kernel's state
 * accesses. A known byte count in the kernel's own access pattern, used to calibrate the
 * rocprofv3 FETCH_SIZE / WRITE_SIZE counters (MI355X_MICROARCH.md, HBM section). */
int tb_diag_stream_copy(const uint32_t *src_dev, uint32_t *dst_dev, int n, int rows, int device, void *stream);
/* Diagnostics: `waves` one-wave workgroups that only stay resident (s_sleep) for `microseconds` on `stream`: the footprint of
 * the fast-forward waves without their arithmetic (tools/diag/r03_idle_probe.py: do resident waves shorten the dispatch gap between
 * the dependent launches of a graph?). */
int tb_diag_idle(int waves, int microseconds, int device, void *stream);
/* Diagnostics: out_dev[i] = 1 if SwingRacket-v0 env i's next step, from its current state, leaves the common path of the two-wave
 * step kernel (TbOptions.step_waves: the very test that kernel runs, tb_kernels.hpp two_wave_rare), else 0. n_envs bytes, on `stream`. */
int tb_diag_two_wave_gate(TbHandle *h, uint8_t *out_dev, void *stream);
/* Test hook: the nth device allocation of the pipeline or its pool from now on -- tb_set_pipeline(h, 1), or the pool that
 * tb_set_params allocates -- fails with hipErrorOutOfMemory (0 = off). tb_set_pipeline is all-or-nothing: after a failure the handle is as if the pipeline had never
 * been enabled (nothing half-allocated for a later step to park into), and a second call starts over. */
int tb_diag_fail_alloc(int nth);

#ifdef __cplusplus
}
#endif
#endif /* TB_STEPPER_H */
