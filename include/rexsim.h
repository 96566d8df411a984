/*
 * rexsim.h -- C ABI of the MI355X-native batched Rex simulator (librexsim_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of nicrusso7/rex-gym: what the reference does
 * per environment through `RexGymEnv.step()/reset()` (rex_gym/envs/rex_gym_env.py:296-414), i.e.
 *   envs/gym/walk_env.py:246-324   action -> staged gait parameters -> 12 joint targets
 *   model/gait_planner.py:96-134   Bezier/stance foot trajectories
 *   model/kinematics.py:104-142    closed-form leg IK
 *   model/rex.py:158-163,568-641   Step / ApplyAction (action_repeat x motor model + torque)
 *   model/motor.py:76-143          DC-motor PD actuator
 *   pybullet.stepSimulation        (third-party pybullet==2.8.3, requirements.txt:2)
 *   model/rex.py:717-733           ReceiveObservation
 *   envs/rex_gym_env.py:490-542    termination + reward, walk_env.py:356-362 observation
 * is done here for N environments at once by hand-written gfx950 kernels, one env per lane.
 *
 * The agents' rollout loop -- a policy in the loop -- runs inside the launch as well: rex_set_policy (the
 * feed-forward Gaussian MLP every shipped config uses) or rex_set_policy_recurrent (the GRU policy of
 * agents/scripts/networks.py:113-159, on a caller-owned per-env state), then rex_step_policy /
 * rex_step_segment_policy.
 *
 * The reference has no FFI: its boundary is the Python Gym protocol.  The binding a maintainer
 * adds is a ctypes stub; `rex_gym_amd/envs` is that stub plus the Gym surface.
 *
 * Conventions: every pointer named d_* is a DEVICE pointer (e.g. torch.Tensor.data_ptr()),
 * owned by the caller.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All calls return 0 on success or a negative REX_E* code; nothing throws; `rex_last_error()`
 * returns a thread-local message.  One host thread per RexSim.
 */
#ifndef REXSIM_H
#define REXSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REX_ABI_VERSION 6
#define REX_API __attribute__((visibility("default")))

/* tasks (reference env classes) */
#define REX_TASK_WALK   0   /* envs/gym/walk_env.py   RexWalkEnv      */
#define REX_TASK_GALLOP 1   /* envs/gym/gallop_env.py RexReactiveEnv  */
#define REX_TASK_TURN   2   /* envs/gym/turn_env.py   RexTurnEnv      */
#define REX_TASK_POSES  3   /* envs/gym/poses_env.py  RexPosesEnv     */
#define REX_TASK_STANDUP 4  /* envs/gym/standup_env.py RexStandupEnv  (the signal kwarg is unused by the env) */
#define REX_TASK_MIXED  5   /* every env runs ONE of the tasks in RexConfig.task_mix, drawn per env from its global
                               index (BASELINE.json configs[4]: the reference gets such a batch by handing BatchEnv a
                               list of different env objects, agents/tools/batch_env.py:21-44) */
/* signal_type kwarg of the reference envs */
#define REX_SIGNAL_IK 0
#define REX_SIGNAL_OL 1

/* `mark` kwarg of the reference envs (model/mark_constants.py:1-120): the robot variant.  'arm' adds the
 * 6-joint arm of rex_arm.urdf, its 6 motors held at ARM_POSES['rest'] (rex_gym_env.py:347-353). */
#define REX_MARK_BASE 0
#define REX_MARK_ARM  1

#define REX_NUM_MOTORS 12       /* mark 'base' */
#define REX_NUM_MOTORS_ARM 18   /* mark 'arm'  */

/* error codes */
#define REX_OK          0
#define REX_EINVAL     -1   /* bad argument / config */
#define REX_EHIP       -2   /* HIP runtime error (message in rex_last_error) */
#define REX_ENODEV     -3   /* no usable gfx950 device */
#define REX_ENOMEM     -4

/*
 * Per-env persistent state: SoA, float32 words, word-major ([REX_STATE_WORDS][num_envs]) so that
 * lane i of a wavefront reads word w of env i at d_state[w * num_envs + i] (coalesced).
 * Integer words are stored as raw int32 bits.
 *
 * Clocks (ABI 5).  The reference's clocks are Python floats: the env clock `step_counter * time_step` (rex.py:155-156),
 * GaitPlanner._last_time, the env's end_time.  With a 5 ms control step and gait periods such as 0.5 s, comparisons like
 * `phi >= 0.99`, `phi <= 0.5`, `t <= 0.8 + end_time` are exact ties in real numbers, decided by double rounding.  The
 * state therefore keeps those instants as the ENV STEP COUNT at which they were taken (int words LASTT, ENDTIME) and the
 * kernels rebuild the double the reference held from it; float32 carries values, never a decision of the controller.
 */
enum RexStateWord {
  REX_S_POS      = 0,   /* 3: base position, world [m]                   (getBasePositionAndOrientation) */
  REX_S_QUAT     = 3,   /* 4: base orientation x,y,z,w                                                  */
  REX_S_LINVEL   = 7,   /* 3: base linear velocity, world                (getBaseVelocity)               */
  REX_S_ANGVEL   = 10,  /* 3: base angular velocity, world                                               */
  REX_S_Q        = 13,  /* 12: motor angles, order of model/mark_constants.py:3-8                        */
  REX_S_QD       = 25,  /* 12: motor velocities                                                          */
  REX_S_PHI      = 37,  /* gait phase, float32 copy (GaitPlanner._phi, gait_planner.py:10); its one use, `_phi >= 0.99`
                           (gait_planner.py:106), is taken in double and kept as REX_F_PHASE_WRAP              */
  REX_S_LASTT    = 38,  /* int: env step whose clock GaitPlanner._last_time holds (gait_planner.py:12,107)       */
  REX_S_ALPHA    = 39,  /* gait rotation carry   (GaitPlanner._alpha,     gait_planner.py:13)            */
  REX_S_TARGET   = 40,  /* episode target (x position, or yaw for turn)  (walk_env.py:143-147)           */
  REX_S_ENDTIME  = 41,  /* int: env step at which the goal was reached; end_time = its clock (walk_env.py:213)   */
  REX_S_AUX      = 42,  /* task scratch (turn: start yaw)                                                */
  REX_S_FLAGS    = 43,  /* int: REX_F_* bits                                                             */
  REX_S_STEPS    = 44,  /* int: env steps this episode (RexGymEnv._env_step_counter)                     */
  REX_S_EPISODE  = 45,  /* int: episodes started (RNG counter)                                           */
  REX_S_MOTOR_EN = 46,  /* int: bit i = motor i enabled (Rex._motor_enabled_list, rex.py:302)            */
  REX_S_OVERHEAT = 47,  /* 6 ints: 12 x u16 overheat counters, motor 2k in low half (rex.py:301,601-608) */
  REX_S_HIST     = 53,  /* int: observation-history ring, bits 0-7 newest slot, bits 8-15 fill (1..100)      */
  REX_STATE_WORDS = 54
};

#define REX_F_GOAL_REACHED   1u   /* walk_env.py:211 */
#define REX_F_TERMINATING    2u   /* walk_env.py:214 */
#define REX_F_STAY_STILL     4u   /* walk_env.py:280 */
#define REX_F_BACKWARDS      8u   /* walk_env.py:133-136 (episode draw or fixed) */
#define REX_F_DONE          16u   /* last step returned done; must be reset before the next step */
#define REX_F_ENV_GOAL      32u   /* RexGymEnv.env_goal_reached (turn_env.py:338-340) */
#define REX_F_PHASE_WRAP    64u   /* GaitPlanner._phi >= 0.99 after the last loop(): the next loop() latches _last_time
                                     (gait_planner.py:106-107) */

typedef struct RexConfig {
  int32_t abi_version;        /* REX_ABI_VERSION */
  int32_t num_envs;           /* envs in THIS shard */
  int32_t env_index_base;     /* global index of local env 0 (multi-GPU shards): RNG streams are
                                 keyed by the global index so results do not depend on sharding */
  int32_t task;               /* REX_TASK_*   */
  int32_t signal;             /* REX_SIGNAL_* */
  int32_t action_repeat;      /* 5 (walk/turn) or 6 (gallop)  -- walk_env.py:35 */
  int32_t solver_iterations;  /* int(300 / action_repeat)     -- rex_gym_env.py:25,184 */
  float   sim_time_step;      /* control_time_step / action_repeat = 0.001 -- rex_gym_env.py:172 */
  float   motor_kp;           /* 1.0  -- walk_env.py:39 */
  float   motor_kd;           /* 0.02 -- walk_env.py:40 */
  int32_t backwards;          /* -1: draw per episode (reference None), 0/1: fixed -- walk_env.py:133 */
  float   target_position;    /* 0: draw per episode U(1,3) (or -U(2,3) backwards) -- walk_env.py:143 */
  uint64_t seed;              /* Philox key */
  int32_t auto_reset;         /* 1: an env that returns done is reset in the same launch and the
                                 returned observation is the first one of the new episode */
  int32_t max_episode_steps;  /* 0: off; else done at this many steps (LimitDuration, wrappers.py:268) */
  /* reward weights -- rex_gym_env.py:56-59 */
  float   distance_weight, energy_weight, drift_weight, shake_weight;
  float   solver_residual_threshold; /* Bullet's m_leastSquaresResidualThreshold: the PGS sweep loop ends
                                        early once max_row (delta_impulse / invdiag)^2 <= this; PyBullet's
                                        default is 1e-7 and the reference never changes it. 0 = always run
                                        solver_iterations sweeps. */
  /* RexTurnEnv (envs/gym/turn_env.py:129-160): yaw targets; bit 0 of orient_fixed = target_orient is
     given (else drawn U(0.2, 6) per episode), bit 1 = init_orient is given */
  float   target_orient, init_orient;
  int32_t orient_fixed;
  /* RexPosesEnv (envs/gym/poses_env.py:153-192): pose_index -1 = cycle base_y, base_z, roll, pitch, yaw
     per episode with a value drawn in the reference's ranges (rex_gym_env.py:258-265); 0..4 = that
     component held at pose_value (the base_y/base_z/base_roll/base_pitch/base_yaw kwargs) */
  int32_t pose_index;
  float   pose_value;
  /* 1: fold the reference's per-env wrapper stack into the launch (playground/trainer.py:48-52,
     agents/tools/wrappers.py:183-265): ClipAction to [-1,1], RangeNormalize of the action
     ((a+1)/2 (high-low)+low with the env's Box) and of the returned observation (2(o-low)/(high-low)-1).
     d_motor_cmd is unaffected. */
  int32_t range_normalize;
  /* seconds; Rex(pd_latency=, control_latency=) (model/rex.py:59-60,735-763). Non-zero values need
     rex_set_history() before the first reset. */
  float   pd_latency, control_latency;
  /* REX_MARK_BASE / REX_MARK_ARM.  With REX_MARK_ARM the per-env state has rex_state_words() = 69 words (the q, qd
     and overheat blocks grow to 18 motors, every other word keeps its order), d_motor_cmd rows are 18 wide and the
     gallop observation is 4 + 18; the history records of the latency model are 61 words (REX_HISTORY_WORDS_ARM). */
  int32_t mark;
  /* ---- ABI 3 ---- */
  /* GaitPlanner.loop reads WALL-CLOCK time (model/gait_planner.py:108-110: `time.time()`), so the reference's gait
     runs at (wall seconds per simulated second) x the nominal rate of the host it runs on: rendered / real-time
     playback = 1, a host that simulates faster than real time < 1, slower (GUI mode, many worker processes per core)
     > 1.  The gait phase clock here is simulated time x gait_clock_scale.  0 means 1.0. */
  float   gait_clock_scale;
  /* 1: contact rows for the link collision boxes (base, chassis, shoulder, leg, foot boxes of rex.urdf) against the
     ground, next to the toe rows, and for the leg and foot boxes against the boxes of the base body (the reference loads
     the robot with URDF_USE_SELF_COLLISION, model/rex.py:276-281); 0: toes only (the fast path; the boxes of a robot that
     satisfies its env's termination test stay clear of the ground and of each other).
     rex_default_config sets 1 for REX_TASK_POSES -- the env that never terminates and whose roll poses press the base
     into the upper-leg boxes -- and 0 for every other task. */
  int32_t body_contacts;
  /* Rex(observation_noise_stdev=...) (model/rex.py:22,765-769): Gaussian noise added by the sensor getters --
     [0] motor angles, [1] motor velocities, [2] motor torques, [3] base roll/pitch/yaw, [4] base angular rates.
     Every getter call of the reference draws afresh; here every call site of a step draws from the env's Philox
     stream (counter = episode, step, call site).  All 0 (the reference default): no draws. */
  float   noise_stdev[5];
  /* REX_TASK_MIXED: bit t set = task t is in the mix.  Env g runs task_of(g) = the (Philox(seed; g) mod count)-th set
     bit for its whole life (a reference env object never changes class).  All envs use `signal`; the action row is
     as wide as the widest task of the mix, the observation row likewise (narrower tasks leave the tail 0). */
  int32_t task_mix;
  /* Per-reset domain randomisation (the env_randomizer hook, rex_gym_env.py:345-346, turning the knobs of
     Rex.SetBaseMasses / SetLegMasses, model/rex.py:659-692, plus the foot friction): on every reset env g draws
     base-mass scale, leg-mass scale ~ U(mass_scale_lo, mass_scale_hi) and foot friction ~ U(friction_lo, friction_hi)
     from its Philox stream (counter = episode).  lo == hi == 0: off (that quantity keeps its URDF value, or the
     rex_set_body_params entry).  As with changeDynamics(mass=...), inertia tensors keep their load-time values, and
     the reset motion is the nominal robot's (the reference randomises after Rex.Reset). */
  float   mass_scale_lo, mass_scale_hi, friction_lo, friction_hi;
  /* Height the robot is dropped from at reset (ROBOT_INIT_POSITION[terrain_id][2], model/terrain.py:14-20: 0.21 on
     plane / random / maze, 0.85 on mounts, 1.98 on hills).  0 means 0.21. */
  float   init_height;
  /* ---- ABI 4 ---- */
  /* Rex(on_rack=True) (model/rex.py:269-287, rex_gym_env.py:140): the debug mode that hangs the robot on a rack --
     loadURDF(useFixedBase=True) at INIT_RACK_POSITION = [0, 0, 1].  The base neither moves nor turns, the legs swing
     under gravity and the motors; the reset pose is [0, 0, 1] (init_height is ignored) and RexTurnEnv starts at its
     fixed debug yaw 2.1 (turn_env.py:140-143). */
  int32_t on_rack;
  /* ---- ABI 5 ---- */
  /* RexGymEnv(forward_reward_cap=...) (envs/rex_gym_env.py:81,217,525): `forward_reward = min(forward_reward, cap)` in the
     base reward.  +inf (the reference default, what rex_default_config sets): no cap.  NaN is rejected. */
  float   forward_reward_cap;
  /* ---- ABI 6 ---- */
  /* RexReactiveEnv(use_angle_in_observation=False) (envs/gym/gallop_env.py:56,93,344-356,374-377): 1 = the gallop observation is the four
     base words alone (roll, pitch and their rates), without the motor angles; rex_obs_dim() is then 4 for gallop.  0: the reference
     default, 4 + num_motors. */
  int32_t gallop_no_angles;
} RexConfig;

typedef struct RexSim RexSim;

/* Fill *cfg with the reference defaults of `task`/`signal` for `num_envs` envs. */
REX_API int rex_default_config(int task, int signal, int num_envs, RexConfig* cfg);

/* Dimensions implied by a config (action/observation vector lengths of the reference env). */
REX_API int rex_action_dim(const RexConfig* cfg);
REX_API int rex_obs_dim(const RexConfig* cfg);
/* Motors (12 / 18) and per-env state words (REX_STATE_WORDS / 69) of the config's mark. */
REX_API int rex_num_motors(const RexConfig* cfg);
REX_API int rex_state_words(const RexConfig* cfg);

/* Create a simulator on HIP device `device`. `d_state` is a caller-owned device buffer of
 * rex_state_words(cfg) * num_envs float32 words; the library never allocates per-env memory.
 * Computes the settled reset snapshot (rex.py:314-323: 100 + 500 substeps holding the init
 * pose) once, on the device, with the same kernels. */
REX_API int rex_create(const RexConfig* cfg, int device, float* d_state, void* stream, RexSim** out);
REX_API int rex_destroy(RexSim* sim);

/* terrain_type='random' (model/terrain.py:32-54): install a pool of k heightfields. d_heights [k][256*256] float32
 * raw vertex heights in the reference's layout (data[i + j*256], i along x; 5 cm cells centred on the origin),
 * d_mids [k] = (min+max)/2 of each field (Bullet centres the shape there).  Caller-owned device buffers that must
 * outlive the sim.  Each episode of env g uses field (g + 977*episode) mod k; the reset motion is re-run once per
 * field (one settled snapshot each).  k = 0 returns to the flat plane.  Call before rex_reset. */
REX_API int rex_set_terrain(RexSim* sim, const float* d_heights, const float* d_mids, int k, void* stream);

/* Any other heightfield terrain (the reference's 'hills' csv and 'mounts' / 'maze' png fields, model/terrain.py:55-78,
 * whose files live in the pip package pybullet_data and are not part of rex-gym): a pool of k fields of nx x ny vertex
 * heights IN METRES (meshScale z already applied), laid out like rex_set_terrain's (data[ix + iy*nx], ix along x),
 * vertex spacing cell_x / cell_y (meshScale x / y), the grid centred on (origin_x, origin_y).  d_mids[k] = the raw
 * height that ends up at world z = 0: Bullet centres a heightfield shape on the middle of its height range and the
 * reference then places the body at some z0 (terrain.py:64,75), so d_mids[i] = (min_i + max_i) / 2 - z0.  The z = 0
 * ground box of plane.urdf stays underneath, as in the reference.  Everything else as rex_set_terrain. */
REX_API int rex_set_heightfield(RexSim* sim, const float* d_heights, const float* d_mids, int k, int nx, int ny,
                                float cell_x, float cell_y, float origin_x, float origin_y, void* stream);

/* Domain randomisation hooks (the knobs an env_randomizer turns: Rex.SetBaseMasses / SetLegMasses, model/rex.py:659-692;
 * the reference has no friction setter).  d_params: caller-owned device array [3][num_envs], word-major:
 * base-link mass scale, leg-link mass scale, foot friction coefficient; read on every step (so the caller may rewrite
 * entries when it resets envs).  As in Bullet's changeDynamics(mass=...), only masses change: the inertia tensors stay
 * the ones computed at load.  NULL restores (1, 1, 0.5). */
REX_API int rex_set_body_params(RexSim* sim, const float* d_params);

/* The actuator half of the randomisation hooks: the knobs of the reference's MotorModel (model/motor.py:40-74: set_voltage,
 * set_viscous_damping, set_strength_ratios, set_motor_gains) per env.
 * Per-env actuator parameters, read by every step: caller-owned device array [4 + num_motors][num_envs], word-major like d_state:
 * row 0 battery voltage [V] (motor.py MOTOR_VOLTAGE), 1 viscous damping, 2 kp, 3 kd, 4 + m strength ratio of motor m (order of
 * mark_constants).  NULL restores the nominal motor (32 V, 0, RexConfig.motor_kp / motor_kd, 1).  The reset motion is the
 * nominal robot's, as with rex_set_body_params.  In the order of motor.py:116-143: observed = clip(KT pwm V / R), net voltage
 * = clip(pwm V - (KT + damping) qd_true, +-50), the current table, actual torque *= strength -- the overheat protection
 * (rex.py:603) sees the torque after the strength ratio.  Not offered together with the debug event trace (rex_set_event_trace):
 * whichever of the two is set second returns REX_EINVAL. */
REX_API int rex_set_motor_params(RexSim* sim, const float* d_params);

/* Per-reset draws inside the launch (what an env_randomizer would do after Rex.Reset): on every episode start env g draws
 * each quantity ~ U(lo, hi) from its Philox stream; lo == hi == 0: that quantity is not drawn (it keeps its nominal value, or its
 * rex_set_motor_params entry).  strength_per_motor: 1 = one draw per motor, 0 = one per env for all its motors.
 * NULL: off.  REX_EINVAL for lo > hi, negative bounds, a zero upper voltage bound with a non-zero lower one, NaN.
 * The draws are a pure function of (seed, GLOBAL env index, episode ordinal) -- they do not depend on sharding, on the envs
 * per wave or on the segment length, nothing is stored, and they work with auto_reset and inside segment launches -- and use
 * Philox counter words of their own: a rollout with mass / friction ranges is the same with and without them. */
typedef struct RexMotorRandom { float strength_lo, strength_hi, voltage_lo, voltage_hi, damping_lo, damping_hi,
                                      kp_lo, kp_hi, kd_lo, kd_hi; int32_t strength_per_motor; } RexMotorRandom;
REX_API int rex_set_motor_randomization(RexSim* sim, const RexMotorRandom* r);

/* The parameters in effect for every env's CURRENT episode, same layout, to a caller-owned device buffer (one small launch). */
REX_API int rex_get_motor_params(RexSim* sim, float* d_out, void* stream);

/* Debug: trace the discrete events of the restated stepSimulation.  d_trace: caller-owned device buffer uint32 [3][num_envs]
 * (NULL switches the trace off, the default; the caller zeroes it).  While set, every substep folds into word [0][i] of env i
 * which toe points are within the contact breaking distance, the heightfield facet under each of them (under the toe end's
 * centre and under the contact point, and the branch btPlaneSpace1 takes for its friction directions), and which joint / arm
 * bounds are reached -- and every control step the controller's flags and gait latches; into word [1][i] the env's solver sweep
 * count; into word [2][i] the same events as [0] without the arm's bounds (mark arm commands three arm joints beyond their
 * bounds: those rows switch with the last bit of the joint angle).  The words are chained hashes: two runs (or this library and the CPU oracle, which folds the same words the same
 * way) agree on an env's word exactly as long as they took every such decision alike -- what separates their trajectories
 * then is continuous round-off, not a contact that switched.  One read-modify-write of three words per substep; off in
 * production and in bench.py. */
REX_API int rex_set_event_trace(RexSim* sim, uint32_t* d_trace);

/* Observation-history ring for the latency model (Rex._observation_history, deque(maxlen=100) of 43-vectors:
 * q, qd, observed torque, base quaternion, base angular velocity; model/rex.py:122,717-763).  d_history: caller-owned
 * device buffer of REX_HISTORY_LEN * REX_HISTORY_WORDS (_ARM for mark 'arm': 61-vectors) * num_envs float32, laid out
 * [slot][word][env].  Required only
 * when pd_latency or control_latency is non-zero (without a latency the delayed observation is the newest one and the
 * buffer is not used).  The latency model also runs through the reset motion (rex.py:309-323): every reset, by call or
 * in-launch, restores an env's ring to the 100 observations the reset motion leaves behind, so that an episode starts
 * exactly as the reference's does. */
#define REX_HISTORY_LEN 100
#define REX_HISTORY_WORDS 43       /* mark 'base': 3 x 12 + 7 */
#define REX_HISTORY_WORDS_ARM 61   /* mark 'arm':  3 x 18 + 7 */
REX_API int rex_set_history(RexSim* sim, float* d_history);

/* Reset envs. d_indices == NULL: all envs. Else n int32 env indices (device).  Writes the first
 * observation of each reset env to d_obs[row * obs_dim] where row = position in d_indices (or the
 * env index when d_indices is NULL).  Mirrors RexWalkEnv.reset (walk_env.py:125-154). */
REX_API int rex_reset(RexSim* sim, const int32_t* d_indices, int n, float* d_obs, void* stream);

/* One env.step() for every env (rex_gym_env.py:369-414):
 *   d_action [N, action_dim] in  -- raw env action (NOT range-normalised)
 *   d_obs    [N, obs_dim]    out
 *   d_reward [N]             out
 *   d_done   [N] uint8       out
 *   d_motor_cmd [N, 12]      out, nullable -- info['action'], the 12 motor targets
 */
REX_API int rex_step(RexSim* sim, const float* d_action, float* d_obs, float* d_reward,
             uint8_t* d_done, float* d_motor_cmd, void* stream);

/* A rollout SEGMENT in one launch: num_steps consecutive env.step() calls for every env, for a caller that already holds the actions
 * of the whole segment (open-loop rollouts: random-action throughput runs, replayed action tapes, a policy that acts on a stale
 * observation by design).  Step t reads d_action[t] and writes d_obs[t], d_reward[t], d_done[t], d_motor_cmd[t]; the blocks are
 *   d_action [T, N, action_dim]   d_obs [T, N, obs_dim]   d_reward [T, N]   d_done [T, N] uint8   d_motor_cmd [T, N, num_motors] (nullable)
 * and the results are BIT-IDENTICAL to T calls of rex_step on the slices (tests/test_gpu_parity.py::
 * test_segment_launch_is_bit_identical_to_single_steps): the same step code runs T times, an env's state staying in registers in
 * between.  What it buys: a launch ends with its slowest wave; stepping one by one pays the slowest wave of EVERY step (a freshly
 * reset or fallen robot that runs into the solver's sweep cap), a segment pays the largest SUM over a wave's steps.  It replaces
 * nothing of the reference's surface (env.step() stays one rex_step): the reference has no counterpart -- its envs step one
 * action at a time (rex_gym_env.py:369).  Envs that finish an episode inside the segment are reset in the launch when the sim was
 * created with auto_reset, exactly as rex_step does; sims that regroup their envs between steps regroup between segments.
 * num_steps * N * max(action_dim, obs_dim, num_motors) must stay below 2^31. */
REX_API int rex_step_segment(RexSim* sim, int num_steps, const float* d_action, float* d_obs, float* d_reward,
             uint8_t* d_done, float* d_motor_cmd, void* stream);

/* ---- ABI 6: the actor inside the launch -- closed-loop rollouts, one launch per step or per segment ----
 * The reference's rollout is `action = algo.perform(prevob)` -> `batch_env.simulate(action)` every step (agents/tools/simulate.py:
 * 57-76, agents/ppo/algorithm.py:105-134): a policy in the loop, so the actions of step t + 1 do not exist before step t has returned
 * its observation and rex_step_segment cannot serve it.  rex_step_policy / rex_step_segment_policy evaluate the actor of the
 * reference's agents INSIDE the step kernel: the observ filter (agents/ppo/normalize.py:47-66: centre, scale, clip -- with the
 * statistics the caller hands in, frozen for the launch), the network every shipped config uses (agents/scripts/networks.py:66-110
 * ForwardGaussianPolicy: two ReLU layers, tanh mean layer, a free logstd vector; configs.py:29-34) and the Gaussian sample of
 * `network.policy.sample` (Philox keyed by seed, global env index, episode, step: a rollout is a pure function of the seeds and the
 * weights, whatever the sharding or the segment length).
 * The arrays are caller-owned DEVICE buffers; rex_set_policy SNAPSHOTS them (a packing kernel on `stream`, into a library-owned
 * buffer laid out for the kernels: rex_gym_amd/csrc/rex_policy.h), so they only have to stay valid until the stream has passed that
 * point, and a learner that has updated its weights or its filter statistics calls rex_set_policy again.  Weight matrices are
 * input-major: d_w1[k * hidden1 + j] = the weight from input k to unit j (the transpose of a torch.nn.Linear weight; the layout
 * of a TF1 `fully_connected/weights` variable).
 * Needs range_normalize = 1 in the sim's config -- the reference's agents always act through RangeNormalize + ClipAction
 * (playground/trainer.py:48-52): the sampled action is clipped to [-1, 1] and mapped to the env's Box inside the launch, a fused
 * path has no Box test to fail -- a single-task sim (not REX_TASK_MIXED), toes-only contact rows (body_contacts = 0), no event trace. */
typedef struct RexPolicy {
  int32_t obs_dim, action_dim;        /* must equal rex_obs_dim / rex_action_dim of the sim's config */
  int32_t hidden1, hidden2;           /* units of the two ReLU layers (configs.py:31: 200, 100); obs_dim + 12 + hidden1 + hidden2 floats
                                         (each term rounded up to a multiple of 4) per env must fit the kernel's contact-row region of
                                         LDS (448 for mark base up to 8 192 envs) */
  const float* d_w1; const float* d_b1;   /* [obs_dim][hidden1], [hidden1] */
  const float* d_w2; const float* d_b2;   /* [hidden1][hidden2], [hidden2] */
  const float* d_w3; const float* d_b3;   /* [hidden2][action_dim], [action_dim]: the mean layer, tanh on top */
  const float* d_logstd;                  /* [action_dim] */
  const float* d_obs_mean;                /* [obs_dim], nullable (with d_obs_scale): no observ filter */
  const float* d_obs_scale;               /* [obs_dim]: 1 / (std + 1e-8) of the filter (normalize.py:60-62) */
  float   obs_clip;                       /* 5 (algorithm.py:48-52) */
  int32_t sample;                         /* 1: action = mean + exp(logstd) * N(0, 1) (training); 0: action = mean (evaluation) */
  uint64_t seed;                          /* Philox key of the samples */
} RexPolicy;
/* Install the policy (validates the dimensions against the sim, packs the arrays on `stream`); NULL removes it. */
REX_API int rex_set_policy(RexSim* sim, const RexPolicy* policy, void* stream);

/* One closed-loop env.step() for every env: action = perform(d_obs_in), then the step.
 *   d_obs_in [N, obs_dim]     in  -- the observation the envs returned last (rex_reset, or the previous step's d_obs)
 *   d_action [N, action_dim]  out -- the action the policy took, as the agent's memory stores it (BEFORE ClipAction / RangeNormalize)
 *   d_mean   [N, action_dim]  out, nullable -- the policy's mean (algorithm.py:126-133 stores action, mean and logstd)
 *   d_obs, d_reward, d_done, d_motor_cmd  out -- as rex_step (d_obs may NOT alias d_obs_in) */
REX_API int rex_step_policy(RexSim* sim, const float* d_obs_in, float* d_action, float* d_mean, float* d_obs, float* d_reward,
             uint8_t* d_done, float* d_motor_cmd, void* stream);
/* A closed-loop rollout SEGMENT in one launch: step t acts on d_obs[t - 1] (d_obs_in for t = 0) and writes d_action[t], d_mean[t],
 * d_obs[t], d_reward[t], d_done[t], d_motor_cmd[t] -- blocks [T, N, ...] as in rex_step_segment.  BIT-IDENTICAL to T calls of
 * rex_step_policy chained through their observations (tests/test_gpu_policy.py), with what a segment launch buys (rex_step_segment).
 * A caller that keeps one block obs[T + 1, N, obs_dim] passes d_obs_in = obs[0], d_obs = obs[1]: prevob of step t is obs[t]. */
REX_API int rex_step_segment_policy(RexSim* sim, int num_steps, const float* d_obs_in, float* d_action, float* d_mean, float* d_obs,
             float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream);

/* ---- the RECURRENT actor inside the launch (no ABI bump: a new entry point and struct, nothing existing changes) ----
 * The other network of the reference's agents (agents/scripts/networks.py:113-159 RecurrentGaussianPolicy): the last policy layer is
 * tf.contrib.rnn.GRUBlockCell(state_size) on a per-env state h that starts from zero with every episode:
 *   x = relu(W1 filt(obs) + b1);  r, u = sigmoid(Wg [x, h] + bg);  c = tanh(Wc [x, r.h] + bc);  h' = u.h + (1 - u).c;  mean = tanh(W3 h' + b3)
 * (the reset gate acts BEFORE the candidate's product: TensorFlow's cell, not torch.nn.GRU).  rex_step_policy / rex_step_segment_policy
 * run the policy installed LAST by rex_set_policy or rex_set_policy_recurrent; NULL to either removes it.  The weights are snapshotted
 * as rex_set_policy's are.  d_state is NOT: it is the live state [state_size][N] (word-major like the state block), read in front of
 * every perform() and written back behind it, so it must stay valid while the policy is installed.  An env whose episode starts --
 * behind rex_reset (which also zeroes its state rows while a recurrent policy is installed) or behind an in-launch auto-reset -- acts
 * on h = 0; the row of an env whose episode has just ended inside a launch keeps its last h until that next perform().
 * Same restrictions as rex_set_policy.  obs_dim + 12 + hidden1 + 2 state_size floats (each term rounded up to a multiple of 4) per env
 * must fit the kernel's contact-row region of LDS: 200 + 100 does on every variant. */
typedef struct RexRecurrentPolicy {
  int32_t obs_dim, action_dim;            /* must equal rex_obs_dim / rex_action_dim of the sim's config */
  int32_t hidden1, state_size;            /* the ReLU layer in front of the cell; the cell's width, 1..128 (the reference: 100) */
  const float* d_w1; const float* d_b1;   /* [obs_dim][hidden1], [hidden1] */
  const float* d_wg; const float* d_bg;   /* [hidden1 + state_size][2 state_size], [2 state_size]: inputs x then h; units r then u */
  const float* d_wc; const float* d_bc;   /* [hidden1 + state_size][state_size], [state_size]: inputs x then r.h */
  const float* d_w3; const float* d_b3;   /* [state_size][action_dim], [action_dim]: the mean layer on h', tanh on top */
  const float* d_logstd;                  /* [action_dim] */
  const float* d_obs_mean;                /* as RexPolicy */
  const float* d_obs_scale;
  float   obs_clip;
  int32_t sample;
  uint64_t seed;
  float*  d_state;                        /* [state_size][N], caller-owned, live */
} RexRecurrentPolicy;
REX_API int rex_set_policy_recurrent(RexSim* sim, const RexRecurrentPolicy* policy, void* stream);

/* HIP event timing of rex_step launches on their own stream (ms).  rex_set_timing(1): one event pair, read with
 * rex_last_step_ms (synchronises on the launch).  rex_set_timing(2): a ring of event pairs around the last 256 launches,
 * recorded without any host synchronisation between launches (the stream stays full, so a duration is that of the kernel
 * itself, not of an idle queue being refilled); rex_step_times_ms waits for the newest one and returns the last
 * min(max_count, recorded, 256 -- 4096 in mode 3) durations, oldest first -- the return value is their number (< 0: error).
 * rex_set_timing(3): the next 4096 launches are timed on the DEVICE: every workgroup of a launch folds its first / last wall-clock
 * tick (constant 100 MHz counter) into a (min, max) pair, so a duration is first-wave-start to last-wave-end of the kernel
 * alone -- what rocprofv3's kernel trace reports -- with no event or dispatch hand-over in it.
 * In every mode the timed span is the STEP KERNEL's: a sim that regroups its envs every step (single task: from 262 144 envs or
 * REX_REGROUP=1; mixed tasks: beyond one workgroup per SIMD) issues two small sorting launches behind each step kernel on the same
 * stream, and those are NOT inside the span -- compare with the wall clock per step (bench.py reports both: `ms_per_step` next to
 * `roofline.kernel_ms`, and `roofline.regroup_launches_ms` = their difference when the sim regroups). */
REX_API int rex_set_timing(RexSim* sim, int enable);
REX_API int rex_last_step_ms(RexSim* sim, float* ms);
REX_API int rex_step_times_ms(RexSim* sim, float* ms, int max_count);

/* ---- controller-only entry points (parity tests of the controller half) ----
 * n independent problems, row-major device arrays, all float32. */
/* model/kinematics.py:104-142 -- orn[n,3], pos[n,3], frames[n,4,3] (FR,FL,RR,RL) ->
 * angles[n,4,3] in the same leg order (theta, -alpha, -gamma) */
REX_API int rex_ik_solve(int n, const float* d_orn, const float* d_pos, const float* d_frames,
                 float* d_angles, void* stream);
/* model/motor.py:76-143 -- cmd,q,qd,qd_true [n] -> actual, observed torque [n] */
REX_API int rex_motor_torque(int n, const float* d_cmd, const float* d_q, const float* d_qd,
                     const float* d_qd_true, float kp, float kd,
                     float* d_actual, float* d_observed, void* stream);
/* Controller-only twin of rex_motor_torque with per-problem parameters: d_par [n][5] = kp, kd, voltage, damping, strength. */
REX_API int rex_motor_torque_params(int n, const float* d_cmd, const float* d_q, const float* d_qd, const float* d_qd_true,
                                    const float* d_par, float* d_actual, float* d_observed, void* stream);
/* model/gait_planner.py:96-134 with the phase clock on explicit time `now`.
 * mode: 0 walk, 1 gallop.  d_planner [n,3] = (phi, last_time, alpha) in/out; params[n,6] =
 * (v, angle_deg, w_rot, period, direction, now) -- both float64: the clock values and the phase decide branches and must
 * arrive unrounded (see "Clocks" above); the trajectory arithmetic is float32.  frames_out[n,4,3] float32 (FR,FL,RR,RL). */
REX_API int rex_gait_loop(int n, int mode, double* d_planner, const double* d_params,
                  float* d_frames_out, void* stream);

/* Envs per wavefront of the step kernel this sim launches (4, 8, 16: lane groups; 64: one env per lane).  Chosen from
 * the batch size; the environment variable REX_ENVS_PER_WAVE overrides (tests run every variant through it). */
REX_API int rex_envs_per_wave(const RexSim* sim);

/* How a REX_TASK_MIXED batch is laid out over the wavefronts of the step kernel (host-only, no GPU needed).  An env of a
 * mixed batch keeps the task drawn for it for life, so the library decides once which envs share a wave: chunks of
 * neighbouring envs, sorted by task inside a chunk, every task's run padded to whole waves -- a wave then runs ONE task
 * (wave-uniform action_repeat / sweep cap / action box / reward weights) and the chunks' workgroups are dealt to the XCDs.
 * slots[blk * envs_per_wave + k] = env of slot k of workgroup blk (-1: padding), tasks[blk] = that workgroup's task.
 * (A batch that needs more workgroups than one round of the machine holds is instead regrouped every step: one region of whole
 * waves per task, sorted inside by the solver sweeps of the last step; the per-wave rule -- one task -- is the same.)
 * Returns the number of workgroups (pass NULL buffers to size them), or a negative error. */
REX_API int rex_mixed_slot_map(const RexConfig* cfg, int envs_per_wave, int32_t* slots, int32_t* tasks, int max_blocks);

/* Solver sweeps every env ran in the last rex_step (summed over its substeps; after rex_step_segment: the mean per step over the
 * segment), int32 [num_envs] copied to the caller's
 * device buffer -- the key a batch created under REX_REGROUP=1 is regrouped into waves by (opt-in). */
REX_API int rex_get_sweeps(RexSim* sim, int32_t* d_out, void* stream);

/* Rendering (the reference's RexGymEnv.render(mode="rgb_array"), rex_gym_env.py:416-439): a camera that follows each env's
 * base.  rex_render's picture shows the COLLISION geometry the simulator uses (link boxes, full toe cylinders, the arm's
 * collision cylinders -- csrc/rex_render_gen.h), in the links' URDF material colours, over the z = 0 plane (a two-tone checker)
 * and the env's heightfield.  rex_render_visual draws the URDF's visual meshes instead (opt-in: rex_render_set_visuals).  Bullet's b3ComputeViewMatrixFromYawPitchRoll convention, up axis z:
 * eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) (0, 0, 1); perspective with a VERTICAL field of
 * view fov_deg and aspect width / height.  Angles in degrees. */
typedef struct RexCamera { float distance, yaw_deg, pitch_deg, fov_deg, near_plane, far_plane; } RexCamera;
/* The reference's camera: distance 1.0, yaw 0, pitch -30 (rex_gym_env.py:214-216), fov 60, near 0.1, far 100. */
REX_API int rex_default_camera(RexCamera* cam);
/* Render n envs: output row k shows env d_env_ids[k] (int32 device array of state indices, which the caller keeps in
 * [0, num_envs): they are not clamped).  d_rgb: uint8 [n][height][width][3], row 0 = the top of the image; d_depth (may be
 * NULL): float32 [n][height][width], eye-space distance along the view axis [m], far_plane where nothing is hit; d_seg (may
 * be NULL): int16 [n][height][width], -1 nothing, 0 ground, 1 + b body b (rex_model_gen.h numbering; arm bodies 13..18).
 * One launch on `stream`, no host sync; reads the state, writes only the three buffers.  REX_EINVAL without a launch for
 * n < 1, width or height outside 1..4096, n * width * height * 3 >= 2^31, a null d_rgb or d_env_ids, or a distance,
 * fov or near plane that is not positive (or far_plane <= near_plane). */
REX_API int rex_render(RexSim* sim, const RexCamera* cam, const int32_t* d_env_ids, int n, int width, int height,
                       uint8_t* d_rgb, float* d_depth, int16_t* d_seg, void* stream);
/* The visual meshes of the sim's mark (csrc/rex_visual_gen.h: 23 instances for 'base', 29 for 'arm'), as BVHs built on the
 * host (rex_gym_amd/meshes.py).  Host arrays: nodes [num_nodes][16] dwords (float lo0[3] hi0[3] lo1[3] hi1[3] = both children's
 * boxes, int32 c0 c1, 2 unused; c >= 0 an inner node whose index is greater than its parent's, c < 0 a leaf with
 * ~c = first triangle << 3 | (count - 1)); tris [num_tris][9] floats (v0, v1 - v0, v2 - v0) in metres, in the instance's mesh
 * frame; inst_root [num_inst] (a root node, or -1 for an empty mesh) and inst_box [num_inst][6] (the root's mesh-frame box lo,
 * hi).  REX_EINVAL (message in rex_last_error) for a wrong instance count, out-of-range children or triangles, a node with
 * two parents, or a tree deeper than 32 levels.  Uploads on `stream` and waits for the copy; the sim keeps the device copy
 * (replacing an earlier one) until rex_destroy. */
REX_API int rex_render_set_visuals(RexSim* sim, const float* nodes, int num_nodes, const float* tris, int num_tris,
                                   const int32_t* inst_root, const float* inst_box, int num_inst, void* stream);
/* rex_render over the visual meshes: same arguments, outputs and checks, and the same labels (segment 1 + b for every mesh
 * riding on body b).  REX_EINVAL without a launch when no visuals are set. */
REX_API int rex_render_visual(RexSim* sim, const RexCamera* cam, const int32_t* d_env_ids, int n, int width, int height,
                              uint8_t* d_rgb, float* d_depth, int16_t* d_seg, void* stream);

/* Onboard sensors (csrc/rex_sense.h): what the robot perceives of the ground around it, for n envs in one launch each.
 *
 * A depth sensor rigidly mounted on the BASE body.  pos: the eye in the base frame [m].  fwd / up: the optical axis and the
 * image's up direction as unit vectors in the base frame, orthogonal to each other; right = fwd x up.  Pixel (px, py), row 0 the
 * top: ray = fwd + sx right + sy up, sx = (2 (px + .5) / W - 1) tan(fov/2) W / H, sy = (1 - 2 (py + .5) / H) tan(fov/2)  --
 * rex_render's pixel_ray, with the axes turned by the base's rotation: the value written is the eye-space distance along the
 * optical axis [m] of the first hit in [near_plane, far_plane], far_plane where there is none (rex_render's d_depth). */
typedef struct RexDepthSensor {
  float pos[3], fwd[3], up[3];
  float fov_deg, near_plane, far_plane;   /* vertical field of view */
  int32_t width, height;
  int32_t see_robot;                      /* 1: the robot's own collision primitives (rex_render_gen.h) occlude; 0: ground only */
} RexDepthSensor;
/* The robot walks towards body -x: the eye just in front of the front face, pos (-0.18, 0, 0), looking along -x pitched 30
 * degrees down (fwd (-cos 30, 0, -sin 30), up (-sin 30, 0, cos 30)), fov 60, near 0.02, far 10, 32 x 24, see_robot 1. */
REX_API int rex_default_depth_sensor(RexDepthSensor* s);
/* Row k of d_depth (float32 [n][height][width], row 0 of an image the top) is what the sensor of env d_env_ids[k] sees
 * (int32 device array of state indices, kept in [0, num_envs) by the caller: they are not clamped; NULL: envs 0 .. n - 1, n <=
 * num_envs), over the z = 0 plane and the heightfield of the env's current episode.  One launch on `stream`, no host sync;
 * reads the state, the terrain pool and the heightfield, writes only d_depth.  REX_EINVAL (message in rex_last_error) without a
 * launch for a null s or d_depth, n < 1, width or height outside 1..1024, n * width * height >= 2^29, fov_deg outside (0, 180),
 * near_plane <= 0, far_plane <= near_plane, a non-finite field, | |fwd| - 1 |, | |up| - 1 | or |fwd . up| above 1e-3, or
 * see_robot other than 0 or 1. */
REX_API int rex_sense_depth(RexSim* sim, const RexDepthSensor* s, const int32_t* d_env_ids /* NULL: all envs in order */, int n,
                            float* d_depth /* [n][height][width] */, void* stream);
/* Ground height at K points given in the base's YAW frame (x, y [m]: world = base_xy + Rz(yaw) p, yaw = atan2(R10, R00) of the
 * base rotation, 0 when both vanish).  relative = 0: the ground's world z (the contact code's ground_query: the facet's height
 * over the z = 0 plane, 0 on the plane; and 0 beside the grid's footprint, where the renderer draws the plane too);  relative =
 * 1: base z minus that.  d_points: float32 device array.  Env ids, launch
 * and reads as rex_sense_depth; writes only d_out.  REX_EINVAL without a launch for a null d_points or d_out, n < 1, K outside
 * 1..4096, n * K >= 2^31, or relative other than 0 or 1. */
REX_API int rex_height_scan(RexSim* sim, const float* d_points /* [K][2] */, int K, int relative, const int32_t* d_env_ids, int n,
                            float* d_out /* [n][K] */, void* stream);

/* Body and foot kinematics (csrc/rex_kinematics.h): where every link and every foot of n envs is, how it moves, and how far each
 * foot is from the ground -- what rewards and privileged observations are built from, in one read-only launch.
 *
 * NB = rex_num_bodies(cfg): 13 (mark base) or 19 (mark arm), in the body order of REX_PARENT / REXA_PARENT (csrc/rex_model_gen.h,
 * rex_arm_model_gen.h): body 0 the base, 1 + 3 l .. 3 + 3 l the shoulder, leg and foot link of leg l (front_left, front_right,
 * rear_left, rear_right), 13 .. 18 the arm.  Every member of RexKinematicsOut is a device array of n rows, float32 unless
 * noted, or NULL: a null member is not computed.  World frame unless noted.
 *   link_pos    [n][NB][3]  origin of each link frame
 *   link_quat   [n][NB][4]  its orientation x y z w, unit norm (the sign is not fixed)
 *   link_linvel [n][NB][3]  velocity of that origin;  link_angvel [n][NB][3]  angular velocity of the link.  REX_S_LINVEL is
 *                           the velocity of the base link frame's origin, the point REX_S_POS is integrated with (the base's
 *                           centre of mass lies there); the links' follow by  w_b = w_p + qd_j a_j,  v_b = v_p + w_p x (o_b - o_p)
 *   toe_pos     [n][8][3]   the 8 contact candidates of the physics, point p = 2 leg + e for the two ends e of the toe
 *                           cylinder: the lowest point of the end's rim along the ground normal under the end's centre (the
 *                           centre's projection when the cylinder's axis is parallel to that normal)
 *   toe_vel     [n][8][3]   velocity of the foot link's material point there
 *   toe_dist    [n][8]      the signed distance the contact solver sees: (z - ground height) * normal z at the point, the
 *                           1 mm collision margin included (on the plane: toe_pos z).  Beside a heightfield's footprint the
 *                           ground keeps the height of the grid's border, as it does for the solver
 *   toe_normal  [n][8][3]   the ground's unit normal at the point; (0, 0, 1) on the plane
 *   toe_in_reach [n][8]     uint8, 1 where toe_dist < 0.02 m: the contact breaking threshold that activates the point's rows
 *   base_body   [n][9]      base linear velocity, base angular velocity and the unit gravity direction, all in the BASE frame
 *                           (R0^T v, R0^T w, R0^T (0, 0, -1)) */
typedef struct RexKinematicsOut {
  float *link_pos, *link_quat, *link_linvel, *link_angvel;
  float *toe_pos, *toe_vel, *toe_dist, *toe_normal;
  uint8_t* toe_in_reach;
  float* base_body;
} RexKinematicsOut;
/* Number of bodies of the robot of `cfg`: 13 (mark base) or 19 (mark arm); REX_EINVAL for a null cfg. */
REX_API int rex_num_bodies(const RexConfig* cfg);
/* Row k of every output is env d_env_ids[k] (int32 device array of state indices, kept in [0, num_envs) by the caller; NULL: envs
 * 0 .. n - 1, n <= num_envs).  One launch on `stream`, no host sync; reads the state, the terrain pool and the heightfield of the
 * env's current episode, writes only the arrays of `out` (each needs the alignment of its element and no more: element stores).
 * REX_EINVAL (message in rex_last_error) without a launch for a null
 * sim or out, n < 1, n > num_envs without ids, n * NB * 4 >= 2^31, or an `out` whose members are all NULL. */
REX_API int rex_kinematics(RexSim* sim, const int32_t* d_env_ids /* NULL: envs 0 .. n - 1 */, int n, const RexKinematicsOut* out,
                           void* stream);

/* Rigid-body dynamics readout (csrc/rex_dynamics.h): the equations of motion of n envs at their current state, in one read-only
 * launch -- what model-based controllers, torque feed-forward, momentum rewards and ground-reaction estimates are built from.
 * Mark base only (18 degrees of freedom).
 *
 * The generalized velocity is v[18]: v[0:3] the world linear velocity of the base link frame's origin (REX_S_LINVEL), v[3:6] the
 * world angular velocity of the base (REX_S_ANGVEL), v[6:18] the 12 joint rates in motor order -- the order of link_linvel /
 * link_angvel and of the state words.  The outputs are defined by
 *     M(q) vdot + h(q, v) = S^T tau + sum_p J_p^T f_p        (S selects v[6:18]; f_p is a world force at toe point p)
 * Every member of RexDynamicsOut is a float32 device array of n rows, or NULL: a null member is not computed.
 *   mass_matrix  [n][18][18]   M(q), symmetric; both triangles are written, from one value per pair; blocks that couple two
 *                              different legs are exact zeros
 *   bias         [n][18]       h(q, v): Coriolis, centrifugal and gyroscopic terms plus gravity at the sim's g = 10 m/s^2, on the
 *                              left-hand side: a robot at rest has bias[0:3] = (0, 0, +mass * 10).  The sim's Bullet-style linear
 *                              and angular damping forces are NOT part of it
 *   gravity      [n][18]       h(q, 0)
 *   toe_jacobian [n][8][3][18] toe_vel[p] = J_p v for point p = 2 leg + e of rex_kinematics, the foot link's material point at
 *                              toe_pos[p]:  J_p = [ 1 | -[P - o_0]x | a_j x (P - o_j) for the three joints j of the point's leg ],
 *                              o_0 the base origin, a_j and o_j a joint's world axis and position; the columns of the other
 *                              three legs are written as zeros
 *   com          [n][6]        centre of mass: world position, world velocity
 *   momentum     [n][6]        linear momentum, then angular momentum about the centre of mass, world axes
 *   mass         [n]           total mass with the env's scales
 * Masses are the ones the step uses in the env's current episode: REX_MASS times the base / leg mass scale of the explicit
 * rex_set_body_params table or of the per-reset draws of mass_scale_range.  The scales touch the masses only: every link's
 * rotational inertia about its own centre of mass stays the model's constant, for the base as for the legs, as in the step
 * (Bullet keeps the inertia tensors computed at load time).  The on_rack anchor is not part of the readout. */
typedef struct RexDynamicsOut {
  float *mass_matrix;
  float *bias;
  float *gravity;
  float *toe_jacobian;
  float *com;
  float *momentum;
  float *mass;
} RexDynamicsOut;
/* Rows, launch and reads as rex_kinematics, plus the env's mass scales; writes only the arrays of `out`.  mass_matrix and
 * toe_jacobian are written in 16-byte chunks and must be 16-byte aligned (every row of either is a multiple of 16 bytes); the other
 * arrays need the alignment of a float.  REX_EINVAL (message in rex_last_error) without a launch for a null sim or out, n < 1,
 * n > num_envs without ids, n * 8 * 3 * 18 >= 2^31, an `out` whose members are all NULL, a mass_matrix or toe_jacobian that is not
 * 16-byte aligned, or a sim of mark arm. */
REX_API int rex_dynamics(RexSim* sim, const int32_t* d_env_ids /* NULL: envs 0 .. n - 1 */, int n, const RexDynamicsOut* out, void* stream);

/* Solves with the mass matrix (csrc/rex_dynamics_solve.h): the equation above solved on the device, one launch, M(q) never written
 * out -- a block elimination over its structure (the 6 x 6 base block, four 3 x 3 leg blocks that do not couple to each other,
 * the 3 x 6 couplings).  Mark base only.  Rows, ids and launch as rex_dynamics: no host sync; v, the order of its 18 components,
 * the masses and the toe points are rex_dynamics'.
 *
 *   rex_dynamics_solve    x [n][K][18] = M(q)^-1 rhs [n][K][18]: K right-hand sides per row.  d_x may be d_rhs itself (in place).
 *                         The Delassus matrix J M^-1 J^T of the toe points is K = 24 with rhs = the rows of toe_jacobian.
 *   rex_forward_dynamics  vdot [n][18] = M^-1 (S^T tau + sum_p J_p^T f_p + w - h(q, v)) for the load: joint torques tau [n][12],
 *                         world forces f_p [n][8][3] at the toe points p = 2 leg + e, and a base wrench w [n][6] -- a world force
 *                         at the base origin, then a world moment: rows 0..5 of the equation.  A NULL member is zero (all three
 *                         NULL: free fall from the current state); the ground is queried only when toe forces are given.
 *   rex_apply_impulse     the same load as impulses [N s, N m s]:  dv [n][18] = M^-1 (S^T j + sum_p J_p^T p_p + w), written to d_dv
 *                         unless that is NULL, and ADDED to REX_S_LINVEL, REX_S_ANGVEL and REX_S_QD of each row's env in the
 *                         caller-owned state (one float add per word; no other word is touched): an external push between two
 *                         control steps.  The rows must name distinct envs -- the caller's duty, not checked here (two rows of one
 *                         env race on its words).
 * Like `bias`, the forward and the impulse form leave out what the step adds to the rigid-body equation: the Bullet-style damping,
 * joint-limit rows, contact rows and the on_rack anchor.
 * REX_EINVAL (message in rex_last_error) without a launch for: a null sim, rhs, x, vdot, load or impulse; n < 1; n > num_envs without
 * ids; K < 1; n * K * 18 >= 2^31; d_rhs and d_x that overlap without being equal; an impulse whose three members are all NULL; a sim
 * of mark arm; rex_apply_impulse on an on_rack sim (its base hangs on the anchor). */
typedef struct RexDynamicsLoad { const float *joint, *toe, *base; } RexDynamicsLoad;   /* [n][12], [n][8][3], [n][6]; NULL = zero */
REX_API int rex_dynamics_solve(RexSim* sim, const int32_t* d_env_ids /* NULL: envs 0 .. n - 1 */, int n, int K, const float* d_rhs, float* d_x,
                               void* stream);
REX_API int rex_forward_dynamics(RexSim* sim, const int32_t* d_env_ids, int n, const RexDynamicsLoad* load, float* d_vdot, void* stream);
REX_API int rex_apply_impulse(RexSim* sim, const int32_t* d_env_ids, int n, const RexDynamicsLoad* impulse, float* d_dv /* nullable */,
                              void* stream);

/* The contact solve (csrc/rex_contact_solve.h): ground reaction forces at the toe points, joint-limit torques and the
 * contact-consistent next velocity of every row's env -- ONE substep of the step's physics restated for the current state and solved
 * in a read-only launch of its own.  The step, settle and reset kernels are not involved and the state is never written.  Mark base
 * only.  Rows, ids and launch as rex_dynamics: no host sync; v, the order of its 18 components, M, h, J_p, the masses (with the
 * env's scales) and the toe points p = 2 leg + e are rex_dynamics'; mu is the env's toe friction.
 *   1. Free velocity  v* = v + dt M^-1 (S^T tau - h(q, v) - d(q, v)),  d the generalized force of the sim's per-link damping: on every
 *      body a force m (0.04 + 0.04 |vc|) vc at the centre of mass and a moment I w (0.04 + 0.04 |w|).  damping = 0 leaves d out: the
 *      result then sits on the equation of rex_forward_dynamics.
 *   2. Rows, in the solver's order.  (a) Joint-limit rows j = 0..11, only for a joint beyond its bound, gap = min(q - lower,
 *      upper - q) < 0:  J = sgn e_j, 0 <= lambda, rhs = (-gap 0.2 / dt - sgn v*_j) / diag.  (b) Normal rows of the toe points in reach
 *      (dist < 0.02 m), in order of p:  J = n^T J_p, 0 <= lambda, rhs = (poserr + velerr) / diag with velerr = -J v* - (dist > 0 ?
 *      dist / dt : 0) and poserr = dist > 0 ? 0 : -dist 0.2 / dt.  (c) Friction rows in order of p, two per point:  J = t1^T J_p,
 *      t2^T J_p with (t1, t2) Bullet's btPlaneSpace1 of n, rhs = -(J v*) / diag, |lambda| <= mu lambda_n of the normal row's current
 *      value.  diag = J M^-1 J^T.
 *   3. Projected Gauss-Seidel from lambda = 0: each sweep visits the rows in that order, dl = rhs - (J dv) / diag clamped so that
 *      lambda stays in its bounds, dv += M^-1 J^T dl; it stops after `iterations` sweeps or after the first sweep whose largest
 *      (dl diag)^2 is <= residual_threshold.
 *   4. v_next = clamp(v* + dv, +-100).
 * What it takes for the result to be the step's own forces: the step draws tau from the motor model anew in every substep
 * (rex_motor_torque_params reproduces it); the state holds no last torque, so the caller supplies tau.  Link-box rows
 * (body_contacts) and the on_rack anchor are not restated: such sims are refused.
 * Outputs (any member may be NULL; each needs the alignment of its element):  toe_force, the world force on the foot at the toe
 * point (rex_kinematics' toe_pos), N = impulse / dt, 0 for a point out of reach;  toe_lambda, the (normal, t1, t2) impulses, N s;
 * limit_torque, the signed joint torque of the limit rows, N m;  v_next;  sweeps, the env's own sweep count.
 * v_next = v + dt vdot with vdot = rex_forward_dynamics(tau + limit_torque, toe_force) when damping = 0 and no component is clamped.
 * REX_EINVAL (message in rex_last_error) without a launch for: a null sim, in or out; n < 1; n > num_envs without ids; n * 24 >=
 * 2^31; an `out` whose members are all NULL; iterations > 1000; a non-finite dt or threshold; a sim of mark arm, on_rack or with
 * body_contacts. */
typedef struct RexContactSolveIn {
  const float* tau;            /* [n][12] joint torques, or NULL: zero */
  float dt;                    /* <= 0: cfg.sim_time_step */
  int32_t iterations;          /* <= 0: cfg.solver_iterations */
  float residual_threshold;    /* < 0: cfg.solver_residual_threshold; 0: always `iterations` sweeps */
  int32_t damping;             /* 1: with the sim's damping forces (what the step does); 0: without */
} RexContactSolveIn;
typedef struct RexContactSolveOut {     /* any member may be NULL */
  float* toe_force;            /* [n][4][2][3] world force on the foot at kinematics' toe_pos, N = impulse / dt; 0 out of reach */
  float* toe_lambda;           /* [n][4][2][3] (normal, t1, t2) impulses, N s */
  float* limit_torque;         /* [n][12] signed joint torque of the limit rows, N m */
  float* v_next;               /* [n][18] */
  int32_t* sweeps;             /* [n] */
} RexContactSolveOut;
REX_API int rex_contact_solve(RexSim* sim, const int32_t* d_env_ids, int n, const RexContactSolveIn* in, const RexContactSolveOut* out, void* stream);

/* Candidate rollouts (csrc/rex_rollout.h): for every row's env, K candidate command sequences simulated over T control steps of
 * `repeat` substeps each, from the env's current state, in ONE read-only launch -- what a sampling planner (MPPI, CEM), a safety check
 * before an action is applied or the scoring of a policy against its alternatives asks for.  The sim's state is never written; the
 * step, settle and reset kernels are not involved.  Mark base only; toe rows and joint-limit rows only.  Rows, ids, stream and "no
 * host sync" as rex_contact_solve; output row (k, c) is env d_env_ids[k] (or env k) under candidate c.
 * One substep of a row, on its private copy W of the state's words 0..36 (position, quaternion, linear and angular velocity, joint
 * angles and rates):
 *   1. Torque.  `targets`: the motor model of the step's substep (rex_motor_torque / rex_motor_torque_params state it) on (cmd, q, qd,
 *      qd) of W -- with the config's gains, or the env's actuator parameters of its current episode when a table or ranges are set
 *      (rex_set_motor_params, rex_set_motor_randomization) -- multiplied by the env's enable bit in REX_S_MOTOR_EN as it stands at the
 *      call.  `tau`: as given.  The command of control step t holds for its `repeat` substeps; the torque is drawn anew in each.
 *   2. Contact solve.  v_next of rex_contact_solve with damping = 1 on W under that torque, with the env's mass scales, toe friction
 *      and terrain field of its current episode; dt, iterations and residual_threshold as RexContactSolveIn.
 *   3. Integrator.  The step's: semi-implicit Euler with the NEW velocities -- pos += dt lin, q += dt qd, the quaternion turned by
 *      exp(dt w / 2) and normalised.
 * Not advanced: the overheat counters and the motor mask (a motor that would overheat during the rollout keeps drawing torque),
 * controller and gait words, step and episode counters (no reset, no done), sensor noise.
 * Outputs (any member may be NULL, not all):  state, W after the last substep;  trajectory, W after every control step;
 * foot_contact, 1 where either end of the leg's toe carries a positive normal impulse in the control step's last substep;  sweeps,
 * the solver sweeps summed over the row's substeps.
 * REX_EINVAL (message in rex_last_error) without a launch for: a null sim, in or out; both or neither of targets and tau; an `out`
 * whose members are all NULL; n < 1; n > num_envs without ids; candidates < 1, steps < 1 or steps * repeat > 4096; an output of 2^31
 * elements or more; iterations > 1000; a non-finite dt or threshold; a sim of mark arm, with on_rack, with body_contacts or with the
 * latency model on (pd_latency or control_latency > 0: the observation ring is not restated). */
typedef struct RexRolloutIn {
  const float* targets;        /* [n][K][T][12] motor angle commands, rad (what d_motor_cmd / info['action'] hold), or NULL */
  const float* tau;            /* [n][K][T][12] joint torques, N m, or NULL -- exactly one of the two */
  int32_t candidates;          /* K >= 1 */
  int32_t steps;               /* T >= 1 control steps */
  int32_t repeat;              /* substeps per control step; <= 0: cfg.action_repeat */
  float dt;                    /* <= 0: cfg.sim_time_step */
  int32_t iterations;          /* <= 0: cfg.solver_iterations */
  float residual_threshold;    /* < 0: cfg.solver_residual_threshold; 0: always `iterations` sweeps */
} RexRolloutIn;
typedef struct RexRolloutOut {   /* any member may be NULL, not all */
  float* state;                /* [n][K][37]    words 0..36 of the state after the last substep */
  float* trajectory;           /* [n][K][T][37] the same after every control step */
  uint8_t* foot_contact;       /* [n][K][T][4]  a positive normal impulse at either end of the leg's toe in the control step's last substep */
  int32_t* sweeps;             /* [n][K]        solver sweeps summed over the substeps */
} RexRolloutOut;
REX_API int rex_rollout(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutIn* in, const RexRolloutOut* out, void* stream);

/* Candidate rollouts from given states, under base pushes and per-candidate bodies: rex_rollout with up to three per-row inputs in place
 * of what the row would take from its env -- what beam or tree search over `state`, horizons past 4096 substeps (chain the calls),
 * rollouts from an estimated or perturbed state (finite-difference linearisation), "does this action survive a shove" and the scoring
 * of candidates under several mass and friction draws ask for.  The same launch shape, substep, outputs and "no host sync" as
 * rex_rollout; row (k, c) is env d_env_ids[k] (or env k) under candidate c.  Every member of `from` is a float32 device array or NULL;
 * with all three NULL the call computes what rex_rollout computes.
 *   init_state   W of row (k, c) starts as these 37 words -- position, quaternion x y z w, linear and angular velocity, joint angles and
 *                rates, the layout of `state` and `trajectory` -- instead of the env's words 0..36.  Taken as given: the quaternion is not
 *                normalised, nothing is checked, nothing is read back on the host.  Feeding a call's `state` output to the next call
 *                continues the rollout bit for bit: W is emitted as it is held.
 *   base_wrench  a world force at the base origin, N, then a world moment, N m -- the convention of rex_forward_dynamics' base wrench --
 *                for control step t of row (k, c), held over its `repeat` substeps.  It enters step 1 of the substep,
 *                v* = v + dt M^-1 (S^T tau + w - h - d); the rows and the sweeps follow from v* as before.  A wrench of zeros changes no bit.
 *   body         base mass scale, leg mass scale and toe friction of row (k, c), in place of the env's (rex_set_body_params'
 *                triple: the scales touch the masses only, as everywhere else; mu is the friction of the row's toe rows).
 * Everything else a row reads stays its env's at the call: the terrain field of the env's episode, its actuator parameters, its motor
 * enable bits, and whichever of the three is NULL.
 * The states are the caller's, so the kernel was read for arbitrary float input: the one address formed from W, the heightfield lookup
 * under the toe points, clamps its grid coordinates (a NaN lands on cell 0), every table is addressed by launch constants and every
 * loop is bounded by steps, repeat and iterations.  A bad row -- non-finite, huge, a zero quaternion -- yields garbage in that row only.
 * REX_EINVAL (message in rex_last_error) without a launch for everything rex_rollout refuses, and for a NULL `from`.  The three inputs
 * count towards the 2^31-element limit (each is smaller than `trajectory`'s n * K * T * 37, which is held below 2^31 whether it is
 * asked for or not). */
typedef struct RexRolloutFrom {      /* any member may be NULL; all NULL: rex_rollout */
  const float* init_state;           /* [n][K][37] words 0..36 each row starts from, instead of the env's state */
  const float* base_wrench;          /* [n][K][T][6] world force at the base origin and moment, N / N m, held over the control step's substeps */
  const float* body;                 /* [n][K][3] base mass scale, leg mass scale, toe friction of the row, instead of the env's */
} RexRolloutFrom;
REX_API int rex_rollout_from(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutIn* in, const RexRolloutFrom* from,
                             const RexRolloutOut* out, void* stream);

/* The env's controller as a readout (csrc/rex_command.h): for row (k, c) = (env d_env_ids[k] or env k, candidate c) ONE control step of
 * the env's own controller and nothing else -- what rex_step does between loading the env and its first substep: ClipAction plus
 * RangeNormalize when cfg.range_normalize is set, the task's command (walk, gallop, turn: ik and ol; standup; poses) with its goal,
 * brake and hold latches, then the gait planner and the inverse kinematics.  One small read-only launch that calls the step kernels' own
 * command functions in their lane-group form (a lane per row and leg); no host sync; the sim's state is never written.
 *   d_actions   [n][K][A], A = rex_action_dim(cfg): taken as given, as rex_step takes them (no Box check)
 *   d_state     [n][K][37] words 0..36 of the row, or NULL: the env's.  Only position and quaternion are read (the goal tests)
 *   d_ctrl      [n][K][8] the row's controller words REX_S_PHI .. REX_S_STEPS (37..44) as the state block holds them -- raw 32-bit
 *               words, the ints (REX_S_LASTT, REX_S_ENDTIME, REX_S_FLAGS, REX_S_STEPS) as bit patterns --, or NULL: the env's
 *   d_targets   [n][K][12] what d_motor_cmd / info['action'] of the step would hold, or NULL
 *   d_ctrl_next [n][K][8] the eight words as the step would store them for an env whose step returns done = 0: with the epilogue's
 *               REX_S_STEPS + 1 and REX_S_TARGET = fabsf(target); REX_F_DONE is never set.  Or NULL (not both outputs)
 * Read from the env besides: REX_S_EPISODE and the config.  The controller's clock is the env's, REX_S_STEPS x cfg.action_repeat x
 * cfg.sim_time_step.  Sensor noise is not drawn, as in every readout: the turn task's goal test sees the row's true yaw.
 * The inputs are the caller's, so the kernel was read for arbitrary float input: no address is formed from an action, a state or a
 * controller word -- rows are addressed by the row index and the env id, the command functions index their tables by leg and by launch
 * constants, flag bits and (int)aux only select between constants.  A bad row -- a non-finite action, controller words that no step
 * wrote -- yields garbage in that row only.
 * REX_EINVAL (message in rex_last_error) without a launch for: NULL d_actions; both outputs NULL; candidates < 1; a null sim; n < 1;
 * n > num_envs without ids; n * candidates * 37 >= 2^31; a sim of mark arm, of REX_TASK_MIXED or with the latency model on (the turn
 * goal test would read the observation ring). */
REX_API int rex_command(RexSim* sim, const int32_t* d_env_ids, int n, int candidates, const float* d_actions, const float* d_state,
                        const float* d_ctrl, float* d_targets, float* d_ctrl_next, void* stream);

/* Action-space rollouts: where row (k, c) is after T control steps under ACTIONS of the env's own action space (2 numbers for walk-IK
 * and turn, 4 or 8 for the open-loop gaits) -- what shielding a policy action, sampling in the action space instead of 12 x T motor
 * targets and scoring a policy against alternatives ask for.  The controller is closed-loop through its latches (the goal tests read
 * base x or yaw), so targets cannot be precomputed: ONE call enqueues, for t = 0 .. T-1, rex_command on the row's current (state, ctrl)
 * and actions[t], then rex_rollout_from with steps = 1, those targets and the previous step's state -- 2 T launches on `stream`, no host
 * sync, no copies.  The physics IS rex_rollout_from's kernel (a rollout continued from its own `state` is the unsplit rollout bit for
 * bit), the controller IS rex_command's: a single rex_rollout_from launch fed the emitted `targets` reproduces state, trajectory and
 * foot_contact bit for bit.  (A controller inside the rollout launch was tried and not merged: docs/HISTORY.md.)
 * Every per-step array is TIME-MAJOR, the convention of rex_step_segment, so each launch reads and writes a contiguous slice:
 *   in->actions [T][n][K][A];  from->base_wrench [T][n][K][6] (time-major HERE, unlike rex_rollout_from);  from->init_state [n][K][37]
 *   and from->body [n][K][3] as in rex_rollout_from;  in->ctrl [n][K][8] the controller words each row starts from, or NULL: the env's.
 * candidates, steps, repeat, dt, iterations, residual_threshold: RexRolloutIn's, steps x repeat <= 4096.  repeat and dt are the
 * PHYSICS': the controller's clock stays the env's (cfg.action_repeat x cfg.sim_time_step per control step) whatever they are.
 * Outputs (any member may be NULL, not all):  state [n][K][37] and ctrl [n][K][8] after the last step -- feeding them to the next call
 * as from->init_state and in->ctrl continues the rollout bit for bit;  trajectory [T][n][K][37], ctrl_trajectory [T][n][K][8], targets
 * [T][n][K][12], foot_contact [T][n][K][4] per control step;  sweeps [T][n][K] per control step (nothing is summed across launches).
 * Not advanced: the overheat counters and the motor mask, resets, episode counters, sensor noise.  Reward, done and the observation of
 * every control step: rex_rollout_actions_outcome, below.
 * Buffers the caller did not ask for (the state and ctrl ping-pong, one step of targets) live in d_workspace, a device buffer of at
 * least rex_rollout_actions_workspace_bytes(n, candidates) bytes, 4-byte aligned, the caller's (-1 for n < 1, candidates < 1 or
 * n * candidates >= 2^31).
 * REX_EINVAL (message in rex_last_error) before any launch for everything rex_rollout_from and rex_command refuse (with on_rack,
 * body_contacts, the latency model, mark arm, REX_TASK_MIXED), NULL in, from, out or in->actions, an `out` whose members are all NULL,
 * and a NULL or too small workspace. */
typedef struct RexRolloutActionsIn {
  const float* actions;        /* [T][n][K][A] actions of the env's action space, A = rex_action_dim(cfg) */
  const float* ctrl;           /* [n][K][8] controller words REX_S_PHI .. REX_S_STEPS each row starts from, or NULL: the env's */
  int32_t candidates;          /* K >= 1 */
  int32_t steps;               /* T >= 1 control steps */
  int32_t repeat;              /* substeps per control step; <= 0: cfg.action_repeat */
  float dt;                    /* <= 0: cfg.sim_time_step */
  int32_t iterations;          /* <= 0: cfg.solver_iterations */
  float residual_threshold;    /* < 0: cfg.solver_residual_threshold; 0: always `iterations` sweeps */
} RexRolloutActionsIn;
typedef struct RexRolloutActionsOut {   /* any member may be NULL, not all */
  float* state;                /* [n][K][37]    words 0..36 after the last substep */
  float* trajectory;           /* [T][n][K][37] the same after every control step */
  uint8_t* foot_contact;       /* [T][n][K][4]  as RexRolloutOut's, per control step */
  int32_t* sweeps;             /* [T][n][K]     solver sweeps of the control step's substeps */
  float* ctrl;                 /* [n][K][8]     controller words after the last step */
  float* ctrl_trajectory;      /* [T][n][K][8]  the same after every control step */
  float* targets;              /* [T][n][K][12] the motor angle commands the controller emitted */
} RexRolloutActionsOut;
REX_API long long rex_rollout_actions_workspace_bytes(int n, int candidates);
REX_API int rex_rollout_actions(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from,
                                const RexRolloutActionsOut* out, void* d_workspace, long long workspace_bytes, void* stream);

/* The step's epilogue as a readout (csrc/rex_outcome.h): what env.step() would SAY of row (k, c) = (env d_env_ids[k] or env k, candidate
 * c) whose control step ended in the given state -- reward, done and observation, the rest of the Gym tuple beside rex_command's targets.
 * One small read-only launch (a lane per row and leg) that calls the step kernels' own quat_to_euler, euler_to_row2, env_observation and
 * normalize_obs1 and restates the scalar arithmetic between them; no host sync; the sim's state is never written.
 *   d_state        [n][K][37] words 0..36 of the row AFTER the control step, or NULL: the env's
 *   d_ctrl         [n][K][8] the controller words REX_S_PHI .. REX_S_STEPS (37..44) after that step, as rex_command's d_ctrl_next and the
 *                  state block hold them -- REX_S_TARGET already |target|, REX_S_STEPS already + 1, REX_F_ENV_GOAL as the command set it;
 *                  REX_F_DONE in the input is ignored --, raw 32-bit words, or NULL: the env's
 *   d_motor_torque [n][K][12] the OBSERVED motor torques of the control step's last substep (motor.py:116-119: the clipped PD torque, not
 *                  the applied one and not masked by the motor enable bits), as rex_rollout_actions_outcome emits them, or NULL: zeros,
 *                  which leaves the reward's energy term out
 *   out->reward    [n][K]: the forward reward's four branches under forward_reward_cap, drift, shake and energy = -|sum tau_obs x qd| x
 *                  cfg.sim_time_step with the task's weights (rex_gym_env.py:501-542); the turn, standup and poses rewards
 *   out->done      [n][K] 0 / 1: r22 < 0.85, or the true roll / pitch / y test of gallop and standup; REX_F_ENV_GOAL except for standup;
 *                  poses never; REX_S_STEPS >= cfg.max_episode_steps when that is set
 *   out->obs       [n][K][rex_obs_dim(cfg)]: roll, pitch, roll rate, pitch rate, then the gallop env's MapToMinusPiToPi motor angles where
 *                  the row carries them; RangeNormalize applied when cfg.range_normalize is set
 * Conventions of every readout: sensor noise is not drawn; there is NO reset -- on an auto_reset env the observation is the terminal one,
 * which rex_step never returns (it returns the next episode's first) --; nothing is written to the sim.  Read from the env besides: the
 * config.  The inputs are the caller's, so the kernel was read for arbitrary float input: no address is formed from a state or controller
 * word or a torque -- rows are addressed by the row index and the env id, flag bits and the step counter only enter compares.  A bad row
 * yields garbage in that row only.
 * REX_EINVAL (message in rex_last_error) without a launch for: NULL out or an `out` whose members are all NULL; candidates < 1; a null sim;
 * n < 1; n > num_envs without ids; n * candidates * 37 >= 2^31; a sim of mark arm, of REX_TASK_MIXED or with the latency model on (the
 * reward would read the delayed observation). */
typedef struct RexOutcomeOut {   /* any member may be NULL, not all */
  float* reward;               /* [n][K] */
  uint8_t* done;               /* [n][K] 0 / 1 */
  float* obs;                  /* [n][K][obs_dim] */
} RexOutcomeOut;
REX_API int rex_outcome(RexSim* sim, const int32_t* d_env_ids, int n, int candidates, const float* d_state, const float* d_ctrl,
                        const float* d_motor_torque, const RexOutcomeOut* out, void* stream);

/* rex_rollout_actions as a forked env: the same call, the same 2 T launches, with the full Gym tuple per control step.  Per step
 * rex_command, then the rollout kernel's third instantiation, which keeps the observed torques of the step's last substep in registers,
 * stores them and calls the device function of rex_outcome on the row's new state, the command's controller words and those torques --
 * the energy term cannot be recovered from the emitted states (the pre-substep joint rates are gone).  in, from, out, the workspace and its
 * size are rex_rollout_actions'; `out` may have every member NULL here.  outcome (time-major; any member may be NULL, not all):
 *   reward [T][n][K], done [T][n][K], obs [T][n][K][obs_dim]: bit for bit rex_outcome on trajectory[t], ctrl_trajectory[t],
 *   motor_torque[t];  motor_torque [T][n][K][12]: the observed torques, not masked by the motor enable bits.
 * Rows RUN ON after done (no reset inside a rollout): the caller masks with the running OR of done.  A discounted return in torch:
 *   alive = 1 - (done.cumsum(0) - done).clamp(max=1)                 # [T, k, K]: 1 up to and including the step that ended the episode
 *   disc = gamma ** torch.arange(T, device=reward.device)[:, None, None]
 *   ret = (reward * alive * disc).sum(0)                             # [k, K]
 * REX_EINVAL before any launch for everything rex_rollout_actions refuses, a NULL outcome and an outcome whose members are all NULL. */
typedef struct RexRolloutActionsOutcome {   /* any member may be NULL, not all */
  float* reward;               /* [T][n][K] */
  uint8_t* done;               /* [T][n][K] 0 / 1 */
  float* obs;                  /* [T][n][K][obs_dim] */
  float* motor_torque;         /* [T][n][K][12] observed torques of each control step's last substep */
} RexRolloutActionsOutcome;
REX_API int rex_rollout_actions_outcome(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from,
                                        const RexRolloutActionsOut* out, const RexRolloutActionsOutcome* outcome, void* d_workspace,
                                        long long workspace_bytes, void* stream);

/* The acceleration level (csrc/rex_contact_space.h): what a whole-body controller, a force-distribution QP or an analytic contact model
 * needs beside M, h and J_p -- each in one read-only launch, M(q) never written out, the state never written.  Mark base only.  Rows, ids
 * and launch as rex_dynamics: no host sync; v, the order of its 18 components, M, h, J_p, the masses (with the env's scales) and the toe
 * points p = 2 leg + e are rex_dynamics'.  Like `bias`, both calls leave out what the step adds to the rigid-body equation: the
 * Bullet-style damping, joint-limit rows, contact rows and the on_rack anchor.
 *
 *   rex_inverse_dynamics  force [n][18] = M(q) vdot + h(q, v) - S^T tau - sum_p J_p^T f_p - w:  the equation of rex_forward_dynamics solved
 *                         for the force.  vdot [n][18] is the wanted generalized acceleration (NULL: zero); the load is what is applied
 *                         already -- joint torques `joint`, world forces `toe` at the toe points, the base wrench `base` -- and may be NULL,
 *                         as may any member (zero).  force[6:18] is the joint torque still needed; force[0:6] is the force at the base
 *                         origin and the moment that nothing supplies: zero for a motion the given ground forces can produce.  The ground
 *                         is queried only when toe forces are given.  With everything NULL, force = h.
 *   rex_contact_space     for joint torques d_tau [n][12] and a base wrench d_base_wrench [n][6] (either may be NULL: zero), any of
 *     delassus     [n][24][24]  J M^-1 J^T of the eight toe points: row and column 3 p + c, world axis c, for all eight points whether in
 *                               reach or not (as toe_jacobian).  Symmetric positive semidefinite; both triangles are written from one
 *                               value per pair (they carry the same bits)
 *     toe_drift    [n][8][3]    Jdot v: the acceleration of the foot link's material point at toe_pos[p] when vdot = 0.  With w_0 the
 *                               base's angular velocity, w_i = w_i-1 + qd_i a_i and joint points o_i carried by their parents:
 *                               alpha_0 = 0, acc(o_0) = 0;  alpha_i = alpha_i-1 + w_i-1 x (qd_i a_i);
 *                               acc(o_i) = acc(o_i-1) + alpha_i-1 x (o_i - o_i-1) + w_i-1 x (w_i-1 x (o_i - o_i-1));
 *                               drift_p = acc(o_3) + alpha_3 x (P - o_3) + w_3 x (w_3 x (P - o_3))
 *     toe_acc_free [n][8][3]    J_p M^-1 (S^T tau + w - h) + drift_p: the toe acceleration with no ground force.  With forces f [24] at
 *                               the toe points the acceleration is toe_acc_free + delassus f
 *   A NULL member of RexContactSpaceOut is not computed.  delassus is written in 16-byte chunks and must be 16-byte aligned (a row is
 *   2 304 bytes); the other arrays need the alignment of a float.
 * REX_EINVAL (message in rex_last_error) without a launch for: a null sim, force or out; n < 1; n > num_envs without ids; n * 18 >= 2^31;
 * a sim of mark arm; and for rex_contact_space an `out` whose members are all NULL, n * 24 * 24 >= 2^31, a delassus that is not 16-byte
 * aligned. */
typedef struct RexContactSpaceOut {     /* any member may be NULL */
  float* delassus;             /* [n][24][24] */
  float* toe_drift;            /* [n][4][2][3] */
  float* toe_acc_free;         /* [n][4][2][3] */
} RexContactSpaceOut;
REX_API int rex_inverse_dynamics(RexSim* sim, const int32_t* d_env_ids, int n, const float* d_vdot /* nullable */,
                                 const RexDynamicsLoad* load /* nullable */, float* d_force, void* stream);
REX_API int rex_contact_space(RexSim* sim, const int32_t* d_env_ids, int n, const float* d_tau /* nullable */,
                              const float* d_base_wrench /* nullable */, const RexContactSpaceOut* out, void* stream);

/* Force distribution (csrc/rex_force_distribution.h): which ground forces inside the friction cones produce a wanted acceleration, and
 * which joint torques go with them -- a regularised cone-constrained least-squares problem per row, solved by a fixed number of
 * accelerated projected-gradient steps in ONE read-only launch.  Mark base only.  Rows, ids and launch as rex_dynamics: no host sync; v,
 * the order of its 18 components, M, h, J_p, the masses (with the env's scales) and the toe points p = 2 leg + e are rex_dynamics'.
 * For one row, P_p are the eight toe points (rex_kinematics' toe_pos), n_p the ground normal there, o_0 the base origin, d_p = P_p - o_0.
 *   Wanted base wrench   r = (M vdot + h - w)[0:6]: the six base rows of the equation of motion, the rows no motor supplies
 *                        (rex_inverse_dynamics(vdot, base = w)[0:6]).  d_vdot NULL: zero ("hold still"); d_base_wrench NULL: zero.
 *   The ground supplies  A f = (sum_p f_p, sum_p d_p x f_p): the base rows of sum_p J_p^T f_p.
 *   Stance set S         d_stance [n][4], uint8, per LEG (both ends of its toe), nonzero = the leg may push.  NULL: every POINT in reach,
 *                        dist < 0.02 m, rex_kinematics' toe_in_reach.
 *   Cones                K_p = { f : |f - (n_p . f) n_p| <= mu_p (n_p . f) }, the circular Coulomb cone about the local normal, mu_p =
 *                        friction_scale x the env's foot friction (the value rex_contact_solve uses).  It lies inside the step's friction
 *                        pyramid: a force from here is one the simulated contact can hold.  f_p = 0 for p outside S.
 *   Problem              minimise  1/2 (A f - r)^T W (A f - r) + 1/2 eps sum_p |f_p|^2   over f_p in K_p (p in S), f_p = 0 otherwise,
 *                        W = diag(weights), weights > 0, eps > 0: strictly convex, one solution.  A has rank at most 6 against 24
 *                        unknowns, so the regulariser is mandatory.  It biases the solution: even where r is reachable, A f falls short
 *                        of it by a ridge shrinkage of the order eps / sigma_min(A)^2 (base_residual reports it).
 *   Solver               accelerated projected gradient, constant scheme, exactly `iterations` steps from f = y = 0, no early exit:
 *                          L = eps + sum_{p in S} [w_0 + w_1 + w_2 + w_3 (d_y^2 + d_z^2) + w_4 (d_x^2 + d_z^2) + w_5 (d_x^2 + d_y^2)]
 *                          kappa = L / eps,  beta = (sqrt(kappa) - 1) / (sqrt(kappa) + 1);  each step
 *                          u = W (A y - r);  g_p = u_lin + u_ang x d_p + eps y_p;  f+_p = Proj_Kp(y_p - g_p / L);
 *                          y = f+ + beta (f+ - f);  f = f+
 *                        Proj_K, with s = n . x and t = x - s n:  x if |t| <= mu s;  0 if mu |t| <= -s;  else s' n + mu s' t / |t| with
 *                        s' = (s + mu |t|) / (1 + mu^2) (the tangential term is 0 when |t| = 0).  An empty S gives L = eps, f = 0.
 *                        The caller judges convergence from `residual`.
 * Outputs (any member may be NULL: not computed; each needs the alignment of a float):
 *   toe_force     [n][4][2][3]  world N at toe_pos: f after the last step
 *   tau           [n][12]       (M vdot + h)[6:18] - (sum_p J_p^T f_p)[6:18]: the joint torques that realise vdot under those forces.  Like
 *                               `bias`, it holds no damping, joint-limit or motor terms
 *   base_residual [n][6]        r - A f: the wrench the ground does not supply
 *   residual      [n]           L max_p |Proj(f - g(f) / L) - f|_inf, N: the fixed-point residual at the returned f, the optimality measure
 *                               (one more gradient evaluation)
 * Not here: normal-force ceilings or floors, per-point weights, force tracking terms, a warm start.
 * REX_EINVAL (message in rex_last_error) without a launch for: a null sim, params or out; n < 1; n > num_envs without ids; n * 24 >= 2^31;
 * an `out` whose members are all NULL; a weight or eps that is not finite and positive; a friction_scale that is not finite or is
 * negative; iterations outside 1 .. 10000; a sim of mark arm, on_rack or with body_contacts. */
typedef struct RexForceDistributionParams {
  float weights[6];            /* W: base force x, y, z, base moment x, y, z; each > 0 */
  float eps;                   /* > 0 */
  float friction_scale;        /* >= 0: mu_p = friction_scale x the env's foot friction */
  int32_t iterations;          /* 1 .. 10000 */
} RexForceDistributionParams;
typedef struct RexForceDistributionOut {     /* any member may be NULL */
  float* toe_force;            /* [n][4][2][3] */
  float* tau;                  /* [n][12] */
  float* base_residual;        /* [n][6] */
  float* residual;             /* [n] */
} RexForceDistributionOut;
REX_API int rex_force_distribution(RexSim* sim, const int32_t* d_env_ids, int n, const float* d_vdot /* nullable */,
                                   const float* d_base_wrench /* nullable */, const uint8_t* d_stance /* nullable */,
                                   const RexForceDistributionParams* params, RexForceDistributionOut* out, void* stream);

/* ---- the fused PPO learner (csrc/rex_learner.h): the losses of the reference's KL-penalty PPO (agents/ppo/algorithm.py:289-301,
 * 376-434) and their parameter gradients for a ForwardGaussianPolicy network (networks.py:69-112: obs_dim -> hidden1 -> hidden2 ->
 * out_dim, two ReLU layers), one pass over the episode memory per call.  Stateless: no RexSim, the library allocates nothing -- the
 * caller owns every buffer, the workspace included.  All device arrays float32, row-major; the episode memory is R rows (episodes) of T
 * padded steps with a length per row (int32, clamped to 0..T): a step t >= length[r] contributes exactly nothing and is never read.
 * Supported: obs_dim 4, 16 or 22; out_dim (the action dimension) 1, 2, 4 or 8 for the policy net and 1 for the value net; hidden1 <= 256,
 * hidden2 <= 128; R * T * 24 < 2^31 (24 = the widest observation row, padded).  Anything else: REX_EINVAL, message in rex_last_error.
 * Every sum runs in a fixed order: two calls on the same inputs return the same bits. */
typedef struct RexPpoNet {                /* the network, in TORCH layout: a Linear's weight is [out][in], no transposes */
  int32_t obs_dim, out_dim, hidden1, hidden2;
  const float *d_w1, *d_b1;               /* [hidden1][obs_dim], [hidden1] */
  const float *d_w2, *d_b2;               /* [hidden2][hidden1], [hidden2] */
  const float *d_w3, *d_b3;               /* [out_dim][hidden2], [out_dim]: policy: mean = tanh(W3 h2 + b3); value = W3 h2 + b3 */
  const float *d_logstd;                  /* [out_dim] (policy; NULL for the value net) */
} RexPpoNet;
typedef struct RexPpoBatch {
  int32_t rows, steps;                    /* R, T */
  const float *d_observ;                  /* [R][T][obs_dim], already through the observ filter */
  const float *d_action, *d_old_mean, *d_old_logstd;   /* [R][T][out_dim] (policy) */
  const float *d_advantage;               /* [R][T], already normalised (policy) */
  const float *d_return;                  /* [R][T] (value) */
  const int32_t *d_length;                /* [R] */
  float penalty, kl_cutoff, kl_cutoff_coef;   /* the current KL penalty, kl_target * kl_cutoff_factor, kl_cutoff_coef (policy) */
} RexPpoBatch;
typedef struct RexPpoGrad {               /* the gradients, shaped like RexPpoNet's tensors: they can BE the parameters' .grad */
  float *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3, *d_logstd;
} RexPpoGrad;
/* Bytes of workspace the two loss calls below need for a memory of `rows` x `steps` (< 0: unsupported shape).  16-byte aligned. */
REX_API long long rex_ppo_workspace_bytes(int rows, int steps, int obs_dim, int out_dim, int hidden1, int hidden2);
/* utility.py:71-81 and 97-110, one launch, one lane per row, a reverse scan.  With m_t = [t < length]:
 *   return_t = m_t reward_t + discount return_{t+1}                                                       -> d_return (nullable)
 *   lambda_t = m_t reward_t + discount (1 - lambda) value_t + m_t discount lambda lambda_{t+1}            -> d_lambda_return (with d_value) */
REX_API int rex_ppo_returns(int rows, int steps, const float* d_reward, const int32_t* d_length, float discount, float* d_return,
                            const float* d_value, float lambda, float* d_lambda_return, void* stream);
/* The policy loss of algorithm.py:376-434.  With KL_t = diag_normal_kl(old || new) (utility.py:127-132), logp = diag_normal_logpdf AS
 * WRITTEN in utility.py:135-139 (-0.5 (log 2 pi + logstd) - 0.5 ((x - mean) / e^logstd)^2 summed: its -0.5 logstd term kept),
 * ratio_t = exp(logp_new - logp_old), kl_r = (1/T) sum_t m_t KL_t and c = kl_cutoff:
 *   loss = (1/R) sum_r [ -(1/T) sum_t m_t ratio_t adv_t + penalty kl_r + coef [kl_r > c] (kl_r - c)^2 ]
 * (T is the padded step count: the reference's reduce_mean runs over the padded axis.)  Backward seeds of a valid step, l = logstd:
 *   w_r = penalty + 2 coef [kl_r > c] (kl_r - c)
 *   dKL/dm = (m - m0) / e^2l          dKL/dl   = 1 - e^(2 l0 - 2 l) - (m - m0)^2 / e^2l
 *   dlogp/dm = (x - m) / e^2l         dlogp/dl = -0.5 + ((x - m) / e^l)^2
 *   g_m = (-ratio adv dlogp/dm + w_r dKL/dm) / (R T), g_l likewise, g_z = g_m (1 - m^2)
 * d_loss [1] and d_kl_row [R] are always written; grad == NULL makes the call forward-only (the same loss and kl_row, bit for bit).
 * Launches on `stream`, no host synchronisation. */
REX_API int rex_ppo_policy_loss(const RexPpoNet* net, const RexPpoBatch* batch, const RexPpoGrad* grad, float* d_loss, float* d_kl_row,
                                void* d_workspace, void* stream);
/* The value loss of algorithm.py:289-301: loss = (1 / (R T)) sum 0.5 m_t (return_t - value_t)^2 and the gradients of the value net's six
 * tensors (grad->d_logstd is ignored; grad == NULL: forward-only).  d_value_out (nullable): [R][T], the masked values, zero beyond the length. */
REX_API int rex_ppo_value_loss(const RexPpoNet* net, const RexPpoBatch* batch, const RexPpoGrad* grad, float* d_loss, float* d_value_out,
                               void* d_workspace, void* stream);

/* ---- the fused RECURRENT PPO learner (csrc/rex_learner_rnn.h): the policy loss above for the RecurrentGaussianPolicy (networks.py:113-159)
 * and its nine parameter gradients by backpropagation through time.  The value net of a recurrent agent is the plain two-layer network:
 * rex_ppo_value_loss and rex_ppo_returns serve it unchanged.  For one episode row, h_0 = 0, o_t the filtered observation, F = hidden1, H = state:
 *   x_t = relu(W1 o_t + b1)                                    W1 [F][O]
 *   [r_t ; u_t] = sigmoid(Wg [x_t ; h_{t-1}] + bg)             Wg [2H][F+H], rows 0..H-1 = r, H..2H-1 = u
 *   c_t = tanh(Wc [x_t ; r_t * h_{t-1}] + bc)                  Wc [H][F+H]
 *   h_t = u_t h_{t-1} + (1 - u_t) c_t
 *   m_t = tanh(Wm h_t + bm)                                    Wm [A][H];  logstd [A]
 * Loss, kl_row and the seeds g_m, g_l, g_z = g_m (1 - m^2) of a valid step are rex_ppo_policy_loss's.  The backward recurrence, in reverse t
 * with carry_T = 0:
 *   dh   = Wm^T g_z,t + carry
 *   du   = dh (h_{t-1} - c)      dc = dh (1 - u)       carry = dh u
 *   da_c = dc (1 - c^2)          [dx_c ; drh] = Wc^T da_c
 *   dr   = drh h_{t-1}           carry += drh r
 *   da_g = [dr r (1 - r) ; du u (1 - u)]               [dx_g ; dhg] = Wg^T da_g     carry += dhg
 *   dx_t = dx_c + dx_g           da1 = dx_t [W1 o_t + b1 > 0]
 *   dWg += da_g [x_t ; h_{t-1}]^T   dbg += da_g     dWc += da_c [x_t ; r h_{t-1}]^T   dbc += da_c
 *   dWm += g_z h_t^T   dbm += g_z   dlogstd += g_l   dW1 += da1 o_t^T   db1 += da1
 * Supported: state 100; obs_dim 4, 16 or 22; out_dim 1, 2, 4 or 8; hidden1 <= 256; R * T * 24 < 2^31.  Anything else: REX_EINVAL, the
 * offending field named in rex_last_error.  A step t >= length[r] contributes nothing and is never read.  fp32; every sum in a fixed order:
 * two calls on the same inputs return the same bits.  The workspace holds the stored activations of every memory slot -- hidden1 rounded up
 * to 32, + 658 floats per slot: 3 528 bytes at hidden1 = 200 -- the packed weights and the partial gradients. */
typedef struct RexPpoRnnNet {             /* TORCH layout, as RecurrentGaussianPolicy holds them */
  int32_t obs_dim, out_dim, hidden1, state;
  const float *d_w1, *d_b1;               /* [hidden1][obs_dim], [hidden1] */
  const float *d_wg, *d_bg;               /* [2 state][hidden1 + state], [2 state] */
  const float *d_wc, *d_bc;               /* [state][hidden1 + state], [state] */
  const float *d_wm, *d_bm;               /* [out_dim][state], [out_dim] */
  const float *d_logstd;                  /* [out_dim] */
} RexPpoRnnNet;
typedef struct RexPpoRnnGrad {            /* the gradients, shaped like RexPpoRnnNet's tensors */
  float *d_w1, *d_b1, *d_wg, *d_bg, *d_wc, *d_bc, *d_wm, *d_bm, *d_logstd;
} RexPpoRnnGrad;
/* Bytes of workspace rex_ppo_recurrent_policy_loss needs (< 0: unsupported shape, the field named in rex_last_error).  16-byte aligned. */
REX_API long long rex_ppo_recurrent_workspace_bytes(int rows, int steps, int obs_dim, int out_dim, int hidden1, int state);
/* d_loss [1] and d_kl_row [R] are always written; grad == NULL makes the call forward-only (the same loss and kl_row, bit for bit).  The
 * batch is rex_ppo_policy_loss's (d_return unused).  Stateless; launches on `stream`, no host synchronisation. */
REX_API int rex_ppo_recurrent_policy_loss(const RexPpoRnnNet* net, const RexPpoBatch* batch, const RexPpoRnnGrad* grad, float* d_loss,
                                          float* d_kl_row, void* d_workspace, void* stream);

REX_API const char* rex_last_error(void);
REX_API int rex_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REXSIM_H */
