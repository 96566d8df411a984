// rexsim.hip -- kernels + C ABI (include/rexsim.h) of the MI355X-native batched Rex simulator.
// gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC rexsim.hip -o librexsim_hip.so
//
// The step and settle kernels are instantiated in rex_step_*.hip / rex_settle.hip (rex_kernels.h); this file holds the
// simulator's C ABI, the reset kernel and the small kernels (the regrouping sort rex_regroup_count_kernel / rex_regroup_scatter_kernel,
// controller-only entry points).  Which envs of a mixed batch share a wave is host code of its own (rex_placement.h).  The fused PPO
// learners' entry points are rex_learner.hip's; rex_last_error and the message both units set (rex_error.h) live here.
#include "rex_kernels.h"
#include "rex_placement.h"
#include "rex_render.h"
#include "rex_sense.h"
#include "rex_kinematics.h"
#include "rex_dynamics.h"
#include "rex_dynamics_solve.h"
#include "rex_contact_solve.h"
#include "rex_rollout.h"
#include "rex_command.h"
#include "rex_contact_space.h"
#include "rex_force_distribution.h"
#include "rex_visual_gen.h"
#include "rex_error.h"
#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <vector>

namespace rex {

// rex_set_policy: the caller's plain arrays (input-major weight matrices) -> the packed actor.  One thread per destination float.
struct PolSrc { const float *w1, *b1, *w2, *b2, *w3, *b3, *logstd, *mean, *scale; };
// the tail both packed actors end in, destination float t >= o_w3: the output layer [IN][A], its bias, logstd, the observ filter's mean
// and scale [O] (0 / 1 without a filter); zero padding in between
__device__ __forceinline__ float pack_tail(int t, int o_w3, int o_b3, int o_logstd, int o_mean, int o_scale, int IN, int O, int A, const float* w3, const float* b3,
                                           const float* logstd, const float* mean, const float* scale) {
  float v = 0.0f;
  if (t < o_b3) { if (t - o_w3 < IN * A) v = w3[t - o_w3]; }
  else if (t < o_logstd) { if (t - o_b3 < A) v = b3[t - o_b3]; }
  else if (t < o_mean) { if (t - o_logstd < A) v = logstd[t - o_logstd]; }
  else if (t < o_scale) { if (t - o_mean < O && mean) v = mean[t - o_mean]; }
  else if (t < o_scale + O) { v = scale ? scale[t - o_scale] : 1.0f; }
  return v;
}
__global__ void rex_pack_policy_kernel(PolSrc s, int O, int A, int H1, int H2, float* __restrict__ dst) {
  const PolOff o = policy_offsets(O, A, H1, H2);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < o.total; t += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (t < o.b1) { const int r = t & 3, j = (t >> 2) % H1, k = 4 * ((t >> 2) / H1) + r; if (k < O) v = s.w1[k * H1 + j]; }
    else if (t < o.w2) { if (t - o.b1 < H1) v = s.b1[t - o.b1]; }
    else if (t < o.b2) { const int u = t - o.w2, r = u & 3, j = (u >> 2) % H2, k = 4 * ((u >> 2) / H2) + r; if (k < H1) v = s.w2[k * H2 + j]; }
    else if (t < o.w3) { if (t - o.b2 < H2) v = s.b2[t - o.b2]; }
    else v = pack_tail(t, o.w3, o.b3, o.logstd, o.mean, o.scale, H2, O, A, s.w3, s.b3, s.logstd, s.mean, s.scale);
    dst[t] = v;
  }
}

// rex_set_policy_recurrent: the same for the recurrent actor (rnn_offsets).  A gate matrix [ceil(H1 / 4) + ceil(S / 4)][S][4] takes
// its rows from the caller's [H1 + S][ld] matrix: the x rows, zero rows up to a whole quad, the h rows, zero rows; columns col0 + j.
struct RnnSrc { const float *w1, *b1, *wg, *bg, *wc, *bc, *w3, *b3, *logstd, *mean, *scale; };
__device__ __forceinline__ float rnn_gate_weight(int u, int H1, int S, const float* src, int ld, int col0) {
  const int r = u & 3, j = (u >> 2) % S, q = (u >> 2) / S;
  int row;
  if (q < pol_q4(H1)) { row = 4 * q + r; if (row >= H1) return 0.0f; }
  else { row = 4 * (q - pol_q4(H1)) + r; if (row >= S) return 0.0f; row += H1; }
  return src[row * ld + col0 + j];
}
__global__ void rex_pack_rnn_kernel(RnnSrc s, int O, int A, int H1, int S, float* __restrict__ dst) {
  const RnnOff o = rnn_offsets(O, A, H1, S);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < o.total; t += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (t < o.b1) { const int r = t & 3, j = (t >> 2) % H1, k = 4 * ((t >> 2) / H1) + r; if (k < O) v = s.w1[k * H1 + j]; }
    else if (t < o.wr) { if (t - o.b1 < H1) v = s.b1[t - o.b1]; }
    else if (t < o.br) v = rnn_gate_weight(t - o.wr, H1, S, s.wg, 2 * S, 0);
    else if (t < o.wu) { if (t - o.br < S) v = s.bg[t - o.br]; }
    else if (t < o.bu) v = rnn_gate_weight(t - o.wu, H1, S, s.wg, 2 * S, S);
    else if (t < o.wc) { if (t - o.bu < S) v = s.bg[S + t - o.bu]; }
    else if (t < o.bc) v = rnn_gate_weight(t - o.wc, H1, S, s.wc, S, 0);
    else if (t < o.w3) { if (t - o.bc < S) v = s.bc[t - o.bc]; }
    else v = pack_tail(t, o.w3, o.b3, o.logstd, o.mean, o.scale, S, O, A, s.w3, s.b3, s.logstd, s.mean, s.scale);
    dst[t] = v;
  }
}
// rex_reset while a recurrent policy is installed: the GRU state rows [S][n] of the reset envs start from zero
__global__ void rex_zero_rnn_state_kernel(float* __restrict__ state, int n, int S, const int32_t* __restrict__ indices, int count) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= count) return;
  const int i = indices ? indices[r] : r;
  if (i < 0 || i >= n) return;
  for (int k = 0; k < S; ++k) state[(size_t)k * n + i] = 0.0f;
}


// Regrouping: a counting sort of the env indices by the solver sweeps of the last step, most sweeps first (the long waves start
// first), 64 bins, over many workgroups (one workgroup takes 0.3 ms for 262 144 envs: a tenth of their step).  The order inside
// a bin does not matter: an env's result does not depend on its wave-mates.
//   a single-task batch: one class of 64 bins from slot 0; out = DevCfg::perm, perm[k] = env of wave slot k.
//   a REX_TASK_MIXED batch: every task of the mix is a class and owns a STATIC region of the slot map (whole waves; the envs keep
//   their task for life, so the region sizes and its padding slots never change); inside its region a task's envs are sorted --
//   the waves of a large mixed batch then hold envs that need about the same number of sweeps, and the waves that exceed one
//   round of the machine are the short ones.  64 / n_mix sweep bins per task; out = DevCfg::slot_env.
// Workgroup b counts its REX_REGROUP_CHUNK envs per bin; the last workgroup to finish turns the counts into start offsets (a
// class's bins fill its region from its first slot, bins in order, workgroups in order inside a bin); a second launch scatters.
#define REX_REGROUP_CHUNK 1024
__device__ __forceinline__ int regroup_bin(const RegroupKey& key, int sweeps, int i) {
  const int w = key.bins_per_class;
  return (key.cls ? key.cls[i] : 0) * w + (w - 1 - min(sweeps / key.bin_width, w - 1));
}
__global__ __launch_bounds__(256) void rex_regroup_count_kernel(int n, RegroupKey key, const int32_t* __restrict__ sweeps, int32_t* __restrict__ counts,
                                                                unsigned* __restrict__ done) {
  __shared__ int hist[64];
  __shared__ bool last;
  const int t = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
  if (t < 64) hist[t] = 0;
  __syncthreads();
  for (int k = t; k < REX_REGROUP_CHUNK; k += 256) {
    const int i = b * REX_REGROUP_CHUNK + k;
    if (i < n) atomicAdd(&hist[regroup_bin(key, sweeps[i], i)], 1);
  }
  __syncthreads();
  if (t < 64) counts[b * 64 + t] = hist[t];
  __threadfence();
  __syncthreads();
  if (t == 0) last = atomicAdd(done, 1u) == (unsigned)nb - 1u;
  __syncthreads();
  if (!last) return;
  __threadfence();
  // counts[b][bin] -> first slot of workgroup b's envs of that bin
  __shared__ int total[64], first[64];
  if (t < 64) { int acc = 0; for (int k = 0; k < nb; ++k) acc += counts[k * 64 + t]; total[t] = acc; }
  __syncthreads();
  if (t == 0) {
    for (int c = 0; c < key.n_classes; ++c) {
      int acc = key.base[c];
      for (int k = 0; k < key.bins_per_class; ++k) { first[c * key.bins_per_class + k] = acc; acc += total[c * key.bins_per_class + k]; }
    }
    *done = 0u;
  }
  __syncthreads();
  if (t < key.n_classes * key.bins_per_class) { int acc = first[t]; for (int k = 0; k < nb; ++k) { const int c = counts[k * 64 + t]; counts[k * 64 + t] = acc; acc += c; } }
}
__global__ __launch_bounds__(256) void rex_regroup_scatter_kernel(int n, RegroupKey key, const int32_t* __restrict__ sweeps, const int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ out) {
  __shared__ int cursor[64];
  const int t = threadIdx.x, b = blockIdx.x;
  if (t < 64) cursor[t] = counts[b * 64 + t];
  __syncthreads();
  for (int k = t; k < REX_REGROUP_CHUNK; k += 256) {
    const int i = b * REX_REGROUP_CHUNK + k;
    if (i < n) out[atomicAdd(&cursor[regroup_bin(key, sweeps[i], i)], 1)] = i;
  }
}
__global__ void rex_iota_kernel(int n, int32_t* __restrict__ perm) {   // a regrouped single-task batch starts in index order
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = i;
}

// ---- controller-only kernels ----
__global__ void rex_ik_kernel(int n, const float* __restrict__ orn, const float* __restrict__ pos,
                              const float* __restrict__ frames, float* __restrict__ angles) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float o[3], p[3], f[12], a[12];
  for (int k = 0; k < 3; ++k) { o[k] = orn[3 * i + k]; p[k] = pos[3 * i + k]; }
  for (int k = 0; k < 12; ++k) f[k] = frames[12 * i + k];
  ik_solve(o, p, f, a);
  for (int k = 0; k < 12; ++k) angles[12 * i + k] = a[k];
}

__global__ void rex_motor_kernel(int n, const float* __restrict__ cmd, const float* __restrict__ q, const float* __restrict__ qd,
                                 const float* __restrict__ qdt, float kp, float kd, float* __restrict__ actual,
                                 float* __restrict__ observed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a, o;
  motor_torque(cmd[i], q[i], qd[i], qdt[i], kp, kd, a, o);
  actual[i] = a; observed[i] = o;
}

__global__ void rex_motor_params_kernel(int n, const float* __restrict__ cmd, const float* __restrict__ q, const float* __restrict__ qd,
                                        const float* __restrict__ qdt, const float* __restrict__ par, float* __restrict__ actual,
                                        float* __restrict__ observed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a, o;
  motor_torque(cmd[i], q[i], qd[i], qdt[i], par[5 * (size_t)i], par[5 * (size_t)i + 1], par[5 * (size_t)i + 2], par[5 * (size_t)i + 3],
               par[5 * (size_t)i + 4], a, o);
  actual[i] = a; observed[i] = o;
}

// rex_get_motor_params: what rex_substep forms for env i in its current episode, all rows
template <int NM>
__global__ void rex_get_motor_params_kernel(DevCfg c, MotDev mot, const float* __restrict__ state, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.n) return;
  const int gidx = c.env_index_base + i, episode = (int)ldi(state, c.n, Lay<NM>::EPISODE, i);
  const MotorScalars m = motor_scalars(c, mot, i, gidx, episode);
  float st[NM];
  motor_strengths<NM>(c, mot, i, gidx, episode, 0, st);
  out[i] = m.voltage; out[(size_t)c.n + i] = m.damping; out[2 * (size_t)c.n + i] = m.kp; out[3 * (size_t)c.n + i] = m.kd;
#pragma unroll
  for (int j = 0; j < NM; ++j) out[(size_t)(4 + j) * c.n + i] = st[j];
}

__global__ void rex_gait_kernel(int n, int mode, double* __restrict__ planner, const double* __restrict__ params,
                                float* __restrict__ frames) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  GaitState g{planner[3 * i], planner[3 * i + 1], (float)planner[3 * i + 2]};
  const double* p = params + 6 * i;
  float f[12];
  gait_loop(g, mode, (float)p[0], (float)p[1], (float)p[2], p[3], (float)p[4], p[5], f);
  planner[3 * i] = g.phi; planner[3 * i + 1] = g.last_time; planner[3 * i + 2] = g.alpha;
  for (int k = 0; k < 12; ++k) frames[12 * i + k] = f[k];
}

}  // namespace rex

// =================================================================================================
//                                          host side: C ABI
// =================================================================================================

// (rex_error.h declares fail, failf and HIPCHK for every host unit; the message lives here, next to rex_last_error)
static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, const char* detail) {
  snprintf(g_err, sizeof(g_err), fmt, detail ? detail : "");
  return code;
}
int failf(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" {

const char* rex_last_error(void) { return g_err; }
int rex_abi_version(void) { return REX_ABI_VERSION; }

int rex_default_config(int task, int signal, int num_envs, RexConfig* cfg) {
  if (!cfg || num_envs <= 0) return fail(REX_EINVAL, "rex_default_config: bad arguments%s", "");
  if (task != REX_TASK_WALK && task != REX_TASK_GALLOP && task != REX_TASK_TURN && task != REX_TASK_POSES && task != REX_TASK_STANDUP &&
      task != REX_TASK_MIXED) return fail(REX_EINVAL, "rex_default_config: unsupported task%s", "");
  if (signal != REX_SIGNAL_IK && signal != REX_SIGNAL_OL) return fail(REX_EINVAL, "rex_default_config: unsupported signal%s", "");
  memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = REX_ABI_VERSION;
  cfg->num_envs = num_envs;
  cfg->task = task;
  cfg->signal = signal;
  cfg->action_repeat = (task == REX_TASK_GALLOP || task == REX_TASK_POSES) ? 6 : 5;          /* gallop_env.py:47-48, walk_env.py:34-35 */
  cfg->solver_iterations = 300 / cfg->action_repeat;             /* rex_gym_env.py:25,184 */
  cfg->sim_time_step = 0.001f;
  cfg->motor_kp = 1.0f;
  cfg->motor_kd = 0.02f;
  cfg->backwards = -1;
  cfg->target_position = 0.0f;
  cfg->seed = 0;
  cfg->auto_reset = 0;
  cfg->max_episode_steps = 0;
  cfg->distance_weight = 1.0f;                                   /* rex_gym_env.py:56-59 */
  cfg->energy_weight = task == REX_TASK_GALLOP ? 0.005f : 0.0005f;   /* gallop_env.py:45 */
  cfg->drift_weight = 2.0f;
  cfg->shake_weight = 0.005f;
  cfg->pose_index = -1;
  /* RexPosesEnv never terminates (poses_env.py:265) and its roll poses press the rolled base's edge into the upper-leg
     boxes of the low side (profiles/r02_contact_census.md): the one env where the link boxes act */
  cfg->body_contacts = task == REX_TASK_POSES;
  cfg->solver_residual_threshold = 1e-7f;                        /* PyBullet default solverResidualThreshold */
  cfg->forward_reward_cap = INFINITY;                            /* rex_gym_env.py:81 */
  cfg->gallop_no_angles = 0;                                     /* gallop_env.py:56 use_angle_in_observation=True */
  if (task == REX_TASK_MIXED) {   /* BASELINE.json configs[4]: walk, gallop and turn; per-task repeat / sweeps / weights apply per env */
    cfg->task_mix = (1 << REX_TASK_WALK) | (1 << REX_TASK_GALLOP) | (1 << REX_TASK_TURN);
    cfg->action_repeat = 6; cfg->solver_iterations = 60;         /* the largest of the mix (loop bounds only) */
  }
  return REX_OK;
}

static int mix_tasks(const RexConfig* c, int* out) {   // tasks of a REX_TASK_MIXED config, ascending
  int n = 0;
  for (int t = 0; t < 5; ++t) if ((c->task_mix >> t) & 1) out[n++] = t;
  return n;
}

int rex_action_dim(const RexConfig* c) {
  if (!c) return REX_EINVAL;
  if (c->task == REX_TASK_MIXED) {          /* as wide as the widest task of the mix */
    int ts[5], best = REX_EINVAL;
    RexConfig one = *c;
    for (int k = 0, n = mix_tasks(c, ts); k < n; ++k) { one.task = ts[k]; int d = rex_action_dim(&one); if (d > best) best = d; }
    return best;
  }
  if (c->task == REX_TASK_WALK) return c->signal == REX_SIGNAL_IK ? 2 : 8;      /* walk_env.py:104-112 */
  if (c->task == REX_TASK_GALLOP) return c->signal == REX_SIGNAL_IK ? 2 : 4;    /* gallop_env.py:119-130 */
  if (c->task == REX_TASK_TURN) return 2;                                       /* turn_env.py:100-110 */
  if (c->task == REX_TASK_POSES || c->task == REX_TASK_STANDUP) return 1;       /* poses_env.py:115-117, standup_env.py:99-101 */
  return REX_EINVAL;
}
int rex_num_motors(const RexConfig* c) {
  if (!c) return REX_EINVAL;
  return c->mark == REX_MARK_ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;         /* mark_constants.py MARK_DETAILS['motors_num'] */
}
int rex_state_words(const RexConfig* c) {
  if (!c) return REX_EINVAL;
  return c->mark == REX_MARK_ARM ? rex::Lay<REX_NUM_MOTORS_ARM>::WORDS : REX_STATE_WORDS;
}
int rex_obs_dim(const RexConfig* c) {
  if (!c) return REX_EINVAL;
  if (c->gallop_no_angles) return 4;                                             /* use_angle_in_observation=False, gallop_env.py:344-356 */
  if (c->task == REX_TASK_MIXED) return ((c->task_mix >> REX_TASK_GALLOP) & 1) ? 4 + rex_num_motors(c) : 4;
  return c->task == REX_TASK_GALLOP ? 4 + rex_num_motors(c) : 4;                 /* gallop_env.py:349-356 */
}

// Envs per wave (measured on MI355X, walk-IK, steady state; REX_ENVS_PER_WAVE = 4, 8, 16 or 64 overrides).  A wave with
// EPW <= 16 envs spends its other lanes on the per-leg / per-row parallelism inside an env (rex_device.h: 8 lanes per
// env for EPW <= 8, 4 for EPW = 16), which cuts the instructions a lone wave has to issue per env.  Up to 4 096 envs the
// launch is one wave per SIMD and bound by its slowest wave: 4 envs per wave.  From 16 384 envs on, 16 envs per wave
// (4 workgroups per CU fit in LDS) also has the best throughput: 57 M env-steps/s at 131 072 envs against 33 M for the
// one-env-per-lane kernel (EPW = 64), whose 139 KB of LDS rows leave one wave per CU.
static int pick_envs_per_wave(int n) {
  const char* ov = getenv("REX_ENVS_PER_WAVE");
  if (ov) { int v = atoi(ov); if (v == 4 || v == 8 || v == 16 || v == 64) return v; }
  if (n <= 4096) return 4;
  if (n <= 8192) return 8;
  return 16;
}

// kernel instantiations by (envs per wave, mark); the arm rows fit 4 or 16 envs per workgroup in LDS
static int launch_step(RexSim* s, int blocks, hipStream_t st, const float* a, float* o, float* r, uint8_t* d, float* m);
static int launch_settle(RexSim* s, int nrec, hipStream_t st, float* snap);
static int step_group(const RexSim* s) {   // the variant group (rex_kernels.h RexStepGroup) whose kernels step this sim
  const bool arm = s->cfg.mark == REX_MARK_ARM;
  if (s->cfg.task == REX_TASK_MIXED) return arm ? REX_GROUP_MIXED_ARM : REX_GROUP_MIXED_BASE;   // lane groups only (rex_create caps the envs per wave at 16)
  if (s->cfg.body_contacts) return REX_GROUP_BODY;                                              // link-box contact rows: 4 or 8 envs per wave (rex_create caps it)
  return arm ? REX_GROUP_ARM : REX_GROUP_BASE;
}

// RexConfig carries its settings as float32; the reference computes its substep counts from the Python floats the
// caller wrote (int(0.5 / 0.001) = 500, int(0.02 / 0.001) = 20), whose float32 quotients fall just below the integer.
// The counts are therefore taken in double on the shortest decimal each float came from.
static double as_written(float x) {
  char buf[40];
  snprintf(buf, sizeof buf, "%.7g", (double)x);
  return strtod(buf, nullptr);
}
static size_t snapshot_floats(const RexSim* s, int nrec);

static int validate(const RexConfig* c) {
  if (!c) return fail(REX_EINVAL, "null config%s", "");
  if (c->abi_version != REX_ABI_VERSION) return fail(REX_EINVAL, "RexConfig.abi_version mismatch%s", "");
  if (c->num_envs <= 0) return fail(REX_EINVAL, "num_envs must be positive%s", "");
  if (rex_action_dim(c) < 0) return fail(REX_EINVAL, "unsupported task/signal%s", "");
  if (c->action_repeat <= 0 || c->solver_iterations <= 0 || !(c->sim_time_step > 0.0f))
    return fail(REX_EINVAL, "action_repeat, solver_iterations and sim_time_step must be positive%s", "");
  if (c->mark != REX_MARK_BASE && c->mark != REX_MARK_ARM) return fail(REX_EINVAL, "unknown mark%s", "");
  if ((long long)c->num_envs * 128 >= (1ll << 30)) return fail(REX_EINVAL, "num_envs too large for 32-bit state offsets%s", "");
  if (c->gait_clock_scale < 0.0f) return fail(REX_EINVAL, "gait_clock_scale must be >= 0%s", "");
  if (c->body_contacts && c->task == REX_TASK_MIXED) return fail(REX_EINVAL, "body_contacts is not offered together with REX_TASK_MIXED%s", "");
  for (int k = 0; k < 5; ++k) if (c->noise_stdev[k] < 0.0f) return fail(REX_EINVAL, "noise_stdev must be >= 0%s", "");
  if (c->task == REX_TASK_MIXED) {
    const int allowed = (1 << REX_TASK_WALK) | (1 << REX_TASK_GALLOP) | (1 << REX_TASK_TURN);   // tasks that share one reset pose per signal
    if (c->task_mix == 0 || (c->task_mix & ~allowed)) return fail(REX_EINVAL, "task_mix must be a non-empty subset of {walk, gallop, turn}%s", "");
  }
  if (c->forward_reward_cap != c->forward_reward_cap) return fail(REX_EINVAL, "forward_reward_cap is NaN (use +inf for no cap)%s", "");
  if (c->task == REX_TASK_MIXED && c->energy_weight != rex::task_energy_weight(REX_TASK_WALK))
    return fail(REX_EINVAL, "energy_weight is a per-task constant in a REX_TASK_MIXED batch (gallop 0.005, the others 0.0005): leave it at the default%s", "");
  if (c->mass_scale_lo < 0.0f || c->mass_scale_hi < c->mass_scale_lo || c->friction_lo < 0.0f || c->friction_hi < c->friction_lo)
    return fail(REX_EINVAL, "randomisation ranges must satisfy 0 <= lo <= hi%s", "");
  return REX_OK;
}

// a snapshot record: the state words, and behind all records the observation rings the reset motion leaves behind
static bool has_latency(const RexConfig& c) { return c.pd_latency > 0.0f || c.control_latency > 0.0f; }   // the sim keeps observation rings
static size_t snapshot_floats(const RexSim* s, int nrec) {
  return (size_t)nrec * ((size_t)s->words + (has_latency(s->cfg) ? (size_t)REX_HISTORY_LEN * (size_t)s->dev.hist_words : 0));
}

// ---- regrouping: the buffers and the two launches of the per-step sort (rex_regroup_*_kernel) ----
static int regroup_chunks(const RexSim* s) { return (s->cfg.num_envs + REX_REGROUP_CHUNK - 1) / REX_REGROUP_CHUNK; }
// The per-env sweep counts and the sort's [chunks][64] counts + completion counter, zeroed on the caller's stream: ordered ahead of
// the first rex_regroup_count_kernel also when that stream is non-blocking (the hipStreamSynchronize at the end of rex_create covers
// it).  The key: the task slots of the mix as classes -- one class of 64 bins for a single task; the caller of a mixed batch adds the
// classes' regions (base) and the class array.  (rex_destroy frees whatever was allocated: RexSim starts zeroed.)
static hipError_t regroup_alloc(RexSim* s, void* stream) {
  const size_t n = (size_t)s->cfg.num_envs, counts = (size_t)regroup_chunks(s) * 64 + 1;
  const int bins = 64 / s->dev.n_mix;
  s->regroup_key.bin_width = (s->dev.max_repeat * s->dev.max_iterations + bins - 1) / bins;
  s->regroup_key.bins_per_class = bins; s->regroup_key.n_classes = s->dev.n_mix;
  hipError_t e = hipMalloc(&s->d_sweeps, sizeof(int32_t) * n);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_sweeps, 0, sizeof(int32_t) * n, (hipStream_t)stream);
  if (e == hipSuccess) e = hipMalloc(&s->d_regroup, sizeof(int32_t) * counts);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_regroup, 0, sizeof(int32_t) * counts, (hipStream_t)stream);
  if (e == hipSuccess) s->dev.sweeps = s->d_sweeps;
  return e;
}
// next step's grouping from this step's sweep counts (stream-ordered behind the step): a single-task batch sorts its wave slots
// (d_perm), a mixed batch every task's region of the slot map
static void regroup_launch(RexSim* s, hipStream_t st) {
  if (!s->d_regroup) return;
  const int n = s->cfg.num_envs, chunks = regroup_chunks(s);
  unsigned* done = reinterpret_cast<unsigned*>(s->d_regroup + (size_t)chunks * 64);
  int32_t* out = s->d_perm ? s->d_perm : s->d_slot_env;
  hipLaunchKernelGGL(rex::rex_regroup_count_kernel, dim3(chunks), dim3(256), 0, st, n, s->regroup_key, s->d_sweeps, s->d_regroup, done);
  hipLaunchKernelGGL(rex::rex_regroup_scatter_kernel, dim3(chunks), dim3(256), 0, st, n, s->regroup_key, s->d_sweeps, s->d_regroup, out);
}

int rex_create(const RexConfig* cfg, int device, float* d_state, void* stream, RexSim** out) {
  if (!out || !d_state) return fail(REX_EINVAL, "rex_create: null pointer%s", "");
  int rc = validate(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(REX_ENODEV, "no HIP device visible%s", "");
  if (device < 0 || device >= ndev) return fail(REX_EINVAL, "device index out of range%s", "");
  HIPCHK(hipSetDevice(device));
  RexSim* s = new RexSim();
  s->cfg = *cfg;
  s->device = device;
  s->d_state = d_state;
  s->timing = 0;
  s->have_timing = 0;
  s->have_policy = 0; s->use_policy = false; s->d_rnn_state = nullptr; s->rnn_state_size = 0;
  rex::DevCfg& d = s->dev;
  d.n = cfg->num_envs; d.env_index_base = cfg->env_index_base; d.task = cfg->task; d.signal = cfg->signal;
  d.nsteps = 1;
  d.action_repeat = cfg->action_repeat; d.iterations = cfg->solver_iterations; d.dt = cfg->sim_time_step;
  d.kp = cfg->motor_kp; d.kd = cfg->motor_kd; d.res_thr = sqrtf(fmaxf(cfg->solver_residual_threshold, 0.0f)); d.backwards = cfg->backwards; d.target_position = cfg->target_position;
  d.seed_lo = (uint32_t)cfg->seed; d.seed_hi = (uint32_t)(cfg->seed >> 32);
  d.auto_reset = cfg->auto_reset; d.max_steps = cfg->max_episode_steps;
  d.w_dist = cfg->distance_weight; d.w_energy = cfg->energy_weight; d.w_drift = cfg->drift_weight; d.w_shake = cfg->shake_weight;
  d.fwd_cap = cfg->forward_reward_cap;
  d.action_dim = rex_action_dim(cfg); d.obs_dim = rex_obs_dim(cfg);
  s->epw = pick_envs_per_wave(cfg->num_envs);
  if ((cfg->mark == REX_MARK_ARM || cfg->task == REX_TASK_MIXED || cfg->body_contacts) && s->epw > 16) s->epw = 16;
  if (cfg->body_contacts && s->epw > 8) s->epw = 8;   // the link-box rows of 16 envs take 76.8 KB of LDS: two workgroups per CU, half the SIMDs idle
  if (cfg->body_contacts && cfg->mark == REX_MARK_ARM) s->epw = 4;   // mark arm: 42.6 KB at 8 envs per wave would leave room for three workgroups per CU
  d.n_mix = 1; d.mix_task[0] = cfg->task; d.max_repeat = cfg->action_repeat; d.max_iterations = cfg->solver_iterations;
  for (int k = 1; k < 5; ++k) d.mix_task[k] = cfg->task;
  if (cfg->task == REX_TASK_MIXED) {
    int ts[5];
    d.n_mix = mix_tasks(cfg, ts);
    d.max_repeat = 0;
    for (int k = 0; k < d.n_mix; ++k) { d.mix_task[k] = ts[k]; const int r = rex::task_action_repeat(ts[k]); if (r > d.max_repeat) d.max_repeat = r; }
    for (int k = d.n_mix; k < 5; ++k) d.mix_task[k] = ts[0];
    d.action_repeat = d.max_repeat;          // per-task values replace these inside the mixed kernel (wave by wave)
    d.iterations = d.max_iterations = 60;
  }
  d.trace = nullptr;
  d.slot_env = nullptr; d.block_task = nullptr;
  d.mass_lo = cfg->mass_scale_lo; d.mass_hi = cfg->mass_scale_hi; d.mu_lo = cfg->friction_lo; d.mu_hi = cfg->friction_hi;
  s->words = rex_state_words(cfg);
  d.pose_index = cfg->pose_index; d.pose_value = cfg->pose_value;
  d.range_normalize = cfg->range_normalize;
  d.terrain = nullptr; d.terrain_mid = nullptr; d.n_terrain = 0; d.body_params = nullptr;
  s->mot.params = nullptr; s->mot.on = 0; s->mot.per_motor = 1;
  for (int k = 0; k < 5; ++k) { s->mot.lo[k] = 0.0f; s->mot.hi[k] = 0.0f; }
  d.perm = nullptr; d.sweeps = nullptr; d.clock = nullptr; s->d_clock = nullptr; s->h_clock = nullptr;
  d.geo = rex::HfGeom{256, 20.0f, 20.0f, 127.5f, 127.5f, 254.999f, 254.999f}; d.hf_stride = 65536;   /* model/terrain.py:32-54 */
  d.init_z = cfg->init_height > 0.0f ? cfg->init_height : rex::kInitZ;
  d.anchor = 0.0f;
  if (cfg->on_rack) { d.init_z = 1.0f; d.anchor = rex::kRackAnchor; }   /* INIT_RACK_POSITION, rex.py:11 */
  d.noise_on = 0;
  for (int k = 0; k < 5; ++k) { d.noise[k] = cfg->noise_stdev[k]; if (cfg->noise_stdev[k] > 0.0f) d.noise_on = 1; }
  d.hist = nullptr; d.pd_latency = cfg->pd_latency; d.control_latency = cfg->control_latency;
  d.hist_words = 3 * rex_num_motors(cfg) + 7;
  {
    const double dt = as_written(cfg->sim_time_step), pl = as_written(cfg->pd_latency), cl = as_written(cfg->control_latency);
    d.pd_slots = (int)(pl / dt); d.pd_alpha = (float)((pl - d.pd_slots * dt) / dt);
    d.control_slots = (int)(cl / dt); d.control_alpha = (float)((cl - d.control_slots * dt) / dt);
    d.reset_substeps = (int)(0.5 / dt);
  }
  {
    float b;   /* walk_env.py:104-114, gallop_env.py:119-130 (low=+b, high=-b), turn_env.py:100-110, poses_env.py:115-117 */
    if (cfg->task == REX_TASK_WALK) b = cfg->signal == REX_SIGNAL_IK ? 0.4f : 0.01f;
    else if (cfg->task == REX_TASK_GALLOP) b = cfg->signal == REX_SIGNAL_IK ? -0.4f : -0.3f;
    else if (cfg->task == REX_TASK_TURN) b = 0.01f;
    else b = 0.1f;
    d.act_lo = -b; d.act_hi = b;
    d.obs_hi_ang = (float)(2.0 * M_PI) + 0.01f;                      /* walk_env.py:364-378 + OBSERVATION_EPS */
    d.obs_hi_rate = (float)(2.0 * M_PI) / cfg->sim_time_step + 0.01f;
  }
  d.target_orient = cfg->target_orient; d.init_orient = cfg->init_orient; d.orient_fixed = cfg->orient_fixed;
  if (cfg->on_rack) { d.init_orient = 2.1f; d.orient_fixed |= 2; }   /* turn_env.py:140-143 */
  d.dt_d = as_written(cfg->sim_time_step);
  d.gait_clock_d = cfg->gait_clock_scale > 0.0f ? as_written(cfg->gait_clock_scale) : 1.0;
  {
    // Regrouping (REX_REGROUP=1 / 0 overrides) can pay once a SIMD runs several waves one after the other -- below that the
    // launch ends with its slowest wave whatever the grouping.  Measured on MI355X: round 2, one-workgroup sort
    // (profiles/r02_regroup.md): +10 % on the walking workload (gait clock 1.5, sweep counts 0.96 correlated from step to
    // step), -11 % on the falling one (0.52).  Round 3, many-workgroup sort, falling workload: the step kernel -9 % at
    // 262 144 envs and -5 % at 65 536; with the sort's two launches +5.4 % (132.9 -> 140.1 M env-steps/s) and +0.9 % on
    // the whole step.  On by default from 262 144 envs.
    const char* ov = getenv("REX_REGROUP");
    const bool want = (ov ? atoi(ov) != 0 : cfg->num_envs >= 262144) && cfg->task != REX_TASK_MIXED;   // (a mixed batch is placed by its task-sorted slot map)
    if (want) {
      hipError_t e2 = hipMalloc(&s->d_perm, sizeof(int32_t) * (size_t)cfg->num_envs);
      if (e2 == hipSuccess) e2 = regroup_alloc(s, stream);
      if (e2 != hipSuccess) { (void)rex_destroy(s); return fail(REX_ENOMEM, "hipMalloc(regroup): %s", hipGetErrorString(e2)); }
      hipLaunchKernelGGL(rex::rex_iota_kernel, dim3((cfg->num_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, cfg->num_envs, s->d_perm);
      d.perm = s->d_perm;
    }
  }
  if (cfg->task == REX_TASK_MIXED) {
    std::vector<int32_t> slots, tasks;
    const std::vector<int32_t> cls = rex::mixed_classes(d.n, d.env_index_base, d.seed_lo, d.seed_hi, d.n_mix);   // every env's task slot, drawn once
    int busy = rex::task_slot_map(cls, d.n_mix, d.mix_task, s->epw, slots, tasks);
    // up to one workgroup per SIMD (MI355X: 256 CUs x 4 = 1 024) the launch is one wave per SIMD; the padding of the map must not
    // push it into a second round
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    const int one_round = 4 * (cus > 0 ? cus : 256);
    const bool pinned = getenv("REX_ENVS_PER_WAVE") != nullptr;
    // (the envs per wave decide the arithmetic -- the variants agree to rounding, not bit for bit --, so they are a function of the CONFIG alone:
    //  one round of the machine this library is written for, MI355X's 1 024 SIMDs, whatever partition or device it runs on; the device's own
    //  CU count only enters the regrouping decision below, which leaves results unchanged)
    const int one_round_mi355x = 1024;
    while (!pinned && s->epw < 16 && busy > one_round_mi355x) { s->epw *= 2; busy = rex::task_slot_map(cls, d.n_mix, d.mix_task, s->epw, slots, tasks); }
    // More workgroups than the machine holds at once (one wave per SIMD): the batch is regrouped by sweep counts every
    // step (REX_REGROUP=0 / 1 overrides) -- regions of whole waves per task, sorted inside.  Measured at 16 384 mark-arm envs,
    // 16 envs per wave: the padding of the chunked map is a second round of full-length waves; sorted, the late waves are the short ones.
    const char* ov = getenv("REX_REGROUP");
    const bool regroup = ov ? atoi(ov) != 0 : busy > one_round;
    if (regroup) rex::task_region_map(cls, d.n_mix, d.mix_task, s->epw, slots, tasks, s->regroup_key.base);
    s->mixed_blocks = (int)tasks.size();
    hipError_t e2 = hipMalloc(&s->d_slot_env, sizeof(int32_t) * slots.size());
    if (regroup) {
      if (e2 == hipSuccess) e2 = hipMalloc(&s->d_class, sizeof(int32_t) * cls.size());
      if (e2 == hipSuccess) e2 = hipMemcpy(s->d_class, cls.data(), sizeof(int32_t) * cls.size(), hipMemcpyHostToDevice);   // (the hipMemcpy calls block until the data is on the device)
      if (e2 == hipSuccess) e2 = regroup_alloc(s, stream);
      s->regroup_key.cls = s->d_class;
    }
    if (e2 == hipSuccess) e2 = hipMalloc(&s->d_block_task, sizeof(int32_t) * tasks.size());
    if (e2 == hipSuccess) e2 = hipMemcpy(s->d_slot_env, slots.data(), sizeof(int32_t) * slots.size(), hipMemcpyHostToDevice);
    if (e2 == hipSuccess) e2 = hipMemcpy(s->d_block_task, tasks.data(), sizeof(int32_t) * tasks.size(), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) { (void)rex_destroy(s); return fail(REX_ENOMEM, "task slot map: %s", hipGetErrorString(e2)); }
    d.slot_env = s->d_slot_env; d.block_task = s->d_block_task;
  }
  hipError_t e = hipMalloc(&s->d_snap, sizeof(float) * snapshot_floats(s, d.n_mix));
  if (e != hipSuccess) { (void)rex_destroy(s); return fail(REX_ENOMEM, "hipMalloc(snapshot): %s", hipGetErrorString(e)); }
  (void)hipEventCreate(&s->ev0);
  (void)hipEventCreate(&s->ev1);
  for (int k = 0; k < REX_TIMING_RING; ++k) { s->ring0[k] = nullptr; s->ring1[k] = nullptr; }
  s->timed_steps = 0;
  hipStream_t st = (hipStream_t)stream;
  rc = launch_settle(s, d.n_mix, st, s->d_snap);
  if (rc != REX_OK) { (void)rex_destroy(s); return rc; }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemsetAsync(d_state, 0, sizeof(float) * (size_t)s->words * cfg->num_envs, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)rex_destroy(s);
    return fail(REX_EHIP, "settle kernel: %s", hipGetErrorString(e));
  }
  *out = s;
  return REX_OK;
}

static int install_terrain(RexSim* s, const float* d_heights, const float* d_mids, int k, void* stream) {
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  float* snap = nullptr;
  const int nrec = (k > 0 ? k : 1) * s->dev.n_mix;
  HIPCHK(hipMalloc(&snap, sizeof(float) * snapshot_floats(s, nrec)));
  HIPCHK(hipStreamSynchronize(st));
  (void)hipFree(s->d_snap);
  s->d_snap = snap;
  s->dev.terrain = k > 0 ? d_heights : nullptr;
  s->dev.terrain_mid = k > 0 ? d_mids : nullptr;
  s->dev.n_terrain = k;
  const int rc = launch_settle(s, nrec, st, s->d_snap);
  if (rc != REX_OK) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return REX_OK;
}

int rex_set_terrain(RexSim* s, const float* d_heights, const float* d_mids, int k, void* stream) {
  if (!s || k < 0 || k >= 32768 || (k > 0 && (!d_heights || !d_mids))) return fail(REX_EINVAL, "rex_set_terrain: bad arguments (0 <= k < 32768 fields)%s", "");
  s->dev.geo = rex::HfGeom{256, 20.0f, 20.0f, 127.5f, 127.5f, 254.999f, 254.999f};   /* 256 x 256 vertices, 5 cm cells, centred */
  s->dev.hf_stride = 65536;
  return install_terrain(s, d_heights, d_mids, k, stream);
}

int rex_set_heightfield(RexSim* s, const float* d_heights, const float* d_mids, int k, int nx, int ny, float cell_x, float cell_y,
                        float origin_x, float origin_y, void* stream) {
  if (!s || k <= 0 || !d_heights || !d_mids || nx < 2 || ny < 2 || !(cell_x > 0.0f) || !(cell_y > 0.0f) || (long long)nx * ny > (1ll << 26))
    return fail(REX_EINVAL, "rex_set_heightfield: bad arguments%s", "");
  if ((long long)k * nx * ny >= (1ll << 31)) return fail(REX_EINVAL, "rex_set_heightfield: the pool (k fields of nx * ny heights) must stay below 2^31 floats%s", "");
  rex::HfGeom g;
  g.nx = nx; g.inv_cx = 1.0f / cell_x; g.inv_cy = 1.0f / cell_y;
  g.off_x = 0.5f * (float)(nx - 1) - origin_x * g.inv_cx; g.off_y = 0.5f * (float)(ny - 1) - origin_y * g.inv_cy;
  g.max_x = (float)(nx - 1) - 0.001f; g.max_y = (float)(ny - 1) - 0.001f;
  s->dev.geo = g;
  s->dev.hf_stride = nx * ny;
  return install_terrain(s, d_heights, d_mids, k, stream);
}

int rex_set_history(RexSim* s, float* d_history) {
  if (!s) return fail(REX_EINVAL, "rex_set_history: null sim%s", "");
  // without a latency the delayed observation IS the newest one (rex.py:744-745): the ring is not needed, and the
  // snapshot holds none to restore from
  s->dev.hist = has_latency(s->cfg) ? d_history : nullptr;
  return REX_OK;
}

int rex_set_event_trace(RexSim* s, uint32_t* d_trace) {
  if (!s) return fail(REX_EINVAL, "rex_set_event_trace: null sim%s", "");
  if (d_trace && rex::motor_params_on(s->mot))
    return fail(REX_EINVAL, "rex_set_event_trace: the event trace (a debug aid of the nominal robot) is not offered together with motor parameters%s", "");
  s->dev.trace = d_trace;
  return REX_OK;
}

int rex_set_body_params(RexSim* s, const float* d_params) {
  if (!s) return fail(REX_EINVAL, "rex_set_body_params: null sim%s", "");
  s->dev.body_params = d_params;
  return REX_OK;
}

int rex_set_motor_params(RexSim* s, const float* d_params) {
  if (!s) return fail(REX_EINVAL, "rex_set_motor_params: null sim%s", "");
  if (d_params && s->dev.trace) return fail(REX_EINVAL, "rex_set_motor_params: motor parameters are not offered together with the event trace%s", "");
  s->mot.params = d_params;
  return REX_OK;
}

int rex_set_motor_randomization(RexSim* s, const RexMotorRandom* r) {
  if (!s) return fail(REX_EINVAL, "rex_set_motor_randomization: null sim%s", "");
  rex::MotDev& d = s->mot;
  if (!r) {
    for (int k = 0; k < 5; ++k) { d.lo[k] = 0.0f; d.hi[k] = 0.0f; }
    d.on = 0; d.per_motor = 1;
    return REX_OK;
  }
  static const char* const names[5] = {"strength", "voltage", "damping", "kp", "kd"};
  const float lo[5] = {r->strength_lo, r->voltage_lo, r->damping_lo, r->kp_lo, r->kd_lo};
  const float hi[5] = {r->strength_hi, r->voltage_hi, r->damping_hi, r->kp_hi, r->kd_hi};
  for (int k = 0; k < 5; ++k) {   // (written so that a NaN fails: every comparison with one is false)
    if (!(lo[k] >= 0.0f && hi[k] >= lo[k] && hi[k] <= 3.0e38f))
      return fail(REX_EINVAL, "rex_set_motor_randomization: the %s range must satisfy 0 <= lo <= hi (finite)", names[k]);
  }
  if (r->strength_per_motor != 0 && r->strength_per_motor != 1)
    return fail(REX_EINVAL, "rex_set_motor_randomization: strength_per_motor must be 0 or 1%s", "");
  if (s->dev.trace) return fail(REX_EINVAL, "rex_set_motor_randomization: motor parameters are not offered together with the event trace%s", "");
  d.on = 0;
  for (int k = 0; k < 5; ++k) { d.lo[k] = lo[k]; d.hi[k] = hi[k]; if (hi[k] > 0.0f) d.on = 1; }
  d.per_motor = r->strength_per_motor;
  return REX_OK;
}

int rex_get_motor_params(RexSim* s, float* d_out, void* stream) {
  if (!s || !d_out) return fail(REX_EINVAL, "rex_get_motor_params: null %s", !s ? "sim" : "output buffer");
  HIPCHK(hipSetDevice(s->device));
  const int n = s->dev.n;
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_get_motor_params_kernel<18>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, s->mot, s->d_state, d_out);
  else
    hipLaunchKernelGGL(rex::rex_get_motor_params_kernel<12>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->dev, s->mot, s->d_state, d_out);
  HIPCHK(hipGetLastError());
  return REX_OK;
}

int rex_destroy(RexSim* s) {
  if (!s) return REX_OK;
  (void)hipSetDevice(s->device);
  (void)hipFree(s->d_snap);
  if (s->d_clock) (void)hipFree(s->d_clock);
  free(s->h_clock);
  if (s->d_perm) (void)hipFree(s->d_perm);
  if (s->d_sweeps) (void)hipFree(s->d_sweeps);
  if (s->d_regroup) (void)hipFree(s->d_regroup);
  if (s->d_slot_env) (void)hipFree(s->d_slot_env);
  if (s->d_block_task) (void)hipFree(s->d_block_task);
  if (s->d_class) (void)hipFree(s->d_class);
  if (s->d_polbuf) (void)hipFree(s->d_polbuf);
  if (s->d_vis) (void)hipFree(s->d_vis);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  for (int k = 0; k < REX_TIMING_RING; ++k) if (s->ring0[k]) { (void)hipEventDestroy(s->ring0[k]); (void)hipEventDestroy(s->ring1[k]); }
  delete s;
  return REX_OK;
}

int rex_reset(RexSim* s, const int32_t* d_indices, int n, float* d_obs, void* stream) {
  if (!s) return fail(REX_EINVAL, "rex_reset: null sim%s", "");
  if (has_latency(s->cfg) && !s->dev.hist)
    return fail(REX_EINVAL, "rex_reset: pd_latency/control_latency are set but rex_set_history() was not called%s", "");
  const int count = d_indices ? n : s->cfg.num_envs;
  if (count <= 0) return d_indices ? REX_OK : fail(REX_EINVAL, "rex_reset: empty%s", "");
  HIPCHK(hipSetDevice(s->device));
  const int block = 256;
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_reset_kernel<18>, dim3((count + block - 1) / block), dim3(block), 0, (hipStream_t)stream, s->dev,
                       s->d_state, s->d_snap, d_indices, count, d_obs);
  else
    hipLaunchKernelGGL(rex::rex_reset_kernel<12>, dim3((count + block - 1) / block), dim3(block), 0, (hipStream_t)stream, s->dev,
                       s->d_state, s->d_snap, d_indices, count, d_obs);
  HIPCHK(hipGetLastError());
  if (s->have_policy == 2) {   // the recurrent actor: an episode starts from a zero GRU state
    hipLaunchKernelGGL(rex::rex_zero_rnn_state_kernel, dim3((count + block - 1) / block), dim3(block), 0, (hipStream_t)stream, s->d_rnn_state,
                       s->cfg.num_envs, s->rnn_state_size, d_indices, count);
    HIPCHK(hipGetLastError());
  }
  return REX_OK;
}

static int step_launch(RexSim* s, int num_steps, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream);

int rex_step(RexSim* s, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream) {
  if (!s || !d_action || !d_obs || !d_reward || !d_done) return fail(REX_EINVAL, "rex_step: null pointer%s", "");
  return step_launch(s, 1, d_action, d_obs, d_reward, d_done, d_motor_cmd, stream);
}

int rex_step_segment(RexSim* s, int num_steps, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream) {
  if (!s || !d_action || !d_obs || !d_reward || !d_done) return fail(REX_EINVAL, "rex_step_segment: null pointer%s", "");
  if (num_steps < 1) return fail(REX_EINVAL, "rex_step_segment: num_steps must be at least 1%s", "");
  const long long width = std::max(std::max(rex_action_dim(&s->cfg), rex_obs_dim(&s->cfg)), rex_num_motors(&s->cfg));
  if ((long long)num_steps * s->cfg.num_envs * width >= (1ll << 31))
    return fail(REX_EINVAL, "rex_step_segment: a segment this long exceeds the 32-bit element offsets of its blocks (num_steps * num_envs * row width < 2^31)%s", "");
  return step_launch(s, num_steps, d_action, d_obs, d_reward, d_done, d_motor_cmd, stream);
}

// ---- the actor inside the launch (rex_policy.h) ----
static int rows_floats_per_env(const RexSim* s) {   // the contact-row region of the step kernel's LDS, per env of a wave: the actor's scratch
  const bool arm = s->cfg.mark == REX_MARK_ARM;
  const int legf4 = REX_LEG_F4_OF(s->epw, arm, false);
  return 4 * (arm ? REX_LDS_F4_PER_ENV_ARM_OF(s->epw) : REX_ROWS_F4_OF(legf4));
}

// what rex_set_policy and rex_set_policy_recurrent share: may this sim run a fused actor at all, the checks in the order the caller has
// always met them (the entry point's own -- its layer sizes against the LDS scratch, its null pointers -- sit between the dimensions and
// obs_clip), the packed actor's buffer grown to `total` floats and the fields of PolDev that do not depend on the kind of actor
extern "C++" {   // (a template, inside the ABI's extern "C")
template <class OwnChecks>
static int policy_install_common(RexSim* s, const char* who, int obs_dim, int action_dim, const float* d_obs_mean, float obs_clip, int sample, uint64_t seed,
                                 OwnChecks own_checks) {
  if (!rex_step_variant_offered(step_group(s), REX_MODE_POL, false) || s->epw > 16)   // (POL and RNN are offered to the same groups)
    return fail(REX_EINVAL, "%s: the fused actor runs in the single-task lane-group kernels (not REX_TASK_MIXED, body_contacts = 0, REX_ENVS_PER_WAVE <= 16)", who);
  if (!s->cfg.range_normalize)
    return fail(REX_EINVAL, "%s: the sim must fold the reference's wrapper stack (RexConfig.range_normalize = 1): the agents act through "
                            "RangeNormalize + ClipAction (playground/trainer.py:48-52)", who);
  if (obs_dim != rex_obs_dim(&s->cfg) || action_dim != rex_action_dim(&s->cfg))
    return failf(REX_EINVAL, "%s: obs_dim / action_dim %d / %d do not match the sim's %d / %d", who, obs_dim, action_dim, rex_obs_dim(&s->cfg), rex_action_dim(&s->cfg));
  int total = 0;      // floats of the packed actor: the entry point's checks work it out from the sizes they have accepted
  const int rc = own_checks(&total);
  if (rc != REX_OK) return rc;
  if (!(obs_clip > 0.0f) && d_obs_mean) return fail(REX_EINVAL, "%s: obs_clip must be positive", who);
  HIPCHK(hipSetDevice(s->device));
  if (total > s->polbuf_floats) {            // (one buffer, one policy installed at a time; a launch may still be reading the old buffer: the free below waits for the device)
    if (s->d_polbuf) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(s->d_polbuf); s->d_polbuf = nullptr; s->polbuf_floats = 0; }
    if (hipMalloc(&s->d_polbuf, sizeof(float) * (size_t)total) != hipSuccess) return fail(REX_ENOMEM, "%s: hipMalloc", who);
    s->polbuf_floats = total;
  }
  rex::PolDev& d = s->pol;
  d.pk = s->d_polbuf; d.obs_in = nullptr; d.action_out = nullptr; d.mean_out = nullptr;
  d.obs_clip = d_obs_mean ? obs_clip : 0.0f; d.sample = sample ? 1 : 0;
  d.seed_lo = (uint32_t)seed; d.seed_hi = (uint32_t)(seed >> 32);
  return REX_OK;
}
}

int rex_set_policy(RexSim* s, const RexPolicy* p, void* stream) {
  if (!s) return fail(REX_EINVAL, "rex_set_policy: null sim%s", "");
  if (!p) { s->have_policy = 0; return REX_OK; }
  rex::PolOff off;
  const int rc = policy_install_common(s, "rex_set_policy", p->obs_dim, p->action_dim, p->d_obs_mean, p->obs_clip, p->sample, p->seed, [&](int* total) {
    if (p->hidden1 < 1 || p->hidden2 < 1 || p->hidden1 > 4096 || p->hidden2 > 4096 || rex::policy_scratch_floats(p->obs_dim, p->hidden1, p->hidden2) > rows_floats_per_env(s))
      return failf(REX_EINVAL, "rex_set_policy: hidden layers of %d and %d units need %d floats of LDS per env, this kernel variant has %d", p->hidden1, p->hidden2,
                   rex::policy_scratch_floats(p->obs_dim, p->hidden1 > 0 ? p->hidden1 : 0, p->hidden2 > 0 ? p->hidden2 : 0), rows_floats_per_env(s));
    if (!p->d_w1 || !p->d_b1 || !p->d_w2 || !p->d_b2 || !p->d_w3 || !p->d_b3 || !p->d_logstd || (!p->d_obs_mean) != (!p->d_obs_scale))
      return fail(REX_EINVAL, "rex_set_policy: null weight pointer (d_obs_mean and d_obs_scale go together)%s", "");
    off = rex::policy_offsets(p->obs_dim, p->action_dim, p->hidden1, p->hidden2);
    *total = off.total;
    return (int)REX_OK;
  });
  if (rc != REX_OK) return rc;
  // pack (stream-ordered: behind the launches that read the previous contents, ahead of those that follow): input-major matrices ->
  // [k / 4][unit][4], every block 16-byte aligned, zero padding (rex_policy.h)
  rex::PolSrc src{p->d_w1, p->d_b1, p->d_w2, p->d_b2, p->d_w3, p->d_b3, p->d_logstd, p->d_obs_mean, p->d_obs_scale};
  hipLaunchKernelGGL(rex::rex_pack_policy_kernel, dim3((off.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, p->obs_dim, p->action_dim, p->hidden1,
                     p->hidden2, s->d_polbuf);
  HIPCHK(hipGetLastError());
  rex::PolDev& d = s->pol;
  d.h1 = p->hidden1; d.h2 = p->hidden2;
  {   // one copy of the packed actor per four-wave workgroup, in dynamic LDS, if it fits next to the waves' rows (MI355X: 160 KB per CU)
    const bool arm = s->cfg.mark == REX_MARK_ARM;
    const int wave_bytes = (rows_floats_per_env(s) / 4 + REX_PARK_F4_OF(s->epw, arm)) * s->epw * 16;
    const int want = off.total * 4;
    const char* ov = getenv("REX_POLICY_LDS");      // developer A/B runs: 0 streams the weights from L2 everywhere
    const bool fits = REX_POLICY_WAVES(s->epw) > 1 && REX_POLICY_WAVES(s->epw) * wave_bytes + want <= 160 * 1024 && !(ov && atoi(ov) == 0);
    s->pol_lds_bytes = fits ? want : 0;
    d.in_lds = fits ? 1 : 0;
  }
  s->have_policy = 1;
  return REX_OK;
}

int rex_set_policy_recurrent(RexSim* s, const RexRecurrentPolicy* p, void* stream) {
  if (!s) return fail(REX_EINVAL, "rex_set_policy_recurrent: null sim%s", "");
  if (!p) { s->have_policy = 0; return REX_OK; }
  rex::RnnOff off;
  const int rc = policy_install_common(s, "rex_set_policy_recurrent", p->obs_dim, p->action_dim, p->d_obs_mean, p->obs_clip, p->sample, p->seed, [&](int* total) {
    if (p->state_size < 1 || p->state_size > REX_RNN_MAX_STATE)
      return failf(REX_EINVAL, "rex_set_policy_recurrent: state_size %d: the cell is one matrix-core pass per gate, 1..%d units", p->state_size, REX_RNN_MAX_STATE);
    if (p->hidden1 < 1 || p->hidden1 > 4096 || rex::rnn_scratch_floats(p->obs_dim, p->hidden1, p->state_size) > rows_floats_per_env(s))
      return failf(REX_EINVAL, "rex_set_policy_recurrent: a layer of %d units and a cell of %d need %d floats of LDS per env, this kernel variant has %d", p->hidden1, p->state_size,
                   rex::rnn_scratch_floats(p->obs_dim, p->hidden1 > 0 ? p->hidden1 : 0, p->state_size), rows_floats_per_env(s));
    if (!p->d_w1 || !p->d_b1 || !p->d_wg || !p->d_bg || !p->d_wc || !p->d_bc || !p->d_w3 || !p->d_b3 || !p->d_logstd || (!p->d_obs_mean) != (!p->d_obs_scale))
      return fail(REX_EINVAL, "rex_set_policy_recurrent: null weight pointer (d_obs_mean and d_obs_scale go together)%s", "");
    if (!p->d_state) return fail(REX_EINVAL, "rex_set_policy_recurrent: null d_state (the GRU state [state_size][num_envs] is caller-owned)%s", "");
    off = rex::rnn_offsets(p->obs_dim, p->action_dim, p->hidden1, p->state_size);
    *total = off.total;
    return (int)REX_OK;
  });
  if (rc != REX_OK) return rc;
  rex::RnnSrc src{p->d_w1, p->d_b1, p->d_wg, p->d_bg, p->d_wc, p->d_bc, p->d_w3, p->d_b3, p->d_logstd, p->d_obs_mean, p->d_obs_scale};
  hipLaunchKernelGGL(rex::rex_pack_rnn_kernel, dim3((off.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, p->obs_dim, p->action_dim, p->hidden1,
                     p->state_size, s->d_polbuf);
  HIPCHK(hipGetLastError());
  rex::PolDev& d = s->pol;
  d.h1 = p->hidden1; d.h2 = p->state_size;
  d.in_lds = 0;                                  // 364 KB for 4-200-(100)-2: streamed from L2 at every envs-per-wave
  s->pol_lds_bytes = 0;
  s->d_rnn_state = p->d_state; s->rnn_state_size = p->state_size;
  s->have_policy = 2;
  return REX_OK;
}

static int policy_launch(RexSim* s, const char* who, int num_steps, const float* d_obs_in, float* d_action, float* d_mean, float* d_obs, float* d_reward,
                         uint8_t* d_done, float* d_motor_cmd, void* stream) {
  if (!s || !d_obs_in || !d_action || !d_obs || !d_reward || !d_done) return fail(REX_EINVAL, "%s: null pointer", who);
  if (!s->have_policy) return fail(REX_EINVAL, "%s: no policy set (rex_set_policy / rex_set_policy_recurrent)", who);
  if (s->dev.trace) return fail(REX_EINVAL, "%s: not available while an event trace is set (rex_set_event_trace)", who);
  if (num_steps < 1) return fail(REX_EINVAL, "%s: num_steps must be at least 1", who);
  if (d_obs_in == d_obs) return fail(REX_EINVAL, "%s: d_obs must not alias d_obs_in", who);
  const long long width = std::max(std::max(rex_action_dim(&s->cfg), rex_obs_dim(&s->cfg)), rex_num_motors(&s->cfg));
  if ((long long)num_steps * s->cfg.num_envs * width >= (1ll << 31))
    return fail(REX_EINVAL, "%s: a segment this long exceeds the 32-bit element offsets of its blocks (num_steps * num_envs * row width < 2^31)", who);
  s->pol.obs_in = d_obs_in; s->pol.action_out = d_action; s->pol.mean_out = d_mean;
  return step_launch(s, -num_steps, nullptr, d_obs, d_reward, d_done, d_motor_cmd, stream);   // (negative: the fused-actor kernels)
}
int rex_step_policy(RexSim* s, const float* d_obs_in, float* d_action, float* d_mean, float* d_obs, float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream) {
  return policy_launch(s, "rex_step_policy", 1, d_obs_in, d_action, d_mean, d_obs, d_reward, d_done, d_motor_cmd, stream);
}
int rex_step_segment_policy(RexSim* s, int num_steps, const float* d_obs_in, float* d_action, float* d_mean, float* d_obs, float* d_reward, uint8_t* d_done,
                            float* d_motor_cmd, void* stream) {
  return policy_launch(s, "rex_step_segment_policy", num_steps, d_obs_in, d_action, d_mean, d_obs, d_reward, d_done, d_motor_cmd, stream);
}

static int step_launch(RexSim* s, int num_steps, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, float* d_motor_cmd, void* stream) {
  HIPCHK(hipSetDevice(s->device));
  if (s->dev.trace && rex::motor_params_on(s->mot))
    return fail(REX_EINVAL, "the event trace (a debug aid of the nominal robot) is not offered together with motor parameters%s", "");
  s->use_policy = num_steps < 0;
  if (num_steps < 0) num_steps = -num_steps;
  s->dev.nsteps = num_steps;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = s->d_slot_env ? s->mixed_blocks : (s->cfg.num_envs + s->epw - 1) / s->epw;
  hipEvent_t e0 = s->ev0, e1 = s->ev1;
  if (s->timing == 2) {
    const int k = (int)(s->timed_steps % REX_TIMING_RING);
    if (!s->ring0[k]) { HIPCHK(hipEventCreate(&s->ring0[k])); HIPCHK(hipEventCreate(&s->ring1[k])); }
    e0 = s->ring0[k]; e1 = s->ring1[k];
  }
  if (s->timing == 3 && s->timed_steps < REX_CLOCK_SLOTS) {   // device-side timestamps: this launch's (min start, max end) slot
    s->dev.clock = s->d_clock + 2 * REX_CLOCK_WAYS * s->timed_steps;   // (all slots were primed by rex_set_timing: nothing is copied per
    s->timed_steps++;                                         // launch, the queue stays as full as in an untimed run)
  } else s->dev.clock = nullptr;
  if (s->timing == 1 || s->timing == 2) HIPCHK(hipEventRecord(e0, st));
  int rc = launch_step(s, blocks, st, d_action, d_obs, d_reward, d_done, d_motor_cmd);
  if (rc != REX_OK) return rc;
  {   // developer probe (tools/launch_gap.py): REX_STEP_REPEAT=R issues the launch R times back to back from C
    static const int repeat = getenv("REX_STEP_REPEAT") ? atoi(getenv("REX_STEP_REPEAT")) : 1;
    for (int k = 1; k < repeat; ++k) (void)launch_step(s, blocks, st, d_action, d_obs, d_reward, d_done, d_motor_cmd);
  }
  HIPCHK(hipGetLastError());
  // (the timed span is the step kernel's: the regrouping launches below are not part of it)
  if (s->timing == 1 || s->timing == 2) { HIPCHK(hipEventRecord(e1, st)); s->have_timing = 1; if (s->timing == 2) s->timed_steps++; }
  regroup_launch(s, st);
  return REX_OK;
}

int rex_mixed_slot_map(const RexConfig* cfg, int envs_per_wave, int32_t* slots, int32_t* tasks, int max_blocks) {
  if (validate(cfg)) return REX_EINVAL;
  if (cfg->task != REX_TASK_MIXED || (envs_per_wave != 4 && envs_per_wave != 8 && envs_per_wave != 16))
    return fail(REX_EINVAL, "rex_mixed_slot_map: a REX_TASK_MIXED config and 4, 8 or 16 envs per wave%s", "");
  int ts[5];
  const int n_mix = mix_tasks(cfg, ts);
  int32_t mix_task[5];
  for (int k = 0; k < 5; ++k) mix_task[k] = ts[k < n_mix ? k : 0];
  std::vector<int32_t> sl, tk;
  rex::task_slot_map(rex::mixed_classes(cfg->num_envs, cfg->env_index_base, (uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32), n_mix), n_mix, mix_task,
                     envs_per_wave, sl, tk);
  if (slots && tasks) {
    if ((int)tk.size() > max_blocks) return fail(REX_EINVAL, "rex_mixed_slot_map: buffers too small%s", "");
    memcpy(slots, sl.data(), sizeof(int32_t) * sl.size());
    memcpy(tasks, tk.data(), sizeof(int32_t) * tk.size());
  }
  return (int)tk.size();
}

int rex_envs_per_wave(const RexSim* s) { return s ? s->epw : REX_EINVAL; }

int rex_get_sweeps(RexSim* s, int32_t* d_out, void* stream) {
  if (!s || !d_out) return fail(REX_EINVAL, "rex_get_sweeps: null pointer%s", "");
  if (!s->d_sweeps) return fail(REX_EINVAL, "rex_get_sweeps: this sim does not regroup (REX_REGROUP=1 was not set when it was created)%s", "");
  HIPCHK(hipMemcpyAsync(d_out, s->d_sweeps, sizeof(int32_t) * (size_t)s->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return REX_OK;
}

int rex_set_timing(RexSim* s, int enable) {
  if (!s) return fail(REX_EINVAL, "rex_set_timing: null sim%s", "");
  s->timing = (enable == 2 || enable == 3) ? enable : (enable ? 1 : 0);
  s->have_timing = 0;
  s->timed_steps = 0;
  if (s->timing == 3) {   // the next REX_CLOCK_SLOTS launches are timed on the device; prime their (min, max) slots
    HIPCHK(hipSetDevice(s->device));
    const size_t words = (size_t)2 * REX_CLOCK_WAYS * REX_CLOCK_SLOTS;
    if (!s->d_clock) HIPCHK(hipMalloc(&s->d_clock, sizeof(unsigned long long) * words));
    if (!s->h_clock) s->h_clock = (unsigned long long*)malloc(sizeof(unsigned long long) * words);
    if (!s->h_clock) return fail(REX_ENOMEM, "rex_set_timing: host buffer%s", "");
    for (size_t k = 0; k < words / 2; ++k) { s->h_clock[2 * k] = ~0ull; s->h_clock[2 * k + 1] = 0ull; }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(s->d_clock, s->h_clock, sizeof(unsigned long long) * words, hipMemcpyHostToDevice));
  }
  return REX_OK;
}

int rex_step_times_ms(RexSim* s, float* ms, int max_count) {
  if (!s || !ms || max_count <= 0) return fail(REX_EINVAL, "rex_step_times_ms: bad arguments%s", "");
  if ((s->timing != 2 && s->timing != 3) || s->timed_steps == 0) return 0;
  const long long cap = s->timing == 3 ? REX_CLOCK_SLOTS : REX_TIMING_RING;
  long long have = s->timed_steps < cap ? s->timed_steps : cap;
  int n = (int)(have < max_count ? have : max_count);
  HIPCHK(hipSetDevice(s->device));
  if (s->timing == 3) {
    unsigned long long* ticks = s->h_clock;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(ticks, s->d_clock, sizeof(unsigned long long) * 2 * REX_CLOCK_WAYS * REX_CLOCK_SLOTS, hipMemcpyDeviceToHost));
    int khz = 100000;   // s_memrealtime: constant 100 MHz on gfx9
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, s->device);
    for (int j = 0; j < n; ++j) {
      const unsigned long long* t = ticks + (size_t)2 * REX_CLOCK_WAYS * (size_t)(s->timed_steps - n + j);
      unsigned long long first = ~0ull, last = 0ull;       // first wave start / last wave end over the launch's tick pairs
      for (int w = 0; w < REX_CLOCK_WAYS; ++w) { if (t[2 * w] < first) first = t[2 * w]; if (t[2 * w + 1] > last) last = t[2 * w + 1]; }
      ms[j] = last >= first ? (float)((double)(last - first) / (double)khz) : 0.0f;
    }
    return n;
  }
  HIPCHK(hipEventSynchronize(s->ring1[(int)((s->timed_steps - 1) % REX_TIMING_RING)]));
  for (int j = 0; j < n; ++j) {   // oldest of the last n first
    const int k = (int)((s->timed_steps - n + j) % REX_TIMING_RING);
    HIPCHK(hipEventElapsedTime(&ms[j], s->ring0[k], s->ring1[k]));
  }
  return n;
}

int rex_last_step_ms(RexSim* s, float* ms) {
  if (!s || !ms) return fail(REX_EINVAL, "rex_last_step_ms: null pointer%s", "");
  if (!s->have_timing) return fail(REX_EINVAL, "rex_last_step_ms: no timed step recorded%s", "");
  HIPCHK(hipEventSynchronize(s->ev1));
  HIPCHK(hipEventElapsedTime(ms, s->ev0, s->ev1));
  return REX_OK;
}

int rex_default_camera(RexCamera* cam) {
  if (!cam) return fail(REX_EINVAL, "rex_default_camera: null pointer%s", "");
  *cam = RexCamera{1.0f, 0.0f, -30.0f, 60.0f, 0.1f, 100.0f};   // rex_gym_env.py:214-216 and the projection of render(), :416-439
  return REX_OK;
}

// the checks rex_render and rex_render_visual share, and the camera of the launch in world axes
static int render_camera(const char* who, RexSim* s, const RexCamera* cam, const int32_t* d_env_ids, int n, int width, int height,
                         uint8_t* d_rgb, rex::RenderCam& rc) {
  if (!s || !cam || !d_env_ids || !d_rgb) return failf(REX_EINVAL, "%s: null pointer", who);
  if (n < 1 || width < 1 || width > 4096 || height < 1 || height > 4096 || (long long)n * width * height * 3 >= (1ll << 31))
    return failf(REX_EINVAL, "%s: bad image batch (n %d, %d x %d: n >= 1, sides 1..4096, n * w * h * 3 < 2^31)", who, n, width, height);
  if (!(cam->distance > 0.0f) || !(cam->fov_deg > 0.0f) || !(cam->fov_deg < 180.0f) || !(cam->near_plane > 0.0f) ||
      !(cam->far_plane > cam->near_plane))
    return failf(REX_EINVAL, "%s: camera distance, fov and near plane must be positive, fov < 180 and far > near", who);
  // b3ComputeViewMatrixFromYawPitchRoll (up axis z): eye offset R (0, -d, 0), up R (0, 0, 1), R = Rz(yaw) Rx(pitch) (roll 0);
  // then the look-at basis: forward = -offset / d, right = forward x up, up' = right x forward
  const double deg = 3.14159265358979323846 / 180.0;
  const double cy = cos(cam->yaw_deg * deg), sy = sin(cam->yaw_deg * deg), cp = cos(cam->pitch_deg * deg), sp = sin(cam->pitch_deg * deg);
  const double d = cam->distance;
  const double off[3] = {sy * cp * d, -cy * cp * d, -sp * d};            // Rz(yaw) Rx(pitch) (0, -d, 0)
  const double upv[3] = {-sy * -sp, cy * -sp, cp};                       // Rz(yaw) Rx(pitch) (0, 0, 1)
  const double f[3] = {-off[0] / d, -off[1] / d, -off[2] / d};
  double r[3] = {f[1] * upv[2] - f[2] * upv[1], f[2] * upv[0] - f[0] * upv[2], f[0] * upv[1] - f[1] * upv[0]};
  const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  r[0] /= rn; r[1] /= rn; r[2] /= rn;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  for (int k = 0; k < 3; ++k) { rc.off[k] = (float)off[k]; rc.fwd[k] = (float)f[k]; rc.right[k] = (float)r[k]; rc.up[k] = (float)u[k]; }
  const double ty = tan(0.5 * cam->fov_deg * deg);
  rc.tan_y = (float)ty; rc.tan_x = (float)(ty * (double)width / (double)height);
  rc.near_plane = cam->near_plane; rc.far_plane = cam->far_plane;
  return REX_OK;
}

int rex_render(RexSim* s, const RexCamera* cam, const int32_t* d_env_ids, int n, int width, int height, uint8_t* d_rgb, float* d_depth,
               int16_t* d_seg, void* stream) {
  rex::RenderCam rc;
  const int rc_err = render_camera("rex_render", s, cam, d_env_ids, n, width, height, d_rgb, rc);
  if (rc_err != REX_OK) return rc_err;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_render(s, rc, d_env_ids, n, width, height, d_rgb, d_depth, d_seg, (hipStream_t)stream));
  return REX_OK;
}

int rex_render_set_visuals(RexSim* s, const float* nodes, int num_nodes, const float* tris, int num_tris, const int32_t* inst_root,
                           const float* inst_box, int num_inst, void* stream) {
  if (!s || !inst_root || !inst_box || (num_nodes > 0 && !nodes) || (num_tris > 0 && !tris))
    return fail(REX_EINVAL, "rex_render_set_visuals: null pointer%s", "");
  const int want = s->cfg.mark == REX_MARK_ARM ? REX_VIS_N_ARM : REX_VIS_N_BASE;
  if (num_inst != want) return failf(REX_EINVAL, "rex_render_set_visuals: %d instances, this sim's mark draws %d", num_inst, want);
  if (num_nodes < 0 || num_tris < 0 || num_nodes >= (1 << 26) || num_tris >= (1 << 26))
    return failf(REX_EINVAL, "rex_render_set_visuals: bad counts (%d nodes, %d triangles: 0 .. 2^26)", num_nodes, num_tris);
  // every child index points forward (so the tree is acyclic), every leaf's triangles exist, and no root reaches deeper than
  // kMeshStack levels of inner nodes (the kernel's traversal stack)
  std::vector<int> depth(num_nodes, 0), parents(num_nodes, 0);
  for (int i = 0; i < num_nodes; ++i)
    for (int c = 0; c < 2; ++c) {
      int32_t ch;
      memcpy(&ch, nodes + 16 * (size_t)i + 12 + c, 4);
      if (ch >= 0) {
        if (ch <= i || ch >= num_nodes) return failf(REX_EINVAL, "rex_render_set_visuals: node %d: child %d out of range", i, ch);
        ++parents[ch];
      } else {
        const long long start = (long long)(~ch >> 3), cnt = (~ch & 7) + 1;
        if (start + cnt > num_tris) return failf(REX_EINVAL, "rex_render_set_visuals: node %d: leaf triangles %lld..%lld out of range", i, start, start + cnt);
      }
    }
  for (int i = 0; i < num_nodes; ++i) {
    if (parents[i] > 1) return failf(REX_EINVAL, "rex_render_set_visuals: node %d has %d parents", i, parents[i]);
    if (parents[i] == 0) depth[i] = 1;
    if (depth[i] > rex::kMeshStack) return failf(REX_EINVAL, "rex_render_set_visuals: a tree deeper than %d levels", rex::kMeshStack);
    for (int c = 0; c < 2; ++c) {
      int32_t ch;
      memcpy(&ch, nodes + 16 * (size_t)i + 12 + c, 4);
      if (ch >= 0) depth[ch] = depth[i] + 1;
    }
  }
  for (int k = 0; k < num_inst; ++k) {
    if (inst_root[k] < -1 || inst_root[k] >= num_nodes || (inst_root[k] >= 0 && parents[inst_root[k]] != 0))
      return failf(REX_EINVAL, "rex_render_set_visuals: instance %d: root %d is not a root node", k, inst_root[k]);
  }
  HIPCHK(hipSetDevice(s->device));
  const size_t b_nodes = 64 * (size_t)num_nodes, b_tris = 36 * (size_t)num_tris, b_root = 4 * (size_t)num_inst;
  const size_t o_tris = b_nodes, o_root = (o_tris + b_tris + 15) & ~(size_t)15, o_box = o_root + ((b_root + 15) & ~(size_t)15);
  const size_t total = o_box + 24 * (size_t)num_inst;
  void* buf = nullptr;
  hipError_t e = hipMalloc(&buf, total);
  if (e != hipSuccess) return fail(REX_ENOMEM, "rex_render_set_visuals: hipMalloc: %s", hipGetErrorString(e));
  char* b = static_cast<char*>(buf);
  hipStream_t st = (hipStream_t)stream;
  if (b_nodes) e = hipMemcpyAsync(b, nodes, b_nodes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && b_tris) e = hipMemcpyAsync(b + o_tris, tris, b_tris, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_root, inst_root, b_root, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_box, inst_box, 24 * (size_t)num_inst, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the host arrays are the caller's: done with them on return
  if (e != hipSuccess) { (void)hipFree(buf); return fail(REX_EHIP, "rex_render_set_visuals: upload: %s", hipGetErrorString(e)); }
  if (s->d_vis) (void)hipFree(s->d_vis);
  s->d_vis = buf;
  s->d_vis_nodes = reinterpret_cast<float*>(b);
  s->d_vis_tris = reinterpret_cast<float*>(b + o_tris);
  s->d_vis_root = reinterpret_cast<int32_t*>(b + o_root);
  s->d_vis_box = reinterpret_cast<float*>(b + o_box);
  return REX_OK;
}

int rex_render_visual(RexSim* s, const RexCamera* cam, const int32_t* d_env_ids, int n, int width, int height, uint8_t* d_rgb,
                      float* d_depth, int16_t* d_seg, void* stream) {
  rex::RenderCam rc;
  const int rc_err = render_camera("rex_render_visual", s, cam, d_env_ids, n, width, height, d_rgb, rc);
  if (rc_err != REX_OK) return rc_err;
  if (!s->d_vis) return fail(REX_EINVAL, "rex_render_visual: no visual meshes set (rex_render_set_visuals)%s", "");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_render_mesh(s, rc, d_env_ids, n, width, height, d_rgb, d_depth, d_seg, (hipStream_t)stream));
  return REX_OK;
}

static_assert(sizeof(RexDepthSensor) == 60, "RexDepthSensor: 12 floats and 3 int32, no padding (rex_gym_amd/_lib.py mirrors it)");

int rex_default_depth_sensor(RexDepthSensor* d) {
  if (!d) return fail(REX_EINVAL, "rex_default_depth_sensor: null pointer%s", "");
  const float c30 = 0.86602540378443865f, s30 = 0.5f;
  *d = RexDepthSensor{{-0.18f, 0.0f, 0.0f}, {-c30, 0.0f, -s30}, {-s30, 0.0f, c30}, 60.0f, 0.02f, 10.0f, 32, 24, 1};
  return REX_OK;
}

// rows of a sensor call: ids given, or envs 0 .. n - 1
static int sense_rows(const char* who, RexSim* s, const int32_t* d_env_ids, int n) {
  if (!s) return failf(REX_EINVAL, "%s: null sim", who);
  if (n < 1) return failf(REX_EINVAL, "%s: n %d: at least one env", who, n);
  if (!d_env_ids && n > s->cfg.num_envs) return failf(REX_EINVAL, "%s: n %d without env ids, the sim has %d envs", who, n, s->cfg.num_envs);
  return REX_OK;
}

int rex_sense_depth(RexSim* s, const RexDepthSensor* d, const int32_t* d_env_ids, int n, float* d_depth, void* stream) {
  const char* who = "rex_sense_depth";
  if (!d || !d_depth) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = sense_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (d->width < 1 || d->width > 1024 || d->height < 1 || d->height > 1024 || (long long)n * d->width * d->height >= (1ll << 29))
    return failf(REX_EINVAL, "%s: bad image batch (n %d, %d x %d: sides 1..1024, n * w * h < 2^29)", who, n, d->width, d->height);
  const float* f = d->pos;   // pos, fwd, up, fov_deg, near_plane, far_plane: 12 consecutive floats
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(f[k])) return failf(REX_EINVAL, "%s: a non-finite field", who);
  if (!(d->fov_deg > 0.0f) || !(d->fov_deg < 180.0f) || !(d->near_plane > 0.0f) || !(d->far_plane > d->near_plane))
    return failf(REX_EINVAL, "%s: fov must lie in (0, 180), the near plane be positive and far > near", who);
  if (d->see_robot != 0 && d->see_robot != 1) return failf(REX_EINVAL, "%s: see_robot must be 0 or 1", who);
  const double fw[3] = {d->fwd[0], d->fwd[1], d->fwd[2]}, up[3] = {d->up[0], d->up[1], d->up[2]};
  const double nf = sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]), nu = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
  const double dot = fw[0] * up[0] + fw[1] * up[1] + fw[2] * up[2];
  if (fabs(nf - 1.0) > 1e-3 || fabs(nu - 1.0) > 1e-3 || fabs(dot) > 1e-3)
    return failf(REX_EINVAL, "%s: fwd and up must be unit vectors orthogonal to each other (|fwd| %.6f, |up| %.6f, fwd . up %.6f)", who, nf, nu, dot);
  rex::SenseMount m;
  const double r[3] = {fw[1] * up[2] - fw[2] * up[1], fw[2] * up[0] - fw[0] * up[2], fw[0] * up[1] - fw[1] * up[0]};
  for (int k = 0; k < 3; ++k) { m.pos[k] = d->pos[k]; m.fwd[k] = d->fwd[k]; m.up[k] = d->up[k]; m.right[k] = (float)r[k]; }
  const double ty = tan(0.5 * (double)d->fov_deg * (3.14159265358979323846 / 180.0));
  m.tan_y = (float)ty; m.tan_x = (float)(ty * (double)d->width / (double)d->height);
  m.near_plane = d->near_plane; m.far_plane = d->far_plane; m.see_robot = d->see_robot;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_sense_depth(s, m, d_env_ids, n, d->width, d->height, d_depth, (hipStream_t)stream));
  return REX_OK;
}

int rex_height_scan(RexSim* s, const float* d_points, int K, int relative, const int32_t* d_env_ids, int n, float* d_out, void* stream) {
  const char* who = "rex_height_scan";
  if (!d_points || !d_out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = sense_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (K < 1 || K > 4096 || (long long)n * K >= (1ll << 31)) return failf(REX_EINVAL, "%s: K %d, n %d: K in 1..4096, n * K < 2^31", who, K, n);
  if (relative != 0 && relative != 1) return failf(REX_EINVAL, "%s: relative must be 0 or 1", who);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_height_scan(s, d_points, K, relative, d_env_ids, n, d_out, (hipStream_t)stream));
  return REX_OK;
}

static_assert(sizeof(RexKinematicsOut) == 80, "RexKinematicsOut: 10 pointers, no padding (rex_gym_amd/_lib.py mirrors it)");

int rex_num_bodies(const RexConfig* c) {
  if (!c) return REX_EINVAL;
  return c->mark == REX_MARK_ARM ? REX_NB + REXA_NJ : REX_NB;
}

// the tail the readout entry points share: the sim's device, one launch over the rows (a macro, so that HIPCHK's message names the launcher)
#define READOUT_LAUNCH(launcher, args)                            \
  do {                                                            \
    HIPCHK(hipSetDevice(s->device));                              \
    HIPCHK(launcher(s, d_env_ids, n, args, (hipStream_t)stream)); \
    return REX_OK;                                                \
  } while (0)

int rex_kinematics(RexSim* s, const int32_t* d_env_ids, int n, const RexKinematicsOut* out, void* stream) {
  const char* who = "rex_kinematics";
  if (!out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = sense_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * rex_num_bodies(&s->cfg) * 4 >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * bodies * 4 must stay below 2^31", who, n);
  if (!out->link_pos && !out->link_quat && !out->link_linvel && !out->link_angvel && !out->toe_pos && !out->toe_vel && !out->toe_dist &&
      !out->toe_normal && !out->toe_in_reach && !out->base_body)
    return failf(REX_EINVAL, "%s: every output pointer is null", who);
  READOUT_LAUNCH(rex_launch_kinematics, *out);
}

static_assert(sizeof(RexDynamicsOut) == 56, "RexDynamicsOut: 7 pointers, no padding (rex_gym_amd/_lib.py mirrors it)");

int rex_dynamics(RexSim* s, const int32_t* d_env_ids, int n, const RexDynamicsOut* out, void* stream) {
  const char* who = "rex_dynamics";
  if (!out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = sense_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (s->cfg.mark == REX_MARK_ARM) return failf(REX_EINVAL, "%s: mark arm is not supported (18 degrees of freedom only)", who);
  if ((long long)n * rex::kDynJacFloats >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * 8 * 3 * 18 must stay below 2^31", who, n);
  if (!out->mass_matrix && !out->bias && !out->gravity && !out->toe_jacobian && !out->com && !out->momentum && !out->mass)
    return failf(REX_EINVAL, "%s: every output pointer is null", who);
  if (((uintptr_t)out->mass_matrix | (uintptr_t)out->toe_jacobian) & 15u)   // (the kernel writes these two in 16-byte chunks)
    return failf(REX_EINVAL, "%s: mass_matrix and toe_jacobian must be 16-byte aligned", who);
  READOUT_LAUNCH(rex_launch_dynamics, *out);
}

static_assert(sizeof(RexDynamicsLoad) == 24, "RexDynamicsLoad: 3 pointers, no padding (rex_gym_amd/_lib.py mirrors it)");

// what the three solves with M refuse alike: the null and range cases of rex_dynamics, mark arm
static int solve_rows(const char* who, RexSim* s, const int32_t* d_env_ids, int n) {
  const int rows_err = sense_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (s->cfg.mark == REX_MARK_ARM) return failf(REX_EINVAL, "%s: mark arm is not supported (18 degrees of freedom only)", who);
  if ((long long)n * rex::kDynDof >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * 18 must stay below 2^31", who, n);
  return REX_OK;
}

int rex_dynamics_solve(RexSim* s, const int32_t* d_env_ids, int n, int K, const float* d_rhs, float* d_x, void* stream) {
  const char* who = "rex_dynamics_solve";
  if (!d_rhs || !d_x) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (K < 1) return failf(REX_EINVAL, "%s: K %d: at least one right-hand side per row", who, K);
  if ((long long)n * K * rex::kDynDof >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d, K %d: n * K * 18 must stay below 2^31", who, n, K);
  const uintptr_t r0 = (uintptr_t)d_rhs, x0 = (uintptr_t)d_x, bytes = (uintptr_t)n * K * rex::kDynDof * sizeof(float);
  if (r0 != x0 && r0 < x0 + bytes && x0 < r0 + bytes)
    return failf(REX_EINVAL, "%s: d_rhs and d_x overlap in part (the same pointer solves in place; otherwise they must be disjoint)", who);
  rex::RexSolveArgs a{rex::kSolveRhs, K, d_rhs, d_x, nullptr, nullptr, nullptr, nullptr};
  READOUT_LAUNCH(rex_launch_dynamics_solve, a);
}

int rex_forward_dynamics(RexSim* s, const int32_t* d_env_ids, int n, const RexDynamicsLoad* load, float* d_vdot, void* stream) {
  const char* who = "rex_forward_dynamics";
  if (!load || !d_vdot) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  rex::RexSolveArgs a{rex::kSolveForward, 1, nullptr, d_vdot, load->joint, load->toe, load->base, nullptr};
  READOUT_LAUNCH(rex_launch_dynamics_solve, a);
}

int rex_apply_impulse(RexSim* s, const int32_t* d_env_ids, int n, const RexDynamicsLoad* impulse, float* d_dv, void* stream) {
  const char* who = "rex_apply_impulse";
  if (!impulse) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if (!impulse->joint && !impulse->toe && !impulse->base) return failf(REX_EINVAL, "%s: every impulse pointer is null", who);
  if (s->cfg.on_rack) return failf(REX_EINVAL, "%s: an on_rack sim holds its base with an anchor the solve leaves out", who);
  rex::RexSolveArgs a{rex::kSolveImpulse, 1, nullptr, d_dv, impulse->joint, impulse->toe, impulse->base, s->d_state};
  READOUT_LAUNCH(rex_launch_dynamics_solve, a);
}

static_assert(sizeof(RexContactSolveIn) == 24 && sizeof(RexContactSolveOut) == 40, "RexContactSolveIn: a pointer, four 4-byte words; RexContactSolveOut: 5 pointers (rex_gym_amd/_lib.py mirrors them)");

int rex_contact_solve(RexSim* s, const int32_t* d_env_ids, int n, const RexContactSolveIn* in, const RexContactSolveOut* out, void* stream) {
  const char* who = "rex_contact_solve";
  if (!in || !out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * 24 >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * 24 must stay below 2^31", who, n);
  if (s->cfg.on_rack) return failf(REX_EINVAL, "%s: an on_rack sim holds its base with an anchor the solve leaves out", who);
  if (s->cfg.body_contacts) return failf(REX_EINVAL, "%s: a sim with body_contacts solves link-box rows the solve leaves out", who);
  if (!out->toe_force && !out->toe_lambda && !out->limit_torque && !out->v_next && !out->sweeps)
    return failf(REX_EINVAL, "%s: every output pointer is null", who);
  rex::RexContactArgs a{in->tau, in->dt > 0.0f ? in->dt : s->cfg.sim_time_step, in->iterations > 0 ? in->iterations : s->cfg.solver_iterations,
                        in->residual_threshold < 0.0f ? s->cfg.solver_residual_threshold : in->residual_threshold, in->damping != 0, *out};
  if (a.iterations < 1 || a.iterations > rex::kContactMaxIterations)
    return failf(REX_EINVAL, "%s: iterations %d: 1 .. %d", who, a.iterations, rex::kContactMaxIterations);
  if (!(a.dt > 0.0f) || !std::isfinite(a.dt) || !(a.threshold >= 0.0f) || !std::isfinite(a.threshold))
    return failf(REX_EINVAL, "%s: dt %g, residual_threshold %g: a finite dt > 0 and a finite threshold", who, (double)in->dt, (double)in->residual_threshold);
  READOUT_LAUNCH(rex_launch_contact_solve, a);
}

static_assert(sizeof(RexRolloutIn) == 40 && sizeof(RexRolloutOut) == 32, "RexRolloutIn: two pointers, six 4-byte words; RexRolloutOut: 4 pointers (rex_gym_amd/_lib.py mirrors them)");
static_assert(sizeof(RexRolloutFrom) == 24, "RexRolloutFrom: 3 pointers, no padding (rex_gym_amd/_lib.py mirrors it)");

// what rex_rollout and rex_rollout_from refuse alike, and the launch's settings with the config's defaults resolved -> a
// (what the arguments alone decide comes first, in front of everything the sim decides: those refusals need no device)
static int rollout_args(const char* who, RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutIn* in, const RexRolloutOut* out,
                        rex::RexRolloutArgs& a) {
  if ((in->targets != nullptr) == (in->tau != nullptr)) return failf(REX_EINVAL, "%s: exactly one of targets and tau", who);
  if (!out->state && !out->trajectory && !out->foot_contact && !out->sweeps) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  const int K = in->candidates, T = in->steps;
  if (K < 1) return failf(REX_EINVAL, "%s: candidates %d: at least one candidate per env", who, K);
  if (T < 1) return failf(REX_EINVAL, "%s: steps %d: at least one control step", who, T);
  if (T > rex::kRolloutMaxSubsteps || (in->repeat > 0 && (long long)T * in->repeat > rex::kRolloutMaxSubsteps))
    return failf(REX_EINVAL, "%s: steps %d x repeat %d: at most %d substeps", who, T, in->repeat, rex::kRolloutMaxSubsteps);
  if (in->iterations > rex::kContactMaxIterations) return failf(REX_EINVAL, "%s: iterations %d: 1 .. %d", who, in->iterations, rex::kContactMaxIterations);
  if (!std::isfinite(in->dt) || !std::isfinite(in->residual_threshold))
    return failf(REX_EINVAL, "%s: dt %g, residual_threshold %g: a finite dt > 0 and a finite threshold", who, (double)in->dt, (double)in->residual_threshold);
  const int rows_err = solve_rows(who, s, d_env_ids, n);               // a null sim, n < 1, n > num_envs without ids, mark arm
  if (rows_err != REX_OK) return rows_err;
  // (K <= 2^31 - 1 and T <= 4096: the products stay inside 64 bits)
  if ((long long)n * K >= (1ll << 31) || (long long)n * K * T * rex::kRolloutWords >= (1ll << 31))
    return failf(REX_EINVAL, "%s: n %d, candidates %d, steps %d: n * candidates * steps * 37 must stay below 2^31", who, n, K, T);
  if (s->cfg.on_rack) return failf(REX_EINVAL, "%s: an on_rack sim holds its base with an anchor the rollout leaves out", who);
  if (s->cfg.body_contacts) return failf(REX_EINVAL, "%s: a sim with body_contacts solves link-box rows the rollout leaves out", who);
  if (has_latency(s->cfg))
    return failf(REX_EINVAL, "%s: a sim with the latency model on (pd_latency or control_latency > 0) draws its torques from an observation ring the rollout does not restate", who);
  const int repeat = in->repeat > 0 ? in->repeat : s->cfg.action_repeat;
  if (repeat < 1 || (long long)T * repeat > rex::kRolloutMaxSubsteps)
    return failf(REX_EINVAL, "%s: steps %d x repeat %d: at most %d substeps", who, T, repeat, rex::kRolloutMaxSubsteps);
  a = rex::RexRolloutArgs{in->targets, in->tau, K, T, repeat, in->dt > 0.0f ? in->dt : s->cfg.sim_time_step,
                          in->iterations > 0 ? in->iterations : s->cfg.solver_iterations,
                          in->residual_threshold < 0.0f ? s->cfg.solver_residual_threshold : in->residual_threshold, rex::motor_params_on(s->mot) ? 1 : 0, *out};
  if (a.iterations < 1 || a.iterations > rex::kContactMaxIterations)
    return failf(REX_EINVAL, "%s: iterations %d: 1 .. %d", who, a.iterations, rex::kContactMaxIterations);
  if (!(a.dt > 0.0f) || !std::isfinite(a.dt) || !(a.threshold >= 0.0f) || !std::isfinite(a.threshold))
    return failf(REX_EINVAL, "%s: dt %g, residual_threshold %g: a finite dt > 0 and a finite threshold", who, (double)a.dt, (double)a.threshold);
  return REX_OK;
}

int rex_rollout(RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutIn* in, const RexRolloutOut* out, void* stream) {
  const char* who = "rex_rollout";
  if (!in || !out) return failf(REX_EINVAL, "%s: null pointer", who);
  rex::RexRolloutArgs a;
  const int args_err = rollout_args(who, s, d_env_ids, n, in, out, a);
  if (args_err != REX_OK) return args_err;
  READOUT_LAUNCH(rex_launch_rollout, a);
}

// (the three inputs hold n * K * 37, n * K * T * 6 and n * K * 3 elements: each below the n * K * T * 37 that rollout_args holds under 2^31)
int rex_rollout_from(RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutIn* in, const RexRolloutFrom* from, const RexRolloutOut* out,
                     void* stream) {
  const char* who = "rex_rollout_from";
  if (!in || !from || !out) return failf(REX_EINVAL, "%s: null pointer", who);
  rex::RexRolloutArgs a;
  const int args_err = rollout_args(who, s, d_env_ids, n, in, out, a);
  if (args_err != REX_OK) return args_err;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_rollout_from(s, d_env_ids, n, a, *from, (hipStream_t)stream));
  return REX_OK;
}

static_assert(sizeof(RexRolloutActionsIn) == 40 && sizeof(RexRolloutActionsOut) == 56, "RexRolloutActionsIn: two pointers, six 4-byte words; RexRolloutActionsOut: 7 pointers (rex_gym_amd/_lib.py mirrors them)");
static_assert(offsetof(RexRolloutActionsIn, candidates) == 16 && offsetof(RexRolloutActionsIn, residual_threshold) == 36 && offsetof(RexRolloutActionsOut, ctrl) == 32 &&
              offsetof(RexRolloutActionsOut, targets) == 48, "RexRolloutActionsIn / RexRolloutActionsOut: no padding");

// what rex_command refuses of a sim beyond solve_rows (null sim, n, mark arm): the batches whose controller the readout does not restate
static int command_sim(const char* who, const RexSim* s) {
  if (s->cfg.task == REX_TASK_MIXED) return failf(REX_EINVAL, "%s: a REX_TASK_MIXED sim runs a task per env: single-task sims only", who);
  if (has_latency(s->cfg))
    return failf(REX_EINVAL, "%s: a sim with the latency model on (pd_latency or control_latency > 0) reads its orientation (the turn goal test, the reward) from an observation ring the readout does not restate", who);
  return REX_OK;
}

// one rex_command_kernel over n * K rows (arguments checked by the callers); sensor noise is not drawn, as in every readout
static hipError_t launch_command(const RexSim* s, const rex::RexCommandArgs& a, hipStream_t st) {
  rex::DevCfg c = s->dev;
  c.noise_on = 0;
  c.hist = nullptr;
  const int rows = a.n * a.K;
  hipLaunchKernelGGL(rex::rex_command_kernel, dim3((4 * (unsigned)rows + rex::kCommandThreads - 1) / rex::kCommandThreads), dim3(rex::kCommandThreads), 0, st, c, a,
                     (const float*)s->d_state);
  return hipGetLastError();
}

int rex_command(RexSim* s, const int32_t* d_env_ids, int n, int candidates, const float* d_actions, const float* d_state, const float* d_ctrl,
                float* d_targets, float* d_ctrl_next, void* stream) {
  const char* who = "rex_command";
  if (!d_actions) return failf(REX_EINVAL, "%s: null actions", who);
  if (!d_targets && !d_ctrl_next) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  if (candidates < 1) return failf(REX_EINVAL, "%s: candidates %d: at least one candidate per env", who, candidates);
  const int rows_err = solve_rows(who, s, d_env_ids, n);               // a null sim, n < 1, n > num_envs without ids, mark arm
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * candidates * rex::kRolloutWords >= (1ll << 31))
    return failf(REX_EINVAL, "%s: n %d, candidates %d: n * candidates * 37 must stay below 2^31", who, n, candidates);
  const int sim_err = command_sim(who, s);
  if (sim_err != REX_OK) return sim_err;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(launch_command(s, rex::RexCommandArgs{d_actions, d_state, d_ctrl, d_targets, d_ctrl_next, nullptr, d_env_ids, n, candidates}, (hipStream_t)stream));
  return REX_OK;
}

// per row: the state ping-pong (2 x 37 words), the controller words' ping-pong (2 x 8) and one step of targets (12)
long long rex_rollout_actions_workspace_bytes(int n, int candidates) {
  if (n < 1 || candidates < 1 || (long long)n * candidates >= (1ll << 31)) return -1;
  return (long long)n * candidates * (2 * rex::kRolloutWords + 2 * rex::kCommandCtrlWords + 12) * (long long)sizeof(float);
}

static_assert(sizeof(RexOutcomeOut) == 24 && sizeof(RexRolloutActionsOutcome) == 32, "RexOutcomeOut: 3 pointers; RexRolloutActionsOutcome: 4 pointers (rex_gym_amd/_lib.py mirrors them)");
static_assert(offsetof(RexOutcomeOut, done) == 8 && offsetof(RexOutcomeOut, obs) == 16, "RexOutcomeOut: no padding (four pointers in 32 bytes have none either)");

// rex_rollout_actions (oc null) and rex_rollout_actions_outcome: the same checks and the same 2 T launches; with oc every step's rollout
// launch is the kernel's outcome instantiation, fed the command's ctrl_next
static int rollout_actions_run(const char* who, RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from,
                               const RexRolloutActionsOut* out, const RexRolloutActionsOutcome* oc, void* d_workspace, long long workspace_bytes, void* stream) {
  if (!in->actions) return failf(REX_EINVAL, "%s: null actions", who);
  const bool none = !out->state && !out->trajectory && !out->foot_contact && !out->sweeps && !out->ctrl && !out->ctrl_trajectory && !out->targets;
  if (oc ? (!oc->reward && !oc->done && !oc->obs && !oc->motor_torque) : none) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  const long long need = rex_rollout_actions_workspace_bytes(n, in->candidates);
  if (need > 0 && (!d_workspace || workspace_bytes < need))
    return failf(REX_EINVAL, "%s: a workspace of %lld bytes, rex_rollout_actions_workspace_bytes(%d, %d) is %lld", who, d_workspace ? workspace_bytes : 0ll, n, in->candidates, need);
  // the shape and the settings are RexRolloutIn's: checked, and their defaults resolved, by what rex_rollout_from checks them with
  // (the two pointers only say "targets, and an output": every step's launch below gets its own)
  static float probe;
  float* const ws = (float*)d_workspace;
  const RexRolloutIn shape{&probe, nullptr, in->candidates, in->steps, in->repeat, in->dt, in->iterations, in->residual_threshold};
  const RexRolloutOut some{&probe, nullptr, nullptr, nullptr};
  rex::RexRolloutArgs a;
  const int args_err = rollout_args(who, s, d_env_ids, n, &shape, &some, a);
  if (args_err != REX_OK) return args_err;
  const int sim_err = command_sim(who, s);
  if (sim_err != REX_OK) return sim_err;
  const int K = a.K, T = a.T;
  const size_t rows = (size_t)n * K;
  float* const ws_state[2] = {ws, ws + rows * rex::kRolloutWords};
  float* const ws_ctrl[2] = {ws + 2 * rows * rex::kRolloutWords, ws + 2 * rows * rex::kRolloutWords + rows * rex::kCommandCtrlWords};
  float* const ws_targets = ws + 2 * rows * (rex::kRolloutWords + rex::kCommandCtrlWords);
  const int A = s->dev.action_dim;
  HIPCHK(hipSetDevice(s->device));
  const float* state_prev = from->init_state;     // null: the env's own words 0..36
  const float* ctrl_prev = in->ctrl;              // null: the env's own words REX_S_PHI .. REX_S_STEPS
  a.T = 1;
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    float* const tg = out->targets ? out->targets + (size_t)t * rows * 12 : ws_targets;
    float* const cn = out->ctrl_trajectory ? out->ctrl_trajectory + (size_t)t * rows * rex::kCommandCtrlWords : (last && out->ctrl ? out->ctrl : ws_ctrl[t & 1]);
    float* const cc = last && out->ctrl && cn != out->ctrl ? out->ctrl : nullptr;
    HIPCHK(launch_command(s, rex::RexCommandArgs{in->actions + (size_t)t * rows * A, state_prev, ctrl_prev, tg, cn, cc, d_env_ids, n, K}, (hipStream_t)stream));
    float* const traj = out->trajectory ? out->trajectory + (size_t)t * rows * rex::kRolloutWords : nullptr;
    float* const st_out = last ? (out->state ? out->state : ws_state[t & 1]) : (traj ? nullptr : ws_state[t & 1]);
    a.targets = tg;
    a.out = RexRolloutOut{st_out, traj, out->foot_contact ? out->foot_contact + (size_t)t * rows * 4 : nullptr, out->sweeps ? out->sweeps + (size_t)t * rows : nullptr};
    const RexRolloutFrom step{state_prev, from->base_wrench ? from->base_wrench + (size_t)t * rows * 6 : nullptr, from->body};
    if (oc) {
      const RexOutcomeOut oo{oc->reward ? oc->reward + (size_t)t * rows : nullptr, oc->done ? oc->done + (size_t)t * rows : nullptr,
                             oc->obs ? oc->obs + (size_t)t * rows * (size_t)s->dev.obs_dim : nullptr};
      HIPCHK(rex_launch_rollout_outcome(s, d_env_ids, n, a, step, cn, oo, oc->motor_torque ? oc->motor_torque + (size_t)t * rows * 12 : nullptr, (hipStream_t)stream));
    } else HIPCHK(rex_launch_rollout_from(s, d_env_ids, n, a, step, (hipStream_t)stream));
    state_prev = traj ? traj : st_out;
    ctrl_prev = cn;
  }
  return REX_OK;
}

int rex_rollout_actions(RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from, const RexRolloutActionsOut* out,
                        void* d_workspace, long long workspace_bytes, void* stream) {
  const char* who = "rex_rollout_actions";
  if (!in || !from || !out) return failf(REX_EINVAL, "%s: null pointer", who);
  return rollout_actions_run(who, s, d_env_ids, n, in, from, out, nullptr, d_workspace, workspace_bytes, stream);
}

// (obs_dim <= 16 < 37: the outcome arrays stay below the n * K * T * 37 that rollout_args holds under 2^31)
int rex_rollout_actions_outcome(RexSim* s, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from, const RexRolloutActionsOut* out,
                                const RexRolloutActionsOutcome* outcome, void* d_workspace, long long workspace_bytes, void* stream) {
  const char* who = "rex_rollout_actions_outcome";
  if (!in || !from || !out || !outcome) return failf(REX_EINVAL, "%s: null pointer", who);
  return rollout_actions_run(who, s, d_env_ids, n, in, from, out, outcome, d_workspace, workspace_bytes, stream);
}

int rex_outcome(RexSim* s, const int32_t* d_env_ids, int n, int candidates, const float* d_state, const float* d_ctrl, const float* d_motor_torque,
                const RexOutcomeOut* out, void* stream) {
  const char* who = "rex_outcome";
  if (!out) return failf(REX_EINVAL, "%s: null pointer", who);
  if (!out->reward && !out->done && !out->obs) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  if (candidates < 1) return failf(REX_EINVAL, "%s: candidates %d: at least one candidate per env", who, candidates);
  const int rows_err = solve_rows(who, s, d_env_ids, n);               // a null sim, n < 1, n > num_envs without ids, mark arm
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * candidates * rex::kRolloutWords >= (1ll << 31))
    return failf(REX_EINVAL, "%s: n %d, candidates %d: n * candidates * 37 must stay below 2^31", who, n, candidates);
  const int sim_err = command_sim(who, s);
  if (sim_err != REX_OK) return sim_err;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(rex_launch_outcome(s, d_env_ids, n, candidates, d_state, d_ctrl, d_motor_torque, *out, (hipStream_t)stream));
  return REX_OK;
}

static_assert(sizeof(RexContactSpaceOut) == 24, "RexContactSpaceOut: 3 pointers, no padding (rex_gym_amd/_lib.py mirrors it)");

int rex_inverse_dynamics(RexSim* s, const int32_t* d_env_ids, int n, const float* d_vdot, const RexDynamicsLoad* load, float* d_force, void* stream) {
  const char* who = "rex_inverse_dynamics";
  if (!d_force) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  rex::RexInverseArgs a{d_vdot, load ? load->joint : nullptr, load ? load->toe : nullptr, load ? load->base : nullptr, d_force};
  READOUT_LAUNCH(rex_launch_inverse_dynamics, a);
}

int rex_contact_space(RexSim* s, const int32_t* d_env_ids, int n, const float* d_tau, const float* d_base_wrench, const RexContactSpaceOut* out,
                      void* stream) {
  const char* who = "rex_contact_space";
  if (!out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * rex::kDelassusFloats >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * 24 * 24 must stay below 2^31", who, n);
  if (!out->delassus && !out->toe_drift && !out->toe_acc_free) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  if ((uintptr_t)out->delassus & 15u)                        // (the kernel writes it in 16-byte chunks)
    return failf(REX_EINVAL, "%s: delassus must be 16-byte aligned", who);
  rex::RexContactSpaceArgs a{d_tau, d_base_wrench, *out};
  READOUT_LAUNCH(rex_launch_contact_space, a);
}

static_assert(sizeof(RexForceDistributionParams) == 36 && sizeof(RexForceDistributionOut) == 32,
              "RexForceDistributionParams: nine 4-byte words; RexForceDistributionOut: 4 pointers (rex_gym_amd/_lib.py mirrors them)");

int rex_force_distribution(RexSim* s, const int32_t* d_env_ids, int n, const float* d_vdot, const float* d_base_wrench, const uint8_t* d_stance,
                           const RexForceDistributionParams* params, RexForceDistributionOut* out, void* stream) {
  const char* who = "rex_force_distribution";
  if (!params || !out) return failf(REX_EINVAL, "%s: null pointer", who);
  const int rows_err = solve_rows(who, s, d_env_ids, n);
  if (rows_err != REX_OK) return rows_err;
  if ((long long)n * 24 >= (1ll << 31)) return failf(REX_EINVAL, "%s: n %d: n * 24 must stay below 2^31", who, n);
  if (s->cfg.on_rack) return failf(REX_EINVAL, "%s: an on_rack sim holds its base with an anchor the problem leaves out", who);
  if (s->cfg.body_contacts) return failf(REX_EINVAL, "%s: a sim with body_contacts pushes with link boxes the problem leaves out", who);
  if (!out->toe_force && !out->tau && !out->base_residual && !out->residual) return failf(REX_EINVAL, "%s: every output pointer is null", who);
  for (int i = 0; i < 6; ++i)
    if (!(params->weights[i] > 0.0f) || !std::isfinite(params->weights[i]))
      return failf(REX_EINVAL, "%s: weights[%d] %g: every weight must be finite and positive", who, i, (double)params->weights[i]);
  if (!(params->eps > 0.0f) || !std::isfinite(params->eps))
    return failf(REX_EINVAL, "%s: eps %g: the regulariser must be finite and positive (the problem has 24 unknowns and at most 6 equations)", who, (double)params->eps);
  if (!(params->friction_scale >= 0.0f) || !std::isfinite(params->friction_scale))
    return failf(REX_EINVAL, "%s: friction_scale %g: finite and not negative", who, (double)params->friction_scale);
  if (params->iterations < 1 || params->iterations > rex::kForceMaxIterations)
    return failf(REX_EINVAL, "%s: iterations %d: 1 .. %d", who, params->iterations, rex::kForceMaxIterations);
  rex::RexForceArgs a{d_vdot, d_base_wrench, d_stance, {}, params->eps, params->friction_scale, params->iterations, *out};
  for (int i = 0; i < 6; ++i) a.w[i] = params->weights[i];
  READOUT_LAUNCH(rex_launch_force_distribution, a);
}

int rex_ik_solve(int n, const float* d_orn, const float* d_pos, const float* d_frames, float* d_angles, void* stream) {
  if (n <= 0 || !d_orn || !d_pos || !d_frames || !d_angles) return fail(REX_EINVAL, "rex_ik_solve: bad arguments%s", "");
  hipLaunchKernelGGL(rex::rex_ik_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_orn, d_pos, d_frames, d_angles);
  HIPCHK(hipGetLastError());
  return REX_OK;
}

int rex_motor_torque(int n, const float* d_cmd, const float* d_q, const float* d_qd, const float* d_qd_true, float kp, float kd,
                     float* d_actual, float* d_observed, void* stream) {
  if (n <= 0 || !d_cmd || !d_q || !d_qd || !d_qd_true || !d_actual || !d_observed) return fail(REX_EINVAL, "rex_motor_torque: bad arguments%s", "");
  hipLaunchKernelGGL(rex::rex_motor_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_cmd, d_q, d_qd, d_qd_true,
                     kp, kd, d_actual, d_observed);
  HIPCHK(hipGetLastError());
  return REX_OK;
}

int rex_motor_torque_params(int n, const float* d_cmd, const float* d_q, const float* d_qd, const float* d_qd_true, const float* d_par,
                            float* d_actual, float* d_observed, void* stream) {
  if (n <= 0 || !d_cmd || !d_q || !d_qd || !d_qd_true || !d_par || !d_actual || !d_observed)
    return fail(REX_EINVAL, "rex_motor_torque_params: bad arguments%s", "");
  hipLaunchKernelGGL(rex::rex_motor_params_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_cmd, d_q, d_qd, d_qd_true,
                     d_par, d_actual, d_observed);
  HIPCHK(hipGetLastError());
  return REX_OK;
}

int rex_gait_loop(int n, int mode, double* d_planner, const double* d_params, float* d_frames_out, void* stream) {
  if (n <= 0 || (mode != 0 && mode != 1) || !d_planner || !d_params || !d_frames_out) return fail(REX_EINVAL, "rex_gait_loop: bad arguments%s", "");
  hipLaunchKernelGGL(rex::rex_gait_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, mode, d_planner, d_params, d_frames_out);
  HIPCHK(hipGetLastError());
  return REX_OK;
}

#ifdef REX_PROF   /* developer build only (tools/prof_sections.py): cycle counters of the sections of a substep */
REX_API int rex_debug_prof(long long* out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_prof), sizeof(long long) * 10 * 1024) != hipSuccess) return REX_EHIP;
  if (reset) { static long long z[10 * 1024]; if (hipMemcpyToSymbol(HIP_SYMBOL(rex::g_prof), z, sizeof(z)) != hipSuccess) return REX_EHIP; }
  return REX_OK;
}
REX_API int rex_debug_legmask(unsigned* out, int n) {   /* per env: toe points in reach (last substep; OR since the last call) */
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_legmask), sizeof(unsigned) * (size_t)(n < 65536 ? n : 65536)) != hipSuccess) return REX_EHIP;
  static unsigned z[65536];
  if (hipMemcpyToSymbol(HIP_SYMBOL(rex::g_legmask), z, sizeof(z)) != hipSuccess) return REX_EHIP;
  return REX_OK;
}
REX_API int rex_debug_prof2(long long* out, int reset) {   /* the sections of the sweep routine (pgs_dv) */
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_prof2), sizeof(long long) * 16 * 1024) != hipSuccess) return REX_EHIP;
  if (reset) { static long long z[16 * 1024]; if (hipMemcpyToSymbol(HIP_SYMBOL(rex::g_prof2), z, sizeof(z)) != hipSuccess) return REX_EHIP; }
  return REX_OK;
}
REX_API int rex_debug_prof3(long long* out, int reset) {   /* per wave sweep: cycles by envs still running, out-of-line residual blocks taken */
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_prof3), sizeof(long long) * 48 * 1024) != hipSuccess) return REX_EHIP;
  if (reset) { static long long z[48 * 1024]; if (hipMemcpyToSymbol(HIP_SYMBOL(rex::g_prof3), z, sizeof(z)) != hipSuccess) return REX_EHIP; }
  return REX_OK;
}
#endif
}  // extern "C"

// ---- the launchers of every offered variant (rex_kernels.h), nullptr where a combination is not offered or its group was left out of
// a developer build (build.py REX_BUILD_ONLY: -DREX_LEFT_OUT_GROUPS=<bit mask over RexStepGroup>) ----
#ifndef REX_LEFT_OUT_GROUPS
#define REX_LEFT_OUT_GROUPS 0
#endif
typedef void (*StepLauncher)(RexSim*, int, hipStream_t, const float*, float*, float*, uint8_t*, float*);
typedef void (*SettleLauncher)(RexSim*, int, hipStream_t, float*);
template <int GROUP, int MODE, bool MOTOR> static constexpr StepLauncher step_launcher() {
  if constexpr (rex_step_variant_offered(GROUP, MODE, MOTOR) && !((REX_LEFT_OUT_GROUPS >> GROUP) & 1)) return &rex_launch_step<GROUP, MODE, MOTOR>;
  else return nullptr;
}
template <bool ARM> static constexpr SettleLauncher settle_launcher() {
  if constexpr (!((REX_LEFT_OUT_GROUPS >> (ARM ? REX_GROUP_ARM : REX_GROUP_BASE)) & 1)) return &rex_launch_settle<ARM>;
  else return nullptr;
}
#define REX_TABLE_MODE(G, M) { step_launcher<G, M, false>(), step_launcher<G, M, true>() }
#define REX_TABLE_GROUP(G) { REX_TABLE_MODE(G, REX_MODE_STEP), REX_TABLE_MODE(G, REX_MODE_TRACE), REX_TABLE_MODE(G, REX_MODE_SEG), REX_TABLE_MODE(G, REX_MODE_POL), REX_TABLE_MODE(G, REX_MODE_RNN) }
static const StepLauncher step_launchers[REX_NUM_GROUPS][REX_NUM_MODES][2] = {
    REX_TABLE_GROUP(REX_GROUP_BASE), REX_TABLE_GROUP(REX_GROUP_ARM), REX_TABLE_GROUP(REX_GROUP_MIXED_BASE), REX_TABLE_GROUP(REX_GROUP_MIXED_ARM), REX_TABLE_GROUP(REX_GROUP_BODY)};
static const SettleLauncher settle_launchers[2] = {settle_launcher<false>(), settle_launcher<true>()};
static const char* const group_names[REX_NUM_GROUPS] = {"base", "arm", "mixed_base", "mixed_arm", "body"};
static const char* const mode_names[REX_NUM_MODES] = {"step", "trace", "segment", "fused-actor", "recurrent fused-actor"};

static int launch_step(RexSim* s, int blocks, hipStream_t st, const float* a, float* o, float* r, uint8_t* d, float* m) {
  if (s->dev.trace && s->dev.nsteps > 1) {   // a segment under the event trace (debug runs): step by step through the trace kernels
    const int T = s->dev.nsteps, n = s->cfg.num_envs;
    const int ad = rex_action_dim(&s->cfg), od = rex_obs_dim(&s->cfg), nm = rex_num_motors(&s->cfg);
    int rc = REX_OK;
    s->dev.nsteps = 1;
    for (int t = 0; t < T && rc == REX_OK; ++t)
      rc = launch_step(s, blocks, st, a + (size_t)t * n * ad, o + (size_t)t * n * od, r + (size_t)t * n, d + (size_t)t * n, m ? m + (size_t)t * n * nm : nullptr);
    s->dev.nsteps = T;
    return rc;
  }
  // rex_set_motor_params / rex_set_motor_randomization: the segment-shaped instantiations that read the actuator's knobs (rex_step is a
  // segment of one step: the same arithmetic, bit for bit)
  const bool motor = rex::motor_params_on(s->mot);
  const int mode = s->dev.trace    ? REX_MODE_TRACE                                         // rex_set_event_trace (debug runs)
                   : s->use_policy ? (s->have_policy == 2 ? REX_MODE_RNN : REX_MODE_POL)    // rex_step_policy / rex_step_segment_policy
                   : (s->dev.nsteps > 1 || motor) ? REX_MODE_SEG : REX_MODE_STEP;           // rex_step_segment / rex_step
  const int group = step_group(s);
  const StepLauncher launch = step_launchers[group][mode][motor ? 1 : 0];
  if (!launch)
    return failf(REX_EINVAL, "this library has no %s kernels%s of variant group %s (not offered, or left out of a developer build: REX_BUILD_ONLY)", mode_names[mode],
                 motor ? " with motor parameters" : "", group_names[group]);
  launch(s, blocks, st, a, o, r, d, m);
  return REX_OK;
}
static int launch_settle(RexSim* s, int nrec, hipStream_t st, float* snap) {
  const bool arm = s->cfg.mark == REX_MARK_ARM;
  if (!settle_launchers[arm])
    return failf(REX_EINVAL, "this library has no settle kernels of variant group %s (left out of a developer build: REX_BUILD_ONLY)", group_names[arm ? REX_GROUP_ARM : REX_GROUP_BASE]);
  settle_launchers[arm](s, nrec, st, snap);
  return REX_OK;
}
