// rex_outcome.h -- the step's epilogue as a readout (rex_outcome, rex_rollout_actions_outcome in include/rexsim.h): what env.step() says
// after Rex.Step -- reward, done, observation -- for one row, from the row's words 0..36 after the control step, its controller words
// 37..44 after that step and the observed motor torques of the step's last substep.  outcome_row is rex_step_kernel's epilogue lambda
// (rex_kernels.h, "reward" to "termination" and env_observation) in the lane-per-(row, leg) form of the readouts: it calls the step's own
// quat_to_euler, euler_to_row2, env_observation and normalize_obs1 and restates only the scalar arithmetic between them, line for line.
// Sensor noise is not drawn, there is no reset (an auto_reset env's observation here is the terminal one), nothing is written to the sim.
// Its two callers: rex_outcome_kernel (rex_outcome.hip) and rex_rollout_kernel's third instantiation (rex_rollout.hip).
#pragma once
#include "rex_dynamics_leg.h"

namespace rex {

constexpr int kOutcomeCtrlWords = 8;          // REX_S_PHI .. REX_S_STEPS, as rex_command's ctrl_next holds them
static_assert(REX_S_STEPS - REX_S_PHI + 1 == kOutcomeCtrlWords, "the controller words are one block of the state");

namespace {

// what one lane holds of its row's outcome: reward, done and obs[0..3] on every lane of the row, ang the lane's leg's three motor angles
// of the gallop observation (0 elsewhere); obs and ang already range-normalised where the config says so
struct Outcome { float reward; bool done; float obs[4], ang[3]; };

// st, n, idx: the row's words 0..36 read as ldw(st, n, word, idx) -- the sim's state (n = num_envs, idx = env), a caller's [rows][37] row
// (st = its first word, n = 1, idx = 0) or the rollout kernel's copy in LDS.  cw: the eight controller words after the step, raw; of them
// REX_S_TARGET (already fabsf'd), REX_S_FLAGS (REX_F_ENV_GOAL; REX_F_DONE is ignored) and REX_S_STEPS (already + 1) are read.
// tau: the observed torques of the leg's three motors.  Holds a quad sum: every lane of a row's quad calls it.
// No address is formed from a state word, a controller word or a torque.
__device__ __forceinline__ void outcome_row(const DevCfg& cfg, const float* st, int n, int idx, int leg, const uint32_t (&cw)[kOutcomeCtrlWords],
                                            const float (&tau)[3], Outcome& out) {
  constexpr int NM = REX_NUM_MOTORS;
  DevCfg c = cfg;                    // the launch's config with the sensor noise off: the step's helpers draw nothing
  c.noise_on = 0;
  CtrlObs<3> co;                     // control_observation without the latency ring: the row's true words
  float pos[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pos[k] = ldw(st, n, REX_S_POS + k, idx);
    co.w[k] = ldw(st, n, REX_S_ANGVEL + k, idx);
    co.q[k] = ldw(st, n, Lay<NM>::Q + 3 * leg + k, idx);
    co.qd[k] = ldw(st, n, Lay<NM>::QD + 3 * leg + k, idx);
    co.tau[k] = tau[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) co.quat[k] = ldw(st, n, REX_S_QUAT + k, idx);
  const float target = fabsf(__uint_as_float(cw[REX_S_TARGET - REX_S_PHI]));       // rex_gym_env.py:510 (the step has taken it already)
  const uint32_t flags = cw[REX_S_FLAGS - REX_S_PHI];
  const int32_t steps = (int32_t)cw[REX_S_STEPS - REX_S_PHI];

  // ---- reward (rex_gym_env.py:501-542) ----
  float rpy[3], r20, r21, r22;
  quat_to_euler(co.quat, rpy);       // GetBaseOrientation: quat -> RPY -> quat, rex.py:530-537
  euler_to_row2(rpy, r20, r21, r22);
  float x = -pos[0];
  if (c.backwards > 0) x = -x;
  const float T = target;
  float fwd;
  if (x > T + 0.15f) fwd = T - x;
  else if (T <= x && x <= T + 0.15f) fwd = 1.0f;
  else if (x <= 0.05f) fwd = 0.0f;
  else fwd = x / T;
  fwd = fminf(fwd, c.fwd_cap);      // rex_gym_env.py:525
  const float drift = -fabsf(pos[1]);
  const float shake = -fabsf(r20 + r21);
  float dp = 0.0f;                  // GetMotorTorques . GetMotorVelocities: the lane's leg, summed over the row's quad
#pragma unroll
  for (int jl = 0; jl < 3; ++jl) dp += co.tau[jl] * co.qd[jl];
  dp = group_sum<4>(dp);
  const float energy = -fabsf(dp) * c.dt;
  float reward = c.w_dist * fwd + c.w_energy * energy + c.w_drift * drift + c.w_shake * shake;
  if (c.task == REX_TASK_TURN) reward = 0.035f - fabsf(pos[0]) - fabsf(pos[1]);   // turn_env.py:362-367
  if (c.task == REX_TASK_POSES) reward = 1.0f;                                    // poses_env.py:267-269
  if (c.task == REX_TASK_STANDUP) {                                               // standup_env.py:150-166
    float pr = fabsf(pos[0]) + fabsf(pos[1]) + fabsf(0.21f - pos[2]);
    pr = pr < 0.1f ? 1.0f - pr : -pr;
    if (pos[2] > 0.21f) pr = -1.0f - pr;
    reward = pr;
  }

  // ---- termination (rex_gym_env.py:490-499, walk_env.py:326-338, gallop_env.py:315-329) ----
  bool done;
  if (c.task == REX_TASK_GALLOP || c.task == REX_TASK_STANDUP) {
    float trpy[3];
    quat_to_euler(co.quat, trpy);
    done = fabsf(trpy[0]) > 0.3f || fabsf(trpy[1]) > 0.5f || (c.task == REX_TASK_GALLOP && pos[1] > 0.3f);
  } else done = r22 < 0.85f;
  if ((flags & REX_F_ENV_GOAL) && c.task != REX_TASK_STANDUP) done = true;        // rex_gym_env.py:495; standup overrides _termination
  if (c.task == REX_TASK_POSES) done = false;                                     // is_fallen() returns False, poses_env.py:265
  if (c.max_steps > 0 && steps >= c.max_steps) done = true;                       // (steps: the step's e.steps + 1)

  // ---- observation (walk_env.py:356-362, gallop_env.py:349-356) ----
  float obs[4], ang[3];
  env_observation<NM>(c, co, leg, obs, ang);
#pragma unroll
  for (int k = 0; k < 4; ++k) out.obs[k] = c.range_normalize ? normalize_obs1(c, k, obs[k]) : obs[k];
#pragma unroll
  for (int jl = 0; jl < 3; ++jl)
    out.ang[jl] = c.range_normalize && c.task == REX_TASK_GALLOP ? normalize_obs1(c, 4 + 3 * leg + jl, ang[jl]) : ang[jl];
  out.reward = reward;
  out.done = done;
}

// the row's outcome to out.reward[r], out.done[r], out.obs[r][obs_dim] (null members skipped, launch-uniform): the leg-0 lane the reward,
// the leg-1 lane done, the leg-2 lane obs[0..3] and every lane -- where the row carries motor angles (obs_dim = 4 + 12) -- its leg's three
__device__ __forceinline__ void outcome_store(const DevCfg& c, const RexOutcomeOut& out, size_t r, int leg, const Outcome& o) {
  if (out.reward && leg == 0) out.reward[r] = o.reward;
  if (out.done && leg == 1) out.done[r] = o.done ? 1 : 0;
  if (out.obs) {
    float* d = out.obs + r * (size_t)c.obs_dim;
    if (leg == 2) { d[0] = o.obs[0]; d[1] = o.obs[1]; d[2] = o.obs[2]; d[3] = o.obs[3]; }
    if (c.obs_dim >= 4 + REX_NUM_MOTORS) {
#pragma unroll
      for (int jl = 0; jl < 3; ++jl) d[4 + 3 * leg + jl] = o.ang[jl];
    }
  }
}

}  // namespace
}  // namespace rex
