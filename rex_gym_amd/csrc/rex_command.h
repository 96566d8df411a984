// rex_command.h -- the env's controller as a readout (rex_command, rex_rollout_actions in include/rexsim.h): one control step of
// rex_step_kernel's command section -- ClipAction + RangeNormalize, the task's *_command, env_gait_ik -- for row (k, c) = (env ids[k],
// candidate c), on the row's own copy of the controller words.  Nothing is restated: the kernel calls the step's command functions
// (rex_kernels.h) in the lane-group form the 4-, 8- and 16-env step kernels call them in, a lane per (row, leg).  The sim's state is
// never written.  Included by rexsim.hip alone (no object of its own).
#pragma once
#include "rex_kernels.h"

namespace rex {

constexpr int kCommandCtrlWords = 8;          // REX_S_PHI .. REX_S_STEPS: phi, last step, alpha, target, end step, aux, flags, steps
constexpr int kCommandThreads = 128;          // 32 rows of 4 legs per workgroup
static_assert(REX_S_STEPS - REX_S_PHI + 1 == kCommandCtrlWords && REX_S_EPISODE == REX_S_STEPS + 1, "the controller words are one block of the state");

// What one launch does; every member is the same for every thread.
struct RexCommandArgs {
  const float* actions;      // [n][K][A] with A = DevCfg::action_dim
  const float* state;        // [n][K][37] words 0..36 of the row (position and quaternion are read), or null: the env's
  const float* ctrl;         // [n][K][8] the row's controller words as raw 32-bit words, or null: the env's words REX_S_PHI .. REX_S_STEPS
  float* targets;            // [n][K][12] or null
  float* ctrl_next;          // [n][K][8] or null
  float* ctrl_copy;          // [n][K][8] or null: the same words once more (rex_rollout_actions: its `ctrl` next to the last `ctrl_trajectory` slice)
  const int32_t* ids;        // [n] or null: env k
  int n, K;
};

// Row r = t / 4 of the grid's thread t, leg t % 4 (motor order FL, FR, RL, RR).  env_gait_ik<1> ballots over the wave: the lanes of the
// rows past n * K shadow the last row and are masked at the stores -- no lane leaves in front of the ballot.
// Addresses: the row index and the env id alone.  No address is formed from an action, a state or a controller word: the command
// functions index their tables by leg and by launch constants, (int)aux and the flag bits only pick between constants.
__global__ __launch_bounds__(kCommandThreads) void rex_command_kernel(DevCfg c, RexCommandArgs a, const float* __restrict__ env_state) {
  const int rows = a.n * a.K;
  const int t = (int)blockIdx.x * kCommandThreads + (int)threadIdx.x;
  const int leg0 = t & 3;
  const bool inrows = (t >> 2) < rows;
  const int r = inrows ? (t >> 2) : rows - 1;
  const int k = r / a.K;
  const int i = a.ids ? a.ids[k] : k;

  EnvState e{};     // (what the controller does not read -- velocities, joints, counters -- stays 0)
  if (a.state) {
    const float* w = a.state + (size_t)r * 37;
#pragma unroll
    for (int j = 0; j < 3; ++j) e.ph.pos[j] = w[REX_S_POS + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) e.ph.quat[j] = w[REX_S_QUAT + j];
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) e.ph.pos[j] = ldw(env_state, c.n, REX_S_POS + j, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) e.ph.quat[j] = ldw(env_state, c.n, REX_S_QUAT + j, i);
  }
  uint32_t cw[kCommandCtrlWords];
#pragma unroll
  for (int j = 0; j < kCommandCtrlWords; ++j) cw[j] = a.ctrl ? __float_as_uint(a.ctrl[(size_t)r * kCommandCtrlWords + j]) : ldi(env_state, c.n, REX_S_PHI + j, i);
  e.phi = __uint_as_float(cw[REX_S_PHI - REX_S_PHI]); e.last_step = (int32_t)cw[REX_S_LASTT - REX_S_PHI]; e.alpha = __uint_as_float(cw[REX_S_ALPHA - REX_S_PHI]);
  e.target = __uint_as_float(cw[REX_S_TARGET - REX_S_PHI]); e.end_step = (int32_t)cw[REX_S_ENDTIME - REX_S_PHI]; e.aux = __uint_as_float(cw[REX_S_AUX - REX_S_PHI]);
  e.flags = cw[REX_S_FLAGS - REX_S_PHI]; e.steps = (int32_t)cw[REX_S_STEPS - REX_S_PHI];
  e.episode = (int32_t)ldi(env_state, c.n, REX_S_EPISODE, i);

  // the step's own lines between "load" and REX_STAMP(t_command) (rex_step_kernel), NL = 1, mark base, no latency ring
  float act[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = j < c.action_dim ? a.actions[(size_t)r * c.action_dim + j] : 0.0f;
    if (c.range_normalize) {                       // ClipAction + RangeNormalize (wrappers.py:229-234,261-265)
      v = fminf(fmaxf(v, -1.0f), 1.0f);
      v = (v + 1.0f) / 2.0f * (c.act_hi - c.act_lo) + c.act_lo;
    }
    act[j] = v;
  }
  float cmd[3] = {0.0f, 0.0f, 0.0f};
  LegCall call{0, 0, 0.0f, 0.0f, 0.0f, 1.0f, 1.0, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  if (c.task == REX_TASK_GALLOP) gallop_command<1>(c, e, act, leg0, cmd, call);
  else if (c.task == REX_TASK_TURN) {
    const float cq[4] = {e.ph.quat[0], e.ph.quat[1], e.ph.quat[2], e.ph.quat[3]};
    turn_command<1>(c, e, cq, act, leg0, cmd, c.env_index_base + i, call);
  }
  else if (c.task == REX_TASK_POSES) poses_command(c, e, act, call);
  else if (c.task == REX_TASK_STANDUP) standup_command<1>(c, e, act, cmd);
  else walk_command<1>(c, e, act, leg0, cmd, call);
  env_gait_ik<1>(c, e, leg0, call, cmd);
  // what the step's epilogue does to the eight words of an env whose step returns done = 0
  e.target = fabsf(e.target);       // rex_gym_env.py:510
  e.steps += 1;

  if (!inrows) return;
  if (a.targets) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.targets[(size_t)r * 12 + 3 * leg0 + j] = cmd[j];
  }
  // two of the eight words per leg's lane (every lane of the row holds the same eight)
  const uint32_t out[kCommandCtrlWords] = {__float_as_uint(e.phi), (uint32_t)e.last_step, __float_as_uint(e.alpha), __float_as_uint(e.target),
                                           (uint32_t)e.end_step, __float_as_uint(e.aux), e.flags, (uint32_t)e.steps};
#pragma unroll
  for (int j = 0; j < kCommandCtrlWords; ++j) {
    if ((j >> 1) == leg0) {
      if (a.ctrl_next) a.ctrl_next[(size_t)r * kCommandCtrlWords + j] = __uint_as_float(out[j]);
      if (a.ctrl_copy) a.ctrl_copy[(size_t)r * kCommandCtrlWords + j] = __uint_as_float(out[j]);
    }
  }
}

}  // namespace rex
