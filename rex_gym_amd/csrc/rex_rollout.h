// rex_rollout.h -- candidate rollouts (rex_rollout.hip): for every row's env K candidate command sequences over T control steps of
// `repeat` substeps each, from the env's current state, in one read-only launch on the lane mapping, the front end (rex_dynamics_leg.h)
// and the contact rows (rex_contact_rows.h) of rex_contact_solve.  The step, settle and reset kernels are not involved and the sim's
// state is never written.  Mark base only; toe rows and joint-limit rows only (no link-box rows, no on_rack anchor, no latency ring).
//
// The substep and what is not advanced are stated once, at rex_rollout in include/rexsim.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

constexpr int kRolloutMaxSubsteps = 4096;     // steps x repeat: the substep loop is bounded on the host
constexpr int kRolloutWords = 37;             // words 0..36 of the state: position, quaternion, velocities, joint angles and rates

// What one launch does; every member is the same for every thread.  The host has resolved the defaults of RexRolloutIn.
struct RexRolloutArgs {
  const float* targets;      // [n][K][T][12] motor angle commands, or null
  const float* tau;          // [n][K][T][12] joint torques, or null -- exactly one of the two
  int K, T, repeat;          // >= 1; T * repeat <= kRolloutMaxSubsteps
  float dt;                  // > 0
  int iterations;            // 1 .. kContactMaxIterations
  float threshold;           // >= 0; 0: every substep runs `iterations` sweeps
  int motor;                 // 1: the env's actuator parameters are in effect (a table or ranges are set)
  RexRolloutOut out;         // null members are skipped
};

}  // namespace rex

// One rex_rollout_kernel over n * K rows (row r = env d_ids[r / K], or env r / K with d_ids null; candidate r % K).  Arguments are
// checked by the caller (rexsim.hip).
hipError_t rex_launch_rollout(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, hipStream_t st);

// The same over rows that take the state they start from, a base wrench per control step and their body parameters from the caller
// (rex_rollout_from in include/rexsim.h): the kernel's other instantiation, row r reads from.init_state + r * 37, from.base_wrench +
// (r * T + t) * 6 and from.body + r * 3; a null member leaves the env's own in place (no wrench).
hipError_t rex_launch_rollout_from(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, const RexRolloutFrom& from,
                                   hipStream_t st);

// The same once more with the step's epilogue behind every control step (rex_rollout_actions_outcome in include/rexsim.h): the kernel's
// third instantiation.  ctrl [rows][8]: the controller words after this control step (rex_command's ctrl_next) -- per row, so the launch
// is one control step (a.T = 1, as rex_rollout_actions launches it); outcome.reward / done [rows][T], outcome.obs [rows][T][obs_dim] and
// motor_torque [rows][T][12], the observed torques of each control step's last substep: null members are skipped.
hipError_t rex_launch_rollout_outcome(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, const RexRolloutFrom& from,
                                      const float* ctrl, const RexOutcomeOut& outcome, float* motor_torque, hipStream_t st);

// One rex_outcome_kernel over n * K rows (rex_outcome.hip; arguments checked by the caller): null state / ctrl: the env's, null
// motor_torque: zeros.
hipError_t rex_launch_outcome(const RexSim* s, const int32_t* d_ids, int n, int K, const float* state, const float* ctrl, const float* motor_torque,
                              const RexOutcomeOut& out, hipStream_t st);
