// rex_contact_solve.h -- the step's contact problem restated for the env's current state, solved and read out
// (rex_contact_solve.hip): ground reaction forces at the toe points, joint-limit torques, the contact-consistent next velocity and the
// sweep count of one substep of the physics -- toe rows plus joint-limit rows, the step's projected Gauss-Seidel -- in a read-only
// launch next to rex_dynamics_solve, on its front end (rex_dynamics_leg.h) and its factors (rex_dynamics_factor.h).  The step, settle
// and reset kernels are not involved.  Mark base only; no link-box rows (body_contacts) and no on_rack anchor.
//
// The problem and its conventions are stated once, at rex_contact_solve in include/rexsim.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

constexpr int kContactMaxIterations = 1000;       // the sweep loop is bounded on the host

// What one launch does; every member is the same for every thread.  The host has resolved the defaults of RexContactSolveIn.
struct RexContactArgs {
  const float* tau;          // [n][12] joint torques, or null: zero
  float dt;                  // > 0
  int iterations;            // 1 .. kContactMaxIterations
  float threshold;           // >= 0; 0: every env runs `iterations` sweeps
  int damping;               // 1: the sim's per-link damping forces enter the free velocity
  RexContactSolveOut out;    // null members are skipped
};

}  // namespace rex

// One rex_contact_solve_kernel over n rows (row k = env d_ids[k], or env k with d_ids null).  Arguments are checked by the caller
// (rexsim.hip).
hipError_t rex_launch_contact_solve(const RexSim* s, const int32_t* d_ids, int n, const rex::RexContactArgs& a, hipStream_t st);
