// rex_dynamics_solve.h -- solves with the mass matrix of every env, on the device (rex_dynamics_solve.hip): x = M(q)^-1 b for
// right-hand sides the caller gives (rex_dynamics_solve), for the one the equation of motion gives for a load -- forward dynamics,
// vdot = M^-1 (S^T tau + sum_p J_p^T f_p + w - h(q, v)) (rex_forward_dynamics) -- and for an impulse, dv = M^-1 (generalized impulse),
// added to the velocity words of the caller-owned state (rex_apply_impulse: an external push between two control steps).  One launch
// next to rex_dynamics, with its front end (rex_dynamics_leg.h); M is never written out.  Mark base only.
//
// Like rex_dynamics' bias, the forward and the impulse mode leave out what the step adds to the rigid-body equation: Bullet-style
// damping, joint-limit rows, contact rows and the on_rack anchor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

enum RexSolveMode { kSolveRhs = 0, kSolveForward = 1, kSolveImpulse = 2 };

// What one launch does; every member is the same for every thread.
struct RexSolveArgs {
  int mode;                 // RexSolveMode
  int K;                    // kSolveRhs: right-hand sides per row; else 1
  const float* rhs;         // kSolveRhs: [n][K][18] (may be x itself)
  float* x;                 // [n][K][18]; forward: vdot [n][18]; impulse: dv [n][18] or null
  const float* joint;       // forward / impulse: [n][12] joint torques (impulses), or null
  const float* toe;         // [n][8][3] world forces (impulses) at the toe points, or null: the ground is not queried
  const float* base;        // [n][6] force at the base origin and moment (impulses), world axes, or null
  float* state;             // impulse: the state whose velocity words of the row's env gain dv; else null
};

}  // namespace rex

// One rex_dynamics_solve_kernel over n rows (row k = env d_ids[k], or env k with d_ids null).  Arguments are checked by the caller
// (rexsim.hip).
hipError_t rex_launch_dynamics_solve(const RexSim* s, const int32_t* d_ids, int n, const rex::RexSolveArgs& a, hipStream_t st);
