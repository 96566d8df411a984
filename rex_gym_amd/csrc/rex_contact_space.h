// rex_contact_space.h -- the acceleration level of the model-based readout (rex_contact_space.hip): the contact-space (Delassus) matrix
// J M^-1 J^T of the 8 toe points, their drift acceleration Jdot v and their acceleration under no ground force (rex_contact_space), and the
// equation of motion solved for the force, force = M vdot + h - S^T tau - sum_p J_p^T f_p - w (rex_inverse_dynamics) -- read-only launches
// next to rex_dynamics_solve and rex_contact_solve, on their front end (rex_dynamics_leg.h) and their factors (rex_dynamics_factor.h).
// M is never written out.  Mark base only.
//
// Like rex_dynamics' bias, both leave out what the step adds to the rigid-body equation: Bullet-style damping, joint-limit rows, contact
// rows and the on_rack anchor.  The conventions are stated once, at rex_contact_space in include/rexsim.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

constexpr int kDelassusDim = 24;                                   // 8 toe points x 3 world axes
constexpr int kDelassusFloats = kDelassusDim * kDelassusDim;       // floats of one row of delassus

// What one rex_contact_space launch does; every member is the same for every thread.
struct RexContactSpaceArgs {
  const float* tau;          // [n][12] joint torques, or null: zero
  const float* base;         // [n][6] force at the base origin and moment, world axes, or null: zero
  RexContactSpaceOut out;    // null members are skipped
};

// What one rex_inverse_dynamics launch does.
struct RexInverseArgs {
  const float* vdot;         // [n][18] generalized acceleration, or null: zero
  const float* joint;        // [n][12] joint torques already applied, or null
  const float* toe;          // [n][8][3] world forces at the toe points, or null: the ground is not queried
  const float* base;         // [n][6] force at the base origin and moment, world axes, or null
  float* force;              // [n][18]
};

}  // namespace rex

// One rex_contact_space_kernel / rex_inverse_dynamics_kernel over n rows (row k = env d_ids[k], or env k with d_ids null).  Arguments
// are checked by the caller (rexsim.hip): delassus is 16-byte aligned (float4 stores).
hipError_t rex_launch_contact_space(const RexSim* s, const int32_t* d_ids, int n, const rex::RexContactSpaceArgs& a, hipStream_t st);
hipError_t rex_launch_inverse_dynamics(const RexSim* s, const int32_t* d_ids, int n, const rex::RexInverseArgs& a, hipStream_t st);
