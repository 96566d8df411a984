// rex_force_distribution.h -- force distribution per env (rex_force_distribution.hip): the ground forces inside the friction cones of the
// stance toe points that best produce a wanted generalized acceleration, and the joint torques that go with them -- the cone-constrained
// regularised least-squares problem stated at rex_force_distribution in include/rexsim.h, solved by a fixed number of accelerated
// projected-gradient steps in one read-only launch on the front end of the other readouts (rex_dynamics_leg.h).  Mark base only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

constexpr int kForceMaxIterations = 10000;

// What one rex_force_distribution launch does; every member is the same for every thread.
struct RexForceArgs {
  const float* vdot;           // [n][18] wanted generalized acceleration, or null: zero
  const float* base;           // [n][6] force at the base origin and moment, world axes, or null: zero
  const uint8_t* stance;       // [n][4] per leg, nonzero = in the stance set, or null: the points in reach
  float w[6];                  // W
  float eps, friction_scale;
  int iterations;              // checked on the host: 1 .. kForceMaxIterations
  RexForceDistributionOut out; // null members are skipped
};

}  // namespace rex

// One rex_force_distribution_kernel over n rows (row k = env d_ids[k], or env k with d_ids null).  Arguments are checked by the caller
// (rexsim.hip).
hipError_t rex_launch_force_distribution(const RexSim* s, const int32_t* d_ids, int n, const rex::RexForceArgs& a, hipStream_t st);
