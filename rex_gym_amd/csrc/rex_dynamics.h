// rex_dynamics.h -- the equations of motion of every env, read from the state between control steps (rex_dynamics.hip): the
// joint-space mass matrix M(q), the bias forces h(q, v) and their gravity part h(q, 0), the Jacobians of the 8 toe contact
// candidates, the centre of mass and the momentum.  A separate, read-only launch next to rex_kinematics: it reads the
// caller-owned state, the terrain pool and the heightfield (for the toe points) and the env's mass scales, and writes the caller's
// output arrays only.  Mark base only.
//
// The conventions -- the order of v, the sign of h, what the mass scales touch, damping left out -- are stated once, at
// rex_dynamics in include/rexsim.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

// One workgroup serves kDynEnvs consecutive output rows with one lane per (row, leg): 16 rows per wave, a row's legs one DPP quad.
// 32 rows: their slice of toe_jacobian (54 KiB) is staged in LDS on its way out.
constexpr int kDynEnvs = 32;
constexpr int kDynThreads = 4 * kDynEnvs;
constexpr int kDynDof = 18;
constexpr int kDynMassFloats = kDynDof * kDynDof;       // floats of one row of mass_matrix
constexpr int kDynJacFloats = 8 * 3 * kDynDof;          // floats of one row of toe_jacobian

}  // namespace rex

// One rex_dynamics_kernel over n output rows (row k = env d_ids[k], or env k with d_ids null); null members of `out` are skipped.
// Arguments are checked by the caller (rex_dynamics in rexsim.hip): mass_matrix and toe_jacobian are 16-byte aligned (float4 stores).
hipError_t rex_launch_dynamics(const RexSim* s, const int32_t* d_ids, int n, const RexDynamicsOut& out, hipStream_t st);
