// rex_kinematics.h -- body and foot kinematics of every env, read from the state between control steps (rex_kinematics.hip):
// the pose and velocity of every link, the 8 toe contact candidates of the physics with their ground distance and normal, and
// the base's velocity and the gravity direction in the base frame.  A separate, read-only launch next to the renderers and the
// sensors: it reads the caller-owned state, the terrain pool and the heightfield, and writes the caller's output arrays only.
//
// Conventions (the ones of physics_substep, rex_device.h):
//   - REX_S_LINVEL is the world velocity of the ORIGIN of the base link frame, the point REX_S_POS holds and is integrated
//     with (pos += dt * lin); the base's centre of mass lies in that origin (REX_COM[0] = 0), so it is the velocity of both.
//     REX_S_ANGVEL is the world angular velocity of the base.
//   - link_linvel[b] is the world velocity of the origin of link b's frame (the joint that carries it), link_angvel[b] its
//     world angular velocity:  w_b = w_p + qd_j a_j,  v_b = v_p + w_p x (o_b - o_p),  p the parent, a_j the joint's world axis.
//   - toe point p = 2 leg + e is the point P that leg_pass ("toe contact points") hands to emit_rows, in world coordinates;
//     toe_dist and toe_normal are that call's `dist` and `nrm`, toe_in_reach is dist < kBreaking, toe_vel the world velocity of
//     the foot link's material point at P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rexsim.h"

struct RexSim;

namespace rex {

// One workgroup serves kKinEnvs consecutive output rows with one lane per (row, leg): 16 rows per wave.
constexpr int kKinEnvs = 64;
constexpr int kKinThreads = 4 * kKinEnvs;

}  // namespace rex

// One rex_kinematics_kernel over n output rows (row k = env d_ids[k], or env k with d_ids null); null members of `out` are
// skipped.  Arguments are checked by the caller (rex_kinematics in rexsim.hip).
hipError_t rex_launch_kinematics(const RexSim* s, const int32_t* d_ids, int n, const RexKinematicsOut& out, hipStream_t st);
