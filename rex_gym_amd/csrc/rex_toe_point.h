// rex_toe_point.h -- the toe contact candidate of the physics, for the read-only kernels (rex_kinematics.hip, rex_dynamics.hip):
// the geometric front end of leg_pass's "toe contact points" block (rex_device.h), restated from the same constants (kToeRad,
// kToeHalf, REX_TOE_Z) and the contact code's own ground_query -- restated and not shared with leg_pass, so that no step kernel
// compiles differently; shared between the readouts, so that they report one point.  The plane is the heightfield form with
// normal +z and height 0, which is the value the flat branch of leg_pass computes.
#pragma once
#include "rex_kernels.h"

namespace rex {

struct ToePoint { f3 P, nrm; float dist; };

// centre of the toe cylinder of a foot link with origin o and z axis z3 (world)
__device__ __forceinline__ f3 toe_centre(f3 o, f3 z3) { return o + (float)REX_TOE_Z * z3; }

// end e (0, 1) of the toe cylinder with centre tc and unit axis aw (the foot link's y axis, world): the point P that leg_pass hands
// to emit_rows, the ground's normal there and the signed distance (z - ground height) * normal z.  field: the env stands on a
// heightfield (g from env_ground); else g is not read
__device__ __forceinline__ ToePoint toe_point(const Ground& g, bool field, f3 tc, f3 aw, int e) {
  const float sg = e == 0 ? -kToeHalf : kToeHalf;
  const f3 ce = tc + sg * aw;
  f3 n0 = mk(0.f, 0.f, 1.f), nrm = mk(0.f, 0.f, 1.f);
  float h0 = 0.0f, h = 0.0f;
  if (field) ground_query(g, ce.x, ce.y, h0, n0);     // normal under the end centre ...
  const float na = dot(n0, aw);
  const f3 dv = n0 - na * aw;
  const float dn2 = dot(dv, dv);
  const float inv = dn2 > 1e-18f ? rsqrtf(dn2) : 0.0f;
  const f3 P = ce - (kToeRad * inv) * dv;              // ... -> the lowest point along it ...
  if (field) ground_query(g, P.x, P.y, h, nrm);        // ... -> the local plane
  return ToePoint{P, nrm, (P.z - h) * nrm.z};
}

}  // namespace rex
