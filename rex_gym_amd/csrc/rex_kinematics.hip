// rex_kinematics.hip -- body and foot kinematics of every env (rex_kinematics.h).
//
// rex_kinematics_kernel: one lane per (output row, leg), 64 rows per workgroup of 256 threads.
//   1. Forward kinematics in LDS, with the renderer's own functions (rex_render_common.h: fk_base, fk_leg_body, fk_arm_body):
//      the leg-0 lane writes the base's entry, then every lane walks its leg's three bodies, and the leg-3 lane of a mark-arm env
//      the arm's six.  Behind each body the lane derives the link's quaternion and its velocities by the recursion of
//      rex_kinematics.h and writes the link's rows of the requested tensors; the leg-0 lane the base's and base_body.
//   2. The two toe points of the lane's leg: toe_point of rex_toe_point.h (the geometric front end of leg_pass's "toe contact
//      points" block, restated there for this kernel and rex_dynamics.hip) over the contact code's own env_ground; in reach is
//      dist < kBreaking.
// Stores: every lane writes its own short pieces (3 or 4 floats of a link, 6 of a leg's two toe points) straight to the output rows.
// Staging a workgroup's slice of each tensor in LDS and writing it out workgroup-linearly, 16 bytes per lane, was measured and was
// slower (profiles/kinematics.md: 9.3 against 8.1 us for the full readout of 4 096 envs -- two barriers per tensor cost more than the
// wider stores save at 1 KB per env), so the simpler form stays.  A null output pointer is a launch-uniform skip.
// Lanes of rows past the end repeat the last row, take part in the barrier and store nothing.
// (Built as part of rex_render.hip's object, like rex_sense.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_kinematics.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

template <bool ARM>
struct KinDims {
  static constexpr int NB = REX_NB + (ARM ? REXA_NJ : 0);
  static constexpr int NM = ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;
  // floats of one env's tables R[NB][9], o[NB][3]: an odd count, so that the lanes of one leg in neighbouring envs fall on
  // different banks
  static constexpr int kStride = (12 * NB) | 1;
  static constexpr int kLdsBytes = ((kKinEnvs * kStride + 3) & ~3) * (int)sizeof(float);
};
static_assert(KinDims<true>::kLdsBytes <= 64 * 1024, "two workgroups per CU (160 KiB), and no more than the 64 KiB a launch gets by default");

// unit quaternion x y z w of a rotation matrix (row-major): the branch with the largest pivot, then normalised
__device__ __forceinline__ void quat_of(const float* R, float* q) {
  const float tr = R[0] + R[4] + R[8];
  float x, y, z, w;
  if (tr > 0.0f) { w = 1.0f + tr; x = R[7] - R[5]; y = R[2] - R[6]; z = R[3] - R[1]; }
  else if (R[0] >= R[4] && R[0] >= R[8]) { x = 1.0f + R[0] - R[4] - R[8]; y = R[1] + R[3]; z = R[2] + R[6]; w = R[7] - R[5]; }
  else if (R[4] >= R[8]) { x = R[1] + R[3]; y = 1.0f + R[4] - R[0] - R[8]; z = R[5] + R[7]; w = R[2] - R[6]; }
  else { x = R[2] + R[6]; y = R[5] + R[7]; z = 1.0f + R[8] - R[0] - R[4]; w = R[3] - R[1]; }
  const float inv = rsqrtf(x * x + y * y + z * z + w * w);
  q[0] = x * inv; q[1] = y * inv; q[2] = z * inv; q[3] = w * inv;
}

__device__ __forceinline__ void put3(float* dst, f3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

// the rows of link b of output row `row`: its origin o and rotation Rb from the tables, its velocities v and w
template <int NB>
__device__ __forceinline__ void store_link(const RexKinematicsOut& out, bool live, int row, int b, f3 o, const float* Rb, f3 v, f3 w) {
  if (!live) return;
  const size_t at = (size_t)row * NB + b;
  if (out.link_pos) put3(out.link_pos + 3 * at, o);             // (every `if (out.x)` is the same in every thread)
  if (out.link_quat) {
    float q[4];
    quat_of(Rb, q);
    float* dst = out.link_quat + 4 * at;
    dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2]; dst[3] = q[3];
  }
  if (out.link_linvel) put3(out.link_linvel + 3 * at, v);
  if (out.link_angvel) put3(out.link_angvel + 3 * at, w);
}

template <bool ARM>
__global__ void __launch_bounds__(kKinThreads) rex_kinematics_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                     int rows_total, RexKinematicsOut out) {
  using D = KinDims<ARM>;
  constexpr int NB = D::NB, NM = D::NM;
  extern __shared__ __attribute__((aligned(16))) float s_kin[];
  const int n = c.n;
  const int el = threadIdx.x >> 2, leg = threadIdx.x & 3;
  const bool live = blockIdx.x * kKinEnvs + el < rows_total;
  const int row = min(blockIdx.x * kKinEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kKinEnvs) workgroups)
  const int env = ids ? ids[row] : row;                              // the state's env index (checked on the host)
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_kin + el * D::kStride);
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_kin + el * D::kStride + 9 * NB);

  // ---- 1. the chains ----
  if (leg == 0) fk_base(state, n, env, R[0], o[0]);
  __syncthreads();
  const f3 o0 = mk(o[0][0], o[0][1], o[0][2]);
  const f3 v0 = mk(ldw(state, n, REX_S_LINVEL, env), ldw(state, n, REX_S_LINVEL + 1, env), ldw(state, n, REX_S_LINVEL + 2, env));
  const f3 w0 = mk(ldw(state, n, REX_S_ANGVEL, env), ldw(state, n, REX_S_ANGVEL + 1, env), ldw(state, n, REX_S_ANGVEL + 2, env));
  if (leg == 0) {
    const float* R0 = R[0];
    store_link<NB>(out, live, row, 0, o0, R0, v0, w0);
    if (out.base_body && live) {
      float* dst = out.base_body + (size_t)row * 9;
#pragma unroll
      for (int k = 0; k < 3; ++k) {   // R0^T v, R0^T w, R0^T (0, 0, -1)
        dst[k] = R0[k] * v0.x + R0[3 + k] * v0.y + R0[6 + k] * v0.z;
        dst[3 + k] = R0[k] * w0.x + R0[3 + k] * w0.y + R0[6 + k] * w0.z;
        dst[6 + k] = -R0[6 + k];
      }
    }
  }
  // one step down a chain: body b's entry of the tables is written; (op, vp, wp) are its parent's origin and velocities and become
  // its own.  axis: the joint's axis in world (a column of the body's rotation, signed), qd its rate
  auto link = [&](int b, f3 axis, float qd, f3& op, f3& vp, f3& wp) {
    const f3 ob = mk(o[b][0], o[b][1], o[b][2]);
    const f3 v = vp + cross(wp, ob - op);
    const f3 w = wp + qd * axis;
    store_link<NB>(out, live, row, b, ob, R[b], v, w);
    op = ob; vp = v; wp = w;
  };
  f3 op = o0, vp = v0, wp = w0;   // the lane's leg: bodies 1 + 3 leg .. 3 + 3 leg
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int b = 1 + 3 * leg + i, ax = REX_JOINT_AXIS[b - 1];
    fk_leg_body(state, n, env, b, R, o);
    link(b, mk(R[b][ax], R[b][3 + ax], R[b][6 + ax]), ldw(state, n, Lay<NM>::QD + b - 1, env), op, vp, wp);
  }
  if constexpr (ARM) {
    if (leg == 3) {               // the arm: bodies 13 .. 18, one serial chain off the base (REXA_PARENT)
      f3 oa = o0, va = v0, wa = w0;
#pragma unroll
      for (int k = 0; k < REXA_NJ; ++k) {
        const int b = REX_NB + k;
        const float sgn = (float)REXA_AXIS_SIGN[k];
        fk_arm_body(state, n, env, k, R, o);
        link(b, mk(sgn * R[b][2], sgn * R[b][5], sgn * R[b][8]), ldw(state, n, Lay<NM>::QD + 12 + k, env), oa, va, wa);
      }
    }
  }

  // ---- 2. the toe points of this leg (rex_device.h, leg_pass: "toe contact points"; op, vp, wp are the foot link's now) ----
  if (out.toe_pos || out.toe_vel || out.toe_dist || out.toe_normal || out.toe_in_reach) {   // (the same in every thread)
    const int b3 = 3 + 3 * leg;
    const f3 z3 = mk(R[b3][2], R[b3][5], R[b3][8]), aw = mk(R[b3][1], R[b3][4], R[b3][7]);   // the foot link's z, the toe cylinder's axis
    const f3 tc = toe_centre(op, z3);
    const bool field = c.n_terrain > 0;
    Ground g{};
    if (field) g = env_ground(c, env, c.env_index_base + env, (int)ldi(state, n, Lay<NM>::EPISODE, env));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const ToePoint tp = toe_point(g, field, tc, aw, e);
      const f3 P = tp.P, nrm = tp.nrm;
      const float dist = tp.dist;
      if (live) {
        const size_t at = (size_t)row * 8 + 2 * leg + e;   // point p = 2 leg + e
        if (out.toe_pos) put3(out.toe_pos + 3 * at, P);
        if (out.toe_vel) put3(out.toe_vel + 3 * at, vp + cross(wp, P - op));
        if (out.toe_dist) out.toe_dist[at] = dist;
        if (out.toe_normal) put3(out.toe_normal + 3 * at, nrm);
        if (out.toe_in_reach) out.toe_in_reach[at] = dist < kBreaking ? 1 : 0;
      }
    }
  }
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_kinematics(const RexSim* s, const int32_t* d_ids, int n, const RexKinematicsOut& out, hipStream_t st) {
  const int blocks = (n + rex::kKinEnvs - 1) / rex::kKinEnvs;
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_kinematics_kernel<true>, dim3(blocks), dim3(rex::kKinThreads), rex::KinDims<true>::kLdsBytes, st, s->dev, s->d_state,
                       d_ids, n, out);
  else
    hipLaunchKernelGGL(rex::rex_kinematics_kernel<false>, dim3(blocks), dim3(rex::kKinThreads), rex::KinDims<false>::kLdsBytes, st, s->dev, s->d_state,
                       d_ids, n, out);
  return hipGetLastError();
}
