// rex_rollout_leg.h -- what rex_rollout_kernel adds to the readouts' front end (rex_dynamics_leg.h): the chain of a leg walked from a
// copy of the state's words that is not the sim's (dyn_load_leg, the overload), and the integrator at the end of physics_substep
// (rex_device.h, "semi-implicit Euler with the NEW velocities") as a function of its own, every expression spelled as it stands there.
// rex_device.h, rex_kernels.h and rex_dynamics_leg.h are not edited: no other kernel compiles differently.
#pragma once
#include "rex_dynamics_leg.h"

namespace rex {

namespace {

// dyn_load_leg (rex_dynamics_leg.h) with the words 0..36 read from `st` by ldw(st, n, word, idx) -- the workgroup's private copy in LDS,
// [words][n] with n = kDynEnvs and idx the row in the workgroup -- and the env's ground handed in (env_ground, formed once per row).
// R, o: the row's tables in LDS.  Holds one workgroup barrier, after fk_base's reads (every thread of the workgroup calls it).
__device__ __forceinline__ void dyn_load_leg(const float* st, int n, int idx, const Ground& ground, int leg, float (*R)[9], float (*o)[3], DynFront& F) {
  constexpr int NM = REX_NUM_MOTORS;
  if (leg == 0) fk_base(st, n, idx, R[0], o[0]);
  __syncthreads();
  const f3 o0 = mk(o[0][0], o[0][1], o[0][2]);
  F.o0 = o0;
  F.v0 = mk(ldw(st, n, REX_S_LINVEL, idx), ldw(st, n, REX_S_LINVEL + 1, idx), ldw(st, n, REX_S_LINVEL + 2, idx));
  F.w0 = mk(ldw(st, n, REX_S_ANGVEL, idx), ldw(st, n, REX_S_ANGVEL + 1, idx), ldw(st, n, REX_S_ANGVEL + 2, idx));
  F.g = ground;
  const Ground& g = F.g;
  DynLeg& L = F.L;
  F.ofoot = o0; F.z3 = mk(0.f, 0.f, 1.f); F.aw = mk(0.f, 1.f, 0.f);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int b = 1 + 3 * leg + i, ax = REX_JOINT_AXIS[i];
    fk_leg_body(st, n, idx, b, R, o);
    const float* Rb = R[b];
    const f3 ex = mk(Rb[0], Rb[3], Rb[6]), ey = mk(Rb[1], Rb[4], Rb[7]), ez = mk(Rb[2], Rb[5], Rb[8]);
    const f3 ob = mk(o[b][0], o[b][1], o[b][2]);
    L.p[i] = ob - o0;
    L.a[i] = ax == 0 ? ex : ax == 1 ? ey : ez;
    L.r[i] = L.p[i] + ((float)REX_COM[1 + i][0] * ex + (float)REX_COM[1 + i][1] * ey + (float)REX_COM[1 + i][2] * ez);
    L.I[i] = rot_inertia(ex, ey, ez, (float)REX_INERTIA[1 + i][0], (float)REX_INERTIA[1 + i][1], (float)REX_INERTIA[1 + i][2]);
    L.m[i] = (float)REX_MASS[1 + i] * g.leg_mass_scale;
    L.qd[i] = ldw(st, n, Lay<NM>::QD + b - 1, idx);
    if (i == 2) { F.ofoot = ob; F.z3 = ez; F.aw = ey; }
  }
  const float* R0 = R[0];
  const f3 bx = mk(R0[0], R0[3], R0[6]), by = mk(R0[1], R0[4], R0[7]), bz = mk(R0[2], R0[5], R0[8]);
  F.I0 = rot_inertia(bx, by, bz, (float)REX_INERTIA[0][0], (float)REX_INERTIA[0][1], (float)REX_INERTIA[0][2]);
  F.m0 = (float)REX_MASS[0] * g.base_mass_scale;
  F.base = leg == 0 ? 1.0f : 0.0f;
}

// physics_substep's integrator for the base and one leg: pos, quat and the leg's q move along the NEW velocities lin, ang, qd
__device__ __forceinline__ void rollout_integrate(float dt, const float (&lin)[3], const float (&ang)[3], const float (&qd)[3], float (&pos)[3],
                                                  float (&quat)[4], float (&q)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] += dt * lin[k];
#pragma unroll
  for (int j = 0; j < 3; ++j) q[j] += dt * qd[j];
  {
    const float wn = sqrtf(ang[0] * ang[0] + ang[1] * ang[1] + ang[2] * ang[2]);
    const float angle = wn * dt;
    float sc;
    if (wn < 0.001f) sc = 0.5f * dt - dt * dt * dt * 0.020833333333f * wn * wn;
    else { float sh, ch; sincos_fast(0.5f * angle, sh, ch); sc = sh / wn; }
    const float dx = ang[0] * sc, dy = ang[1] * sc, dz = ang[2] * sc, dw = cos_half(0.5f * angle);
    const float qx = quat[0], qy = quat[1], qz = quat[2], qw = quat[3];
    const float nx = dw * qx + dx * qw + dy * qz - dz * qy;
    const float ny = dw * qy - dx * qz + dy * qw + dz * qx;
    const float nz = dw * qz + dx * qy - dy * qx + dz * qw;
    const float nw = dw * qw - dx * qx - dy * qy - dz * qz;
    const float nn = rsqrtf(nx * nx + ny * ny + nz * nz + nw * nw);
    quat[0] = nx * nn; quat[1] = ny * nn; quat[2] = nz * nn; quat[3] = nw * nn;
  }
}

}  // namespace
}  // namespace rex
