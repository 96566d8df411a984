// rex_dynamics_leg.h -- the front end that the kernels of the equations of motion share (rex_dynamics.hip, rex_dynamics_solve.hip, rex_contact_solve.hip, rex_contact_space.hip):
// one lane per (output row, leg) walks its leg's chain in LDS with the renderer's functions, holds the leg in registers (DynLeg),
// forms the composite rigid bodies about the base origin o_0 and from them the leg's columns of the mass matrix -- the coupling
// B_f (6 x 3, column i = (f_i, n_i)) and the leg block H_f (3 x 3) -- and, by DPP quad sums, the base block; leg_bias is the
// Newton-Euler bias wrench.  Sections 1 and 2 of rex_dynamics_kernel, lifted with every expression spelled as it stood there
// (the build fixes arithmetic by source, -ffp-contract=on: rex_dynamics' outputs are bit-identical to those before the lift,
// profiles/dynamics_solve.md).  The formulation is described at the top of rex_dynamics.hip.
// The lane mapping (DynLane), the bias projection h(q, v) (dyn_bias) and the launch (dyn_launch) are here once too, as far as the
// kernels that use them still compile to the code they had (profiles/readout_refactor.md).
#pragma once
#include "rex_render_common.h"
#include "rex_dynamics.h"

namespace rex {

namespace {

// floats of one env's tables R[NB][9], o[NB][3] (odd: the lanes of one leg in neighbouring envs fall on different banks)
constexpr int kDynStride = (12 * REX_NB) | 1;
// LDS of a workgroup's forward-kinematics tables
constexpr int kDynFkBytes = ((kDynEnvs * kDynStride + 3) & ~3) * (int)sizeof(float);

// the leg's model constants are read from leg 0's entries of the tables: the four legs carry the same links
constexpr bool dyn_legs_alike() {
  for (int l = 1; l < REX_NLEG; ++l)
    for (int i = 0; i < 3; ++i) {
      const int a = 1 + i, b = 1 + 3 * l + i;
      if (REX_MASS[a] != REX_MASS[b] || REX_JOINT_AXIS[a - 1] != REX_JOINT_AXIS[b - 1]) return false;
      for (int k = 0; k < 3; ++k)
        if (REX_COM[a][k] != REX_COM[b][k] || REX_INERTIA[a][k] != REX_INERTIA[b][k]) return false;
    }
  for (int b = 0; b < REX_NB; ++b)
    if (REX_INERTIA[b][3] != 0.0 || REX_INERTIA[b][4] != 0.0 || REX_INERTIA[b][5] != 0.0) return false;   // principal axes = body axes
  return REX_COM[0][0] == 0.0 && REX_COM[0][1] == 0.0 && REX_COM[0][2] == 0.0;                             // the base's centre of mass is o_0
}
static_assert(dyn_legs_alike(), "the dynamics kernels read leg 0's link constants for every leg, diagonal inertias, and a base whose centre of mass is its origin");

__device__ __forceinline__ void dput3(float* dst, f3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }
__device__ __forceinline__ f3 quad_sum(f3 v) { return mk(group_sum<4>(v.x), group_sum<4>(v.y), group_sum<4>(v.z)); }
__device__ __forceinline__ float comp(f3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }

// bias wrench of the leg's links at zero generalized acceleration: subtree sums Fs[i], Ns[i] about o_0 (i = 0: the whole leg)
struct DynLeg {
  f3 p[3], r[3], a[3];     // joint points and link centres of mass relative to o_0, joint axes (world)
  s33 I[3];                // link inertias about their centres of mass, world axes
  float m[3], qd[3];
};
__device__ __forceinline__ void leg_bias(const DynLeg& L, f3 w0, f3* Fs, f3* Ns) {
  f3 w = w0, al = mk(0.f, 0.f, 0.f), ao = mk(0.f, 0.f, 0.f), pp = mk(0.f, 0.f, 0.f);
  f3 F[3], N[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const f3 d = L.p[i] - pp;
    ao = ao + cross(al, d) + cross(w, cross(w, d));          // the joint point, carried by the parent
    al = al + L.qd[i] * cross(w, L.a[i]);                    // d/dt (qd a) at constant rate: the axis turns with the parent
    w = w + L.qd[i] * L.a[i];
    const f3 rc = L.r[i] - L.p[i];
    const f3 ac = ao + cross(al, rc) + cross(w, cross(w, rc));
    F[i] = L.m[i] * (ac + mk(0.f, 0.f, kGravity));
    N[i] = mul(L.I[i], al) + cross(w, mul(L.I[i], w)) + cross(L.r[i], F[i]);
    pp = L.p[i];
  }
  Fs[2] = F[2]; Ns[2] = N[2];
  Fs[1] = F[1] + Fs[2]; Ns[1] = N[1] + Ns[2];
  Fs[0] = F[0] + Fs[1]; Ns[0] = N[0] + Ns[1];
}

// ---- the lane: one per (output row, leg), a row's four legs one DPP quad, kDynEnvs rows per workgroup ----
// (the pointers to the row's tables in LDS stay with the kernel: formed here and carried in the struct, they changed the kernels' code)
struct DynLane {
  int el, leg;             // row in the workgroup, leg
  bool live;               // false on the lanes of rows past the end: they repeat the last row and store nothing
  int row, env;            // output row; the state's env index (checked on the host)
  __device__ __forceinline__ DynLane(const int32_t* ids, int rows_total) {
    el = threadIdx.x >> 2; leg = threadIdx.x & 3;
    live = blockIdx.x * kDynEnvs + el < rows_total;
    row = min(blockIdx.x * kDynEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kDynEnvs) workgroups)
    env = ids ? ids[row] : row;
  }
};

// ---- 1. the chain of this leg ----
// what the lane holds of its row's env once the chain is walked
struct DynFront {
  f3 o0, v0, w0;           // base origin, its velocity, the base's angular velocity (world)
  Ground g;
  DynLeg L;
  f3 ofoot, z3, aw;        // the foot link's origin, z axis and toe axis (its y)
  s33 I0;                  // the base body's inertia, world axes
  float m0, base;          // its mass; 1 on the leg-0 lane, which carries the base body into the quad sums, else 0
};
// R, o: the row's tables in LDS.  Holds one workgroup barrier (every thread of the workgroup calls it)
__device__ __forceinline__ void dyn_load_leg(const DevCfg& c, const float* state, int env, int leg, float (*R)[9], float (*o)[3], DynFront& F) {
  constexpr int NM = REX_NUM_MOTORS;
  const int n = c.n;
  if (leg == 0) fk_base(state, n, env, R[0], o[0]);
  __syncthreads();
  const f3 o0 = mk(o[0][0], o[0][1], o[0][2]);
  F.o0 = o0;
  F.v0 = mk(ldw(state, n, REX_S_LINVEL, env), ldw(state, n, REX_S_LINVEL + 1, env), ldw(state, n, REX_S_LINVEL + 2, env));
  F.w0 = mk(ldw(state, n, REX_S_ANGVEL, env), ldw(state, n, REX_S_ANGVEL + 1, env), ldw(state, n, REX_S_ANGVEL + 2, env));
  F.g = env_ground(c, env, c.env_index_base + env, (int)ldi(state, n, Lay<NM>::EPISODE, env));
  const Ground& g = F.g;
  DynLeg& L = F.L;
  F.ofoot = o0; F.z3 = mk(0.f, 0.f, 1.f); F.aw = mk(0.f, 1.f, 0.f);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int b = 1 + 3 * leg + i, ax = REX_JOINT_AXIS[i];
    fk_leg_body(state, n, env, b, R, o);
    const float* Rb = R[b];
    const f3 ex = mk(Rb[0], Rb[3], Rb[6]), ey = mk(Rb[1], Rb[4], Rb[7]), ez = mk(Rb[2], Rb[5], Rb[8]);
    const f3 ob = mk(o[b][0], o[b][1], o[b][2]);
    L.p[i] = ob - o0;
    L.a[i] = ax == 0 ? ex : ax == 1 ? ey : ez;
    L.r[i] = L.p[i] + ((float)REX_COM[1 + i][0] * ex + (float)REX_COM[1 + i][1] * ey + (float)REX_COM[1 + i][2] * ez);
    L.I[i] = rot_inertia(ex, ey, ez, (float)REX_INERTIA[1 + i][0], (float)REX_INERTIA[1 + i][1], (float)REX_INERTIA[1 + i][2]);
    L.m[i] = (float)REX_MASS[1 + i] * g.leg_mass_scale;
    L.qd[i] = ldw(state, n, Lay<NM>::QD + b - 1, env);
    if (i == 2) { F.ofoot = ob; F.z3 = ez; F.aw = ey; }
  }
  const float* R0 = R[0];
  const f3 bx = mk(R0[0], R0[3], R0[6]), by = mk(R0[1], R0[4], R0[7]), bz = mk(R0[2], R0[5], R0[8]);
  F.I0 = rot_inertia(bx, by, bz, (float)REX_INERTIA[0][0], (float)REX_INERTIA[0][1], (float)REX_INERTIA[0][2]);
  F.m0 = (float)REX_MASS[0] * g.base_mass_scale;
  F.base = leg == 0 ? 1.0f : 0.0f;
}

// ---- 2. composites, the leg's blocks of M ----
struct DynComposite {
  float mc[3]; f3 hc[3]; s33 Ic[3];      // subtree i of the leg: mass, first moment and rotational inertia about o_0
  f3 u[3], f[3], nn[3];                  // u_i = p_i x a_i; column i of B_f: (f_i, n_i)
  float mt; f3 ht; s33 It;               // the whole robot, on every lane of the quad: the base block [ mt 1, -[ht]x ; [ht]x, It ]
};
__device__ __forceinline__ void dyn_composites(const DynFront& F, DynComposite& C) {
  const DynLeg& L = F.L;
  const s33& I0 = F.I0;
  const float m0 = F.m0, base = F.base;
  float (&mc)[3] = C.mc; f3 (&hc)[3] = C.hc; s33 (&Ic)[3] = C.Ic;
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    mc[i] = L.m[i]; hc[i] = L.m[i] * L.r[i]; Ic[i] = L.I[i];
    add_point(Ic[i], L.m[i], L.r[i]);
    if (i < 2) { mc[i] += mc[i + 1]; hc[i] = hc[i] + hc[i + 1]; add(Ic[i], Ic[i + 1]); }
  }
  f3 (&u)[3] = C.u; f3 (&f)[3] = C.f; f3 (&nn)[3] = C.nn;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u[i] = cross(L.p[i], L.a[i]);
    f[i] = mc[i] * u[i] + cross(L.a[i], hc[i]);
    nn[i] = mul(Ic[i], L.a[i]) + cross(hc[i], u[i]);
  }
  C.mt = group_sum<4>(mc[0] + base * m0);
  C.ht = quad_sum(hc[0]);
  s33 It = Ic[0];
  It.xx += base * I0.xx; It.yy += base * I0.yy; It.zz += base * I0.zz; It.xy += base * I0.xy; It.xz += base * I0.xz; It.yz += base * I0.yz;
  It.xx = group_sum<4>(It.xx); It.yy = group_sum<4>(It.yy); It.zz = group_sum<4>(It.zz);
  It.xy = group_sum<4>(It.xy); It.xz = group_sum<4>(It.xz); It.yz = group_sum<4>(It.yz);
  C.It = It;
}
// H_f, both triangles written from one value
__device__ __forceinline__ void dyn_leg_block(const DynLeg& L, const DynComposite& C, float (&H)[3][3]) {
  const f3 (&u)[3] = C.u; const f3 (&f)[3] = C.f; const f3 (&nn)[3] = C.nn;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) H[i][j] = H[j][i] = dot(u[j], f[i]) + dot(L.a[j], nn[i]);
}

// ---- behind the front end: what the readouts agree on ----
// h(q, v) as rex_dynamics' bias: the base rows Ft, Nt (about o_0; the quad's sum, on every lane) and the leg's rows
// tq_i = a_i . (N_i - p_i x F_i), from leg_bias and the base body (a_c = 0, F = m g z, N = w x I w, on the leg-0 lane)
__device__ __forceinline__ void dyn_bias(const DynFront& F, f3& Ft, f3& Nt, float (&tq)[3]) {
  const DynLeg& L = F.L;
  f3 Fs[3], Ns[3];
  leg_bias(L, F.w0, Fs, Ns);
  const f3 gz = mk(0.f, 0.f, kGravity);
  Ft = quad_sum(Fs[0] + (F.base * F.m0) * gz);
  Nt = quad_sum(Ns[0] + F.base * cross(F.w0, mul(F.I0, F.w0)));
#pragma unroll
  for (int i = 0; i < 3; ++i) tq[i] = dot(L.a[i], Ns[i] - cross(L.p[i], Fs[i]));
}

// one kernel of this mapping over n rows (row k = env ids[k], or env k with ids null) with lds_bytes of dynamic LDS
template <typename Kernel, typename Args>
hipError_t dyn_launch(Kernel kernel, int lds_bytes, const RexSim* s, const int32_t* ids, int n, const Args& args, hipStream_t st) {
  const int blocks = (n + kDynEnvs - 1) / kDynEnvs;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kDynThreads), lds_bytes, st, s->dev, s->d_state, ids, n, args);
  return hipGetLastError();
}

}  // namespace
}  // namespace rex
