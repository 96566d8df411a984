// rex_dynamics.hip -- mass matrix, bias forces, toe Jacobians, centre of mass and momentum of every env (rex_dynamics.h).
//
// rex_dynamics_kernel: one lane per (output row, leg), 32 rows per workgroup of 128 threads; mark base.
//   1. Forward kinematics in LDS with the renderer's functions (fk_base, fk_leg_body), exactly as rex_kinematics_kernel walks
//      them, so that both readouts describe one pose; the lane then holds its leg in registers: joint points p_i and link centres
//      of mass r_i relative to the base origin o_0, joint axes a_i, the links' world inertias about their centres of mass.
//   2. Composite rigid bodies in world-aligned axes about o_0 (the formulation at the top of rex_device.h, minus the whitening):
//      subtree i of the leg has mass mc_i, first moment hc_i = sum m_k r_k and rotational inertia Ic_i about o_0.  A unit rate of
//      joint i moves that composite with angular velocity a_i and velocity u_i = p_i x a_i of its material point at o_0, which
//      gives it the momentum  f_i = mc_i u_i + a_i x hc_i,  n_i = Ic_i a_i + hc_i x u_i  (n about o_0): column i of the coupling
//      B_f is (f_i, n_i), and  H_f[i][j] = u_j . f_i + a_j . n_i  for j <= i.
//   3. Newton-Euler with zero generalized acceleration: per link the bias accelerations, the wrench  F = m (a_c + g z),
//      N = I alpha + w x I w,  summed over the subtree about o_0;  h_i = a_i . (N_i - p_i x F_i).  With v = 0 only gravity is
//      left, which the composites give directly:  g a_i . ((hc_i - mc_i p_i) x z).
//   4. The base block, the base rows of bias / gravity, com, momentum and mass are the base body (added by the leg-0 lane) plus
//      the sum over the four lanes of the row -- one DPP quad: group_sum<4>, two quad_perm adds, no LDS, every lane holds the total.
//   5. The two toe points of the leg (toe_point, rex_toe_point.h: the point rex_kinematics reports) and their Jacobians
//      J_p = [ 1 | -[P - o_0]x | a_i x (P - o_0 - p_i) in the leg's three columns | 0 ].
// Every entry of M is written twice from one value (both triangles); blocks between two legs and the other legs' columns of J
// are written as zeros.  Stores: a workgroup's rows of M (1 296 B each) and of J (1 728 B each) are one contiguous range of
// the output, so the lanes stage them in LDS -- over the FK tables, which are dead by then -- and the workgroup writes the range
// linearly, 16 bytes per lane; per-lane stores of the 72-byte rows were measured and are slower (profiles/dynamics.md: 17.6
// against 12.1 us for the full readout of 4 096 envs), unlike at the 1 KB per env of rex_kinematics.  The small outputs (bias,
// gravity, com, momentum, mass) are stored by the lanes that hold them.  A null output pointer is a launch-uniform skip.  Lanes
// of rows past the end repeat the last row, take part in the barriers and the quad sums, and store nothing to global memory.
// (Built as part of rex_render.hip's object, like rex_kinematics.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_dynamics.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

// floats of one env's tables R[NB][9], o[NB][3] (odd: the lanes of one leg in neighbouring envs fall on different banks)
constexpr int kDynStride = (12 * REX_NB) | 1;
// dynamic LDS of a workgroup: the FK tables, then over them (once every lane holds its leg in registers) the workgroup's rows of
// M, then of J, on their way out
constexpr int kDynFkBytes = ((kDynEnvs * kDynStride + 3) & ~3) * (int)sizeof(float);
constexpr int kDynStageBytes = kDynEnvs * kDynJacFloats * (int)sizeof(float);
constexpr int kDynLdsBytes = kDynStageBytes > kDynFkBytes ? kDynStageBytes : kDynFkBytes;
static_assert(kDynLdsBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");
static_assert(kDynMassFloats % 4 == 0 && kDynJacFloats % 4 == 0, "a row of M or J is a whole number of 16-byte chunks");

// count4 float4 chunks from LDS to dst (16-byte aligned), workgroup-linearly: lane t writes chunks t, t + kDynThreads, ...
__device__ __forceinline__ void flush_rows(const float* lds, float* dst, int count4) {
  const float4* src4 = reinterpret_cast<const float4*>(lds);
  float4* dst4 = reinterpret_cast<float4*>(dst);
  for (int k = threadIdx.x; k < count4; k += kDynThreads) dst4[k] = src4[k];
}

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
static_assert(dyn_legs_alike(), "rex_dynamics_kernel reads leg 0's link constants for every leg, diagonal inertias, and a base whose centre of mass is its origin");

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

__global__ void __launch_bounds__(kDynThreads) rex_dynamics_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                   int rows_total, RexDynamicsOut out) {
  constexpr int NM = REX_NUM_MOTORS;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const int n = c.n;
  const int el = threadIdx.x >> 2, leg = threadIdx.x & 3;
  const bool live = blockIdx.x * kDynEnvs + el < rows_total;
  const int row = min(blockIdx.x * kDynEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kDynEnvs) workgroups)
  const int env = ids ? ids[row] : row;                              // the state's env index (checked on the host)
  const int rows_live = min(kDynEnvs, rows_total - (int)blockIdx.x * kDynEnvs);   // this workgroup's rows of the output
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_dyn + el * kDynStride);
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_dyn + el * kDynStride + 9 * REX_NB);

  // ---- 1. the chain of this leg ----
  if (leg == 0) fk_base(state, n, env, R[0], o[0]);
  __syncthreads();
  const f3 o0 = mk(o[0][0], o[0][1], o[0][2]);
  const f3 v0 = mk(ldw(state, n, REX_S_LINVEL, env), ldw(state, n, REX_S_LINVEL + 1, env), ldw(state, n, REX_S_LINVEL + 2, env));
  const f3 w0 = mk(ldw(state, n, REX_S_ANGVEL, env), ldw(state, n, REX_S_ANGVEL + 1, env), ldw(state, n, REX_S_ANGVEL + 2, env));
  const Ground g = env_ground(c, env, c.env_index_base + env, (int)ldi(state, n, Lay<NM>::EPISODE, env));
  DynLeg L;
  f3 ofoot = o0, z3 = mk(0.f, 0.f, 1.f), aw = mk(0.f, 1.f, 0.f);     // the foot link's origin, z axis and toe axis (its y)
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
    if (i == 2) { ofoot = ob; z3 = ez; aw = ey; }
  }
  const float* R0 = R[0];
  const f3 bx = mk(R0[0], R0[3], R0[6]), by = mk(R0[1], R0[4], R0[7]), bz = mk(R0[2], R0[5], R0[8]);
  const s33 I0 = rot_inertia(bx, by, bz, (float)REX_INERTIA[0][0], (float)REX_INERTIA[0][1], (float)REX_INERTIA[0][2]);
  const float m0 = (float)REX_MASS[0] * g.base_mass_scale;
  const float base = leg == 0 ? 1.0f : 0.0f;     // the leg-0 lane carries the base body into the quad sums

  // ---- 2. composites, the leg's blocks of M ----
  float mc[3]; f3 hc[3]; s33 Ic[3];
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    mc[i] = L.m[i]; hc[i] = L.m[i] * L.r[i]; Ic[i] = L.I[i];
    add_point(Ic[i], L.m[i], L.r[i]);
    if (i < 2) { mc[i] += mc[i + 1]; hc[i] = hc[i] + hc[i + 1]; add(Ic[i], Ic[i + 1]); }
  }
  f3 u[3], f[3], nn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u[i] = cross(L.p[i], L.a[i]);
    f[i] = mc[i] * u[i] + cross(L.a[i], hc[i]);
    nn[i] = mul(Ic[i], L.a[i]) + cross(hc[i], u[i]);
  }
  const float mt = group_sum<4>(mc[0] + base * m0);
  const f3 ht = quad_sum(hc[0]);
  s33 It = Ic[0];
  It.xx += base * I0.xx; It.yy += base * I0.yy; It.zz += base * I0.zz; It.xy += base * I0.xy; It.xz += base * I0.xz; It.yz += base * I0.yz;
  It.xx = group_sum<4>(It.xx); It.yy = group_sum<4>(It.yy); It.zz = group_sum<4>(It.zz);
  It.xy = group_sum<4>(It.xy); It.xz = group_sum<4>(It.xz); It.yz = group_sum<4>(It.yz);

  if (out.mass_matrix) {                                   // (every `if (out.x)` is the same in every thread)
    float H[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) H[i][j] = H[j][i] = dot(u[j], f[i]) + dot(L.a[j], nn[i]);
    __syncthreads();                                       // every lane holds its leg in registers: the FK tables are dead
    {
      float* Mr = s_dyn + el * kDynMassFloats;             // the row's M in LDS (lanes past the end stage their copy of the last row)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        float* leg_row = Mr + (6 + 3 * leg + i) * kDynDof;      // row 6 + 3 leg + i: B^T, then H in the leg's own columns
        dput3(leg_row, f[i]);
        dput3(leg_row + 3, nn[i]);
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
          for (int j = 0; j < 3; ++j) leg_row[6 + 3 * l + j] = l == leg ? H[i][j] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {                            // column 6 + 3 leg + i of the base rows: B
          Mr[k * kDynDof + 6 + 3 * leg + i] = comp(f[i], k);
          Mr[(3 + k) * kDynDof + 6 + 3 * leg + i] = comp(nn[i], k);
        }
      }
      // the base's 6 x 6 block [ m 1, -[h]x ; [h]x, Io ]: rows 0 and 4 by the leg-0 lane, 1 and 5 by leg 1, 2 by leg 2, 3 by leg 3
      auto row6 = [&](int r, float c0, float c1, float c2, float c3, float c4, float c5) {
        float* d = Mr + r * kDynDof;
        d[0] = c0; d[1] = c1; d[2] = c2; d[3] = c3; d[4] = c4; d[5] = c5;
      };
      if (leg == 0) { row6(0, mt, 0.f, 0.f, 0.f, ht.z, -ht.y); row6(4, ht.z, 0.f, -ht.x, It.xy, It.yy, It.yz); }
      else if (leg == 1) { row6(1, 0.f, mt, 0.f, -ht.z, 0.f, ht.x); row6(5, -ht.y, ht.x, 0.f, It.xz, It.yz, It.zz); }
      else if (leg == 2) row6(2, 0.f, 0.f, mt, ht.y, -ht.x, 0.f);
      else row6(3, 0.f, -ht.z, ht.y, It.xx, It.xy, It.xz);
    }
    __syncthreads();
    flush_rows(s_dyn, out.mass_matrix + (size_t)blockIdx.x * kDynEnvs * kDynMassFloats, rows_live * (kDynMassFloats / 4));
  }

  // ---- 3. bias and gravity ----
  const f3 gz = mk(0.f, 0.f, kGravity);
  if (out.gravity) {
    float tq[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tq[i] = dot(L.a[i], cross(hc[i] - mc[i] * L.p[i], gz));
    if (live) {
      float* d = out.gravity + (size_t)row * kDynDof;
      d[6 + 3 * leg] = tq[0]; d[7 + 3 * leg] = tq[1]; d[8 + 3 * leg] = tq[2];
      if (leg == 0) { dput3(d, mt * gz); dput3(d + 3, cross(ht, gz)); }
    }
  }
  if (out.bias) {
    f3 Fs[3], Ns[3];
    leg_bias(L, w0, Fs, Ns);
    float tq[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tq[i] = dot(L.a[i], Ns[i] - cross(L.p[i], Fs[i]));
    const f3 Ft = quad_sum(Fs[0] + (base * m0) * gz);                           // the base: a_c = 0, F = m g z, N = w x I w
    const f3 Nt = quad_sum(Ns[0] + base * cross(w0, mul(I0, w0)));
    if (live) {
      float* d = out.bias + (size_t)row * kDynDof;
      d[6 + 3 * leg] = tq[0]; d[7 + 3 * leg] = tq[1]; d[8 + 3 * leg] = tq[2];
      if (leg == 0) { dput3(d, Ft); dput3(d + 3, Nt); }
    }
  }

  // ---- 4. centre of mass, momentum, mass ----
  if (out.com || out.momentum) {
    f3 w = w0, vo = v0, pp = mk(0.f, 0.f, 0.f);
    f3 pl = (base * m0) * v0, lo = base * mul(I0, w0);                          // linear momentum; angular momentum about o_0
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      vo = vo + cross(w, L.p[i] - pp);
      w = w + L.qd[i] * L.a[i];
      const f3 mv = L.m[i] * (vo + cross(w, L.r[i] - L.p[i]));
      pl = pl + mv;
      lo = lo + mul(L.I[i], w) + cross(L.r[i], mv);
      pp = L.p[i];
    }
    pl = quad_sum(pl); lo = quad_sum(lo);
    const float inv = 1.0f / mt;
    const f3 rc = inv * ht;                                                     // centre of mass relative to o_0
    if (live && leg == 1 && out.com) { dput3(out.com + (size_t)row * 6, o0 + rc); dput3(out.com + (size_t)row * 6 + 3, inv * pl); }
    if (live && leg == 2 && out.momentum) { dput3(out.momentum + (size_t)row * 6, pl); dput3(out.momentum + (size_t)row * 6 + 3, lo - cross(rc, pl)); }
  }
  if (out.mass && live && leg == 3) out.mass[row] = mt;

  // ---- 5. the toe points of this leg and their Jacobians ----
  if (out.toe_jacobian) {
    __syncthreads();                                       // the FK tables, or the staged M, are dead
    const f3 tc = toe_centre(ofoot, z3);
    const bool field = c.n_terrain > 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f3 d = toe_point(g, field, tc, aw, e).P - o0;
      f3 col[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) col[i] = cross(L.a[i], d - L.p[i]);
      {
        float* J = s_dyn + el * kDynJacFloats + (2 * leg + e) * 3 * kDynDof;          // point p = 2 leg + e of the row, in LDS
        const float skew[3][3] = {{0.f, d.z, -d.y}, {-d.z, 0.f, d.x}, {d.y, -d.x, 0.f}};      // -[d]x
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float* Jk = J + k * kDynDof;
#pragma unroll
          for (int j = 0; j < 3; ++j) { Jk[j] = j == k ? 1.0f : 0.0f; Jk[3 + j] = skew[k][j]; }
#pragma unroll
          for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int i = 0; i < 3; ++i) Jk[6 + 3 * l + i] = l == leg ? comp(col[i], k) : 0.0f;
        }
      }
    }
    __syncthreads();
    flush_rows(s_dyn, out.toe_jacobian + (size_t)blockIdx.x * kDynEnvs * kDynJacFloats, rows_live * (kDynJacFloats / 4));
  }
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_dynamics(const RexSim* s, const int32_t* d_ids, int n, const RexDynamicsOut& out, hipStream_t st) {
  const int blocks = (n + rex::kDynEnvs - 1) / rex::kDynEnvs;
  hipLaunchKernelGGL(rex::rex_dynamics_kernel, dim3(blocks), dim3(rex::kDynThreads), rex::kDynLdsBytes, st, s->dev, s->d_state, d_ids, n, out);
  return hipGetLastError();
}
