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
// Sections 1 and 2, the lane mapping (DynLane) and section 3's bias (dyn_bias) live in rex_dynamics_leg.h, which rex_dynamics_solve.hip
// (the solves with M) includes too.
// (Built as part of rex_render.hip's object, like rex_kinematics.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_dynamics.h"
#include "rex_dynamics_leg.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

// dynamic LDS of a workgroup: the FK tables, then over them (once every lane holds its leg in registers) the workgroup's rows of
// M, then of J, on their way out
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

__global__ void __launch_bounds__(kDynThreads) rex_dynamics_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                   int rows_total, RexDynamicsOut out) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const DynLane T(ids, rows_total);
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_dyn + T.el * kDynStride);      // the row's tables in LDS
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_dyn + T.el * kDynStride + 9 * REX_NB);
  const int el = T.el, leg = T.leg, row = T.row;
  const bool live = T.live;
  const int rows_live = min(kDynEnvs, rows_total - (int)blockIdx.x * kDynEnvs);   // this workgroup's rows of the output

  // ---- 1. the chain of this leg, 2. composites and the leg's blocks of M (rex_dynamics_leg.h) ----
  DynFront F;
  dyn_load_leg(c, state, T.env, T.leg, R, o, F);
  DynComposite C;
  dyn_composites(F, C);
  const f3 o0 = F.o0, v0 = F.v0, w0 = F.w0;
  const DynLeg& L = F.L;
  const s33& I0 = F.I0;
  const float m0 = F.m0, base = F.base, mt = C.mt;
  const float (&mc)[3] = C.mc; const f3 (&hc)[3] = C.hc; const f3 (&f)[3] = C.f; const f3 (&nn)[3] = C.nn;
  const f3 ht = C.ht;
  const s33 It = C.It;

  if (out.mass_matrix) {                                   // (every `if (out.x)` is the same in every thread)
    float H[3][3];
    dyn_leg_block(L, C, H);
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
    f3 Ft, Nt;
    float tq[3];
    dyn_bias(F, Ft, Nt, tq);
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
    const f3 tc = toe_centre(F.ofoot, F.z3);
    const bool field = c.n_terrain > 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f3 d = toe_point(F.g, field, tc, F.aw, e).P - o0;
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
  return rex::dyn_launch(rex::rex_dynamics_kernel, rex::kDynLdsBytes, s, d_ids, n, out, st);
}
