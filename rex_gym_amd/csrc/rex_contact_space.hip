// rex_contact_space.hip -- the contact-space (Delassus) matrix of the toe points, their drift and free accelerations, and inverse
// dynamics, for every env (rex_contact_space.h; the conventions: rex_contact_space in include/rexsim.h).
//
// Both kernels: one lane per (output row, leg), a row's four legs one DPP quad, 32 rows per workgroup -- the mapping and the front end
// (rex_dynamics_leg.h) of rex_dynamics_solve_kernel and rex_contact_solve_kernel.  The FK tables in LDS are the only shared memory; the
// state is only read.  A null output pointer is a launch-uniform skip.  Lanes of rows past the end repeat the last row, take part in the
// barrier, the quad sums and the broadcasts, and store nothing.
//
// rex_contact_space_kernel, all in registers:
//   1. toe_drift.  Down the lane's leg with w_0 the base's angular velocity and the base origin unaccelerated (vdot = 0):
//          acc(o_i) = acc(o_i-1) + alpha_i-1 x (o_i - o_i-1) + w_i-1 x (w_i-1 x (o_i - o_i-1)),   alpha_i = alpha_i-1 + w_i-1 x (qd_i a_i),
//          w_i = w_i-1 + qd_i a_i;  drift_p = acc(o_3) + alpha_3 x (P - o_3) + w_3 x (w_3 x (P - o_3))
//      -- leg_bias' recursion with the toe point (toe_point, rex_toe_point.h: the point rex_kinematics and rex_dynamics report) in the
//      place of the foot link's centre of mass.
//   2. toe_acc_free = J_p M^-1 (S^T tau + w - h) + drift_p:  h from leg_bias as rex_forward_dynamics forms it, one dyn_msolve with the
//      factors (rex_dynamics_factor.h), then  J_p x = x_lin + x_ang x (P - o_0) + sum_i x_i a_i x (P - o_i).
//   3. delassus.  The lane's six point rows (2 ends x 3 world axes; row 3 e + c is J_p's row c: base columns (e_c, (P - o_0) x e_c), leg
//      columns col_i . e_c) in the whitened coordinates of rex_contact_solve.hip section 2,
//          Jt = ( G^-1 (J_b^T - Y_f^T J_f^T),  D^-1/2 L^-1 J_f^T ),
//      in which M is the identity: an entry of J M^-1 J^T is the 9-term dot product of two rows of one leg and the 6-term dot product of
//      the base parts of rows of two legs.  The base parts of leg f's rows reach the quad by quad_perm broadcasts (constant patterns);
//      every lane forms its 6 x 24 slice.  Each product is summed over i = 0 .. 8 in that order from one multiply-add per term, on
//      whichever lane: the two lanes of a cross-leg pair, and the two triangles of a leg's own block, carry the same bits.
//      Stores: the lane's slice is 576 contiguous bytes of the row's 2 304; it goes out from the registers in 16-byte chunks, twelve
//      columns (two legs) at a time.  Staging a workgroup's rows in LDS for a linear write -- what rex_dynamics does for M and J; 32
//      rows are 72 KiB, so with the dynamic-LDS limit raised past the default 64 KiB -- was measured and is slower: 12.2 against 11.7 us
//      for 4 096 envs (13.3 against 12.7 us on the terrain; profiles/contact_space.md).
//
// rex_inverse_dynamics_kernel:  force = M vdot + h - S^T tau - sum_p J_p^T f_p - w  from the blocks at hand, M never assembled:
//      y_0 = Mb x_0 + sum_f B_f x_f  (the sum over the legs one quad sum),  y_f = B_f^T x_0 + H_f x_f;  h and the load as
//      rex_forward_dynamics forms them (the ground is queried only when toe forces are given).  No factorisation.
// (Built as part of rex_render.hip's object, like rex_contact_solve.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_contact_space.h"
#include "rex_dynamics_leg.h"
#include "rex_dynamics_factor.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

static_assert(kDynFkBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");
static_assert(kDelassusDim == 6 * REX_NLEG, "six point rows a leg");

__global__ void __launch_bounds__(kDynThreads) rex_contact_space_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                        int rows_total, RexContactSpaceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_csp[];
  const int el = threadIdx.x >> 2, leg = threadIdx.x & 3;
  const bool live = blockIdx.x * kDynEnvs + el < rows_total;
  const int row = min(blockIdx.x * kDynEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kDynEnvs) workgroups)
  const int env = ids ? ids[row] : row;                              // the state's env index (checked on the host)
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_csp + el * kDynStride);
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_csp + el * kDynStride + 9 * REX_NB);

  // ---- the leg and its composites (rex_dynamics_leg.h); the two toe points of the leg ----
  DynFront F;
  dyn_load_leg(c, state, env, leg, R, o, F);
  DynComposite C;
  dyn_composites(F, C);
  const DynLeg& L = F.L;
  const RexContactSpaceOut& out = a.out;
  f3 d[2], col[2][3];                                        // P - o_0; a_i x (P - o_i)
  {
    const f3 tc = toe_centre(F.ofoot, F.z3);
    const bool field = c.n_terrain > 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      d[e] = toe_point(F.g, field, tc, F.aw, e).P - F.o0;
#pragma unroll
      for (int i = 0; i < 3; ++i) col[e][i] = cross(L.a[i], d[e] - L.p[i]);
    }
  }

  // ---- 1. the drift acceleration Jdot v ----
  f3 drift[2];
  if (out.toe_drift || out.toe_acc_free) {                   // (every pointer test is the same in every thread)
    f3 w = F.w0, al = mk(0.f, 0.f, 0.f), ao = mk(0.f, 0.f, 0.f), pp = mk(0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const f3 dp = L.p[i] - pp;
      ao = ao + cross(al, dp) + cross(w, cross(w, dp));      // the joint point, carried by the parent
      al = al + L.qd[i] * cross(w, L.a[i]);                  // d/dt (qd a) at constant rate: the axis turns with the parent
      w = w + L.qd[i] * L.a[i];
      pp = L.p[i];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f3 rp = d[e] - L.p[2];
      drift[e] = ao + cross(al, rp) + cross(w, cross(w, rp));
    }
    if (out.toe_drift && live) {
      float* t = out.toe_drift + ((size_t)row * 8 + 2 * leg) * 3;
      dput3(t, drift[0]); dput3(t + 3, drift[1]);
    }
  }
  if (!out.toe_acc_free && !out.delassus) return;

  // ---- the leg block and the factors (rex_dynamics_factor.h) ----
  float H[3][3];
  dyn_leg_block(L, C, H);
  DynFactor Q;
  dyn_factor(C, H, Q);

  // ---- 2. the acceleration without ground forces ----
  if (out.toe_acc_free) {
    float bf[3] = {0.f, 0.f, 0.f};
    if (a.tau) {
      const float* t = a.tau + (size_t)row * 12 + 3 * leg;
      bf[0] = t[0]; bf[1] = t[1]; bf[2] = t[2];
    }
    f3 bl = mk(0.f, 0.f, 0.f), bn = mk(0.f, 0.f, 0.f);
    if (a.base) {
      const float* w = a.base + (size_t)row * 6;
      bl = mk(w[0], w[1], w[2]);
      bn = mk(w[3], w[4], w[5]);
    }
    f3 Fs[3], Ns[3];
    leg_bias(L, F.w0, Fs, Ns);                               // h as rex_dynamics' bias
    const f3 gz = mk(0.f, 0.f, kGravity);
    const f3 Ft = quad_sum(Fs[0] + (F.base * F.m0) * gz);
    const f3 Nt = quad_sum(Ns[0] + F.base * cross(F.w0, mul(F.I0, F.w0)));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float tq = dot(L.a[i], Ns[i] - cross(L.p[i], Fs[i]));
      bf[i] -= tq;
    }
    bl = bl - Ft; bn = bn - Nt;
    const float b0[6] = {bl.x, bl.y, bl.z, bn.x, bn.y, bn.z};
    float x0[6], xf[3];
    dyn_msolve(Q, b0, bf, x0, xf);
    const f3 xl = mk(x0[0], x0[1], x0[2]), xa = mk(x0[3], x0[4], x0[5]);
    if (live) {
      float* t = out.toe_acc_free + ((size_t)row * 8 + 2 * leg) * 3;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const f3 jx = xl + cross(xa, d[e]) + (xf[0] * col[e][0] + xf[1] * col[e][1] + xf[2] * col[e][2]);
        dput3(t + 3 * e, jx + drift[e]);
      }
    }
  }
  if (!out.delassus) return;

  // ---- 3. the whitened rows of this leg, and their products ----
  const float sd[3] = {sqrtf(Q.hq.i0), sqrtf(Q.hq.i1), sqrtf(Q.hq.i2)};       // D^-1/2
  float jt[6][9];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const int k = 3 * e + ax;
      const f3 u = mk(ax == 0 ? 1.f : 0.f, ax == 1 ? 1.f : 0.f, ax == 2 ? 1.f : 0.f);
      const f3 du = cross(d[e], u);
      const float jb[6] = {u.x, u.y, u.z, du.x, du.y, du.z};
      const float jf[3] = {comp(col[e][0], ax), comp(col[e][1], ax), comp(col[e][2], ax)};
      const float t0 = jf[0], t1 = jf[1] - Q.hq.l10 * t0, t2 = jf[2] - Q.hq.l20 * t0 - Q.hq.l21 * t1;      // L^-1 J_f^T
      jt[k][6] = t0 * sd[0]; jt[k][7] = t1 * sd[1]; jt[k][8] = t2 * sd[2];
#pragma unroll
      for (int i = 0; i < 6; ++i) {                                                                      // G^-1 (J_b^T - Y_f^T J_f^T)
        float t = jb[i] - (Q.Y[0][i] * jf[0] + Q.Y[1][i] * jf[1] + Q.Y[2][i] * jf[2]);
#pragma unroll
        for (int m = 0; m < i; ++m) t -= Q.aq.g[i][m] * jt[k][m];
        jt[k][i] = t * Q.aq.inv[i];
      }
    }
  float* dst = out.delassus + (size_t)row * kDelassusFloats + (size_t)(6 * leg) * kDelassusDim;      // rows 6 leg .. 6 leg + 5 of the env's matrix
#pragma unroll
  for (int half = 0; half < 2; ++half) {                     // columns 12 half .. 12 half + 11: the rows of legs 2 half and 2 half + 1
    float acc[6][12];
#pragma unroll
    for (int ff = 0; ff < 2; ++ff) {
      const int f = 2 * half + ff;                           // (a constant after unrolling)
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) {
        float b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) b[i] = quad_bcast(jt[kk][i], f);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          float s = 0.0f;
#pragma unroll
          for (int i = 0; i < 6; ++i) s += jt[k][i] * b[i];
          float s9 = s;                                      // on the owner b is its own row kk: the leg part joins
#pragma unroll
          for (int i = 6; i < 9; ++i) s9 += jt[k][i] * jt[kk][i];
          acc[k][6 * ff + kk] = leg == f ? s9 : s;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        float4* d4 = reinterpret_cast<float4*>(dst + k * kDelassusDim + 12 * half);
#pragma unroll
        for (int q = 0; q < 3; ++q) d4[q] = make_float4(acc[k][4 * q], acc[k][4 * q + 1], acc[k][4 * q + 2], acc[k][4 * q + 3]);
      }
    }
  }
}

__global__ void __launch_bounds__(kDynThreads) rex_inverse_dynamics_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                           int rows_total, RexInverseArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_inv[];
  const DynLane T(ids, rows_total);
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_inv + T.el * kDynStride);      // the row's tables in LDS
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_inv + T.el * kDynStride + 9 * REX_NB);
  const int leg = T.leg, row = T.row;

  DynFront F;
  dyn_load_leg(c, state, T.env, T.leg, R, o, F);
  const DynLeg& L = F.L;

  // ---- h(q, v) as rex_dynamics' bias ----
  f3 yl, yn;                                                 // base rows: force, moment about o_0
  float yf[3];
  {
    f3 Fs[3], Ns[3];
    leg_bias(L, F.w0, Fs, Ns);
    const f3 gz = mk(0.f, 0.f, kGravity);
    yl = quad_sum(Fs[0] + (F.base * F.m0) * gz);
    yn = quad_sum(Ns[0] + F.base * cross(F.w0, mul(F.I0, F.w0)));
#pragma unroll
    for (int i = 0; i < 3; ++i) yf[i] = dot(L.a[i], Ns[i] - cross(L.p[i], Fs[i]));
  }

  // ---- + M vdot from the blocks:  y_0 = Mb x_0 + sum_f B_f x_f,  y_f = B_f^T x_0 + H_f x_f ----
  if (a.vdot) {                                              // (every pointer test is the same in every thread)
    DynComposite C;
    dyn_composites(F, C);
    float H[3][3];
    dyn_leg_block(L, C, H);
    const float* x = a.vdot + (size_t)row * kDynDof;
    const f3 xl = mk(x[0], x[1], x[2]), xa = mk(x[3], x[4], x[5]);
    const float xf[3] = {x[6 + 3 * leg], x[7 + 3 * leg], x[8 + 3 * leg]};
    const f3 Bl = quad_sum(xf[0] * C.f[0] + xf[1] * C.f[1] + xf[2] * C.f[2]);
    const f3 Bn = quad_sum(xf[0] * C.nn[0] + xf[1] * C.nn[1] + xf[2] * C.nn[2]);
    yl = yl + (C.mt * xl + cross(xa, C.ht) + Bl);            // [ mt 1, -[ht]x ]
    yn = yn + (cross(C.ht, xl) + mul(C.It, xa) + Bn);        // [ [ht]x, It ]
#pragma unroll
    for (int i = 0; i < 3; ++i) yf[i] += dot(C.f[i], xl) + dot(C.nn[i], xa) + (H[i][0] * xf[0] + H[i][1] * xf[1] + H[i][2] * xf[2]);
  }

  // ---- - the load  S^T tau + sum_p J_p^T f_p + w,  as rex_forward_dynamics assembles it ----
  f3 bl = mk(0.f, 0.f, 0.f), bn = mk(0.f, 0.f, 0.f);
  float bf[3] = {0.f, 0.f, 0.f};
  if (a.joint) {
    const float* t = a.joint + (size_t)row * 12 + 3 * leg;
    bf[0] = t[0]; bf[1] = t[1]; bf[2] = t[2];
  }
  if (a.toe) {
    const f3 tc = toe_centre(F.ofoot, F.z3);
    const bool field = c.n_terrain > 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f3 d = toe_point(F.g, field, tc, F.aw, e).P - F.o0;
      const float* fp = a.toe + ((size_t)row * 8 + 2 * leg + e) * 3;
      const f3 fe = mk(fp[0], fp[1], fp[2]);
      bl = bl + fe;
      bn = bn + cross(d, fe);
#pragma unroll
      for (int i = 0; i < 3; ++i) bf[i] += dot(cross(L.a[i], d - L.p[i]), fe);
    }
    bl = quad_sum(bl); bn = quad_sum(bn);
  }
  if (a.base) {
    const float* w = a.base + (size_t)row * 6;
    bl = bl + mk(w[0], w[1], w[2]);
    bn = bn + mk(w[3], w[4], w[5]);
  }
  if (T.live) {                                              // the lane's share, as rex_dynamics_solve_kernel stores a solution
    float* t = a.force + (size_t)row * kDynDof;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[6 + 3 * leg + i] = yf[i] - bf[i];
    if (leg == 0) dput3(t, yl - bl);
    else if (leg == 1) dput3(t + 3, yn - bn);
  }
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_contact_space(const RexSim* s, const int32_t* d_ids, int n, const rex::RexContactSpaceArgs& a, hipStream_t st) {
  return rex::dyn_launch(rex::rex_contact_space_kernel, rex::kDynFkBytes, s, d_ids, n, a, st);
}

hipError_t rex_launch_inverse_dynamics(const RexSim* s, const int32_t* d_ids, int n, const rex::RexInverseArgs& a, hipStream_t st) {
  return rex::dyn_launch(rex::rex_inverse_dynamics_kernel, rex::kDynFkBytes, s, d_ids, n, a, st);
}
