// rex_dynamics_solve.hip -- x = M(q)^-1 b for every env by block elimination, M never leaving the registers (rex_dynamics_solve.h).
//
// rex_dynamics_solve_kernel: one lane per (output row, leg), a row's four legs one DPP quad, 32 rows per workgroup -- the mapping and
// the front end of rex_dynamics_kernel (rex_dynamics_leg.h): after it the lane holds its leg's block H_f (3 x 3, symmetric positive
// definite), its coupling B_f (6 x 3) and, like every lane of the quad, the base block Mb.  In the order v = (base 6, leg 0, .. leg 3)
//     M = [ Mb  B_0 .. B_3 ;  B_f^T  H_f on the diagonal, zeros between two legs ],
// so, all in registers (rex_dynamics_factor.h, shared with rex_contact_solve.hip):
//   1. H_f = L D L^T (3 x 3, three reciprocals).
//   2. Y_f = H_f^-1 B_f^T (3 x 6).
//   3. The Schur complement A = Mb - sum_f B_f Y_f: 21 entries, one group_sum<4> each; every lane of the quad holds A.
//   4. A = G G^T (Cholesky of the 6 x 6, on every lane: redundant work, no LDS and no atomics).
//   5. Per right-hand side b = (b_0 [6], b_f [3] per leg):  c = b_0 - sum_f Y_f^T b_f (six group sums),  x_0 = A^-1 c,
//      x_f = H_f^-1 b_f - Y_f x_0.
// Modes (launch-uniform, RexSolveArgs::mode):
//   kSolveRhs      K right-hand sides per row from rhs [n][K][18] to x [n][K][18]; rhs may be x itself (a row's right-hand side k
//                  is in the quad's registers before any of its lanes stores the solution k).
//   kSolveForward  one right-hand side assembled here,  b = S^T tau + sum_p J_p^T f_p + w - h(q, v):  tau the lane's three joints;
//                  f_p at the lane's own two toe points (toe_point, rex_toe_point.h: the point rex_kinematics and rex_dynamics
//                  report; the ground is queried only when toe forces are given), the base rows of J_p^T f_p = (f, (P - o_0) x f)
//                  by quad sum, the leg rows col_i . f with col_i = a_i x (P - o_0 - p_i);  w the wrench at the base origin;
//                  h by dyn_bias, which is rex_dynamics' bias.  x is vdot [n][18].
//   kSolveImpulse  the same assembly without h, every input an impulse; x is dv [n][18] (or null), and the lanes add dv to the
//                  velocity words of the row's env -- REX_S_LINVEL by the leg-0 lane, REX_S_ANGVEL by the leg-1 lane, the leg's
//                  three REX_S_QD words by its own lane -- one fp32 add per word from the value the front end read; no other
//                  state word is touched.  Rows must name distinct envs (the caller's duty, include/rexsim.h).
// What the two assembled modes leave out is stated once, in rex_dynamics_solve.h.
// Stores: each lane stores its own 3 (or 3 + 3) floats of a solution.  Staging a workgroup's solutions in LDS and writing them
// linearly was measured and is slower at every K (7.43 against 7.10 us at K = 1, 25.6 against 19.7 us at K = 24 for 4 096 envs,
// profiles/dynamics_solve.md): a solution is 72 bytes a row, not the 1 296 of a row of M, and the two barriers per solution cost
// more than the narrower stores.  Lanes of rows past the end repeat the last row, take part in the barrier and the quad sums, and
// store nothing.
// (Built as part of rex_render.hip's object, like rex_dynamics.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_dynamics_solve.h"
#include "rex_dynamics_leg.h"
#include "rex_dynamics_factor.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

static_assert(kDynFkBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");

__global__ void __launch_bounds__(kDynThreads) rex_dynamics_solve_kernel(DevCfg c, const float* state, const int32_t* __restrict__ ids,
                                                                         int rows_total, RexSolveArgs a) {
  constexpr int NM = REX_NUM_MOTORS;
  extern __shared__ __attribute__((aligned(16))) float s_sol[];
  const DynLane T(ids, rows_total);
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_sol + T.el * kDynStride);      // the row's tables in LDS
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_sol + T.el * kDynStride + 9 * REX_NB);
  const int el = T.el, leg = T.leg, row = T.row, env = T.env;
  const bool live = T.live;

  // ---- the leg, its composites, H_f and B_f, the base block (rex_dynamics_leg.h) ----
  DynFront F;
  dyn_load_leg(c, state, T.env, T.leg, R, o, F);
  DynComposite C;
  dyn_composites(F, C);
  const DynLeg& L = F.L;
  float H[3][3];
  dyn_leg_block(L, C, H);

  // ---- 1.-4. the factors (rex_dynamics_factor.h) ----
  DynFactor Q;
  dyn_factor(C, H, Q);

  // the lane's share of a solution: its leg's three joints; the base's linear part by the leg-0 lane, its angular part by the leg-1 lane
  auto store = [&](float* d, const float (&x0)[6], const float (&xf)[3]) {
    d[6 + 3 * leg] = xf[0]; d[7 + 3 * leg] = xf[1]; d[8 + 3 * leg] = xf[2];
    if (leg == 0) { d[0] = x0[0]; d[1] = x0[1]; d[2] = x0[2]; }
    else if (leg == 1) { d[3] = x0[3]; d[4] = x0[4]; d[5] = x0[5]; }
  };
  // a solution of every row of the workgroup to wg[row in the workgroup * stride + 0 .. 17]
  auto emit = [&](float* wg, size_t stride, const float (&x0)[6], const float (&xf)[3]) {
    if (live) store(wg + (size_t)el * stride, x0, xf);
  };
  const size_t wg_row = (size_t)blockIdx.x * kDynEnvs;       // the workgroup's first row

  if (a.mode == kSolveRhs) {                                 // (a.mode and every pointer test below are the same in every thread)
    for (int k = 0; k < a.K; ++k) {
      const size_t at = ((size_t)row * (size_t)a.K + (size_t)k) * kDynDof;
      const float* b = a.rhs + at;
      const float b0[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
      const float bf[3] = {b[6 + 3 * leg], b[7 + 3 * leg], b[8 + 3 * leg]};
      float x0[6], xf[3];
      dyn_msolve(Q, b0, bf, x0, xf);
      emit(a.x + (wg_row * (size_t)a.K + (size_t)k) * kDynDof, (size_t)a.K * kDynDof, x0, xf);
    }
    return;
  }

  // ---- the right-hand side of a load: b = S^T tau + sum_p J_p^T f_p + w (- h) ----
  f3 bl = mk(0.f, 0.f, 0.f), bn = mk(0.f, 0.f, 0.f);         // base rows: force, moment about o_0
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
  if (a.mode == kSolveForward) {                             // h as rex_dynamics' bias
    f3 Ft, Nt;
    float tq[3];
    dyn_bias(F, Ft, Nt, tq);
#pragma unroll
    for (int i = 0; i < 3; ++i) bf[i] -= tq[i];
    bl = bl - Ft; bn = bn - Nt;
  }
  const float b0[6] = {bl.x, bl.y, bl.z, bn.x, bn.y, bn.z};
  float x0[6], xf[3];
  dyn_msolve(Q, b0, bf, x0, xf);
  if (a.x) emit(a.x + wg_row * kDynDof, kDynDof, x0, xf);
  if (a.state && live) {                                             // the push: v += dv, one add per word
    const int n = c.n;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float v = L.qd[i] + xf[i];
      stw(a.state, n, Lay<NM>::QD + 3 * leg + i, env, v);
    }
    if (leg == 0) {
      const f3 v = F.v0 + mk(x0[0], x0[1], x0[2]);
      stw(a.state, n, REX_S_LINVEL, env, v.x); stw(a.state, n, REX_S_LINVEL + 1, env, v.y); stw(a.state, n, REX_S_LINVEL + 2, env, v.z);
    } else if (leg == 1) {
      const f3 v = F.w0 + mk(x0[3], x0[4], x0[5]);
      stw(a.state, n, REX_S_ANGVEL, env, v.x); stw(a.state, n, REX_S_ANGVEL + 1, env, v.y); stw(a.state, n, REX_S_ANGVEL + 2, env, v.z);
    }
  }
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_dynamics_solve(const RexSim* s, const int32_t* d_ids, int n, const rex::RexSolveArgs& a, hipStream_t st) {
  return rex::dyn_launch(rex::rex_dynamics_solve_kernel, rex::kDynFkBytes, s, d_ids, n, a, st);
}
