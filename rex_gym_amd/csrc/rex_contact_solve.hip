// rex_contact_solve.hip -- one substep's contact problem of every env, restated from the state, solved and read out
// (rex_contact_solve.h; the problem: rex_contact_solve in include/rexsim.h).
//
// rex_contact_solve_kernel: one lane per (output row, leg), a row's four legs one DPP quad, 32 rows per workgroup -- the mapping, the
// front end (rex_dynamics_leg.h) and the factors (rex_dynamics_factor.h) of rex_dynamics_solve_kernel.  Then, all in registers:
//   1. The free velocity  v* = v + dt M^-1 (S^T tau - h - d):  h from leg_bias as rex_forward_dynamics forms it; d, the sim's
//      per-link damping (force m (kLinDamp + kLinDamp |vc|) vc at the centre of mass, moment (kAngDamp + kAngDamp |w|) I w), is added to
//      the links' bias wrenches before their projection, so it takes h's path; one solve with the factors.
//   2. The rows of the lane's leg, 9 of the env's 36: local 0..2 the joint-limit rows of its joints, 3..4 the normal rows of its two toe
//      points (toe_point, rex_toe_point.h), 5..8 their friction rows (plane_space).  Each row is kept in the whitened coordinates of
//      rex_device.h's header comment, taken from the factors at hand: with H_f = L D L^T, G_f = L D^1/2 and A = G G^T,
//          y = G^T v_base,   z_f = G_f^T (qd_f + Y_f v_base)
//      make the mass matrix the identity, and a row J = (J_b [6], J_f [3] in its own leg's columns) becomes ONE 9-vector
//          Jt = ( G^-1 (J_b^T - Y_f^T J_f^T),  D^-1/2 L^-1 J_f^T )
//      that is Jacobian and unit-impulse response at once; its diagonal J M^-1 J^T is |Jt|^2.  81 registers a lane, and no lane stores
//      another lane's rows.  The alternative, M^-1 J^T per row, is dense -- 18 floats a row next to the 9 of J, 83 KB of LDS for a
//      workgroup's 32 x 36 responses, past the 64 KiB a launch gets by default -- and was not built (profiles/contact_solve.md).
//   3. Projected Gauss-Seidel in the oracle's row order -- limit rows j = 0..11, normal rows p = 0..7, friction rows (p, 0), (p, 1) --
//      fully unrolled: the owner of global row r is a compile-time constant, so every lane evaluates ITS local row of that kind, the
//      owner's impulse step dl and the six base entries of its Jt reach the quad by quad_perm broadcasts (constant patterns), every
//      lane moves its copy of y, the owner alone moves its z_f and its lambda.  No LDS and no atomics in the loop.  Rows that are not
//      active (a joint inside its bounds, a point out of reach) have the bounds 0..0: they run as no-ops, the quad never diverges on
//      the active set, and they add nothing to the residual.
//   4. An env is done after `iterations` sweeps or after the first one whose largest (dl diag)^2 is within the threshold.  Until the
//      last env of the wave is done (one ballot per sweep) its lanes stay predicated off by a select, not by the exec mask: `done`
//      joins the owner's predicate, so its dl is 0, its lambdas, y and z keep their bits and its count stands still.  (With the lanes
//      masked off instead, a partly finished wave ran 1.5 x slower per sweep than a full one, profiles/contact_solve.md.)
//   5. v_next = clamp(v* + W^-1 (y, z), +-kMaxCoordVel); forces = impulses / dt.
// The FK tables in LDS are the only shared memory; the state is only read.  A null output pointer is a launch-uniform skip.  Lanes of
// rows past the end repeat the last row, take part in the barrier, the quad sums and the ballots, and store nothing.
// (Built as part of rex_render.hip's object, like rex_dynamics_solve.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_contact_solve.h"
#include "rex_contact_rows.h"

namespace rex {

namespace {

static_assert(kDynFkBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");

__global__ void __launch_bounds__(kDynThreads) rex_contact_solve_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                        int rows_total, RexContactArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_con[];
  const int el = threadIdx.x >> 2, leg = threadIdx.x & 3;
  const bool live = blockIdx.x * kDynEnvs + el < rows_total;
  const int row = min(blockIdx.x * kDynEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kDynEnvs) workgroups)
  const int env = ids ? ids[row] : row;                              // the state's env index (checked on the host)
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_con + el * kDynStride);
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_con + el * kDynStride + 9 * REX_NB);

  // ---- the leg, its composites, H_f and B_f, the base block (rex_dynamics_leg.h); the factors (rex_dynamics_factor.h) ----
  DynFront F;
  dyn_load_leg(c, state, env, leg, R, o, F);
  DynComposite C;
  dyn_composites(F, C);
  const DynLeg& L = F.L;
  float H[3][3];
  dyn_leg_block(L, C, H);
  DynFactor Q;
  dyn_factor(C, H, Q);
  const float dt = a.dt;

  // ---- 1. the free velocity (sections 1-5: rex_contact_rows.h) ----
  float vs0[6], vsf[3];
  {
    float bf[3] = {0.f, 0.f, 0.f};
    if (a.tau) {                                              // (a.tau, a.damping and every output pointer are the same in every thread)
      const float* t = a.tau + (size_t)row * 12 + 3 * leg;
      bf[0] = t[0]; bf[1] = t[1]; bf[2] = t[2];
    }
    con_free_velocity(F, Q, bf, a.damping, dt, vs0, vsf);
  }

  // ---- 2. the rows of this leg ----
  ConRows P;
  con_build_rows(state, c.n, env, leg, c.n_terrain > 0, F, Q, dt, vs0, vsf, P);
  const float (&lam)[9] = P.lam; const float (&hi)[5] = P.hi; const float (&lsgn)[3] = P.lsgn; const f3 (&nrm)[2] = P.nrm;

  // ---- 3., 4. projected Gauss-Seidel on the whitened velocity change ----
  const int count = con_sweeps(P, F.g.mu, leg, a.iterations, a.threshold);

  // ---- 5. the readout ----
  const RexContactSolveOut& out = a.out;
  if (out.v_next) {
    float dx[6], dq[3];
    con_velocity_change(Q, P, dx, dq);
    if (live) {
      float* d = out.v_next + (size_t)row * kDynDof;
#pragma unroll
      for (int i = 0; i < 3; ++i) d[6 + 3 * leg + i] = clampf(vsf[i] + dq[i], -kMaxCoordVel, kMaxCoordVel);
      if (leg == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = clampf(vs0[i] + dx[i], -kMaxCoordVel, kMaxCoordVel);
      } else if (leg == 1) {
#pragma unroll
        for (int i = 3; i < 6; ++i) d[i] = clampf(vs0[i] + dx[i], -kMaxCoordVel, kMaxCoordVel);
      }
    }
  }
  if (out.toe_lambda && live) {
    float* d = out.toe_lambda + ((size_t)row * 8 + 2 * leg) * 3;
#pragma unroll
    for (int e = 0; e < 2; ++e) { d[3 * e] = lam[3 + e]; d[3 * e + 1] = lam[5 + 2 * e]; d[3 * e + 2] = lam[6 + 2 * e]; }
  }
  if (out.toe_force && live) {
    float* d = out.toe_force + ((size_t)row * 8 + 2 * leg) * 3;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      f3 t1, t2;
      plane_space(nrm[e], t1, t2);
      const f3 imp = lam[3 + e] * nrm[e] + lam[5 + 2 * e] * t1 + lam[6 + 2 * e] * t2;
      const bool act = hi[3 + e] > 0.0f;
      d[3 * e] = act ? imp.x / dt : 0.0f; d[3 * e + 1] = act ? imp.y / dt : 0.0f; d[3 * e + 2] = act ? imp.z / dt : 0.0f;
    }
  }
  if (out.limit_torque && live) {
    float* d = out.limit_torque + (size_t)row * 12 + 3 * leg;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = lsgn[k] * lam[k] / dt;
  }
  if (out.sweeps && live && leg == 0) out.sweeps[row] = count;
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_contact_solve(const RexSim* s, const int32_t* d_ids, int n, const rex::RexContactArgs& a, hipStream_t st) {
  return rex::dyn_launch(rex::rex_contact_solve_kernel, rex::kDynFkBytes, s, d_ids, n, a, st);
}
