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
#include "rex_dynamics_leg.h"
#include "rex_dynamics_factor.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

static_assert(kDynFkBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");

constexpr float kRowUnbounded = 1e10f;       // upper bound of an active unilateral row (the oracle's)

__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, dpp_f<kDppXor1>(v));
  return fmaxf(v, dpp_f<kDppXor2>(v));
}

__global__ void __launch_bounds__(kDynThreads) rex_contact_solve_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                        int rows_total, RexContactArgs a) {
  constexpr int NM = REX_NUM_MOTORS;
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

  // ---- 1. the free velocity ----
  float vs0[6], vsf[3];
  {
    float bf[3] = {0.f, 0.f, 0.f};
    if (a.tau) {                                              // (a.tau, a.damping and every output pointer are the same in every thread)
      const float* t = a.tau + (size_t)row * 12 + 3 * leg;
      bf[0] = t[0]; bf[1] = t[1]; bf[2] = t[2];
    }
    f3 Fs[3], Ns[3];
    leg_bias(L, F.w0, Fs, Ns);
    f3 F0 = (F.base * F.m0) * mk(0.f, 0.f, kGravity), N0 = F.base * cross(F.w0, mul(F.I0, F.w0));      // the base body, on the leg-0 lane
    if (a.damping) {
      f3 w = F.w0, vo = F.v0, pp = mk(0.f, 0.f, 0.f);
      f3 Fd[3], Nd[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        vo = vo + cross(w, L.p[i] - pp);                      // the joint point, carried by the parent
        w = w + L.qd[i] * L.a[i];
        const f3 vc = vo + cross(w, L.r[i] - L.p[i]);
        const float dl = kLinDamp + kLinDamp * sqrtf(dot(vc, vc)), da = kAngDamp + kAngDamp * sqrtf(dot(w, w));
        Fd[i] = (L.m[i] * dl) * vc;
        Nd[i] = da * mul(L.I[i], w) + cross(L.r[i], Fd[i]);
        pp = L.p[i];
      }
      Fs[2] = Fs[2] + Fd[2]; Ns[2] = Ns[2] + Nd[2];
      Fs[1] = Fs[1] + (Fd[1] + Fd[2]); Ns[1] = Ns[1] + (Nd[1] + Nd[2]);
      Fs[0] = Fs[0] + (Fd[0] + (Fd[1] + Fd[2])); Ns[0] = Ns[0] + (Nd[0] + (Nd[1] + Nd[2]));
      const float dl0 = kLinDamp + kLinDamp * sqrtf(dot(F.v0, F.v0)), da0 = kAngDamp + kAngDamp * sqrtf(dot(F.w0, F.w0));
      F0 = F0 + (F.base * F.m0 * dl0) * F.v0;
      N0 = N0 + (F.base * da0) * mul(F.I0, F.w0);
    }
    const f3 Ft = quad_sum(Fs[0] + F0), Nt = quad_sum(Ns[0] + N0);
#pragma unroll
    for (int i = 0; i < 3; ++i) bf[i] -= dot(L.a[i], Ns[i] - cross(L.p[i], Fs[i]));
    const float b0[6] = {-Ft.x, -Ft.y, -Ft.z, -Nt.x, -Nt.y, -Nt.z};
    float x0[6], xf[3];
    dyn_msolve(Q, b0, bf, x0, xf);
    vs0[0] = F.v0.x + dt * x0[0]; vs0[1] = F.v0.y + dt * x0[1]; vs0[2] = F.v0.z + dt * x0[2];
    vs0[3] = F.w0.x + dt * x0[3]; vs0[4] = F.w0.y + dt * x0[4]; vs0[5] = F.w0.z + dt * x0[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) vsf[i] = L.qd[i] + dt * xf[i];
  }

  // ---- 2. the rows of this leg ----
  const float sd[3] = {sqrtf(Q.hq.i0), sqrtf(Q.hq.i1), sqrtf(Q.hq.i2)};       // D^-1/2
  float jt[9][9], rhs[9], dg[9], idg[9], hi[5], lam[9];
  // local row k from its Jacobian (jb: the base's columns, jf: the leg's); -> J v*
  auto whiten = [&](int k, const float (&jb)[6], const float (&jf)[3]) {
    const float t0 = jf[0], t1 = jf[1] - Q.hq.l10 * t0, t2 = jf[2] - Q.hq.l20 * t0 - Q.hq.l21 * t1;      // L^-1 J_f^T
    jt[k][6] = t0 * sd[0]; jt[k][7] = t1 * sd[1]; jt[k][8] = t2 * sd[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                                                      // G^-1 (J_b^T - Y_f^T J_f^T)
      float t = jb[i] - (Q.Y[0][i] * jf[0] + Q.Y[1][i] * jf[1] + Q.Y[2][i] * jf[2]);
#pragma unroll
      for (int m = 0; m < i; ++m) t -= Q.aq.g[i][m] * jt[k][m];
      jt[k][i] = t * Q.aq.inv[i];
    }
    float d = 0.0f, vel = jf[0] * vsf[0] + jf[1] * vsf[1] + jf[2] * vsf[2];
#pragma unroll
    for (int i = 0; i < 9; ++i) d += jt[k][i] * jt[k][i];
#pragma unroll
    for (int i = 0; i < 6; ++i) vel += jb[i] * vs0[i];
    dg[k] = d; idg[k] = 1.0f / d; lam[k] = 0.0f;
    return vel;
  };
  float lsgn[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {                               // (a) the near bound of each joint, a row once it is passed
    const float q = ldw(state, c.n, Lay<NM>::Q + 3 * leg + k, env);
    const float lo_gap = q - (float)REX_LEG_LIMIT_LO[k], hi_gap = (float)REX_LEG_LIMIT_HI[k] - q;
    const bool lower = lo_gap < hi_gap;
    const float gap = lower ? lo_gap : hi_gap;
    const bool act = gap < 0.0f;
    lsgn[k] = lower ? 1.0f : -1.0f;
    const float jb[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float jf[3] = {k == 0 ? lsgn[k] : 0.f, k == 1 ? lsgn[k] : 0.f, k == 2 ? lsgn[k] : 0.f};
    const float vel = whiten(k, jb, jf);
    rhs[k] = act ? (-gap * kErp / dt - vel) * idg[k] : 0.0f;
    hi[k] = act ? kRowUnbounded : 0.0f;
  }
  const float mu = F.g.mu;
  f3 nrm[2];
  {
    const f3 tc = toe_centre(F.ofoot, F.z3);
    const bool field = c.n_terrain > 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {                             // (b), (c) the two toe points: normal, then the two tangents
      const ToePoint tp = toe_point(F.g, field, tc, F.aw, e);
      const f3 d = tp.P - F.o0;
      const bool act = tp.dist < kBreaking;
      nrm[e] = tp.nrm;
      f3 t1, t2;
      plane_space(tp.nrm, t1, t2);
      f3 col[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) col[i] = cross(L.a[i], d - L.p[i]);
#pragma unroll
      for (int dir = 0; dir < 3; ++dir) {
        const f3 u = dir == 0 ? tp.nrm : dir == 1 ? t1 : t2;
        const f3 du = cross(d, u);
        const float jb[6] = {u.x, u.y, u.z, du.x, du.y, du.z};
        const float jf[3] = {dot(col[0], u), dot(col[1], u), dot(col[2], u)};
        const int k = dir == 0 ? 3 + e : 5 + 2 * e + (dir - 1);
        const float vel = whiten(k, jb, jf);
        if (dir == 0) {
          const float poserr = tp.dist > 0.0f ? 0.0f : -tp.dist * kErp / dt;
          const float velerr = -vel - (tp.dist > 0.0f ? tp.dist / dt : 0.0f);
          rhs[k] = act ? (poserr + velerr) * idg[k] : 0.0f;
          hi[k] = act ? kRowUnbounded : 0.0f;
        } else {
          rhs[k] = act ? -vel * idg[k] : 0.0f;
        }
      }
    }
  }

  // ---- 3., 4. projected Gauss-Seidel on the whitened velocity change (y on every lane of the quad, z the lane's own) ----
  float y[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, z[3] = {0.f, 0.f, 0.f};
  float worst = 0.0f;
  bool done = false;
  // global row owned by leg f (a constant after unrolling), local index k; kn: the local index of a friction row's normal row, else -1
  auto sweep_row = [&](int f, int k, int kn) {
    float vel = jt[k][6] * z[0] + jt[k][7] * z[1] + jt[k][8] * z[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) vel += jt[k][i] * y[i];
    const float top = kn >= 0 ? mu * lam[kn >= 0 ? kn : 0] : hi[k < 5 ? k : 0];     // (kn and k are constants here)
    const float bot = kn >= 0 ? -top : 0.0f;
    float dl = rhs[k] - vel * idg[k];
    const float want = lam[k] + dl;
    const float sum = fminf(fmaxf(want, bot), top);          // the oracle's two-sided clamp without a branch: 36 taken branches a sweep cost
    dl = sum != want ? sum - lam[k] : dl;                     // more than the sweep's arithmetic once part of the wave is predicated off
    const bool own = (leg == f) & !done;                      // a finished env sweeps on with dl = 0: nothing of it moves any more
    lam[k] = own ? sum : lam[k];
    const float dlo = own ? dl : 0.0f;
    z[0] += jt[k][6] * dlo; z[1] += jt[k][7] * dlo; z[2] += jt[k][8] * dlo;
    const float res = dlo * dg[k];
    worst = fmaxf(worst, res * res);
    const float dlq = quad_bcast(dlo, f);
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] += quad_bcast(jt[k][i], f) * dlq;
  };
  int count = 0;
  for (int it = 0; it < a.iterations; ++it) {
    worst = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; ++j) sweep_row(j / 3, j % 3, -1);
#pragma unroll
    for (int p = 0; p < 8; ++p) sweep_row(p >> 1, 3 + (p & 1), -1);
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      sweep_row(p >> 1, 5 + 2 * (p & 1), 3 + (p & 1));
      sweep_row(p >> 1, 6 + 2 * (p & 1), 3 + (p & 1));
    }
    count += done ? 0 : 1;
    done = done || (a.threshold > 0.0f && quad_max(worst) <= a.threshold);      // (the same in the four lanes of a quad)
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
  }

  // ---- 5. the readout ----
  const RexContactSolveOut& out = a.out;
  if (out.v_next) {
    float dx[6], dq[3];
#pragma unroll
    for (int i = 5; i >= 0; --i) {                            // G^-T y
      float t = y[i];
#pragma unroll
      for (int m = i + 1; m < 6; ++m) t -= Q.aq.g[m][i] * dx[m];
      dx[i] = t * Q.aq.inv[i];
    }
    const float t0 = z[0] * sd[0], t1 = z[1] * sd[1], t2 = z[2] * sd[2];          // L^-T D^-1/2 z - Y_f dv_base
    dq[2] = t2; dq[1] = t1 - Q.hq.l21 * dq[2]; dq[0] = t0 - Q.hq.l10 * dq[1] - Q.hq.l20 * dq[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int m = 0; m < 6; ++m) dq[i] -= Q.Y[i][m] * dx[m];
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
