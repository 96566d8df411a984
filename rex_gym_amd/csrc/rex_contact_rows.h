// rex_contact_rows.h -- one substep's contact problem of a lane's leg, from the front end (rex_dynamics_leg.h) and the factors
// (rex_dynamics_factor.h) to the velocity change: sections 1-5 of rex_contact_solve_kernel as device functions, shared by
// rex_contact_solve.hip (one substep of the state as it is) and rex_rollout.hip (substep after substep of a private copy).  Lifted with
// every expression spelled as it stood in rex_contact_solve_kernel (the build fixes arithmetic by source, -ffp-contract=on:
// rex_contact_solve's outputs are bit-identical to those before the lift, profiles/rollout.md).  The sections, the whitened rows and the
// predication of finished envs are described at the top of rex_contact_solve.hip.
#pragma once
#include "rex_render_common.h"
#include "rex_dynamics_leg.h"
#include "rex_dynamics_factor.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

constexpr float kRowUnbounded = 1e10f;       // upper bound of an active unilateral row (the oracle's)

__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, dpp_f<kDppXor1>(v));
  return fmaxf(v, dpp_f<kDppXor2>(v));
}

// the 9 rows of the lane's leg (local 0..2 the joint-limit rows, 3..4 the normal rows of its two toe points, 5..8 their friction rows)
// in whitened coordinates, and the solver's state
struct ConRows {
  float sd[3];                                 // D^-1/2
  float jt[9][9], rhs[9], dg[9], idg[9], hi[5], lam[9];
  float lsgn[3];                               // sign of the limit rows
  f3 nrm[2];                                   // the ground's normal at the two toe points
  float y[6], z[3];                            // the whitened velocity change: y on every lane of the quad, z the lane's own
};

// ---- 1. the free velocity ----
// bf: the leg's joint torques on entry (the bias and the damping are taken off here).  WRENCH: wrench [6] is a world force at the base
// origin and a world moment (rex_forward_dynamics' base_wrench), the same on every lane of the quad; else it is not read.  Ft, Nt are
// the bias wrench about the base origin, so the wrench is taken off them once per row, behind the quad sum; x - (+0) is x: a zero
// wrench changes no bit.  (A template argument, so that the callers without a wrench compile to the code they had:
// profiles/rollout_from.md)
template <bool WRENCH = false>
__device__ __forceinline__ void con_free_velocity(const DynFront& F, const DynFactor& Q, float (&bf)[3], int damping, float dt, float (&vs0)[6],
                                                  float (&vsf)[3], const float* wrench = nullptr) {
  const DynLeg& L = F.L;
  f3 Fs[3], Ns[3];
  leg_bias(L, F.w0, Fs, Ns);
  f3 F0 = (F.base * F.m0) * mk(0.f, 0.f, kGravity), N0 = F.base * cross(F.w0, mul(F.I0, F.w0));      // the base body, on the leg-0 lane
  if (damping) {
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
  f3 Ft = quad_sum(Fs[0] + F0), Nt = quad_sum(Ns[0] + N0);
  if constexpr (WRENCH) {
    Ft = Ft - mk(wrench[0], wrench[1], wrench[2]);
    Nt = Nt - mk(wrench[3], wrench[4], wrench[5]);
  }
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
// st, n, idx: where the leg's joint angles are read (ldw(st, n, Lay::Q + j, idx)); field: the env stands on a heightfield
__device__ __forceinline__ void con_build_rows(const float* st, int n, int idx, int leg, bool field, const DynFront& F, const DynFactor& Q, float dt,
                                               const float (&vs0)[6], const float (&vsf)[3], ConRows& P) {
  constexpr int NM = REX_NUM_MOTORS;
  const DynLeg& L = F.L;
  float (&sd)[3] = P.sd;
  sd[0] = sqrtf(Q.hq.i0); sd[1] = sqrtf(Q.hq.i1); sd[2] = sqrtf(Q.hq.i2);       // D^-1/2
  float (&jt)[9][9] = P.jt; float (&rhs)[9] = P.rhs; float (&dg)[9] = P.dg; float (&idg)[9] = P.idg; float (&hi)[5] = P.hi; float (&lam)[9] = P.lam;
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
  float (&lsgn)[3] = P.lsgn;
#pragma unroll
  for (int k = 0; k < 3; ++k) {                               // (a) the near bound of each joint, a row once it is passed
    const float q = ldw(st, n, Lay<NM>::Q + 3 * leg + k, idx);
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
  f3 (&nrm)[2] = P.nrm;
  {
    const f3 tc = toe_centre(F.ofoot, F.z3);
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
}

// ---- 3., 4. projected Gauss-Seidel on the whitened velocity change (y on every lane of the quad, z the lane's own) ----
// -> the env's own sweep count (the same in the four lanes of a quad).  Every thread of the wave calls it (one ballot per sweep)
__device__ __forceinline__ int con_sweeps(ConRows& P, float mu, int leg, int iterations, float threshold) {
  float (&jt)[9][9] = P.jt; float (&rhs)[9] = P.rhs; float (&dg)[9] = P.dg; float (&idg)[9] = P.idg; float (&hi)[5] = P.hi; float (&lam)[9] = P.lam;
  float (&y)[6] = P.y; float (&z)[3] = P.z;
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) z[i] = 0.f;
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
  for (int it = 0; it < iterations; ++it) {
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
    done = done || (threshold > 0.0f && quad_max(worst) <= threshold);      // (the same in the four lanes of a quad)
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
  }
  return count;
}

// ---- 5. the velocity change in the coordinates of v: dx the base's six, dq the leg's three ----
__device__ __forceinline__ void con_velocity_change(const DynFactor& Q, const ConRows& P, float (&dx)[6], float (&dq)[3]) {
  const float (&sd)[3] = P.sd; const float (&y)[6] = P.y; const float (&z)[3] = P.z;
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
}

}  // namespace
}  // namespace rex
