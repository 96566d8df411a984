// rex_force_distribution.hip -- force distribution per env (rex_force_distribution.h; the problem and the iteration are stated once, at
// rex_force_distribution in include/rexsim.h):
//
//     minimise  1/2 (A f - r)^T W (A f - r) + 1/2 eps sum_p |f_p|^2    over f_p in K_p (p in S), f_p = 0 otherwise
//
// with r = (M vdot + h - w)[0:6] the base rows of the equation of motion, A f = (sum_p f_p, sum_p d_p x f_p) what the ground supplies there,
// K_p the circular friction cone about the ground normal at toe point p -- by `iterations` accelerated projected-gradient steps from zero.
//
// The mapping of rex_contact_space_kernel: one lane per (output row, leg), a row's four legs one DPP quad, 32 rows per workgroup, the front end
// of rex_dynamics_leg.h.  The FK tables in LDS are the only shared memory; the state is only read; no atomics.  A null output pointer is a
// launch-uniform skip.  Lanes of rows past the end repeat the last row, take part in the barrier and in every quad sum, and store nothing.
//   Set-up.  h and M vdot as rex_inverse_dynamics_kernel forms them (dyn_bias; dyn_composites and dyn_leg_block when vdot is given; no
//     factorisation); the lane's two toe points with their normals, d = P - o_0 and col_i = a_i x (P - o_i) (toe_point, rex_toe_point.h);
//     mu; the step bound L by one quad sum.
//   Loop.  Each lane owns the six unknowns of its leg.  A y is six quad sums a step; the gradient, the cone projection (selects, no
//     branches) and the momentum step are lane-local.  The loop bound is a kernel argument, the same in every lane: no early exit.
//   Read-out.  One more gradient at the returned f gives base_residual = r - A f and the fixed-point residual; tau from col.
// (Built as part of rex_render.hip's object, like rex_contact_space.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_force_distribution.h"
#include "rex_dynamics_leg.h"
#include "rex_toe_point.h"

namespace rex {

namespace {

static_assert(kDynFkBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");

__device__ __forceinline__ float force_quad_max(float v) {
  v = fmaxf(v, dpp_f<kDppXor1>(v));
  return fmaxf(v, dpp_f<kDppXor2>(v));
}

// one toe point of the problem
struct ForcePoint {
  f3 d, nrm;               // P - o_0, the ground normal at P
  bool in;                 // in the stance set
};

// Proj_K of x onto the cone of half-angle atan(mu) about p.nrm (inv = 1 / (1 + mu^2)); zero for a point outside the stance set
__device__ __forceinline__ f3 cone_project(const ForcePoint& p, float mu, float inv, f3 x) {
  const float s = dot(p.nrm, x);
  const f3 t = x - s * p.nrm;
  const float tn = sqrtf(dot(t, t));
  const float sp = (s + mu * tn) * inv;
  const float k = tn > 0.0f ? mu * sp / tn : 0.0f;
  const f3 edge = sp * p.nrm + k * t;
  const bool keep = tn <= mu * s, none = mu * tn <= -s;
  const f3 zero = mk(0.f, 0.f, 0.f);
  const f3 q = keep ? x : (none ? zero : edge);
  return p.in ? q : zero;
}

// the base rows of sum_p J_p^T x_p over the quad: (sum x, sum d x x)
__device__ __forceinline__ void ground_wrench(const ForcePoint (&p)[2], const f3 (&x)[2], f3& lin, f3& ang) {
  lin = quad_sum(x[0] + x[1]);
  ang = quad_sum(cross(p[0].d, x[0]) + cross(p[1].d, x[1]));
}

__global__ void __launch_bounds__(kDynThreads) rex_force_distribution_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                             int rows_total, RexForceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_fd[];
  const DynLane T(ids, rows_total);
  float (*R)[9] = reinterpret_cast<float (*)[9]>(s_fd + T.el * kDynStride);       // the row's tables in LDS
  float (*o)[3] = reinterpret_cast<float (*)[3]>(s_fd + T.el * kDynStride + 9 * REX_NB);
  const int leg = T.leg, row = T.row;

  DynFront F;
  dyn_load_leg(c, state, T.env, T.leg, R, o, F);
  const DynLeg& L = F.L;
  const RexForceDistributionOut& out = a.out;

  // ---- M vdot + h: the base rows yl, yn (on every lane of the quad) and the leg's rows yf, as rex_inverse_dynamics_kernel ----
  f3 yl, yn;
  float yf[3];
  dyn_bias(F, yl, yn, yf);
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
  f3 rl = yl, rn = yn;                                       // r: the wanted base wrench
  if (a.base) {
    const float* w = a.base + (size_t)row * 6;
    rl = rl - mk(w[0], w[1], w[2]);
    rn = rn - mk(w[3], w[4], w[5]);
  }

  // ---- the lane's two toe points, the cones, the step bound ----
  ForcePoint p[2];
  f3 col[2][3];                                              // a_i x (P - o_i)
  const f3 wl = mk(a.w[0], a.w[1], a.w[2]), wa = mk(a.w[3], a.w[4], a.w[5]);
  const float eps = a.eps;
  float trace = 0.0f;
  {
    const f3 tc = toe_centre(F.ofoot, F.z3);
    const bool field = c.n_terrain > 0;
    const bool given = a.stance ? a.stance[(size_t)row * 4 + leg] != 0 : false;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const ToePoint tp = toe_point(F.g, field, tc, F.aw, e);
      p[e].d = tp.P - F.o0;
      p[e].nrm = tp.nrm;
      p[e].in = a.stance ? given : tp.dist < kBreaking;
      const f3 d = p[e].d;
#pragma unroll
      for (int i = 0; i < 3; ++i) col[e][i] = cross(L.a[i], d - L.p[i]);
      const float t = wl.x + wl.y + wl.z + wa.x * (d.y * d.y + d.z * d.z) + wa.y * (d.x * d.x + d.z * d.z) + wa.z * (d.x * d.x + d.y * d.y);
      trace += p[e].in ? t : 0.0f;
    }
  }
  const float mu = a.friction_scale * F.g.mu, inv_cone = 1.0f / (1.0f + mu * mu);
  const float Lip = eps + group_sum<4>(trace);               // trace(W^1/2 A_S A_S^T W^1/2) + eps
  const float sk = sqrtf(Lip / eps), beta = (sk - 1.0f) / (sk + 1.0f), step = 1.0f / Lip;

  // ---- the iteration ----
  f3 f[2] = {mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)}, y[2] = {mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)};
  for (int it = 0; it < a.iterations; ++it) {                // (the same bound in every lane)
    f3 Al, An;
    ground_wrench(p, y, Al, An);
    const f3 ul = mk(wl.x * (Al.x - rl.x), wl.y * (Al.y - rl.y), wl.z * (Al.z - rl.z));
    const f3 ua = mk(wa.x * (An.x - rn.x), wa.y * (An.y - rn.y), wa.z * (An.z - rn.z));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f3 g = ul + cross(ua, p[e].d) + eps * y[e];
      const f3 fn = cone_project(p[e], mu, inv_cone, y[e] - step * g);
      y[e] = fn + beta * (fn - f[e]);
      f[e] = fn;
    }
  }

  // ---- read-out ----
  if (T.live) {
    if (out.toe_force) {
      float* t = out.toe_force + ((size_t)row * 8 + 2 * leg) * 3;
      dput3(t, f[0]); dput3(t + 3, f[1]);
    }
    if (out.tau) {
      float* t = out.tau + (size_t)row * 12 + 3 * leg;
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = yf[i] - (dot(col[0][i], f[0]) + dot(col[1][i], f[1]));
    }
  }
  if (!out.base_residual && !out.residual) return;
  f3 Al, An;
  ground_wrench(p, f, Al, An);
  if (out.base_residual && T.live) {
    float* t = out.base_residual + (size_t)row * 6;
    if (leg == 0) dput3(t, rl - Al);
    else if (leg == 1) dput3(t + 3, rn - An);
  }
  if (!out.residual) return;
  const f3 ul = mk(wl.x * (Al.x - rl.x), wl.y * (Al.y - rl.y), wl.z * (Al.z - rl.z));
  const f3 ua = mk(wa.x * (An.x - rn.x), wa.y * (An.y - rn.y), wa.z * (An.z - rn.z));
  float worst = 0.0f;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const f3 g = ul + cross(ua, p[e].d) + eps * f[e];
    const f3 m = cone_project(p[e], mu, inv_cone, f[e] - step * g) - f[e];
    worst = fmaxf(worst, fmaxf(fabsf(m.x), fmaxf(fabsf(m.y), fabsf(m.z))));
  }
  worst = force_quad_max(worst);
  if (T.live && leg == 0) out.residual[row] = Lip * worst;
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_force_distribution(const RexSim* s, const int32_t* d_ids, int n, const rex::RexForceArgs& a, hipStream_t st) {
  return rex::dyn_launch(rex::rex_force_distribution_kernel, rex::kDynFkBytes, s, d_ids, n, a, st);
}
