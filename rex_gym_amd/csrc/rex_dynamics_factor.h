// rex_dynamics_factor.h -- the block elimination of M(q) that the kernels behind the front end of rex_dynamics_leg.h share
// (rex_dynamics_solve.hip, rex_contact_solve.hip): in the order v = (base 6, leg 0, .. leg 3)
//     M = [ Mb  B_0 .. B_3 ;  B_f^T  H_f on the diagonal, zeros between two legs ],
// so, all in registers, one lane per (row, leg), a row's four legs one DPP quad:
//   1. H_f = L D L^T (3 x 3, three reciprocals).
//   2. Y_f = H_f^-1 B_f^T (3 x 6).
//   3. The Schur complement A = Mb - sum_f B_f Y_f: 21 entries, one group_sum<4> each; every lane of the quad holds A.
//   4. A = G G^T (Cholesky of the 6 x 6, on every lane: redundant work, no LDS and no atomics).
//   5. Per right-hand side b = (b_0 [6], b_f [3] per leg):  c = b_0 - sum_f Y_f^T b_f (six group sums),  x_0 = A^-1 c,
//      x_f = H_f^-1 b_f - Y_f x_0.
// Lifted from rex_dynamics_solve_kernel with every expression spelled as it stood there (the build fixes arithmetic by source,
// -ffp-contract=on: rex_dynamics_solve's outputs are bit-identical to those before the lift, profiles/contact_solve.md).
#pragma once
#include "rex_dynamics_leg.h"

namespace rex {

namespace {

// H = L D L^T of a symmetric positive definite 3 x 3, the reciprocals of D kept
struct Ldl3 { float l10, l20, l21, i0, i1, i2; };
__device__ __forceinline__ Ldl3 ldl3(const float (&H)[3][3]) {
  Ldl3 q;
  q.i0 = 1.0f / H[0][0];
  q.l10 = H[1][0] * q.i0;
  q.l20 = H[2][0] * q.i0;
  const float d1 = H[1][1] - q.l10 * H[1][0];
  q.i1 = 1.0f / d1;
  const float t21 = H[2][1] - q.l20 * H[1][0];
  q.l21 = t21 * q.i1;
  const float d2 = H[2][2] - q.l20 * H[2][0] - q.l21 * t21;
  q.i2 = 1.0f / d2;
  return q;
}
__device__ __forceinline__ void ldl3_solve(const Ldl3& q, float b0, float b1, float b2, float (&x)[3]) {
  const float y1 = b1 - q.l10 * b0;
  const float y2 = b2 - q.l20 * b0 - q.l21 * y1;
  x[2] = y2 * q.i2;
  x[1] = y1 * q.i1 - q.l21 * x[2];
  x[0] = b0 * q.i0 - q.l10 * x[1] - q.l20 * x[2];
}

// A = G G^T of a symmetric positive definite 6 x 6 (lower triangle read); G's strict lower triangle and the reciprocals of its diagonal
struct Chol6 { float g[6][6], inv[6]; };
__device__ __forceinline__ void chol6(const float (&A)[6][6], Chol6& q) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= q.g[j][k] * q.g[j][k];
    q.inv[j] = 1.0f / sqrtf(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= q.g[i][k] * q.g[j][k];
      q.g[i][j] = t * q.inv[j];
    }
  }
}
__device__ __forceinline__ void chol6_solve(const Chol6& q, const float (&c)[6], float (&x)[6]) {
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float t = c[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= q.g[i][k] * y[k];
    y[i] = t * q.inv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float t = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= q.g[k][i] * x[k];
    x[i] = t * q.inv[i];
  }
}

// ---- 1.-4. the factors of the lane's row: hq and Y its leg's, aq the quad's ----
struct DynFactor { Ldl3 hq; float Y[3][6]; Chol6 aq; };
__device__ __forceinline__ void dyn_factor(const DynComposite& C, const float (&H)[3][3], DynFactor& Q) {
  Q.hq = ldl3(H);
  const Ldl3& hq = Q.hq;
  float (&Y)[3][6] = Q.Y;                                    // Y_f = H_f^-1 B_f^T: column k solves for row k of B_f
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float y[3];
    if (k < 3) ldl3_solve(hq, comp(C.f[0], k), comp(C.f[1], k), comp(C.f[2], k), y);
    else ldl3_solve(hq, comp(C.nn[0], k - 3), comp(C.nn[1], k - 3), comp(C.nn[2], k - 3), y);
    Y[0][k] = y[0]; Y[1][k] = y[1]; Y[2][k] = y[2];
  }
  const f3 ht = C.ht;
  const s33 It = C.It;
  const float Mb[6][6] = {{C.mt, 0.f, 0.f, 0.f, ht.z, -ht.y}, {0.f, C.mt, 0.f, -ht.z, 0.f, ht.x}, {0.f, 0.f, C.mt, ht.y, -ht.x, 0.f},
                          {0.f, -ht.z, ht.y, It.xx, It.xy, It.xz}, {ht.z, 0.f, -ht.x, It.xy, It.yy, It.yz}, {-ht.y, ht.x, 0.f, It.xz, It.yz, It.zz}};
  float A[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int k = 0; k <= r; ++k) {
      const float br0 = r < 3 ? comp(C.f[0], r) : comp(C.nn[0], r - 3), br1 = r < 3 ? comp(C.f[1], r) : comp(C.nn[1], r - 3),
                  br2 = r < 3 ? comp(C.f[2], r) : comp(C.nn[2], r - 3);
      const float s = br0 * Y[0][k] + br1 * Y[1][k] + br2 * Y[2][k];
      A[r][k] = A[k][r] = Mb[r][k] - group_sum<4>(s);
    }
  chol6(A, Q.aq);
}

// ---- 5. x = M^-1 (b0, bf of every leg); x0 on every lane of the quad, xf the lane's own ----
__device__ __forceinline__ void dyn_msolve(const DynFactor& Q, const float (&b0)[6], const float (&bf)[3], float (&x0)[6], float (&xf)[3]) {
  const float (&Y)[3][6] = Q.Y;
  float cc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float t = Y[0][k] * bf[0] + Y[1][k] * bf[1] + Y[2][k] * bf[2];
    cc[k] = b0[k] - group_sum<4>(t);
  }
  chol6_solve(Q.aq, cc, x0);
  float hs[3];
  ldl3_solve(Q.hq, bf[0], bf[1], bf[2], hs);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float t = hs[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) t -= Y[i][k] * x0[k];
    xf[i] = t;
  }
}

}  // namespace
}  // namespace rex
