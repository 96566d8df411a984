// rex_render_common.h -- the parts of the two render kernels that must agree (rex_render.hip: collision geometry;
// rex_render_mesh.hip: visual meshes): forward kinematics from the SoA state, the camera ray of a pixel, the ray tests of the
// collision primitives, the ground plane / checker / heightfield, sky and Lambert shading, and the whole-dword image stores.
// Both kernels include it, so the ground and sky pixels of the two pictures come from the same code; the depth sensor
// (rex_sense.hip) casts its rays with the same functions.
#pragma once
#include "rex_kernels.h"
#include "rex_render.h"

namespace rex {

namespace {

constexpr int kRenderThreads = 256;
constexpr int kPixPerThread = 4;
constexpr int kTilePixels = kRenderThreads * kPixPerThread;

__device__ __forceinline__ void mat_mul(const float* A, const float* B, float* C) {   // row-major 3x3: C = A B
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// R = rotation by angle a about axis k (0 = x, 1 = y, 2 = z), row-major
__device__ __forceinline__ void axis_rot(int k, float a, float* R) {
  float s, c;
  sincosf(a, &s, &c);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = 0.0f;
  const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
  R[4 * k] = 1.0f;
  R[3 * i1 + i1] = c; R[3 * i1 + i2] = -s;
  R[3 * i2 + i1] = s; R[3 * i2 + i2] = c;
}

// forward kinematics from the SoA state, body by body: world rotation s_R[b] (row-major) and origin s_o[b].  A body needs its
// parent's entry; the four leg chains (bodies 1 + 3 l .. 3 + 3 l) and the arm's chain hang off the base and off nothing else.
// base pose: position, quaternion x y z w
__device__ __forceinline__ void fk_base(const float* __restrict__ state, int n, int env, float* R0, float* o0) {
  const float px = ldw(state, n, REX_S_POS, env), py = ldw(state, n, REX_S_POS + 1, env), pz = ldw(state, n, REX_S_POS + 2, env);
  const float qx = ldw(state, n, REX_S_QUAT, env), qy = ldw(state, n, REX_S_QUAT + 1, env);
  const float qz = ldw(state, n, REX_S_QUAT + 2, env), qw = ldw(state, n, REX_S_QUAT + 3, env);
  R0[0] = 1.0f - 2.0f * (qy * qy + qz * qz); R0[1] = 2.0f * (qx * qy - qz * qw); R0[2] = 2.0f * (qx * qz + qy * qw);
  R0[3] = 2.0f * (qx * qy + qz * qw); R0[4] = 1.0f - 2.0f * (qx * qx + qz * qz); R0[5] = 2.0f * (qy * qz - qx * qw);
  R0[6] = 2.0f * (qx * qz - qy * qw); R0[7] = 2.0f * (qy * qz + qx * qw); R0[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
  o0[0] = px; o0[1] = py; o0[2] = pz;
}

// legs: body b hangs off REX_PARENT[b] through joint b - 1 (joint frames carry no fixed rotation)
__device__ __forceinline__ void fk_leg_body(const float* __restrict__ state, int n, int env, int b, float (*s_R)[9], float (*s_o)[3]) {
  const int p = REX_PARENT[b], j = b - 1;
  const float* Rp = s_R[p];
  float Rq[9];
  axis_rot(REX_JOINT_AXIS[j], ldw(state, n, REX_S_Q + j, env), Rq);
  mat_mul(Rp, Rq, s_R[b]);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    s_o[b][k] = s_o[p][k] + Rp[3 * k] * (float)REX_JOINT_POS[j][0] + Rp[3 * k + 1] * (float)REX_JOINT_POS[j][1] +
                Rp[3 * k + 2] * (float)REX_JOINT_POS[j][2];
}

// arm: body 13 + k hangs off REXA_PARENT[k]: joint frame at REXA_POS[k] with fixed rotation REXA_E0[k], turning about
// REXA_AXIS_SIGN[k] * z by motor 12 + k
__device__ __forceinline__ void fk_arm_body(const float* __restrict__ state, int n, int env, int k, float (*s_R)[9], float (*s_o)[3]) {
  const int b = REX_NB + k, p = REXA_PARENT[k];
  const float* Rp = s_R[p];
  float E[9], J[9], Rq[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = (float)REXA_E0[k][e];
  mat_mul(Rp, E, J);
  axis_rot(2, (float)REXA_AXIS_SIGN[k] * ldw(state, n, REX_S_Q + 12 + k, env), Rq);
  mat_mul(J, Rq, s_R[b]);
#pragma unroll
  for (int e = 0; e < 3; ++e)
    s_o[b][e] = s_o[p][e] + Rp[3 * e] * (float)REXA_POS[k][0] + Rp[3 * e + 1] * (float)REXA_POS[k][1] +
                Rp[3 * e + 2] * (float)REXA_POS[k][2];
}

// forward kinematics of env `env` (one thread): every body b, and the eye of the follow camera in s_eye
template <bool ARM>
__device__ __forceinline__ void render_fk(const float* __restrict__ state, int n, int env, const RenderCam& cam, float (*s_R)[9],
                                          float (*s_o)[3], float* s_eye) {
  fk_base(state, n, env, s_R[0], s_o[0]);
  s_eye[0] = s_o[0][0] + cam.off[0]; s_eye[1] = s_o[0][1] + cam.off[1]; s_eye[2] = s_o[0][2] + cam.off[2];
  for (int b = 1; b < REX_NB; ++b) fk_leg_body(state, n, env, b, s_R, s_o);
  if (ARM) {
    for (int k = 0; k < (ARM ? REXA_NJ : 0); ++k) fk_arm_body(state, n, env, k, s_R, s_o);
  }
}

// the env's heightfield (ground_query's grid and triangulation, heights minus mid): first facet hit in [t0, t1] by a 2-D DDA
// over the cells the ray's ground track crosses.  Outside the grid only the plane is drawn.
__device__ __forceinline__ bool hit_field(const Ground& g, int ny, const float* o, const float* d, float t0, float t1, float& t,
                                          float* n) {
  const HfGeom& q = g.geo;
  const int nx = q.nx;
  const float gx0 = o[0] * q.inv_cx + q.off_x, gy0 = o[1] * q.inv_cy + q.off_y;   // ray in grid (vertex index) coordinates
  const float gdx = d[0] * q.inv_cx, gdy = d[1] * q.inv_cy;
  const float X1 = (float)(nx - 1), Y1 = (float)(ny - 1);
  // clip [t0, t1] to the grid's footprint
  if (gdx != 0.0f) {
    float ta = (0.0f - gx0) / gdx, tb = (X1 - gx0) / gdx;
    if (ta > tb) { const float x = ta; ta = tb; tb = x; }
    t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
  } else if (gx0 < 0.0f || gx0 > X1) return false;
  if (gdy != 0.0f) {
    float ta = (0.0f - gy0) / gdy, tb = (Y1 - gy0) / gdy;
    if (ta > tb) { const float x = ta; ta = tb; tb = x; }
    t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
  } else if (gy0 < 0.0f || gy0 > Y1) return false;
  if (!(t0 <= t1)) return false;
  int i = min(max((int)floorf(gx0 + t0 * gdx), 0), nx - 2);
  int j = min(max((int)floorf(gy0 + t0 * gdy), 0), ny - 2);
  const int si = gdx > 0.0f ? 1 : -1, sj = gdy > 0.0f ? 1 : -1;
  const float idx = gdx != 0.0f ? 1.0f / fabsf(gdx) : INFINITY, idy = gdy != 0.0f ? 1.0f / fabsf(gdy) : INFINITY;
  float tx = gdx != 0.0f ? ((float)(gdx > 0.0f ? i + 1 : i) - gx0) / gdx : INFINITY;
  float ty = gdy != 0.0f ? ((float)(gdy > 0.0f ? j + 1 : j) - gy0) / gdy : INFINITY;
  for (int step = 0; step < nx + ny; ++step) {
    const unsigned base = g.off + (unsigned)(j * nx + i);
    const float h00 = g.h[base] - g.mid, h10 = g.h[base + 1u] - g.mid;
    const float h01 = g.h[base + (unsigned)nx] - g.mid, h11 = g.h[base + (unsigned)nx + 1u] - g.mid;
    const float u0 = gx0 - (float)i, v0 = gy0 - (float)j;
    float best = INFINITY, bn0 = 0.f, bn1 = 0.f;
    // lower triangle (u + v <= 1): z = h00 + u (h10 - h00) + v (h01 - h00)
    {
      const float a = h10 - h00, b = h01 - h00;
      const float den = d[2] - gdx * a - gdy * b;
      if (den != 0.0f) {
        const float ts = (h00 + u0 * a + v0 * b - o[2]) / den;
        const float u = u0 + ts * gdx, v = v0 + ts * gdy;
        if (u >= -1e-6f && v >= -1e-6f && u + v <= 1.0f + 1e-6f && ts >= t0 && ts <= t1 && ts < best) {
          best = ts; bn0 = a * q.inv_cx; bn1 = b * q.inv_cy;
        }
      }
    }
    // upper triangle (u + v > 1): z = h11 + (1 - u) (h01 - h11) + (1 - v) (h10 - h11)
    {
      const float a = h01 - h11, b = h10 - h11;
      const float den = d[2] + gdx * a + gdy * b;
      if (den != 0.0f) {
        const float ts = (h11 + (1.0f - u0) * a + (1.0f - v0) * b - o[2]) / den;
        const float u = u0 + ts * gdx, v = v0 + ts * gdy;
        if (u <= 1.0f + 1e-6f && v <= 1.0f + 1e-6f && u + v >= 1.0f - 1e-6f && ts >= t0 && ts <= t1 && ts < best) {
          best = ts; bn0 = -a * q.inv_cx; bn1 = -b * q.inv_cy;
        }
      }
    }
    if (best < INFINITY) {
      t = best;
      const float inv = 1.0f / sqrtf(bn0 * bn0 + bn1 * bn1 + 1.0f);
      n[0] = -bn0 * inv; n[1] = -bn1 * inv; n[2] = inv;
      return true;
    }
    const float tnext = fminf(tx, ty);
    if (tnext > t1) return false;
    if (tx <= ty) { i += si; tx += idx; if (i < 0 || i > nx - 2) return false; }
    else { j += sj; ty += idy; if (j < 0 || j > ny - 2) return false; }
  }
  return false;
}

// nearest hit t >= near of the ray (o, d) in a primitive's local frame; returns false if none.  n: local normal at the hit
// (not yet turned towards the eye).  Inside a primitive (the near plane cuts it) the exit is the hit, as a rasteriser
// clipped by the near plane would show it.
__device__ __forceinline__ bool hit_box(const float* o, const float* d, const float* h, float tnear, float& t, float* n) {
  float t0 = -INFINITY, t1 = INFINITY;
  int a0 = 0, a1 = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float inv = 1.0f / d[k];
    float ta = (-h[k] - o[k]) * inv, tb = (h[k] - o[k]) * inv;
    if (ta > tb) { const float x = ta; ta = tb; tb = x; }
    if (ta > t0) { t0 = ta; a0 = k; }
    if (tb < t1) { t1 = tb; a1 = k; }
  }
  if (!(t0 <= t1)) return false;
  int a;
  float sgn;
  if (t0 >= tnear) { t = t0; a = a0; sgn = d[a0] > 0.0f ? -1.0f : 1.0f; }
  else if (t1 >= tnear) { t = t1; a = a1; sgn = d[a1] > 0.0f ? 1.0f : -1.0f; }
  else return false;
  n[0] = a == 0 ? sgn : 0.0f; n[1] = a == 1 ? sgn : 0.0f; n[2] = a == 2 ? sgn : 0.0f;
  return true;
}

// cylinder about the local z axis: radius h[0], half length h[2], flat caps
__device__ __forceinline__ bool hit_cyl(const float* o, const float* d, const float* h, float tnear, float& t, float* n) {
  const float r = h[0], hz = h[2];
  float best = INFINITY;
  int which = -1;   // 0 side, 1 cap
  const float a = d[0] * d[0] + d[1] * d[1];
  if (a > 0.0f) {
    // closest approach of the ray to the axis first, then the two roots about it (no cancellation in b^2 - 4ac)
    const float tc = -(o[0] * d[0] + o[1] * d[1]) / a;
    const float px = o[0] + tc * d[0], py = o[1] + tc * d[1];
    const float q = r * r - (px * px + py * py);
    if (q >= 0.0f) {
      const float dt = sqrtf(q / a);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float ts = s == 0 ? tc - dt : tc + dt;
        const float z = o[2] + ts * d[2];
        if (ts >= tnear && ts < best && fabsf(z) <= hz) { best = ts; which = 0; }
      }
    }
  }
  if (d[2] != 0.0f) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float zc = s == 0 ? -hz : hz;
      const float ts = (zc - o[2]) / d[2];
      const float x = o[0] + ts * d[0], y = o[1] + ts * d[1];
      if (ts >= tnear && ts < best && x * x + y * y <= r * r) { best = ts; which = 1 + s; }
    }
  }
  if (which < 0) return false;
  t = best;
  if (which == 0) {
    const float x = o[0] + t * d[0], y = o[1] + t * d[1];
    const float inv = 1.0f / sqrtf(x * x + y * y);
    n[0] = x * inv; n[1] = y * inv; n[2] = 0.0f;
  } else {
    n[0] = 0.0f; n[1] = 0.0f; n[2] = which == 1 ? -1.0f : 1.0f;
  }
  return true;
}

__device__ __forceinline__ uint32_t to_u8(float c) { return (uint32_t)fminf(floorf(255.0f * c + 0.5f), 255.0f); }

// the un-normalised ray of pixel p (row-major, row 0 = the top): its parameter t is the eye-space depth
__device__ __forceinline__ void pixel_ray(long long p, int W, int H, const RenderCam& cam, float* d) {
  const int py = (int)(p / W), px = (int)(p - (long long)py * W);
  const float sx = (2.0f * ((float)px + 0.5f) / (float)W - 1.0f) * cam.tan_x;
  const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)H) * cam.tan_y;
#pragma unroll
  for (int r = 0; r < 3; ++r) d[r] = cam.fwd[r] + sx * cam.right[r] + sy * cam.up[r];
}

// the ground along the ray (eye, d) in front of the robot's hit `best` (INFINITY if nothing): the z = 0 plane, and the
// heightfield above it, bounded by the plane, the far plane and the robot's hit.  -> t of the ground's hit (INFINITY: none),
// its normal in gn
__device__ __forceinline__ float ground_hit(const Ground& g, int ny, const float* eye, const float* d, const RenderCam& cam, float best,
                                            float* gn) {
  const float tplane = d[2] < 0.0f ? -eye[2] / d[2] : INFINITY;
  float tg = INFINITY;
  gn[0] = 0.f; gn[1] = 0.f; gn[2] = 1.f;
  if (tplane >= cam.near_plane) tg = tplane;
  if (g.h) {
    float tf, fn[3];
    if (hit_field(g, ny, eye, d, cam.near_plane, fminf(fminf(tplane, cam.far_plane), best), tf, fn) && tf < tg) {
      tg = tf; gn[0] = fn[0]; gn[1] = fn[1]; gn[2] = fn[2];
    }
  }
  return tg;
}

// the rest of a pixel after the robot: `best` (INFINITY if nothing), its normal bn (world, either side) and albedo alb and
// segment bseg; the ground in front of it, then sky or shading -> packed RGB, and depth / segment where something is hit
__device__ __forceinline__ uint32_t shade_pixel(const Ground& g, int ny, const float* eye, const float* d, const RenderCam& cam,
                                                float best, float* bn, float* alb, int bseg, float& dep, int& sg) {
  float gn[3];
  const float tg = ground_hit(g, ny, eye, d, cam, best, gn);
  if (tg < best) {
    best = tg; bseg = 0;
    bn[0] = gn[0]; bn[1] = gn[1]; bn[2] = gn[2];
    const float hx = eye[0] + tg * d[0], hy = eye[1] + tg * d[1];
    const bool a = (((int)floorf(hx) + (int)floorf(hy)) & 1) == 0;
    alb[0] = a ? kCheckerAR : kCheckerBR; alb[1] = a ? kCheckerAG : kCheckerBG; alb[2] = a ? kCheckerAB : kCheckerBB;
  }
  float cr = kSkyR, cg = kSkyG, cb = kSkyB;
  if (best <= cam.far_plane) {
    if (bn[0] * d[0] + bn[1] * d[1] + bn[2] * d[2] > 0.0f) { bn[0] = -bn[0]; bn[1] = -bn[1]; bn[2] = -bn[2]; }
    const float lam = kAmbient + kDiffuse * fmaxf(0.0f, bn[0] * kLightX + bn[1] * kLightY + bn[2] * kLightZ);
    cr = alb[0] * lam; cg = alb[1] * lam; cb = alb[2] * lam;
    dep = best; sg = bseg;
  }
  return to_u8(cr) | (to_u8(cg) << 8) | (to_u8(cb) << 16);
}

// outputs: whole dwords when the image size and the buffers allow it (vec), else element by element
__device__ __forceinline__ void store_pixels(int vec, int row, long long HW, long long p0, const uint32_t* col, const float* dep,
                                             const int* sg, uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                             int16_t* __restrict__ seg) {
  const size_t img = (size_t)row * (size_t)HW;
  if (vec) {
    uint32_t* o = reinterpret_cast<uint32_t*>(rgb + 3 * (img + (size_t)p0));
    o[0] = col[0] | (col[1] << 24);
    o[1] = (col[1] >> 8) | (col[2] << 16);
    o[2] = (col[2] >> 16) | (col[3] << 8);
    if (depth) *reinterpret_cast<float4*>(depth + img + (size_t)p0) = make_float4(dep[0], dep[1], dep[2], dep[3]);
    if (seg) {
      uint32_t* s2 = reinterpret_cast<uint32_t*>(seg + img + (size_t)p0);
      s2[0] = ((uint32_t)sg[0] & 0xFFFFu) | ((uint32_t)sg[1] << 16);
      s2[1] = ((uint32_t)sg[2] & 0xFFFFu) | ((uint32_t)sg[3] << 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < kPixPerThread; ++e) {
      if (p0 + e >= HW) break;
      const size_t q = img + (size_t)(p0 + e);
      rgb[3 * q] = (uint8_t)(col[e] & 0xFFu); rgb[3 * q + 1] = (uint8_t)((col[e] >> 8) & 0xFFu); rgb[3 * q + 2] = (uint8_t)(col[e] >> 16);
      if (depth) depth[q] = dep[e];
      if (seg) seg[q] = (int16_t)sg[e];
    }
  }
}

}  // namespace
}  // namespace rex
