// rex_render.hip -- rex_render_kernel (rex_render.h): one workgroup per (env, tile of 1 024 pixels), 256 threads, 4 pixels
// per thread.  Prologue: the env's base pose and joint angles from the SoA state -> forward kinematics through the
// REX_PARENT / REX_JOINT_POS / REX_JOINT_AXIS chain (mark 'arm': the REXA_* chain) -> the primitives of rex_render_gen.h in
// world space, with the eye in each primitive's own frame, in LDS.  Per pixel: one ray against every primitive (slab test
// in the box frame, analytic capped cylinder), against the z = 0 plane and, with a terrain pool, against the env's
// heightfield (2-D DDA over its cells, two triangles per cell split as ground_query splits them); the nearest hit
// between the near and the far plane is shaded.  Reads the state, writes the image buffers only.
#include "rex_kernels.h"
#include "rex_render.h"
#include "rex_render_gen.h"

namespace rex {

namespace {

constexpr int kRenderThreads = 256;
constexpr int kPixPerThread = 4;
constexpr int kTilePixels = kRenderThreads * kPixPerThread;

// a primitive in world space: its local axes (columns of REX_RENDER_ROT turned by the body), the eye in local
// coordinates, its extents, its albedo and its segment (1 + body)
struct RPrim {
  float ex[3], ey[3], ez[3];
  float eye[3];
  float h[3];
  float rgb[3];
  int seg, kind;
};

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

__device__ __forceinline__ uint32_t to_u8(float c) { return (uint32_t)fminf(floorf(255.0f * c + 0.5f), 255.0f); }

template <bool ARM>
__global__ void __launch_bounds__(kRenderThreads) rex_render_kernel(DevCfg c, const float* __restrict__ state, RenderCam cam,
                                                                    const int32_t* __restrict__ ids, int W, int H, int vec,
                                                                    uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                                    int16_t* __restrict__ seg) {
  constexpr int NM = ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;
  constexpr int NB = REX_NB + (ARM ? REXA_NJ : 0);
  constexpr int NP = ARM ? REX_RENDER_NPRIM_ARM : REX_RENDER_NPRIM_BASE;
  __shared__ float s_R[NB][9], s_o[NB][3];
  __shared__ RPrim s_p[NP];
  __shared__ float s_eye[3];
  const int row = blockIdx.x;            // output row
  const int env = ids[row];              // the state's env index (checked on the host)
  const int n = c.n;
  const int tid = threadIdx.x;
  if (tid == 0) {
    // base pose: position, quaternion x y z w
    const float px = ldw(state, n, REX_S_POS, env), py = ldw(state, n, REX_S_POS + 1, env), pz = ldw(state, n, REX_S_POS + 2, env);
    const float qx = ldw(state, n, REX_S_QUAT, env), qy = ldw(state, n, REX_S_QUAT + 1, env);
    const float qz = ldw(state, n, REX_S_QUAT + 2, env), qw = ldw(state, n, REX_S_QUAT + 3, env);
    float* R0 = s_R[0];
    R0[0] = 1.0f - 2.0f * (qy * qy + qz * qz); R0[1] = 2.0f * (qx * qy - qz * qw); R0[2] = 2.0f * (qx * qz + qy * qw);
    R0[3] = 2.0f * (qx * qy + qz * qw); R0[4] = 1.0f - 2.0f * (qx * qx + qz * qz); R0[5] = 2.0f * (qy * qz - qx * qw);
    R0[6] = 2.0f * (qx * qz - qy * qw); R0[7] = 2.0f * (qy * qz + qx * qw); R0[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
    s_o[0][0] = px; s_o[0][1] = py; s_o[0][2] = pz;
    s_eye[0] = px + cam.off[0]; s_eye[1] = py + cam.off[1]; s_eye[2] = pz + cam.off[2];
    // legs: body b hangs off REX_PARENT[b] through joint b - 1 (joint frames carry no fixed rotation)
    for (int b = 1; b < REX_NB; ++b) {
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
    if (ARM) {
      for (int k = 0; k < (ARM ? REXA_NJ : 0); ++k) {
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
    }
  }
  __syncthreads();
  if (tid < NP) {
    const int k = tid, b = REX_RENDER_BODY[k];
    const float* Rb = s_R[b];
    RPrim& P = s_p[k];
    float c3[3], ax[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      c3[r] = s_o[b][r] + Rb[3 * r] * (float)REX_RENDER_POS[k][0] + Rb[3 * r + 1] * (float)REX_RENDER_POS[k][1] +
              Rb[3 * r + 2] * (float)REX_RENDER_POS[k][2];
#pragma unroll
      for (int a = 0; a < 3; ++a)   // local axis a = column a of REX_RENDER_ROT, in world
        ax[a][r] = Rb[3 * r] * (float)REX_RENDER_ROT[k][a] + Rb[3 * r + 1] * (float)REX_RENDER_ROT[k][3 + a] +
                   Rb[3 * r + 2] * (float)REX_RENDER_ROT[k][6 + a];
    }
    const float rx = s_eye[0] - c3[0], ry = s_eye[1] - c3[1], rz = s_eye[2] - c3[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      P.ex[r] = ax[0][r]; P.ey[r] = ax[1][r]; P.ez[r] = ax[2][r];
      P.h[r] = (float)REX_RENDER_EXT[k][r]; P.rgb[r] = (float)REX_RENDER_RGB[k][r];
      P.eye[r] = rx * ax[r][0] + ry * ax[r][1] + rz * ax[r][2];
    }
    P.seg = 1 + b;
    P.kind = REX_RENDER_KIND[k];
  }
  __syncthreads();

  Ground g{};
  int ny = 0;
  if (c.n_terrain > 0) {
    g = env_ground(c, env, c.env_index_base + env, (int)ldi(state, n, Lay<NM>::EPISODE, env));
    ny = c.hf_stride / c.geo.nx;
  }
  const float eye[3] = {s_eye[0], s_eye[1], s_eye[2]};
  const long long HW = (long long)W * H;
  const long long p0 = ((long long)blockIdx.y * kRenderThreads + tid) * kPixPerThread;
  if (p0 >= HW) return;
  uint32_t col[kPixPerThread];
  float dep[kPixPerThread];
  int sg[kPixPerThread];
#pragma unroll
  for (int e = 0; e < kPixPerThread; ++e) {
    const long long p = p0 + e;
    col[e] = 0u; dep[e] = cam.far_plane; sg[e] = -1;
    if (p >= HW) continue;
    const int py = (int)(p / W), px = (int)(p - (long long)py * W);
    const float sx = (2.0f * ((float)px + 0.5f) / (float)W - 1.0f) * cam.tan_x;
    const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)H) * cam.tan_y;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = cam.fwd[r] + sx * cam.right[r] + sy * cam.up[r];
    float best = INFINITY, bn[3] = {0.f, 0.f, 1.f}, alb[3] = {0.f, 0.f, 0.f};
    int bseg = -1, bk = -1;
    float bnl[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k = 0; k < NP; ++k) {   // (a loop, not unrolled: the primitives are wave-uniform LDS reads, and 25 inlined tests cost registers)
      const RPrim& P = s_p[k];
      const float dl[3] = {d[0] * P.ex[0] + d[1] * P.ex[1] + d[2] * P.ex[2], d[0] * P.ey[0] + d[1] * P.ey[1] + d[2] * P.ey[2],
                           d[0] * P.ez[0] + d[1] * P.ez[1] + d[2] * P.ez[2]};
      float t, nl[3];
      const bool hit = P.kind == REX_RENDER_BOX ? hit_box(P.eye, dl, P.h, cam.near_plane, t, nl)
                                                            : hit_cyl(P.eye, dl, P.h, cam.near_plane, t, nl);
      if (hit && t < best) { best = t; bk = k; bnl[0] = nl[0]; bnl[1] = nl[1]; bnl[2] = nl[2]; }
    }
    if (bk >= 0) {
      const RPrim& P = s_p[bk];
#pragma unroll
      for (int r = 0; r < 3; ++r) { bn[r] = bnl[0] * P.ex[r] + bnl[1] * P.ey[r] + bnl[2] * P.ez[r]; alb[r] = P.rgb[r]; }
      bseg = P.seg;
    }
    // ground: the z = 0 plane, and the heightfield above it
    const float tplane = d[2] < 0.0f ? -eye[2] / d[2] : INFINITY;
    float tg = INFINITY, gn[3] = {0.f, 0.f, 1.f};
    if (tplane >= cam.near_plane) tg = tplane;
    if (g.h) {
      float tf, fn[3];
      if (hit_field(g, ny, eye, d, cam.near_plane, fminf(fminf(tplane, cam.far_plane), best), tf, fn) && tf < tg) {
        tg = tf; gn[0] = fn[0]; gn[1] = fn[1]; gn[2] = fn[2];
      }
    }
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
      dep[e] = best; sg[e] = bseg;
    }
    col[e] = to_u8(cr) | (to_u8(cg) << 8) | (to_u8(cb) << 16);
  }
  // outputs: whole dwords when the image size and the buffers allow it (vec), else element by element
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

hipError_t rex_launch_render(const RexSim* s, const rex::RenderCam& cam, const int32_t* d_ids, int n, int width, int height,
                             uint8_t* d_rgb, float* d_depth, int16_t* d_seg, hipStream_t st) {
  const long long hw = (long long)width * height;
  const int tiles = (int)((hw + rex::kTilePixels - 1) / rex::kTilePixels);
  // whole-dword stores: 4 pixels of a thread never straddle two images and every buffer is aligned for its vector width
  const int vec = (hw % 4 == 0) && ((uintptr_t)d_rgb % 4 == 0) && ((uintptr_t)d_depth % 16 == 0) && ((uintptr_t)d_seg % 4 == 0);
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_render_kernel<true>, dim3(n, tiles), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, cam, d_ids,
                       width, height, vec, d_rgb, d_depth, d_seg);
  else
    hipLaunchKernelGGL(rex::rex_render_kernel<false>, dim3(n, tiles), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, cam, d_ids,
                       width, height, vec, d_rgb, d_depth, d_seg);
  return hipGetLastError();
}
