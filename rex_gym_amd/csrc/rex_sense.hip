// rex_sense.hip -- the onboard sensors (rex_sense.h).
//
// rex_sense_depth_kernel: depth only, from a camera mounted on the base.  A sensor image is small (16 x 12 .. 64 x 48) and there is
// one per env and control step, so a workgroup of 256 threads x 4 pixels serves E = max(1, 1 024 / (W H)) consecutive output rows
// (at most kSenseMaxEnvs), whose pixels are one contiguous run of the output; an image of more than 1 024 pixels is tiled as in
// rex_render (E = 1, blockIdx.y the tile).  Prologue, in LDS per env of the workgroup: the base pose (one thread per env), then
// the four leg chains and the arm's chain side by side (one thread per env and chain), then the primitives of rex_render_gen.h in
// world space with the eye in each primitive's own frame (one thread per env and primitive), and the env's eye and view axes: the
// mount turned by the base's rotation.  Per pixel: rex_render's ray (pixel_ray) against every primitive (hit_box, hit_cyl), then
// the ground (ground_hit: the z = 0 plane and the env's heightfield) -- the functions of rex_render_common.h, no second copy.
//
// rex_height_scan_kernel: one thread per (row, point): the point in the base's yaw frame -> world (x, y) -> env_ground and
// ground_query, the contact code's own.
//
// Both read the state and write their output only.  (Built as part of rex_render.hip's object: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_render_common.h"
#include "rex_render_gen.h"
#include "rex_sense.h"

namespace rex {

namespace {

// a primitive in world space, as the ray test needs it: its local axes, the eye in local coordinates, its extents, its kind
struct alignas(16) SPrim {
  float ex[3], ey[3], ez[3];
  float eye[3];
  float h[3];
  int kind;
};
static_assert(sizeof(SPrim) == 64, "four 16-byte LDS reads per primitive");

// what the pixels of one env share: the camera in world axes (cam.off: the eye relative to the base), the eye, the env's index
struct alignas(16) SEnv {
  RenderCam cam;
  float eye[3];
  int env;
};

template <bool ARM>
struct SenseEnvLds {
  static constexpr int NB = REX_NB + (ARM ? REXA_NJ : 0);
  static constexpr int NP = ARM ? REX_RENDER_NPRIM_ARM : REX_RENDER_NPRIM_BASE;
  SEnv e;
  SPrim p[NP];
  float R[NB][9], o[NB][3];
};
// LDS bytes per env: an odd number of 16-byte slots, so that lanes of one wave that read the same entry of neighbouring envs'
// tables (a wave spans several envs when the images are small) fall on different banks
template <bool ARM>
constexpr int kSenseStride = (int)(((sizeof(SenseEnvLds<ARM>) + 15) / 16) | 1) * 16;

template <bool ARM>
__global__ void __launch_bounds__(kRenderThreads) rex_sense_depth_kernel(DevCfg c, const float* __restrict__ state, SenseMount m,
                                                                         const int32_t* __restrict__ ids, int rows_total, int epb, int W,
                                                                         int H, int vec, float* __restrict__ depth) {
  using L = SenseEnvLds<ARM>;
  constexpr int NM = ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;
  constexpr int NP = L::NP;
  constexpr int NCHAIN = ARM ? 5 : 4;
  extern __shared__ __attribute__((aligned(16))) char s_sense[];
  const int n = c.n;
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * epb;                  // first output row of this workgroup
  const int rows = min(epb, rows_total - row0);       // >= 1: the grid has ceil(rows_total / epb) workgroups
  auto lds = [&](int r) -> L& { return *reinterpret_cast<L*>(s_sense + (size_t)r * kSenseStride<ARM>); };

  // base pose, eye and view axes: one thread per env
  if (tid < rows) {
    L& Q = lds(tid);
    const int env = ids ? ids[row0 + tid] : row0 + tid;   // the state's env index (checked on the host)
    fk_base(state, n, env, Q.R[0], Q.o[0]);
    const float* R0 = Q.R[0];
    SEnv& E = Q.e;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      E.cam.off[r] = R0[3 * r] * m.pos[0] + R0[3 * r + 1] * m.pos[1] + R0[3 * r + 2] * m.pos[2];
      E.cam.fwd[r] = R0[3 * r] * m.fwd[0] + R0[3 * r + 1] * m.fwd[1] + R0[3 * r + 2] * m.fwd[2];
      E.cam.right[r] = R0[3 * r] * m.right[0] + R0[3 * r + 1] * m.right[1] + R0[3 * r + 2] * m.right[2];
      E.cam.up[r] = R0[3 * r] * m.up[0] + R0[3 * r + 1] * m.up[1] + R0[3 * r + 2] * m.up[2];
      E.eye[r] = Q.o[0][r] + E.cam.off[r];
    }
    E.cam.tan_x = m.tan_x; E.cam.tan_y = m.tan_y; E.cam.near_plane = m.near_plane; E.cam.far_plane = m.far_plane;
    E.env = env;
  }
  if (m.see_robot) {   // (the same in every thread)
    __syncthreads();
    // the chains hang off the base and off nothing else: one thread per (env, chain)
    if (tid < rows * NCHAIN) {
      const int r = tid / NCHAIN, ch = tid - r * NCHAIN;
      L& Q = lds(r);
      const int env = Q.e.env;
      if (ch < 4) {
        for (int b = 1 + 3 * ch; b < 4 + 3 * ch; ++b) fk_leg_body(state, n, env, b, Q.R, Q.o);
      } else {
        for (int k = 0; k < (ARM ? REXA_NJ : 0); ++k) fk_arm_body(state, n, env, k, Q.R, Q.o);
      }
    }
    __syncthreads();
    // the primitives of every env in world space, the eye in each one's frame
    for (int i = tid; i < rows * NP; i += kRenderThreads) {
      const int r = i / NP, k = i - r * NP, b = REX_RENDER_BODY[k];
      L& Q = lds(r);
      const float* Rb = Q.R[b];
      SPrim& P = Q.p[k];
      float c3[3], ax[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        c3[a] = Q.o[b][a] + Rb[3 * a] * (float)REX_RENDER_POS[k][0] + Rb[3 * a + 1] * (float)REX_RENDER_POS[k][1] +
                Rb[3 * a + 2] * (float)REX_RENDER_POS[k][2];
#pragma unroll
        for (int q = 0; q < 3; ++q)   // local axis q = column q of REX_RENDER_ROT, in world
          ax[q][a] = Rb[3 * a] * (float)REX_RENDER_ROT[k][q] + Rb[3 * a + 1] * (float)REX_RENDER_ROT[k][3 + q] +
                     Rb[3 * a + 2] * (float)REX_RENDER_ROT[k][6 + q];
      }
      const float rx = Q.e.eye[0] - c3[0], ry = Q.e.eye[1] - c3[1], rz = Q.e.eye[2] - c3[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        P.ex[a] = ax[0][a]; P.ey[a] = ax[1][a]; P.ez[a] = ax[2][a];
        P.h[a] = (float)REX_RENDER_EXT[k][a];
        P.eye[a] = rx * ax[a][0] + ry * ax[a][1] + rz * ax[a][2];
      }
      P.kind = REX_RENDER_KIND[k];
    }
  }
  __syncthreads();

  // this thread's 4 consecutive floats of the workgroup's run of rows * W * H pixels (they may lie in two images when
  // W H % 4 != 0, and past the end of the last one)
  const int HW = W * H;                              // (n * W * H < 2^29, checked on the host)
  const int total = rows * HW;
  const int q0 = (blockIdx.y * kRenderThreads + tid) * kPixPerThread;
  if (q0 >= total) return;
  const int ny = c.n_terrain > 0 ? c.hf_stride / c.geo.nx : 0;
  int r = q0 / HW, p = q0 - r * HW;
  int r_ground = -1;
  Ground g{};
  float dep[kPixPerThread];
#pragma unroll
  for (int e = 0; e < kPixPerThread; ++e) {
    dep[e] = m.far_plane;
    if (q0 + e >= total) continue;
    const L& Q = lds(r);
    const SEnv& E = Q.e;
    if (c.n_terrain > 0 && r != r_ground) {
      g = env_ground(c, E.env, c.env_index_base + E.env, (int)ldi(state, n, Lay<NM>::EPISODE, E.env));
      r_ground = r;
    }
    float d[3];
    pixel_ray(p, W, H, E.cam, d);
    float best = INFINITY;
    if (m.see_robot) {
#pragma unroll 1
      for (int k = 0; k < NP; ++k) {   // (a loop, not unrolled, as in rex_render)
        const SPrim& P = Q.p[k];
        const float dl[3] = {d[0] * P.ex[0] + d[1] * P.ex[1] + d[2] * P.ex[2], d[0] * P.ey[0] + d[1] * P.ey[1] + d[2] * P.ey[2],
                             d[0] * P.ez[0] + d[1] * P.ez[1] + d[2] * P.ez[2]};
        float t, nl[3];
        const bool hit = P.kind == REX_RENDER_BOX ? hit_box(P.eye, dl, P.h, m.near_plane, t, nl) : hit_cyl(P.eye, dl, P.h, m.near_plane, t, nl);
        if (hit && t < best) best = t;
      }
    }
    const float eye[3] = {E.eye[0], E.eye[1], E.eye[2]};
    float gn[3];
    const float tg = ground_hit(g, ny, eye, d, E.cam, best, gn);
    if (tg < best) best = tg;
    if (best <= m.far_plane) dep[e] = best;
    if (++p == HW) { p = 0; ++r; }
  }
  float* out = depth + ((size_t)row0 * (size_t)HW + (size_t)q0);
  if (vec) {   // W H % 4 == 0 and a 16-byte aligned buffer: the 4 pixels lie in one image, inside the run
    *reinterpret_cast<float4*>(out) = make_float4(dep[0], dep[1], dep[2], dep[3]);
  } else {
#pragma unroll
    for (int e = 0; e < kPixPerThread; ++e)
      if (q0 + e < total) out[e] = dep[e];
  }
}

template <bool ARM>
__global__ void __launch_bounds__(kRenderThreads) rex_height_scan_kernel(DevCfg c, const float* __restrict__ state,
                                                                         const float* __restrict__ points, int K, int relative,
                                                                         const int32_t* __restrict__ ids, int rows_total,
                                                                         float* __restrict__ out) {
  constexpr int NM = ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;
  const int idx = blockIdx.x * kRenderThreads + threadIdx.x;   // (rows * K < 2^31, checked on the host)
  if (idx >= rows_total * K) return;
  const int n = c.n;
  const int row = idx / K, k = idx - row * K;
  const int env = ids ? ids[row] : row;
  const float px = ldw(state, n, REX_S_POS, env), py = ldw(state, n, REX_S_POS + 1, env), pz = ldw(state, n, REX_S_POS + 2, env);
  const float qx = ldw(state, n, REX_S_QUAT, env), qy = ldw(state, n, REX_S_QUAT + 1, env);
  const float qz = ldw(state, n, REX_S_QUAT + 2, env), qw = ldw(state, n, REX_S_QUAT + 3, env);
  // yaw = atan2(R10, R00) of the base rotation: its cosine and sine are (R00, R10) normalised; (1, 0) when both vanish
  const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r10 = 2.0f * (qx * qy + qz * qw);
  const float len = sqrtf(r00 * r00 + r10 * r10);
  const float cy = len > 0.0f ? r00 / len : 1.0f, sy = len > 0.0f ? r10 / len : 0.0f;
  const float ux = points[2 * k], uy = points[2 * k + 1];
  const float x = px + (cy * ux - sy * uy), y = py + (sy * ux + cy * uy);
  float h = 0.0f;
  if (c.n_terrain > 0) {
    // the heightfield has the extent of its grid, as the renderer draws it (hit_field) and as Bullet's shape has it: beside it
    // lies the plane.  (ground_query alone would hold the border's height on, which the contact code never needs: the
    // robots do not leave the field.)
    const float gx = x * c.geo.inv_cx + c.geo.off_x, gy = y * c.geo.inv_cy + c.geo.off_y;
    const int ny = c.hf_stride / c.geo.nx;
    if (gx >= 0.0f && gx <= (float)(c.geo.nx - 1) && gy >= 0.0f && gy <= (float)(ny - 1)) {
      const Ground g = env_ground(c, env, c.env_index_base + env, (int)ldi(state, n, Lay<NM>::EPISODE, env));
      f3 nrm;
      ground_query(g, x, y, h, nrm);
    }
  }
  out[idx] = relative ? pz - h : h;
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_sense_depth(const RexSim* s, const rex::SenseMount& m, const int32_t* d_ids, int n, int width, int height,
                                  float* d_depth, hipStream_t st) {
  const int hw = width * height;
  const int epb = hw >= rex::kTilePixels ? 1 : (rex::kTilePixels / hw < rex::kSenseMaxEnvs ? rex::kTilePixels / hw : rex::kSenseMaxEnvs);
  const int tiles = epb > 1 ? 1 : (hw + rex::kTilePixels - 1) / rex::kTilePixels;
  const int blocks = (n + epb - 1) / epb;
  // whole 16-byte stores: 4 pixels of a thread never straddle two images and the buffer is aligned
  const int vec = (hw % 4 == 0) && ((uintptr_t)d_depth % 16 == 0);
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_sense_depth_kernel<true>, dim3(blocks, tiles), dim3(rex::kRenderThreads),
                       (size_t)epb * rex::kSenseStride<true>, st, s->dev, s->d_state, m, d_ids, n, epb, width, height, vec, d_depth);
  else
    hipLaunchKernelGGL(rex::rex_sense_depth_kernel<false>, dim3(blocks, tiles), dim3(rex::kRenderThreads),
                       (size_t)epb * rex::kSenseStride<false>, st, s->dev, s->d_state, m, d_ids, n, epb, width, height, vec, d_depth);
  return hipGetLastError();
}

hipError_t rex_launch_height_scan(const RexSim* s, const float* d_points, int K, int relative, const int32_t* d_ids, int n, float* d_out,
                                  hipStream_t st) {
  const int blocks = (int)(((long long)n * K + rex::kRenderThreads - 1) / rex::kRenderThreads);
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_height_scan_kernel<true>, dim3(blocks), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, d_points, K,
                       relative, d_ids, n, d_out);
  else
    hipLaunchKernelGGL(rex::rex_height_scan_kernel<false>, dim3(blocks), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, d_points, K,
                       relative, d_ids, n, d_out);
  return hipGetLastError();
}
