// rex_render.hip -- rex_render_kernel (rex_render.h): one workgroup per (env, tile of 1 024 pixels), 256 threads, 4 pixels
// per thread.  Prologue: the env's base pose and joint angles from the SoA state -> forward kinematics through the
// REX_PARENT / REX_JOINT_POS / REX_JOINT_AXIS chain (mark 'arm': the REXA_* chain) -> the primitives of rex_render_gen.h in
// world space, with the eye in each primitive's own frame, in LDS.  Per pixel: one ray against every primitive (slab test
// in the box frame, analytic capped cylinder), against the z = 0 plane and, with a terrain pool, against the env's
// heightfield (2-D DDA over its cells, two triangles per cell split as ground_query splits them); the nearest hit
// between the near and the far plane is shaded.  Reads the state, writes the image buffers only.
#include "rex_render_common.h"
#include "rex_render_gen.h"

namespace rex {

namespace {

// a primitive in world space: its local axes (columns of REX_RENDER_ROT turned by the body), the eye in local
// coordinates, its extents, its albedo and its segment (1 + body)
struct RPrim {
  float ex[3], ey[3], ez[3];
  float eye[3];
  float h[3];
  float rgb[3];
  int seg, kind;
};

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
  if (tid == 0) render_fk<ARM>(state, n, env, cam, s_R, s_o, s_eye);
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
    float d[3];
    pixel_ray(p, W, H, cam, d);
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
    col[e] = shade_pixel(g, ny, eye, d, cam, best, bn, alb, bseg, dep[e], sg[e]);
  }
  store_pixels(vec, row, HW, p0, col, dep, sg, rgb, depth, seg);
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

// the onboard sensors (rex_sense_depth, rex_height_scan): compiled into this object, next to the functions they share with the renderer
#include "rex_sense.hip"
// body and foot kinematics (rex_kinematics): the same forward kinematics once more, read out instead of drawn
#include "rex_kinematics.hip"
// the equations of motion at that pose (rex_dynamics): mass matrix, bias forces, toe Jacobians
#include "rex_dynamics.hip"
// solves with that mass matrix (rex_dynamics_solve, rex_forward_dynamics, rex_apply_impulse): the same front end, M kept in registers
#include "rex_dynamics_solve.hip"
// one substep's contact problem at that state (rex_contact_solve): the same front end and factors, then the step's projected Gauss-Seidel
#include "rex_contact_solve.hip"
// the acceleration level (rex_contact_space, rex_inverse_dynamics): the same front end and factors, the toe points' Delassus matrix
#include "rex_contact_space.hip"
// force distribution (rex_force_distribution): the same front end, then a fixed-length projected-gradient solve over the toe forces
#include "rex_force_distribution.hip"
// candidate rollouts (rex_rollout): the same front end and contact rows, substep after substep on a private copy of the state
#include "rex_rollout.hip"
// the step's epilogue as a readout (rex_outcome): reward, done and observation of given rows; rex_rollout.hip calls its device function
#include "rex_outcome.hip"
