// rex_render_mesh.hip -- rex_render_mesh_kernel (rex_render.h): the same picture as rex_render_kernel, drawn from the robot's
// visual meshes (rex_visual_gen.h + the BVHs of rex_render_set_visuals) instead of its collision primitives.  Same grid: one
// workgroup per (env, tile of 1 024 pixels), 256 threads, 4 consecutive pixels per thread.
// Prologue: forward kinematics (rex_render_common.h) -> every visual instance in LDS: its mesh axes in world, the eye in mesh
// coordinates, its world AABB (from the mesh's root box), colour, segment and root node.  Per pixel: the ray against each
// instance's world AABB (skipped when its entry is not nearer than the best hit so far), then, in mesh coordinates with the
// direction left un-normalised (so t stays the eye-space depth and hits of different instances compare directly), a BVH
// traversal that visits the nearer child first with a per-thread stack in LDS, and two-sided ray-triangle tests (CAD
// winding is not reliable).  The hit is shaded flat with its geometric normal; ground, sky and stores are the collision
// kernel's code.  Reads the state and the visual buffers, writes the image buffers only, uses no scratch.
#include "rex_render_common.h"
#include "rex_visual_gen.h"

namespace rex {

namespace {

// a visual instance in world space: mesh axis a in world = ax[a] (columns of the body rotation times REX_VIS_ROT), the eye
// in mesh coordinates, the world AABB, albedo, segment (1 + body) and root node (-1: an empty mesh, never hit)
struct MInst {
  float ax[3][3];
  float eye[3];
  float lo[3], hi[3];
  float rgb[3];
  int seg, root;
};

// slab test of the ray (o, inverse direction id) against [lo, hi]: entry / exit parameters
__device__ __forceinline__ void slab(const float* o, const float* id, float lx, float ly, float lz, float hx, float hy, float hz,
                                     float& t0, float& t1) {
  const float ax = (lx - o[0]) * id[0], bx = (hx - o[0]) * id[0];
  const float ay = (ly - o[1]) * id[1], by = (hy - o[1]) * id[1];
  const float az = (lz - o[2]) * id[2], bz = (hz - o[2]) * id[2];
  t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
}

template <bool ARM>
__global__ void __launch_bounds__(kRenderThreads) rex_render_mesh_kernel(DevCfg c, const float* __restrict__ state, RenderCam cam,
                                                                         const int32_t* __restrict__ ids, int W, int H, int vec,
                                                                         const float4* __restrict__ nodes, const float* __restrict__ tris,
                                                                         const int32_t* __restrict__ vroot, const float* __restrict__ vbox,
                                                                         uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                                         int16_t* __restrict__ seg) {
  constexpr int NM = ARM ? REX_NUM_MOTORS_ARM : REX_NUM_MOTORS;
  constexpr int NB = REX_NB + (ARM ? REXA_NJ : 0);
  constexpr int NI = ARM ? REX_VIS_N_ARM : REX_VIS_N_BASE;
  __shared__ float s_R[NB][9], s_o[NB][3];
  __shared__ MInst s_i[NI];
  __shared__ float s_eye[3];
  __shared__ int s_stack[kMeshStack][kRenderThreads];   // entry k of thread t at [k][t]: consecutive lanes, distinct banks
  const int row = blockIdx.x;
  const int env = ids[row];
  const int n = c.n;
  const int tid = threadIdx.x;
  if (tid == 0) render_fk<ARM>(state, n, env, cam, s_R, s_o, s_eye);
  __syncthreads();
  if (tid < NI) {
    const int k = tid, b = REX_VIS_BODY[k];
    const float* Rb = s_R[b];
    MInst& I = s_i[k];
    float t[3], R[3][3];   // mesh frame in world: origin t, rotation R (row-major)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      t[r] = s_o[b][r] + Rb[3 * r] * (float)REX_VIS_POS[k][0] + Rb[3 * r + 1] * (float)REX_VIS_POS[k][1] +
             Rb[3 * r + 2] * (float)REX_VIS_POS[k][2];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        R[r][a] = Rb[3 * r] * (float)REX_VIS_ROT[k][a] + Rb[3 * r + 1] * (float)REX_VIS_ROT[k][3 + a] +
                  Rb[3 * r + 2] * (float)REX_VIS_ROT[k][6 + a];
    }
    const float rx = s_eye[0] - t[0], ry = s_eye[1] - t[1], rz = s_eye[2] - t[2];
    const float* bx = vbox + 6 * k;   // mesh-frame root box lo[3], hi[3]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      I.ax[a][0] = R[0][a]; I.ax[a][1] = R[1][a]; I.ax[a][2] = R[2][a];
      I.eye[a] = rx * R[0][a] + ry * R[1][a] + rz * R[2][a];
      I.rgb[a] = (float)REX_VIS_RGB[k][a];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {   // world AABB of the rotated root box: centre +- |R| half extents
      float cw = t[r], hw = 0.0f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        cw += R[r][a] * 0.5f * (bx[a] + bx[3 + a]);
        hw += fabsf(R[r][a]) * 0.5f * (bx[3 + a] - bx[a]);
      }
      hw += 1e-5f * (fabsf(cw) + hw) + 1e-6f;   // float rounding of the map: grow, never shrink
      I.lo[r] = cw - hw; I.hi[r] = cw + hw;
    }
    I.seg = 1 + b;
    I.root = vroot[k];
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
  int* stack = &s_stack[0][tid];
  uint32_t col[kPixPerThread];
  float dep[kPixPerThread];
  int sg[kPixPerThread];
#pragma unroll 1
  for (int e = 0; e < kPixPerThread; ++e) {
    const long long p = p0 + e;
    col[e] = 0u; dep[e] = cam.far_plane; sg[e] = -1;
    if (p >= HW) continue;
    float d[3];
    pixel_ray(p, W, H, cam, d);
    const float idw[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    const float tnear = cam.near_plane;
    float best = INFINITY;
    int bi = -1, bt = 0;
#pragma unroll 1
    for (int k = 0; k < NI; ++k) {
      const MInst& I = s_i[k];
      if (I.root < 0) continue;
      float ta, tb;
      slab(eye, idw, I.lo[0], I.lo[1], I.lo[2], I.hi[0], I.hi[1], I.hi[2], ta, tb);
      if (!(ta <= tb) || tb < tnear || ta >= best) continue;
      const float o[3] = {I.eye[0], I.eye[1], I.eye[2]};
      const float dm[3] = {d[0] * I.ax[0][0] + d[1] * I.ax[0][1] + d[2] * I.ax[0][2],
                           d[0] * I.ax[1][0] + d[1] * I.ax[1][1] + d[2] * I.ax[1][2],
                           d[0] * I.ax[2][0] + d[1] * I.ax[2][1] + d[2] * I.ax[2][2]};
      const float id[3] = {1.0f / dm[0], 1.0f / dm[1], 1.0f / dm[2]};
      int cur = I.root, sp = 0;
      while (true) {
        if (cur >= 0) {   // inner node: both children's boxes, nearer child first
          const float4* nd = nodes + 4 * (size_t)cur;
          const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
          float a0, a1, b0, b1;
          slab(o, id, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, a0, a1);
          slab(o, id, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, b0, b1);
          const bool h0 = a0 <= a1 && a1 >= tnear && a0 < best;
          const bool h1 = b0 <= b1 && b1 >= tnear && b0 < best;
          const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
          if (h0 && h1) {
            const bool first0 = a0 <= b0;
            if (sp < kMeshStack) { stack[sp * kRenderThreads] = first0 ? c1 : c0; ++sp; }
            cur = first0 ? c0 : c1;
            continue;
          }
          if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
        } else {          // leaf: ~cur = start << 3 | (count - 1)
          const int v = ~cur, start = v >> 3, cnt = (v & 7) + 1;
          for (int i = start; i < start + cnt; ++i) {
            const float* T = tris + 9 * (size_t)i;
            const float e1[3] = {T[3], T[4], T[5]}, e2[3] = {T[6], T[7], T[8]};
            const float pv[3] = {dm[1] * e2[2] - dm[2] * e2[1], dm[2] * e2[0] - dm[0] * e2[2], dm[0] * e2[1] - dm[1] * e2[0]};
            const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
            if (det == 0.0f) continue;   // two-sided: either sign of det is a front face
            const float inv = 1.0f / det;
            const float s[3] = {o[0] - T[0], o[1] - T[1], o[2] - T[2]};
            const float u = (s[0] * pv[0] + s[1] * pv[1] + s[2] * pv[2]) * inv;
            if (!(u >= 0.0f && u <= 1.0f)) continue;
            const float qv[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
            const float w = (dm[0] * qv[0] + dm[1] * qv[1] + dm[2] * qv[2]) * inv;
            if (!(w >= 0.0f && u + w <= 1.0f)) continue;
            const float tt = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
            if (tt >= tnear && tt < best) { best = tt; bi = k; bt = i; }
          }
        }
        if (sp == 0) break;
        --sp;
        cur = stack[sp * kRenderThreads];
      }
    }
    float bn[3] = {0.f, 0.f, 1.f}, alb[3] = {0.f, 0.f, 0.f};
    int bseg = -1;
    if (bi >= 0) {   // flat shading: the triangle's geometric normal e1 x e2, in world (shade_pixel turns it to the eye)
      const MInst& I = s_i[bi];
      const float* T = tris + 9 * (size_t)bt;
      const float nm[3] = {T[4] * T[8] - T[5] * T[7], T[5] * T[6] - T[3] * T[8], T[3] * T[7] - T[4] * T[6]};
      float nw[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) nw[r] = nm[0] * I.ax[0][r] + nm[1] * I.ax[1][r] + nm[2] * I.ax[2][r];
      const float len = sqrtf(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]);
      const float il = len > 0.0f ? 1.0f / len : 0.0f;
#pragma unroll
      for (int r = 0; r < 3; ++r) { bn[r] = nw[r] * il; alb[r] = I.rgb[r]; }
      bseg = I.seg;
    }
    col[e] = shade_pixel(g, ny, eye, d, cam, best, bn, alb, bseg, dep[e], sg[e]);
  }
  store_pixels(vec, row, HW, p0, col, dep, sg, rgb, depth, seg);
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_render_mesh(const RexSim* s, const rex::RenderCam& cam, const int32_t* d_ids, int n, int width, int height,
                                  uint8_t* d_rgb, float* d_depth, int16_t* d_seg, hipStream_t st) {
  const long long hw = (long long)width * height;
  const int tiles = (int)((hw + rex::kTilePixels - 1) / rex::kTilePixels);
  const int vec = (hw % 4 == 0) && ((uintptr_t)d_rgb % 4 == 0) && ((uintptr_t)d_depth % 16 == 0) && ((uintptr_t)d_seg % 4 == 0);
  const float4* nodes = reinterpret_cast<const float4*>(s->d_vis_nodes);
  if (s->cfg.mark == REX_MARK_ARM)
    hipLaunchKernelGGL(rex::rex_render_mesh_kernel<true>, dim3(n, tiles), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, cam,
                       d_ids, width, height, vec, nodes, s->d_vis_tris, s->d_vis_root, s->d_vis_box, d_rgb, d_depth, d_seg);
  else
    hipLaunchKernelGGL(rex::rex_render_mesh_kernel<false>, dim3(n, tiles), dim3(rex::kRenderThreads), 0, st, s->dev, s->d_state, cam,
                       d_ids, width, height, vec, nodes, s->d_vis_tris, s->d_vis_root, s->d_vis_box, d_rgb, d_depth, d_seg);
  return hipGetLastError();
}
