// rex_render.h -- batched ray-cast renderer of the simulated scene: what the camera of the reference's
// RexGymEnv.render(mode="rgb_array") (rex_gym_env.py:416-439) would see, over the ground plane / the env's heightfield.
// rex_render draws the COLLISION geometry the simulator uses (rex_render_gen.h: link boxes, full toe cylinders, the arm's
// cylinders); rex_render_visual draws the URDF's visual meshes (rex_visual_gen.h, BVHs set by rex_render_set_visuals).
// Separate, read-only launches: they read the caller-owned state, the terrain pool and the visual buffers, and write the
// caller's image buffers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RexSim;

namespace rex {

// The camera of one rex_render call, in world axes.  The host turns (distance, yaw, pitch) into these with Bullet's
// b3ComputeViewMatrixFromYawPitchRoll convention (rexsim.hip, rex_render): the eye of env i sits at base_pos(i) + off;
// fwd / right / up are the unit view axes.  A pixel's ray is fwd + sx * right + sy * up with sx, sy in
// [-tan_x, tan_x] x [-tan_y, tan_y]: its parameter t IS the eye-space depth along fwd.
struct RenderCam {
  float off[3], fwd[3], right[3], up[3];
  float tan_x, tan_y;   // tan(fov_y / 2) * width / height, tan(fov_y / 2)
  float near_plane, far_plane;
};

// Shading constants (our choice; the reference's renderer and its checker texture are not reproduced):
//   Lambert with one directional light kLight (unit vector towards the light) and an ambient term:
//     colour = albedo * (kAmbient + kDiffuse * max(0, n . kLight)), n the surface normal facing the camera;
//   8-bit value = min(255, floor(255 * colour + 0.5)); rays that hit nothing get kSky.
//   Ground: a two-tone checker of 1 m squares (plane.obj repeats its texture every 2 m: two squares per repeat and axis);
//   square (floor(x), floor(y)) takes kCheckerA when floor(x) + floor(y) is even, else kCheckerB; heightfield facets too.
constexpr float kLightX = 0.36f, kLightY = -0.48f, kLightZ = 0.8f;
constexpr float kAmbient = 0.35f, kDiffuse = 0.65f;
constexpr float kSkyR = 0.70f, kSkyG = 0.80f, kSkyB = 0.92f;
constexpr float kCheckerAR = 0.25f, kCheckerAG = 0.40f, kCheckerAB = 0.65f;
constexpr float kCheckerBR = 0.85f, kCheckerBG = 0.88f, kCheckerBB = 0.92f;

// The mesh kernel's per-thread BVH traversal stack (LDS, 256 threads x 32 entries x 4 B = 32 KiB): rex_render_set_visuals
// refuses trees with more than kMeshStack levels of inner nodes, so a traversal never holds more entries.
constexpr int kMeshStack = 32;

}  // namespace rex

// Launch one rex_render_kernel over n envs (d_ids[k] = the state's env index of output row k): grid (n, pixel tiles of
// 1 024 pixels), 256 threads, each shading 4 consecutive pixels.  d_depth / d_seg may be null.  Arguments are checked
// by the caller (rex_render in rexsim.hip).
hipError_t rex_launch_render(const RexSim* s, const rex::RenderCam& cam, const int32_t* d_ids, int n, int width, int height,
                             uint8_t* d_rgb, float* d_depth, int16_t* d_seg, hipStream_t st);
// The same over the visual meshes (rex_render_mesh.hip): the BVH buffers of rex_render_set_visuals, already validated.
hipError_t rex_launch_render_mesh(const RexSim* s, const rex::RenderCam& cam, const int32_t* d_ids, int n, int width, int height,
                                  uint8_t* d_rgb, float* d_depth, int16_t* d_seg, hipStream_t st);
