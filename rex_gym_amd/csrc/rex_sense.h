// rex_sense.h -- onboard sensors of every env, read from the state between control steps (rex_sense.hip): a depth camera
// rigidly mounted on the base body (rex_sense_depth) and the ground's height at points around the base (rex_height_scan).
// Separate, read-only launches next to the renderers: they read the caller-owned state, the terrain pool and the heightfield,
// and write the caller's output buffer only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RexSim;

namespace rex {

// The mount of one rex_sense_depth call, in the BASE frame: the eye and the unit view axes (right = fwd x up, worked out on the
// host).  The kernel turns them by each env's base rotation; a pixel's ray is rex_render's (rex_render.h, RenderCam).
struct SenseMount {
  float pos[3], fwd[3], right[3], up[3];
  float tan_x, tan_y;   // tan(fov_y / 2) * width / height, tan(fov_y / 2)
  float near_plane, far_plane;
  int see_robot;        // 0: the ground only
};

// Most envs one workgroup of the depth kernel serves: it takes max(1, 1 024 / (width * height)) of them, so that its 256 threads
// x 4 pixels are busy at sensor sizes, and their tables (2.6 KiB an env) stay a quarter of the LDS of a CU.
constexpr int kSenseMaxEnvs = 16;

}  // namespace rex

// One rex_sense_depth_kernel over n output rows (row k = env d_ids[k], or env k with d_ids null).  Arguments are checked by
// the caller (rex_sense_depth in rexsim.hip).
hipError_t rex_launch_sense_depth(const RexSim* s, const rex::SenseMount& m, const int32_t* d_ids, int n, int width, int height,
                                  float* d_depth, hipStream_t st);
// One rex_height_scan_kernel: K points [K][2] in the base's yaw frame for each of n rows -> d_out [n][K].
hipError_t rex_launch_height_scan(const RexSim* s, const float* d_points, int K, int relative, const int32_t* d_ids, int n,
                                  float* d_out, hipStream_t st);
