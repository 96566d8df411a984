// rex_step_base.hip -- instantiates the kernels of one variant group (rex_kernels.h): mark base, single task, toes only: 4 / 8 / 16 envs per wave (lane groups) and 64 (one env per lane).
#include "rex_kernels.h"

template <> void rex_launch_step<REX_GROUP_BASE, REX_TU_MODE, REX_TU_MOT != 0>(RexSim* s, int blocks, hipStream_t st, const float* a, float* o, float* r, uint8_t* d, float* m) {
  constexpr bool lanes = !rex_mode_has_actor(REX_TU_MODE);   // (the fused actor spreads its neurons over the lanes of an env group: lane-group kernels only)
  if (lanes && s->epw == 64) REX_LAUNCH_STEP(lanes ? 64 : 4, false, false, false);   // (an actor unit's dead branch names no <64> instantiation)
  else REX_LAUNCH_BY_EPW(false, false, false);
}
