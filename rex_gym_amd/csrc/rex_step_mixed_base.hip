// rex_step_mixed_base.hip -- instantiates the kernels of one variant group (rex_kernels.h): mark base, REX_TASK_MIXED.
#include "rex_kernels.h"

template <> void rex_launch_step<REX_GROUP_MIXED_BASE, REX_TU_MODE, REX_TU_MOT != 0>(RexSim* s, int blocks, hipStream_t st, const float* a, float* o, float* r, uint8_t* d, float* m) {
  REX_LAUNCH_BY_EPW(false, true, false);
}
