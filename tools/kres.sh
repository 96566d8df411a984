#!/bin/bash
# resource usage (AGPRs, scratch) of every kernel of one variant group's translation unit, with extra compiler flags:
#   tools/kres.sh step_arm '-DREX_TARGET_BY_DIVISION(EPW,ARM)=0' ...
#   tools/kres.sh step_base -DREX_TU_MODE=REX_MODE_POL      the fused-actor kernels; REX_MODE_RNN: the recurrent ones (step_base, step_arm);
#                           REX_MODE_TRACE / REX_MODE_SEG: any step unit; -DREX_TU_MOT=1 next to SEG, POL, RNN (csrc/rex_kernels.h RexStepMode)
#   tools/kres.sh render   the rollout kernel's instantiations and the outcome kernel (built into the readout object): registers, scratch, LDS
cd "$(dirname "$0")/.."
G=$1; shift
FLAGS=$(python -c "from rex_gym_amd.build import COMPILE_FLAGS; print(' '.join(COMPILE_FLAGS))")   # the library's own compile flags
D=scratch/isa_$$_$RANDOM
mkdir -p $D && cd $D
if [ "$G" = render ]; then
  hipcc $FLAGS -Rpass-analysis=kernel-resource-usage "$@" -I ../../rex_gym_amd/csrc -c ../../rex_gym_amd/csrc/rex_render.hip -o /dev/null 2>&1 \
    | grep -E "Function Name: .*rex_(rollout|outcome)_kernel| VGPRs:|AGPRs:|SGPRs:|ScratchSize|LDS Size|Occupancy" | grep -A6 "Function Name" | grep -v "^--" \
    | sed 's/.*Function Name: _ZN3rex12_GLOBAL__N_118/K /; s/EEEvNS_6DevCfg.*//; s/ENS_6DevCfg.*//; s/.*remark: *//; s/\[-Rpass.*//' | paste - - - - - - -
  cd ../..; rm -rf $D; exit 0
fi
hipcc $FLAGS -Rpass-analysis=kernel-resource-usage "$@" -I ../../rex_gym_amd/csrc -c ../../rex_gym_amd/csrc/rex_${G}.hip -o /dev/null 2>&1 \
  | grep -E "Function Name: .*rex_(step|settle)_kernel|AGPRs:|ScratchSize" | sed 's/.*Function Name: _ZN3rex15rex_step_kernel/K /; s/.*Function Name: _ZN3rex17rex_settle_kernel/S /; s/EEEv.*//; s/.*remark: *//; s/\[-Rpass.*//' | paste - - -
cd ../..; rm -rf $D
