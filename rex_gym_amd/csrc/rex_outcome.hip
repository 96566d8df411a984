// rex_outcome.hip -- rex_outcome: reward, done and observation of row (k, c) = (env ids[k], candidate c) as env.step() would return them
// for a row whose control step ended in the given state, controller words and observed motor torques (rex_outcome.h: the step's epilogue
// as a device function; include/rexsim.h: the call).  One small read-only launch, a lane per (row, leg) as rex_command_kernel's: 32 rows
// of 4 legs per workgroup, no LDS.  Global memory is only read (the inputs, or the env's words) and written (the outputs); the sim's
// state is not written.  Lanes of rows past the end shadow the last row through the quad sum and store nothing.
// Addresses: the row index and the env id alone.  No address is formed from a state word, a controller word or a torque: flag bits and the
// step counter only enter compares.  A bad row -- non-finite words, controller words no step wrote -- yields garbage in that row only.
// (Built as part of rex_render.hip's object, like rex_rollout.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include "rex_outcome.h"

namespace rex {

namespace {

constexpr int kOutcomeThreads = 128;          // 32 rows of 4 legs per workgroup

// What one launch does; every member is the same for every thread.
struct RexOutcomeArgs {
  const float* state;          // [n][K][37] words 0..36 after the control step, or null: the env's
  const float* ctrl;           // [n][K][8] controller words after the step as raw 32-bit words, or null: the env's words REX_S_PHI .. REX_S_STEPS
  const float* motor_torque;   // [n][K][12] observed torques of the step's last substep, or null: zeros
  RexOutcomeOut out;           // null members are skipped
  const int32_t* ids;          // [n] or null: env k
  int n, K;
};

__global__ __launch_bounds__(kOutcomeThreads) void rex_outcome_kernel(DevCfg c, RexOutcomeArgs a, const float* __restrict__ env_state) {
  const int rows = a.n * a.K;
  const int t = (int)blockIdx.x * kOutcomeThreads + (int)threadIdx.x;
  const int leg = t & 3;
  const bool inrows = (t >> 2) < rows;
  const int r = inrows ? (t >> 2) : rows - 1;
  const int k = r / a.K;
  const int i = a.ids ? a.ids[k] : k;             // the state's env index (checked on the host)

  uint32_t cw[kOutcomeCtrlWords];
#pragma unroll
  for (int j = 0; j < kOutcomeCtrlWords; ++j) cw[j] = a.ctrl ? __float_as_uint(a.ctrl[(size_t)r * kOutcomeCtrlWords + j]) : ldi(env_state, c.n, REX_S_PHI + j, i);
  float tau[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) tau[j] = a.motor_torque ? a.motor_torque[(size_t)r * REX_NUM_MOTORS + 3 * leg + j] : 0.0f;
  Outcome o;
  // the caller's row, [37] words side by side, or the env's column of the word-major state
  outcome_row(c, a.state ? a.state + (size_t)r * 37 : env_state, a.state ? 1 : c.n, a.state ? 0 : i, leg, cw, tau, o);
  if (!inrows) return;
  outcome_store(c, a.out, (size_t)r, leg, o);
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_outcome(const RexSim* s, const int32_t* d_ids, int n, int K, const float* state, const float* ctrl, const float* motor_torque,
                              const RexOutcomeOut& out, hipStream_t st) {
  const rex::RexOutcomeArgs a{state, ctrl, motor_torque, out, d_ids, n, K};
  const unsigned rows = (unsigned)n * (unsigned)K;
  hipLaunchKernelGGL(rex::rex_outcome_kernel, dim3((4 * rows + rex::kOutcomeThreads - 1) / rex::kOutcomeThreads), dim3(rex::kOutcomeThreads), 0, st, s->dev, a,
                     (const float*)s->d_state);
  return hipGetLastError();
}
