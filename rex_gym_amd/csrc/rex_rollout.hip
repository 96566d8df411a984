// rex_rollout.hip -- candidate rollouts: K command sequences per env over T control steps of `repeat` substeps, simulated from the env's
// current state on a private copy, read out and never written back (rex_rollout.h; the substep: rex_rollout in include/rexsim.h).
//
// rex_rollout_kernel: the mapping of rex_contact_solve_kernel -- one lane per (row, leg), a row's four legs one DPP quad, 32 rows per
// workgroup -- with row r = (env ids[r / K], candidate r % K).  The row's copy W of the state's words 0..36 lives in LDS, [37][32] floats
// behind the FK tables; the front end reads it through fk_base / fk_leg_body / ldw with stride 32 and the row's column
// (rex_rollout_leg.h: dyn_load_leg, the overload).  What does not change over the rollout is formed once per row: the env's ground
// (env_ground: mass scales, toe friction, the terrain field of its episode), its motor enable bits and, when a table or ranges are set, its
// actuator parameters (motor_scalars, motor_strengths).  Then, per substep:
//   1. the torque: the motor model of rex_substep on (cmd, q, qd, qd) of W times the enable bit, or tau as given;
//   2. sections 1-5 of rex_contact_solve_kernel with damping = 1 (rex_contact_rows.h) on W under that torque -> v_next;
//   3. physics_substep's integrator (rex_rollout_leg.h: rollout_integrate); the lanes write the advanced W -- every lane its leg's q and
//      qd, the leg-0 lane the position and linear velocity, the leg-1 lane the quaternion and angular velocity, the writers of
//      rex_contact_solve's v_next -- and the workgroup meets at a barrier before anything reads it: the emission of `trajectory` and the
//      next substep's front end (whose own barrier sits after fk_base's reads and does not cover it).
// Every loop is bounded by launch-uniform numbers the host has checked (T x repeat <= 4096 substeps of <= 1000 sweeps).  Global memory
// is only read (state, commands) and written (outputs); the sim's state is not written.  Not advanced: overheat counters and the motor
// mask, controller and gait words, step and episode counters, sensor noise.  Lanes of rows past the end repeat the last row, take every
// barrier, quad sum and ballot, and store nothing to global memory.
//
// The kernel is a template over its argument.  With RexRolloutLaunch it is rex_rollout's, as above.  With RexRolloutFromLaunch it is
// rex_rollout_from's (rex_rollout.h), the same source with three reads more, each behind a launch-uniform null test:
//   load    W from init_state + row * 37 instead of the state;
//   body    after env_ground, the two mass scales and mu of the row's Ground from body + row * 3;
//   wrench  base_wrench + (row * T + t) * 6, read beside the command once per control step and handed to con_free_velocity, which takes
//           it off the bias wrench about the base origin (zeros when the pointer is null: x - (+0) is x, the same bits).
// W is then the caller's, so what a row computes from W was read for arbitrary float input, non-finite and huge values included:
//   - the only address formed from W is ground_query's (rex_device.h), under the toe points: the grid coordinate goes through
//     fminf(fmaxf(x, 0), max) before the conversion to int -- a NaN comes out as 0, an infinity as a bound -- so the four heights read
//     lie inside the env's field; the field itself (Ground::off, mid) comes from the env's episode word, never from W;
//   - the FK tables and W in LDS are addressed by the lane's row and leg, constants of the launch; the rows of ConRows by unrolled
//     constants; the motor model's table is a minimum of lines; sincos_fast and sincosf reduce in registers, their quadrant is used in
//     selects only;
//   - the loops run T, repeat and at most `iterations` times, all launch-uniform; con_sweeps leaves early on a ballot but never later.
// A bad row yields garbage in that row only: rows share nothing but the barriers and the ballot of the sweep loop's early exit, which a
// row that never converges can only hold to the `iterations` every row is allowed anyway.
// With RexRolloutOutcomeLaunch it is rex_rollout_actions_outcome's: rex_rollout_from's with the step's epilogue behind every control step.
// The observed torque of the motor model (`obs`, what rex_substep keeps as ms.tau_obs: not act x enable) of the step's last substep stays
// in three registers; behind the substep loop's last barrier the lanes store it and call outcome_row (rex_outcome.h) on W, the row's
// controller words after the step (ctrl + row * 8, read and never used as an address) and those torques.  Every store sits behind `live`
// and a launch-uniform null test; outcome_row's quad sum is taken by every lane.
// (Built as part of rex_render.hip's object, like rex_contact_solve.hip: rex_gym_amd/build.py INCLUDED_IN.)
#include <type_traits>
#include "rex_render_common.h"
#include "rex_rollout.h"
#include "rex_contact_rows.h"
#include "rex_rollout_leg.h"
#include "rex_outcome.h"

namespace rex {

namespace {

constexpr int kRolloutFkFloats = (kDynEnvs * kDynStride + 3) & ~3;                     // the FK tables of the workgroup's rows
constexpr int kRolloutBytes = (kRolloutFkFloats + kRolloutWords * kDynEnvs) * (int)sizeof(float);
static_assert(kRolloutFkFloats * (int)sizeof(float) == kDynFkBytes && kRolloutBytes <= 64 * 1024, "no more than the 64 KiB a launch gets by default");
static_assert(REX_S_POS == 0 && REX_S_QUAT == 3 && REX_S_LINVEL == 7 && REX_S_ANGVEL == 10 && Lay<REX_NUM_MOTORS>::Q == 13 &&
              Lay<REX_NUM_MOTORS>::QD + REX_NUM_MOTORS == kRolloutWords, "W holds the words 0..36 in the state's order");

// the kernel's argument: the launch's settings and the sim's actuator knobs; for rex_rollout_from the per-row inputs behind them
struct RexRolloutLaunch { RexRolloutArgs a; MotDev mot; };
struct RexRolloutFromLaunch : RexRolloutLaunch { RexRolloutFrom from; };
struct RexRolloutOutcomeLaunch : RexRolloutFromLaunch {
  const float* ctrl;         // [rows][8] the controller words after this control step
  RexOutcomeOut outcome;     // reward, done [rows][T], obs [rows][T][obs_dim]; null members are skipped
  float* motor_torque;       // [rows][T][12] or null
};

template <class Launch>
__global__ void __launch_bounds__(kDynThreads) rex_rollout_kernel(DevCfg c, const float* __restrict__ state, const int32_t* __restrict__ ids,
                                                                  int rows_total, Launch la) {
  constexpr int NM = REX_NUM_MOTORS, NE = kDynEnvs;
  constexpr bool OUTCOME = std::is_same<Launch, RexRolloutOutcomeLaunch>::value;
  constexpr bool FROM = std::is_same<Launch, RexRolloutFromLaunch>::value || OUTCOME;
  extern __shared__ __attribute__((aligned(16))) float s_roll[];
  const RexRolloutArgs& a = la.a;
  const int el0 = threadIdx.x >> 2, leg0 = threadIdx.x & 3, el = el0, leg = leg0;
  const bool live = blockIdx.x * kDynEnvs + el < rows_total;
  const int row = min(blockIdx.x * kDynEnvs + el, rows_total - 1);   // (the grid has ceil(rows_total / kDynEnvs) workgroups)
  const int er = row / a.K;                                          // the row of env ids; row % K is the candidate
  const int env = ids ? ids[er] : er;                                // the state's env index (checked on the host)
  float* W = s_roll + kRolloutFkFloats;                              // [kRolloutWords][NE]: word w of this row at W[w * NE + el]

  // ---- the row's copy of the state, and what stays as it is at the call ----
  if constexpr (FROM) {
    if (la.from.init_state) {                                        // (every pointer of `from` is the same in every thread)
      const float* src = la.from.init_state + (size_t)row * kRolloutWords;
      for (int w = leg; w < kRolloutWords; w += 4) W[w * NE + el] = src[w];
    } else {
      for (int w = leg; w < kRolloutWords; w += 4) W[w * NE + el] = ldw(state, c.n, w, env);
    }
  } else {
    for (int w = leg; w < kRolloutWords; w += 4) W[w * NE + el] = ldw(state, c.n, w, env);
  }
  const int gidx = c.env_index_base + env, episode = (int)ldi(state, c.n, Lay<NM>::EPISODE, env);
  Ground ground = env_ground(c, env, gidx, episode);
  if constexpr (FROM) {
    if (la.from.body) {
      const float* b = la.from.body + (size_t)row * 3;
      ground.base_mass_scale = b[0]; ground.leg_mass_scale = b[1]; ground.mu = b[2];
    }
  }
  const Ground g = ground;
  const uint32_t motor_en = ldi(state, c.n, Lay<NM>::MOTOR_EN, env);
  MotorScalars mp{kMotorVoltage, 0.0f, c.kp, c.kd};
  float strength[3] = {1.0f, 1.0f, 1.0f};
  if (a.motor) {                                                     // (a.motor, a.targets and every output pointer are the same in every thread)
    mp = motor_scalars(c, la.mot, env, gidx, episode);
    motor_strengths<3>(c, la.mot, env, gidx, episode, 3 * leg, strength);
  }
  const bool field = c.n_terrain > 0;
  const float dt = a.dt;
  const float* commands = a.targets ? a.targets : a.tau;
  const RexRolloutOut& out = a.out;
  __syncthreads();                                                   // W is written; the front end's first reads follow

  int count = 0;
  for (int t = 0; t < a.T; ++t) {
    float cmd[3];
    {
      const float* p = commands + ((size_t)row * a.T + t) * 12 + 3 * leg;
      cmd[0] = p[0]; cmd[1] = p[1]; cmd[2] = p[2];
    }
    float wrench[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                // (FROM only) the control step's base wrench, on every lane of the row
    if constexpr (FROM) {
      if (la.from.base_wrench) {
        const float* p = la.from.base_wrench + ((size_t)row * a.T + t) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) wrench[i] = p[i];
      }
    }
    bool touch = false;
    float tobs[3] = {0.0f, 0.0f, 0.0f};                              // (OUTCOME only) the observed torques of the control step's last substep
    for (int r = 0; r < a.repeat; ++r) {
      // opaque copies of the lane's row and leg: what the front end forms from them alone (table addresses, the leg's model constants) is
      // invariant over the substeps, and would otherwise be hoisted in front of the loops and carried through every solver sweep
      int el = el0, leg = leg0;
      asm volatile("" : "+v"(el), "+v"(leg));
      float (*R)[9] = reinterpret_cast<float (*)[9]>(s_roll + el * kDynStride);
      float (*o)[3] = reinterpret_cast<float (*)[3]>(s_roll + el * kDynStride + 9 * REX_NB);
      // ---- the leg, its composites, H_f and B_f, the base block; the factors ----
      DynFront F;
      dyn_load_leg(W, NE, el, g, leg, R, o, F);
      DynComposite C;
      dyn_composites(F, C);
      const DynLeg& L = F.L;
      float H[3][3];
      dyn_leg_block(L, C, H);
      DynFactor Q;
      dyn_factor(C, H, Q);

      // ---- 1. the torque ----
      float bf[3];
      if (a.targets) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float q = ldw(W, NE, Lay<NM>::Q + 3 * leg + i, el), qd = L.qd[i];
          float act, obs;
          if (a.motor) motor_torque(cmd[i], q, qd, qd, mp.kp, mp.kd, mp.voltage, mp.damping, strength[i], act, obs);
          else motor_torque(cmd[i], q, qd, qd, c.kp, c.kd, act, obs);
          bf[i] = ((motor_en >> (3 * leg + i)) & 1u) ? act : 0.0f;
          if constexpr (OUTCOME) tobs[i] = obs;
        }
      } else {
        bf[0] = cmd[0]; bf[1] = cmd[1]; bf[2] = cmd[2];
      }

      // ---- 2. v_next of rex_contact_solve with damping = 1 ----
      float vs0[6], vsf[3];
      if constexpr (FROM) con_free_velocity<true>(F, Q, bf, 1, dt, vs0, vsf, wrench);
      else con_free_velocity(F, Q, bf, 1, dt, vs0, vsf);
      ConRows P;
      con_build_rows(W, NE, el, leg, field, F, Q, dt, vs0, vsf, P);
      count += con_sweeps(P, g.mu, leg, a.iterations, a.threshold);
      float dx[6], dq[3];
      con_velocity_change(Q, P, dx, dq);
      float lin[3], ang[3], qd[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        lin[i] = clampf(vs0[i] + dx[i], -kMaxCoordVel, kMaxCoordVel);
        ang[i] = clampf(vs0[3 + i] + dx[3 + i], -kMaxCoordVel, kMaxCoordVel);
        qd[i] = clampf(vsf[i] + dq[i], -kMaxCoordVel, kMaxCoordVel);
      }
      touch = P.lam[3] > 0.0f || P.lam[4] > 0.0f;

      // ---- 3. the integrator; the advanced W ----
      float pos[3], quat[4], q[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { pos[i] = ldw(W, NE, REX_S_POS + i, el); q[i] = ldw(W, NE, Lay<NM>::Q + 3 * leg + i, el); }
#pragma unroll
      for (int i = 0; i < 4; ++i) quat[i] = ldw(W, NE, REX_S_QUAT + i, el);
      rollout_integrate(dt, lin, ang, qd, pos, quat, q);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        W[(Lay<NM>::Q + 3 * leg + i) * NE + el] = q[i];
        W[(Lay<NM>::QD + 3 * leg + i) * NE + el] = qd[i];
      }
      if (leg == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { W[(REX_S_POS + i) * NE + el] = pos[i]; W[(REX_S_LINVEL + i) * NE + el] = lin[i]; }
      } else if (leg == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) W[(REX_S_QUAT + i) * NE + el] = quat[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) W[(REX_S_ANGVEL + i) * NE + el] = ang[i];
      }
      __syncthreads();                                               // the advanced W is written; its next reads follow
    }
    if (live) {
      if (out.trajectory) {
        float* d = out.trajectory + ((size_t)row * a.T + t) * kRolloutWords;
        for (int w = leg; w < kRolloutWords; w += 4) d[w] = W[w * NE + el];
      }
      if (out.foot_contact) out.foot_contact[((size_t)row * a.T + t) * 4 + leg] = touch ? 1 : 0;
    }
    if constexpr (OUTCOME) {                                         // the step's epilogue on the advanced W (behind the loop's last barrier)
      if (la.motor_torque && live) {
        float* d = la.motor_torque + ((size_t)row * a.T + t) * NM + 3 * leg;
        d[0] = tobs[0]; d[1] = tobs[1]; d[2] = tobs[2];
      }
      if (la.outcome.reward || la.outcome.done || la.outcome.obs) {  // (the same in every thread: nobody misses the quad sum)
        uint32_t cw[kOutcomeCtrlWords];
#pragma unroll
        for (int j = 0; j < kOutcomeCtrlWords; ++j) cw[j] = __float_as_uint(la.ctrl[(size_t)row * kOutcomeCtrlWords + j]);
        Outcome o;
        outcome_row(c, W, NE, el0, leg0, cw, tobs, o);
        if (live) outcome_store(c, la.outcome, (size_t)row * a.T + t, leg0, o);
      }
    }
  }
  if (live) {
    if (out.state) {
      float* d = out.state + (size_t)row * kRolloutWords;
      for (int w = leg; w < kRolloutWords; w += 4) d[w] = W[w * NE + el];
    }
    if (out.sweeps && leg == 0) out.sweeps[row] = count;
  }
}

}  // namespace
}  // namespace rex

hipError_t rex_launch_rollout(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, hipStream_t st) {
  const rex::RexRolloutLaunch la{a, s->mot};
  return rex::dyn_launch(rex::rex_rollout_kernel<rex::RexRolloutLaunch>, rex::kRolloutBytes, s, d_ids, n * a.K, la, st);
}

hipError_t rex_launch_rollout_from(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, const RexRolloutFrom& from,
                                   hipStream_t st) {
  const rex::RexRolloutFromLaunch la{{a, s->mot}, from};
  return rex::dyn_launch(rex::rex_rollout_kernel<rex::RexRolloutFromLaunch>, rex::kRolloutBytes, s, d_ids, n * a.K, la, st);
}

hipError_t rex_launch_rollout_outcome(const RexSim* s, const int32_t* d_ids, int n, const rex::RexRolloutArgs& a, const RexRolloutFrom& from,
                                      const float* ctrl, const RexOutcomeOut& outcome, float* motor_torque, hipStream_t st) {
  const rex::RexRolloutOutcomeLaunch la{{{a, s->mot}, from}, ctrl, outcome, motor_torque};
  return rex::dyn_launch(rex::rex_rollout_kernel<rex::RexRolloutOutcomeLaunch>, rex::kRolloutBytes, s, d_ids, n * a.K, la, st);
}
