"""One substep of the step against the readout's references, the parts that need no GPU (tests/step_readout_ref.py holds the recipe).

An orclib.OracleEnv (walk, ik, action_repeat 1, 60 sweeps) gets a scene's body parameters (dynamics_ref.scene_scales, the friction of
contact_solve_ref.scene_params) and terrain, is reset, gets the synthetic columns of contact_solve_ref.scene_states written over words
0 .. 36 and the episode word (the quaternion normalised in float64, as in tests/test_contact_solve_host.py), and takes one step with a
seeded action.  With tau = the motor model on the returned motor command and the pre-step joint state:

  1. v_next of contact_solve_ref.reference on the pre-step state against the velocity words after the step -- the contact reference
     restates the step's substep on every scene: per-env mass scales, per-env friction, the random pool and the custom field;
  2. the positions, quaternion and joint angles after the step against kinematics_ref.advance of the pre-step state along the new
     velocities (symplectic Euler; the oracle normalises the quaternion, and so does the comparison);
  3. the float32 floor of one substep: OracleEnv(np.float32) against OracleEnv(np.float64) from the same states and actions, which the step
     bound of tests/test_gpu_step_readout.py is FACTOR (4) x of;
  4. the share of every scene's envs that enters the comparisons, and what the step does to the counters.

Measured here (float64; gap relative to max(1, |v|), integrator absolute; envs `done` after the step are advanced like the others):

    scene         threshold   gap to the oracle   pos        quat       q          float32 floor   kept     done
    1   plane     0 / 1e-7    6.4e-16             0          0          0          4.008e-07       1 / 1    0
    5   plane     0 / 1e-7    1.8e-15             0          0          0          1.523e-06       3 / 3    1
    67  plane     0           9.7e-15             0          2.2e-16    0          1.090e-05       63 / 63  19
    67  plane     1e-7        1.1e-14             0          2.2e-16    0          1.090e-05       63 / 63  19
    130 plane     0           1.7e-14             0          2.2e-16    0          1.465e-05       126/126  31
    130 plane     1e-7        1.7e-14             0          2.2e-16    0          5.807e-05       126/126  31
    67  random    0 / 1e-7    1.5e-14             0          2.2e-16    0          1.029e-04       63 / 63  16
    67  custom    0 / 1e-7    4.0e-13             0          2.2e-16    0          1.674e-04       62 / 63  19

With the custom field's grid constants formed in float64 (1 / 0.7, the offsets, n - 1 - 0.001) instead of the float32 values the product's
host code and the oracle hold, the custom scene's gap was 3.7e-05 in 19 of 63 envs: kinematics_ref.grid_constants and clamp_limit."""
import numpy as np
import pytest

import contact_solve_ref as cr
import kinematics_ref as kr
import step_readout_ref as sr

ORACLE_GAP = 4.0e-13                    # the largest `gap to the oracle` of the table
ORACLE_BOUND = 100 * ORACLE_GAP
INTEGRATOR_GAP = 2.0 ** -52             # the largest integrator deviation of the table: one unit in the last place of 1
INTEGRATOR_BOUND = 100 * INTEGRATOR_GAP
STEP_FLOOR = {0.0: 1.674e-04, cr.THRESHOLD: 1.674e-04}          # the largest `float32 floor` per threshold


class Measured:
    """one scene at one threshold: the float64 and the float32 oracle stepped once from the scene's synthetic states"""

    def __init__(self, n, ground, thr):
        import test_gpu_kinematics as tk
        self.n, self.ground, self.thr = n, ground, thr
        keep = self.keep = kr.scene_keep(n)
        S, self.kinds = cr.scene_states(n, ground)
        S64 = S.astype(np.float64)
        S64[3:7, keep:] /= np.linalg.norm(S64[3:7, keep:], axis=0)
        fields = kr.scene_fields(ground)
        ep = S[kr.episode_word(False)].view(np.int32)
        bp, act = sr.body_params(n), sr.actions(n)
        o64, o32 = sr.oracle_env(n, ground, thr), sr.oracle_env(n, ground, thr, np.float32)
        self.before, self.after, cmd, self.done = sr.oracle_substep(o64, S64, keep, act)
        _, after32, _, _ = sr.oracle_substep(o32, S64, keep, act)
        o64.close(), o32.close()
        assert np.array_equal(self.before[0:37, keep:], S64[0:37, keep:])
        self.gap, self.integ, self.floor, self.compared, self.kept = {}, {}, {}, [], []
        for g in range(keep, n):
            fld = kr.field_of(fields, g, ep[g])
            ref = cr.reference(S64, g, fld, (bp[0, g], bp[1, g]), float(bp[2, g]), sr.motor_tau(cmd[g], self.before, g),
                               residual_threshold=sr.threshold32(thr))
            self.gap[g] = sr.vel_error(ref["v_next"], self.after[sr.VEL_WORDS, g])
            self.integ[g] = sr.integrator_errors(self.before, self.after, g)
            self.floor[g] = sr.vel_error(after32[sr.VEL_WORDS, g], self.after[sr.VEL_WORDS, g])
            if cr.compared(S, g, fld, ref, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"]):
                self.compared.append(g)
            if sr.kept(S, g, fld, ref, self.before[46, g], tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"]):
                self.kept.append(g)


@pytest.fixture(scope="module")
def measured():
    made = {}

    def get(n, ground, thr):
        if (n, ground, thr) not in made:
            made[(n, ground, thr)] = Measured(n, ground, thr)
        return made[(n, ground, thr)]
    return get


IDS = ["%d-%s" % s for s in sr.SCENES]
THR_IDS = ["sixty_sweeps", "default_threshold"]


# ---------------------------------------------------------------- 0. the grid the reference holds
def test_reference_holds_the_grid_constants_of_the_host_code():
    """The constants are float32 values (rex_set_heightfield of csrc/rexsim.hip: `g.inv_cx = 1.0f / cell_x`, `g.off_x = 0.5f * (float)(nx - 1)
    - origin_x * g.inv_cx`, `g.max_x = (float)(nx - 1) - 0.001f`; rex_set_terrain: `HfGeom{256, 20.0f, 20.0f, 127.5f, 127.5f, 254.999f,
    254.999f}`), and differ from their float64 namesakes where those are not representable."""
    f = np.float32
    for fld in kr.scene_fields("custom"):
        assert all(float(f(c)) == c for c in fld[4:8])
        assert fld[4:6] == (float(f(1) / f(0.5)), float(f(1) / f(0.7))) and fld[5] != 1.0 / 0.7
        assert fld[6:8] == (float(f(6) - f(0.4) * f(2)), float(f(4) + f(0.3) * (f(1) / f(0.7))))
    assert kr.clamp_limit(256) == float(f(254.999)) != 254.999 and kr.clamp_limit(13) == float(f(12) - f(0.001)) != 12 - 0.001
    assert kr.random_terrain_field(np.zeros((1, 65536)), [0.0], 0)[2:] == (256, 256, 20.0, 20.0, 127.5, 127.5)
    # beside the footprint the clamp decides: far out in +y and at the limit itself the query stands on the same point of the last cell row
    fld = kr.scene_fields("custom")[1]
    y_limit = (kr.clamp_limit(kr.CUSTOM_NY) - fld[7]) / fld[5]
    far, at = kr.ground_query(fld, 0.3, 40.0), kr.ground_query(fld, 0.3, y_limit + 1e-9)
    assert far[2] == at[2] and far[0] == at[0] and (far[2] == 0 or (far[2] - 1) // 2 // kr.CUSTOM_NX == kr.CUSTOM_NY - 2)


# ---------------------------------------------------------------- 1. the contact reference restates the step's substep
@pytest.mark.parametrize("threshold", sr.THRESHOLDS, ids=THR_IDS)
@pytest.mark.parametrize("n,ground", sr.SCENES, ids=IDS)
def test_reference_restates_the_oracles_step(measured, n, ground, threshold):
    """v_next of the reference against the velocity words after one OracleEnv.step, every synthetic env (the done ones too), relative to
    max(1, |v|): the worst value of the module's table, asserted at 100 x that and below the 1e-7 that would still tell two problems apart."""
    m = measured(n, ground, threshold)
    g = max(m.gap, key=m.gap.get)
    print((n, ground, threshold), "gap to the oracle %.3e (env %d, %s; bound %.1e), %d envs, %d done" % (m.gap[g], g, m.kinds[g], ORACLE_BOUND, len(m.gap), m.done[m.keep:].sum()))
    assert ORACLE_BOUND < 1e-7 and len(m.gap) == n - m.keep
    assert m.gap[g] <= ORACLE_BOUND, (g, m.kinds[g], m.gap[g])


# ---------------------------------------------------------------- 2. the integrator
@pytest.mark.parametrize("n,ground", sr.SCENES, ids=IDS)
def test_positions_advance_along_the_new_velocities(measured, n, ground):
    """pos += dt v', q += dt qd', quat = normalised exp(dt w' / 2) quat with the velocities AFTER the solve; every synthetic env, float64
    round-off: measured at most 2^-52 (the quaternion), asserted at 100 x that."""
    m = measured(n, ground, 0.0)
    worst = np.max(list(m.integ.values()), axis=0)
    print((n, ground), "integrator pos %.2e quat %.2e q %.2e (bound %.1e)" % (*worst, INTEGRATOR_BOUND))
    assert np.all(worst <= INTEGRATOR_BOUND), worst
    moved = [g for g in m.gap if np.abs(m.after[0:3, g] - m.before[0:3, g]).max() > 0]
    assert len(moved) >= 0.9 * len(m.gap) or n == 1


# ---------------------------------------------------------------- 3. the float32 floor behind the GPU test's step bound
def test_step_bound_of_the_gpu_test_is_the_stated_multiple_of_the_float32_floor(measured):
    """Per threshold the largest deviation of the float32 oracle's velocity words from the float64 oracle's after one substep from the same
    states, over the envs contact_solve_ref.compared keeps, all six scenes: the GPU test's bound is FACTOR (4) x that, with 2 % of slack for
    another libm.  (At 1e-7 the two precisions may leave the sweep loop after different counts, which moves the result by less than the
    threshold: DESIGN.md.)"""
    import test_gpu_step_readout as tg
    assert tg.FACTOR == 4.0 and set(tg.STEP_BOUNDS) == set(sr.THRESHOLDS)
    for thr in sr.THRESHOLDS:
        floor = max(measured(n, ground, thr).floor[g] for n, ground in sr.SCENES for g in measured(n, ground, thr).compared)
        print("threshold %g: float32 floor of one substep %.3e, written %.3e, bound %.3e" % (thr, floor, STEP_FLOOR[thr], tg.STEP_BOUNDS[thr]))
        assert tg.STEP_BOUNDS[thr] <= tg.FACTOR * STEP_FLOOR[thr] * (1 + 1e-9)
        assert 0 < tg.STEP_BOUNDS[thr] <= tg.FACTOR * floor * 1.02, (thr, tg.STEP_BOUNDS[thr], floor)


def test_readout_bounds_of_the_real_columns_lie_under_their_familys_floor():
    """The GPU test's leading columns keep the env's own state: the robot standing on eight toe points after the reset and 8 steps, whose
    redundant contact rows the 60 sweeps do not resolve (the last sweep's residual is 1e-5, not 0).  contact_solve_ref.measure_floors
    does not see that family (its leading columns are zero on the CPU), so its floor is measured here, over step_readout_ref.real_family
    of the five scenes: reference() in float32 against float64 under the step's torque.  Measured: toe_force 7.402e-04, toe_lambda
    7.402e-04 (plane), v_next 5.446e-04 (random pool) -- above the synthetic floors (1.832e-04, 1.913e-04, 1.001e-04).  The GPU test
    holds the real columns to REAL_BOUNDS, which must stay under FACTOR (4) x these floors and not under the bounds of the synthetic family."""
    import test_gpu_contact_solve as tc
    import test_gpu_step_readout as tg
    floors = {k: 0.0 for k in cr.FIELDS}
    for n, ground in [s for s in sr.SCENES if s[0] > 1]:
        keep = kr.scene_keep(n)
        S, ep, cmd = sr.real_family(n, ground, keep)
        fields, bp = kr.scene_fields(ground), sr.body_params(n)
        for g in range(keep):
            kw = dict(field=kr.field_of(fields, g, ep[g]), scales=(bp[0, g], bp[1, g]), mu=float(bp[2, g]), tau=sr.motor_tau(cmd[g], S, g))
            r64 = cr.reference(S, g, **kw)
            assert r64["in_reach"].sum() >= 4
            for k, v in cr.errors(cr.reference(S, g, dtype=np.float32, **kw), r64).items():
                floors[k] = max(floors[k], v)
    print("float32 floor of the readout over the real family:", {k: "%.3e" % v for k, v in floors.items()})
    for k in ("toe_force", "toe_lambda", "v_next"):
        assert tc.BOUNDS[k] <= tg.REAL_BOUNDS[k] <= tg.FACTOR * floors[k] * 1.02, (k, tg.REAL_BOUNDS[k], floors[k])
    assert tg.REAL_BOUNDS["limit_torque"] == tc.BOUNDS["limit_torque"]


# ---------------------------------------------------------------- 4. who is compared, and the counters
@pytest.mark.parametrize("n,ground", sr.SCENES, ids=IDS)
def test_at_least_nine_tenths_of_every_scene_are_compared(measured, n, ground):
    """step_readout_ref.kept -- contact_solve_ref.compared, no component of v_next at the +-100 clamp, every motor enabled -- from the
    reference alone; the done envs are not left out."""
    m = measured(n, ground, 0.0)
    print((n, ground), "kept %d, compared %d of %d" % (len(m.kept), len(m.compared), n - m.keep))
    assert set(m.kept) <= set(m.compared) and len(m.kept) >= 0.9 * (n - m.keep)
    assert n < 67 or any(m.done[g] for g in m.kept)


@pytest.mark.parametrize("n,ground", [(67, "plane"), (67, "custom")], ids=["67-plane", "67-custom"])
def test_the_step_counts_one_step_and_keeps_the_episode(measured, n, ground):
    """What the GPU test expects of the integer words: REX_S_STEPS + 1 in every env, done or not (auto-reset is off), REX_S_EPISODE and the
    motor mask as they were, REX_F_DONE set exactly where done is returned."""
    import orclib
    m = measured(n, ground, 0.0)
    b, a = m.before, m.after
    assert np.array_equal(a[orclib.S_STEPS], b[orclib.S_STEPS] + 1) and np.array_equal(a[orclib.S_EPISODE], b[orclib.S_EPISODE])
    assert np.all(b[orclib.S_MOTOR_EN] == sr.ALL_MOTORS) and np.array_equal(a[orclib.S_MOTOR_EN], b[orclib.S_MOTOR_EN])
    assert np.array_equal((a[orclib.S_FLAGS].astype(np.int64) & orclib.F_DONE) != 0, m.done) and m.done.any() and not m.done.all()
