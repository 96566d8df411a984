"""The step kernels and the contact-solve readout on ONE state (MI355X): what holds RexBatchEnv.contact_solve's "one substep of the step's
physics, restated" and rex_motor_torque / rex_motor_torque_params' "reproduces the torque the step draws".

The env: walk, ik, action_repeat 1, control time step 0.001 s, 60 sweeps, no latency, auto-reset off (step_readout_ref.STEP_KW on top of
test_gpu_kinematics.make_env) -- one env.step() is one physics substep.  Per case: reset, 8 random steps, the synthetic columns of
contact_solve_ref's scene, the scene's mass scales and friction; S0 = the state; one step with seeded actions -> S1 and the motor command;
S0 written back (bits asserted); tau = rex_motor_torque(cmd, q0, qd0, qd0) (rex_motor_torque_params in the actuator case);
env.contact_solve(tau=tau) with the config's dt, sweeps and threshold.  The float64 reference is contact_solve_ref.reference on S0 with
tau_ref, the motor model evaluated in float64 on the host from the same command.  Over the envs step_readout_ref.kept keeps (at least 90 %
of every case, asserted; envs the step reports `done` are advanced like the others and are not left out):

  a. step against truth: the velocity words of S1 against the reference's v_next at STEP_BOUNDS -- FACTOR (4) x the deviation of the
     float32 oracle's substep from the float64 oracle's over the same scenes (tests/test_step_readout_host.py measures it on the CPU:
     1.674e-04 at both thresholds), relative to max(1, |v|);
  b. readout against truth under the step's own, saturated torques: every contact_solve output at test_gpu_contact_solve.BOUNDS;
  c. integrator: S1's positions and joint angles are S0's plus dt x S1's own velocities within 2^-23 (|x0| + |dt v|) per word -- one rounded
     product of magnitude |dt v| and one rounded sum of magnitude at most |x0| + |dt v|, each half a unit in the last place, fused or not,
     with dt the float32 the config carries.  The quaternion against kinematics_ref.advance, normalised, within QUAT_TOL = 12 x 2^-24: the
     four-term sums n_k = dw q_k + ... of csrc/rex_device.h (products and partial sums of magnitude <= 1.26, 4.9 x 2^-24); the squared norm
     (4 x 2^-24 relative, half of it after the root), rsqrtf (one unit in the last place, 2 x 2^-24) and the final product (2^-24): 5 x
     2^-24 along q; and the errors of sincos_fast (~1 ulp), of |w| and of the quotient sh / |w|, which enter scaled by sin(angle / 2) <=
     0.087 at the +-100 rad/s clamp: under 2 x 2^-24 together;
  d. contact_solve leaves the state's bits alone; the step adds 1 to REX_S_STEPS, keeps REX_S_EPISODE and the motor mask, sets REX_F_DONE
     where it returns done, counts the overheat words by |tau| > 2.45 N m, and moves the velocities of every env.

b. splits the columns: the synthetic ones are held to test_gpu_contact_solve.BOUNDS, the leading real ones -- the robot standing on all eight
toe points, 60 sweeps short of resolving its redundant rows, a family whose float32 floor the CPU test measures at 7.40e-04 (toe_force)
and 5.45e-04 (v_next) -- to REAL_BOUNDS below.

Worst values seen on the MI355X (a: bound 6.696e-04; b: toe_force, toe_lambda, limit_torque, v_next; c: in units of the tolerance; 4 envs
per wave unless said otherwise; profiles/step_readout.md has the CPU side):

    case                      kept     a. synthetic  a. real    b. synthetic                             b. real (force, v_next)  c. pos, q, quat
    5 plane                   5/5      1.98e-06      4.93e-05   0, 0, 0, 3.49e-06                        7.62e-04, 3.79e-05       0.32 0.46 0.08
    130 plane                 130/130  8.29e-06      4.96e-05   3.62e-05, 3.62e-05, 4.43e-06, 1.10e-05   7.97e-04, 3.68e-05       0.47 0.48 0.12
    67 random                 67/67    6.59e-05      5.30e-04   1.18e-04, 1.19e-04, 4.96e-06, 2.12e-04   1.10e-04, 5.45e-04       0.46 0.48 0.10
    67 custom, threshold 0    66/67    3.09e-04      4.30e-05   2.57e-04, 2.57e-04, 3.86e-06, 3.69e-04   1.27e-05, 9.24e-06       0.47 0.49 0.14
    67 custom, 1e-7           66/67    3.09e-04      4.31e-05   2.57e-04, 2.57e-04, 3.86e-06, 3.69e-04   1.29e-05, 9.46e-06       0.47 0.50 0.14
    67 custom, 4 per wave     66/67    3.087e-04     4.297e-05  (the readout does not depend on it)                               0.47 0.49 0.14
    67 custom, 8 per wave     66/67    3.087e-04     4.297e-05
    67 custom, 16 per wave    66/67    2.845e-04     4.290e-05
    67 custom, 64 per wave    66/67    3.594e-04     4.294e-05
    67 plane, actuators       67/67    8.42e-06      4.83e-05   1.40e-05, 1.40e-05, 2.00e-06, 9.01e-06   8.17e-04, 3.66e-05       0.48 0.48 0.13
    67 plane, latency 1.3 ms           5.60e-06      5.01e-05   (4 per wave; 64: 6.31e-06, 4.99e-05)                              0.46 0.47 0.12
    67 plane, latency 97.7 ms          6.92e-06      5.01e-05   (64 per wave: 4.78e-06, 4.99e-05)                                 0.46 0.49 0.11
    67 custom, latency 1.3 ms          5.56e-05      4.36e-05                                                                     0.46 0.49 0.14
    67 custom, latency 97.7 ms         5.56e-05      4.36e-05                                                                     0.47 0.48 0.12

The latency rows (test_physics_under_the_delayed_torque): pd_latency / control_latency on, latency_ref.make_ring(S0) in env.history; tau
is the motor model's on the PD-delayed joint angles and rates and the true rates of S0.  With the reference under the torque of the undelayed
reading a. reads 2.4e-02 .. 2.0e-01 (median), with the delayed rate taken for the true one 1.5e-03 .. 3.6e-02.

With the reference wrong on purpose a. reads 1.3e-01 (friction 0.5 for the env's own), 7.2e-02 (mass scales 1), 1.0e-01 (base and leg scale
swapped), 2.3 (the pool's next field), 1.9e-02 (the torque off by 1 %)."""
import numpy as np
import pytest

import contact_solve_ref as cr
import kinematics_ref as kr
import latency_ref as lr
import step_readout_ref as sr
import test_gpu_contact_solve as tc
import test_gpu_kinematics as tk

pytestmark = pytest.mark.gpu

FACTOR = 4.0
STEP_BOUNDS = {0.0: 6.696e-04, cr.THRESHOLD: 6.696e-04}
# b. on the leading real columns: the readout bounds as they stood before the grid constants of the reference were mended (they have gone down
# since, for the synthetic family they are measured over).  The real columns are another family -- a robot standing on all eight toe points,
# the solve of its redundant contact rows not converged after 60 sweeps -- whose own float32 floor is larger than either
# (tests/test_step_readout_host.py measures it: toe_force 7.40e-04, v_next 5.45e-04), so 4 x that floor would allow more than these do.
REAL_BOUNDS = {"toe_force": 1.388e-03, "toe_lambda": 1.113e-03, "limit_torque": tc.BOUNDS["limit_torque"], "v_next": 6.340e-04}
ULP = 2.0 ** -23
QUAT_TOL = 12 * 2.0 ** -24
OVERHEAT_TORQUE = 2.45
S_FLAGS, S_STEPS, S_EPISODE, S_MOTOR_EN, S_OVERHEAT = 43, 44, 45, 46, 47          # include/rexsim.h, mark base
F_DONE = 16


def motor_tau_gpu(env, cmd, S0, params=None, seen=None):
    """rex_motor_torque (params None: the config's gains) or rex_motor_torque_params on (cmd, q0, qd0, qd0) -> tau [n, 12] on the device;
    seen: (q, qd) [n, 12] device tensors, what the PD loop sees under the latency model, in place of the first q0, qd0"""
    import torch
    from rex_gym_amd import _lib
    n = env.num_envs
    qd = S0[25:37].t().contiguous()
    q, qd_seen = (S0[13:25].t().contiguous(), qd) if seen is None else (seen[0].contiguous(), seen[1].contiguous())
    cmd = cmd.contiguous()
    act, obs = torch.zeros_like(cmd), torch.zeros_like(cmd)
    if params is None:
        _lib.check(env._L.rex_motor_torque(12 * n, cmd.data_ptr(), q.data_ptr(), qd_seen.data_ptr(), qd.data_ptr(), float(env.config.motor_kp),
                                           float(env.config.motor_kd), act.data_ptr(), obs.data_ptr(), env._stream_ptr()), "rex_motor_torque")
    else:
        par = np.zeros((n, 12, 5), np.float32)                 # kp, kd, voltage, damping, strength per problem
        for k, name in enumerate(("kp", "kd", "voltage", "damping")):
            par[:, :, k] = params[name][:, None]
        par[:, :, 4] = params["strength"].T
        par = tc.dev(env, par)
        _lib.check(env._L.rex_motor_torque_params(12 * n, cmd.data_ptr(), q.data_ptr(), qd_seen.data_ptr(), qd.data_ptr(), par.data_ptr(),
                                                  act.data_ptr(), obs.data_ptr(), env._stream_ptr()), "rex_motor_torque_params")
    torch.cuda.synchronize()
    return act


class Case:
    """one case run end to end; `share`: a Case of the same scene whose S0 (and what the reference says about S0 alone) is reused;
    `latency`: (pd, control) [s] -- the latency model on, latency_ref.make_ring(S0) in env.history under latency_ref.cursors: the PD loop sees
    the delayed joint angles and rates, the back-EMF the true rates (tests/test_gpu_latency.py has the ring's own checks)"""

    def __init__(self, n, ground, thr, motor=False, share=None, latency=None):
        import torch
        self.n, self.ground, self.thr = n, ground, thr
        lat = {} if latency is None else dict(pd_latency=latency[0], control_latency=latency[1])
        self.env = env = tk.make_env("base", n, ground, solver_residual_threshold=thr, check_actions=False, **lat, **sr.STEP_KW)
        assert env.config.action_repeat == 1 and env.config.solver_iterations == cr.ITERATIONS and env.config.auto_reset == 0
        assert env.config.max_episode_steps == 0 and env.config.sim_time_step == np.float32(cr.DT)
        self.epw = env._L.rex_envs_per_wave(env._h)
        self.kinds = tc.write_states(env, n, ground)
        bp = sr.body_params(n)
        env.set_body_params(base_mass_scale=bp[0], leg_mass_scale=bp[1], foot_friction=bp[2])
        self.params = sr.motor_params(n) if motor else None
        if motor:
            env.set_motor_params(**self.params)
        if share is not None:
            env.state.copy_(share.S0)
        seen = None
        if latency is not None:
            heads, lengths = lr.cursors(n, int(latency[0] / lr.DT), int(latency[1] / lr.DT))
            ring = lr.make_ring(env.state.cpu().numpy(), lr.RING_SEED, heads)
            env.history.copy_(torch.as_tensor(ring.reshape(env.history.shape), device=env.device))
            env.state.view(torch.int32)[lr.hist_word()] = torch.as_tensor(lr.cursor(heads, lengths), device=env.device)
            R0 = env.history.clone()
            seen = lr.delayed_batch(ring, heads, lengths, latency[0], lr.DT)[0:24]            # float64 [24, n]: q, qd as the PD loop sees them
        S0 = self.S0 = env.state.clone()
        _, _, done, info = env.step(tc.dev(env, sr.actions(n)))
        torch.cuda.synchronize()
        self.S1, self.cmd, self.done = env.state.clone(), info["action"].clone(), done.cpu().numpy().astype(bool)
        env.state.copy_(S0)
        if latency is not None:
            env.history.copy_(R0)
        torch.cuda.synchronize()
        assert torch.equal(tc.bits(env.state), tc.bits(S0))
        self.s0, self.s1 = S0.cpu().numpy(), self.S1.cpu().numpy()
        assert np.all(self.s0[S_MOTOR_EN].view(np.int32) == sr.ALL_MOTORS)
        self.seen = seen
        self.tau = motor_tau_gpu(env, self.cmd, S0, self.params, None if seen is None else (tc.dev(env, seen[0:12].T), tc.dev(env, seen[12:24].T)))
        self.con = env.contact_solve(tau=self.tau)
        torch.cuda.synchronize()
        self.untouched = torch.equal(tc.bits(env.state), tc.bits(S0))
        self.gpu = tc.to_numpy(self.con)
        # the float64 reference on S0 under tau_ref
        heights = env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = env.terrain_mids.cpu().numpy() if ground != "plane" else None
        fields = kr.scene_fields(ground, heights, mids)
        ep = self.s0[S_EPISODE].view(np.int32)
        cmd = self.cmd.cpu().numpy()
        p = self.params
        self.rows, self.geometry, self.ok, self.tau_ref = [], [], np.zeros(n, bool), np.zeros((n, 12))
        self.again = []                                        # per env: the reference on S0 under another torque
        for g in range(n):
            fld = kr.field_of(fields, g, ep[g])
            if motor:
                tau = sr.motor_tau_params(cmd[g], self.s0, g, float(p["voltage"][g]), float(p["damping"][g]), float(p["kp"][g]), float(p["kd"][g]), p["strength"][:, g])
            else:
                obs = {} if seen is None else dict(q_obs=seen[0:12, g], qd_obs=seen[12:24, g])
                tau = sr.motor_tau(cmd[g], self.s0, g, float(env.config.motor_kp), float(env.config.motor_kd), **obs)
            dyn = share.rows[g]["dyn"] if share is not None else None
            ref = cr.reference(self.s0, g, fld, (bp[0, g], bp[1, g]), float(bp[2, g]), tau, residual_threshold=sr.threshold32(thr), dyn=dyn)
            self.again.append(lambda tau, g=g, fld=fld: cr.reference(self.s0, g, fld, (bp[0, g], bp[1, g]), float(bp[2, g]), tau,
                                                                    residual_threshold=sr.threshold32(thr), dyn=self.rows[g]["dyn"]))
            geometry = share.geometry[g] if share is not None else cr.compared(self.s0, g, fld, ref, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"])
            self.rows.append(ref)
            self.tau_ref[g] = tau
            self.ok[g] = geometry and not np.any(np.abs(ref["v_next"]) >= cr.MAX_VEL)
            self.geometry.append(geometry)

    def worst(self):
        """-> (synthetic, real): per family of columns a dict, per check the worst value over the kept envs and the env it belongs to"""
        out = {False: {k: (0.0, -1, "") for k in ("step",) + cr.FIELDS}, True: {k: (0.0, -1, "") for k in ("step",) + cr.FIELDS}}
        for g in np.nonzero(self.ok)[0]:
            e = dict(step=sr.vel_error(self.s1[sr.VEL_WORDS, g], self.rows[g]["v_next"]))
            e.update(cr.errors({k: self.gpu[k][g] for k in cr.FIELDS}, self.rows[g]))
            family = out[self.kinds[g] == "real"]
            for k, v in e.items():
                if not v <= family[k][0]:
                    family[k] = (v, int(g), self.kinds[g])
        return out[False], out[True]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, ground, thr, motor=False, epw=None, latency=None):
        key = (n, ground, thr, motor, epw) + (() if latency is None else (latency,))
        if key not in made:
            share = made.get((67, "custom", 0.0, False, None)) if (n, ground) == (67, "custom") else None
            if latency is not None:
                share = get(n, ground, 0.0)
            made[key] = Case(n, ground, thr, motor, share, latency)
        return made[key]
    yield get
    for c in made.values():
        c.env.close()


def check(c, label):
    """the assertions a. .. d. of the module docstring on one case"""
    n, dt = c.n, float(np.float32(cr.DT))
    s0, s1 = c.s0.astype(np.float64), c.s1.astype(np.float64)
    bound = STEP_BOUNDS[c.thr]
    w, real = c.worst()
    print(label, "envs per wave %d, kept %d of %d, done %d" % (c.epw, c.ok.sum(), n, c.done.sum()))
    print("   a. step v / bound: synthetic %.3e, real %.3e / %.3e (envs %d, %d)" % (w["step"][0], real["step"][0], bound, w["step"][1], real["step"][1]))
    print("   b. readout / bound, synthetic", {k: "%.3e / %.3e" % (w[k][0], tc.BOUNDS[k]) for k in cr.FIELDS})
    print("   b. readout / bound, real     ", {k: "%.3e / %.3e" % (real[k][0], REAL_BOUNDS[k]) for k in cr.FIELDS})
    # c. the integrator, every env
    move = dt * s1[sr.VEL_WORDS]
    e_pos = np.abs(s1[0:3] - (s0[0:3] + move[0:3])) / (ULP * (np.abs(s0[0:3]) + np.abs(move[0:3])) + 1e-300)
    e_q = np.abs(s1[13:25] - (s0[13:25] + move[6:18])) / (ULP * (np.abs(s0[13:25]) + np.abs(move[6:18])) + 1e-300)
    e_quat = np.array([sr.integrator_errors(s0, s1, g, dt)[1] for g in range(n)]) / QUAT_TOL
    print("   c. integrator in units of the tolerance: pos %.3f, q %.3f, quat %.3f" % (e_pos.max(), e_q.max(), e_quat.max()))
    if c.thr > 0:
        print("   sweeps of contact_solve at threshold %g:" % c.thr, {int(k): int(v) for k, v in zip(*np.unique(c.gpu["sweeps"], return_counts=True))})
    assert c.ok.sum() >= 0.9 * n, (c.ok.sum(), n)
    assert w["step"][0] <= bound and real["step"][0] <= bound, ("a", w["step"], real["step"])
    assert all(w[k][0] <= tc.BOUNDS[k] for k in cr.FIELDS), ("b", {k: w[k] for k in cr.FIELDS if not w[k][0] <= tc.BOUNDS[k]})
    assert all(real[k][0] <= REAL_BOUNDS[k] for k in cr.FIELDS), ("b, real", {k: real[k] for k in cr.FIELDS if not real[k][0] <= REAL_BOUNDS[k]})
    assert e_pos.max() <= 1.0 and e_q.max() <= 1.0 and e_quat.max() <= 1.0, ("c", e_pos.max(), e_q.max(), e_quat.max())
    assert np.all(np.abs(np.linalg.norm(s1[3:7], axis=0) - 1.0) <= 5 * 2.0 ** -24)           # the normalisation's share of QUAT_TOL
    # d. untouched words and counters
    assert c.untouched
    i0, i1 = c.s0.view(np.int32), c.s1.view(np.int32)
    assert np.array_equal(i1[S_STEPS], i0[S_STEPS] + 1) and np.array_equal(i1[S_EPISODE], i0[S_EPISODE]) and np.array_equal(i1[S_MOTOR_EN], i0[S_MOTOR_EN])
    assert np.array_equal((i1[S_FLAGS] & F_DONE) != 0, c.done | ((i0[S_FLAGS] & F_DONE) != 0))
    assert np.all(np.any(c.s1[sr.VEL_WORDS] != c.s0[sr.VEL_WORDS], axis=0)) and np.any(c.s1[0:3] != c.s0[0:3], axis=0).sum() >= 0.9 * n
    tau = np.abs(c.tau.cpu().numpy().astype(np.float64))                                     # [n, 12]
    heat0 = np.stack([i0[S_OVERHEAT + j // 2].view(np.uint32) >> (16 * (j % 2)) & 0xFFFF for j in range(12)], axis=1).astype(np.int64)
    heat1 = np.stack([i1[S_OVERHEAT + j // 2].view(np.uint32) >> (16 * (j % 2)) & 0xFFFF for j in range(12)], axis=1).astype(np.int64)
    clear = np.abs(tau - OVERHEAT_TORQUE) > 1e-4
    assert np.array_equal(heat1[clear], np.where(tau > OVERHEAT_TORQUE, heat0 + 1, 0)[clear]) and (tau > OVERHEAT_TORQUE).any() and clear.mean() > 0.99
    # the torques the step drew are saturated ones: new loads for the readout
    assert (np.abs(c.tau_ref) > 3.0).any() and np.abs(c.tau_ref - c.tau.cpu().numpy()).max() <= 2e-5 * 1.3 + 1e-5 * 3.5 * 1.3


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("n,ground,thr", [(5, "plane", 0.0), (130, "plane", 0.0), (67, "random", 0.0), (67, "custom", 0.0), (67, "custom", cr.THRESHOLD)],
                         ids=["5-plane", "130-plane", "67-random", "67-custom", "67-custom-default_threshold"])
def test_step_and_readout_on_one_state(cases, n, ground, thr):
    check(cases(n, ground, thr), (n, ground, thr))


@pytest.mark.parametrize("epw", [4, 8, 16, 64])
def test_every_solver_layout_from_the_same_state(cases, monkeypatch, epw):
    """REX_ENVS_PER_WAVE 4 / 8 / 16 / 64: the four solver layouts of the step kernels, from the S0 of the default case, each held to a. .. d."""
    import torch
    base = cases(67, "custom", 0.0)
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = cases(67, "custom", 0.0, epw=epw)
    assert c.epw == epw and torch.equal(tc.bits(c.S0), tc.bits(base.S0))
    check(c, (67, "custom", 0.0, "epw %d" % epw))


def test_heterogeneous_actuators(cases):
    """set_motor_params with per-env voltage, damping, kp, kd and a strength row per motor on (67, plane): the _mseg instantiations of the
    step, with tau from rex_motor_torque_params"""
    c = cases(67, "plane", 0.0, motor=True)
    plain = sr.motor_tau(c.cmd.cpu().numpy()[10], c.s0, 10)
    assert np.abs(plain - c.tau_ref[10]).max() > 0.05                     # the parameters do enter
    check(c, (67, "plane", 0.0, "actuators"))


@pytest.mark.parametrize("epw", [4, 64])
@pytest.mark.parametrize("ground", ["plane", "custom"])
@pytest.mark.parametrize("latency", [(0.0013, 0.0037), (0.0977, 0.0985)], ids=["1.3ms", "97.7ms"])
def test_physics_under_the_delayed_torque(cases, monkeypatch, latency, ground, epw):
    """The latency model on (check C of tests/test_gpu_latency.py): the torque the step draws is the motor model's on the PD-delayed joint
    angles and rates and the TRUE rates of S0 -- a. .. d. unchanged, the overheat counters counting the actual torque.  Teeth: the float64
    reference under the torque of the undelayed reading, and of the delayed rate taken for the true one, misses a."""
    base = cases(67, ground, 0.0)
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = cases(67, ground, 0.0, epw=epw, latency=latency)
    assert c.epw == epw and np.array_equal(c.s0[0:lr.hist_word()].view(np.int32), base.s0[0:lr.hist_word()].view(np.int32))
    assert c.env.config.pd_latency == np.float32(latency[0]) and c.env.history is not None
    check(c, (67, ground, 0.0, "epw %d" % epw, "latency", latency))
    cmd, kp, kd = c.cmd.cpu().numpy().astype(np.float64), float(c.env.config.motor_kp), float(c.env.config.motor_kd)
    q0, qd0 = c.s0[13:25].astype(np.float64), c.s0[25:37].astype(np.float64)
    wrong = {"undelayed": sr.motor_model(cmd.T, q0, qd0, qd0, kp=kp, kd=kd)[0].T,
             "delayed rate as the true one": sr.motor_model(cmd.T, c.seen[0:12], c.seen[12:24], c.seen[12:24], kp=kp, kd=kd)[0].T}
    some = np.nonzero(c.ok)[0][::5]                                           # every fifth kept env: the reference once more, under the wrong torque
    for name, tau in wrong.items():
        e = np.array([sr.vel_error(c.s1[sr.VEL_WORDS, g], c.again[g](tau[g])["v_next"]) for g in some])
        print("   teeth, %s: a. reads %.1e (median), over the bound in %d of %d envs" % (name, np.median(e), (e > STEP_BOUNDS[c.thr]).sum(), len(some)))
        # (1.3 ms: the rates move by a few tenths of a rad/s between the two blended entries; the delayed rate shows in about half the envs)
        assert (e > STEP_BOUNDS[c.thr]).mean() >= 0.5 or (name != "undelayed" and latency[0] < 0.01)
