"""The latency model on the GPU (MI355X), held to the contents of the ring: hist_at, delay_slots, delayed_word, receive_observation,
control_observation and the PD read of rex_substep (csrc/rex_kernels.h) and the host's pd_slots / pd_alpha (csrc/rexsim.hip) against the
float64 blend of tests/latency_ref.py, which tests/test_latency_host.py holds to the reference's own Rex._GetDelayedObservation.

The ring is a caller-owned device buffer (env.history, [slot][word][env]) and the cursor a caller-writable state word (REX_S_HIST: head in
bits 0-7, length in bits 8-15), so no trajectory is needed.  Per case (class Run): an env of step_readout_ref.STEP_KW (action_repeat 1,
control time step 0.001 s, 60 sweeps, auto-reset off, no episode limit: one step() is one substep) unless said otherwise; reset, 8
random steps; the joint angles are placed within 0.25 rad of the motor command the step will issue (taken from a dry step) and the joint
rates clipped to +-10 rad/s (under a PD latency of 98 ms the reset motion leaves the joints far from the command and fast: on the flat
ends of the motor model, where no reading shows); all but the first three envs get the orientations and angular rates of latency_ref.tilted_states (tilts of up to 1.2 rad,
the base lifted so that the lowest toe point is 2 cm over the ground); latency_ref.make_ring(S0) -- 100 entries that all differ, the newest
one S0's own -- is written into env.history and latency_ref.cursors into REX_S_HIST: heads cycle through 0, 1, 42, 98, 99 (the two
blended slots wrap through 99 -> 0), every second env has length 100, the only length the product itself produces, the others cycle
through 1, 2, n_pd + 1, n_pd + 2, n_c + 1, n_c + 2, 100 -- short lengths exercise the branches of delay_slots (`len == 1`, `n + 1 >= len`)
that the reset motion, 600 observations long, never leaves behind.  S0 and R are cloned, one step with seeded actions is taken, S1, R',
obs, reward and info["action"] are read back.  r: the substeps of the step (1; 5 or 6 in G and in a mixed batch).

  A. ring integrity, every env, bitwise: REX_S_HIST of S1 is (head + r) % 100 | min(len + r, 100) << 8; the newest slot of R' holds S1's q,
     qd, quaternion and angular velocity; every slot of R' but the r new ones equals R (padding lanes, ragged last waves, stray owners).
     One case passes its ring with rex_set_history as an offset pointer into a larger allocation: the 64 guard words on each side keep their
     bits.
  B. the PD-delayed observation through the observed torque: the torque words of every new entry against the motor model's observed torque
     (motor.py:127-129: clip(Kt pwm V / R, +-5.7) with pwm = clip(kp (cmd - q_pd) - kd qd_pd, +-1)) in float64 on the blend of the ring as
     it stood before that substep (R with the earlier new entries of R'), under the cursor of that substep.  Tolerance: the project's motor
     tolerance, atol 2e-5, rtol 1e-5 (test_motor_kernel_vs_reference_golden).  The float32 blend's share of it: three
     roundings of half a unit in the last place on |q| <= 1.6 rad, 3 x 2^-25 x 1.6 = 1.4e-7 rad, times Kt V / R = 16.4 N m per unit of pwm
     at kp 1: 2.4e-6 N m; on |qd| <= 8 rad/s 7e-7 rad/s times kd x 16.4 = 0.33: 2.4e-7 N m.  No (env, motor) pair is left out.  The
     observed torque does not depend on the true joint rate (motor.py:127), so the true rate is held by C, not here.
  D. the control-delayed observation: the float64 blend of R' under the cursor of S1, both read back from the device (D does not depend
     on B).  obs[2], obs[3] (the blended w[0], w[1]) and, gallop, obs[4:16] (the blended q, which make_ring keeps inside (-pi, pi))
     within 4 x 2^-24 x (|x| + |y|) per word, x and y the two blended entries: one rounding of 1 - alpha, two products and one sum, each
     half a unit in the last place of a magnitude of at most |x| + |y|, fused or not.  In 8 further envs of the gallop case every q of the
     ring lies just past +-pi, so that MapToMinusPiToPi acts: held to 2e-6, the float32 2 pi.  obs[0], obs[1] (roll, pitch of the blended,
     unnormalised quaternion) within FACTOR (4) x the float32 floor tests/test_latency_host.py measures on the same rings: roll 2.306e-07,
     pitch 3.889e-07 rad -> bounds 9.224e-07, 1.556e-06.
  E. the torque words on the control path, through the reward's energy term: envs 2i and 2i + 1 are identical in state, ring, cursor and
     action but for the torque words of the two control slots (which nothing in the physics reads): S1 bit-identical within a pair;
     reward_a - reward_b = w_energy x dt x (|dp_b| - |dp_a|), dp the sum of tau x qd over the blended control record, within
     2^-23 (|r_a| + |r_b|) + 16 x 2^-24 x w_energy x dt x sum |tau x qd| (the smaller sum of the pair); |dp| is in the hundreds.
  F. the turn env's goal test reads the control-delayed yaw, before the substep (R and the cursor of S0): REX_S_TARGET is written so that in
     the first half of the envs the delayed yaw is within 0.004 of it and the state's own at least 0.04 away, in the second half the
     reverse; after the step REX_F_GOAL_REACHED and REX_F_TERMINATING are set and REX_S_ENDTIME is the step word in exactly the first half.
  G. several substeps in one launch (the default walk and gallop configs, action_repeat 5 and 6): A and B for every new entry, with the
     integrator identity q_k = q_(k-1) + dt qd_k within 2^-23 (|q_(k-1)| + |dt qd_k|) between consecutive new entries
     (test_gpu_step_readout's check c.): ring traffic between the lanes of a launch.
  C. (physics under the delayed torque: the actual torque, the true against the delayed joint rate) lives in
     tests/test_gpu_step_readout.py, test_physics_under_the_delayed_torque: its Case with latency=(pd, control).

Teeth (asserted, numpy only, over the envs of length 100 -- for shorter rings several wrong readings coincide with the right one by
construction): the reference of B and D computed wrong on purpose -- alpha <-> 1 - alpha, a read one slot newer, one slot older, PD
and control latency exchanged, the q and qd word blocks exchanged -- must exceed the check's bound in at least half of the compared
entries; for B over the motors with |kp (cmd - q) - kd qd| < 0.7, which are at least 90 % of all (asserted).  (The exchange of alpha
and 1 - alpha is not asserted for D at the control latency 0.0985, whose alpha is 0.5.)

Seen on the MI355X (profiles/latency.md has every case): B at most 0.065 of its tolerance, D 0.22 of its bounds (w 0.223, roll and pitch
0.210, q 0.214, wrapped q 0.195), G 0.493, E 0.276.  The wrong references, walk ik at (0.0013, 0.0037): beyond the bound in every compared
entry, by a median of 8e2 (alpha), 1e3 (a slot newer), 2e3 (a slot older), 3e3 (latencies exchanged), 1e5 (blocks) tolerances in B and
7e4, 1e5, 1e5, 2e5 bounds in D's w, 2e3 .. 5e3 in roll and pitch; the lowest share over all cases is 0.86 (mixed batch, B, blocks)."""
import numpy as np
import pytest

import kinematics_ref as kr
import latency_ref as lr
import step_readout_ref as sr
import test_gpu_contact_solve as tc
import test_gpu_render as col

pytestmark = pytest.mark.gpu

FACTOR = 4.0
MOTOR_ATOL, MOTOR_RTOL = 2e-5, 1e-5
EULER_BOUND = FACTOR * np.array(lr.EULER_FLOOR)
WRAP_BOUND = 2e-6
ULP = 2.0 ** -23
W_ENERGY = {"gallop": 0.005, "walk": 0.0005}
REPEAT = {"walk": 5, "gallop": 6}
S_TARGET, S_ENDTIME, S_FLAGS, S_STEPS = 40, 41, 43, 44                      # include/rexsim.h, mark base
F_GOAL, F_TERMINATING, F_STAY = 1, 2, 4
GUARD, SENTINEL = 64, -12345.5
KEEP = 3                                                                    # leading envs that keep their own orientation
MAIN = (0.0013, 0.0037)
TEETH_B = ("alpha", "n-1", "n+1", "exchanged", "blocks")


def yaw_rotated(q, delta):
    """the quaternion (x, y, z, w) [4] turned by `delta` about the world's z axis, float64"""
    a = np.array([0.0, 0.0, np.sin(delta / 2), np.cos(delta / 2)])
    return kr._quat_mul(a, np.asarray(q, np.float64))


class Run:
    """one case end to end; see the module docstring.  pairs: E's twin envs; turn: F's targets; near_pi: that many trailing envs whose ring
    holds joint angles just past +-pi; guard: the ring inside a larger allocation; step_kw False: the task's own action_repeat"""

    def __init__(self, pd, ctl, n=67, task="walk", signal="ik", mark="base", step_kw=True, params=False, near_pi=0, guard=False, pairs=False,
                 turn=False, **kw):
        import torch
        from rex_gym_amd import RexBatchEnv, _lib
        self.pd, self.ctl, self.n, self.task, self.near_pi, self.guard = pd, ctl, n, task, near_pi, guard
        extra = dict(sr.STEP_KW) if step_kw else {}
        extra.update(kw)
        env = self.env = RexBatchEnv(n, task=task, signal_type=signal, mark=mark, seed=5, check_actions=False, pd_latency=pd, control_latency=ctl,
                                     **extra)
        nm = self.nm = env.num_motors
        arm, W, hw = nm == 18, lr.words(nm), lr.hist_word(nm)
        assert hw == env.state_words - 1 and tuple(env.history.shape) == (lr.LEN * W, n)
        assert env.config.sim_time_step == np.float32(lr.DT) and env.config.auto_reset == 0 and env.config.max_episode_steps == 0
        self.epw = env._L.rex_envs_per_wave(env._h)
        if guard:
            self.big = torch.full((GUARD + lr.LEN * W * n + GUARD,), SENTINEL, dtype=torch.float32, device=env.device)
            env.history = self.big[GUARD:GUARD + lr.LEN * W * n].view(lr.LEN * W, n)
            _lib.check(env._L.rex_set_history(env._h, env.history.data_ptr()), "rex_set_history")
        env.reset()
        col._steps(env, 8, seed=2)
        self.params = None
        if params:
            self.params = sr.motor_params(n)
            env.set_motor_params(**self.params)
        torch.cuda.synchronize()
        twins = np.arange(n)
        if pairs:
            twins[1:2 * (n // 2):2] -= 1
        lo, hi = np.minimum(env.action_space.low, env.action_space.high), np.maximum(env.action_space.low, env.action_space.high)
        act = tc.dev(env, np.random.RandomState(77 + n).uniform(lo, hi, (n, env.action_dim)).astype(np.float32)[twins])
        # ---- the motor command the step will issue (it does not depend on what is written below): a dry step, then the state and ring back
        if pairs:
            idx = torch.as_tensor(twins, device=env.device)
            env.state.copy_(env.state[:, idx])
            env.history.copy_(env.history[:, idx])
        S_real, R_real = env.state.clone(), env.history.clone()
        cmd0 = env.step(act)[3]["action"].clone()
        env.state.copy_(S_real)
        env.history.copy_(R_real)
        torch.cuda.synchronize()
        # ---- S0: joint angles around the command, tilted orientations, E's twins, D's joints past +-pi
        s = env.state.cpu().numpy().copy()
        rng = np.random.RandomState(100 + n)
        if not turn:
            s[13:13 + nm] = cmd0.cpu().numpy().T + rng.uniform(-0.25, 0.25, (nm, n)).astype(np.float32)
            s[13 + nm:13 + 2 * nm] = np.clip(s[13 + nm:13 + 2 * nm], -10.0, 10.0)
        T = lr.tilted_states(n, lr.TILT_SEEDS[n])
        s[3:7, KEEP:], s[10:13, KEEP:] = T[3:7, KEEP:], T[10:13, KEEP:]
        for g in range(KEEP, n):
            r = kr.reference(s, g, arm, None)
            s[2, g] += np.float32(0.02 - float((r["toe_dist"] / r["toe_normal"][:, 2]).min()))
        if pairs:
            s = s[:, twins]
        n_pd, n_c = int(pd / lr.DT), int(ctl / lr.DT)
        heads, lengths = lr.cursors(n, n_pd, n_c)
        if pairs:
            heads, lengths = heads[twins], np.maximum(lengths[twins], 2)
        if turn:
            lengths = np.maximum(lengths, n_c + 1)
        rb, sb = lr.blocks(nm), lr.state_blocks(nm)
        R = lr.make_ring(s, lr.RING_SEED, heads, nm)
        for g in range(n - near_pi, n):
            R[:, rb["q"], g] = ((1 if g % 2 else -1) * (np.pi + rng.uniform(0.002, 0.1, (lr.LEN, nm)))).astype(np.float32)
            s[sb["q"], g] = R[heads[g], rb["q"], g]
        if pairs:
            R = R[:, :, twins]
            for g in range(0, 2 * (n // 2), 2):
                h1, l1 = lr.received(heads[g], lengths[g])
                k0, k1, _ = lr.slots(ctl, lr.DT, int(l1))
                assert k0 >= 1
                for k in {k0, k1}:
                    sl = (h1 - k) % lr.LEN
                    sign = rng.choice([-1.0, 1.0], nm)
                    R[sl, rb["qd"], g] = R[sl, rb["qd"], g + 1] = (sign * rng.uniform(20, 30, nm)).astype(np.float32)
                    R[sl, rb["tau"], g] = (sign * rng.uniform(2, 3, nm)).astype(np.float32)
                    R[sl, rb["tau"], g + 1] = (rng.choice([-1.0, 1.0], nm) * rng.uniform(0.5, 3, nm)).astype(np.float32)
        if turn:
            for g in range(n):
                for k in range(1, lr.LEN):
                    R[(heads[g] - k) % lr.LEN, rb["quat"], g] = yaw_rotated(s[3:7, g], 0.06 + 0.002 * k).astype(np.float32)
            cz = lambda yaw: np.where(yaw < 0, yaw + 6.28, yaw)
            d = lr.delayed_batch(R, heads, lengths, ctl, lr.DT)
            self.cz_delayed, self.cz_own = cz(lr.quat_to_euler(d[rb["quat"]])[2]), cz(lr.quat_to_euler(s[3:7])[2])
            self.first = np.arange(n) < n // 2
            s[S_TARGET] = (np.where(self.first, self.cz_delayed, self.cz_own) + 0.004 * (-1.0) ** np.arange(n)).astype(np.float32)
            flags = s[S_FLAGS].view(np.int32)
            flags &= ~(F_GOAL | F_TERMINATING | F_STAY)
        self.heads, self.lengths = heads, lengths
        env.state.copy_(torch.as_tensor(s, device=env.device))
        env.state.view(torch.int32)[hw] = torch.as_tensor(lr.cursor(heads, lengths), device=env.device)
        env.history.copy_(torch.as_tensor(R.reshape(lr.LEN * W, n), device=env.device))
        torch.cuda.synchronize()
        S0, R0 = env.state.clone(), env.history.clone()
        obs, reward, done, info = env.step(act)
        torch.cuda.synchronize()
        assert turn or torch.equal(tc.bits(info["action"]), tc.bits(cmd0))
        self.s0, self.s1 = S0.cpu().numpy(), env.state.cpu().numpy()
        self.r0, self.r1 = R0.cpu().numpy().reshape(lr.LEN, W, n), env.history.cpu().numpy().reshape(lr.LEN, W, n)
        assert np.array_equal(self.r0.view(np.int32), R.view(np.int32)) and np.array_equal(self.s0[:hw].view(np.int32), s[:hw].view(np.int32))
        self.obs, self.reward, self.cmd = obs.cpu().numpy().astype(np.float64), reward.cpu().numpy().astype(np.float64), info["action"].cpu().numpy()
        self.head1, self.len1 = lr.uncursor(self.s1[hw].view(np.int32))
        if task == "mixed":
            from rex_gym_amd import _lib as L
            ids = env.task_ids().cpu().numpy()
            self.tasks = np.array([{L.TASKS[t]: t for t in env.tasks}[int(i)] for i in ids])
            self.rep = np.array([REPEAT[t] for t in self.tasks])
        else:
            self.tasks = np.array([task] * n)
            self.rep = np.full(n, env.config.action_repeat)
        self.kp, self.kd = float(env.config.motor_kp), float(env.config.motor_kd)

    def ring_before(self, k):
        """the rings as they stood before substep k (1 ..): R with the new entries 1 .. k - 1 of R'"""
        R = self.r0.copy()
        for g in range(self.n):
            for j in range(1, min(k - 1, self.rep[g]) + 1):
                sl = (self.heads[g] + j) % lr.LEN
                R[sl, :, g] = self.r1[sl, :, g]
        return R

    def label(self):
        return "%s %s n %d, %d per wave, pd %g control %g" % (self.task, "arm" if self.nm == 18 else "base", self.n, self.epw, self.pd, self.ctl)


@pytest.fixture(scope="module")
def runs():
    made = {}

    def get(*key, **kw):
        k = key + tuple(sorted(kw.items()))
        if k not in made:
            made[k] = Run(*key, **{a: v for a, v in kw.items() if a != "epw"})       # (epw: REX_ENVS_PER_WAVE of the caller, part of the key)
        return made[k]
    yield get
    for r in made.values():
        r.env.close()


# ---------------------------------------------------------------- the checks
def check_a(c):
    n, nm = c.n, c.nm
    rb, sb = lr.blocks(nm), lr.state_blocks(nm)
    h1, l1 = lr.received(c.heads, c.lengths, c.rep)
    assert np.array_equal(c.head1, h1) and np.array_equal(c.len1, l1), ("A cursor", c.label())
    b0, b1, s1 = c.r0.view(np.int32), c.r1.view(np.int32), c.s1.view(np.int32)
    for g in range(n):
        for name in ("q", "qd", "quat", "w"):
            assert np.array_equal(b1[h1[g], rb[name], g], s1[sb[name], g]), ("A newest entry", name, g, c.label())
        old = np.ones(lr.LEN, bool)
        old[(c.heads[g] + 1 + np.arange(c.rep[g])) % lr.LEN] = False
        assert np.array_equal(b1[old, :, g], b0[old, :, g]), ("A other slots", g, c.label())
        new = c.r1[~old, :, g]
        assert np.all(np.isfinite(new))
    if c.guard:
        big = c.big.cpu().numpy()
        assert np.all(big[:GUARD] == np.float32(SENTINEL)) and np.all(big[-GUARD:] == np.float32(SENTINEL))


def pd_reference(c, k, wrong=None):
    """-> (reference [n, nm], q, qd of the right blend [nm, n]) for the torque words of new entry k"""
    R = c.ring_before(k).astype(np.float64)
    h, l = lr.received(c.heads, c.lengths, k - 1)
    latency = c.ctl if wrong == "exchanged" else c.pd
    ref = lr.pd_torque(c.cmd, R, h, l, latency, lr.DT, c.nm, None if wrong == "exchanged" else wrong, c.params, c.kp, c.kd)
    d = lr.delayed_batch(R, h, l, c.pd, lr.DT)
    return ref, d[lr.blocks(c.nm)["q"]], d[lr.blocks(c.nm)["qd"]]


def check_b(c, teeth=False):
    nm, rb = c.nm, lr.blocks(c.nm)
    worst, margins = 0.0, {}
    for k in range(1, int(c.rep.max()) + 1):
        on = c.rep >= k
        got = np.stack([c.r1[(c.heads[g] + k) % lr.LEN, rb["tau"], g] for g in range(c.n)]).astype(np.float64)      # [n, nm]
        ref, q, qd = pd_reference(c, k)
        tol = MOTOR_ATOL + MOTOR_RTOL * np.abs(ref)
        e = (np.abs(got - ref) / tol)[on]
        worst = max(worst, e.max())
        assert e.max() <= 1.0, ("B", c.label(), "entry", k, np.argwhere((np.abs(got - ref) / tol > 1.0) & on[:, None])[:8], e.max())
        if teeth:
            kp = c.params["kp"].astype(np.float64) if c.params else c.kp
            kd = c.params["kd"].astype(np.float64) if c.params else c.kd
            off_flat = (np.abs(kp * (c.cmd.T - q) - kd * qd) < 0.7).T
            off_flat[c.n - c.near_pi:] = False                                   # (D's envs with every joint past +-pi: not counted)
            assert off_flat[:c.n - c.near_pi].mean() >= 0.9, ("B teeth: motors off the flat end", off_flat.mean())
            full = (on & (c.lengths == lr.LEN))[:, None] & off_flat
            for wrong in TEETH_B:
                bad = np.abs(got - pd_reference(c, k, wrong)[0]) / tol
                margins.setdefault(wrong, []).append(((bad > 1.0) & full).sum() / full.sum())
                margins.setdefault(wrong + " median", []).append(float(np.median(bad[full])))
    print("   B. torque words / tolerance: %.3f" % worst, c.label())
    for wrong in TEETH_B if teeth else ():
        print("      teeth %-10s exceeds in %.2f of the entries, median %.1f x the tolerance" % (wrong, min(margins[wrong]), min(margins[wrong + " median"])))
        assert min(margins[wrong]) >= 0.5, ("B teeth", wrong, margins[wrong])
    return worst


def control_reference(c, wrong=None):
    """-> (the float64 control record [W, n] of R' under S1's cursor, the per-word bound)"""
    latency = c.pd if wrong == "exchanged" else c.ctl
    x, y, al = lr.blend_pair(c.r1.astype(np.float64), c.head1, c.len1, c.ctl, lr.DT)
    if wrong is None:
        return (1.0 - al) * x + al * y, lr.blend_bound(x, y)
    d = lr.delayed_batch(c.r1, c.head1, c.len1, latency, lr.DT, None if wrong in ("exchanged", "blocks") else wrong)
    if wrong == "blocks":
        rb = lr.blocks(c.nm)
        d[rb["q"]], d[rb["qd"]] = d[rb["qd"]].copy(), d[rb["q"]].copy()
    return d, lr.blend_bound(x, y)


def wrapped(q):
    """MapToMinusPiToPi, rex.py:26-41, float64"""
    a = np.fmod(q, 2 * np.pi)
    return np.where(a >= np.pi, a - 2 * np.pi, np.where(a < -np.pi, a + 2 * np.pi, a))


def d_errors(c, wrong=None):
    """-> (dict of error / bound arrays: w [2, n], rp [2, n], q and "q wrapped" [nm, envs], dict of the env behind every column)"""
    nm, rb = c.nm, lr.blocks(c.nm)
    ref, bound = control_reference(c, wrong)
    obs = c.obs.T                                                                    # [obs_dim, n]
    bound = bound + 1e-300
    out, envs = {"w": np.abs(obs[2:4] - ref[rb["w"]][0:2]) / bound[rb["w"]][0:2]}, {"w": np.arange(c.n), "rp": np.arange(c.n)}
    rpy = lr.quat_to_euler(ref[rb["quat"]])
    out["rp"] = np.abs(obs[0:2] - np.stack(rpy[0:2])) / EULER_BOUND[:, None]
    if obs.shape[0] > 4:
        assert obs.shape[0] == 4 + nm
        gallop = c.tasks == "gallop"
        plain = np.arange(c.n) < c.n - c.near_pi
        if wrong is None:
            assert np.all(np.abs(ref[rb["q"]][:, plain]) < np.pi - 1e-3) and np.all(np.abs(ref[rb["q"]][:, ~plain]) > np.pi + 1e-3)
            assert np.all(obs[4:][:, ~gallop] == 0.0)
        qb = np.where(plain[None, :], bound[rb["q"]], WRAP_BOUND)
        e = np.abs(obs[4:] - wrapped(ref[rb["q"]])) / qb
        out["q"], out["q wrapped"] = e[:, gallop & plain], e[:, gallop & ~plain]
        envs["q"], envs["q wrapped"] = np.nonzero(gallop & plain)[0], np.nonzero(gallop & ~plain)[0]
    return out, envs


def check_d(c, teeth=False):
    e, _ = d_errors(c)
    print("   D. control observation / bound:", {k: "%.3f" % v.max() for k, v in e.items() if v.size}, c.label())
    for k, v in e.items():
        assert v.size == 0 or v.max() <= 1.0, ("D", k, c.label(), np.argwhere(v > 1.0)[:8], v.max())
    if teeth:
        full = c.lengths == lr.LEN
        for wrong in TEETH_B:
            if wrong == "alpha" and abs(lr.slots(c.ctl, lr.DT, lr.LEN)[2] - 0.5) < 0.1:       # (control latency 0.0985: the blend is even)
                continue
            bad, envs = d_errors(c, wrong)
            for k in ("w", "q", "rp"):
                if k not in bad or (wrong == "blocks" and k != "q"):
                    continue
                v = bad[k][:, full[envs[k]]]
                print("      teeth %-10s %-2s exceeds in %.2f of the entries, median %.1f x the bound" % (wrong, k, (v > 1.0).mean(), np.median(v)))
                assert (v > 1.0).mean() >= 0.5, ("D teeth", wrong, k, (v > 1.0).mean())
    return e


def check_g(c):
    """the integrator identity between consecutive new entries"""
    rb, dt = lr.blocks(c.nm), float(np.float32(lr.DT))
    worst = 0.0
    for g in range(c.n):
        e = c.r1[(c.heads[g] + np.arange(c.rep[g] + 1)) % lr.LEN, :, g].astype(np.float64)        # entries 0 (S0's) .. r
        q, qd = e[:, rb["q"]], e[:, rb["qd"]]
        move = dt * qd[1:]
        worst = max(worst, (np.abs(q[1:] - (q[:-1] + move)) / (ULP * (np.abs(q[:-1]) + np.abs(move)) + 1e-300)).max())
    print("   G. q_k = q_(k-1) + dt qd_k in units of the tolerance: %.3f" % worst, c.label())
    assert worst <= 1.0, ("G", worst)


def abd(c, teeth=False):
    print(c.label())
    check_a(c)
    check_b(c, teeth)
    check_d(c, teeth)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("pd,ctl", lr.PAIRS)
def test_every_latency_pair(runs, pd, ctl):
    """A, B, D: mark base, walk ik, 67 envs at 4 per wave; teeth at the pairs whose two latencies both blend two entries"""
    c = runs(pd, ctl, guard=(pd, ctl) == MAIN)
    assert c.epw == 4
    abd(c, teeth=(pd, ctl) in lr.PAIRS[:4])


@pytest.mark.parametrize("epw,n", [(8, 67), (16, 67), (64, 130)])
def test_every_layout_of_the_base_group(runs, monkeypatch, epw, n):
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, n=n, epw=epw)
    assert c.epw == epw
    abd(c, teeth=True)


def test_control_observation_of_the_gallop_env(runs):
    """D on 16 entries: gallop, signal ol, 67 + 8 envs, the last 8 with joint angles past +-pi"""
    c = runs(*MAIN, n=75, task="gallop", signal="ol", near_pi=8)
    assert c.obs.shape == (75, 16)
    abd(c, teeth=True)


@pytest.mark.parametrize("epw", [4, 8, 16])
def test_arm_group(runs, monkeypatch, epw):
    """61-word records; the arm's words are written by the `live` lane"""
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, mark="arm", epw=epw)
    assert c.epw == epw and c.nm == 18 and c.r1.shape[1] == 61
    abd(c, teeth=True)


@pytest.mark.parametrize("epw", [4, 8])
def test_link_box_group(runs, monkeypatch, epw):
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, body_contacts=True, epw=epw)
    assert c.epw == epw and c.env.config.body_contacts == 1
    abd(c, teeth=True)


@pytest.mark.parametrize("epw", [4, 8, 16])
def test_mixed_walk_and_gallop_batch(runs, monkeypatch, epw):
    """a mixed batch steps 5 (walk) or 6 (gallop) substeps per env in one launch; rows by state index"""
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, task="mixed", tasks=("walk", "gallop"), step_kw=False, epw=epw)
    assert c.epw == epw and set(c.tasks) == {"walk", "gallop"} and c.obs.shape == (67, 16)
    abd(c, teeth=True)
    check_g(c)


def test_per_env_actuators(runs):
    """set_motor_params: the _mseg instantiations, the reference through the per-env voltage, kp and kd"""
    c = runs(*MAIN, params=True)
    plain = lr.pd_torque(c.cmd, c.r0, c.heads, c.lengths, c.pd, lr.DT)
    mine = lr.pd_torque(c.cmd, c.r0, c.heads, c.lengths, c.pd, lr.DT, params=c.params)
    assert np.abs(plain - mine).max() > 0.05                                 # the parameters do enter
    abd(c, teeth=True)


@pytest.mark.parametrize("epw", [4, 16])
@pytest.mark.parametrize("task,signal", [("gallop", "ol"), ("walk", "ik")])
def test_torque_words_through_the_energy_term(runs, monkeypatch, epw, task, signal):
    """E"""
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, task=task, signal=signal, pairs=True, epw=epw)
    assert c.epw == epw and abs(c.env.config.energy_weight - W_ENERGY[task]) < 1e-9
    check_a(c)
    rb, w, dt = lr.blocks(), W_ENERGY[task], lr.DT
    ref, _ = control_reference(c)
    terms = ref[rb["tau"]] * ref[rb["qd"]]
    dp, mass = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    a, b = np.arange(0, 2 * (c.n // 2), 2), np.arange(1, 2 * (c.n // 2), 2)
    hw = lr.hist_word()
    assert np.array_equal(c.s1[:, a].view(np.int32), c.s1[:, b].view(np.int32)), "E: the twins' states differ"
    assert np.array_equal(c.s0[:, a].view(np.int32), c.s0[:, b].view(np.int32)) and np.array_equal(c.head1[a], c.head1[b]) and hw == 53
    want = w * dt * (np.abs(dp[b]) - np.abs(dp[a]))
    tol = ULP * (np.abs(c.reward[a]) + np.abs(c.reward[b])) + 16 * 2.0 ** -24 * w * dt * np.minimum(mass[a], mass[b])
    err = np.abs((c.reward[a] - c.reward[b]) - want)
    print(c.label(), "E. reward difference / tolerance: %.3f; |dp| %.0f .. %.0f; the term / tolerance: median %.0f" %
          ((err / tol).max(), np.abs(dp[a]).min(), np.abs(dp[a]).max(), np.median(np.abs(want) / tol)))
    assert (err / tol).max() <= 1.0, ("E", np.argwhere(err > tol)[:8], (err / tol).max())
    assert np.abs(dp[a]).min() >= 100 and np.median(np.abs(want) / tol) >= 100


@pytest.mark.parametrize("epw", [4, 16])
def test_turn_goal_reads_the_delayed_yaw(runs, monkeypatch, epw):
    """F"""
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, task="turn", signal="ik", turn=True, epw=epw)
    assert c.epw == epw
    check_a(c)
    target = c.s0[S_TARGET].astype(np.float64)
    near, far = np.where(c.first, c.cz_delayed, c.cz_own), np.where(c.first, c.cz_own, c.cz_delayed)
    assert np.all(np.abs(target - near) <= 0.0045) and np.all(np.abs(target - far) >= 0.04)             # the set-up, in numpy
    i0, i1 = c.s0.view(np.int32), c.s1.view(np.int32)
    assert np.all(i0[S_FLAGS] & (F_GOAL | F_TERMINATING | F_STAY) == 0)
    goal, term = (i1[S_FLAGS] & F_GOAL) != 0, (i1[S_FLAGS] & F_TERMINATING) != 0
    print(c.label(), "F. goal reached in %d of the first %d, %d of the other %d" % (goal[c.first].sum(), c.first.sum(), goal[~c.first].sum(), (~c.first).sum()))
    assert np.array_equal(goal, c.first) and np.array_equal(term, c.first)
    assert np.array_equal(i1[S_ENDTIME][c.first], i0[S_STEPS][c.first]) and np.array_equal(i1[S_ENDTIME][~c.first], i0[S_ENDTIME][~c.first])


@pytest.mark.parametrize("epw", [4, 16])
@pytest.mark.parametrize("task,signal", [("walk", "ik"), ("gallop", "ol")])
def test_several_substeps_in_one_launch(runs, monkeypatch, epw, task, signal):
    """G: the default configs (action_repeat 5 and 6)"""
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    c = runs(*MAIN, task=task, signal=signal, step_kw=False, epw=epw)
    assert c.epw == epw and np.all(c.rep == REPEAT[task])
    abd(c, teeth=True)
    check_g(c)
