"""The latency model in float64, numpy only: what tests/test_latency_host.py (CPU) and tests/test_gpu_latency.py (MI355X) hold the
observation-history ring of csrc/rex_kernels.h to (hist_at, delay_slots, delayed_word, receive_observation, control_observation and the PD
read of rex_substep), restated from the reference's Rex._observation_history / _GetDelayedObservation (model/rex.py:122,717-763).

The ring of one env is [100][words] (words = 3 x motors + 7: q, qd, observed torque, base quaternion x y z w, base angular velocity); the
entry received k substeps ago sits in slot (head - k) % 100; the cursor word REX_S_HIST is head | length << 8.  On the device the rings of
a batch are one tensor [100 x words, n] (env.history): row slot x words + word.

    slots(latency, dt, length)                 which two entries are blended, and with which weight: rex.py:743-752 on Python floats
    delayed(ring, head, length, latency, dt)   the blended record of one env
    delayed_batch(...)                         the same over a batch, optionally wrong on purpose (the teeth of the GPU test)
    quat_to_euler(q)                           csrc/rex_kernels.h quat_to_euler on the quaternion as given (the blend is not normalised)
    make_ring(S0, seed, heads)                 rings whose 100 entries all differ, the newest one S0's own
"""
import numpy as np

import step_readout_ref as sr

DT = 0.001                                  # the substep of step_readout_ref.STEP_KW, as the Python float the caller writes
PAIRS = [(0.0003, 0.0013), (0.0013, 0.0037), (0.0037, 0.0234), (0.0977, 0.0985), (0.099, 0.25), (0.0234, 0), (0, 0.0013)]   # (pd, control) [s]
EULER_FLOOR = (2.306e-07, 3.889e-07)         # roll, pitch [rad]: the float32 floor tests/test_latency_host.py measures
TILT_SEEDS = {67: 3, 130: 4, 75: 5}           # tilted_states(n, seed) of the batch sizes the GPU test runs; rings from RING_SEED
RING_SEED = 11
LEN = 100                              # REX_HISTORY_LEN: deque(maxlen=100), rex.py:122


def hist_word(nm=12):
    """REX_S_HIST, the cursor word: the state's last (53 for mark base; csrc/rex_kernels.h Lay<NM>::HIST)"""
    return 13 + 2 * nm + 10 + nm // 2


def words(nm=12):
    return 3 * nm + 7


def blocks(nm=12):
    """the word ranges of a record: q, qd, tau, quat, w"""
    return dict(q=slice(0, nm), qd=slice(nm, 2 * nm), tau=slice(2 * nm, 3 * nm), quat=slice(3 * nm, 3 * nm + 4), w=slice(3 * nm + 4, 3 * nm + 7))


def state_blocks(nm=12):
    """the state words a record's q, qd, quat, w are copies of (include/rexsim.h REX_S_*)"""
    return dict(q=slice(13, 13 + nm), qd=slice(13 + nm, 13 + 2 * nm), quat=slice(3, 7), w=slice(10, 13))


def slots(latency, dt, length):
    """-> (k0, k1, alpha): the delayed observation is (1 - alpha) x entry k0 ago + alpha x entry k1 ago (rex.py:743-752)"""
    if latency <= 0 or length == 1:
        return 0, 0, 0.0
    n_steps_ago = int(latency / dt)
    if n_steps_ago + 1 >= length:
        return length - 1, length - 1, 0.0
    remaining_latency = latency - n_steps_ago * dt
    return n_steps_ago, n_steps_ago + 1, remaining_latency / dt


WRONG = ("alpha", "n-1", "n+1")             # delayed_batch(wrong=...): alpha <-> 1 - alpha, a read one slot newer, one slot older


def delayed(ring, head, length, latency, dt, wrong=None):
    """ring [100, words] float64 -> the record `latency` seconds old [words]"""
    ring = np.asarray(ring, np.float64)
    k0, k1, alpha = slots(latency, dt, int(length))
    if wrong == "alpha":
        alpha = 1.0 - alpha if k1 != k0 else alpha
    elif wrong == "n-1":
        k0, k1 = max(k0 - 1, 0), max(k1 - 1, 0)
    elif wrong == "n+1":
        k0, k1 = min(k0 + 1, int(length) - 1), min(k1 + 1, int(length) - 1)
    return (1.0 - alpha) * ring[(int(head) - k0) % LEN] + alpha * ring[(int(head) - k1) % LEN]


def delayed_batch(R, heads, lengths, latency, dt, wrong=None):
    """R [100, words, n] -> [words, n] float64"""
    R = np.asarray(R, np.float64)
    return np.stack([delayed(R[:, :, g], heads[g], lengths[g], latency, dt, wrong) for g in range(R.shape[2])], axis=1)


def cursor(heads, lengths):
    """-> REX_S_HIST words (int32)"""
    return (np.asarray(heads, np.int64) | (np.asarray(lengths, np.int64) << 8)).astype(np.int32)


def uncursor(word):
    word = np.asarray(word).astype(np.int64)
    return word & 0xFF, (word >> 8) & 0xFF


def received(heads, lengths, count=1):
    """the cursor after `count` more observations (rex.py:732: appendleft on a deque of at most 100)"""
    return (np.asarray(heads) + count) % LEN, np.minimum(np.asarray(lengths) + count, LEN)


def quat_to_euler(q, xp=np, dtype=np.float64):
    """q [4, ...] (x, y, z, w), not normalised -> roll, pitch, yaw as csrc/rex_kernels.h quat_to_euler (pybullet's getEulerFromQuaternion)
    states them, away from the poles of the pitch (|sin pitch| < 0.99999, asserted); dtype float32 restates it in single precision"""
    x, y, z, w = (xp.asarray(c, dtype) for c in q)
    two = dtype(2.0)
    sqx, sqy, sqz, squ = x * x, y * y, z * z, w * w
    sarg = -two * (x * z - w * y)
    assert np.all(np.abs(sarg) < 0.99999)
    pitch = xp.arcsin(sarg)
    roll = xp.arctan2(two * (y * z + w * x), squ - sqx - sqy + sqz)
    yaw = xp.arctan2(two * (x * y + w * z), squ + sqx - sqy - sqz)
    return roll, pitch, yaw


def blend32(x, y, alpha):
    """delayed_word of csrc/rex_kernels.h in float32, products and sum rounded one by one"""
    a = np.asarray(alpha, np.float32)
    return (np.float32(1.0) - a) * np.asarray(x, np.float32) + a * np.asarray(y, np.float32)


def blend_bound(x, y):
    """what a float32 (1 - alpha) x + alpha y may differ by from the float64 one on the same float32 inputs: one rounding of 1 - alpha,
    two of the products and one of the sum, fused or not -- each half a unit in the last place of a magnitude <= |x| + |y|"""
    return 4.0 * 2.0 ** -24 * (np.abs(x) + np.abs(y))


def blend_pair(R, heads, lengths, latency, dt):
    """-> (x, y, alpha): the two entries [words, n] each and the weights [n] that delayed_batch blends"""
    n = R.shape[2]
    x, y, al = np.zeros(R.shape[1:]), np.zeros(R.shape[1:]), np.zeros(n)
    for g in range(n):
        k0, k1, al[g] = slots(latency, dt, int(lengths[g]))
        x[:, g], y[:, g] = R[(int(heads[g]) - k0) % LEN, :, g], R[(int(heads[g]) - k1) % LEN, :, g]
    return x, y, al


STEP = dict(q=1e-2, qd=0.3, quat=5e-3, w=0.2)      # per-slot steps of make_ring's walk
Q_MAX, QD_MAX = 3.1, 90.0                          # older entries stay inside (-pi, pi) and well under the +-100 rad/s clamp


def make_ring(S0, seed, heads, nm=12):
    """S0 [state words, n] float32, heads [n] -> rings [100, words, n] float32.  The entry at `head` is exactly S0's q, qd, quaternion and
    angular velocity, as it always is in the product; older entries walk away from it backwards with uniform per-slot steps of up to STEP
    (1e-2 rad in q, 0.3 rad/s in qd, 5e-3 in the quaternion components, 0.2 rad/s in w); the torque words are independent uniform values
    in +-3.  The walk is taken in float64 and rounded to float32, the values both the reference and the GPU start from."""
    S0 = np.asarray(S0, np.float32)
    n, W = S0.shape[1], words(nm)
    rng = np.random.RandomState(seed)
    ago = np.zeros((LEN, W, n))
    rb, sb = blocks(nm), state_blocks(nm)
    for name in ("q", "qd", "quat", "w"):
        x0 = S0[sb[name]].astype(np.float64)
        walk = np.cumsum(rng.uniform(-STEP[name], STEP[name], (LEN - 1,) + x0.shape), axis=0)
        old = x0[None] + walk
        if name == "q":
            old = np.clip(old, -Q_MAX, Q_MAX)
        elif name == "qd":
            old = np.clip(old, -QD_MAX, QD_MAX)
        ago[0, rb[name]] = x0
        ago[1:, rb[name]] = old
    ago[:, rb["tau"]] = rng.uniform(-3.0, 3.0, (LEN, nm, n))
    ring = np.zeros((LEN, W, n), np.float32)
    for g in range(n):
        ring[(int(heads[g]) - np.arange(LEN)) % LEN, :, g] = ago[:, :, g]
    assert np.all(np.abs(ago[1:, rb["q"]]) < np.pi) and np.all(np.abs(ago[1:, rb["qd"]]) <= QD_MAX)
    return ring


def tilted_states(n, seed, words=37):
    """[words, n] float32, zero but for the base quaternion (words 3 .. 6) and angular velocity (10 .. 12): a tilt of up to 1.2 rad about a
    horizontal axis after a random yaw (the orientations of kinematics_ref's synthetic states) and rates in +-3 rad/s -- the orientations
    over which the roll and pitch of the control observation are compared, on the CPU (the float32 floor) and on the GPU alike"""
    rng = np.random.RandomState(seed)
    S = np.zeros((words, n), np.float32)
    for g in range(n):
        tilt, heading, yaw = rng.uniform(0, 1.2), rng.uniform(0, 2 * np.pi), rng.uniform(-np.pi, np.pi)
        a = [0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]
        b = [np.sin(tilt / 2) * np.cos(heading), np.sin(tilt / 2) * np.sin(heading), 0, np.cos(tilt / 2)]
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        S[3:7, g] = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz]
        S[10:13, g] = rng.uniform(-3, 3, 3)
    return S


def euler_floor(S0, seed, pairs=PAIRS, dt=DT):
    """(roll, pitch): the largest deviation of blend -> quat_to_euler restated in float32 from the float64 one over make_ring(S0, seed)
    rings under cursors() of every latency pair, as absolute angles [rad]"""
    n = S0.shape[1]
    worst = np.zeros(2)
    for pd, ctl in pairs:
        heads, lengths = cursors(n, int(pd / dt), int(ctl / dt))
        R = make_ring(S0, seed, heads)
        x, y, al = blend_pair(R, heads, lengths, ctl, dt)
        qs = blocks()["quat"]
        want = quat_to_euler(((1.0 - al) * x + al * y)[qs])
        got = quat_to_euler(blend32(x[qs], y[qs], al), dtype=np.float32)
        for k in range(2):
            worst[k] = max(worst[k], np.abs(got[k].astype(np.float64) - want[k]).max())
    return worst


def cursors(n, n_pd, n_c):
    """-> (heads, lengths) [n]: heads cycle through 0, 1, 42, 98, 99; every second env has length 100 (the only length the product itself
    produces), the others cycle through 1, 2, n_pd + 1, n_pd + 2, n_c + 1, n_c + 2, 100, capped to 1 .. 100 -- short lengths exercise
    the branches of delay_slots that the reset motion (600 observations) never leaves behind"""
    heads = np.array([(0, 1, 42, 98, 99)[g % 5] for g in range(n)])
    short = [min(max(v, 1), LEN) for v in (1, 2, n_pd + 1, n_pd + 2, n_c + 1, n_c + 2, LEN)]
    lengths = np.array([LEN if g % 2 == 0 else short[(g // 2) % 7] for g in range(n)])
    return heads, lengths


def pd_torque(cmd, R, heads, lengths, pd_latency, dt, nm=12, wrong=None, params=None, kp=1.0, kd=0.02):
    """The torque the sensor reports [n, nm] (motor.py:127-129) under the PD-delayed observation: cmd [n, nm]; wrong: one of WRONG, or
    "blocks" (the q and qd word blocks exchanged); params: step_readout_ref.motor_params' dict (per-env voltage, kp, kd)"""
    rb = blocks(nm)
    d = delayed_batch(R, heads, lengths, pd_latency, dt, wrong if wrong in WRONG else None)
    q, qd = d[rb["q"]], d[rb["qd"]]
    if wrong == "blocks":
        q, qd = qd, q
    kw = dict(kp=kp, kd=kd)
    if params is not None:
        kw = {k: params[k].astype(np.float64) for k in ("voltage", "damping", "kp", "kd", "strength")}
    return sr.motor_model(np.asarray(cmd, np.float64).T, q, qd, qd, **kw)[1].T
