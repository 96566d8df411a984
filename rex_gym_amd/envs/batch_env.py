"""RexBatchEnv: N reference environments stepped by one HIP launch.

Stands where the reference puts `BatchEnv` over N `ExternalProcess`-wrapped envs
(rex_gym/agents/tools/batch_env.py:18-115, wrappers.py:294-458): same call shapes
(`len(env)`, `env[i]`, `step(actions[N,A]) -> (obs[N,O], reward[N], done[N], infos)`,
`reset(indices=None)`), but the state never leaves HBM and there is no IPC.

PyTorch is used for device memory and streams only; all compute is in librexsim_hip.so.
"""
import ctypes
import math

import numpy as np

from .. import _lib
from .spaces import Box

OBSERVATION_EPS = 0.01  # rex_gym_env.py:20


def _spaces(task, signal, sim_dt, num_motors=12):
    """Box bounds of the reference envs (part of the drop-in contract)."""
    if task == "walk":      # walk_env.py:104-114
        hi = {"ik": 0.4, "ol": 0.01}[signal]
        dim = {"ik": 2, "ol": 8}[signal]
        action = Box(-np.full(dim, hi), np.full(dim, hi))
        ub = np.array([2 * math.pi, 2 * math.pi, 2 * math.pi / sim_dt, 2 * math.pi / sim_dt])   # walk_env.py:364-378
    elif task == "gallop":  # gallop_env.py:119-130 -- low/high are inverted in the reference
        hi = {"ik": 0.4, "ol": 0.3}[signal]
        dim = {"ik": 2, "ol": 4}[signal]
        action = Box(np.full(dim, hi), -np.full(dim, hi))
        ub = np.array([2 * math.pi, 2 * math.pi, 2 * math.pi / sim_dt, 2 * math.pi / sim_dt] + [2 * math.pi] * num_motors)
    elif task == "turn":    # turn_env.py:100-110
        action = Box(-np.full(2, 0.01), np.full(2, 0.01))
        ub = np.array([2 * math.pi, 2 * math.pi, 2 * math.pi / sim_dt, 2 * math.pi / sim_dt])
    elif task == "standup":  # standup_env.py:99-101,200-204 (signal_type is unused by the env)
        action = Box(-np.full(1, 0.1), np.full(1, 0.1))
        ub = np.array([2 * math.pi, 2 * math.pi, 2 * math.pi / sim_dt, 2 * math.pi / sim_dt])
    elif task == "poses":   # poses_env.py:115-117
        action = Box(-np.full(1, 0.1), np.full(1, 0.1))
        ub = np.array([2 * math.pi, 2 * math.pi, 2 * math.pi / sim_dt, 2 * math.pi / sim_dt])
    else:
        raise ValueError(f"unsupported task {task!r}")
    obs = Box(-(ub + OBSERVATION_EPS), ub + OBSERVATION_EPS)  # rex_gym_env.py:277-278
    return action, obs


class _EnvView:
    """`batch_env[i]`: attribute access to one env, as BatchEnv.__getitem__ gives (batch_env.py:44-46)."""

    def __init__(self, batch, index):
        self._batch, self.index = batch, index
        self.action_space, self.observation_space = batch.action_space, batch.observation_space

    def state(self):
        return self._batch.state[:, self.index].clone()


class StepOut:
    """Output tensors of a step, validated once (RexBatchEnv.bind_out): the tensors and their device pointers."""
    __slots__ = ("obs", "reward", "done", "done_bool", "p_obs", "p_reward", "p_done")

    def __init__(self, obs, reward, done, torch):
        self.obs, self.reward, self.done = obs, reward, done
        self.done_bool = done if done.dtype == torch.bool else done.view(torch.bool)
        self.p_obs, self.p_reward, self.p_done = obs.data_ptr(), reward.data_ptr(), done.data_ptr()


class RexBatchEnv:
    metadata = {"render.modes": ["rgb_array"]}

    def __init__(self, num_envs, task="walk", signal_type="ik", device=0, seed=0, env_index_base=0,
                 auto_reset=False, max_episode_steps=0, backwards=None, target_position=None,
                 target_orient=None, init_orient=None, base_y=None, base_z=None, base_roll=None, base_pitch=None,
                 base_yaw=None,
                 motor_kp=1.0, motor_kd=0.02, control_time_step=None, action_repeat=None, control_latency=0.0,
                 pd_latency=0.0,
                 solver_iterations=None, solver_residual_threshold=None,
                 range_normalize=False, check_actions=True, terrain_type="plane", terrain_pool=64, terrain_seed=10,
                 mark="base", render=False, stream=None, gait_clock_scale=1.0,
                 distance_weight=None, energy_weight=None, drift_weight=None, shake_weight=None,
                 tasks=None, mass_scale_range=None, friction_range=None, observation_noise_stdev=None,
                 heightfield=None, heightfield_cell=None, heightfield_origin=(0.0, 0.0, 0.0), init_height=None,
                 body_contacts=None, on_rack=False, env_randomizer=None, forward_reward_cap=None, use_angle_in_observation=True,
                 motor_strength_range=None, battery_voltage_range=None, motor_damping_range=None, motor_kp_range=None,
                 motor_kd_range=None, motor_strength_per_motor=True, **ignored):
        import torch
        # Reference constructor keywords that only touch the GUI, logging or debugging are accepted and ignored; anything
        # else that would change what the env computes is an error here, not a silent no-op.
        harmless = {"debug", "urdf_version", "num_steps_to_log", "log_path", "terrain_id", "urdf_root", "reflection",
                    "draw_foot_path", "hard_reset"}
        unknown = sorted(set(ignored) - harmless)
        if unknown:
            raise TypeError(f"RexBatchEnv: unsupported keyword(s) {unknown}")
        # EnvRandomizer objects (rex_gym_env.py:225,345-346,400-401): host-side hooks, called with this env at every reset()
        # (`randomize_env`) and step() (`randomize_step`, when the object has one); they reach the robot through `self.rex`
        self._env_randomizers = ([] if not env_randomizer else list(env_randomizer) if isinstance(env_randomizer, (list, tuple))
                                 else [env_randomizer])
        if self._env_randomizers and auto_reset:
            raise ValueError("env_randomizer hooks run on the host inside reset(); with auto_reset the resets happen inside the "
                             "launch -- use mass_scale_range / friction_range and the motor_*_range / battery_voltage_range "
                             "keywords (per-reset draws in the kernel) instead")
        # per-reset draws of the actuator's knobs inside the launch (rex_set_motor_randomization): (lo, hi) each, None: not drawn
        motor_random = _lib.RexMotorRandom()
        motor_random.strength_per_motor = int(bool(motor_strength_per_motor))
        for name, rng in (("strength", motor_strength_range), ("voltage", battery_voltage_range), ("damping", motor_damping_range),
                          ("kp", motor_kp_range), ("kd", motor_kd_range)):
            if rng is None:
                continue
            try:
                lo, hi = (float(v) for v in rng)
            except (TypeError, ValueError):
                raise ValueError(f"the {name} range must be a pair (lo, hi)") from None
            if not (0.0 <= lo <= hi < float("inf")):     # (false for NaN as well)
                raise ValueError(f"the {name} range must satisfy 0 <= lo <= hi (finite), got ({lo}, {hi})")
            setattr(motor_random, name + "_lo", lo); setattr(motor_random, name + "_hi", hi)
        self._motor_random = motor_random if any(r is not None for r in (motor_strength_range, battery_voltage_range, motor_damping_range,
                                                                         motor_kp_range, motor_kd_range)) else None
        self._randomize_indices = None
        if terrain_type in ("hills", "mounts", "maze") and heightfield is None:
            raise NotImplementedError(
                f"terrain_type={terrain_type!r}: the reference loads this field from the pip package pybullet_data "
                "(model/terrain.py:55-78), which is not part of rex-gym; with that package at hand: "
                f"RexBatchEnv(..., terrain_type={terrain_type!r}, **rex_gym_amd.terrain.load_reference_terrain({terrain_type!r}, "
                "pybullet_data.getDataPath())) -- or pass the heights yourself as heightfield=<array [ny, nx] in metres>, "
                "heightfield_cell=(cx, cy), heightfield_origin=(x, y, z), init_height=...")
        if terrain_type not in ("plane", "random", "hills", "mounts", "maze", "custom") or mark not in _lib.MARKS or render:
            raise NotImplementedError("terrain_type must be 'plane', 'random' or a heightfield ('hills', 'mounts', 'maze', "
                                      "'custom' with heightfield=...); mark 'base' or 'arm'; render=False")
        if heightfield is not None and terrain_type in ("plane", "random"):
            raise ValueError("heightfield=... goes with terrain_type 'custom' / 'hills' / 'mounts' / 'maze'")
        if task not in _lib.TASKS or signal_type not in _lib.SIGNALS:
            raise ValueError(f"unsupported task/signal {task}/{signal_type}")
        if tasks is not None and task != "mixed":
            raise ValueError("`tasks` goes with task='mixed'")
        self._torch = torch
        self._L = _lib.lib()   # raises if the HIP library is absent: no fallback
        if not torch.cuda.is_available():
            raise _lib.RexSimError("no HIP device visible to PyTorch: RexBatchEnv needs an MI355X (no CPU fallback)")
        self.num_envs = int(num_envs)
        self.task, self.signal_type = task, signal_type
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        cfg = _lib.RexConfig()
        _lib.check(self._L.rex_default_config(_lib.TASKS[task], _lib.SIGNALS[signal_type], self.num_envs,
                                             ctypes.byref(cfg)), "rex_default_config")
        if action_repeat is not None:
            cfg.action_repeat = int(action_repeat)
            cfg.solver_iterations = int(300 / cfg.action_repeat)        # rex_gym_env.py:184
        if control_time_step is not None:
            cfg.sim_time_step = float(control_time_step) / cfg.action_repeat  # rex_gym_env.py:172
        if solver_iterations is not None:
            cfg.solver_iterations = int(solver_iterations)
        if solver_residual_threshold is not None:
            cfg.solver_residual_threshold = float(solver_residual_threshold)
        if task == "mixed":   # BASELINE.json configs[4]: every env runs one task of the mix, drawn per env (REX_TASK_MIXED)
            names = ("walk", "gallop", "turn") if tasks is None else tuple(tasks)
            if not names or any(t not in ("walk", "gallop", "turn") for t in names):
                raise ValueError("tasks must be a non-empty subset of ('walk', 'gallop', 'turn')")
            cfg.task_mix = sum(1 << _lib.TASKS[t] for t in set(names))
            self.tasks = tuple(t for t in ("walk", "gallop", "turn") if t in names)
        for rng, lo_name, hi_name in ((mass_scale_range, "mass_scale_lo", "mass_scale_hi"), (friction_range, "friction_lo", "friction_hi")):
            if rng is not None:   # per-reset draws of the env_randomizer hook (rex_gym_env.py:345-346)
                setattr(cfg, lo_name, float(rng[0])); setattr(cfg, hi_name, float(rng[1]))
        if observation_noise_stdev is not None:   # Rex(observation_noise_stdev=...), rex.py:22: angle, velocity, torque, rpy, rpy rate
            if len(observation_noise_stdev) != 5:
                raise ValueError("observation_noise_stdev has 5 entries (motor angle, velocity, torque, base rpy, base rpy rate)")
            for k, v in enumerate(observation_noise_stdev):
                cfg.noise_stdev[k] = float(v)
        if init_height is None and terrain_type in ("hills", "mounts"):
            init_height = {"hills": 1.98, "mounts": 0.85}[terrain_type]     # ROBOT_INIT_POSITION, terrain.py:14-20
        if init_height is not None:
            cfg.init_height = float(init_height)
        cfg.on_rack = int(bool(on_rack))               # debug rack: fixed base at [0, 0, 1] (rex.py:269-287)
        if body_contacts is not None:   # link collision boxes vs ground and vs the base body, next to the toe rows (include/rexsim.h);
            cfg.body_contacts = int(bool(body_contacts))   # None: the task's default (on for 'poses')
        cfg.motor_kp, cfg.motor_kd = float(motor_kp), float(motor_kd)
        cfg.gait_clock_scale = float(gait_clock_scale)     # wall-clock seconds per simulated second (gait_planner.py:108-110)
        for name, v in (("distance_weight", distance_weight), ("energy_weight", energy_weight),
                        ("drift_weight", drift_weight), ("shake_weight", shake_weight)):   # rex_gym_env.py:56-59
            if v is not None:
                setattr(cfg, name, float(v))
        if not use_angle_in_observation:       # RexReactiveEnv(use_angle_in_observation=False): the four base words alone (gallop_env.py:344-356)
            if task != "gallop":
                raise ValueError("use_angle_in_observation is a keyword of the gallop env (RexReactiveEnv)")
            cfg.gallop_no_angles = 1
        if forward_reward_cap is not None:     # `min(forward_reward, cap)` in the base reward, rex_gym_env.py:81,525
            cfg.forward_reward_cap = float(forward_reward_cap)
        if task == "mixed" and energy_weight is not None:
            raise ValueError("energy_weight is a per-task constant in a mixed batch (gallop 0.005, walk / turn 0.0005)")
        cfg.backwards = -1 if backwards is None else int(bool(backwards))
        cfg.target_position = 0.0 if not target_position else float(target_position)
        if target_orient:                      # `if not self._target_orient` -> drawn (turn_env.py:137)
            cfg.target_orient = float(target_orient); cfg.orient_fixed |= 1
        if init_orient is not None:            # `if self._init_orient is None` -> drawn (turn_env.py:146)
            cfg.init_orient = float(init_orient); cfg.orient_fixed |= 2
        pose_kw = (base_y, base_z, base_roll, base_pitch, base_yaw)
        if task == "poses" and any(v is not None for v in pose_kw):   # fill_next_pose_and_target, poses_env.py:172-187
            vals = [0.0 if v is None else float(v) for v in pose_kw]
            k = next((i for i, v in enumerate(vals[:4]) if v != 0.0), 4)
            cfg.pose_index, cfg.pose_value = k, vals[k]
        cfg.pd_latency, cfg.control_latency = float(pd_latency or 0.0), float(control_latency or 0.0)
        cfg.range_normalize = int(bool(range_normalize))
        cfg.seed = int(seed) & (2 ** 64 - 1)
        cfg.env_index_base = int(env_index_base)
        cfg.auto_reset = int(bool(auto_reset))
        cfg.max_episode_steps = int(max_episode_steps)
        cfg.mark = _lib.MARKS[mark]
        self.mark = mark
        self.config = cfg
        self.num_motors = self._L.rex_num_motors(ctypes.byref(cfg))    # mark_constants.MARK_DETAILS['motors_num']
        self.state_words = self._L.rex_state_words(ctypes.byref(cfg))
        self.action_dim = self._L.rex_action_dim(ctypes.byref(cfg))
        self.obs_dim = self._L.rex_obs_dim(ctypes.byref(cfg))
        if task == "mixed":   # the widest task of the mix; narrower tasks ignore / zero the tail of their rows
            per = {t: _spaces(t, signal_type, cfg.sim_time_step, self.num_motors) for t in self.tasks}
            self.task_action_spaces = {t: sp[0] for t, sp in per.items()}
            wide_a = max(per.values(), key=lambda sp: sp[0].shape[0])[0]
            wide_o = max(per.values(), key=lambda sp: sp[1].shape[0])[1]
            tight = min(float(np.abs(sp[0].high).min()) for sp in per.values())     # inside every task's Box
            self.action_space, self.observation_space = Box(-np.full(wide_a.shape, tight), np.full(wide_a.shape, tight)), wide_o
        else:
            self.action_space, self.observation_space = _spaces(task, signal_type, cfg.sim_time_step, self.num_motors if use_angle_in_observation else 0)
        if range_normalize:   # RangeNormalize / ClipAction expose [-1, 1] boxes (wrappers.py:205-219)
            self.inner_action_space, self.inner_observation_space = self.action_space, self.observation_space
            self.action_space = Box(-np.ones(self.action_space.shape), np.ones(self.action_space.shape))
            self.observation_space = Box(-np.ones(self.observation_space.shape), np.ones(self.observation_space.shape))
        self.control_time_step = cfg.sim_time_step * cfg.action_repeat
        self.check_actions = bool(check_actions)
        self._act_lo = self._act_hi = None
        self._stream = stream
        with torch.cuda.device(self.device):
            self.state = torch.zeros((self.state_words, self.num_envs), dtype=torch.float32, device=self.device)
            self._obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
            self._reward = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
            self._done = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            self._cmd = torch.zeros((self.num_envs, self.num_motors), dtype=torch.float32, device=self.device)
            handle = ctypes.c_void_p()
            _lib.check(self._L.rex_create(ctypes.byref(cfg), self.device.index, self.state.data_ptr(),
                                          self._stream_ptr(), ctypes.byref(handle)), "rex_create")
        self._h = handle
        self._own_out = StepOut(self._obs, self._reward, self._done, torch)
        self.motor_params_tensor = None
        if self._motor_random is not None:
            _lib.check(self._L.rex_set_motor_randomization(self._h, ctypes.byref(self._motor_random)), "rex_set_motor_randomization")
        self._p_cmd, self._info = self._cmd.data_ptr(), {"action": self._cmd}
        self._needs_reset = True
        from .rex_knobs import RexKnobs
        self.rex = RexKnobs(self)
        if cfg.pd_latency > 0 or cfg.control_latency > 0:   # observation-history ring of the latency model (rex.py:122)
            with torch.cuda.device(self.device):
                self.history = torch.zeros((100 * (3 * self.num_motors + 7), self.num_envs), dtype=torch.float32, device=self.device)
            _lib.check(self._L.rex_set_history(self._h, self.history.data_ptr()), "rex_set_history")
        self.terrain_type = terrain_type
        if heightfield is not None:    # model/terrain.py:55-78 style fields, supplied by the caller
            h = np.asarray(heightfield, dtype=np.float32)
            if h.ndim == 2:
                h = h[None]
            if h.ndim != 3 or heightfield_cell is None:
                raise ValueError("heightfield must be [ny, nx] or [k, ny, nx] (metres) and heightfield_cell=(cx, cy) given")
            ox, oy, oz = (float(v) for v in heightfield_origin)
            mids = np.array([0.5 * (float(f.min()) + float(f.max())) - oz for f in h], dtype=np.float32)   # Bullet centres the shape, then places it at z0
            with torch.cuda.device(self.device):
                self.terrain_heights = torch.from_numpy(np.ascontiguousarray(h)).to(self.device)
                self.terrain_mids = torch.from_numpy(mids).to(self.device)
                _lib.check(self._L.rex_set_heightfield(self._h, self.terrain_heights.data_ptr(), self.terrain_mids.data_ptr(),
                                                       int(h.shape[0]), int(h.shape[2]), int(h.shape[1]), float(heightfield_cell[0]),
                                                       float(heightfield_cell[1]), ox, oy, self._stream_ptr()), "rex_set_heightfield")
        if terrain_type == "random":   # model/terrain.py:32-54 -- a pool of fields instead of one per env
            from ..terrain import random_terrain_pool
            h, m = random_terrain_pool(int(terrain_pool), int(terrain_seed))
            with torch.cuda.device(self.device):
                self.terrain_heights = torch.from_numpy(h).to(self.device)
                self.terrain_mids = torch.from_numpy(m).to(self.device)
                _lib.check(self._L.rex_set_terrain(self._h, self.terrain_heights.data_ptr(), self.terrain_mids.data_ptr(),
                                                   int(terrain_pool), self._stream_ptr()), "rex_set_terrain")

    # ---- plumbing ----
    def _stream_ptr(self):
        s = self._stream if self._stream is not None else self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def task_ids(self):
        """task='mixed': the task every env runs, as a device int32 tensor of REX_TASK_* ids (drawn per env from its global
        index, fixed for the env's life -- the same draw the kernels make)."""
        torch = self._torch
        if self.task != "mixed":
            return torch.full((self.num_envs,), _lib.TASKS[self.task], dtype=torch.int32, device=self.device)
        from .philox import philox4x32
        g = np.arange(self.num_envs, dtype=np.uint32) + np.uint32(self.config.env_index_base)
        ctr = np.stack([np.full_like(g, 0xFFFFFFFF), g, np.full_like(g, 2), np.zeros_like(g)])
        out = philox4x32(ctr, np.uint32(self.config.seed & 0xFFFFFFFF), np.uint32(self.config.seed >> 32))
        ids = np.array([_lib.TASKS[t] for t in self.tasks], dtype=np.int32)
        return torch.from_numpy(ids[(out[0] % np.uint32(len(ids))).astype(np.int64)]).to(self.device)

    def _on_stream(self):
        """Context in which host-side staging (dtype / device conversion of actions and indices) is issued: the stream the
        kernels are launched on, so that a RexBatchEnv(stream=...) orders its copies with its launches by itself."""
        import contextlib
        return self._torch.cuda.stream(self._stream) if self._stream is not None else contextlib.nullcontext()

    def __len__(self):
        return self.num_envs

    def __getitem__(self, index):
        return _EnvView(self, index)

    def seed(self, seed=None):
        return [seed]

    def close(self):
        if getattr(self, "_h", None):
            self._torch.cuda.synchronize(self.device)
            self._L.rex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_event_trace(self, enable=True):
        """Debug (rex_set_event_trace): fold the discrete events of every physics substep -- toe points in reach, the heightfield
        facets under them, joint / arm bounds reached -- into a chained hash per env, and the solver sweep counts into a second
        one, and the events without the arm's bounds into a third.  Returns the device tensor uint32-as-int32 [3, num_envs] the launches
        update (zeroed here); False switches it off."""
        torch = self._torch
        if not enable:
            _lib.check(self._L.rex_set_event_trace(self._h, None), "rex_set_event_trace")
            self._trace = None
            return None
        self._trace = torch.zeros((3, self.num_envs), dtype=torch.int32, device=self.device)
        _lib.check(self._L.rex_set_event_trace(self._h, self._trace.data_ptr()), "rex_set_event_trace")
        return self._trace

    def set_timing(self, enable=True):
        """True / 1: time the last launch (last_step_ms); 2: a ring of the last 256 launches, no sync in between (step_times_ms)."""
        _lib.check(self._L.rex_set_timing(self._h, int(enable)), "rex_set_timing")

    def step_times_ms(self, count=256):
        buf = (ctypes.c_float * int(count))()
        n = self._L.rex_step_times_ms(self._h, buf, int(count))
        _lib.check(min(n, 0), "rex_step_times_ms")
        return list(buf[:n])

    def last_step_ms(self):
        ms = ctypes.c_float()
        _lib.check(self._L.rex_last_step_ms(self._h, ctypes.byref(ms)), "rex_last_step_ms")
        return ms.value

    def set_body_params(self, base_mass_scale=None, leg_mass_scale=None, foot_friction=None):
        """Per-env domain randomisation (the knobs of Rex.SetBaseMasses / SetLegMasses, rex.py:659-692, plus the foot
        friction). Each argument: None (keep), a float, or an [N] tensor/array. The values live in `self.body_params`
        ([3, N] device tensor) and may be edited in place between steps."""
        torch = self._torch
        if getattr(self, "body_params", None) is None:
            self.body_params = torch.tensor([[1.0], [1.0], [0.5]], device=self.device).repeat(1, self.num_envs).contiguous()
            _lib.check(self._L.rex_set_body_params(self._h, self.body_params.data_ptr()), "rex_set_body_params")
        for row, v in enumerate((base_mass_scale, leg_mass_scale, foot_friction)):
            if v is not None:
                self.body_params[row] = torch.as_tensor(v, dtype=torch.float32, device=self.device)
        return self.body_params

    def set_motor_params(self, voltage=None, damping=None, kp=None, kd=None, strength=None):
        """Per-env actuator parameters (the knobs of the reference's MotorModel, model/motor.py:40-74, and the PD gains of
        Rex.ApplyAction). Each argument: None (keep), a float, or an [N] tensor/array; strength also [num_motors, N] (one ratio
        per motor, mark_constants order). The values live in the returned [4 + num_motors, N] device tensor -- rows voltage,
        viscous damping, kp, kd, then the strength ratios -- which starts nominal (32 V, 0, motor_kp, motor_kd, 1) and may be
        edited in place between steps. The reset motion stays the nominal robot's, as with set_body_params."""
        torch = self._torch
        if self.motor_params_tensor is None:
            nominal = [32.0, 0.0, float(self.config.motor_kp), float(self.config.motor_kd)] + [1.0] * self.num_motors
            table = torch.tensor(nominal, dtype=torch.float32, device=self.device)[:, None].repeat(1, self.num_envs).contiguous()
            _lib.check(self._L.rex_set_motor_params(self._h, table.data_ptr()), "rex_set_motor_params")
            self.motor_params_tensor = table
        p = self.motor_params_tensor
        for row, v in enumerate((voltage, damping, kp, kd)):
            if v is not None:
                p[row] = torch.as_tensor(v, dtype=torch.float32, device=self.device)
        if strength is not None:
            p[4:] = torch.as_tensor(strength, dtype=torch.float32, device=self.device)
        return p

    def motor_params(self):
        """The actuator parameters in effect for every env's current episode -- explicit entries and per-reset draws -- as a new
        [4 + num_motors, N] device tensor (rex_get_motor_params; rows as in set_motor_params)."""
        torch = self._torch
        out = torch.empty((4 + self.num_motors, self.num_envs), dtype=torch.float32, device=self.device)
        _lib.check(self._L.rex_get_motor_params(self._h, out.data_ptr(), self._stream_ptr()), "rex_get_motor_params")
        return out

    # ---- Gym / BatchEnv surface ----
    def reset(self, indices=None):
        """Reset all envs (indices=None) or the given ones; returns their first observations."""
        torch = self._torch
        if indices is None:
            _lib.check(self._L.rex_reset(self._h, None, 0, self._obs.data_ptr(), self._stream_ptr()), "rex_reset")
            self._needs_reset = False
            self._randomize(None)
            return self._obs.clone()
        with self._on_stream():
            idx = torch.as_tensor(indices, dtype=torch.int32, device=self.device).contiguous()
            obs = torch.empty((idx.numel(), self.obs_dim), dtype=torch.float32, device=self.device)
            if idx.numel():
                _lib.check(self._L.rex_reset(self._h, idx.data_ptr(), idx.numel(), obs.data_ptr(), self._stream_ptr()),
                           "rex_reset")
                self._randomize(idx)
        return obs

    def add_env_randomizer(self, env_randomizer):     # rex_gym_env.py:293-294
        self._env_randomizers.append(env_randomizer)

    def _randomize(self, idx):
        # after Rex.Reset, as in the reference (rex_gym_env.py:341-346): the reset motion is the nominal robot's
        self._randomize_indices = idx
        for r in self._env_randomizers:
            r.randomize_env(self)
        self._randomize_indices = None

    def step(self, actions, out=None):
        """actions [N, action_dim] (device float32 tensor, or array-like). Returns device tensors
        (obs [N,O], reward [N], done [N] bool) and info {'action': motor command [N,12]}.

        out=(obs [N,O] float32, reward [N] float32, done [N] uint8 or bool): the launch writes its results straight into
        these contiguous device tensors -- e.g. slice t of a rollout segment [T, N, ...] that is handed to the learner
        (sharding.gather_rollout) -- instead of the env's own buffers; nothing is copied."""
        torch = self._torch
        if self._needs_reset:
            raise RuntimeError("Must reset environment.")   # wrappers.py:286-288 semantics
        for r in self._env_randomizers:                     # rex_gym_env.py:400-401
            if hasattr(r, "randomize_step"):
                r.randomize_step(self)
        with self._on_stream():
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
            if a.shape != (self.num_envs, self.action_dim):
                raise ValueError(f"actions must have shape {(self.num_envs, self.action_dim)}, got {tuple(a.shape)}")
            a = a.contiguous()
            if self.check_actions:
                # BatchEnv.step: `if not env.action_space.contains(action): raise ValueError` for every env (agents/tools/
                # batch_env.py:76-79), in the Box's own dtype (float32).  Behind the folded ClipAction the space is unbounded
                # (wrappers.py:254-259): only non-finite actions are invalid.  The verdict is read back from the device, i.e. one
                # host synchronisation per step, as in the reference (issued on the env's own stream, behind the staging copy
                # above); throughput loops that have validated their actions beforehand pass check_actions=False.
                bad = ~torch.isfinite(a)
                if not self.config.range_normalize:
                    lo, hi = self._action_bounds()
                    bad |= (a < lo) | (a > hi)
                rows = bad.any(dim=1)
                if bool(rows.any()):
                    i = int(torch.nonzero(rows)[0])
                    raise ValueError(f"Invalid action at index {i}: {a[i].tolist()}")
        if out is None:
            out = self._own_out
        elif not isinstance(out, StepOut):
            out = self.bind_out(*out)
        _lib.check(self._L.rex_step(self._h, a.data_ptr(), out.p_obs, out.p_reward, out.p_done, self._p_cmd, self._stream_ptr()), "rex_step")
        return out.obs, out.reward, out.done_bool, self._info

    def load_visual_meshes(self, data_path=None):
        """Read the URDF's visual meshes (rex_gym_amd/meshes.py; parsed and built once per process), build their BVHs and hand
        them to the library (rex_render_set_visuals).  data_path = rex_gym.util.pybullet_data.getDataPath() (default: that
        of an installed rex_gym).  Returns the loaded meshes; .missing lists the files not found, drawn as their links'
        collision primitives.  After this, render() draws the meshes unless asked for geometry="collision"."""
        from .. import meshes
        vm = meshes.load(data_path, self.mark)
        box = np.ascontiguousarray(np.concatenate([vm.lo, vm.hi], axis=1), dtype=np.float32)
        with self._on_stream():
            _lib.check(self._L.rex_render_set_visuals(self._h, vm.nodes.ctypes.data, len(vm.nodes), vm.tris.ctypes.data, len(vm.tris),
                                                      vm.root.ctypes.data, box.ctypes.data, len(vm.root), self._stream_ptr()),
                       "rex_render_set_visuals")
        self._visuals = vm
        return vm

    def render(self, mode="rgb_array", env_ids=None, width=480, height=360, camera=None, depth=False, segmentation=False,
               geometry=None):
        """Camera images of the batch (rex_render / rex_render_visual): the reference's RexGymEnv.render(mode="rgb_array")
        (rex_gym_env.py:416-439) for many envs in one launch, on the env's stream, with no host sync.  geometry "collision"
        draws the collision geometry the simulator uses (link boxes, full toe cylinders, the arm's collision cylinders);
        "visual" the URDF's visual meshes, as the reference draws them (loading them first with load_visual_meshes() from
        the default location if this env has none); None = "visual" once meshes are loaded on this env, else "collision".

        env_ids: the envs to draw (default all), row k of the result is env env_ids[k].  camera: a dict (or _lib.RexCamera)
        with any of distance, yaw_deg, pitch_deg, fov_deg, near_plane, far_plane; the rest from the reference's camera
        (1.0, 0, -30, 60, 0.1, 100).  Returns uint8 [k, height, width, 3] (row 0 = the top of the image); with depth or
        segmentation, (rgb, {"depth": float32 [k, H, W] eye-space metres, far where nothing is hit, "segmentation": int16
        [k, H, W] -1 nothing, 0 ground, 1 + b body b}) -- the entry not asked for is None."""
        torch = self._torch
        if mode != "rgb_array":
            raise NotImplementedError(f"render mode {mode!r}: RexBatchEnv renders 'rgb_array' only (no GUI)")
        if geometry is None:
            geometry = "visual" if getattr(self, "_visuals", None) is not None else "collision"
        if geometry not in ("collision", "visual"):
            raise ValueError(f"render: geometry must be 'collision', 'visual' or None, got {geometry!r}")
        cam = self._camera(camera)
        width, height = int(width), int(height)
        if not (1 <= width <= 4096 and 1 <= height <= 4096):
            raise ValueError(f"render: width and height must lie in 1..4096, got {width} x {height}")
        if not (cam.distance > 0 and 0 < cam.fov_deg < 180 and cam.near_plane > 0 and cam.far_plane > cam.near_plane):
            raise ValueError("render: camera distance, fov and near plane must be positive (fov < 180, far > near)")
        with self._on_stream():
            if env_ids is None:
                if getattr(self, "_all_ids", None) is None:
                    self._all_ids = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
                ids = self._all_ids
            else:
                ids, _ = self._row_ids(env_ids, "render")
            k = int(ids.numel())
            if k * width * height * 3 >= 2 ** 31:
                raise ValueError("render: k * width * height * 3 must stay below 2^31 bytes")
            if geometry == "visual" and getattr(self, "_visuals", None) is None:
                self.load_visual_meshes()
            rgb = torch.empty((k, height, width, 3), dtype=torch.uint8, device=self.device)
            dep = torch.empty((k, height, width), dtype=torch.float32, device=self.device) if depth else None
            seg = torch.empty((k, height, width), dtype=torch.int16, device=self.device) if segmentation else None
            fn = "rex_render_visual" if geometry == "visual" else "rex_render"
            _lib.check(getattr(self._L, fn)(self._h, ctypes.byref(cam), ids.data_ptr(), k, width, height, rgb.data_ptr(),
                                            dep.data_ptr() if dep is not None else None, seg.data_ptr() if seg is not None else None,
                                            self._stream_ptr()), fn)
        if depth or segmentation:
            return rgb, {"depth": dep, "segmentation": seg}
        return rgb

    def _camera(self, camera):
        if isinstance(camera, _lib.RexCamera):
            return camera
        cam = _lib.RexCamera()
        _lib.check(self._L.rex_default_camera(ctypes.byref(cam)), "rex_default_camera")
        for key, v in (camera or {}).items():
            if key not in ("distance", "yaw_deg", "pitch_deg", "fov_deg", "near_plane", "far_plane"):
                raise TypeError(f"render: unknown camera field {key!r}")
            setattr(cam, key, float(v))
        return cam

    def _row_ids(self, env_ids, who):
        """env_ids of render() and the sensors -> (int32 device tensor, or None for every env in order; the number of output rows)"""
        if env_ids is None:
            return None, self.num_envs
        host = np.asarray(env_ids.cpu() if hasattr(env_ids, "cpu") else env_ids, dtype=np.int64).reshape(-1)
        if host.size == 0 or host.min() < 0 or host.max() >= self.num_envs:
            raise IndexError(f"{who}: env_ids must be non-empty and lie in [0, {self.num_envs})")
        return self._torch.as_tensor(host.astype(np.int32), device=self.device), int(host.size)

    # ---- onboard sensors (rex_gym_amd/sensors.py) ----
    def depth_sensor(self, width=32, height=24, position=(-0.18, 0.0, 0.0), pitch_deg=-30.0, yaw_deg=0.0, roll_deg=0.0, fov_deg=60.0,
                     near_plane=0.02, far_plane=10.0, see_robot=True, fwd=None, up=None):
        """A depth camera mounted on the base body of every env (rex_sense_depth): `position` is the eye in the base frame, the
        view axes come from sensors.mount_axes(pitch_deg, yaw_deg, roll_deg) (negative pitch looks down; the default sits just
        in front of the front face and looks 30 degrees down the walking direction, body -x) or are given as unit vectors
        fwd / up in the base frame.  fov_deg is the vertical field of view.  see_robot=False: the ground only (the plane and
        the env's heightfield), the robot's own links do not occlude.  Returns a sensors.DepthSensor: .read(env_ids=None,
        out=None) -> float32 [k, height, width] on the env's device and stream, no host sync.  Bad sizes, planes or axes raise
        here, before any launch."""
        from .. import sensors
        if (fwd is None) != (up is None):
            raise ValueError("depth_sensor: give both fwd and up, or neither")
        if fwd is None:
            fwd, up = sensors.mount_axes(pitch_deg, yaw_deg, roll_deg)
        return sensors.DepthSensor(self, width, height, position, fwd, up, fov_deg, near_plane, far_plane, see_robot)

    def height_scan(self, points, env_ids=None, relative=True, out=None):
        """The ground's height at K points around every base (rex_height_scan): points [K, 2] (x, y in metres) in the base's
        YAW frame -- the grid turns with the robot's heading and stays level.  relative=True: base z minus the ground's
        height; False: the ground's world z (the heightfield facet over the plane, 0 on the plane and beside the field).
        Returns float32 [k, K] on the env's device and stream (`out`: a tensor of that shape to fill), env_ids as in
        render().  The points are uploaded once per distinct array; a float32 device tensor is used as it is."""
        from .. import sensors
        torch = self._torch
        with self._on_stream():
            if isinstance(points, torch.Tensor) and points.device == self.device and points.dtype == torch.float32 and points.is_contiguous():
                pts = points
            else:
                host = np.ascontiguousarray(points.cpu() if hasattr(points, "cpu") else points, dtype=np.float32)
                if host.ndim != 2 or host.shape[1] != 2 or not 1 <= host.shape[0] <= sensors.MAX_POINTS:
                    raise ValueError(f"height_scan: points must be [K, 2] with K in 1..{sensors.MAX_POINTS}, got {host.shape}")
                if not np.all(np.isfinite(host)):
                    raise ValueError("height_scan: points must be finite")
                cache = self.__dict__.setdefault("_scan_points", {})
                key = (host.shape, host.tobytes())
                if key not in cache:
                    if len(cache) >= 8:
                        cache.clear()
                    cache[key] = torch.as_tensor(host, device=self.device)
                pts = cache[key]
            if pts.dim() != 2 or pts.shape[1] != 2 or not 1 <= pts.shape[0] <= sensors.MAX_POINTS:
                raise ValueError(f"height_scan: points must be [K, 2] with K in 1..{sensors.MAX_POINTS}, got {tuple(pts.shape)}")
            K = int(pts.shape[0])
            ids, k = self._row_ids(env_ids, "height_scan")
            if k * K >= 2 ** 31:
                raise ValueError("height_scan: k * K must stay below 2^31")
            if out is None:
                out = torch.empty((k, K), dtype=torch.float32, device=self.device)
            else:
                sensors.check_out(out, (k, K), self, "height_scan")
            _lib.check(self._L.rex_height_scan(self._h, pts.data_ptr(), K, 1 if relative else 0, ids.data_ptr() if ids is not None else None,
                                               k, out.data_ptr(), self._stream_ptr()), "rex_height_scan")
        return out

    # ---- body and foot kinematics (rex_gym_amd/kinematics.py) ----
    @property
    def num_bodies(self):
        """Number of links of the robot (rex_num_bodies): 13, or 19 with mark='arm'."""
        return self._L.rex_num_bodies(ctypes.byref(self.config))

    @property
    def body_names(self):
        """The link names in body order (the rows of link_pos ... link_angvel of kinematics()), from the model tables."""
        from .. import kinematics
        return kinematics.body_names(self.mark)

    def kinematics(self, env_ids=None, fields=None, out=None):
        """Where every link and foot is and how it moves (rex_kinematics), in one read-only launch on the env's device and
        stream, no host sync.  Returns a kinematics.Kinematics whose attributes are tensors of k rows (env_ids as in render();
        default: every env, in order), world frame unless noted:
          link_pos [k, NB, 3], link_quat [k, NB, 4] (x y z w), link_linvel, link_angvel [k, NB, 3]: each link frame's origin,
              orientation, the origin's velocity and the link's angular velocity; body order = env.body_names
          toe_pos, toe_vel [k, 4, 2, 3]: the physics' contact candidate at both ends of each toe, and the foot's velocity there
          toe_dist [k, 4, 2], toe_normal [k, 4, 2, 3]: the signed distance to the ground the solver sees, and the ground's normal
          toe_in_reach [k, 4, 2] uint8: toe_dist under the 2 cm contact breaking threshold
          base_body [k, 9]: base linear velocity, angular velocity and the unit gravity direction, in the base frame
        and the properties foot_clearance [k, 4] (the nearer end) and foot_in_reach [k, 4] (either end).
        fields: the names to compute (default all; the others are None); unknown names raise ValueError.  out: an earlier result
        for the same fields and row count to refill -- checked once, then reused, so that a read every step allocates nothing.
        Every argument error is raised before any launch."""
        from .. import kinematics
        return kinematics.read(self, env_ids, fields, out)

    # ---- rigid-body dynamics (rex_gym_amd/dynamics.py) ----
    @property
    def dof_names(self):
        """The 18 names of the generalized velocity's components (rows and columns of dynamics()): six of the base -- world linear
        velocity of the base origin, world angular velocity -- then the motor names in motor order, from the model tables."""
        from .. import dynamics
        return dynamics.dof_names()

    def dynamics(self, env_ids=None, fields=None, out=None):
        """The equations of motion at the current state (rex_dynamics), in one read-only launch on the env's device and stream, no
        host sync:  M(q) vdot + bias(q, v) = S^T tau + sum_p J_p^T f_p  with v = (base linear velocity, base angular velocity, 12
        joint rates), world axes (env.dof_names).  Returns a dynamics.Dynamics whose attributes are float32 tensors of k rows
        (env_ids as in render(); default: every env, in order):
          mass_matrix [k, 18, 18]: M(q), symmetric
          bias [k, 18]: Coriolis, centrifugal and gyroscopic terms plus gravity (g = 10; at rest bias[0:3] = (0, 0, +mass * 10));
              the sim's damping forces are not part of it.  gravity [k, 18]: bias at v = 0
          toe_jacobian [k, 4, 2, 3, 18]: toe_vel = J v for the contact candidate at both ends of each toe (kinematics().toe_pos)
          com [k, 6]: centre of mass, world position and velocity (properties com_pos, com_vel)
          momentum [k, 6]: linear momentum, angular momentum about the centre of mass;  mass [k]: total mass
        Masses carry the env's base / leg mass scales of the current episode; rotational inertias do not, as in the step.
        fields, out: as in kinematics().  Mark 'arm' raises NotImplementedError.  Every argument error is raised before any launch."""
        from .. import dynamics
        return dynamics.read(self, env_ids, fields, out)

    def dynamics_solve(self, rhs, env_ids=None, out=None):
        """x = M(q)^-1 rhs at the current state (rex_dynamics_solve), one launch on the env's device and stream, no host sync; M is
        never written out.  rhs: float32 [k, 18] or [k, K, 18] on the device, contiguous (rows and env_ids as in dynamics()); returns
        a tensor of the same shape.  out: a tensor of that shape to fill; out=rhs solves in place.  The Delassus matrix of the toe
        points is J M^-1 J^T:  J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(k, 24, 18);
        W = torch.einsum("kpd,kqd->kpq", J, env.dynamics_solve(J)).  Mark 'arm' raises NotImplementedError.  Every argument error is
        raised before any launch."""
        from .. import dynamics
        return dynamics.solve(self, rhs, env_ids, out)

    def forward_dynamics(self, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
        """vdot [k, 18] = M^-1 (S^T tau + sum_p J_p^T f_p + w - bias) at the current state (rex_forward_dynamics): the acceleration
        the rigid-body equation of dynamics() gives for joint torques tau [k, 12], world forces toe_forces [k, 4, 2, 3] at the toe
        points (kinematics().toe_pos) and base_wrench [k, 6] -- a world force at the base origin, then a world moment.  float32
        device tensors; one without the row dimension ([12], [4, 2, 3], [6]) holds for every row; None is zero, and at least one
        must be given.  Like bias it leaves out the sim's damping, joint limits, contacts and the on_rack anchor.  Read-only."""
        from .. import dynamics
        return dynamics.forward(self, tau, toe_forces, base_wrench, env_ids, out)

    def push(self, base_impulse=None, toe_impulses=None, joint_impulses=None, env_ids=None, out=None):
        """An external push between two control steps (rex_apply_impulse): the impulses -- base_impulse [k, 6] (N s at the base
        origin, then N m s), toe_impulses [k, 4, 2, 3] at the toe points, joint_impulses [k, 12]; shapes and None as the loads of
        forward_dynamics() -- change the generalized velocity by dv = M^-1 (generalized impulse).  dv [k, 18] is ADDED to the
        base's linear and angular velocity and the joint rates of the envs in the state, and returned.  Nothing else in the state
        changes; the next step() starts from the pushed velocities.  Raises before any launch: before the first reset()
        (RuntimeError), duplicate env_ids (ValueError), mark 'arm' (NotImplementedError), an on_rack env (ValueError)."""
        from .. import dynamics
        return dynamics.push(self, base_impulse, toe_impulses, joint_impulses, env_ids, out)

    # ---- the contact solve (rex_gym_amd/contact.py) ----
    def contact_solve(self, tau=None, env_ids=None, fields=None, out=None, dt=None, iterations=None, residual_threshold=None, damping=True):
        """Ground reaction forces, joint-limit torques and the contact-consistent next velocity at the current state
        (rex_contact_solve): ONE substep of the step's physics -- free velocity under tau [k, 12] or [12] (None: zero), the toe
        rows and joint-limit rows, the step's projected Gauss-Seidel -- restated and solved in a read-only launch on the env's
        device and stream, no host sync; the state is never written.  Returns a contact.ContactSolve whose attributes are
        tensors of k rows (env_ids as in render()), conventions of dynamics():
          toe_force [k, 4, 2, 3]: world force on the foot at kinematics().toe_pos, N (impulse / dt); 0 for a point out of reach
          toe_lambda [k, 4, 2, 3]: the (normal, t1, t2) impulses, N s;  limit_torque [k, 12]: the limit rows' joint torque, N m
          v_next [k, 18]: clamp(v* + dv, +-100);  sweeps [k] int32: the env's own sweep count
        and the properties foot_force [k, 4, 3] and foot_contact [k, 4] bool.  dt, iterations (at most 1000), residual_threshold:
        None takes the config's; residual_threshold=0 runs every env for `iterations` sweeps.  damping=False leaves the sim's
        damping forces out: v_next = v + dt forward_dynamics(tau + limit_torque, toe_force) then.  For the step's own forces
        the caller supplies tau: the step draws it from the motor model in every substep (rex_motor_torque_params reproduces it)
        and the state holds no last torque.  fields, out: as in kinematics().  Mark 'arm' raises NotImplementedError; on_rack and
        body_contacts envs raise ValueError (the anchor and the link-box rows are not restated).  Every argument error is
        raised before any launch."""
        from .. import contact
        return contact.solve(self, tau, env_ids, fields, out, dt, iterations, residual_threshold, damping)

    # ---- candidate rollouts (rex_gym_amd/rollout.py) ----
    def rollout(self, targets=None, tau=None, repeat=None, env_ids=None, fields=None, out=None, dt=None, iterations=None, residual_threshold=None,
                init_state=None, base_wrench=None, body=None):
        """Where every env is after T control steps under each of K candidate command sequences (rex_rollout): simulated from the
        current state on a private copy, in ONE read-only launch on the env's device and stream, no host sync; the state is never
        written.  Commands: exactly one of targets -- motor angle commands, rad, what info['action'] holds -- and tau -- joint
        torques, N m --, a float32 device tensor [k, K, T, 12], contiguous (k rows: env_ids as in render(); default every env, in
        order).  The command of control step t holds for `repeat` substeps (None: the config's action_repeat; T x repeat <= 4096).
        One substep: the torque -- the step's motor model on (command, q, qd, qd) with the config's gains, or the env's actuator
        parameters when set_motor_params / motor randomisation is in effect, times the env's motor enable bit as it stands now; or
        tau as given --, then v_next of contact_solve() under it (toe rows and joint-limit rows, the env's mass scales, friction and
        terrain field of its current episode), then the step's integrator.  dt, iterations (at most 1000), residual_threshold: as
        in contact_solve().  Returns a rollout.Rollout that unpacks like the namedtuple (state, trajectory, foot_contact, sweeps):
          state [k, K, 37]: the state's words 0..36 after the last substep -- position 0:3, quaternion 3:7 (x y z w), linear velocity
              7:10, angular velocity 10:13, joint angles 13:25, joint rates 25:37;  trajectory [k, K, T, 37]: after every control step
          foot_contact [k, K, T, 4] uint8: a positive normal impulse at either end of the leg's toe in the control step's last substep
          sweeps [k, K] int32: solver sweeps summed over the substeps
        NOT advanced: the overheat counters and the motor mask, controller and gait words, step and episode counters (no reset, no
        done), sensor noise.  fields, out: as in kinematics().  Mark 'arm' raises NotImplementedError; on_rack, body_contacts and
        latency-model envs raise ValueError (the anchor, the link-box rows and the observation ring are not restated).  Every argument
        error is raised before any launch.
        Per-row inputs in place of the env's own (rex_rollout_from; float32 device tensors, contiguous, each may be None):
          init_state [k, K, 37] or [k, 37] (every candidate alike): the words 0..36 each row starts from -- a previous call's `state`
              continues that rollout bit for bit (beam search, horizons past 4096 substeps); an estimated or perturbed state.  Taken as
              given: not normalised, not checked; a bad row yields garbage in that row only
          base_wrench [k, K, T, 6]: a world force at the base origin, N, and a world moment, N m (forward_dynamics()' convention), held
              over the control step's substeps: v* = v + dt M^-1 (S^T tau + w - bias - damping)
          body [k, K, 3]: base mass scale, leg mass scale, toe friction of the row (set_body_params' triple)
        The terrain field, the actuator parameters and the motor enable bits stay the env's.  With all three None the call is
        rex_rollout as before."""
        from .. import rollout
        return rollout.run(self, targets, tau, repeat, env_ids, fields, out, dt, iterations, residual_threshold, init_state, base_wrench, body)

    # ---- the controller as a readout, rollouts in the action space (rex_gym_amd/rollout_actions.py) ----
    def command(self, actions, state=None, ctrl=None, env_ids=None, out=None):
        """ONE control step of the env's own controller per row and nothing else (rex_command): what env.step(actions) does between
        loading the env and its first substep -- ClipAction + RangeNormalize when range_normalize is set, the task's command with its
        goal, brake and hold latches, the gait planner and the inverse kinematics -- in one small read-only launch of the step kernels'
        own functions, no host sync; the state is never written.  actions: float32 device tensor [k, K, A], contiguous ([k, A]: K = 1;
        k rows: env_ids as in render(), no env twice), taken as given as step(check_actions=False) takes them.  state [k, K, 37] (or
        [k, 37]): the words 0..36 of the row, of which position and quaternion are read (None: the env's).  ctrl [k, K, 8] (or [k, 8]):
        the controller words 37..44 as the state block holds them, ints as bit patterns (None: the env's).  Returns (targets [k, K, 12],
        what info['action'] of the step would hold; ctrl [k, K, 8], the words as the step would store them for an env whose step returns
        done = 0: steps + 1, target = |target|, REX_F_DONE never set).  out=(targets, ctrl): refilled in place.  Sensor noise is not
        drawn: the turn goal test sees the row's true yaw.  Mark 'arm' raises NotImplementedError; mixed batches and latency-model envs
        raise ValueError.  Every argument error is raised before any launch."""
        from .. import rollout_actions
        return rollout_actions.command(self, actions, state, ctrl, env_ids, out)

    def rollout_actions(self, actions, repeat=None, init_state=None, ctrl=None, base_wrench=None, body=None, env_ids=None, fields=None, out=None,
                        dt=None, iterations=None, residual_threshold=None):
        """Where every row is after T control steps under ACTIONS of the env's own action space (rex_rollout_actions): per control step
        command() on the row's current (state, ctrl), then rollout()'s kernel for one control step from the previous state -- 2 T
        launches enqueued by one call on the env's device and stream, no host sync, no copies; the state is never written.  Every
        per-step tensor is TIME-MAJOR, as in step_segment: actions float32 [T, k, K, A] ([T, k, A]: K = 1), base_wrench [T, k, K, 6].
        init_state [k, K, 37] or [k, 37], body [k, K, 3]: as in rollout().  ctrl [k, K, 8] or [k, 8]: the controller words each row
        starts from (None: the env's).  repeat, dt, iterations, residual_threshold: the PHYSICS' settings as in rollout() (T x repeat <=
        4096); the controller's clock stays the env's, action_repeat x dt of the config per control step.  Returns a
        rollout_actions.ActionRollout that unpacks like the namedtuple (state, trajectory, foot_contact, sweeps, ctrl, ctrl_trajectory,
        targets):
          state [k, K, 37], ctrl [k, K, 8]: after the last step -- handed back as init_state= and ctrl= they continue the rollout bit for bit
          trajectory [T, k, K, 37], ctrl_trajectory [T, k, K, 8], targets [T, k, K, 12], foot_contact [T, k, K, 4] uint8, sweeps [T, k, K]
              int32: per control step (sweeps is not summed over the steps)
        with the views of rollout()'s result (base_pos, ..., joint_rates) and flags, steps: int32 views of ctrl.  A single
        rollout(targets=ro.targets.permute(1, 2, 0, 3).contiguous(), ...) reproduces state, trajectory and foot_contact bit for bit.
        Named in fields= beside them (never computed otherwise; fields=None stays those seven), the step's epilogue per control step, in
        the same 2 T launches (rex_rollout_actions_outcome): reward [T, k, K], done [T, k, K] uint8, obs [T, k, K, obs_dim] -- bit for
        bit outcome(trajectory[t], ctrl_trajectory[t], motor_torque[t]) -- and motor_torque [T, k, K, 12], the observed motor torques
        of each step's last substep (not masked by the motor enable bits).  Rows run on after done: mask with the running OR of done
        (rex_gym_amd/rollout_actions.py shows a discounted return in three lines).
        NOT advanced: the overheat counters and the motor mask, resets, episode counters, sensor noise.  fields, out: as
        in kinematics(); the workspace is allocated once per shape and kept.  Refuses what command() and rollout() refuse (mark 'arm',
        mixed, latency, on_rack, body_contacts).  Every argument error is raised before any launch."""
        from .. import rollout_actions
        return rollout_actions.run(self, actions, repeat, init_state, ctrl, base_wrench, body, env_ids, fields, out, dt, iterations, residual_threshold)

    # ---- the step's epilogue as a readout (rex_gym_amd/outcome.py) ----
    def outcome(self, state=None, ctrl=None, motor_torque=None, env_ids=None, fields=None, out=None):
        """What env.step() would SAY of a row whose control step ended in the given state (rex_outcome): reward, done and observation in
        one small read-only launch of the step kernels' own functions, no host sync; the state is never written.  state [k, K, 37] (or
        [k, 37]): the words 0..36 AFTER the control step (None: the env's).  ctrl [k, K, 8] (or [k, 8]): the controller words 37..44
        after it, as command()'s second result and the state block hold them -- target already |target|, steps already + 1; the done flag
        in them is ignored (None: the env's).  motor_torque [k, K, 12] (or [k, 12]): the OBSERVED motor torques of the step's last
        substep, as rollout_actions' motor_torque holds them (None: zeros -- the reward's energy term is left out).  k rows: env_ids
        as in render(), no env twice.  Returns an outcome.Outcome with reward [k, K], done [k, K] uint8, obs [k, K, obs_dim] -- [k],
        [k], [k, obs_dim] when no input carries a candidate axis --: the forward reward's branches under forward_reward_cap, drift, shake
        and energy = -|sum tau x qd| x dt, or the turn, standup, poses reward; r22 < 0.85 or the gallop / standup roll-pitch-y test, the
        goal flag, max_episode_steps; roll, pitch and their rates, the gallop env's motor angles, RangeNormalize when range_normalize is
        set.  Sensor noise is not drawn; there is NO reset: on an auto_reset env obs is the terminal observation, which step() never
        returns.  fields, out: as in kinematics().  Mark 'arm' raises NotImplementedError; mixed batches and latency-model envs raise
        ValueError.  Every argument error is raised before any launch."""
        from .. import outcome
        return outcome.run(self, state, ctrl, motor_torque, env_ids, fields, out)

    # ---- the acceleration level (rex_gym_amd/contact_space.py) ----
    def inverse_dynamics(self, vdot=None, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
        """need [k, 18] = M vdot + bias - S^T tau - sum_p J_p^T f_p - w at the current state (rex_inverse_dynamics): the equation of
        forward_dynamics() solved for the force, one read-only launch, M never written out.  vdot [k, 18] is the wanted generalized
        acceleration; tau [k, 12], toe_forces [k, 4, 2, 3] and base_wrench [k, 6] are what is applied already (shapes, broadcasting
        and None = zero as in forward_dynamics(); all None is allowed: need = bias).  need[:, 6:] is the joint torque still
        needed; need[:, :6] is the force at the base origin and the moment that nothing supplies -- zero for a motion the given
        ground forces can produce.  Mark 'arm' raises NotImplementedError.  Every argument error is raised before any launch."""
        from .. import contact_space
        return contact_space.inverse(self, vdot, tau, toe_forces, base_wrench, env_ids, out)

    def contact_space(self, tau=None, base_wrench=None, fields=None, env_ids=None, out=None):
        """The contact-space quantities of the 8 toe points at the current state (rex_contact_space), one read-only launch on the
        env's device and stream, no host sync.  Returns a contact_space.ContactSpace whose attributes are float32 tensors of k rows
        (env_ids as in render()), conventions of dynamics():
          delassus [k, 24, 24]: J M^-1 J^T, row and column 3 p + c for point p = 2 leg + end and world axis c, for all eight
              points whether in reach or not; symmetric, both triangles the same bits
          toe_drift [k, 4, 2, 3]: Jdot v, the acceleration of the foot's material point at kinematics().toe_pos when vdot = 0
          toe_acc_free [k, 4, 2, 3]: J M^-1 (S^T tau + w - bias) + toe_drift for joint torques tau [k, 12] or [12] and
              base_wrench [k, 6] or [6] (None: zero): the toe acceleration with no ground force
        With ground forces f the toe acceleration is toe_acc_free + delassus f.  fields, out: as in kinematics().  Mark 'arm'
        raises NotImplementedError.  Every argument error is raised before any launch."""
        from .. import contact_space
        return contact_space.read(self, tau, base_wrench, fields, env_ids, out)

    # ---- force distribution (rex_gym_amd/force_distribution.py) ----
    def force_distribution(self, vdot=None, base_wrench=None, stance=None, weights=None, eps=None, friction_scale=1.0, iterations=None,
                           fields=None, env_ids=None, out=None):
        """Which ground forces inside the friction cones produce the acceleration vdot [k, 18] (None: zero, "hold still") under the
        base wrench base_wrench [k, 6] (None: zero), and which joint torques go with them (rex_force_distribution): one read-only
        launch on the env's device and stream, no host sync.  With r = (M vdot + bias - base_wrench)[:6], the base rows no motor
        supplies, and A f = (sum_p f_p, sum_p (toe_pos_p - base origin) x f_p), it solves per env
            minimise 1/2 (A f - r)^T diag(weights) (A f - r) + 1/2 eps sum_p |f_p|^2
        over f_p in the circular cone |tangential| <= mu_p normal about the ground normal at the toe point, mu_p = friction_scale x
        the env's foot friction, and f_p = 0 for the points outside the stance set, by exactly `iterations` accelerated
        projected-gradient steps from zero (no early exit: judge convergence from `residual`).  stance: bool or uint8 [k, 4] on
        the device, per leg (both ends of its toe); None: every point kinematics().toe_in_reach reports.  weights: 6 positive
        numbers (None: 1, 1, 1, 100, 100, 100 -- a moment counted over a 0.1 m lever); eps > 0 (None: 0.01) makes the solution
        unique and shrinks it: A f falls short of a reachable r by the order of eps / sigma_min(A)^2; iterations: 1 .. 10000
        (None: force_distribution.ITERATIONS).  Returns a force_distribution.ForceDistribution of float32 tensors of k rows:
          toe_force [k, 4, 2, 3]: world N at kinematics().toe_pos;  tau [k, 12]: (M vdot + bias)[6:] - (sum_p J_p^T f_p)[6:], no
          damping, joint-limit or motor terms;  base_residual [k, 6]: r - A f;  residual [k]: the fixed-point residual, N
        fields, env_ids, out: as in contact_space().  Mark 'arm' raises NotImplementedError; on_rack and body_contacts envs raise
        ValueError.  Every argument error is raised before any launch."""
        from .. import force_distribution
        return force_distribution.solve(self, vdot, base_wrench, stance, weights, eps, friction_scale, iterations, fields, env_ids, out)

    def _action_bounds(self):
        if self._act_lo is None:
            torch = self._torch
            self._act_lo = torch.as_tensor(np.minimum(self.action_space.low, self.action_space.high).astype(np.float32), device=self.device)
            self._act_hi = torch.as_tensor(np.maximum(self.action_space.low, self.action_space.high).astype(np.float32), device=self.device)
        return self._act_lo, self._act_hi

    def step_segment(self, actions, out=None, motor_cmd=None):
        """A rollout segment in ONE launch (rex_step_segment): actions [T, N, action_dim] that the caller already holds -- an
        open-loop rollout: random-action throughput runs, a replayed action tape -- gives (obs [T, N, O], reward [T, N],
        done [T, N] bool), bit-identical to T calls of step() on the slices.  A wave goes on to its envs' next step as soon as it
        has finished this one, so the launch ends with the largest sum of a wave's step times instead of paying the slowest wave of
        every step.  The reference has no counterpart (its envs take one action at a time); step() is unchanged.

        out=(obs, reward, done): contiguous device tensors of those shapes (done uint8 or bool) the launch writes into.
        motor_cmd: optional [T, N, num_motors] float32 tensor for info['action'] of every step (without it info['action'] is None:
        a segment does not record the motor commands unless asked to).  Per-step randomizers
        (randomize_step) and the per-step Box test do not fit a segment: envs that use them raise."""
        torch = self._torch
        if self._needs_reset:
            raise RuntimeError("Must reset environment.")
        if any(hasattr(r, "randomize_step") for r in self._env_randomizers):
            raise ValueError("step_segment: a randomizer with randomize_step() acts between steps; use step()")
        with self._on_stream():
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
            if a.dim() != 3 or a.shape[1:] != (self.num_envs, self.action_dim) or a.shape[0] < 1:
                raise ValueError(f"actions must have shape (T, {self.num_envs}, {self.action_dim}), got {tuple(a.shape)}")
            a = a.contiguous()
            T = int(a.shape[0])
            if self.check_actions:     # the Box test of BatchEnv.step on the whole segment up front: one host synchronisation
                bad = ~torch.isfinite(a)
                if not self.config.range_normalize:
                    lo, hi = self._action_bounds()
                    bad |= (a < lo) | (a > hi)
                if bool(bad.any()):
                    t, i = (int(v) for v in torch.nonzero(bad.any(dim=2))[0])
                    raise ValueError(f"Invalid action at step {t}, index {i}: {a[t, i].tolist()}")
            if out is None:
                out = (torch.empty((T, self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device),
                       torch.empty((T, self.num_envs), dtype=torch.float32, device=self.device),
                       torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device))
            obs, reward, done = out
            for t_, shape, dt in ((obs, (T, self.num_envs, self.obs_dim), (torch.float32,)), (reward, (T, self.num_envs), (torch.float32,)),
                                  (done, (T, self.num_envs), (torch.uint8, torch.bool))):
                if tuple(t_.shape) != shape or t_.dtype not in dt or not t_.is_contiguous() or t_.device != self.device:
                    raise ValueError(f"out tensors must be contiguous on {self.device}: obs {(T, self.num_envs, self.obs_dim)} float32, "
                                     f"reward {(T, self.num_envs)} float32, done {(T, self.num_envs)} uint8 / bool")
            p_cmd = None
            if motor_cmd is not None:
                nm = self._info["action"].shape[1]
                if tuple(motor_cmd.shape) != (T, self.num_envs, nm) or motor_cmd.dtype != torch.float32 or not motor_cmd.is_contiguous() \
                        or motor_cmd.device != self.device:
                    raise ValueError(f"motor_cmd must be a contiguous float32 tensor of shape {(T, self.num_envs, nm)} on {self.device}")
                p_cmd = motor_cmd.data_ptr()
        _lib.check(self._L.rex_step_segment(self._h, T, a.data_ptr(), obs.data_ptr(), reward.data_ptr(), done.data_ptr(), p_cmd, self._stream_ptr()),
                   "rex_step_segment")
        return obs, reward, (done if done.dtype == torch.bool else done.view(torch.bool)), {"action": motor_cmd}

    # ---- the actor inside the launch (rex_set_policy / rex_step_policy / rex_step_segment_policy) ----
    def set_policy(self, w1=None, b1=None, w2=None, b2=None, w3=None, b3=None, logstd=None, obs_mean=None, obs_scale=None, obs_clip=5.0, sample=True, seed=0):
        """Install the actor the closed-loop launches evaluate (include/rexsim.h `RexPolicy`): the reference's ForwardGaussianPolicy
        (agents/scripts/networks.py:66-110) behind its observ filter (agents/ppo/normalize.py:47-66).  Contiguous float32 device
        tensors, INPUT-major weights: w1 [obs_dim, h1], w2 [h1, h2], w3 [h2, action_dim] (the transpose of torch.nn.Linear.weight),
        biases and logstd as vectors, obs_mean / obs_scale [obs_dim] or both None.  The library snapshots them (a packing kernel on the
        env's stream): call set_policy again after the weights or the filter statistics have changed; set_policy(None) removes the policy.
        The env must have been created with range_normalize=True (the agents act through RangeNormalize + ClipAction)."""
        torch = self._torch
        if w1 is None:
            _lib.check(self._L.rex_set_policy(self._h, None, None), "rex_set_policy")
            self._policy = None
            return
        ts = dict(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, logstd=logstd)
        if (obs_mean is None) != (obs_scale is None):
            raise ValueError("obs_mean and obs_scale go together")
        if obs_mean is not None:
            ts.update(obs_mean=obs_mean, obs_scale=obs_scale)
        for name, t in ts.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"set_policy: {name} must be a contiguous float32 tensor on {self.device}")
        h1, h2 = int(w1.shape[1]) if w1.dim() == 2 else -1, int(w2.shape[1]) if w2.dim() == 2 else -1
        want = dict(w1=(self.obs_dim, h1), b1=(h1,), w2=(h1, h2), b2=(h2,), w3=(h2, self.action_dim), b3=(self.action_dim,),
                    logstd=(self.action_dim,), obs_mean=(self.obs_dim,), obs_scale=(self.obs_dim,))
        for name, t in ts.items():
            if tuple(t.shape) != want[name]:
                raise ValueError(f"set_policy: {name} has shape {tuple(t.shape)}, expected {want[name]}")
        pol = _lib.RexPolicy()
        pol.obs_dim, pol.action_dim, pol.hidden1, pol.hidden2 = self.obs_dim, self.action_dim, h1, h2
        for name in ("w1", "b1", "w2", "b2", "w3", "b3", "logstd", "obs_mean", "obs_scale"):
            setattr(pol, "d_" + name, ts[name].data_ptr() if name in ts else None)
        pol.obs_clip, pol.sample, pol.seed = float(obs_clip), int(bool(sample)), int(seed) & (2 ** 64 - 1)
        _lib.check(self._L.rex_set_policy(self._h, ctypes.byref(pol), self._stream_ptr()), "rex_set_policy")
        self._policy = True

    def set_policy_recurrent(self, w1=None, b1=None, wg=None, bg=None, wc=None, bc=None, w3=None, b3=None, logstd=None, state=None,
                             obs_mean=None, obs_scale=None, obs_clip=5.0, sample=True, seed=0):
        """Install the RECURRENT actor (include/rexsim.h `RexRecurrentPolicy`): the reference's RecurrentGaussianPolicy
        (agents/scripts/networks.py:113-159) -- one ReLU layer, then TensorFlow's GRU cell of S units, then the tanh mean layer.  As
        set_policy: contiguous float32 device tensors, INPUT-major weights: w1 [obs_dim, h1], wg [h1 + S, 2 S] (inputs x then h, units r
        then u), wc [h1 + S, S], w3 [S, action_dim].  The weights are snapshotted; `state` [S, num_envs] is not: the launches read and
        write it at every step, reset() zeroes the rows (columns of this tensor) of the envs it resets, and it must stay alive while
        the policy is installed (the env keeps a reference).  set_policy_recurrent(None) removes the policy."""
        torch = self._torch
        if w1 is None:
            _lib.check(self._L.rex_set_policy_recurrent(self._h, None, None), "rex_set_policy_recurrent")
            self._policy = None
            self._policy_state = None
            return
        ts = dict(w1=w1, b1=b1, wg=wg, bg=bg, wc=wc, bc=bc, w3=w3, b3=b3, logstd=logstd, state=state)
        if (obs_mean is None) != (obs_scale is None):
            raise ValueError("obs_mean and obs_scale go together")
        if obs_mean is not None:
            ts.update(obs_mean=obs_mean, obs_scale=obs_scale)
        for name, t in ts.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"set_policy_recurrent: {name} must be a contiguous float32 tensor on {self.device}")
        h1, S = int(w1.shape[1]) if w1.dim() == 2 else -1, int(wc.shape[1]) if wc.dim() == 2 else -1
        want = dict(w1=(self.obs_dim, h1), b1=(h1,), wg=(h1 + S, 2 * S), bg=(2 * S,), wc=(h1 + S, S), bc=(S,), w3=(S, self.action_dim),
                    b3=(self.action_dim,), logstd=(self.action_dim,), state=(S, self.num_envs), obs_mean=(self.obs_dim,), obs_scale=(self.obs_dim,))
        for name, t in ts.items():
            if tuple(t.shape) != want[name]:
                raise ValueError(f"set_policy_recurrent: {name} has shape {tuple(t.shape)}, expected {want[name]}")
        pol = _lib.RexRecurrentPolicy()
        pol.obs_dim, pol.action_dim, pol.hidden1, pol.state_size = self.obs_dim, self.action_dim, h1, S
        for name in ("w1", "b1", "wg", "bg", "wc", "bc", "w3", "b3", "logstd", "obs_mean", "obs_scale", "state"):
            setattr(pol, "d_" + name, ts[name].data_ptr() if name in ts else None)
        pol.obs_clip, pol.sample, pol.seed = float(obs_clip), int(bool(sample)), int(seed) & (2 ** 64 - 1)
        _lib.check(self._L.rex_set_policy_recurrent(self._h, ctypes.byref(pol), self._stream_ptr()), "rex_set_policy_recurrent")
        self._policy = True
        self._policy_state = state

    def _policy_blocks(self, T, obs_in, out, action, mean, motor_cmd):
        torch = self._torch
        if self._needs_reset:
            raise RuntimeError("Must reset environment.")
        if getattr(self, "_policy", None) is None:
            raise RuntimeError("no policy set: call set_policy(...) first")
        if any(hasattr(r, "randomize_step") for r in self._env_randomizers):
            raise ValueError("a randomizer with randomize_step() acts between steps on the host; use step()")
        n, lead = self.num_envs, ((T,) if T is not None else ())
        def block(t, shape, dts, name):
            if t is None:
                return torch.empty(lead + shape, dtype=dts[0], device=self.device)
            if tuple(t.shape) != lead + shape or t.dtype not in dts or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous {dts[0]} tensor of shape {lead + shape} on {self.device}")
            return t
        if not isinstance(obs_in, torch.Tensor) or tuple(obs_in.shape) != (n, self.obs_dim) or obs_in.dtype != torch.float32 \
                or not obs_in.is_contiguous() or obs_in.device != self.device:
            raise ValueError(f"obs_in must be a contiguous float32 tensor of shape {(n, self.obs_dim)} on {self.device}")
        o, r, d = out if out is not None else (None, None, None)
        o = block(o, (n, self.obs_dim), (torch.float32,), "out obs")
        r = block(r, (n,), (torch.float32,), "out reward")
        d = block(d, (n,), (torch.uint8, torch.bool), "out done")
        action = block(action, (n, self.action_dim), (torch.float32,), "action")
        mean = block(mean, (n, self.action_dim), (torch.float32,), "mean")
        if motor_cmd is not None:
            motor_cmd = block(motor_cmd, (n, self.num_motors), (torch.float32,), "motor_cmd")
        return obs_in, o, r, d, action, mean, motor_cmd

    def step_policy(self, obs_in, out=None, action=None, mean=None, motor_cmd=None):
        """One CLOSED-LOOP env.step() of every env in one launch (rex_step_policy): action = policy(obs_in) -- obs_in [N, obs_dim]
        is what the envs returned last (reset() or the previous step) --, then the step.  Returns (obs, reward, done, info) as
        step(); info['policy_action'] [N, A] is the action the policy took as the agent's memory stores it (before ClipAction /
        RangeNormalize), info['policy_mean'] its mean, info['action'] the motor commands (the tensor passed as motor_cmd, else None)."""
        torch = self._torch
        obs_in, o, r, d, action, mean, motor_cmd = self._policy_blocks(None, obs_in, out, action, mean, motor_cmd)
        _lib.check(self._L.rex_step_policy(self._h, obs_in.data_ptr(), action.data_ptr(), mean.data_ptr(), o.data_ptr(), r.data_ptr(), d.data_ptr(),
                                           motor_cmd.data_ptr() if motor_cmd is not None else None, self._stream_ptr()), "rex_step_policy")
        return o, r, (d if d.dtype == torch.bool else d.view(torch.bool)), {"action": motor_cmd, "policy_action": action, "policy_mean": mean}

    def step_segment_policy(self, num_steps, obs_in, out=None, action=None, mean=None, motor_cmd=None):
        """A closed-loop rollout SEGMENT in one launch (rex_step_segment_policy): T = num_steps consecutive step_policy() calls, step t
        acting on the observation of step t - 1 (obs_in for t = 0), bit-identical to them.  Blocks [T, N, ...]: returns (obs, reward,
        done, info) with info['policy_action'] / ['policy_mean'] [T, N, A].  A caller that keeps obs[T + 1, N, O] passes
        obs_in=obs[0], out=(obs[1:], reward, done): the policy's input of step t is obs[t]."""
        torch = self._torch
        T = int(num_steps)
        if T < 1:
            raise ValueError("num_steps must be at least 1")
        obs_in, o, r, d, action, mean, motor_cmd = self._policy_blocks(T, obs_in, out, action, mean, motor_cmd)
        _lib.check(self._L.rex_step_segment_policy(self._h, T, obs_in.data_ptr(), action.data_ptr(), mean.data_ptr(), o.data_ptr(), r.data_ptr(),
                                                   d.data_ptr(), motor_cmd.data_ptr() if motor_cmd is not None else None, self._stream_ptr()),
                   "rex_step_segment_policy")
        return o, r, (d if d.dtype == torch.bool else d.view(torch.bool)), {"action": motor_cmd, "policy_action": action, "policy_mean": mean}

    def bind_out(self, obs, reward, done):
        """Validate a set of output tensors once (`step(..., out=...)`): returns a StepOut that a loop can pass again and again."""
        torch = self._torch
        for t, shape, dt in ((obs, (self.num_envs, self.obs_dim), (torch.float32,)), (reward, (self.num_envs,), (torch.float32,)),
                             (done, (self.num_envs,), (torch.uint8, torch.bool))):
            if tuple(t.shape) != shape or t.dtype not in dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"out tensors must be contiguous on {self.device}: obs {(self.num_envs, self.obs_dim)} float32, "
                                 f"reward {(self.num_envs,)} float32, done {(self.num_envs,)} uint8 / bool")
        return StepOut(obs, reward, done, torch)
