"""ctypes binding of the C ABI in include/rexsim.h (librexsim_hip.so).

There is NO CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os

from . import build as _build

TASKS = {"walk": 0, "gallop": 1, "turn": 2, "poses": 3, "standup": 4, "mixed": 5}
SIGNALS = {"ik": 0, "ol": 1}
MARKS = {"base": 0, "arm": 1}
STATE_WORDS = 54      # mark 'base'; rex_state_words(cfg) for the others
NUM_MOTORS = 12       # mark 'base'; rex_num_motors(cfg) for the others
ABI_VERSION = 6


class RexConfig(ctypes.Structure):
    """Mirror of `struct RexConfig` (include/rexsim.h)."""
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("num_envs", ctypes.c_int32), ("env_index_base", ctypes.c_int32),
        ("task", ctypes.c_int32), ("signal", ctypes.c_int32), ("action_repeat", ctypes.c_int32),
        ("solver_iterations", ctypes.c_int32), ("sim_time_step", ctypes.c_float),
        ("motor_kp", ctypes.c_float), ("motor_kd", ctypes.c_float), ("backwards", ctypes.c_int32),
        ("target_position", ctypes.c_float), ("seed", ctypes.c_uint64), ("auto_reset", ctypes.c_int32),
        ("max_episode_steps", ctypes.c_int32), ("distance_weight", ctypes.c_float),
        ("energy_weight", ctypes.c_float), ("drift_weight", ctypes.c_float), ("shake_weight", ctypes.c_float),
        ("solver_residual_threshold", ctypes.c_float), ("target_orient", ctypes.c_float),
        ("init_orient", ctypes.c_float), ("orient_fixed", ctypes.c_int32), ("pose_index", ctypes.c_int32),
        ("pose_value", ctypes.c_float), ("range_normalize", ctypes.c_int32), ("pd_latency", ctypes.c_float), ("control_latency", ctypes.c_float),
        ("mark", ctypes.c_int32),
        ("gait_clock_scale", ctypes.c_float), ("body_contacts", ctypes.c_int32), ("noise_stdev", ctypes.c_float * 5),
        ("task_mix", ctypes.c_int32), ("mass_scale_lo", ctypes.c_float), ("mass_scale_hi", ctypes.c_float),
        ("friction_lo", ctypes.c_float), ("friction_hi", ctypes.c_float), ("init_height", ctypes.c_float), ("on_rack", ctypes.c_int32),
        ("forward_reward_cap", ctypes.c_float), ("gallop_no_angles", ctypes.c_int32),
    ]


class RexPolicy(ctypes.Structure):
    """Mirror of `struct RexPolicy` (include/rexsim.h): the actor evaluated inside the launch."""
    _fields_ = [
        ("obs_dim", ctypes.c_int32), ("action_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32), ("hidden2", ctypes.c_int32),
        ("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_w2", ctypes.c_void_p), ("d_b2", ctypes.c_void_p),
        ("d_w3", ctypes.c_void_p), ("d_b3", ctypes.c_void_p), ("d_logstd", ctypes.c_void_p),
        ("d_obs_mean", ctypes.c_void_p), ("d_obs_scale", ctypes.c_void_p),
        ("obs_clip", ctypes.c_float), ("sample", ctypes.c_int32), ("seed", ctypes.c_uint64),
    ]


class RexRecurrentPolicy(ctypes.Structure):
    """Mirror of `struct RexRecurrentPolicy` (include/rexsim.h): the recurrent actor (a GRU cell on a live per-env state)."""
    _fields_ = [
        ("obs_dim", ctypes.c_int32), ("action_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32), ("state_size", ctypes.c_int32),
        ("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_wg", ctypes.c_void_p), ("d_bg", ctypes.c_void_p),
        ("d_wc", ctypes.c_void_p), ("d_bc", ctypes.c_void_p), ("d_w3", ctypes.c_void_p), ("d_b3", ctypes.c_void_p), ("d_logstd", ctypes.c_void_p),
        ("d_obs_mean", ctypes.c_void_p), ("d_obs_scale", ctypes.c_void_p),
        ("obs_clip", ctypes.c_float), ("sample", ctypes.c_int32), ("seed", ctypes.c_uint64),
        ("d_state", ctypes.c_void_p),
    ]


class RexMotorRandom(ctypes.Structure):
    """Mirror of `struct RexMotorRandom` (include/rexsim.h): per-reset uniform ranges of the actuator's knobs (lo == hi == 0: not drawn)."""
    _fields_ = [("strength_lo", ctypes.c_float), ("strength_hi", ctypes.c_float), ("voltage_lo", ctypes.c_float), ("voltage_hi", ctypes.c_float),
                ("damping_lo", ctypes.c_float), ("damping_hi", ctypes.c_float), ("kp_lo", ctypes.c_float), ("kp_hi", ctypes.c_float),
                ("kd_lo", ctypes.c_float), ("kd_hi", ctypes.c_float), ("strength_per_motor", ctypes.c_int32)]


class RexCamera(ctypes.Structure):
    """Mirror of `struct RexCamera` (include/rexsim.h): the follow camera of rex_render (angles in degrees)."""
    _fields_ = [("distance", ctypes.c_float), ("yaw_deg", ctypes.c_float), ("pitch_deg", ctypes.c_float),
                ("fov_deg", ctypes.c_float), ("near_plane", ctypes.c_float), ("far_plane", ctypes.c_float)]


class RexDepthSensor(ctypes.Structure):
    """Mirror of `struct RexDepthSensor` (include/rexsim.h): a depth camera mounted on the base (vectors in the base frame)."""
    _fields_ = [("pos", ctypes.c_float * 3), ("fwd", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("fov_deg", ctypes.c_float), ("near_plane", ctypes.c_float), ("far_plane", ctypes.c_float),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("see_robot", ctypes.c_int32)]


class RexKinematicsOut(ctypes.Structure):
    """Mirror of `struct RexKinematicsOut` (include/rexsim.h): the device arrays rex_kinematics fills (a null one is skipped)."""
    _fields_ = [("link_pos", ctypes.c_void_p), ("link_quat", ctypes.c_void_p), ("link_linvel", ctypes.c_void_p), ("link_angvel", ctypes.c_void_p),
                ("toe_pos", ctypes.c_void_p), ("toe_vel", ctypes.c_void_p), ("toe_dist", ctypes.c_void_p), ("toe_normal", ctypes.c_void_p),
                ("toe_in_reach", ctypes.c_void_p), ("base_body", ctypes.c_void_p)]


class RexDynamicsOut(ctypes.Structure):
    """Mirror of `struct RexDynamicsOut` (include/rexsim.h): the device arrays rex_dynamics fills (a null one is skipped)."""
    _fields_ = [("mass_matrix", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gravity", ctypes.c_void_p), ("toe_jacobian", ctypes.c_void_p),
                ("com", ctypes.c_void_p), ("momentum", ctypes.c_void_p), ("mass", ctypes.c_void_p)]


class RexDynamicsLoad(ctypes.Structure):
    """Mirror of `struct RexDynamicsLoad` (include/rexsim.h): the device arrays of a load or an impulse (a null one is zero)."""
    _fields_ = [("joint", ctypes.c_void_p), ("toe", ctypes.c_void_p), ("base", ctypes.c_void_p)]


class RexContactSolveIn(ctypes.Structure):
    """Mirror of `struct RexContactSolveIn` (include/rexsim.h): the torques and the solver settings of rex_contact_solve (a value <= 0,
    for the threshold < 0, takes the config's)."""
    _fields_ = [("tau", ctypes.c_void_p), ("dt", ctypes.c_float), ("iterations", ctypes.c_int32), ("residual_threshold", ctypes.c_float),
                ("damping", ctypes.c_int32)]


class RexContactSolveOut(ctypes.Structure):
    """Mirror of `struct RexContactSolveOut` (include/rexsim.h): the device arrays rex_contact_solve fills (a null one is skipped)."""
    _fields_ = [("toe_force", ctypes.c_void_p), ("toe_lambda", ctypes.c_void_p), ("limit_torque", ctypes.c_void_p), ("v_next", ctypes.c_void_p),
                ("sweeps", ctypes.c_void_p)]


class RexRolloutIn(ctypes.Structure):
    """Mirror of `struct RexRolloutIn` (include/rexsim.h): the commands (exactly one of targets and tau), the shape and the solver settings
    of rex_rollout (repeat, dt, iterations <= 0, for the threshold < 0, take the config's)."""
    _fields_ = [("targets", ctypes.c_void_p), ("tau", ctypes.c_void_p), ("candidates", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("repeat", ctypes.c_int32), ("dt", ctypes.c_float), ("iterations", ctypes.c_int32), ("residual_threshold", ctypes.c_float)]


class RexRolloutOut(ctypes.Structure):
    """Mirror of `struct RexRolloutOut` (include/rexsim.h): the device arrays rex_rollout fills (a null one is skipped)."""
    _fields_ = [("state", ctypes.c_void_p), ("trajectory", ctypes.c_void_p), ("foot_contact", ctypes.c_void_p), ("sweeps", ctypes.c_void_p)]


class RexRolloutFrom(ctypes.Structure):
    """Mirror of `struct RexRolloutFrom` (include/rexsim.h): what rex_rollout_from takes per row in place of the env's own -- the state the
    row starts from, the base wrench of every control step, the body parameters (a null one: the env's, or no wrench)."""
    _fields_ = [("init_state", ctypes.c_void_p), ("base_wrench", ctypes.c_void_p), ("body", ctypes.c_void_p)]


class RexRolloutActionsIn(ctypes.Structure):
    """Mirror of `struct RexRolloutActionsIn` (include/rexsim.h): the time-major actions, the controller words the rows start from (null:
    the env's), then the shape and the solver settings as RexRolloutIn holds them."""
    _fields_ = [("actions", ctypes.c_void_p), ("ctrl", ctypes.c_void_p), ("candidates", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("repeat", ctypes.c_int32), ("dt", ctypes.c_float), ("iterations", ctypes.c_int32), ("residual_threshold", ctypes.c_float)]


class RexRolloutActionsOut(ctypes.Structure):
    """Mirror of `struct RexRolloutActionsOut` (include/rexsim.h): the device arrays rex_rollout_actions fills (a null one is skipped)."""
    _fields_ = [("state", ctypes.c_void_p), ("trajectory", ctypes.c_void_p), ("foot_contact", ctypes.c_void_p), ("sweeps", ctypes.c_void_p),
                ("ctrl", ctypes.c_void_p), ("ctrl_trajectory", ctypes.c_void_p), ("targets", ctypes.c_void_p)]


class RexOutcomeOut(ctypes.Structure):
    """Mirror of `struct RexOutcomeOut` (include/rexsim.h): the device arrays rex_outcome fills (a null one is skipped)."""
    _fields_ = [("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("obs", ctypes.c_void_p)]


class RexRolloutActionsOutcome(ctypes.Structure):
    """Mirror of `struct RexRolloutActionsOutcome` (include/rexsim.h): the time-major device arrays rex_rollout_actions_outcome fills beside
    RexRolloutActionsOut's (a null one is skipped)."""
    _fields_ = [("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("obs", ctypes.c_void_p), ("motor_torque", ctypes.c_void_p)]


class RexContactSpaceOut(ctypes.Structure):
    """Mirror of `struct RexContactSpaceOut` (include/rexsim.h): the device arrays rex_contact_space fills (a null one is skipped)."""
    _fields_ = [("delassus", ctypes.c_void_p), ("toe_drift", ctypes.c_void_p), ("toe_acc_free", ctypes.c_void_p)]


class RexForceDistributionParams(ctypes.Structure):
    """Mirror of `struct RexForceDistributionParams` (include/rexsim.h): the weights, the regulariser, the friction scale and the step
    count of rex_force_distribution."""
    _fields_ = [("weights", ctypes.c_float * 6), ("eps", ctypes.c_float), ("friction_scale", ctypes.c_float), ("iterations", ctypes.c_int32)]


class RexForceDistributionOut(ctypes.Structure):
    """Mirror of `struct RexForceDistributionOut` (include/rexsim.h): the device arrays rex_force_distribution fills (a null one is skipped)."""
    _fields_ = [("toe_force", ctypes.c_void_p), ("tau", ctypes.c_void_p), ("base_residual", ctypes.c_void_p), ("residual", ctypes.c_void_p)]


class RexPpoNet(ctypes.Structure):
    """Mirror of `struct RexPpoNet` (include/rexsim.h): a two-layer ReLU network of the fused learner, torch layout."""
    _fields_ = [("obs_dim", ctypes.c_int32), ("out_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32), ("hidden2", ctypes.c_int32),
                ("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_w2", ctypes.c_void_p), ("d_b2", ctypes.c_void_p),
                ("d_w3", ctypes.c_void_p), ("d_b3", ctypes.c_void_p), ("d_logstd", ctypes.c_void_p)]


class RexPpoBatch(ctypes.Structure):
    """Mirror of `struct RexPpoBatch` (include/rexsim.h): the episode memory one loss call runs over."""
    _fields_ = [("rows", ctypes.c_int32), ("steps", ctypes.c_int32), ("d_observ", ctypes.c_void_p),
                ("d_action", ctypes.c_void_p), ("d_old_mean", ctypes.c_void_p), ("d_old_logstd", ctypes.c_void_p),
                ("d_advantage", ctypes.c_void_p), ("d_return", ctypes.c_void_p), ("d_length", ctypes.c_void_p),
                ("penalty", ctypes.c_float), ("kl_cutoff", ctypes.c_float), ("kl_cutoff_coef", ctypes.c_float)]


class RexPpoGrad(ctypes.Structure):
    """Mirror of `struct RexPpoGrad` (include/rexsim.h): where the gradients go, shaped like the network's tensors."""
    _fields_ = [("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_w2", ctypes.c_void_p), ("d_b2", ctypes.c_void_p),
                ("d_w3", ctypes.c_void_p), ("d_b3", ctypes.c_void_p), ("d_logstd", ctypes.c_void_p)]


class RexPpoRnnNet(ctypes.Structure):
    """Mirror of `struct RexPpoRnnNet` (include/rexsim.h): the recurrent policy of the fused recurrent learner, torch layout."""
    _fields_ = [("obs_dim", ctypes.c_int32), ("out_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32), ("state", ctypes.c_int32),
                ("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_wg", ctypes.c_void_p), ("d_bg", ctypes.c_void_p),
                ("d_wc", ctypes.c_void_p), ("d_bc", ctypes.c_void_p), ("d_wm", ctypes.c_void_p), ("d_bm", ctypes.c_void_p),
                ("d_logstd", ctypes.c_void_p)]


class RexPpoRnnGrad(ctypes.Structure):
    """Mirror of `struct RexPpoRnnGrad` (include/rexsim.h): where the nine gradients go."""
    _fields_ = [("d_w1", ctypes.c_void_p), ("d_b1", ctypes.c_void_p), ("d_wg", ctypes.c_void_p), ("d_bg", ctypes.c_void_p),
                ("d_wc", ctypes.c_void_p), ("d_bc", ctypes.c_void_p), ("d_wm", ctypes.c_void_p), ("d_bm", ctypes.c_void_p),
                ("d_logstd", ctypes.c_void_p)]


class RexSimError(RuntimeError):
    pass


_lib = None

_SIGS = {
    "rex_default_config": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_action_dim": ([ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_obs_dim": ([ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_num_motors": ([ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_state_words": ([ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_create": ([ctypes.POINTER(RexConfig), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "rex_destroy": ([ctypes.c_void_p], ctypes.c_int),
    "rex_set_body_params": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_set_motor_params": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_set_motor_randomization": ([ctypes.c_void_p, ctypes.POINTER(RexMotorRandom)], ctypes.c_int),
    "rex_get_motor_params": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_set_history": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_set_terrain": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "rex_set_heightfield": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p], ctypes.c_int),
    "rex_reset": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_step": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_step_segment": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_set_policy": ([ctypes.c_void_p, ctypes.POINTER(RexPolicy), ctypes.c_void_p], ctypes.c_int),
    "rex_set_policy_recurrent": ([ctypes.c_void_p, ctypes.POINTER(RexRecurrentPolicy), ctypes.c_void_p], ctypes.c_int),
    "rex_step_policy": ([ctypes.c_void_p] + [ctypes.c_void_p] * 8, ctypes.c_int),
    "rex_step_segment_policy": ([ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 8, ctypes.c_int),
    "rex_set_timing": ([ctypes.c_void_p, ctypes.c_int], ctypes.c_int),
    "rex_last_step_ms": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "rex_ik_solve": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_void_p], ctypes.c_int),
    "rex_motor_torque": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
                         ctypes.c_int),
    "rex_motor_torque_params": ([ctypes.c_int] + [ctypes.c_void_p] * 8, ctypes.c_int),
    "rex_gait_loop": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p], ctypes.c_int),
    "rex_set_event_trace": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_envs_per_wave": ([ctypes.c_void_p], ctypes.c_int),
    "rex_mixed_slot_map": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int], ctypes.c_int),
    "rex_get_sweeps": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_step_times_ms": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int], ctypes.c_int),
    "rex_default_camera": ([ctypes.POINTER(RexCamera)], ctypes.c_int),
    "rex_render": ([ctypes.c_void_p, ctypes.POINTER(RexCamera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_render_set_visuals": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "rex_render_visual": ([ctypes.c_void_p, ctypes.POINTER(RexCamera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_default_depth_sensor": ([ctypes.POINTER(RexDepthSensor)], ctypes.c_int),
    "rex_sense_depth": ([ctypes.c_void_p, ctypes.POINTER(RexDepthSensor), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p],
                        ctypes.c_int),
    "rex_height_scan": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                         ctypes.c_void_p], ctypes.c_int),
    "rex_num_bodies": ([ctypes.POINTER(RexConfig)], ctypes.c_int),
    "rex_kinematics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexKinematicsOut), ctypes.c_void_p], ctypes.c_int),
    "rex_dynamics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexDynamicsOut), ctypes.c_void_p], ctypes.c_int),
    "rex_dynamics_solve": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_forward_dynamics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexDynamicsLoad), ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_apply_impulse": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexDynamicsLoad), ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_contact_solve": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexContactSolveIn), ctypes.POINTER(RexContactSolveOut),
                           ctypes.c_void_p], ctypes.c_int),
    "rex_rollout": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexRolloutIn), ctypes.POINTER(RexRolloutOut), ctypes.c_void_p],
                    ctypes.c_int),
    "rex_rollout_from": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexRolloutIn), ctypes.POINTER(RexRolloutFrom),
                          ctypes.POINTER(RexRolloutOut), ctypes.c_void_p], ctypes.c_int),
    "rex_command": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6, ctypes.c_int),
    "rex_rollout_actions_workspace_bytes": ([ctypes.c_int, ctypes.c_int], ctypes.c_longlong),
    "rex_rollout_actions": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexRolloutActionsIn), ctypes.POINTER(RexRolloutFrom),
                             ctypes.POINTER(RexRolloutActionsOut), ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p], ctypes.c_int),
    "rex_outcome": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                     ctypes.POINTER(RexOutcomeOut), ctypes.c_void_p], ctypes.c_int),
    "rex_rollout_actions_outcome": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RexRolloutActionsIn), ctypes.POINTER(RexRolloutFrom),
                                     ctypes.POINTER(RexRolloutActionsOut), ctypes.POINTER(RexRolloutActionsOutcome), ctypes.c_void_p, ctypes.c_longlong,
                                     ctypes.c_void_p], ctypes.c_int),
    "rex_inverse_dynamics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(RexDynamicsLoad), ctypes.c_void_p,
                              ctypes.c_void_p], ctypes.c_int),
    "rex_contact_space": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RexContactSpaceOut),
                           ctypes.c_void_p], ctypes.c_int),
    "rex_force_distribution": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(RexForceDistributionParams), ctypes.POINTER(RexForceDistributionOut), ctypes.c_void_p], ctypes.c_int),
    "rex_ppo_workspace_bytes": ([ctypes.c_int] * 6, ctypes.c_longlong),
    "rex_ppo_returns": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                         ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_ppo_policy_loss": ([ctypes.POINTER(RexPpoNet), ctypes.POINTER(RexPpoBatch), ctypes.POINTER(RexPpoGrad), ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_ppo_value_loss": ([ctypes.POINTER(RexPpoNet), ctypes.POINTER(RexPpoBatch), ctypes.POINTER(RexPpoGrad), ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_ppo_recurrent_workspace_bytes": ([ctypes.c_int] * 6, ctypes.c_longlong),
    "rex_ppo_recurrent_policy_loss": ([ctypes.POINTER(RexPpoRnnNet), ctypes.POINTER(RexPpoBatch), ctypes.POINTER(RexPpoRnnGrad), ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rex_last_error": ([], ctypes.c_char_p),
    "rex_abi_version": ([], ctypes.c_int),
}
EXPORTED_SYMBOLS = tuple(_SIGS)


def lib():
    """Load (once) the HIP library. Raises RexSimError if it is not there -- never falls back."""
    global _lib
    if _lib is None:
        path = _build.LIB_PATH
        if not os.path.exists(path):
            raise RexSimError(
                f"{path} is missing: build it with `python -m rex_gym_amd.build` (needs hipcc). "
                "rex_gym_amd has no CPU fallback.")
        # PyTorch first: it carries its own HIP runtime, and a process must not end up with two of them (the library would
        # bind to the system one if it were loaded before torch, and the second runtime to start sees no device)
        import torch  # noqa: F401
        l = ctypes.CDLL(path)
        l.rex_abi_version.restype = ctypes.c_int
        if l.rex_abi_version() != ABI_VERSION:
            raise RexSimError(f"{path}: ABI version {l.rex_abi_version()}, this package binds version {ABI_VERSION}: rebuild it "
                              "(`python -m rex_gym_amd.build`)")
        for name, (argtypes, restype) in _SIGS.items():
            try:
                fn = getattr(l, name)
            except AttributeError:      # the ABI header and the library disagree
                raise RexSimError(f"{path} does not export {name}: a stale build -- rebuild it (`python -m rex_gym_amd.build`)") from None
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().rex_last_error().decode("utf-8", "replace")
        raise RexSimError(f"{what} failed (code {rc}): {msg}")
