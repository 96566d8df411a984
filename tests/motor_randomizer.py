"""An env_randomizer written against the REFERENCE's surface (rex_gym_env.py:345-346,400-401): it turns the actuator's knobs
through `env.rex._motor_model` (model/motor.py:40-74) and the PD gains Rex.ApplyAction hands to it (`env.rex._kp / _kd`,
rex.py:590-600).  The very same class drives the reference's env classes in tests/golden/make_motor_golden.py and this
project's env classes in tests/test_gpu_motor_params.py."""


class MotorRandomizer:
    def __init__(self, strength=None, voltage=None, damping=None, kp=None, kd=None):
        self.strength, self.voltage, self.damping, self.kp, self.kd = strength, voltage, damping, kp, kd

    def randomize_env(self, env):
        mm = env.rex._motor_model
        if self.strength is not None:
            mm.set_strength_ratios(self.strength)
        if self.voltage is not None:
            mm.set_voltage(self.voltage)
        if self.damping is not None:
            mm.set_viscous_damping(self.damping)
        if self.kp is not None:
            env.rex._kp = self.kp
        if self.kd is not None:
            env.rex._kd = self.kd

    def randomize_step(self, env):     # rex_gym_env.py:401 calls it on every step
        pass
