"""Worker of tests/test_gpu_parity.py::test_left_out_variant_group_is_an_error_return.  Runs in a subprocess with
    REX_LIB_PATH = rex_gym_amd/librexsim_hip_diag.so   (built with only="arm,mixed_arm": the other groups' launchers are not in it)
a base-mark sim cannot be created -- the package's ordinary error, naming the group, before any kernel launch -- and a mark-arm sim
in the same process resets and steps."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    assert os.environ.get("REX_LIB_PATH", "").endswith("librexsim_hip_diag.so")
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    try:
        RexBatchEnv(4, task="walk", signal_type="ik")
    except _lib.RexSimError as e:
        msg = str(e)
    else:
        raise AssertionError("a base-mark sim was created on a library without the base group")
    assert "rex_create" in msg and "variant group base" in msg and "REX_BUILD_ONLY" in msg, msg
    env = RexBatchEnv(4, task="walk", signal_type="ik", mark="arm")
    env.reset()
    obs, reward, done, _ = env.step(torch.zeros(4, env.action_dim, device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(reward).all()) and done.shape == (4,)
    env.close()
    print("ok: " + msg)


if __name__ == "__main__":
    main()
