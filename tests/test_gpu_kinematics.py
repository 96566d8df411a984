"""Body and foot kinematics on the GPU (rex_kinematics, csrc/rex_kinematics.hip) against the float64 numpy reference of
tests/kinematics_ref.py: forward kinematics from tests/test_gpu_render.py, the textbook velocity recursion, the toe cylinder of
rex_render_gen.h, a two-stage ground query restated from the facet rule of the render tests.

States: synthetic, from fixed-seed generators (kinematics_ref.scene_states: bases within +-3 m, tilts up to 1.2 rad, joints anywhere
inside their limits, random twists, the lowest toe -0.01 .. 0.06 m from the ground), written into env.state behind a few real states
after 8 random steps; the last four columns of a large scene are the corner cases -- a base rolled exactly 90 degrees (toe axes
parallel to the plane's normal: the branch without a radial offset), an env beside the heightfield's footprint, an upside-down base,
an env at the origin with every velocity 0.  Scenes (kinematics_ref.SCENES): 1, 5, 67 and 130 envs (a partial 4-lane group, a partial
wave, a partial last workgroup), both marks, the plane, the reference's random terrain and a [2, 9, 13] pool with unequal cells and a
shifted origin, each with two episodes in use.

Bounds: 4 x the largest deviation of the reference evaluated in float32 from the same reference in float64, per field, over the
synthetic states of all scenes (tests/test_kinematics_host.py measures them without a GPU and holds BOUNDS to them):

    field         floor       bound      measure
    link_pos      6.291e-07   2.516e-06  m, largest component
    link_quat     1.126e-07   4.504e-07  1 - |q_gpu . q_ref|
    link_linvel   2.385e-06   9.540e-06  |dv| / max(1, |v|)
    link_angvel   3.863e-07   1.545e-06  |dw| / max(1, |w|)
    toe_pos       7.486e-07   2.994e-06  m
    toe_vel       3.178e-06   1.271e-05  |dv| / max(1, |v|)
    toe_dist      4.031e-07   1.612e-06  m
    toe_normal    1.002e-07   4.010e-07  largest component
    base_body     1.706e-07   6.823e-07  velocities relative as above, gravity direction absolute

Discrete outputs: on a heightfield a toe point is compared (all toe_* fields) only if the facets of both ground queries stay what they are
when the reference's query points move by the toe_pos bound in +-x and +-y; toe_in_reach must equal the reference wherever
|dist_ref - 0.02| exceeds the toe_dist bound.  At most 10 % of a scene's points may be left out either way (asserted; the reference
alone leaves out 0 of 3 608 synthetic points), and the kept points must cover the cases of assert_cases_cover."""
import ctypes

import numpy as np
import pytest

import kinematics_ref as kr
import test_gpu_render as col

pytestmark = pytest.mark.gpu

BOUNDS = {"link_pos": 2.516e-06, "link_quat": 4.504e-07, "link_linvel": 9.540e-06, "link_angvel": 1.545e-06, "toe_pos": 2.994e-06,
          "toe_vel": 1.271e-05, "toe_dist": 1.612e-06, "toe_normal": 4.010e-07, "base_body": 6.823e-07}
QUAT_NORM = 4 * 2.0 ** -23                 # a float32 vector normalised in float32: a few ulp of 1
TOE_FIELDS = ("toe_pos", "toe_vel", "toe_dist", "toe_normal")


# ---------------------------------------------------------------- the reference's side of a scene (no GPU needed)
def scene_reference(mark, n, ground, state, heights=None, mids=None, env_index_base=0):
    """Per env of a scene: dict(ref, ok [8], kind).  state: the env's state as numpy, or None for the synthetic columns alone (then the
    real columns are left out)."""
    arm = mark == "arm"
    S, kinds = kr.scene_states(arm, n, ground, kr.scene_keep(n))
    first = 0
    if state is None:
        state, first = S, kr.scene_keep(n)
    fields = kr.scene_fields(ground, heights, mids)
    episode = state[kr.episode_word(arm)].view(np.int32)
    rows = []
    for g in range(first, n):
        f = kr.field_of(fields, g, episode[g], env_index_base)
        r = kr.reference(state, g, arm, f)
        rows.append(dict(env=g, ref=r, ok=kr.stable_points(state, g, arm, f, r, BOUNDS["toe_pos"]), kind=kinds[g], field=f))
    return rows


def count_cases(rows, seen):
    """what the kept toe points of a scene exercise, from the reference alone"""
    for row in rows:
        r, ok = row["ref"], row["ok"]
        clear = ok & (np.abs(r["toe_dist"] - kr.BREAKING) > BOUNDS["toe_dist"])
        on_field = row["field"] is not None
        for name, mask in (("lower_triangle", on_field & (r["fid1"] > 0) & (r["fid1"] % 2 == 1)), ("upper_triangle", (r["fid1"] > 0) & (r["fid1"] % 2 == 0)),
                           ("plane_under_field", on_field & (r["fid1"] == 0)), ("tilted_first_normal", r["fid0"] > 0),
                           ("in_reach", clear & r["toe_in_reach"]), ("out_of_reach", clear & ~r["toe_in_reach"]), ("negative", r["toe_dist"] < 0),
                           ("degenerate", r["degenerate"]), ("off_footprint", on_field & (row["kind"] == "off")), ("upside_down", row["kind"] == "upside")):
            seen[name] = seen.get(name, 0) + int((ok & mask).sum())


def assert_cases_cover(seen):
    """Both triangle kinds, the plane inside a field's footprint, in-reach and out-of-reach points, negative distances, the degenerate-axis
    points and the env beside the footprint are among the compared points."""
    for name in ("lower_triangle", "upper_triangle", "plane_under_field", "tilted_first_normal", "in_reach", "out_of_reach", "negative"):
        assert seen.get(name, 0) >= 20, (name, seen)
    for name in ("degenerate", "off_footprint", "upside_down"):
        assert seen.get(name, 0) >= 8, (name, seen)


# ---------------------------------------------------------------- the GPU's side
def make_env(mark, n, ground, **extra):
    """The env of a scene: reset, 8 random steps, then the synthetic columns written over all but the first few envs.  `extra`: further
    keywords of RexBatchEnv (tests/test_gpu_step_readout.py)."""
    import torch
    from rex_gym_amd import RexBatchEnv
    kw = dict(task="walk", signal_type="ik", mark=mark, seed=5, **extra)
    if ground == "random":
        kw.update(terrain_type="random", terrain_pool=kr.POOL)
    elif ground == "custom":
        kw.update(terrain_type="custom", heightfield=kr.custom_fields(), heightfield_cell=kr.CUSTOM_CELL, heightfield_origin=kr.CUSTOM_ORIGIN,
                  init_height=0.6)
    env = RexBatchEnv(n, **kw)
    env.reset()
    col._steps(env, 8, seed=2)
    arm, keep = mark == "arm", kr.scene_keep(n)
    S, _ = kr.scene_states(arm, n, ground, keep)
    words, ew = 13 + 2 * kr.num_motors(arm), kr.episode_word(arm)
    dev = torch.as_tensor(S, device=env.device)            # float32 to float32: the episode word keeps its bits
    env.state[0:words, keep:] = dev[0:words, keep:]
    env.state[ew, keep:] = dev[ew, keep:]
    torch.cuda.synchronize()
    return env


def to_numpy(kin):
    """a Kinematics -> a dict of numpy arrays shaped as the reference's (toe arrays [k, 8, ...])"""
    out = {}
    for name in kin.fields:
        a = getattr(kin, name).cpu().numpy()
        out[name] = a.reshape((a.shape[0], 8) + a.shape[3:]) if name.startswith("toe_") else a
    return out


def check_rows(gpu, rows, what):
    """gpu: to_numpy() of rows' envs in order.  Every field against the reference at BOUNDS; -> (points, points left out)"""
    worst = {k: 0.0 for k in kr.FLOAT_FIELDS}
    points = left_out = 0
    failures = []
    for k, row in enumerate(rows):
        r, ok = row["ref"], row["ok"]
        e = kr.errors({name: gpu[name][k] for name in kr.FLOAT_FIELDS}, r)
        for name in kr.FLOAT_FIELDS:
            v = e[name][ok] if name in TOE_FIELDS else e[name]
            if v.size:
                worst[name] = max(worst[name], float(v.max()))
                if not np.all(v <= BOUNDS[name]):
                    failures.append((name, row["env"], row["kind"], float(v.max())))
        norm = np.linalg.norm(gpu["link_quat"][k].astype(np.float64), axis=-1)
        if not np.all(np.abs(norm - 1.0) <= QUAT_NORM):
            failures.append(("quat norm", row["env"], row["kind"], float(np.abs(norm - 1).max())))
        clear = ok & (np.abs(r["toe_dist"] - kr.BREAKING) > BOUNDS["toe_dist"])
        if not np.array_equal(gpu["toe_in_reach"][k][clear] != 0, r["toe_in_reach"][clear]):
            failures.append(("toe_in_reach", row["env"], row["kind"], 0.0))
        if not np.all(gpu["toe_in_reach"][k] <= 1):
            failures.append(("toe_in_reach is 0 or 1", row["env"], row["kind"], 0.0))
        points, left_out = points + 8, left_out + int((~clear).sum())
    print(what, "worst / bound:", {k: "%.2e / %.2e" % (worst[k], BOUNDS[k]) for k in kr.FLOAT_FIELDS}, "left out %d of %d" % (left_out, points))
    assert not failures, (what, failures[:8], len(failures))
    assert left_out <= 0.1 * points, (what, left_out, points)
    return points, left_out


@pytest.fixture(scope="module")
def scenes():
    """(mark, n, ground) -> (env, state numpy, reference rows, full readout as numpy), built once per scene"""
    import torch
    made = {}

    def get(mark, n, ground):
        key = (mark, n, ground)
        if key not in made:
            env = make_env(mark, n, ground)
            state = env.state.cpu().numpy()
            heights = env.terrain_heights.cpu().numpy() if ground != "plane" else None
            mids = env.terrain_mids.cpu().numpy() if ground != "plane" else None
            rows = scene_reference(mark, n, ground, state, heights, mids)
            kin = env.kinematics()
            torch.cuda.synchronize()
            made[key] = (env, state, rows, to_numpy(kin), kin)
        return made[key]
    yield get
    for env, *_ in made.values():
        env.close()


# ---------------------------------------------------------------- a. every scene against the reference
@pytest.mark.parametrize("mark,n,ground", kr.SCENES)
def test_scene_against_the_reference(scenes, mark, n, ground):
    env, state, rows, gpu, kin = scenes(mark, n, ground)
    nb = 19 if mark == "arm" else 13
    assert env.num_bodies == nb == len(env.body_names)
    assert kin.link_pos.shape == (n, nb, 3) and kin.link_quat.shape == (n, nb, 4) and kin.toe_pos.shape == (n, 4, 2, 3)
    assert kin.toe_dist.shape == (n, 4, 2) and kin.toe_in_reach.shape == (n, 4, 2) and kin.base_body.shape == (n, 9)
    assert str(kin.toe_in_reach.dtype) == "torch.uint8" and str(kin.link_pos.dtype) == "torch.float32" and kin.link_pos.device == env.device
    check_rows(gpu, rows, (mark, n, ground))
    # the synthetic columns are the ones the floors were measured over: the episode word arrived, and picks the field
    S, _ = kr.scene_states(mark == "arm", n, ground, kr.scene_keep(n))
    keep = kr.scene_keep(n)
    assert np.array_equal(state[kr.episode_word(mark == "arm"), keep:].view(np.int32), S[-1, keep:].view(np.int32))
    assert np.array_equal(state[0:13, keep:], S[0:13, keep:])
    # the convenience properties
    assert np.array_equal(kin.foot_clearance.cpu().numpy(), gpu["toe_dist"].reshape(n, 4, 2).min(-1))
    assert np.array_equal(kin.foot_in_reach.cpu().numpy(), gpu["toe_in_reach"].reshape(n, 4, 2).any(-1))


def test_cases_cover(scenes):
    """From the reference alone, over the large scenes as the GPU test compares them (their real columns included)."""
    seen = {}
    for mark, n, ground in kr.SCENES:
        if n >= 67:
            count_cases(scenes(mark, n, ground)[2], seen)
    print(seen)
    assert_cases_cover(seen)
    spread = np.concatenate([row["ref"]["toe_dist"] for row in scenes("base", 130, "plane")[2]])
    assert (spread < 0).sum() >= 10 and ((spread > 0) & (spread < kr.BREAKING)).sum() >= 10 and ((spread > kr.BREAKING) & (spread < 0.06)).sum() >= 10


# ---------------------------------------------------------------- b. env ids
@pytest.mark.parametrize("ids", [list(range(66, -1, -1)), [5, 66, 5, 0], [63, 64, 12]], ids=["reversed", "duplicate", "three"])
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids(scenes, ids, ground):
    import torch
    env, state, rows, full, _ = scenes("base", 67, ground)
    part = env.kinematics(env_ids=ids)
    torch.cuda.synchronize()
    part = to_numpy(part)
    for name in full:
        assert part[name].shape[0] == len(ids)
        assert np.array_equal(part[name].view(np.uint8), full[name][ids].view(np.uint8)), name          # bit for bit the full call's rows
    check_rows(part, [rows[g] for g in ids], ("ids", ground, len(ids)))
    assert not np.array_equal(full["link_pos"][0], full["link_pos"][5])


def test_mixed_batch_rows_are_state_indices():
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(48, task="mixed", signal_type="ik", seed=11)
    env.reset()
    col._steps(env, 8, seed=4)
    ids = [0, 7, 19, 30, 47]
    kin = env.kinematics(env_ids=ids)
    torch.cuda.synchronize()
    state = env.state.cpu().numpy()
    rows = []
    for g in ids:
        r = kr.reference(state, g, False, None)
        rows.append(dict(env=g, ref=r, ok=np.ones(8, bool), kind="real", field=None))
    check_rows(to_numpy(kin), rows, "mixed")
    assert len({tuple(np.round(r["ref"]["link_pos"][3], 4)) for r in rows}) == len(ids)      # the rows differ: another env's state would show
    env.close()


# ---------------------------------------------------------------- c. the contract
FIELD_NAMES = list(BOUNDS) + ["toe_in_reach"]


@pytest.mark.parametrize("mark,ground", [("base", "custom"), ("arm", "plane")])
def test_each_field_alone_is_the_full_calls_and_the_state_is_untouched(scenes, mark, ground):
    import torch
    env, state, _, full, _ = scenes(mark, 67, ground)
    for name in FIELD_NAMES:
        one = env.kinematics(fields=[name])
        torch.cuda.synchronize()
        assert one.fields == (name,) and all(getattr(one, other) is None for other in FIELD_NAMES if other != name)
        assert np.array_equal(to_numpy(one)[name].view(np.uint8), full[name].view(np.uint8)), name
    pair = env.kinematics(fields=("toe_dist", "link_quat"))
    torch.cuda.synchronize()
    assert pair.fields == ("link_quat", "toe_dist")
    assert np.array_equal(to_numpy(pair)["toe_dist"].view(np.uint8), full["toe_dist"].view(np.uint8))
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), state.view(np.uint32))


@pytest.mark.parametrize("mark,n", [("base", 67), ("arm", 67), ("base", 5)])
def test_guard_words_and_unaligned_outputs(scenes, mark, n):
    """Every output 16 elements into a larger buffer, then one element further (a float for the float arrays, a byte for toe_in_reach: off
    every wider alignment): the sentinels in front of and behind each survive, and both placements hold the bits of the env's own readout."""
    import torch
    from rex_gym_amd import _lib, kinematics
    env, _, _, full, _ = scenes(mark, n, "plane")
    nb = env.num_bodies
    for offset in (0, 1):
        bufs, ptrs, sizes = {}, {}, {}
        for name, (_, is_u8) in kinematics.FIELDS.items():
            size = int(np.prod(kinematics.field_shape(name, n, nb)))
            dtype, item, fill = (torch.uint8, 1, 0x5A) if is_u8 else (torch.float32, 4, -7.0)
            bufs[name] = torch.full((size + 64,), fill, dtype=dtype, device=env.device)
            assert bufs[name].data_ptr() % 16 == 0
            ptrs[name], sizes[name] = bufs[name].data_ptr() + (16 + offset) * item, size
        assert env._L.rex_kinematics(env._h, None, n, ctypes.byref(_lib.RexKinematicsOut(**ptrs)), env._stream_ptr()) == 0, env._L.rex_last_error()
        torch.cuda.synchronize()
        for name, (_, is_u8) in kinematics.FIELDS.items():
            b, lo, fill = bufs[name].cpu().numpy(), 16 + offset, (0x5A if is_u8 else -7.0)
            assert np.all(b[:lo] == fill) and np.all(b[lo + sizes[name]:] == fill), (name, offset)
            assert np.array_equal(b[lo:lo + sizes[name]].view(np.uint8), full[name].reshape(-1).view(np.uint8)), (name, offset)


def test_out_is_reused_and_checked(scenes):
    import torch
    env, _, _, full, _ = scenes("base", 67, "plane")
    first = env.kinematics(fields=("toe_pos", "toe_dist"))
    tensors = (first.toe_pos, first.toe_dist)
    first.toe_pos.fill_(-1.0)
    for _ in range(2):
        again = env.kinematics(fields=("toe_pos", "toe_dist"), out=first)
        assert again is first and (again.toe_pos, again.toe_dist) == tensors and again.toe_pos is tensors[0]
    torch.cuda.synchronize()
    assert np.array_equal(to_numpy(first)["toe_pos"].view(np.uint8), full["toe_pos"].view(np.uint8))
    with pytest.raises(ValueError):
        env.kinematics(out=first)                                      # other fields
    with pytest.raises(ValueError):
        env.kinematics(fields=("toe_pos", "toe_dist"), env_ids=[1, 2], out=first)      # another row count
    with pytest.raises(ValueError):
        env.kinematics(out=first.toe_pos)                              # not a result
    part = env.kinematics(fields=("toe_pos", "toe_dist"), env_ids=[1, 2])
    assert env.kinematics(fields=("toe_pos", "toe_dist"), env_ids=[2, 1], out=part) is part


def test_bad_arguments_raise_before_any_launch(scenes):
    import torch
    from rex_gym_amd import _lib
    env, state, _, _, _ = scenes("base", 67, "plane")
    for ids in ([67], [-1], []):
        with pytest.raises(IndexError):
            env.kinematics(env_ids=ids)
    for fields in (["toe_force"], ["toe_pos", "nope"], []):
        with pytest.raises(ValueError):
            env.kinematics(fields=fields)
    # the library's own checks, past the Python ones
    L, buf = env._L, torch.zeros(67 * 13 * 4, dtype=torch.float32, device=env.device)
    good = _lib.RexKinematicsOut(link_quat=buf.data_ptr())
    empty = _lib.RexKinematicsOut()
    for sim, n, out, msg in ((env._h, 0, good, b"at least one env"), (env._h, -3, good, b"at least one env"), (env._h, 68, good, b"without env ids"),
                             (env._h, 67, None, b"null pointer"), (env._h, 67, empty, b"every output pointer is null"), (None, 67, good, b"null sim")):
        rc = L.rex_kinematics(sim, None, n, ctypes.byref(out) if out is not None else None, env._stream_ptr())
        assert rc == -1 and msg in L.rex_last_error(), (n, msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), state.view(np.uint32))


# ---------------------------------------------------------------- d. across kernels, and a standing robot
def test_ground_under_the_toes_is_the_height_scans(scenes):
    """toe_pos.z - toe_dist / toe_normal.z is the ground's height under the toe point: env.height_scan(relative=False) at the same (x, y),
    given in each env's yaw frame, one env at a time.  Two kernels, so both bounds apply: the scan's own (1e-5 m plus what the ground
    changes by within 1e-5 m, tests/test_gpu_depth_sensor.py), and this readout's for toe_pos (in z) and toe_dist (over the normal's z)."""
    import math
    import torch
    env, state, rows, gpu, _ = scenes("base", 67, "custom")
    compared = 0
    for g in list(range(0, 12)) + [63, 64, 65, 66]:
        row, f = rows[g], rows[g]["field"]
        pos, dist, nz = gpu["toe_pos"][g].astype(np.float64), gpu["toe_dist"][g].astype(np.float64), gpu["toe_normal"][g][:, 2].astype(np.float64)
        s = state[:, g].astype(np.float64)
        x, y, z, w = s[3:7]
        r00, r10 = 1 - 2 * (y * y + z * z), 2 * (x * y + z * w)
        yaw = math.atan2(r10, r00)
        c, sn = math.cos(yaw), math.sin(yaw)
        d = pos[:, 0:2] - s[0:2]
        pts = np.stack([c * d[:, 0] + sn * d[:, 1], -sn * d[:, 0] + c * d[:, 1]], 1).astype(np.float32)
        if math.hypot(r00, r10) < 1e-3:
            continue                                                       # the yaw frame of a base pointing straight up is not defined
        scan = env.height_scan(pts, env_ids=[g], relative=False)
        torch.cuda.synchronize()
        scan = scan.cpu().numpy()[0]
        for p in range(8):
            if not row["ok"][p] or not col.field_inside(f, pos[p, 0], pos[p, 1]):
                continue
            # the scan's point is the toe's (x, y) through float32 yaw-frame coordinates: within 1e-5 m of it
            want = kr.ground_query(f, pos[p, 0], pos[p, 1])[0]
            vary = max(abs(kr.ground_query(f, pos[p, 0] + dx, pos[p, 1] + dy)[0] - want) for dx in (-1e-5, 0, 1e-5) for dy in (-1e-5, 0, 1e-5))
            bound = 1e-5 + vary + BOUNDS["toe_pos"] + BOUNDS["toe_dist"] / nz[p]
            assert abs((pos[p, 2] - dist[p] / nz[p]) - scan[p]) <= bound, (g, p, float(pos[p, 2] - dist[p] / nz[p]), float(scan[p]), bound)
            compared += 1
    assert compared >= 40, compared


@pytest.mark.parametrize("mark", ["base", "arm"])
def test_after_reset_on_the_plane_every_foot_is_in_reach(mark):
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(37, task="walk", signal_type="ik", mark=mark, seed=9)
    env.reset()
    kin = env.kinematics(fields=("toe_in_reach", "toe_dist", "toe_normal"))
    torch.cuda.synchronize()
    assert bool(kin.foot_in_reach.all()), kin.foot_clearance.min(0)
    assert kin.foot_in_reach.shape == (37, 4) and kin.foot_clearance.shape == (37, 4)
    assert bool((kin.toe_normal[..., 2] == 1).all())
    with pytest.raises(AttributeError):
        env.kinematics(fields=("link_pos",)).foot_clearance
    env.close()
