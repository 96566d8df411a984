"""The mesh renderer (rex_render_visual, csrc/rex_render_mesh.hip; RexBatchEnv.render(geometry="visual")) on the GPU.

The reference here is a brute-force caster with no BVH: every instance's triangles as read from the committed fixtures
(tests/golden/meshes, unpacked into a temporary data path), placed by forward kinematics restated in tests/test_gpu_render.py
and the table parsed from rex_visual_gen.h, intersected with every ray in float64 with torch on the device.  The shading
constants are the ones csrc/rex_render.h documents."""
import ctypes
import json
import lzma
import os
import shutil

import numpy as np
import pytest

import test_gpu_render as col
from test_gpu_render import CAMERAS, _interior, _steps, camera_rays, fk, full_camera, ground_shade

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "meshes")


@pytest.fixture(scope="module")
def data_path(tmp_path_factory):
    """The fixtures unpacked as rex_gym.util.pybullet_data.getDataPath() lays them out."""
    out = tmp_path_factory.mktemp("pybullet_data")
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)
    for rel in manifest:
        dst = out / "assets" / "urdf" / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        with lzma.open(os.path.join(GOLDEN, "assets", "urdf", rel + ".xz")) as f, open(dst, "wb") as g:
            shutil.copyfileobj(f, g)
    return str(out)


def brute_cast(state, env, arm, W, H, data_path, field=None, camera=None, info=None):
    """(rgb uint8 [H, W, 3], depth float64 [H, W], segment int [H, W]) of env `env`, every triangle against every ray; the
    ground, the far plane and the shading are the collision reference's (ground_shade, whose facts `info` receives)."""
    import torch
    from rex_gym_amd import meshes
    tab = meshes.visual_table()
    cam = full_camera(camera)
    near, far = cam["near_plane"], cam["far_plane"]
    Rs, Os = fk(state, env, arm)
    eye, d = camera_rays(Os[0], W, H, cam)
    dev = torch.device("cuda")
    D = torch.as_tensor(d, dtype=torch.float64, device=dev)
    E = torch.as_tensor(eye, dtype=torch.float64, device=dev)
    P = len(d)
    best = torch.full((P,), float("inf"), dtype=torch.float64, device=dev)
    nrm = torch.zeros((P, 3), dtype=torch.float64, device=dev)
    seg = torch.full((P,), -1, dtype=torch.int64, device=dev)
    alb = torch.zeros((P, 3), dtype=torch.float64, device=dev)
    urdf = os.path.join(data_path, "assets", "urdf")
    for k in range(tab.count("arm" if arm else "base")):
        path = os.path.join(urdf, tab.mesh[k])
        if os.path.exists(path):
            tri = meshes.read_mesh(path) * tab.scale[k]
        elif tab.fb_kind[k] >= 0:   # the documented fallback: the link's collision primitive, in the body frame
            tri = (meshes.tessellate(tab.fb_kind[k], tab.fb_ext[k]) @ tab.fb_rot[k].T + tab.fb_pos[k] - tab.pos[k]) @ tab.rot[k]
        else:
            continue
        b = tab.body[k]
        R, t = Rs[b] @ tab.rot[k], Os[b] + Rs[b] @ tab.pos[k]
        V = torch.as_tensor(tri @ R.T + t, dtype=torch.float64, device=dev)
        v0, e1, e2 = V[:, 0], V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        for c in range(0, len(V), 1024):
            a0, a1, a2 = v0[c:c + 1024], e1[c:c + 1024], e2[c:c + 1024]
            pv = torch.cross(D[:, None, :].expand(-1, len(a0), -1), a2[None].expand(P, -1, -1), dim=-1)
            det = (a1[None] * pv).sum(-1)
            inv = 1.0 / det
            s = E - a0
            u = (s[None] * pv).sum(-1) * inv
            q = torch.cross(s, a1, dim=-1)
            v = (D @ q.T) * inv
            tt = (a2 * q).sum(-1)[None] * inv
            ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (tt >= near)
            tt = torch.where(ok, tt, torch.full_like(tt, float("inf")))
            tmin, arg = tt.min(1)
            better = tmin < best
            if bool(better.any()):
                n = torch.cross(a1[arg], a2[arg], dim=-1)
                best = torch.where(better, tmin, best)
                nrm = torch.where(better[:, None], n, nrm)
                seg = torch.where(better, torch.full_like(seg, 1 + int(b)), seg)
                alb = torch.where(better[:, None], torch.as_tensor(tab.rgb[k], device=dev), alb)
    best, nrm, seg, alb = best.cpu().numpy(), nrm.cpu().numpy(), seg.cpu().numpy(), alb.cpu().numpy()
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    rgb, best, ground, hit, g = ground_shade(eye, d, best, nrm, alb, field, near, far)
    seg = np.where(ground, 0, seg)
    if info is not None:
        info.update({k: v.reshape(H, W) for k, v in g.items()})
    return (rgb.reshape(H, W, 3), np.where(hit, best, far).reshape(H, W), np.where(hit, seg, -1).reshape(H, W))


def compare(env, ids, W, H, data_path, field_of=None, camera=None):
    import torch
    rgb, extra = env.render(env_ids=ids, width=W, height=H, depth=True, segmentation=True, geometry="visual", camera=camera)
    torch.cuda.synchronize()
    rgb, dep, seg = rgb.cpu().numpy(), extra["depth"].cpu().numpy(), extra["segmentation"].cpu().numpy()
    state = env.state.cpu().numpy()
    skies = []          # per row: the sky pixels whose depth was held to the far plane
    for k, e in enumerate(ids):
        info = {}
        nrgb, ndep, nseg = brute_cast(state, e, env.mark == "arm", W, H, data_path, field_of(e) if field_of else None, camera, info)
        inner = _interior(nseg)
        if field_of:    # on a heightfield: not the pixels no float32 caster can be held to (ground_shade: grazing facets, nearer
            inner &= ~info["amb"]                         # ties); without one the mask is empty
        assert inner.mean() > 0.5
        assert (seg[k][inner] == nseg[inner]).mean() >= 0.995, (e, W, H, int((seg[k][inner] != nseg[inner]).sum()))
        both = inner & (seg[k] == nseg) & (nseg >= 0)
        err = np.abs(dep[k].astype(np.float64) - ndep)
        assert np.all(err[both] <= 1e-4), (e, W, H, float(err[both].max()))
        sky = inner & (seg[k] < 0) & (nseg < 0)          # nothing within the far plane: the depth is the far plane
        assert np.all(dep[k][sky] == np.float32(full_camera(camera)["far_plane"])), (e, W, H)
        drgb = np.abs(rgb[k].astype(int) - nrgb.astype(int)).max(-1)
        flat = inner & ~info["amb_rgb"]                  # (a facet edge switches the normal, not the depth)
        assert (drgb[flat] <= 1).mean() >= 0.99, (e, W, H, float((drgb[flat] <= 1).mean()))
        assert (nseg > 0).sum() >= 10 and (seg[k] > 0).sum() >= 10   # the robot is in the picture
        skies.append(int(sky.sum()))
    return skies


# ---------------------------------------------------------------- a. against the brute-force caster
@pytest.mark.parametrize("W,H", [(64, 48), (160, 120)])
def test_walk_ik_batch_after_random_steps(W, H, data_path):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(8, task="walk", signal_type="ik", seed=3)
    vm = env.load_visual_meshes(data_path)
    assert vm.missing == [] and vm.depth <= 32
    env.reset()
    _steps(env, 30)
    compare(env, [0, 5] if W == 64 else [3], W, H, data_path)
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (160, 120)])
def test_crouched_standup(W, H, data_path):
    from rex_gym_amd.envs.gym.standup_env import RexStandupEnv
    env = RexStandupEnv()
    env.load_visual_meshes(data_path)
    env.reset()
    compare(env._batch, [0], W, H, data_path)
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (160, 120)])
def test_mark_arm_with_fallback_cylinders(W, H, data_path):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(4, task="walk", signal_type="ik", mark="arm", seed=1)
    with pytest.warns(UserWarning, match="section_1.obj"):
        vm = env.load_visual_meshes(data_path)
    assert vm.missing == ["meshes/section_1.obj", "meshes/section_3.obj", "meshes/section_4.obj"]
    env.reset()
    _steps(env, 10)
    compare(env, [2] if W == 160 else [0, 2], W, H, data_path)
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (160, 120)])
def test_mixed_task_batch_renders_state_indices(W, H, data_path):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(48, task="mixed", signal_type="ik", seed=11)
    env.load_visual_meshes(data_path)
    env.reset()
    _steps(env, 12, seed=4)
    compare(env, [7, 30] if W == 64 else [19], W, H, data_path)
    env.close()


# ---------------------------------------------------------------- b. box meshes reproduce the collision picture
def _box_meshes(tmp_path):
    """Synthetic mesh files: each holds the collision boxes of the links that use it, in that file's mesh frame and units
    (mm for the STLs); toe cylinders finely tessellated; leg covers and arm files empty.  -> data path."""
    import struct
    from rex_gym_amd import meshes
    tab = meshes.visual_table()
    urdf = tmp_path / "box_data" / "assets" / "urdf"
    tris = {}
    for k in range(tab.n_base):
        if tab.mesh[k] in tris:
            continue
        if tab.fb_kind[k] < 0:
            tri = np.zeros((0, 3, 3))
        else:
            seg = 720 if tab.fb_kind[k] == meshes.KIND_CYL else 48
            body = meshes.tessellate(tab.fb_kind[k], tab.fb_ext[k], segments=seg) @ tab.fb_rot[k].T + tab.fb_pos[k]
            tri = (body - tab.pos[k]) @ tab.rot[k] / tab.scale[k]
        tris[tab.mesh[k]] = tri
    for rel, tri in tris.items():
        p = urdf / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        with open(p, "wb") as f:
            f.write(b"\0" * 80 + struct.pack("<I", len(tri)))
            for t in tri.astype(np.float32):
                f.write(struct.pack("<12fH", 0, 0, 0, *t.ravel(), 0))
    return str(tmp_path / "box_data")


def test_box_meshes_reproduce_the_collision_picture(tmp_path):
    import torch
    from rex_gym_amd import RexBatchEnv
    path = _box_meshes(tmp_path)
    env = RexBatchEnv(6, task="walk", signal_type="ik", seed=5)
    env.load_visual_meshes(path)
    env.reset()
    _steps(env, 20)
    W, H = 160, 120
    c_rgb, c = env.render(width=W, height=H, depth=True, segmentation=True, geometry="collision")
    v_rgb, v = env.render(width=W, height=H, depth=True, segmentation=True, geometry="visual")
    torch.cuda.synchronize()
    cs, vs = c["segmentation"].cpu().numpy(), v["segmentation"].cpu().numpy()
    cd, vd = c["depth"].cpu().numpy(), v["depth"].cpu().numpy()
    cr, vr = c_rgb.cpu().numpy().astype(int), v_rgb.cpu().numpy().astype(int)
    from rex_gym_amd import meshes
    boxes = {1 + b for b in range(13)}
    checked = 0
    for k in range(env.num_envs):
        inner = _interior(cs[k]) & np.isin(cs[k], list(boxes))
        assert np.array_equal(vs[k][inner], cs[k][inner]), (k, int((vs[k][inner] != cs[k][inner]).sum()))
        assert np.abs(vd[k] - cd[k])[inner].max(initial=0) <= 1e-5
        # colour on pixels inside one flat face as well: along an edge between two faces the face a ray takes is a coin toss
        face = inner & _interior(cr[k][..., 0] * 65536 + cr[k][..., 1] * 256 + cr[k][..., 2])
        assert np.abs(vr[k] - cr[k]).max(-1)[face].max(initial=0) <= 1
        checked += int(inner.sum())
    assert checked > 0.01 * env.num_envs * W * H
    assert meshes.visual_table().n_base == 23
    env.close()


# ---------------------------------------------------------------- c. ground and sky agree with the collision render
@pytest.mark.parametrize("terrain", ["plane", "random"])
def test_ground_and_sky_match_collision_render(terrain, data_path):
    import torch
    from rex_gym_amd import RexBatchEnv
    kw = dict(terrain_type="random", terrain_pool=8) if terrain == "random" else {}
    env = RexBatchEnv(4, task="walk", signal_type="ik", seed=2, **kw)
    env.load_visual_meshes(data_path)
    env.reset()
    _steps(env, 5)
    W, H = 96, 72
    c_rgb, c = env.render(width=W, height=H, depth=True, segmentation=True, geometry="collision")
    v_rgb, v = env.render(width=W, height=H, depth=True, segmentation=True, geometry="visual")
    torch.cuda.synchronize()
    cs, vs = c["segmentation"].cpu().numpy(), v["segmentation"].cpu().numpy()
    both = (cs <= 0) & (vs <= 0)
    assert both.mean() > 0.5
    assert np.array_equal(cs[both], vs[both])
    cd, vd = c["depth"].cpu().numpy()[both].astype(np.float64), v["depth"].cpu().numpy()[both].astype(np.float64)
    assert np.all(np.abs(cd - vd) <= 1e-6 * np.abs(cd))
    assert np.abs(c_rgb.cpu().numpy().astype(int) - v_rgb.cpu().numpy().astype(int)).max(-1)[both].max() <= 1
    env.close()


# ---------------------------------------------------------------- d. read-only, order-independent; the default untouched
def test_visual_render_is_read_only_and_order_independent(data_path):
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(8, task="walk", signal_type="ik", seed=9, check_actions=False)
    env.load_visual_meshes(data_path)
    env.reset()
    _steps(env, 6)
    before = env.state.clone()
    full, fx = env.render(width=96, height=72, depth=True, segmentation=True)       # geometry None -> visual once loaded
    part, px = env.render(env_ids=[5, 2, 5], width=96, height=72, depth=True, segmentation=True, geometry="visual")
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), before.view(torch.int32))
    for k, e in enumerate([5, 2, 5]):
        assert torch.equal(part[k], full[e])
        assert torch.equal(px["depth"][k], fx["depth"][e]) and torch.equal(px["segmentation"][k], fx["segmentation"][e])
    odd = env.render(env_ids=[3], width=97, height=73, geometry="visual")     # the element-wise store path
    assert odd.shape == (1, 73, 97, 3)
    env.close()


def test_collision_render_unchanged_with_meshes_loaded(data_path):
    import torch
    from rex_gym_amd import RexBatchEnv
    a = RexBatchEnv(4, task="walk", signal_type="ik", seed=4, check_actions=False)
    b = RexBatchEnv(4, task="walk", signal_type="ik", seed=4, check_actions=False)
    a.load_visual_meshes(data_path)
    for e in (a, b):
        e.reset()
        _steps(e, 8, seed=1)
    ra, xa = a.render(width=80, height=60, depth=True, segmentation=True, geometry="collision")
    rb, xb = b.render(width=80, height=60, depth=True, segmentation=True)
    torch.cuda.synchronize()
    assert torch.equal(ra, rb) and torch.equal(xa["depth"].view(torch.int32), xb["depth"].view(torch.int32))
    assert torch.equal(xa["segmentation"], xb["segmentation"])
    a.close()
    b.close()


# ---------------------------------------------------------------- e. errors before any launch
def test_errors_before_any_launch(tmp_path, monkeypatch, data_path):
    import torch
    from rex_gym_amd import RexBatchEnv, _lib, meshes
    env = RexBatchEnv(2, task="walk", signal_type="ik")
    env.reset()
    with pytest.raises(ValueError, match="geometry"):
        env.render(width=8, height=8, geometry="mesh")
    monkeypatch.setattr(meshes, "default_data_path", lambda: None)
    with pytest.raises(ValueError, match="data_path"):
        env.render(width=8, height=8, geometry="visual")
    with pytest.raises(ValueError, match="data_path"):
        env.load_visual_meshes(str(tmp_path / "nowhere"))
    L, p = env._L, env._stream_ptr()
    cam = _lib.RexCamera()
    L.rex_default_camera(ctypes.byref(cam))
    ids = torch.zeros(1, dtype=torch.int32, device=env.device)
    out = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=env.device)
    assert L.rex_render_visual(env._h, ctypes.byref(cam), ids.data_ptr(), 1, 4, 4, out.data_ptr(), None, None, p) == -1
    assert b"no visual meshes" in L.rex_last_error()
    vm = meshes.load(data_path, "base")
    box = np.ascontiguousarray(np.concatenate([vm.lo, vm.hi], axis=1), dtype=np.float32)

    def setv(nodes, tris, root, n_inst=None):
        return L.rex_render_set_visuals(env._h, nodes.ctypes.data, len(nodes), tris.ctypes.data, len(tris), root.ctypes.data,
                                        box.ctypes.data, len(root) if n_inst is None else n_inst, p)
    assert setv(vm.nodes, vm.tris, vm.root, n_inst=22) == -1
    bad = vm.nodes.copy()
    bad.view(np.int32)[0, 12] = len(bad)            # a child out of range
    assert setv(bad, vm.tris, vm.root) == -1
    bad = vm.nodes.copy()
    bad.view(np.int32)[1, 13] = 0                  # a backward child (a cycle)
    assert setv(bad, vm.tris, vm.root) == -1
    assert setv(vm.nodes, vm.tris[:-10], vm.root) == -1   # leaves past the triangles
    root = vm.root.copy()
    root[3] = 1                                    # not a root
    assert setv(vm.nodes, vm.tris, root) == -1
    # a chain 33 levels deep
    chain = np.zeros((33, 16), np.float32)
    ci = chain.view(np.int32)
    for i in range(33):
        ci[i, 12] = i + 1 if i < 32 else ~0
        ci[i, 13] = ~0
    tri = np.zeros((1, 9), np.float32)
    r = np.full(23, -1, np.int32)
    r[0] = 0
    assert setv(chain, tri, r) == -1 and b"deeper" in L.rex_last_error()
    assert L.rex_render_visual(env._h, ctypes.byref(cam), ids.data_ptr(), 1, 4, 4, out.data_ptr(), None, None, p) == -1
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
    env.close()


# ---------------------------------------------------------------- f. video
def test_policy_player_video_meshes(tmp_path, data_path):
    Image = pytest.importorskip("PIL.Image")
    from rex_gym_amd.agents import policy_player
    src = os.path.join(ROOT, "tests", "golden", "policies", "walk", "ik")
    dst = tmp_path / "walk_ik"
    dst.mkdir()
    for name in os.listdir(src):
        if name.endswith(".xz"):
            with lzma.open(os.path.join(src, name)) as f, open(dst / name[:-3], "wb") as g:
                shutil.copyfileobj(f, g)
        else:
            shutil.copyfile(os.path.join(src, name), dst / name)
    gif = str(tmp_path / "walk.gif")
    policy_player.main(["--env", "walk", "--signal-type", "ik", "--checkpoint", str(dst / "model.ckpt-2000000"), "--num-envs", "2",
                        "--max-steps", "20", "--video", gif, "--video-meshes", data_path])
    im = Image.open(gif)
    assert im.n_frames == 20 and im.size == (480, 360)


# ---------------------------------------------------------------- g. cameras other than the default (tests/test_gpu_render.py, h)
@pytest.mark.parametrize("name,W,H", [("quadrant", 64, 48), ("near_far", 64, 48), ("down", 64, 48), ("default", 63, 47)])
def test_cameras_on_the_plane(name, W, H, plane_meshes, data_path):
    """the traversal order of the BVH, the instance box rejection and the two-sided triangle test under other ray directions"""
    skies = compare(plane_meshes, [0, 3], W, H, data_path, camera=CAMERAS[name])
    assert name != "near_far" or min(skies) >= 0.2 * W * H      # the far plane's depth is compared


@pytest.fixture(scope="module")
def plane_meshes(data_path):
    env = col.plane_batch("base")
    env.load_visual_meshes(data_path)
    yield env
    env.close()


# ---------------------------------------------------------------- h. the caller-supplied heightfield pool (test_gpu_render.py, i)
@pytest.fixture(scope="module")
def field_meshes(data_path):
    env, _, field_of = col.custom_field_scene()
    env.load_visual_meshes(data_path)
    yield env, field_of
    env.close()


@pytest.mark.parametrize("name", ["default", "quadrant"])
def test_custom_heightfield(name, field_meshes, data_path):
    """the mesh kernel's ground against the reference's (the same rays at the same fields as the collision suite casts)"""
    env, field_of = field_meshes
    compare(env, [0, 1, 2, 3], 64, 48, data_path, field_of=field_of, camera=CAMERAS[name])


# ---------------------------------------------------------------- i. the store paths (test_gpu_render.py, j)
def test_vector_stores_equal_scalar_stores(plane_meshes):
    col.check_vector_stores_equal_scalar_stores(plane_meshes, "rex_render_visual")


@pytest.mark.parametrize("W,H", [(61, 47), (64, 48)])
def test_nothing_outside_the_images(plane_meshes, W, H):
    col.check_nothing_outside_the_images(plane_meshes, "rex_render_visual", W, H, True, True)
