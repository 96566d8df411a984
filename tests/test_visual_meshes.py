"""The visual-mesh side of the renderer on the host: the STL / OBJ readers, the BVH builder's invariants, the generated table
csrc/rex_visual_gen.h against poses worked by hand from the reference's URDFs (as tests/test_model_table.py does), the
committed fixtures (tests/golden/meshes) and the mesh kernel's resource usage.  No GPU."""
import hashlib
import json
import lzma
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from rex_gym_amd import meshes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "meshes")
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    MANIFEST = json.load(_f)


def _binary_stl(tri, header=b""):
    out = header.ljust(80, b"\0")[:80] + struct.pack("<I", len(tri))
    for t in np.asarray(tri, dtype=np.float32):
        out += struct.pack("<12fH", 0, 0, 1, *t.ravel(), 0)
    return out


def _ascii_stl(tri):
    s = "solid test\n"
    for t in tri:
        s += "  facet normal 0 0 1\n    outer loop\n"
        for v in t:
            s += "      vertex %.9g %.9g %.9g\n" % tuple(v)
        s += "    endloop\n  endfacet\n"
    return (s + "endsolid test\n").encode()


TRI = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.5, -1.25, 2], [3, 4, 5], [-6, 7.5, -8]]], dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------- readers
def test_stl_binary_ascii_and_solid_header_agree():
    a = meshes.read_stl(_binary_stl(TRI))
    b = meshes.read_stl(_ascii_stl(TRI))
    c = meshes.read_stl(_binary_stl(TRI, header=b"solid but binary"))
    assert a.shape == (2, 3, 3)
    assert np.array_equal(a, TRI) and np.array_equal(b, TRI) and np.array_equal(c, TRI)


def test_truncated_stl_raises(tmp_path):
    data = _binary_stl(TRI)
    for bad in (data[:-1], data[:90], data[:50], _binary_stl(TRI, header=b"solid x")[:-7], _ascii_stl(TRI)[:-30]):
        with pytest.raises(ValueError):
            meshes.read_stl(bad)
    p = tmp_path / "t.stl"
    p.write_bytes(data[:-3])
    with pytest.raises(ValueError, match="t.stl"):
        meshes.read_mesh(str(p))


def test_obj_face_forms_negative_indices_and_quads():
    text = "\n".join(["# test", "v 0 0 0", "v 1 0 0", "v 1 1 0", "v 0 1 0", "vn 0 0 1", "vt 0 0",
                      "f 1 2 3", "f 1/1 2/1 3/1", "f 1//1 2//1 3//1", "f 1/1/1 2/1/1 3/1/1",
                      "f -4 -3 -2", "f 1 2 3 4", ""])
    t = meshes.read_obj(text)
    tri = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], dtype=np.float64)
    assert t.shape == (7, 3, 3)
    for k in range(6):
        assert np.array_equal(t[k], tri)
    assert np.array_equal(t[6], [[0, 0, 0], [1, 1, 0], [0, 1, 0]])   # the quad's second fan triangle
    with pytest.raises(ValueError):
        meshes.read_obj("v 0 0 0\nf 1 2 3\n")


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    out = tmp_path_factory.mktemp("pybullet_data")
    for rel in MANIFEST:
        dst = out / "assets" / "urdf" / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        with lzma.open(os.path.join(GOLDEN, "assets", "urdf", rel + ".xz")) as f, open(dst, "wb") as g:
            shutil.copyfileobj(f, g)
    return str(out)


def test_fixtures_match_the_manifest(fixtures):
    assert len(MANIFEST) == 15
    assert MANIFEST["stl/mainbody.stl"]["triangles"] == 22968
    assert MANIFEST["stl/foot.stl"]["triangles"] == 21496
    assert MANIFEST["meshes/section_2.obj"]["triangles"] == 44284
    for rel, m in MANIFEST.items():
        path = os.path.join(fixtures, "assets", "urdf", rel)
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == m["sha256"], rel
        assert len(meshes.read_mesh(path)) == m["triangles"], rel
        assert os.path.getsize(os.path.join(GOLDEN, "assets", "urdf", rel + ".xz")) < 1 << 20


# -------------------------------------------------------------------------------------------------------------- BVH
def check_bvh(tri, b):
    n = len(tri)
    if n == 0:
        assert len(b.nodes) == 0 and len(b.tris) == 0 and b.depth == 0
        return
    ni = b.nodes.view(np.int32)
    seen = np.zeros(n, dtype=int)
    depth = {0: 1}
    parent_box = {0: (b.lo, b.hi)}
    assert np.all(ni[:, 14:] == 0)
    for i in range(len(b.nodes)):
        plo, phi = parent_box[i]
        ranges = set()
        for c in range(2):
            lo, hi = b.nodes[i, 6 * c:6 * c + 3], b.nodes[i, 6 * c + 3:6 * c + 6]
            assert np.all(lo >= plo) and np.all(hi <= phi), i    # child boxes inside their parent
            code = int(ni[i, 12 + c])
            if code >= 0:
                assert code > i
                depth[code] = depth[i] + 1
                parent_box[code] = (lo, hi)
            else:
                v = ~code
                s, k = v >> 3, (v & 7) + 1
                assert 1 <= k <= meshes.LEAF
                if (s, k) in ranges:     # (a mesh that fits one leaf: both children are that leaf)
                    continue
                ranges.add((s, k))
                seen[s:s + k] += 1
                t = b.tris[s:s + k].astype(np.float64)
                v0, v1, v2 = t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]
                for v_ in (v0, v1, v2):
                    assert np.all(v_ >= lo - 1e-7) and np.all(v_ <= hi + 1e-7)
    assert np.all(seen == 1)           # every triangle in exactly one leaf
    assert max(depth.values()) == b.depth <= meshes.MAX_DEPTH
    assert np.array_equal(np.sort(b.order), np.arange(n))
    src = np.asarray(tri, dtype=np.float64)[b.order]
    assert np.allclose(b.tris[:, :3], src[:, 0], atol=1e-6)


DEGENERATE = {
    "identical": np.tile(TRI[1], (10000, 1, 1)),
    "zero_area": np.stack([np.random.RandomState(0).rand(5000, 3)] * 3, axis=1),
    "one": TRI[:1],
    "empty": np.zeros((0, 3, 3)),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_bvh_invariants_on_degenerate_input(name):
    tri = DEGENERATE[name]
    b = meshes.build_bvh(tri)
    check_bvh(tri, b)
    if len(tri) > meshes.LEAF:     # median splits: the depth depends on the count only
        assert b.depth == int(np.ceil(np.log2(len(tri) / meshes.LEAF)))
        with pytest.raises(ValueError, match="deeper"):   # the builder fails loudly rather than emit a deeper tree
            meshes.build_bvh(tri, max_depth=b.depth - 1)


@pytest.mark.parametrize("rel", sorted(MANIFEST))
def test_bvh_invariants_and_determinism_on_fixtures(rel, fixtures):
    tri = meshes.read_mesh(os.path.join(fixtures, "assets", "urdf", rel))
    a, b = meshes.build_bvh(tri), meshes.build_bvh(tri)
    check_bvh(tri, a)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.tris.tobytes() == b.tris.tobytes()


# ------------------------------------------------------------------------------------------------------------ table
def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def test_table_counts_and_hand_worked_entries():
    t = meshes.visual_table()
    assert t.n_base == 23 and t.n_arm == 29 and t.count("base") == 23 and t.count("arm") == 29
    assert t.mesh[:3] == ["stl/mainbody.stl", "stl/frontpart.stl", "stl/backpart.stl"] and set(t.body[:3]) == {0}
    assert np.allclose(t.pos[0], [-0.045, -0.060, -0.015]) and np.allclose(t.rot[0], np.eye(3))   # rex.urdf:16-22
    k = t.links.index("front_left_toe_link")
    # the toe: fixed joint front_left_toe (rex.urdf: origin xyz 0 0 -0.115 in the foot link) then the visual origin
    assert t.body[k] == 3 and t.mesh[k] == "stl/foot.stl" and t.scale[k] == 0.001
    assert np.allclose(t.pos[k], np.array([0, 0, -0.115]) + np.array([0, -0.01, 0]))
    assert np.allclose(t.rot[k], _rpy(0, -0.4001, 0))
    assert np.allclose(t.rgb[k], [0.6, 0.6, 0.6])
    assert t.fb_kind[k] == meshes.KIND_CYL
    k = t.links.index("rear_right_leg_link_cover")       # a leg cover: merged into the leg body, no collision shape
    assert t.body[k] == 11 and t.mesh[k] == "stl/rarm_cover.stl" and t.fb_kind[k] == -1
    assert np.allclose(t.pos[k], [-0.125, -0.15, -0.02]) and np.allclose(t.rgb[k], [0.92, 0.83, 0.0])
    k = t.links.index("front_left_foot_link")
    assert t.body[k] == 3 and np.allclose(t.rgb[k], [0.1, 0.1, 0.1]) and t.fb_kind[k] == meshes.KIND_BOX
    k = t.links.index("arm_section_2")
    assert t.body[k] == 15 and t.scale[k] == 1.0 and t.mesh[k] == "meshes/section_2.obj"
    assert np.allclose(t.rot[k], _rpy(0, 1.5707963267949, 0))


def test_arm_fixtures_report_missing_sections(fixtures):
    with pytest.warns(UserWarning, match="section_1.obj"):
        vm = meshes.load(fixtures, "arm")
    assert vm.missing == ["meshes/section_1.obj", "meshes/section_3.obj", "meshes/section_4.obj"]
    assert len(vm.root) == 29 and vm.depth <= meshes.MAX_DEPTH and (vm.root >= 0).all()   # the fallbacks are cylinders
    base = meshes.load(fixtures, "base")
    assert base.missing == [] and len(base.root) == 23 and len(base.tris) == 150178 and base.distinct == 12
    assert base.seconds < 30


def test_missing_data_path_names_the_argument(tmp_path, monkeypatch):
    monkeypatch.setattr(meshes, "default_data_path", lambda: None)
    with pytest.raises(ValueError, match="data_path"):
        meshes.load(None)
    with pytest.raises(ValueError, match="data_path"):
        meshes.load(str(tmp_path))


def test_generated_headers_regenerate_byte_identical(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compile_model
    if not (os.path.exists(compile_model.DEFAULT_URDF) and os.path.exists(compile_model.DEFAULT_ARM_URDF)):
        pytest.skip("the reference URDFs are not on this machine")
    csrc = os.path.join(ROOT, "rex_gym_amd", "csrc")
    names = ["rex_model_gen.h", "rex_arm_model_gen.h", "rex_render_gen.h", "rex_visual_gen.h"]
    before = {n: open(os.path.join(csrc, n), "rb").read() for n in names}
    work = tmp_path / "csrc"
    work.mkdir()
    out = str(work / "rex_model_gen.h")
    env = dict(os.environ)
    code = ("import sys, os; sys.path.insert(0, %r); import compile_model as c; d = %r; "
            "c.DEFAULT_ARM_OUT = os.path.join(d, 'rex_arm_model_gen.h'); c.DEFAULT_RENDER_OUT = os.path.join(d, 'rex_render_gen.h'); "
            "c.DEFAULT_VISUAL_OUT = os.path.join(d, 'rex_visual_gen.h'); sys.argv = ['x', '--out', %r]; c.main(); "
            "c.emit_arm(c.load_bodies(c.DEFAULT_URDF, c.BASE_MOTOR_NAMES)[0]); c.emit_render(); c.emit_visual()"
            % (os.path.join(ROOT, "tools"), str(work), out))
    subprocess.check_call([sys.executable, "-c", code], env=env, stdout=subprocess.DEVNULL)
    for n in names:
        assert open(work / n, "rb").read() == before[n], n


# -------------------------------------------------------------------------------------------------------- resources
def test_mesh_kernel_uses_no_scratch(tmp_path):
    from rex_gym_amd import build
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc] + build.COMPILE_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-I", build.CSRC, "-c",
                        os.path.join(build.CSRC, "rex_render_mesh.hip"), "-o", str(tmp_path / "m.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif "ScratchSize" in line and name and "rex_render_mesh_kernel" in name:
            seen[name] = int(line.rsplit(":", 1)[1].split()[0])
    assert len(seen) == 2 and all(v == 0 for v in seen.values()), seen
    assert any("ILb0E" in k for k in seen) and any("ILb1E" in k for k in seen)
