"""Stores the visual mesh files the reference's rex.urdf / rex_arm.urdf draw under tests/golden/meshes/ for the mesh-renderer
tests (tests/test_visual_meshes.py, tests/test_gpu_render_mesh.py): each file xz-compressed (preset 9e), laid out as
assets/urdf/<path as the URDF names it>.xz, so that a test unpacks them into a temporary data path the way the reference's
rex_gym.util.pybullet_data.getDataPath() lays them out; plus manifest.json with each file's triangle count and the sha256 of
its raw bytes.  Files the URDFs name but the reference does not ship (the arm's section_1/3/4.obj) are left out, as there.

Run where the reference tree is present:  python tests/golden/make_mesh_golden.py <reference tree>
"""
import hashlib
import json
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "meshes")


def main(reference):
    sys.path.insert(0, ROOT)
    from rex_gym_amd import meshes
    src = os.path.join(reference, "rex_gym", "util", "pybullet_data", "assets", "urdf")
    manifest = {}
    for rel in sorted(set(meshes.visual_table().mesh)):
        path = os.path.join(src, rel)
        if not os.path.exists(path):
            continue
        with open(path, "rb") as f:
            raw = f.read()
        dst = os.path.join(OUT, "assets", "urdf", rel + ".xz")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "wb") as f:
            f.write(lzma.compress(raw, preset=9 | lzma.PRESET_EXTREME))
        manifest[rel] = {"triangles": int(len(meshes.read_mesh(path))), "sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw)}
        print(rel, manifest[rel]["triangles"], os.path.getsize(dst))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
