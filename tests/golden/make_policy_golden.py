"""Stores the tensor bundles of the policy checkpoints the reference ships (rex_gym/policies/) under tests/golden/policies/ for
tests/test_agents_policy_player.py: every .index as it is, every .data shard xz-compressed (the test unpacks them into a
temporary directory).  Data only: no .meta graph, no config.yaml.

walk / ik and turn / ik are stored MASKED: their PPO episode memory (`memory/*`, 2.2 MB and 1.1 MB of rollout buffer that no
test reads) is zeroed in place, which keeps each file inside the repository's size limit.  Every other tensor keeps its bytes
at its offset, and the .index is TensorFlow's own, so the network and observ filter still pass their stored crc32c; the
zeroed tensors fail theirs (the reader refuses them), and the byte-for-byte rewrite test runs on the unmasked checkpoints only.

Run where the reference tree is present:  python tests/golden/make_policy_golden.py <reference tree>
"""
import lzma
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "policies")
# the five complete checkpoints, and walk / ol whose .data shard the reference does not ship (its .index only)
PREFIXES = ["walk/ik/model.ckpt-2000000", "turn/ik/model.ckpt-2000000", "turn/ol/model.ckpt-2000000", "poses/model.ckpt-2000000",
            "standup/ol/model.ckpt-2000000", "walk/ol/model.ckpt-4000000"]
MASKED = ["walk/ik/model.ckpt-2000000", "turn/ik/model.ckpt-2000000"]     # (tests/test_agents_policy_player.py MASKED)
MASKED_SCOPE = "memory/"


def main(reference):
    sys.path.insert(0, ROOT)
    from rex_gym_amd.agents.tf_checkpoint import Checkpoint
    src_root = os.path.join(reference, "rex_gym", "policies")
    for rel in PREFIXES:
        src, dst = os.path.join(src_root, rel), os.path.join(OUT, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(src + ".index", dst + ".index")
        data = src + ".data-00000-of-00001"
        if os.path.exists(data):
            with open(data, "rb") as f:
                buf = bytearray(f.read())
            if rel in MASKED:
                for name, e in Checkpoint(src).entries.items():
                    if name.startswith(MASKED_SCOPE):
                        buf[e["offset"]:e["offset"] + e["size"]] = bytes(e["size"])
            with lzma.open(dst + ".data-00000-of-00001.xz", "wb", preset=9 | lzma.PRESET_EXTREME) as g:
                g.write(bytes(buf))
        print(rel, "(memory/* zeroed)" if rel in MASKED else "")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
