"""Copy the robot descriptions tests/test_sim_cpu.py parses into tests/golden/robots/, xz-compressed, one file per asset.

    python tests/golden/make_golden_robots.py <directory holding the reference's Robot/ tree>

Each URDF is stored with exactly the mesh files it names (wx200 and allegro: binary STL; franka: the COLLADA visuals), at the
same relative paths under Robot/, so the URDFs' own mesh references resolve once the tree is unpacked (tests/_robots.py).
The files are data: they are read by autourdf_amd.sim_data's URDF / mesh readers and never executed."""
import lzma
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "robots")
URDFS = ["Robot/interbotix_descriptions/urdf/wx200_real.urdf",
         "Robot/allegro_hand_description/allegro_hand_description_left.urdf",
         "Robot/franka/franka_panda.urdf"]


def mesh_paths(src_root, urdf_rel):
    """Paths (relative to src_root) of the meshes a URDF's <visual> elements name, resolved as sim_data.UrdfRobot does."""
    text = open(os.path.join(src_root, urdf_rel)).read()
    out = []
    for vis in re.findall(r"<visual>.*?</visual>", text, re.S):
        for name in re.findall(r'<mesh[^>]*filename="([^"]+)"', vis):
            if name.startswith("package://"):
                rel = "Robot/" + name[len("package://"):]
            elif name.startswith("Robot/"):
                rel = name
            else:
                rel = os.path.normpath(os.path.join(os.path.dirname(urdf_rel), name))
            if rel not in out:
                out.append(rel)
    return out


def main(src_root):
    shutil.rmtree(OUT, ignore_errors=True)
    total = 0
    for urdf in URDFS:
        for rel in [urdf] + mesh_paths(src_root, urdf):
            dst = os.path.join(OUT, rel + ".xz")
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(os.path.join(src_root, rel), "rb") as f:
                data = lzma.compress(f.read(), preset=9 | lzma.PRESET_EXTREME)
            assert len(data) < 1 << 20, (rel, len(data))
            with open(dst, "wb") as f:
                f.write(data)
            total += len(data)
            print(f"{rel}: {len(data)} B")
    print(f"total {total} B")


if __name__ == "__main__":
    main(sys.argv[1])
