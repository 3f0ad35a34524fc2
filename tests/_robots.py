"""Real robot descriptions for the tests: tests/golden/robots/ holds URDFs and the meshes they name, xz-compressed, one file per
asset, at their paths under Robot/ (tests/golden/make_golden_robots.py made them).  `unpack_robots(d)` writes the tree to `d` and
returns the path of d/Robot, so a URDF's own mesh references resolve as they do in the original tree."""
import lzma
import os

GOLDEN_ROBOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robots")


def unpack_robots(d):
    for dirpath, _, files in os.walk(GOLDEN_ROBOTS):
        for name in files:
            if not name.endswith(".xz"):
                continue
            src = os.path.join(dirpath, name)
            dst = os.path.join(str(d), os.path.relpath(src, GOLDEN_ROBOTS)[:-len(".xz")])
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(src, "rb") as f, open(dst, "wb") as g:
                g.write(lzma.decompress(f.read()))
    return os.path.join(str(d), "Robot")
