"""No GPU: the C entries of the three point queries (creg_point_mesh_f64, creg_pose_fit_system_f64, creg_link_moments_f64) answer
one bad argument each with CREG_EINVAL and a fixed text, and their *_workspace_bytes calls answer fixed sizes.  There is no device
here (a HIP call would give CREG_EHIP) and the pointers are made-up addresses that are never dereferenced: every case returns
before any HIP call.  The texts and the sizes were recorded by running these tables against the library as it was before the three
entries shared point_query_check (mesh_pose.hip), when each spelled its checks itself."""
import ctypes

import pytest

EINVAL = -1
P = ctypes.c_void_p(0x1000)
NAN = float("nan")
BIG = 2 ** 64 - 1                                                # a workspace that is never the fault
PM, PF, LM = "creg_point_mesh_f64", "creg_pose_fit_system_f64", "creg_link_moments_f64"

# every entry's arguments by name, valid as they stand: F = 300 triangles in L = 3 links, P = 2 poses, N = 100 points, J = 4 joints
MESH = dict(tri=P, tri_start=P, n_tri=300, link_T=P, n_links=3, n_poses=2, pts=P, pt_start=P, n_pts=100, d_max=0.5)
ARGS = {
    PM: dict(MESH, dist2=P, tri_idx=P, link_box=P, workspace=P, workspace_bytes=44288, stream=None),
    PF: dict(MESH, tri_idx=P, parent=P, child=P, type=P, origin=P, axis=P, n_joints=4, chain=P, center=P, H=P, g=P, cost=P, n=P,
             workspace=P, workspace_bytes=5120, stream=None),
    LM: dict(MESH, tri_idx=P, ref=P, mom=P, cnt=P, workspace=P, workspace_bytes=1280, stream=None),
}
SHIFT = {PM: 6, PF: 5, LM: 6}                                    # a tile is 1 << SHIFT rows

NULL_PM = "null pt_start, or null pts / dist2 / tri_idx with n_pts 100"
NULL_PF = "null pt_start, chain, center, H, g, cost or n"
NULL_LM = "null pt_start, ref, mom or cnt"
SLOTS = "n_poses >= 1 and (n_pts >> %d) + n_poses < 2^31 (got %d)"
# (entry, the one fault, creg_last_error() after it without the entry's name)
FAULTS = [(e, f, t) for e in (PM, PF, LM) for f, t in [
    (dict(d_max=-1.0), "d_max must be >= 0 (+inf allowed), got -1"),
    (dict(d_max=NAN), "d_max must be >= 0 (+inf allowed), got nan"),
    (dict(n_pts=-1), "0 <= n_pts < 2^31 (got -1)"),
    (dict(n_pts=2 ** 31), "0 <= n_pts < 2^31 (got 2147483648)"),
    (dict(tri=None), "null pointer"),
    (dict(tri_start=None), "null pointer"),
    (dict(link_T=None), "null pointer"),
    (dict(workspace=None), "null pointer"),
    (dict(workspace_bytes=ARGS[e]["workspace_bytes"] - 1),
     "workspace of %d bytes, %d needed" % (ARGS[e]["workspace_bytes"] - 1, ARGS[e]["workspace_bytes"])),
]] + [
    # n_poses = 0, and the tile-slot count (n_pts >> SHIFT) + n_poses at 2^31
    (PM, dict(n_poses=0), "bad argument (n_tri 300, n_links 3, n_poses 0, n_pairs 0)"),
    (PF, dict(n_poses=0), SLOTS % (5, 0)),
    (LM, dict(n_poses=0), SLOTS % (6, 0)),
    (PM, dict(n_poses=2 ** 31 - (100 >> 6), workspace_bytes=BIG), "(n_pts >> 6) + n_poses < 2^31 (got 2147483648)"),
    (PF, dict(n_poses=2 ** 31 - (100 >> 5), workspace_bytes=BIG), SLOTS % (5, 2147483645)),
    (LM, dict(n_poses=2 ** 31 - (100 >> 6), workspace_bytes=BIG), SLOTS % (6, 2147483647)),
    # n_links = 0 and 65536, n_joints = 59 (D = 65) and -1
    (PM, dict(n_links=0), "bad argument (n_tri 300, n_links 0, n_poses 2, n_pairs 0)"),
    (PF, dict(n_links=0), "bad argument (n_tri 300, n_links 0, n_poses 2, n_pairs 0)"),
    (LM, dict(n_links=0), "1 <= n_links <= 65535 (got 0)"),
    (PM, dict(n_links=65536, workspace_bytes=BIG), "n_tri < 2^31 and n_links <= 65535 (got 300, 65536)"),
    (PF, dict(n_links=65536, workspace_bytes=BIG), "n_tri < 2^31 and n_links <= 65535 (got 300, 65536)"),
    (LM, dict(n_links=65536, workspace_bytes=BIG), "1 <= n_links <= 65535 (got 65536)"),
    (PF, dict(n_joints=59, workspace_bytes=BIG), "0 <= n_joints and D = 6 + n_joints <= 64 (got n_joints 59)"),
    (PF, dict(n_joints=-1), "0 <= n_joints and D = 6 + n_joints <= 64 (got n_joints -1)"),
    # null pt_start, null per-point arrays with n_pts > 0, each entry's null outputs and tables
    (PM, dict(pt_start=None), NULL_PM), (PM, dict(pts=None), NULL_PM), (PM, dict(tri_idx=None), NULL_PM), (PM, dict(dist2=None), NULL_PM),
    (PF, dict(pt_start=None), NULL_PF), (PF, dict(chain=None), NULL_PF), (PF, dict(center=None), NULL_PF), (PF, dict(H=None), NULL_PF),
    (PF, dict(g=None), NULL_PF), (PF, dict(cost=None), NULL_PF), (PF, dict(n=None), NULL_PF),
    (PF, dict(pts=None), "null pts / tri_idx with n_pts 100"), (PF, dict(tri_idx=None), "null pts / tri_idx with n_pts 100"),
    (PF, dict(parent=None), "null joint table with n_joints 4"), (PF, dict(axis=None), "null joint table with n_joints 4"),
    (LM, dict(pt_start=None), NULL_LM), (LM, dict(ref=None), NULL_LM), (LM, dict(mom=None), NULL_LM), (LM, dict(cnt=None), NULL_LM),
    (LM, dict(pts=None), "null pts / tri_idx with n_pts 100"), (LM, dict(tri_idx=None), "null pts / tri_idx with n_pts 100"),
]

# (the counts, the size): point mesh (n_tri, n_links, n_poses, n_pts), the other two (n_poses, n_pts, n_joints or n_links)
SIZES = {
    "creg_point_mesh_workspace_bytes": [
        ((300, 3, 2, 100), 44288), ((0, 1, 1, 0), 512), ((1000, 5, 7, 12345), 508928), ((300, 65536, 2, 100), 12626432),
        ((-1, 3, 2, 100), 0), ((2 ** 31, 3, 2, 100), 0), ((300, 0, 2, 100), 0), ((300, 3, 0, 100), 0), ((300, 3, 2, -1), 0),
        ((300, 3, 2, 2 ** 31), 0)],
    "creg_pose_fit_workspace_bytes": [
        ((2, 100, 4), 5120), ((1, 0, 0), 512), ((7, 12345, 58), 13071872), ((2 ** 31 - 4, 100, 0), 755914243840),
        ((0, 100, 4), 0), ((2, -1, 4), 0), ((2, 2 ** 31, 4), 0), ((2, 100, -1), 0), ((2, 100, 59), 0), ((2 ** 31 - 3, 100, 4), 0)],
    "creg_link_moments_workspace_bytes": [
        ((2, 100, 3), 1280), ((1, 0, 1), 256), ((7, 12345, 65535), 1773639424), ((2 ** 31 - 2, 100, 1), 292057776128),
        ((0, 100, 3), 0), ((2, -1, 3), 0), ((2, 2 ** 31, 3), 0), ((2, 100, 0), 0), ((2, 100, 65536), 0), ((2 ** 31 - 1, 100, 3), 0)],
}


@pytest.fixture(scope="module")
def lib():
    from autourdf_amd import _lib
    return _lib.load(check_device=False)


def test_the_tables_follow_the_bound_signatures():
    from autourdf_amd import _lib
    for entry, args in ARGS.items():
        assert len(args) == len(_lib.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("entry,fault,text", FAULTS, ids=[f"{e[5:-4]}-{'-'.join(f)}-{i}" for i, (e, f, _) in enumerate(FAULTS)])
def test_one_fault_gives_einval_and_the_recorded_text(lib, entry, fault, text):
    assert set(fault) <= set(ARGS[entry]), (entry, fault)
    rc = getattr(lib, entry)(*dict(ARGS[entry], **fault).values())
    assert (rc, lib.creg_last_error().decode()) == (EINVAL, f"{entry}: {text}")


def test_the_fault_table_covers_every_entry_and_every_fault():
    seen = [(e, tuple(sorted(f))) for e, f, _ in FAULTS]
    outs = {PM: ("dist2", "tri_idx"), PF: ("H", "g", "cost", "n"), LM: ("mom", "cnt")}
    for e in (PM, PF, LM):
        assert seen.count((e, ("d_max",))) == 2 and seen.count((e, ("n_pts",))) == 2, e            # negative and NaN, -1 and 2^31
        for f in (("n_poses",), ("n_poses", "workspace_bytes"), ("n_links",), ("n_links", "workspace_bytes"), ("pt_start",), ("pts",),
                  ("tri_idx",), ("workspace_bytes",)) + tuple((o,) for o in outs[e]):
            assert (e, f) in seen, (e, f)
    assert (PF, ("n_joints", "workspace_bytes")) in seen


def test_the_workspace_sizes_are_the_recorded_ones(lib):
    for name, rows in SIZES.items():
        for counts, size in rows:
            assert getattr(lib, name)(*counts) == size, (name, counts)
    for entry, size in ((PM, lib.creg_point_mesh_workspace_bytes(300, 3, 2, 100)), (PF, lib.creg_pose_fit_workspace_bytes(2, 100, 4)),
                        (LM, lib.creg_link_moments_workspace_bytes(2, 100, 3))):
        assert ARGS[entry]["workspace_bytes"] == size, entry
