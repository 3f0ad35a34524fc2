"""No GPU: the C entries of the URDF stage's joint part answer one bad argument each with CREG_EINVAL and a fixed text.  There is
no device here (a HIP call would give CREG_EHIP) and the pointers are made-up addresses that are never dereferenced: every case
returns before any HIP call.  The texts are those of the library before the entries shared their argument checks."""
import ctypes

import pytest

OK, EINVAL = 0, -1
P = ctypes.c_void_p(0x1000)
NAN, INF = float("nan"), float("inf")

# every entry's arguments by name, valid as they stand (S=2 sequences of T=20 steps, K=8 clusters in L=4 links, J=3 joints)
ARGS = {
    "creg_joint_axes_f64": dict(
        coords=P, S=2, T=20, K=8, link_clusters=P, link_offsets=P, n_link_clusters=8, joints=P, J=3, start_step=0, num_steps=10,
        interval=1, sample_axis=P, sample_angle=P, sample_point=P, sample_usable=P, local_axis=P, local_pos=P, global_pos=P,
        global_axis=P, count=P, first_pose=P, stream=None),
    "creg_joint_types_f64": dict(
        coords=P, S=2, T=20, K=8, link_clusters=P, link_offsets=P, n_link_clusters=8, L=4, joints=P, J=3, start_step=0,
        num_steps=10, interval=1, turn_min=2e-4, slide_min=1e-6, sample_angle=P, sample_slide=P, sample_kind=P, counts=P, type=P,
        slide_axis=P, global_axis=P, global_pos=P, stream=None),
    "creg_joint_positions_f64": dict(
        link_T=P, S=2, T=20, L=4, joints=P, J=3, local_axis=P, local_pos=P, ref_seq=0, ref_step=0, start_step=0, num_steps=10,
        q=P, tilt=P, slip=P, summary=P, where=P, stream=None),
    "creg_joint_slides_f64": dict(
        link_T=P, S=2, T=20, L=4, joints=P, J=3, local_axis=P, ref_seq=0, ref_step=0, start_step=0, num_steps=10, q=P, tilt=P,
        slip=P, summary=P, where=P, stream=None),
    "creg_link_poses_f64": dict(
        coords=P, S=2, T=20, K=8, link_clusters=P, link_offsets=P, n_link_clusters=8, L=4, link_T=P, stream=None),
}
SAMPLED = ("creg_joint_axes_f64", "creg_joint_types_f64")
SERIES = ("creg_joint_positions_f64", "creg_joint_slides_f64")

# (entry, the one fault, return code, creg_last_error() after it)
FAULTS = [
    # K = 257
    ("creg_joint_axes_f64", dict(K=257), "creg_joint_axes_f64: bad size (S=2, T=20, K=257, J=3; K <= 256)"),
    ("creg_joint_types_f64", dict(K=257), "creg_joint_types_f64: bad size (S=2, T=20, K=257, L=4, J=3; K <= 256)"),
    ("creg_link_poses_f64", dict(K=257), "creg_link_poses_f64: bad size (S=2, T=20, K=257, L=4; K <= 256, S*T*L < 2^31)"),
    # num_steps = 0
    ("creg_joint_axes_f64", dict(num_steps=0), "creg_joint_axes_f64: bad steps (start=0, num=0, interval=1)"),
    ("creg_joint_types_f64", dict(num_steps=0), "creg_joint_types_f64: bad steps (start=0, num=0, interval=1)"),
    ("creg_joint_positions_f64", dict(num_steps=0), "creg_joint_positions_f64: steps [0, 0 + 0) out of range for T=20"),
    ("creg_joint_slides_f64", dict(num_steps=0), "creg_joint_slides_f64: steps [0, 0 + 0) out of range for T=20"),
    # interval = 0
    ("creg_joint_axes_f64", dict(interval=0), "creg_joint_axes_f64: bad steps (start=0, num=10, interval=0)"),
    ("creg_joint_types_f64", dict(interval=0), "creg_joint_types_f64: bad steps (start=0, num=10, interval=0)"),
    # start_step + num_steps = T + 1
    ("creg_joint_axes_f64", dict(start_step=11), "creg_joint_axes_f64: step 20 out of range for T=20"),
    ("creg_joint_types_f64", dict(start_step=11), "creg_joint_types_f64: step 20 out of range for T=20"),
    ("creg_joint_positions_f64", dict(start_step=11), "creg_joint_positions_f64: steps [11, 11 + 10) out of range for T=20"),
    ("creg_joint_slides_f64", dict(start_step=11), "creg_joint_slides_f64: steps [11, 11 + 10) out of range for T=20"),
    # 4097 samples: one sequence of 4098 steps at interval 1
    ("creg_joint_axes_f64", dict(S=1, T=5000, num_steps=4098), "creg_joint_axes_f64: 4097 samples per joint (max 4096)"),
    ("creg_joint_types_f64", dict(S=1, T=5000, num_steps=4098), "creg_joint_types_f64: 4097 samples per joint (max 4096)"),
    # S = 65536
    ("creg_joint_positions_f64", dict(S=65536), "creg_joint_positions_f64: bad size (S=65536, T=20, L=4, J=3; S <= 65535)"),
    ("creg_joint_slides_f64", dict(S=65536), "creg_joint_slides_f64: bad size (S=65536, T=20, L=4, J=3; S <= 65535)"),
    # ref_seq = S, ref_step = T
    ("creg_joint_positions_f64", dict(ref_seq=2), "creg_joint_positions_f64: reference pose (2, 0) outside (S=2, T=20)"),
    ("creg_joint_slides_f64", dict(ref_seq=2), "creg_joint_slides_f64: reference pose (2, 0) outside (S=2, T=20)"),
    ("creg_joint_positions_f64", dict(ref_step=20), "creg_joint_positions_f64: reference pose (0, 20) outside (S=2, T=20)"),
    ("creg_joint_slides_f64", dict(ref_step=20), "creg_joint_slides_f64: reference pose (0, 20) outside (S=2, T=20)"),
    # a null required pointer: the first, the last, and the samples' own message
    ("creg_joint_axes_f64", dict(coords=None), "creg_joint_axes_f64: null pointer"),
    ("creg_joint_axes_f64", dict(count=None), "creg_joint_axes_f64: null pointer"),
    ("creg_joint_axes_f64", dict(sample_point=None), "creg_joint_axes_f64: null sample output"),
    ("creg_joint_types_f64", dict(coords=None), "creg_joint_types_f64: null pointer"),
    ("creg_joint_types_f64", dict(global_pos=None), "creg_joint_types_f64: null pointer"),
    ("creg_joint_types_f64", dict(sample_kind=None), "creg_joint_types_f64: null sample output"),
    ("creg_joint_positions_f64", dict(link_T=None), "creg_joint_positions_f64: null pointer"),
    ("creg_joint_positions_f64", dict(local_pos=None), "creg_joint_positions_f64: null pointer"),
    ("creg_joint_positions_f64", dict(where=None), "creg_joint_positions_f64: null pointer"),
    ("creg_joint_slides_f64", dict(link_T=None), "creg_joint_slides_f64: null pointer"),
    ("creg_joint_slides_f64", dict(where=None), "creg_joint_slides_f64: null pointer"),
    ("creg_link_poses_f64", dict(coords=None), "creg_link_poses_f64: null pointer"),
    ("creg_link_poses_f64", dict(link_T=None), "creg_link_poses_f64: null pointer"),
    # thresholds that are not finite or negative
    ("creg_joint_types_f64", dict(turn_min=NAN),
     "creg_joint_types_f64: turn_min and slide_min must be finite and >= 0 (got nan, 1e-06)"),
    ("creg_joint_types_f64", dict(slide_min=INF),
     "creg_joint_types_f64: turn_min and slide_min must be finite and >= 0 (got 0.0002, inf)"),
    ("creg_joint_types_f64", dict(turn_min=-1e-3),
     "creg_joint_types_f64: turn_min and slide_min must be finite and >= 0 (got -0.001, 1e-06)"),
    ("creg_joint_types_f64", dict(slide_min=-1.0),
     "creg_joint_types_f64: turn_min and slide_min must be finite and >= 0 (got 0.0002, -1)"),
]


@pytest.fixture(scope="module")
def lib():
    from autourdf_amd import _lib
    return _lib.load(check_device=False)


def _call(lib, entry, **fault):
    args = dict(ARGS[entry], **fault)
    assert set(fault) <= set(ARGS[entry]), (entry, fault)
    rc = getattr(lib, entry)(*args.values())
    return rc, lib.creg_last_error().decode()


def test_the_tables_follow_the_bound_signatures():
    from autourdf_amd import _lib
    for entry, args in ARGS.items():
        assert len(args) == len(_lib.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("entry,fault,text", FAULTS, ids=[f"{e[5:-4]}-{'-'.join(f)}-{i}" for i, (e, f, _) in enumerate(FAULTS)])
def test_one_fault_gives_the_recorded_code_and_text(lib, entry, fault, text):
    assert _call(lib, entry, **fault) == (EINVAL, text)


def test_the_fault_table_covers_every_entry_and_every_fault():
    seen = {(e, tuple(sorted(f))) for e, f, _ in FAULTS}
    for e in SAMPLED:
        for f in (("K",), ("num_steps",), ("interval",), ("start_step",), ("S", "T", "num_steps"), ("coords",)):
            assert (e, f) in seen, (e, f)
    for e in SERIES:
        for f in (("num_steps",), ("start_step",), ("S",), ("ref_seq",), ("ref_step",), ("link_T",)):
            assert (e, f) in seen, (e, f)
    assert {("creg_link_poses_f64", ("K",)), ("creg_link_poses_f64", ("coords",))} <= seen


def test_no_joint_is_ok_before_the_pointers_are_looked_at(lib):
    """J == 0 with valid sizes: the three younger entries return CREG_OK before they look at a pointer; creg_joint_axes_f64
    refuses null pointers first and returns CREG_OK only with them in place."""
    nulls = {"creg_joint_types_f64": ("coords", "joints", "counts", "type", "slide_axis", "global_axis", "global_pos", "sample_kind"),
             "creg_joint_positions_f64": ("link_T", "joints", "local_axis", "local_pos", "q", "tilt", "slip", "summary", "where"),
             "creg_joint_slides_f64": ("link_T", "joints", "local_axis", "q", "tilt", "slip", "summary", "where")}
    for entry, names in nulls.items():
        assert _call(lib, entry, J=0)[0] == OK, entry
        assert _call(lib, entry, J=0, **{n: None for n in names})[0] == OK, entry
    assert _call(lib, "creg_joint_axes_f64", J=0)[0] == OK
    assert _call(lib, "creg_joint_axes_f64", J=0, joints=None) == (EINVAL, "creg_joint_axes_f64: null pointer")
    # a bad size is still refused without joints
    for entry in SAMPLED + SERIES:
        rc, text = _call(lib, entry, J=0, T=0)
        assert rc == EINVAL and text.startswith(entry + ": bad size"), (entry, text)
