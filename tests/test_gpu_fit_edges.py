"""GPU: creg_pose_fit_system_f64 (csrc/pose_fit.hip) and creg_link_moments_f64 (csrc/link_moments.hip) at their tile, width, slot
and table edges, on the synthetic chain robot of tests/_fit_edges.py (59 links, 58 joints: D up to the limit of 64).

Every value comparison is bit equality with the ordered restatements of _fit_edges -- the header's "order" paragraph in float64,
checked on the CPU against the long-double sums by tests/test_fit_edges_cpu.py -- or an exact zero or an exact count; nothing
here is measured from a kernel.  No input lies outside the header's contract: pt_start and tri_start never decrease, and values
out of range stand only where the header clamps them or reads them as "no correspondence".  Every test runs under its own
watchdog, which ends the process: a hung kernel must not be waited on."""
import ctypes
import faulthandler
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_edges as E  # noqa: E402
import _link_moments_ref as lm  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("A", "B", "C", "C_loose", "D")
POISON = 0x7FF80000DEADBEEF                                      # a quiet NaN
GUARD, SENTINEL_ROWS, SENTINEL = 256, 64, -7


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(got, want, keys, what=""):
    for key in keys:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (what, key)
        np.testing.assert_array_equal(bits(got[key]), bits(want[key]), err_msg=f"{what} {key}")


# ------------------------------------------------------------------------------------------ cases and references, built once
@functools.lru_cache(maxsize=None)
def robot():
    return E.chain_robot()


@functools.lru_cache(maxsize=None)
def case_of(name):
    return E.loose_ends(case_of("C")) if name == "C_loose" else E.layout(robot(), name)


@functools.lru_cache(maxsize=None)
def want_system(name, J):
    return E.system_of(case_of(name), E.table_of_width(robot(), J))


@functools.lru_cache(maxsize=None)
def want_moments(name, L):
    return E.moments_of(E.cut_links(case_of(name), L))


SYSTEM_KEYS, MOMENT_KEYS = ("H", "g", "cost", "n"), ("mom", "cnt")


def run_system(case, table):
    from autourdf_amd import ops
    out = ops.pose_fit_system(dev(case["tri"]), dev(case["tri_start"]), dev(case["link_T"]), dev(case["pts"]), dev(case["pt_start"]),
                              dev(case["tri_idx"]), table, dev(case["center"]), case["d_max"])
    return dict(zip(SYSTEM_KEYS, (x.cpu().numpy() for x in out)))


def run_moments(case):
    from autourdf_amd import ops
    out = ops.link_moments(dev(case["tri"]), dev(case["tri_start"]), dev(case["link_T"]), dev(case["pts"]), dev(case["pt_start"]),
                           dev(case["tri_idx"]), dev(case["ref"]), case["d_max"])
    return dict(zip(MOMENT_KEYS, (x.cpu().numpy() for x in out)))


@functools.lru_cache(maxsize=None)
def got_system(name, J):
    return run_system(case_of(name), E.table_of_width(robot(), J))


@functools.lru_cache(maxsize=None)
def got_moments(name, L):
    return run_moments(E.cut_links(case_of(name), L))


# ------------------------------------------------------------------------------------------ the C ABI with poisoned buffers
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _poisoned(need):
    """need bytes of a NaN bit pattern and GUARD bytes of 0xA5 behind them."""
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device="cuda")
    ws[:need].view(torch.int64).fill_(POISON)
    ws[need:].fill_(0xA5)
    return ws


def _outputs(shapes):
    """Per (rows, tail shape, dtype) a buffer of rows + 64 rows of the sentinel."""
    return [torch.full((rows + SENTINEL_ROWS,) + tail, SENTINEL, dtype=dt, device="cuda") for rows, tail, dt in shapes]


def _check_buffers(outs, rows, ws, need, what):
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[rows:] == SENTINEL).all()), (what, "rows behind an output were written")
        assert not bool(torch.isnan(o[:rows].to(torch.float64)).any()), (what, "a NaN of the workspace reached an output")
    assert bool((ws[need:] == 0xA5).all()), (what, "bytes past workspace_bytes were written")


def abi_system(case, table, chain=None, n_pts=None):
    """creg_pose_fit_system_f64 with a caller-built chain, sentinel rows behind every output, a workspace of NaNs and guard bytes
    behind it -> (rc, outputs as run_system gives them)."""
    from autourdf_amd import _lib, ops
    lib = _lib.load()
    P, L, F, J = len(case["link_T"]), case["link_T"].shape[1], len(case["tri"]), len(table["parent"])
    N = len(case["pts"]) if n_pts is None else n_pts
    D = 6 + J
    d = {k: dev(case[k]) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "center")}
    tdev = [dev(np.ascontiguousarray(table[k])) for k in ("parent", "child", "type", "origin", "axis")]
    mask = ops.joint_chains(table) if chain is None else np.array([int(x) for x in chain], np.uint64)
    cdev = dev(mask.view(np.int64))
    need = lib.creg_pose_fit_workspace_bytes(P, N, J)
    assert need > 0 and need % 256 == 0
    ws = _poisoned(need)
    outs = _outputs([(P, (D, D), torch.float64), (P, (D,), torch.float64), (P, (), torch.float64), (P, (), torch.int64)])
    rc = lib.creg_pose_fit_system_f64(_ptr(d["tri"]), _ptr(d["tri_start"]), F, _ptr(d["link_T"]), L, P, _ptr(d["pts"]), _ptr(d["pt_start"]), N,
                                      float(case["d_max"]), _ptr(d["tri_idx"]), *[_ptr(t) for t in tdev], J, _ptr(cdev), _ptr(d["center"]),
                                      *[_ptr(o) for o in outs], _ptr(ws), need, None)
    _check_buffers(outs, P, ws, need, f"pose fit D = {D}")
    return rc, dict(zip(SYSTEM_KEYS, (o[:P].cpu().numpy() for o in outs)))


def abi_moments(case, n_pts=None):
    from autourdf_amd import _lib
    lib = _lib.load()
    P, L, F = len(case["link_T"]), case["link_T"].shape[1], len(case["tri"])
    N = len(case["pts"]) if n_pts is None else n_pts
    d = {k: dev(case[k]) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "ref")}
    need = lib.creg_link_moments_workspace_bytes(P, N, L)
    assert need > 0 and need % 256 == 0
    ws = _poisoned(need)
    outs = _outputs([(P, (L, 16), torch.float64), (P, (L,), torch.int64)])
    rc = lib.creg_link_moments_f64(_ptr(d["tri"]), _ptr(d["tri_start"]), F, _ptr(d["link_T"]), L, P, _ptr(d["pts"]), _ptr(d["pt_start"]), N,
                                   float(case["d_max"]), _ptr(d["tri_idx"]), _ptr(d["ref"]), *[_ptr(o) for o in outs], _ptr(ws), need, None)
    _check_buffers(outs, P, ws, need, f"link moments L = {L}")
    return rc, dict(zip(MOMENT_KEYS, (o[:P].cpu().numpy() for o in outs)))


# ================================================================================================ 1. the order, in bits
@pytest.mark.parametrize("J", E.POSE_FIT_WIDTHS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_pose_fit_has_the_bits_of_the_ordered_restatement(name, J):
    """k_pose_fit_tiles / k_pose_fit_finish: layouts A (every pose size around a tile of 32, main loop with a tail of 0 .. 3
    tiles, empty poses first, last and in a run), B (100 one-row poses: p dominates the slot), C (unowned rows in front and
    behind), C with pt_start[0] = -3, pt_start[P] = n_pts + 9, and D (11, 13 and 15 tiles), at D = 6 (no joint: the frames kernel is skipped), 15 (E = 242:
    one chunk, one trip), 16 (E = 274: two chunks, a second trip), 63 and 64 (the limit: 17 chunks, chain bits up to 57, two
    skipped joints).  H, g, cost and n equal the header's order bit for bit."""
    got, want = got_system(name, J), want_system(name, J)
    same_bits(got, want, SYSTEM_KEYS, f"layout {name} D = {6 + J}")
    np.testing.assert_array_equal(bits(got["H"]), bits(got["H"].transpose(0, 2, 1)))
    kinds = np.asarray(robot()["table"]["type"])[:J]
    still = [6 + j for j in range(J) if kinds[j] not in (1, 2) or (J == 58 and j in E.SKIPPED)]
    assert not bits(got["H"][:, still, :]).any() and not bits(got["H"][:, :, still]).any() and not bits(got["g"][:, still]).any()
    assert got["n"].sum() > 100


@pytest.mark.parametrize("L", E.MOMENT_WIDTHS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_link_moments_have_the_bits_of_the_ordered_restatement(name, L):
    """k_link_moments_tiles / k_link_moments_finish: the same layouts (tiles of 64: in A to C a main loop with a tail of 0 or 1 tiles,
    and 1, 2 and 3 tiles alone; in D 6, 7 and 8 tiles, a main loop with a tail of 2, 3 and 0 -- only behind a main loop does a tail
    tile added into the wrong running sum change bits, see test_fit_edges_cpu.py) at L = 1, 15 (255 entries: one trip), 16 (272: a second trip) and 59 (1003: four trips); the smaller
    L are the chain's first links, the rows of the others then carry a tri_idx past the mesh."""
    got, want = got_moments(name, L), want_moments(name, L)
    same_bits(got, want, MOMENT_KEYS, f"layout {name} L = {L}")
    assert not bits(got["mom"][got["cnt"] == 0]).any() and got["cnt"].sum() > 0


def test_loose_ends_are_clamped_not_ignored():
    """pt_start[0] = -3 and pt_start[P] = n_pts + 9: pose 0 owns the five rows in front and the last pose the seven behind (they
    have none in layout C itself), the poses between keep their bits."""
    tight, loose = got_system("C", 9), got_system("C_loose", 9)
    assert tight["n"][0] == 0 and loose["n"][0] > 0 and tight["n"][-1] == 0 and loose["n"][-1] > 0
    same_bits({k: v[1:-1] for k, v in loose.items()}, {k: v[1:-1] for k, v in tight.items()}, SYSTEM_KEYS)
    mt, ml = got_moments("C", 59), got_moments("C_loose", 59)
    assert mt["cnt"][0].sum() == 0 and ml["cnt"][0].sum() == loose["n"][0] and ml["cnt"][-1].sum() == loose["n"][-1]
    same_bits({k: v[1:-1] for k, v in ml.items()}, {k: v[1:-1] for k, v in mt.items()}, MOMENT_KEYS)


# ================================================================================================ 2. table and link edges
@pytest.mark.parametrize("bad", [False, True], ids=["borders", "no_correspondence"])
def test_link_borders_empty_links_and_rows_without_correspondence(bad):
    """The bisection for the link and the range checks: tri_start = -5 4 4 4 12 F + 7 over F = 16 triangles (clamped ends, two
    empty links sharing a start), rows at the first and last triangle of every link that has rows; with ``bad`` five rows carry
    tri_idx -1, F, F + 1, INT32_MIN and INT32_MAX.  Counts by hand, sums in the bits of the restatement (every link under its
    own pose: a row given to a neighbouring link shows), so the neighbours of the five rows keep their bits."""
    case = E.border_case(bad=bad)
    by_hand = np.bincount(E.border_links(case["tri_idx"]), minlength=5)
    assert by_hand.sum() == (35 if bad else 40) and by_hand[1] == by_hand[2] == 0
    mom = run_moments(case)
    np.testing.assert_array_equal(mom["cnt"][0], by_hand)
    same_bits(mom, E.moments_of(case), MOMENT_KEYS)
    table = lm._no_joints(5)
    got = run_system(case, dict(table))
    assert got["n"][0] == by_hand.sum()
    same_bits(got, E.system_of(case, table), SYSTEM_KEYS)


def test_gate_tie_contributes_and_one_ulp_below_does_not():
    """dot(r, r) = 0.0625 exactly against d_max^2: in at d_max = 0.25, out at the next double below, in at d_max = inf."""
    for d_max, n in ((E.GATE, 1), (float(np.nextafter(E.GATE, 0.0)), 0), (np.inf, 1)):
        case = E.gate_case(d_max)
        got, mom = run_system(case, lm._no_joints(1)), run_moments(case)
        assert got["n"][0] == n and got["cost"][0] == 0.0625 * n and mom["cnt"][0, 0] == n and mom["mom"][0, 0, 15] == 0.0625 * n, d_max
        np.testing.assert_array_equal(got["H"][0, 3:6, 3:6], float(n) * np.eye(3))
        assert got["g"][0, 3] == -0.25 * n and mom["mom"][0, 0, 12] == -0.25 * n


def test_d_max_zero_keeps_a_point_on_the_surface():
    case = E.zero_gate_case()
    got, mom = run_system(case, lm._no_joints(1)), run_moments(case)
    assert list(got["n"]) == [1, 0] and list(mom["cnt"][:, 0]) == [1, 0]
    assert bits(got["cost"])[0] == 0 and not got["g"].any() and not got["H"][1].any() and not mom["mom"][1].any()
    np.testing.assert_array_equal(got["H"][0, 3:6, 3:6], np.eye(3))
    same_bits(got, E.system_of(case, lm._no_joints(1)), SYSTEM_KEYS)
    same_bits(mom, E.moments_of(case), MOMENT_KEYS)


def test_chain_bits_above_32_and_a_cleared_bit_through_the_c_abi():
    """48 rows on the last link of the J = 58 chain: the columns 6 + j of every revolute and prismatic joint j = 4 .. 57 of its
    chain are non-zero -- j >= 32 among them -- and those of type 0, type 3 and the two skipped joints exactly 0.0.  With bit 40
    cleared in a caller-built chain, exactly row and column 46 become 0.0 and every other entry keeps its bits."""
    case, table = E.last_link_case(robot()), E.table_of_width(robot(), 58)
    chain = pf.chains(table)
    rc, got = abi_system(case, table, chain)
    assert rc == 0 and got["n"][0] == 48
    same_bits(got, E.system_of(case, table), SYSTEM_KEYS)
    same_bits(got, run_system(case, table), SYSTEM_KEYS)                       # the wrapper's own chain masks
    kinds, diag = np.asarray(table["type"]), np.diagonal(got["H"][0])
    for j in range(58):
        moves = kinds[j] in (1, 2) and j >= 4
        assert (diag[6 + j] > 0) == moves and (got["g"][0, 6 + j] != 0) == moves, j
        if not moves:
            assert not bits(got["H"][0, 6 + j]).any() and not bits(got["H"][0, :, 6 + j]).any() and bits(got["g"][0])[6 + j] == 0, j
    cleared = list(chain)
    cleared[58] &= ~(1 << E.HIGH_BIT)
    rc, less = abi_system(case, table, cleared)
    assert rc == 0
    k = 6 + E.HIGH_BIT
    assert not bits(less["H"][0, k]).any() and not bits(less["H"][0, :, k]).any() and bits(less["g"][0])[k] == 0
    keep = np.arange(64) != k
    np.testing.assert_array_equal(bits(less["H"][0][np.ix_(keep, keep)]), bits(got["H"][0][np.ix_(keep, keep)]))
    np.testing.assert_array_equal(bits(less["g"][0][keep]), bits(got["g"][0][keep]))
    same_bits({k_: less[k_] for k_ in ("cost", "n")}, got, ("cost", "n"))


# ================================================================================================ 3. independence
@pytest.mark.parametrize("p", [4, 10, 13])
def test_a_pose_alone_has_the_bits_it_has_among_the_others(p):
    """Poses 4 (33 rows), 10 (129) and 13 (289) of layout A alone in a call, at D = 64 and L = 59: another slot, another start
    row, the same bits."""
    alone = E.one_pose(case_of("A"), p)
    got = run_system(alone, E.table_of_width(robot(), 58))
    same_bits(got, {k: v[p:p + 1] for k, v in got_system("A", 58).items()}, SYSTEM_KEYS, f"pose {p}")
    mom = run_moments(alone)
    same_bits(mom, {k: v[p:p + 1] for k, v in got_moments("A", 59).items()}, MOMENT_KEYS, f"pose {p}")


def test_two_runs_and_a_link_without_the_others_give_the_same_bits():
    case = case_of("A")
    same_bits(run_system(case, E.table_of_width(robot(), 58)), got_system("A", 58), SYSTEM_KEYS)
    first = got_moments("A", 59)
    same_bits(run_moments(case), first, MOMENT_KEYS)
    link = want_moments("A", 59)["link"]
    only = dict(case, tri_idx=np.where(link == 30, case["tri_idx"], -1).astype(np.int32))
    mom = run_moments(only)
    assert first["cnt"][:, 30].sum() >= 5 and (first["cnt"][:, 30] > 0).sum() >= 3
    same_bits({k: v[:, 30] for k, v in mom.items()}, {k: v[:, 30] for k, v in first.items()}, MOMENT_KEYS)
    others = np.arange(59) != 30
    assert not bits(mom["mom"][:, others]).any() and not mom["cnt"][:, others].any()


# ================================================================================================ 4. buffers, 5. the limit
@pytest.mark.parametrize("J", [10, 58])
@pytest.mark.parametrize("name", ["A", "C"])
def test_pose_fit_reads_no_slot_it_did_not_write_and_writes_nothing_else(name, J):
    """The C ABI at D = 16 and D = 64 (the limit: the call returns 0 with 52.6 KiB of dynamic LDS) with a workspace of NaNs: every
    slot the finish pass reads was written by the tile pass, so the outputs have the bits of the restatement; the 64 sentinel
    rows behind every output and the 256 bytes behind workspace_bytes are untouched."""
    rc, got = abi_system(case_of(name), E.table_of_width(robot(), J))
    assert rc == 0
    same_bits(got, want_system(name, J), SYSTEM_KEYS, f"layout {name} D = {6 + J}")


@pytest.mark.parametrize("L", [16, 59])
@pytest.mark.parametrize("name", ["A", "C"])
def test_link_moments_read_no_slot_they_did_not_write_and_write_nothing_else(name, L):
    rc, got = abi_moments(E.cut_links(case_of(name), L))
    assert rc == 0
    same_bits(got, want_moments(name, L), MOMENT_KEYS, f"layout {name} L = {L}")


def test_no_points_and_several_poses_give_zeros_from_a_poisoned_workspace():
    """n_pts = 0: the tile pass is not launched, the finish pass reads no slot; pt_start keeps its values, all clamped to 0."""
    case = case_of("A")
    rc, got = abi_system(case, E.table_of_width(robot(), 58), n_pts=0)
    assert rc == 0 and got["H"].shape == (15, 64, 64)
    assert not any(bits(got[k]).any() for k in SYSTEM_KEYS)
    rc, mom = abi_moments(case, n_pts=0)
    assert rc == 0 and mom["mom"].shape == (15, 59, 16)
    assert not any(bits(mom[k]).any() for k in MOMENT_KEYS)
