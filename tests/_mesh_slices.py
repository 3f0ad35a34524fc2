"""The scenes of the launch-slice suite (tests/test_mesh_slices_cpu.py, tests/test_gpu_mesh_slices.py), no GPU.

The five mesh queries that pose a whole batch in one call -- creg_mesh_collide_f64, creg_mesh_clearance_f64, creg_mesh_contain_f64,
creg_point_mesh_f64, creg_mesh_cover_f64 -- cut it into launches of 65535 poses, and the pair queries also into launches of 65535
pairs (contain: 32767, two directions per pair).  A kernel of a later launch indexes with p = p0 + blockIdx.z and m = m0 +
blockIdx.y.  To reach that code without restating 65544 poses on the CPU, a long batch here is a short one repeated:

    K = 7 pose templates     tiled_poses(P)[p] = template[p % 7];   65535 % 7  = 1
    B = 11 base pairs        tiled_pairs(M)[m] = base[m % 11];      65535 % 11 = 8,   32767 % 11 = 9

A row of every output is a function of its own pose and pair alone, so row (p, m) of a long call carries the bits of row (p % 7,
m % 11) of the short call.  No remainder is 0: block 0 of a later launch that lost its offset would compute template 0 or base
pair 0 where template 1, base pair 8 or 9 belongs, and the templates' and pairs' answers differ (test_mesh_slices_cpu.py)."""
import functools

import numpy as np

import _clearance_ref as clref
import _contain_ref as conref
import _mesh_cover_ref as mcref
import _point_mesh_ref as pref
from _collide_ref import all_pairs, box_mesh, mesh_collide, pack, random_rotation, rigid, uv_sphere

K = 7                                                            # pose templates
SLICE, HALF_SLICE = 65535, 32767                                 # poses or pairs per launch; contain's pairs per launch
P_LONG = M_LONG = SLICE + 9                                      # one full slice and 9 more: every template occurs in the second
# default_rng(11) gives one (template, pair) cell with a unique positive clearance, and only 20 of the seeds 0 .. 7999 give three, so
# that the witnesses get compared: 5140 is the first of them that also has a pair of non-empty links beyond d_max
SEED, CLOUD_SEED, CONTAIN_SEED = 5140, 12, 13
D_MAX = 0.05
CLOUD_SIZES = (0, 1, 65, 2, 64, 3, 5)                            # points per template: none, around the 64-point tile, a few
LOOSE = (-5, 7)                                                  # tri_start[0] and tri_start[L] - F of the loose table
LOOSE_PTS = (-3, 9)                                              # contain's pt_start likewise


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)                                  # shared among the tests: left unchanged
    return arrays


# ------------------------------------------------------------------------------------------ the articulated scene
@functools.lru_cache(maxsize=None)
def scene():
    """tri (49,3,3), tri_start (5), templates (7,4,4,4): one large triangle, a box of 12, a sphere of 36 and an empty link under
    seven sets of random poses close enough for every pair of non-empty links to touch in some and not in others."""
    rng = np.random.default_rng(SEED)
    meshes = [np.array([[[-0.15, -0.1, 0.0], [0.15, -0.1, 0.0], [0.0, 0.2, 0.0]]]), box_mesh(0.06, 0.08, 0.1),
              uv_sphere(0.1, seg=6, rings=4), np.zeros((0, 3, 3))]
    tri, start = pack(meshes)
    assert len(tri) == 49
    templates = np.array([[rigid(random_rotation(rng), rng.uniform(-0.12, 0.12, 3)) for _ in meshes] for _ in range(K)])
    return frozen(tri, start, templates)


def tiled_poses(P, templates=None):
    """link_T (P,L,4,4) with link_T[p] = template[p % 7]."""
    templates = scene()[2] if templates is None else templates
    return templates[np.arange(P) % K]


def tiled(rows, n):
    """rows[i % len(rows)] for i < n along the first axis: what a long call must return, from the short call's rows."""
    return rows[np.arange(n) % len(rows)]


def loose(start, n, ends=LOOSE):
    """A copy of the start table with its two ends outside 0 .. n: the header promises they are clamped."""
    out = np.array(start)
    out[0], out[-1] = ends[0], n + ends[1]
    return out


# ------------------------------------------------------------------------------------------ the pair list
VALID = all_pairs(4)                                             # (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); link 3 is the empty one
BASE_PAIRS = np.array([tuple(p) for p in VALID] + [(1, 0), (3, 2), (-1, 1), (2, 2), (1, 3)], np.int32)
NOT_EVALUATED = np.array([not (0 <= a < 4 and 0 <= b < 4) or a == b or 3 in (a, b) for a, b in BASE_PAIRS])   # invalid, same link, empty link
assert len(BASE_PAIRS) == 11 and NOT_EVALUATED.sum() == 7 and not NOT_EVALUATED[[0, 1, 3, 6]].any()


def tiled_pairs(M):
    """pairs (M,2) int32 with pairs[m] = BASE_PAIRS[m % 11]; invalid entries among them: through the C ABI only."""
    return np.ascontiguousarray(BASE_PAIRS[np.arange(M) % len(BASE_PAIRS)])


# ------------------------------------------------------------------------------------------ the point clouds of the point queries
@functools.lru_cache(maxsize=None)
def clouds():
    """pts (140,3), pt_start (8) of the seven templates' clouds: uniform in the scene's box grown by 0.05, one NaN point in every
    template with at least 3 points."""
    tri, start, templates = scene()
    rng = np.random.default_rng(CLOUD_SEED)
    W = np.concatenate([pref.posed_mesh(tri, start, T).reshape(-1, 3) for T in templates])
    lo, hi = W.min(0) - 0.05, W.max(0) + 0.05
    pts = []
    for n in CLOUD_SIZES:
        x = rng.uniform(lo, hi, (n, 3))
        if n >= 3:
            x[n // 2, n % 3] = np.nan
        pts.append(x)
    return frozen(np.concatenate(pts), np.concatenate([[0], np.cumsum(CLOUD_SIZES)]).astype(np.int64))


def tiled_cloud(P):
    """pts, pt_start (P+1) of the long call -- pose p owns a copy of template p % 7's cloud -- and ``src`` (n_pts): the row of
    clouds()' pts that each long row copies."""
    pts, cut = clouds()
    sizes = np.asarray(CLOUD_SIZES)[np.arange(P) % K]
    pt_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    per_cycle = np.arange(int(cut[-1]))
    src = np.concatenate([np.tile(per_cycle, P // K), per_cycle[:int(cut[P % K])]])
    assert len(src) == pt_start[-1]
    return pts[src], pt_start, src


def cloud_diagonal():
    tri, start, templates = scene()
    return pref.scene_diagonal(tri, start, templates, clouds()[0])


def point_ambiguous(d_max, tol2):
    """(140) bool, the point direction of _mesh_cover_ref.ambiguous: the live points with a restated d2 within tol2 of d_max^2.
    (Its runner-up clause has no twin here: neighbouring triangles tie exactly along an edge, and the point-mesh check compares
    the chosen row by its restated d2, not by its number.)"""
    tri, start, templates = scene()
    pts, cut = clouds()
    dmax2 = np.float64(d_max) * np.float64(d_max)
    out = np.zeros(len(pts), bool)
    if not np.isfinite(dmax2):
        return out
    for p, T in enumerate(templates):
        s, e = int(cut[p]), int(cut[p + 1])
        full = mcref.gated_matrix(pref.posed_mesh(tri, start, T), pts[s:e], dmax2)
        out[s:e] = (np.isfinite(full) & (np.abs(full - dmax2) <= tol2)).any(1)
    return out


# ------------------------------------------------------------------------------------------ the containment scene
CONTAIN_Q = 9
INNER_OFFSETS = ((0.0, 0.0, 0.0), (0.04, -0.03, 0.02), (0.3, 0.0, 0.0), (0.0, -0.26, 0.1), (-0.03, 0.04, -0.04), (0.093, 0.004, -0.003),
                 (0.0, 0.0, 0.19))                               # link 1 in link 0's frame: inside, inside, far, far, inside, across a face, outside but in the box's reach


@functools.lru_cache(maxsize=None)
def contain_scene():
    """tri (36,3,3), tri_start (5), pts (27,3), pt_start (5), templates (7,4,4,4): _contain_ref.nested_cubes with a fourth, empty
    link without points, the small cube (link 1) placed by INNER_OFFSETS in the large one's frame (wholly inside it in three
    templates, not inside in four) and a middle cube (link 2, half 0.05) that wanders through the large one's wall."""
    rng = np.random.default_rng(CONTAIN_SEED)
    tri, start = pack([box_mesh(0.1, 0.1, 0.1), box_mesh(0.02, 0.02, 0.02), box_mesh(0.05, 0.05, 0.05), np.zeros((0, 3, 3))])
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    pts = np.concatenate([np.concatenate([0.9 * h * corners, np.zeros((1, 3))]) for h in (0.1, 0.02, 0.05)])
    pt_start = np.array([0, 9, 18, 27, 27], np.int64)
    templates = []
    for off in INNER_OFFSETS:
        G = rigid(random_rotation(rng), rng.uniform(-0.2, 0.2, 3))
        templates.append([G, G @ rigid(random_rotation(rng), off), G @ rigid(random_rotation(rng), rng.uniform(-0.12, 0.12, 3)),
                          rigid(random_rotation(rng), rng.uniform(-0.1, 0.1, 3))])
    return frozen(tri, start, pts, pt_start, np.array(templates))


# ------------------------------------------------------------------------------------------ the restatements, once
@functools.lru_cache(maxsize=None)
def want_collide(base=False):
    """The restatement on the 7 templates with the 6 valid pairs, or (``base``) with the 11 base pairs."""
    tri, start, templates = scene()
    return frozen(*mesh_collide(tri, start, templates, BASE_PAIRS if base else VALID))


@functools.lru_cache(maxsize=None)
def want_clearance(base=False):
    tri, start, templates = scene()
    return frozen(*clref.mesh_clearance(tri, start, templates, BASE_PAIRS if base else VALID, D_MAX, runner_up=True))


@functools.lru_cache(maxsize=None)
def want_point_mesh(d_max):
    tri, start, templates = scene()
    return frozen(*pref.point_mesh(tri, start, templates, *clouds(), d_max))


@functools.lru_cache(maxsize=None)
def want_mesh_cover(d_max=D_MAX):
    tri, start, templates = scene()
    return frozen(*mcref.mesh_cover(tri, start, templates, *clouds(), d_max))


@functools.lru_cache(maxsize=None)
def want_contain(base=False):
    """inside, first, winding, link_box, long-double winding and sum|omega| / (4 pi) on the containment scene's 7 templates."""
    tri, start, pts, pt_start, templates = contain_scene()
    return frozen(*conref.mesh_contain(tri, start, pts, pt_start, templates, BASE_PAIRS if base else VALID, CONTAIN_Q, truth=True))


def differing_templates(rows, shifts=(SLICE % 11,)):
    """Two templates for the pair slice's P = 2 from their (7, 11, ...) base-pair rows: each answers differently from itself rolled
    by every shift (a launch that lost m0 answers for base pair y where y + shift belongs), and the two answer differently."""
    ok = [t for t in range(K) if all(np.roll(rows[t], -s, 0).tobytes() != rows[t].tobytes() for s in shifts)]
    for t in ok[1:]:
        if rows[t].tobytes() != rows[ok[0]].tobytes():
            return [ok[0], t]
    raise AssertionError("no two templates whose base-pair answers differ")


CONTAIN_SHIFTS = (HALF_SLICE % 11, 2 * HALF_SLICE % 11)         # 9 and 7: the heads of contain's second and third launch
