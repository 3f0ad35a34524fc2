"""The conditions the launch-slice suite (tests/test_gpu_mesh_slices.py) leans on, checked on the numpy restatements alone (no GPU):
the seven templates give answers that differ from template to template and from pair to pair, so a row computed from the wrong
pose or pair shows; the long batches put another template and another base pair at the head of every later launch; the new
lattice cases count what the contract says."""
import numpy as np
import pytest

import _clearance_ref as clref
import _collide_ref as ref
import _mesh_cover_ref as mcref
import _mesh_slices as ms

PAIRED = [0, 1, 3]                                               # the rows of VALID without the empty link: (0,1) (0,2) (1,2)


def test_collide_outcomes_over_the_templates():
    """Every pair of non-empty links has both outcomes over the templates or is pinned as always / never colliding; at least two
    have both, every pair with the empty link has none."""
    count, first, _ = ms.want_collide()
    hits = (count > 0).sum(0)
    assert ms.VALID[PAIRED].tolist() == [[0, 1], [0, 2], [1, 2]]
    assert hits.tolist() == [4, 2, 0, 4, 0, 0]                   # the empty link never
    assert ((hits[PAIRED] > 0) & (hits[PAIRED] < ms.K)).sum() >= 2
    assert ((first == -1).all(-1) == (count == 0)).all()
    assert len({count[t].tobytes() + first[t].tobytes() for t in range(ms.K)}) == ms.K       # no two templates answer alike


def test_clearance_has_zeros_positives_infinities_and_unique_minima():
    tri, start, templates = ms.scene()
    d2, wit, _, second = ms.want_clearance()
    pos = np.isfinite(d2) & (d2 > 0)
    assert ((d2 == 0).sum(), pos.sum(), np.isinf(d2).sum()) == (10, 10, 22)
    assert np.isinf(d2[:, PAIRED]).sum() == 1                    # one pair of non-empty links beyond d_max, 21 cells with the empty link
    bound = 1e-12 * clref.scene_diagonal(tri, start, templates)
    with np.errstate(invalid="ignore"):
        unique = pos & (np.sqrt(second) - np.sqrt(d2) > bound)
    assert unique.sum() >= 3                                     # the GPU check compares the witnesses there
    assert len({d2[t].tobytes() + wit[t].tobytes() for t in range(ms.K)}) == ms.K


def test_point_queries_are_unambiguous_on_the_templates():
    tri, start, templates = ms.scene()
    pts, cut = ms.clouds()
    assert np.diff(cut).tolist() == list(ms.CLOUD_SIZES) and np.isnan(pts).any(1).sum() == 4
    tol2 = 1e-12 * ms.cloud_diagonal() ** 2
    assert mcref.ambiguous(tri, start, templates, pts, cut, ms.D_MAX, tol2).mean() <= 0.01
    for d_max in (ms.D_MAX, np.inf):
        assert ms.point_ambiguous(d_max, tol2).mean() <= 0.01
    near, far = ms.want_point_mesh(ms.D_MAX), ms.want_point_mesh(np.inf)
    assert 20 <= np.isfinite(near[0]).sum() < np.isfinite(far[0]).sum() == len(pts) - 4           # d_max cuts; only the NaN points miss at +inf
    cover = ms.want_mesh_cover()
    assert np.isinf(cover[0][0]).all() and np.isfinite(cover[0][[2, 4]]).any(1).all()            # template 0 has no points, 2 and 4 a tile's worth
    assert (cover[2] > 0).sum() >= 20


def test_contain_scene_decides_far_from_a_half_and_has_both_outcomes():
    inside, first, wind, _, _, mag = ms.want_contain()
    evaluated = mag > 0
    assert evaluated.sum() >= 50 and (np.abs(np.abs(wind[evaluated]) - 0.5) > 1e-3).all()
    small_in_large = inside[:, 0, 1]                             # pair (0,1), direction 1: link 1's points against link 0
    assert ms.VALID[0].tolist() == [0, 1]
    assert (small_in_large == ms.CONTAIN_Q).sum() >= 2 and (small_in_large < ms.CONTAIN_Q).sum() >= 2
    assert (inside[:, [2, 4, 5]] == 0).all() and (first[:, [2, 4, 5]] == -1).all()               # the empty link, either way round
    assert len({wind[t].tobytes() for t in range(ms.K)}) == ms.K
    pts, pt_start = ms.contain_scene()[2:4]
    assert np.diff(pt_start).max() <= ms.CONTAIN_Q <= 16


def test_the_head_of_every_later_launch_is_not_template_or_pair_zero():
    _, _, templates = ms.scene()
    assert ms.P_LONG == ms.M_LONG == 65544 and ms.SLICE % ms.K == 1 and ms.SLICE % 11 == 8 and ms.HALF_SLICE % 11 == 9
    link_T = ms.tiled_poses(ms.P_LONG)
    assert link_T.shape == (65544, 4, 4, 4) and link_T[ms.SLICE].tobytes() == templates[1].tobytes() != templates[0].tobytes()
    assert {p % ms.K for p in range(ms.SLICE, ms.P_LONG)} == set(range(ms.K))                    # every template in the second slice
    pairs = ms.tiled_pairs(ms.M_LONG)
    assert pairs.dtype == np.int32 and pairs.shape == (65544, 2)
    assert pairs[ms.SLICE].tolist() == ms.BASE_PAIRS[8].tolist() and pairs[ms.HALF_SLICE].tolist() == ms.BASE_PAIRS[9].tolist()
    assert pairs[2 * ms.HALF_SLICE].tolist() == ms.BASE_PAIRS[7].tolist()                        # contain's third launch
    assert ms.BASE_PAIRS[:6].tolist() == ref.all_pairs(4).tolist()
    assert ms.BASE_PAIRS[6:].tolist() == [[1, 0], [3, 2], [-1, 1], [2, 2], [1, 3]]
    pts, pt_start, src = ms.tiled_cloud(ms.P_LONG)
    assert len(pts) == 9363 * 140 + 66 and pt_start[ms.SLICE] == 9362 * 140 and (np.diff(pt_start[ms.SLICE:]) == [1, 65, 2, 64, 3, 5, 0, 1, 65]).all()
    cut = ms.clouds()[1]
    assert (src[pt_start[ms.SLICE + 1]:pt_start[ms.SLICE + 2]] == np.arange(cut[2], cut[3])).all()
    loose = ms.loose(ms.scene()[1], 49)
    assert loose.tolist() == [-5, 1, 13, 49, 56] and np.clip(loose, 0, 49).tolist() == ms.scene()[1].tolist()


def test_the_base_pairs_answer_differently_on_the_two_templates_of_the_pair_slice():
    """The pair slice runs P = 2 on two templates that answer differently, each also differently from itself with the base pairs
    rolled by 8 (contain: 9 and 7): what a launch that lost m0 would return."""
    count, first, _ = ms.want_collide(base=True)
    assert (count[:, ms.NOT_EVALUATED] == 0).all() and (first[:, ms.NOT_EVALUATED] == -1).all()
    assert (count[:, 6] == count[:, 0]).all() and (first[:, 6] == first[:, 0, ::-1]).all()      # (1,0) is (0,1) with the rows swapped
    d2 = ms.want_clearance(base=True)[0]
    assert np.isinf(d2[:, ms.NOT_EVALUATED]).all()
    inside, _, wind = ms.want_contain(base=True)[:3]
    assert (inside[:, ms.NOT_EVALUATED] == 0).all() and (wind[:, ms.NOT_EVALUATED] == 0.0).all()
    assert ms.CONTAIN_SHIFTS == (9, 7)
    for rows, shifts in ((count, (8,)), (d2, (8,)), (wind, ms.CONTAIN_SHIFTS)):
        a, b = ms.differing_templates(rows, shifts)
        assert a != b and rows[a].tobytes() != rows[b].tobytes()
        for t in (a, b):
            assert all(np.roll(rows[t], -s, 0).tobytes() != rows[t].tobytes() for s in shifts)


@pytest.mark.parametrize("name", ["identical", "shared_edge", "shared_vertex", "point_on_face", "collinear_piercing", "two_edges_pierce"])
def test_the_new_lattice_counts(name):
    other, want = ref.LATTICE[name]
    assert want == {"collinear_piercing": 1, "two_edges_pierce": 1}.get(name, 0)
    A, B = np.array([ref.BASE], np.float64), np.array([other], np.float64)
    assert len(ref.colliding_pairs(A, B)[0]) == want and len(ref.colliding_pairs(B, A)[0]) == want
