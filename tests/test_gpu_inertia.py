"""GPU: mass properties of link meshes (inertia.hip through ops and the C ABI; DESIGN N4) against tests/_inertia_ref.py --
the raw sums within creg.h's k roundings of their exact values, the derived outputs against the restatement evaluated on
the kernel's own sums, bits that do not depend on the other links of a call or on the run, sentinel-guarded buffers, open and inward
meshes, a link of more than 65536 facets, a box far from the origin, the mesher's output, and the coord_map command line with --density end to end.  Measured maxima are
printed before each assertion (run with -s to see them)."""
import ctypes
import json
import math
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _inertia_ref as I  # noqa: E402

EPS = 2.0 ** -52
DERIVED = 16 * EPS                                                   # per operation chain, relative to the output's largest entry
KEYS = ("sums", "volume", "area", "closure", "mass", "com", "inertia", "principal", "axes")
SIZES = (4, 12, 20, 254, 256, 258, 510, 512, 514, 1280, 0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def ops():
    from autourdf_amd import ops as o
    return o


def mixed_links():
    """Links of SIZES facets, link-sized, 0.3 .. 0.5 from the origin, vertices rounded to float32."""
    meshes = [I.tetrahedron((0, 0, 0), (0.06, 0.01, 0), (0.01, 0.05, 0.01), (0.02, 0.01, 0.07)), I.box(0.05, 0.03, 0.08),
              I.icosphere(0, (0.04, 0.03, 0.05))]
    meshes += [I.bipyramid(n, 0.04 + 0.0001 * n, 0.03) for n in (127, 128, 129, 255, 256, 257)]
    meshes.append(I.icosphere(3, (0.05, 0.03, 0.08)))
    rng = np.random.default_rng(7)
    tris = []
    for m in meshes:
        shift = rng.uniform(0.3, 0.5, 3) * rng.choice([-1.0, 1.0], 3)
        tris.append(I.triangles(m, shift=shift, f32=True))
    tris.append(np.zeros((0, 3, 3)))
    assert tuple(len(t) for t in tris) == SIZES
    return tris


@pytest.fixture(scope="module")
def mixed(dev):
    """The links, their exact sums (computed once) and the mixed call's outputs."""
    tris = mixed_links()
    exact = [I.exact_sums(t) for t in tris]
    tri, start = I.pack(tris)
    density = np.linspace(800.0, 2700.0, len(tris))
    out = ops().mesh_inertia(torch.from_numpy(tri).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(density).to(dev))
    return dict(tris=tris, exact=exact, tri=tri, start=start, density=density, out=out)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def check_sums(S, tri, exact=None):
    """max over the 14 sums of |got - exact| / (2^-53 sum|term|), asserted against creg.h's k."""
    tot, tot_abs = exact if exact is not None else I.exact_sums(tri)
    worst = 0.0
    for k in range(I.N_TERMS):
        err = abs(I.Fraction(float(S[k])) - tot[k])
        if tot_abs[k] > 0:
            worst = max(worst, float(err / (tot_abs[k] * I.Fraction(I.U))))
        else:
            assert err == 0
    return worst


def check_derived(got, S, r, density, tag):
    """One link's derived outputs against the restatement evaluated on the kernel's own sums S."""
    want = I.derive(S, r, density)
    worst = {}
    for k in ("volume", "area", "closure", "mass", "com", "inertia", "principal"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        scale = abs(float(w)) if k == "closure" else float(np.max(np.abs(w)))
        if scale > 0:
            worst[k] = float(np.max(np.abs(g - w))) / scale / EPS
        else:                                                        # a restated zero is exact: 0 here, anything else fails below
            worst[k] = 0.0 if (g == w).all() else float("inf")
    J, w, V = I.full(got["inertia"]), np.asarray(got["principal"]), np.asarray(got["axes"])
    lam = float(np.max(np.abs(w)))
    worst["axes residual"] = float(np.max(np.abs(J @ V.T - V.T * w))) / lam / EPS
    worst["axes orthonormal"] = float(np.max(np.abs(V @ V.T - np.eye(3)))) / EPS
    print(f"{tag}: derived outputs, max error in 2^-52 of the output's largest entry: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= DERIVED / EPS, (tag, k, v)
    assert (np.diff(w) >= 0).all() and np.linalg.det(V) > 0
    return worst


# ------------------------------------------------------------------------------------------------ one call, mixed links
def test_mixed_links_sums_within_k_roundings_and_derived_outputs(mixed):
    out = {k: v.cpu().numpy() for k, v in mixed["out"].items()}
    assert sorted(out) == sorted(KEYS)
    L = len(SIZES)
    assert out["sums"].shape == (L, 14) and out["com"].shape == (L, 3) and out["inertia"].shape == (L, 6)
    assert out["principal"].shape == (L, 3) and out["axes"].shape == (L, 3, 3) and out["volume"].shape == (L,)
    for l, tri in enumerate(mixed["tris"][:-1]):
        F = len(tri)
        worst = check_sums(out["sums"][l], tri, mixed["exact"][l])
        same = bool((out["sums"][l] == I.link_sums(tri)).all())
        print(f"link {l} F={F}: max |sum - exact| / (2^-53 sum|term|) = {worst:.3f}, k = {I.k_bound(F)}; "
              f"sums bit-equal to the restated tree: {same}")
        assert worst <= I.k_bound(F) <= 32 + math.ceil(math.log2(F))
        check_derived({k: out[k][l] for k in KEYS}, out["sums"][l], tri[0, 0], mixed["density"][l], f"link {l} F={F}")
        assert out["volume"][l] > 0 and out["mass"][l] > 0
    e = L - 1                                                        # the empty link: zeros and NaNs
    assert (out["sums"][e] == 0).all() and out["volume"][e] == 0 and out["area"][e] == 0 and out["closure"][e] == 0
    assert out["mass"][e] == 0
    for k in ("com", "inertia", "principal", "axes"):
        assert np.isnan(out[k][e]).all(), k


def test_every_link_alone_gives_the_bits_of_the_mixed_call(dev, mixed):
    for l, tri in enumerate(mixed["tris"]):
        t, s = I.pack([tri])
        alone = ops().mesh_inertia(torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev), float(mixed["density"][l]))
        for k in KEYS:
            assert same_bits(alone[k][0], mixed["out"][k][l]), (l, len(tri), k)
    # and in another place of another call: behind links that move its first triangle off a multiple of 256
    order = [9, 10, 3, 0, 6, 10, 1]
    t, s = I.pack([mixed["tris"][i] for i in order])
    again = ops().mesh_inertia(torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev),
                               torch.from_numpy(mixed["density"][order].copy()).to(dev))
    for at, l in enumerate(order):
        for k in KEYS:
            assert same_bits(again[k][at], mixed["out"][k][l]), (at, l, k)


def test_two_runs_give_the_same_bits(dev, mixed):
    again = ops().mesh_inertia(torch.from_numpy(mixed["tri"]).to(dev), torch.from_numpy(mixed["start"]).to(dev),
                               torch.from_numpy(mixed["density"]).to(dev))
    for k in KEYS:
        assert same_bits(again[k], mixed["out"][k]), k


def test_density_forms_and_refusals(dev, mixed):
    o = ops()
    tri, start = torch.from_numpy(mixed["tri"]).to(dev), torch.from_numpy(mixed["start"]).to(dev)
    L = len(SIZES)
    a = o.mesh_inertia(tri, start)                                   # density 1: mass is the volume
    assert torch.equal(a["mass"], a["volume"])
    b = o.mesh_inertia(tri, start, np.full(L, 1.0))
    for k in KEYS:
        assert same_bits(a[k], b[k])
    with pytest.raises(ValueError, match="density"):
        o.mesh_inertia(tri, start, np.ones(L + 1))
    with pytest.raises(ValueError, match="tri"):
        o.mesh_inertia(tri.reshape(-1, 9), start)
    with pytest.raises(ValueError, match="tri_start"):
        o.mesh_inertia(tri, start[:1])
    with pytest.raises(TypeError):
        o.mesh_inertia(tri.float(), start)
    with pytest.raises(TypeError):
        o.mesh_inertia(tri, start.int())
    with pytest.raises(RuntimeError):
        o.mesh_inertia(tri.cpu(), start)


def test_nothing_is_written_outside_the_buffers(dev, mixed):
    """The C ABI on sentinel-filled outputs with spare rows behind each, and a workspace with spare bytes behind it."""
    from autourdf_amd import _lib
    L_ = _lib.load()
    tri, start = torch.from_numpy(mixed["tri"]).to(dev), torch.from_numpy(mixed["start"]).to(dev)
    density = torch.from_numpy(mixed["density"]).to(dev)
    F, L, PAD, SENT = tri.shape[0], len(SIZES), 64, -7e30
    shapes = dict(sums=(14,), volume=(), area=(), closure=(), mass=(), com=(3,), inertia=(6,), principal=(3,), axes=(3, 3))
    bufs = {k: torch.full((L + PAD,) + shapes[k], SENT, dtype=torch.float64, device=dev) for k in KEYS}
    wsb = int(L_.creg_mesh_inertia_workspace_bytes(F, L))
    assert wsb % 8 == 0
    ws = torch.full((wsb // 8 + PAD,), SENT, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda n_tri, n_links, nbytes: L_.creg_mesh_inertia_f64(p(tri), p(start), n_tri, n_links, p(density), *[p(bufs[k]) for k in KEYS],
                                                                   p(ws), nbytes, st)
    # refusals launch nothing
    assert call(F, L, wsb - 8) == -1 and b"workspace" in L_.creg_last_error()
    assert call(F, 0, wsb) == -1 and call(-1, L, wsb) == -1 and call(F, 65536, wsb) == -1 and call(1 << 31, L, wsb) == -1
    torch.cuda.synchronize()
    assert all((b == SENT).all() for b in bufs.values()) and (ws == SENT).all()
    assert call(F, L, wsb) == 0
    torch.cuda.synchronize()
    assert (ws[wsb // 8:] == SENT).all()
    for k in KEYS:
        assert (bufs[k][L:] == SENT).all(), k
        assert not (bufs[k][:L] == SENT).any(), k                    # every row is written, the empty link's too
        assert same_bits(bufs[k][:L], mixed["out"][k]), k


# ------------------------------------------------------------------------------------------------ open, inward, large
def test_open_and_inward_meshes_report_their_closure_and_volume(dev):
    """A box without one facet, a sphere without one of 1280 and a box turned inside out: closure is about the missing
    facet's share of the area (far above rounding), the inward volume is negative, all as the restatement says."""
    shift = (0.35, -0.41, 0.46)
    box = I.triangles(I.box(0.05, 0.03, 0.08), shift=shift, f32=True)
    ico = I.triangles(I.icosphere(3, (0.05, 0.03, 0.08)), shift=shift, f32=True)
    tris = [box[:-1], ico[1:], box[:, ::-1].copy(), box]
    tri, start = I.pack(tris)
    out = {k: v.cpu().numpy() for k, v in ops().mesh_inertia(torch.from_numpy(tri).to(dev), torch.from_numpy(start).to(dev), 1500.0).items()}
    for l, t in enumerate(tris):
        worst = check_sums(out["sums"][l], t)
        print(f"link {l} F={len(t)}: max |sum - exact| / (2^-53 sum|term|) = {worst:.3f}, k = {I.k_bound(len(t))}; closure {out['closure'][l]:.6e}")
        assert worst <= I.k_bound(len(t))
        check_derived({k: out[k][l] for k in KEYS}, out["sums"][l], t[0, 0], 1500.0, f"link {l} F={len(t)}")
    # the missing facet's area vector is what is left of sum n: half of |n| of that facet over the remaining area
    for l, (whole, gone) in enumerate(((box, box[-1]), (ico, ico[0]))):
        n = np.cross(gone[1] - gone[0], gone[2] - gone[0])
        want = np.linalg.norm(n) / 2 / out["area"][l]
        # sum n is within k roundings of sum |n| per component, and closure is already relative to sum |n|
        assert abs(out["closure"][l] - want) <= (math.sqrt(3) * I.k_bound(len(whole)) + 8) * I.U and out["closure"][l] > 1e-4
    assert out["closure"][2] <= math.sqrt(3) * 26 * I.U and out["closure"][3] <= math.sqrt(3) * 26 * I.U
    # every d of a convex body seen from one of its vertices has one sign: each volume is within k roundings of itself
    assert out["volume"][2] < 0 and abs(out["volume"][2] + out["volume"][3]) <= 2 * 26 * I.U * out["volume"][3] and out["mass"][2] < 0


def test_a_link_of_more_than_65536_triangles_between_small_ones(dev):
    """81 920 facets = 320 chunks: blocks of the chunk pass make a second trip (the grid holds 128), and the finishing pass
    reduces two groups of partials in place before its last level.  The bits are the restated tree's, alone or not."""
    big = I.triangles(I.icosphere(6, (0.05, 0.03, 0.08)), shift=(0.35, -0.41, 0.46), f32=True)
    small = I.triangles(I.box(0.05, 0.03, 0.08), shift=(-0.3, 0.4, 0.5), f32=True)
    assert len(big) == 81920 and I.k_bound(len(big)) == 35
    tri, start = I.pack([small, big, small])
    rho = np.array([900.0, 1100.0, 1300.0])
    dev_out = ops().mesh_inertia(torch.from_numpy(tri).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(rho).to(dev))
    out = {k: v.cpu().numpy() for k, v in dev_out.items()}
    want = I.link_sums(big)
    check_against_restated_sums(out["sums"][1], big, "81920 facets")
    same = bool((out["sums"][1] == want).all())
    print(f"81920 facets: sums bit-equal to the restated tree: {same}; closure {out['closure'][1]:.3e}, volume {out['volume'][1]:.6e}")
    assert same
    check_derived({k: out[k][1] for k in KEYS}, out["sums"][1], big[0, 0], rho[1], "81920 facets")
    assert (out["sums"][0] == I.link_sums(small)).all() and (out["sums"][2] == out["sums"][0]).all()
    # a stretched sphere of these radii: the volume of the inscribed polyhedron is just below the ellipsoid's
    ell = 4 / 3 * np.pi * 0.05 * 0.03 * 0.08
    assert 0.999 * ell < out["volume"][1] < ell and out["closure"][1] <= math.sqrt(3) * 35 * I.U
    t, s = I.pack([big])
    alone = ops().mesh_inertia(torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev), float(rho[1]))
    again = ops().mesh_inertia(torch.from_numpy(tri).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(rho).to(dev))
    for k in KEYS:
        assert same_bits(alone[k][0], dev_out[k][1]), k
        assert same_bits(again[k], dev_out[k]), k


# ------------------------------------------------------------------------------------------------ far from the origin
def test_a_box_1000_units_away_has_the_inertia_of_the_box_at_the_origin(dev):
    """Edges and offsets are binary fractions, so every vertex is exact in both places: only the reference point keeps the
    sums from cancelling 1000^2-sized second moments."""
    near = I.triangles(I.box(0.25, 0.5, 0.125))
    shift = np.array([1000.0, -1000.0, 1000.0])
    far = near + shift
    assert ((far - shift) == near).all()
    tri, start = I.pack([near, far])
    out = {k: v.cpu().numpy() for k, v in ops().mesh_inertia(torch.from_numpy(tri).to(dev), torch.from_numpy(start).to(dev), 1000.0).items()}
    scale = np.abs(out["inertia"][0]).max()
    err = np.abs(out["inertia"][1] - out["inertia"][0]).max() / scale
    cerr = np.abs((out["com"][1] - shift) - out["com"][0]).max() / 1000.0
    print(f"box at 1000: inertia differs by {err / EPS:.2f} x 2^-52 of its largest entry, com by {cerr / EPS:.2f} x 2^-52 of 1000")
    assert err <= DERIVED and cerr <= DERIVED
    m = 1000.0 * 0.25 * 0.5 * 0.125
    want = np.array([m / 12 * (0.5 ** 2 + 0.125 ** 2), 0, 0, m / 12 * (0.25 ** 2 + 0.125 ** 2), 0, m / 12 * (0.25 ** 2 + 0.5 ** 2)])
    np.testing.assert_allclose(out["inertia"][1], want, rtol=0, atol=(I.k_bound(12) + 16) * EPS * want.max())
    np.testing.assert_allclose(out["volume"], 0.25 * 0.5 * 0.125, rtol=DERIVED)


# ------------------------------------------------------------------------------------------------ the mesher
def capsule(n, seed, radius=0.03, length=0.12):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-length / 2, length / 2, n)
    th = rng.uniform(0, 2 * np.pi, n)
    p = np.stack([radius * np.cos(th), radius * np.sin(th), z], 1) + rng.normal(scale=5e-4, size=(n, 3))
    return p.astype(np.float32).astype(np.float64) + np.array([0.4, -0.3, 0.35])


def check_against_restated_sums(S, tri, tag):
    """Kernel sums against the restatement's on the same triangles: both are within k roundings of the exact sums."""
    t = I.terms(tri)
    ref, tot_abs = I.tree_sum(t), np.abs(t).sum(0)
    k = I.k_bound(len(tri))
    worst = float(np.max(np.abs(S - ref) / (I.U * tot_abs)))
    print(f"{tag}: F={len(tri)}, max |sum - restated sum| / (2^-53 sum|term|) = {worst:.3f}, allowed 2 k = {2 * k}")
    assert worst <= 2 * k


def test_meshes_of_the_mesher(dev):
    clouds = [capsule(3000, 1), capsule(1200, 2, 0.02, 0.07)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    meshes = ops().voxel_mesh(torch.from_numpy(np.concatenate(clouds)).to(dev), torch.from_numpy(off).to(dev), 0.01, smooth=True)
    tris = [m["vertices"][m["triangles"].long()] for m in meshes]
    start = torch.tensor(np.concatenate([[0], np.cumsum([len(t) for t in tris])]), dtype=torch.int64, device=dev)
    out = {k: v.cpu().numpy() for k, v in ops().mesh_inertia(torch.cat(tris).contiguous(), start, 1100.0).items()}
    for l, t in enumerate(tris):
        t = t.cpu().numpy()
        check_against_restated_sums(out["sums"][l], t, f"mesher link {l}")
        check_derived({k: out[k][l] for k in KEYS}, out["sums"][l], t[0, 0], 1100.0, f"mesher link {l}")
        print(f"mesher link {l}: volume {out['volume'][l]:.6e}, closure {out['closure'][l]:.3e}")
        assert out["volume"][l] > 0 and out["closure"][l] <= math.sqrt(3) * I.k_bound(len(t)) * I.U
        lam = out["principal"][l]
        assert lam[0] > 0 and lam[0] + lam[1] >= lam[2]


# ------------------------------------------------------------------------------------------------ end to end
def _registration_fixture(golden, tmp_path, params):
    """The set-up of test_gpu_link_mesh.py's command-line test: the golden registration as the files coord_map reads."""
    from _ply import write_ascii_ply
    u = golden("urdf_reference.npz")
    M = u["a.matrices"]                                                        # (2,10,20,4,4), six links
    S, T, K = M.shape[:3]
    robot, cams, step = "testbot", 20, 4
    (tmp_path / "parameters.json").write_text(json.dumps({robot: dict({"num_seg": K, "dof": 5}, **params)}))
    rng = np.random.default_rng(0)
    for s in range(S):
        part = tmp_path / f"data/part/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq{s}"
        (part / "matrix").mkdir(parents=True)
        (part / "cluster").mkdir()
        for t in range(T):
            np.save(part / f"matrix/{t:04}.npy", M[s, t] if t == 0 else M[s, t].astype(np.float32))
            np.savez(part / f"cluster/{t:04}.npz", **{str(k): rng.normal(scale=0.02, size=(16, 3)).astype(np.float32)
                                                     for k in range(K)})
            raw = tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams/seq{s}/{t:04}"
            raw.mkdir(parents=True)
            a = 0.9 / (2 * math.sqrt(3))
            write_ascii_ply(str(raw / "robot.ply"), np.vstack([rng.uniform(-a, a, size=(62, 3)), [[-a] * 3, [a] * 3]]))
    return robot, K, step, cams


def _run(tmp_path, *options):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "autourdf_amd.coord_map", "--robot", "testbot", "--unknown_dof", "--end_video", "2",
                           *options], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)


def _inertials(root):
    num = lambda s: np.array(s.split(), np.float64)
    out = {}
    for link in root.findall("link"):
        i = link.find("inertial")
        out[link.get("name")] = dict(xyz=num(i.find("origin").get("xyz")), rpy=i.find("origin").get("rpy"), mass=i.find("mass").get("value"),
                                     inertia=[i.find("inertia").get(k) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")],
                                     visual=num(link.find("visual/origin").get("xyz")), mesh=link.find("visual/geometry/mesh").get("filename"))
    return out


def test_command_line_with_a_density_fills_the_inertial_blocks(dev, golden, tmp_path):
    from autourdf_amd import link
    # parameters.json asks for another density; the option on the command line wins
    robot, K, step, cams = _registration_fixture(golden, tmp_path, {"density": 5.0})
    rho = 1250.0
    r = _run(tmp_path, "--voxel_size", "0.01", "--density", str(rho))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    urdf = tmp_path / f"data/urdf/{robot}_{K}_seg/{step}_deg_{cams}_cams.urdf"
    mesh_dir = tmp_path / f"data/mesh/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq0"
    blocks = _inertials(ET.parse(urdf).getroot())
    assert len(blocks) == 6
    saved = json.load(open(mesh_dir / "inertial.json"))
    assert sorted(saved) == sorted(blocks)
    for name, b in sorted(blocks.items()):
        tri = link.read_stl(str(tmp_path / b["mesh"]))[:, 1:4].astype(np.float64)
        t, s = I.pack([tri])
        out = {k: v.cpu().numpy()[0] for k, v in ops().mesh_inertia(torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev), rho).items()}
        check_against_restated_sums(out["sums"], tri, name)
        same = bool((out["sums"] == I.link_sums(tri)).all())
        print(f"{name}: sums of the file's triangles bit-equal to the restated tree: {same}")
        want = I.derive(I.link_sums(tri), tri[0, 0], rho)            # the restatement alone, on the file's triangles
        got_J = np.array([float(x) for x in b["inertia"]])
        errs = (abs(float(b["mass"]) - want["mass"]) / want["mass"], np.abs(got_J - want["inertia"]).max() / np.abs(want["inertia"]).max(),
                np.abs(b["xyz"] - (want["com"] + b["visual"])).max() / np.abs(want["com"] + b["visual"]).max())
        print(f"{name}: F={len(tri)} mass {float(b['mass']):.6e}; URDF against the restatement, in 2^-52: mass {errs[0] / EPS:.2f}, "
              f"inertia {errs[1] / EPS:.2f}, origin {errs[2] / EPS:.2f}")
        assert max(errs) <= DERIVED and b["rpy"] == "0.0 0.0 0.0"
        assert float(b["mass"]) > 0 and saved[name]["mass"] == float(b["mass"])
        lam = np.linalg.eigvalsh(I.full(got_J))
        assert lam[0] > 0 and lam[0] + lam[1] >= lam[2] * (1 - DERIVED)
    # without a density the inertial blocks stay the placeholders
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5}}))
    os.remove(mesh_dir / "inertial.json")
    r = _run(tmp_path, "--voxel_size", "0.01")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (mesh_dir / "inertial.json").exists()
    for name, b in _inertials(ET.parse(urdf).getroot()).items():
        assert b["mass"] == "1.0" and b["inertia"] == ["0.1", "0.0", "0.0", "0.1", "0.0", "0.1"]
        assert (b["xyz"] == b["visual"]).all()


def test_command_line_density_without_a_voxel_size_writes_nothing(dev, golden, tmp_path):
    _registration_fixture(golden, tmp_path, {})
    r = _run(tmp_path, "--density", "1000")
    assert r.returncode != 0 and "ValueError" in r.stderr and "--voxel_size" in r.stderr
    assert not (tmp_path / "data/urdf").exists() and not (tmp_path / "data/mesh").exists()
