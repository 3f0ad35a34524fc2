"""CPU: host logic and the C-ABI surface (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_produces_library_and_every_declared_symbol_resolves():
    from autourdf_amd.build import build_lib
    lib_path = build_lib()
    assert os.path.exists(lib_path)
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    declared = set(re.findall(r"\b(creg_[a-z0-9_]+)\s*\(", header))
    declared -= {"creg_status"}
    from autourdf_amd import _lib
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = ctypes.CDLL(lib_path)
    for name in declared:
        assert getattr(L, name) is not None
    lib = _lib.load(check_device=False)
    assert lib.creg_version() >= 100


def test_kmeans_workspace_sizes_are_pinned_across_the_geometry_switches():
    """creg_kmeans_workspace_bytes / creg_kmeans_batch_workspace_bytes are pure host arithmetic (the pruned E-step's geometry and
    the workspace layout): n on both sides of every switch of the geometry (cell bits at 2048 / 16384 / 131072, row slots per lane
    and workgroup counts above 16384, 49152, 98304), k at both ends and at the 128 of the batched form.  The numbers are those of
    the library before the host driver was restructured; callers' allocations depend on them."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    ks = (1, 128, 1024)
    expected = {   # n: (workspace bytes per k, batch workspace bytes per k at batch = 3)
        17: ((153344, 1440512, 10744576), (768, 43776, 344832)),
        2048: ((346368, 1633536, 10937600), (49920, 92160, 393216)),
        16384: ((1494528, 2781696, 12085760), (393984, 436224, 737280)),
        16385: ((1495552, 2782720, 12086784), (393984, 436992, 738048)),
        49153: ((3340544, 4627712, 13931776), (1180416, 1223424, 1524480)),
        98305: ((6108160, 7395328, 16699392), (2360064, 2403072, 2704128)),
        131072: ((8795904, 10083072, 19387136), (3146496, 3188736, 3489792)),
        262144: ((16249600, 17536768, 26840832), (6292224, 6334464, 6635520)),
    }
    for n, (one, batch) in expected.items():
        assert tuple(lib.creg_kmeans_workspace_bytes(n, k) for k in ks) == one, n
        assert tuple(lib.creg_kmeans_batch_workspace_bytes(n, k, 3) for k in ks) == batch, n
    assert lib.creg_kmeans_workspace_bytes(0, 1) == 0 and lib.creg_kmeans_workspace_bytes(17, 0) == 0
    assert lib.creg_kmeans_batch_workspace_bytes(17, 1, 0) == 0


def test_mesh_pair_workspace_sizes_are_pinned_across_the_chunk_and_tile_switches():
    """creg_mesh_collide / clearance / contain_workspace_bytes are pure host arithmetic: the shared prefix posed | chunk_box |
    link_box, then each query's own tail.  n_tri on both sides of a 256-triangle chunk and of the 128-wide tile grid (32768),
    with and without pairs.  The numbers are those of the library before the three entries shared one posing stage; callers'
    allocations depend on them.  The one difference: creg_mesh_collide_workspace_bytes answered n_tri = 2^31 with a size the
    entry itself refused; it now returns 0 as the other two always did."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    tris = (0, 1, 255, 256, 257, 32768, 32769)
    expected = {   # (n_links, n_poses, n_pairs): per n_tri (collide, clearance, contain at q_stride 1, contain at 16)
        (1, 1, 0): ((512, 512, 512, 512), (768, 768, 768, 768), (18944, 18944, 18944, 18944), (18944, 18944, 18944, 18944), (19200, 19200, 19200, 19200), (2365952, 2365952, 2365952, 2365952), (2366208, 2366208, 2366208, 2366208)),
        (1, 1, 5): ((768, 1024, 768, 1792), (1024, 1280, 1024, 2048), (19200, 19456, 19200, 20224), (19200, 19456, 19200, 20224), (19456, 19712, 19456, 21760), (2366208, 2376192, 2376192, 2529792), (2366464, 2376448, 2376704, 2531328)),
        (1, 3, 0): ((768, 768, 768, 768), (1024, 1024, 1024, 1024), (56064, 56064, 56064, 56064), (56064, 56064, 56064, 56064), (56320, 56320, 56320, 56320), (7097088, 7097088, 7097088, 7097088), (7097344, 7097344, 7097344, 7097344)),
        (1, 3, 5): ((1024, 1280, 1024, 4608), (1280, 1536, 1280, 4864), (56320, 56576, 56320, 59904), (56320, 56576, 56320, 59904), (56576, 56832, 56832, 64000), (7097344, 7127808, 7127808, 7588608), (7097600, 7128064, 7128320, 7592704)),
        (12, 1, 0): ((1536, 1536, 1536, 1536), (1792, 1792, 1792, 1792), (19968, 19968, 19968, 19968), (19968, 19968, 19968, 19968), (20224, 20224, 20224, 20224), (2366976, 2366976, 2366976, 2366976), (2367232, 2367232, 2367232, 2367232)),
        (12, 1, 5): ((1792, 2048, 1792, 2816), (2048, 2304, 2048, 3072), (20224, 20480, 20224, 21248), (20224, 20480, 20224, 21248), (20480, 20736, 20480, 22784), (2367232, 2377216, 2377216, 2530816), (2367488, 2377472, 2377728, 2532352)),
        (12, 3, 0): ((3840, 3840, 3840, 3840), (4096, 4096, 4096, 4096), (59136, 59136, 59136, 59136), (59136, 59136, 59136, 59136), (59392, 59392, 59392, 59392), (7100160, 7100160, 7100160, 7100160), (7100416, 7100416, 7100416, 7100416)),
        (12, 3, 5): ((4096, 4352, 4096, 7680), (4352, 4608, 4352, 7936), (59392, 59648, 59392, 62976), (59392, 59648, 59392, 62976), (59648, 59904, 59904, 67072), (7100416, 7130880, 7130880, 7591680), (7100672, 7131136, 7131392, 7595776)),
    }
    for (n_links, n_poses, n_pairs), rows in expected.items():
        for n_tri, want in zip(tris, rows):
            args = (n_tri, n_links, n_poses, n_pairs)
            got = (lib.creg_mesh_collide_workspace_bytes(*args), lib.creg_mesh_clearance_workspace_bytes(*args),
                   lib.creg_mesh_contain_workspace_bytes(*args, 1), lib.creg_mesh_contain_workspace_bytes(*args, 16))
            assert got == want, args
    for bad in ((-1, 1, 1, 0), (1 << 31, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1)):
        assert lib.creg_mesh_collide_workspace_bytes(*bad) == 0 and lib.creg_mesh_clearance_workspace_bytes(*bad) == 0, bad
        assert lib.creg_mesh_contain_workspace_bytes(*bad, 1) == 0, bad
    assert lib.creg_mesh_contain_workspace_bytes(1, 1, 1, 0, 0) == 0 and lib.creg_mesh_contain_workspace_bytes(1, 1, 1, 0, 17) == 0


def test_icp_workspace_sizes_are_pinned_across_every_term_of_the_layout():
    """creg_icp_workspace_bytes / creg_icp_batch_workspace_bytes are pure host arithmetic: the larger of the two regimes'
    layouts.  n on both sides of a 64-source chunk, n / k on both sides of the regime's 1024, nf on both sides of 65536, k on
    both sides of the coordinate pool's cap min(4 nf, k nf), one configs[4]-like shape; batch 1 and 3.  The numbers are those
    of the library before icp.hip was split and the many-workgroup layout became one carve function; callers' allocations
    depend on them."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    expected = {   # (n, nf, k): (workspace bytes, batch workspace bytes at batch = 1, at batch = 3)
        (63, 100, 1): (28672, 28672, 86016),
        (64, 100, 1): (28672, 28672, 86016),
        (65, 100, 1): (29440, 29440, 88320),
        (1024, 100, 1): (80640, 80640, 241920),
        (1025, 100, 1): (81408, 81408, 244224),
        (2048, 500, 2): (192256, 192256, 576768),
        (2050, 500, 2): (193024, 193024, 579072),
        (200, 65536, 2): (5815040, 5815040, 17445120),
        (200, 65537, 2): (5816320, 5816320, 17448960),
        (1000, 777, 3): (210944, 210944, 632832),
        (1000, 777, 4): (262400, 262400, 787200),
        (1000, 777, 5): (282624, 282624, 847872),
        (120000, 120000, 30): (40620288, 40620288, 121860864),
    }
    for shape, want in expected.items():
        got = (lib.creg_icp_workspace_bytes(*shape), lib.creg_icp_batch_workspace_bytes(*shape, 1), lib.creg_icp_batch_workspace_bytes(*shape, 3))
        assert got == want, shape
    for bad in ((0, 100, 1), (100, 0, 1), (100, 100, 0), (-1, 100, 1)):
        assert lib.creg_icp_workspace_bytes(*bad) == 0 and lib.creg_icp_batch_workspace_bytes(*bad, 1) == 0, bad
    assert lib.creg_icp_batch_workspace_bytes(100, 100, 1, 0) == 0 and lib.creg_icp_batch_workspace_bytes(100, 100, 1, -1) == 0


def test_icp_entries_refuse_bad_arguments_before_any_device_call():
    """The ICP entries, creg_aabb_mask_f64 and creg_kabsch_f64 answer a bad argument with CREG_EINVAL and their own name in the
    error text.  There is no device here (a HIP call would give CREG_EHIP) and the pointers are made-up addresses that are never
    dereferenced.  Shapes of both regimes; the null field inside problem 1 of 2 at a one-workgroup shape (every problem is checked
    before the first launch)."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    EINVAL = -1
    p, big = ctypes.c_void_p(0x1000), 1 << 40

    def refused(rc, *words):
        text = lib.creg_last_error().decode()
        assert rc == EINVAL and all(w in text for w in words), (rc, text, words)

    def problem(**null):
        fields = {name: (None if name in null else p) for name, _ in _lib.IcpProblem._fields_}
        fields["tgt_offsets"] = fields["world_offsets"] = None
        return _lib.IcpProblem(**fields)

    def batch(probs, nbatch=None, n=100, k=2, nf=100, max_it=10, ws=p, ws_bytes=big):
        arr = (_lib.IcpProblem * max(len(probs), 1))(*probs)
        return lib.creg_masked_icp_batch_f64(arr if probs else None, len(probs) if nbatch is None else nbatch, n, k, nf, 1.2, 1.0, max_it, 0, ws, ws_bytes, None)

    def single(n=100, k=2, nf=100, max_it=10, local=p, ws=p, ws_bytes=big):
        return lib.creg_masked_icp_f64(local, p, None, n, p, k, p, nf, p, 1.2, 1.0, max_it, 0, p, p, p, ws, ws_bytes, None)

    def p2p(n=100, k=2, m=100, max_it=10, src=p, toff=p, ws=p, ws_bytes=big):
        return lib.creg_icp_p2p_f64(src, n, p, p, m, toff, k, p, 1.0, max_it, p, p, p, ws, ws_bytes, None)

    who = "creg_masked_icp_batch_f64"
    refused(batch([]), who, "null pointer")                                        # a null problem pointer
    refused(batch([problem()], ws=None), who, "null pointer")
    refused(batch([problem()], nbatch=0), who, "batch must be in 1..16")
    refused(batch([problem()] * 17), who, "batch must be in 1..16")
    refused(batch([problem()], n=0), who, "no source points")
    refused(batch([problem()], max_it=0), who, "bad size")
    refused(batch([problem()], k=0), who, "bad size")
    need = lib.creg_icp_batch_workspace_bytes(100, 100, 2, 2)
    refused(batch([problem()] * 2, ws_bytes=need - 1), who, "workspace too small", str(need))
    refused(batch([problem(), problem(M_out=1)]), who, "null pointer in problem 1")
    refused(batch([problem(frame=1), problem()]), who, "null pointer in problem 0")
    for n, k, nf in ((100, 2, 100), (2050, 2, 500)):                              # one workgroup per cluster | many workgroups
        need = lib.creg_icp_workspace_bytes(n, nf, k)
        who = "creg_masked_icp_f64"
        refused(single(n=0, k=k, nf=nf), who, "no source points")
        refused(single(n=n, k=k, nf=nf, max_it=0), who, "bad size")
        refused(single(n=n, k=k, nf=nf, ws=None), who, "null pointer")
        refused(single(n=n, k=k, nf=nf, ws_bytes=need - 1), who, "workspace too small", str(need))
        refused(single(n=n, k=k, nf=nf, local=None), who, "null pointer in problem 0")
        who = "creg_icp_p2p_f64"
        refused(p2p(n=0, k=k, m=nf), who, "no source points")
        refused(p2p(n=n, k=k, m=nf, max_it=0), who, "bad size")
        refused(p2p(n=n, k=k, m=nf, toff=None), who, "null pointer")
        refused(p2p(n=n, k=k, m=nf, ws_bytes=need - 1), who, "workspace too small", str(need))
        refused(p2p(n=n, k=k, m=nf, src=None), who, "null pointer in problem 0")
    for args in ((None, p, 2, p, 100, 1.2, p, p, p, None), (p, p, 0, p, 100, 1.2, p, p, p, None), (p, p, 2, p, 0, 1.2, p, p, p, None),
                 (p, p, 2, p, 1 << 31, 1.2, p, p, p, None), (p, p, 2, p, 100, 1.2, None, p, p, None), (p, p, 2, p, 100, 1.2, p, None, p, None)):
        refused(lib.creg_aabb_mask_f64(*args), "creg_aabb_mask_f64", "bad argument")
    refused(lib.creg_kabsch_f64(None, p, None, 10, p, 1, p, None), "creg_kabsch_f64", "null pointer")
    refused(lib.creg_kabsch_f64(p, p, None, 10, p, 0, p, None), "creg_kabsch_f64", "bad size")


def _train_shape(rot=0, hidden=64, k=20, n_pred=4096, n_tgt=4096, nn_search=0, batch=1):
    from autourdf_amd import _lib
    return _lib.TrainShape(rot=rot, k=k, hidden=hidden, epochs=300, n_pred=n_pred, n_tgt=n_tgt, use_graph=1, batch=batch,
                           graph_branches=0, nn_search=nn_search)


def test_train_workspace_sizes_are_pinned_across_the_layout_switches(monkeypatch):
    """creg_train_workspace_bytes is pure host arithmetic (make_dims + carve): every pose representation at both ends of the hidden
    widths; k on both sides of the KP rounding (20 | 21, 40) and at 1; n_tgt where the points per lane switch (4096 | 4097), where
    the sixteen-queries search and the one-chunk sort end (16384 | 16385) and where the pruned search ends (65536 | 65537), under
    each nn_search; n_pred on both sides of the PS_MAXB block bound (31488 | 31489 at 64-point blocks and k = 20) and of the 16-bit
    index bound (65534 | 65535); batch 0, 1, 5, 64.  300 epochs.  The numbers are those of the library before train_engine.hip was
    split; callers' allocations depend on them.  CREG_NN_ROWS changes the layout and is unset here."""
    from autourdf_amd import _lib
    monkeypatch.delenv("CREG_NN_ROWS", raising=False)
    lib = _lib.load(check_device=False)
    size = lambda **kw: lib.creg_train_workspace_bytes(ctypes.byref(_train_shape(**kw)))
    by_rot_hidden = {(0, 64): 788992, (0, 512): 7673856, (1, 64): 759296, (1, 512): 5597696, (2, 64): 808704, (2, 512): 7822592,
                     (3, 64): 779008, (3, 512): 7599360}
    for (rot, hidden), want in by_rot_hidden.items():
        assert size(rot=rot, hidden=hidden) == want, (rot, hidden)
    for k, want in {1: 740864, 20: 788992, 21: 826880, 40: 875008, 256: 1818112}.items():
        assert size(k=k) == want, k
    by_n_tgt = {   # n_tgt: bytes at nn_search 0, 1, 2
        4096: (788992, 554496, 788992), 4097: (793600, 564224, 916480), 16384: (1191424, 761856, 1306624),
        16385: (1312768, 762368, 1312768), 65536: (2890240, 1554432, 2890240), 65537: (1554944, 1554944, 1554944)}
    for n_tgt, want in by_n_tgt.items():
        assert tuple(size(n_tgt=n_tgt, nn_search=s) for s in (0, 1, 2)) == want, n_tgt
    by_n_pred = {   # (n_pred, n_tgt): bytes at nn_search 0, 2
        (31488, 4096): (3431424, 3431424), (31489, 4096): (2376960, 2376960), (31488, 16384): (3836928, 3941376),
        (31489, 16384): (3950848, 3950848), (65534, 16384): (7217152, 7217152), (65535, 16384): (4959744, 4959744)}
    for (n_pred, n_tgt), want in by_n_pred.items():
        assert tuple(size(n_pred=n_pred, n_tgt=n_tgt, nn_search=s) for s in (0, 2)) == want, (n_pred, n_tgt)
    for batch, want in {0: 788992, 1: 788992, 5: 3944960, 64: 50495488}.items():
        assert size(batch=batch) == want, batch
    assert size(rot=2, hidden=512, k=193) == 10694144
    assert lib.creg_train_workspace_bytes(None) == 0


def test_train_workspace_is_zero_bytes_for_a_shape_outside_the_plan(monkeypatch):
    """Shapes creg_train_workspace_bytes must answer with 0: batch 65, k 257, hidden 96, and '6d' at hidden 512 with k 194 --
    the limit include/creg.h states (k <= 193 there; '6d' <= 227 at the narrower widths: k_bd's feature pieces).  The library
    before train_engine.hip was split did not hold the first of the two (10696448 bytes at k 194); this one does."""
    from autourdf_amd import _lib
    monkeypatch.delenv("CREG_NN_ROWS", raising=False)
    lib = _lib.load(check_device=False)
    size = lambda **kw: lib.creg_train_workspace_bytes(ctypes.byref(_train_shape(**kw)))
    assert size(batch=65) == 0 and size(batch=-1) == 0
    assert size(k=257) == 0 and size(k=0) == 0
    assert size(hidden=96) == 0
    assert size(rot=2, hidden=64, k=228) == 0 and size(rot=2, hidden=256, k=228) == 0 and size(rot=2, hidden=256, k=227) > 0
    assert size(rot=2, hidden=512, k=194) == 0 and size(rot=2, hidden=512, k=227) == 0 and size(rot=2, hidden=512, k=193) > 0
    assert size(rot=0, hidden=512, k=194) > 0 and size(rot=1, hidden=512, k=256) > 0          # the other representations: up to 256


def test_train_plan_entries_refuse_bad_arguments_before_any_device_call():
    """creg_train_plan_create answers a bad argument with CREG_EINVAL and its own name; so do run_batch, resume, probe and profile
    on a null plan.  Without a device a HIP call gives CREG_EHIP: what a create with everything in order then returns, the plan
    freed again and the caller's pointer left alone.  The workspace is a made-up address that is never dereferenced."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    EINVAL, EHIP = -1, -2
    ws, big = ctypes.c_void_p(0x10000), 1 << 40

    def refused(rc, *words):
        text = lib.creg_last_error().decode()
        assert rc == EINVAL and all(w in text for w in words), (rc, text, words)

    def create(shape=None, ws=ws, ws_bytes=big, out=True):
        plan = ctypes.c_void_p(0)
        rc = lib.creg_train_plan_create(ctypes.byref(shape or _train_shape()), ws, ws_bytes, ctypes.byref(plan) if out else None)
        assert (plan.value is None) == (rc != 0)                         # a failed create leaves the caller's pointer alone
        if plan.value:
            lib.creg_train_plan_destroy(plan)
        return rc

    who = "creg_train_plan_create"
    refused(create(out=False), who, "null pointer")
    refused(create(ws=None), who, "null pointer")
    for bad in (_train_shape(hidden=96), _train_shape(k=257), _train_shape(rot=4), _train_shape(n_tgt=0)):
        refused(create(bad), who, "unsupported shape")
    refused(create(ws=ctypes.c_void_p(0x10080)), who, "256-byte aligned")
    for batch in (-1, 65):
        refused(create(_train_shape(batch=batch)), who, "batch must be in [0, 64]")
    for shape in (_train_shape(), _train_shape(batch=5, n_tgt=16385)):
        need = lib.creg_train_workspace_bytes(ctypes.byref(shape))
        refused(create(shape, ws_bytes=need - 1), who, "workspace too small", str(need))
        # everything in order: the first device call (k_bd's dynamic-LDS limit) fails without a device; with one the plan is made
        assert create(shape, ws_bytes=need) == (EHIP if lib.creg_device_check() != 0 else 0)
    args, state, us = _lib.TrainArgs(), _lib.TrainState(), (ctypes.c_float * 12)()
    refused(lib.creg_train_plan_run_batch(None, ctypes.byref(args), 1, None), "creg_train_plan_run_batch", "null pointer")
    refused(lib.creg_train_plan_run(None, ctypes.byref(args), None), "creg_train_plan_run_batch", "null pointer")
    refused(lib.creg_train_plan_resume(None, ctypes.byref(args), ctypes.byref(state), 1, None, None, None, None), "creg_train_plan_resume", "null pointer")
    refused(lib.creg_train_plan_probe(None, ctypes.byref(args), None, None, None, None, None), "creg_train_plan_probe", "null pointer")
    refused(lib.creg_train_plan_profile(None, ctypes.byref(args), 1, us, None), "creg_train_plan_profile", "bad argument")
    assert lib.creg_train_plan_destroy(None) == 0


def test_every_environment_variable_the_library_reads_is_documented():
    """Every getenv("CREG_...") of the library's sources has a row of its own in the "Environment" table of INTEGRATION.md."""
    csrc = os.path.join(ROOT, "autourdf_amd", "csrc")
    read = set()
    for fn in os.listdir(csrc):
        if fn.endswith((".hip", ".h")):
            read |= set(re.findall(r'getenv\("(CREG_\w+)"\)', open(os.path.join(csrc, fn)).read()))
    assert "CREG_NN_ROWS" in read and "CREG_KM_SPIN_LIMIT" in read           # (the scan does find them)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("## Environment"):doc.index("## Build / test")]
    rows = set()
    for line in table.splitlines():
        if line.startswith("| `"):
            rows |= set(re.findall(r"`(\w+)`", line.split("|")[1]))
    assert read <= rows, sorted(read - rows)


def test_product_path_has_no_cpu_fallback_and_never_imports_the_oracle():
    import torch
    from autourdf_amd import dq_func, ops
    with pytest.raises(RuntimeError):
        ops.nn_l1_bidir(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        dq_func.transform_to_dualquat(torch.eye(4)[None])
    pkg = os.path.join(ROOT, "autourdf_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), fn
            assert "/root/reference" not in src, fn


def test_drop_in_signatures_match_the_reference_surface():
    import inspect
    from autourdf_amd import cluster_icp, dq_func, helper_functions, mlp_reg, model_utils
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(mlp_reg.train) == ["m", "y", "model", "clusters", "stop", "learning_rate", "scheduler_patience",
                                  "scheduler_factor"]
    d = inspect.signature(mlp_reg.train).parameters
    assert (d["stop"].default, d["learning_rate"].default, d["scheduler_patience"].default,
            d["scheduler_factor"].default) == (200, 0.0002, 5, 0.7)
    assert sig(mlp_reg.calculate_pc) == ["local_clusters", "matrices"]
    assert sig(mlp_reg.resample_cluster) == ["segments", "idx", "n_clusters", "matrices", "normal", "visual"]
    assert sig(mlp_reg.match) == ["data_dir", "idx"]
    assert sig(cluster_icp.masked_icp)[:9] == ["clusters_local", "clusters_world", "step_pc_np", "matrices", "visual",
                                               "ori", "scale", "th", "colors"]
    assert sig(cluster_icp.Segments.__init__) == ["self", "data_path", "sample_size"]
    assert sig(cluster_icp.Segments.k_means_cluster)[:5] == ["self", "pc_id", "num", "normal", "colors"]
    for name in ("transform_from_rot_trans", "quaternion_conjugate", "quat_trans_to_dualquat", "rot_trans_to_dualquat",
                 "transform_to_dualquat", "dualquat_to_quat_trans", "dualquat_to_rot_trans", "dualquat_to_transform",
                 "dualquat_multiply", "dualquat_invert", "point_to_dualquat"):
        assert callable(getattr(dq_func, name))
    assert callable(helper_functions.save_pc_npz) and callable(helper_functions.load_pc_npz)
    q = model_utils.QRegMLP(True, hidden_dim=512)
    assert sum(p.numel() for p in q.parameters()) == 425991
    from oracle import models
    assert list(q.state_dict()) and set(q.state_dict()) == set(models.QRegMLP(True, 512).state_dict())
    assert set(model_utils.DQRegMLP(512).state_dict()) == set(models.DQRegMLP(512).state_dict())


def test_models_forward_match_reference_golden(golden):
    import torch
    from autourdf_amd import model_utils
    g = golden("models_reference.npz")
    q = model_utils.QRegMLP(True, hidden_dim=32)
    q.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("q.")})
    t, r = q(torch.from_numpy(g["q_in"]))
    np.testing.assert_allclose(t.detach().numpy(), g["q_out_t"], atol=1e-7)
    np.testing.assert_allclose(r.detach().numpy(), g["q_out_r"], atol=1e-7)
    d = model_utils.DQRegMLP(hidden_dim=32)
    d.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("dq.")})
    np.testing.assert_allclose(d(torch.from_numpy(g["dq_in"])).detach().numpy(), g["dq_out"], atol=1e-7)
    from oracle import models as omodels
    for mod in (model_utils, omodels):                      # product modules and oracle restatements alike
        r = mod.RRegMLP(hidden_dim=32)
        r.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("r6d.")})
        t, rr = r(torch.from_numpy(g["r6d_in"]))
        np.testing.assert_allclose(t.detach().numpy(), g["r6d_out_t"], atol=1e-7)
        np.testing.assert_allclose(rr.detach().numpy(), g["r6d_out_r"], atol=1e-7)
        e = mod.RegMLP(6, 3)
        e.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("rpy.")})
        t, rr = e(torch.from_numpy(g["rpy_in"]))
        np.testing.assert_allclose(t.detach().numpy(), g["rpy_out_t"], atol=1e-7)
        np.testing.assert_allclose(rr.detach().numpy(), g["rpy_out_r"], atol=1e-7)


def test_train_plan_parameter_layout_matches_every_reference_model():
    """The four --r choices (mlp_reg.py:276-291) on the fused plan: the tensor shapes ops.TrainPlan expects (in Q_PARAM_ORDER /
    DQ_PARAM_ORDER) are the models' own, at the reference's widths -- 512, and 3 for RegMLP(6, 3) -- and at the padded width."""
    import types
    from autourdf_amd import mlp_reg, model_utils, ops
    cases = [("q", model_utils.QRegMLP(True, 512)), ("dq", model_utils.DQRegMLP(512)), ("6d", model_utils.RRegMLP(512)),
             ("rpy", model_utils.RegMLP(6, 3)), ("6d", model_utils.RRegMLP(100)), ("rpy", model_utils.RegMLP(True, 64))]
    for rot, model in cases:
        got_rot, params, hidden = mlp_reg._model_params(model)
        assert got_rot == rot and hidden == model.encoder[0].out_features
        order = ops.DQ_PARAM_ORDER if rot == "dq" else ops.Q_PARAM_ORDER
        shapes = ops.TrainPlan._param_shapes(types.SimpleNamespace(rot=ops.TRAIN_ROT[rot]), hidden)
        assert len(params) == len(order) == len(shapes)
        for name, p, want in zip(order, params, shapes):
            assert tuple(p.shape) == tuple(want), (rot, name, tuple(p.shape), want)
        padded = ops.TrainPlan._param_shapes(types.SimpleNamespace(rot=ops.TRAIN_ROT[rot]), next(t for t in ops.TRAIN_HIDDEN_TILES if t >= hidden))
        assert all(all(a <= b for a, b in zip(sm, sp)) for sm, sp in zip(shapes, padded))
    with pytest.raises(NotImplementedError):
        import torch
        mlp_reg._model_params(torch.nn.Linear(3, 3))


def test_npz_roundtrip_keeps_order_and_dtype(tmp_path):
    from autourdf_amd.helper_functions import load_pc_npz, save_pc_npz
    rng = np.random.default_rng(0)
    segs = [rng.normal(size=(n, 3)) for n in (5, 0, 12, 3, 7, 1, 9, 2, 4, 6, 8, 10)]     # > 10: '10' sorts after '1'
    save_pc_npz(segs, str(tmp_path / "c.npz"))
    back = load_pc_npz(str(tmp_path / "c.npz"))
    assert len(back) == len(segs)
    for a, b in zip(segs, back):
        np.testing.assert_array_equal(a, b)


def test_ply_reader_ascii_and_binary(tmp_path):
    from autourdf_amd.cluster_icp import read_point_cloud
    pts = np.random.default_rng(1).normal(size=(17, 3))
    p1 = tmp_path / "a.ply"
    with open(p1, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment x\nelement vertex 17\nproperty double x\nproperty double y\n"
                "property double z\nend_header\n")
        for r in pts:
            f.write("%.17g %.17g %.17g\n" % tuple(r))
    np.testing.assert_array_equal(read_point_cloud(str(p1)).points, pts)
    p2 = tmp_path / "b.ply"
    rec = np.zeros(17, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    with open(p2, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\nproperty float y\n"
                b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        f.write(rec.tobytes())
    np.testing.assert_array_equal(read_point_cloud(str(p2)).points, pts.astype(np.float32).astype(np.float64))


def test_synthetic_sequences_are_seeded_and_sized():
    from autourdf_amd.synthetic import initial_segmentation, make_sequence
    a = make_sequence("wx200_5", 2, 3, 4096)
    b = make_sequence("wx200_5", 2, 3, 4096)
    assert all(x.shape == (4096, 3) and x.dtype == np.float64 for x in a)
    assert all((x == y).all() for x, y in zip(a, b))
    assert not (a[0] == make_sequence("wx200_5", 3, 1, 4096)[0]).all()
    mats, clusters, lab = initial_segmentation(a[0], 20, seed=0)
    assert mats.shape == (20, 4, 4) and sum(len(c) for c in clusters) == 4096 and lab.dtype == np.int32
    for r in ("franka", "allegro", "chain32"):
        assert make_sequence(r, 0, 1, 512)[0].shape == (512, 3)


def test_kmeans_plusplus_follows_sklearns_draw_sequence(golden):
    """Segments.k_means_cluster seeds like scikit-learn does (global RandomState, k-means++ on centred data): with the
    same np.random.seed, live sklearn's k_means(init="k-means++") and our seeding + Lloyd give identical labels, and
    the reference-minted segmentation golden (reference Segments.k_means_cluster under np.random.seed) is reproduced."""
    import numpy as np
    from sklearn.cluster import k_means
    from autourdf_amd.cluster_icp import kmeans_plusplus_sklearn
    from oracle import kmeans as okm
    g = golden("segments_reference.npz")
    X = g["frame"]
    for seed in (int(g["seed"]), 0, 5):
        np.random.seed(seed)
        _, lab, _ = k_means(X.copy(), init="k-means++", n_clusters=8)
        np.random.seed(seed)
        idx = kmeans_plusplus_sklearn(X, 8, np.random.mtrand._rand)
        _, olab, _, _ = okm.k_means(X, X[idx])
        np.testing.assert_array_equal(lab, olab)
    np.random.seed(int(g["seed"]))
    idx = kmeans_plusplus_sklearn(X, 8, np.random.mtrand._rand)
    _, olab, _, _ = okm.k_means(X, X[idx])
    np.testing.assert_array_equal(np.cumsum([0] + list(np.bincount(olab, minlength=8))), g["offsets"])
    for i in range(8):
        np.testing.assert_allclose(X[olab == i].mean(0), g["matrices"][i][:3, 3], atol=1e-14)


def test_dq_autograd_formulas_match_the_oracle_values_and_gradients():
    """autourdf_amd._dq_autograd (the torch restatements the drop-in differentiates in its backward) against oracle.dq, which
    is pinned to the reference module's goldens: values and input gradients, fp64 on the CPU."""
    import torch
    from autourdf_amd import _dq_autograd as ag
    from oracle import dq as odq
    from scipy.spatial.transform import Rotation
    g = torch.Generator().manual_seed(4)
    M = torch.eye(4, dtype=torch.float64).repeat(24, 1, 1)
    M[:, :3, :3] = torch.from_numpy(Rotation.random(24, random_state=2).as_matrix())
    M[:, :3, 3] = torch.randn(24, 3, generator=g, dtype=torch.float64)
    d1 = odq.transform_to_dualquat(M) + 0.05 * torch.randn(24, 8, generator=g, dtype=torch.float64)
    d2 = odq.transform_to_dualquat(M.flip(0)) + 0.05 * torch.randn(24, 8, generator=g, dtype=torch.float64)
    cases = [(ag.transform_to_dualquat, odq.transform_to_dualquat, (M,)),
             (ag.quat_trans_to_dualquat, odq.quat_trans_to_dualquat, (d1[:, :4].clone(), M[:, :3, 3].clone())),
             (ag.dualquat_to_quat_trans, odq.dualquat_to_quat_trans, (d1,)),
             (ag.dualquat_multiply, odq.dualquat_multiply, (d1, d2)),
             (ag.dualquat_invert, odq.dualquat_invert, (d1,))]
    for mine, ref, ins in cases:
        a = [x.clone().requires_grad_(True) for x in ins]
        b = [x.clone().requires_grad_(True) for x in ins]
        oa, ob = mine(*a), ref(*b)
        oa, ob = (oa if isinstance(oa, tuple) else (oa,)), (ob if isinstance(ob, tuple) else (ob,))
        for x, y in zip(oa, ob):
            assert torch.allclose(x, y, atol=1e-13)
        w = [torch.randn(x.shape, generator=g, dtype=torch.float64) for x in oa]
        sum((x * ww).sum() for x, ww in zip(oa, w)).backward()
        sum((y * ww).sum() for y, ww in zip(ob, w)).backward()
        for x, y in zip(a, b):
            assert torch.allclose(x.grad, y.grad, atol=1e-12)


def test_file_writer_is_bounded_and_does_not_mask_the_frame_loops_error():
    """mlp_reg._FileWriter: at most MAX_PENDING frames wait behind the worker (a job pins a frame's device tensors), a
    submit blocks instead of queueing more, the worker's error surfaces in close() -- unless another exception is already propagating,
    which it must not replace."""
    import sys
    import threading
    import time
    from autourdf_amd import mlp_reg
    w = mlp_reg._FileWriter()
    gate, done = threading.Event(), []
    w.submit(lambda: gate.wait(10))                       # the worker is busy with this one
    for i in range(mlp_reg._FileWriter.MAX_PENDING):
        w.submit(done.append, i)                         # fills the queue
    t = threading.Thread(target=lambda: w.submit(done.append, "late"))
    t.start()
    time.sleep(0.3)
    assert t.is_alive()                                  # the submit beyond the bound waits
    gate.set()
    t.join(10)
    w.close()
    assert done == list(range(mlp_reg._FileWriter.MAX_PENDING)) + ["late"]

    def boom():
        raise ValueError("disk full")

    w = mlp_reg._FileWriter()
    w.submit(boom)
    time.sleep(0.2)
    with pytest.raises(KeyError):
        try:
            raise KeyError("the frame loop's own error")
        finally:
            w.close(propagating=sys.exc_info()[0] is not None)
    w = mlp_reg._FileWriter()
    w.submit(boom)
    time.sleep(0.2)
    with pytest.raises(ValueError):
        w.close()


def test_register_sequence_surfaces_a_writer_failure_inside_a_callers_except_block(monkeypatch, tmp_path):
    """`finally: writer.close(propagating=sys.exc_info()[0] is not None)` was also true when register_sequence was merely
    CALLED from inside somebody's `except` block -- a genuine file-writer failure was then swallowed and the frames were lost without a
    message.  The frame loop now tracks its own failure: the writer's error comes out, the loop's own error is still never replaced."""
    import time
    import torch
    from autourdf_amd import mlp_reg

    def boom():
        raise ValueError("disk full")

    def frames_ok(*a, writer, **kw):
        writer.submit(boom)
        time.sleep(0.2)

    def frames_fail(*a, writer, **kw):
        writer.submit(boom)
        time.sleep(0.2)
        raise KeyError("the frame loop's own error")

    monkeypatch.setattr(mlp_reg, "DEVICE", torch.device("cpu"))
    monkeypatch.setattr(mlp_reg, "_register_frames", frames_ok)
    args = (None, np.eye(4)[None].repeat(2, 0), [np.zeros((3, 3)), np.zeros((2, 3))])
    with pytest.raises(ValueError, match="disk full"):
        try:
            raise RuntimeError("the caller is handling something else")
        except RuntimeError:
            mlp_reg.register_sequence(*args, save_dir=str(tmp_path) + "/", models=(None, None))
    monkeypatch.setattr(mlp_reg, "_register_frames", frames_fail)
    with pytest.raises(KeyError):
        mlp_reg.register_sequence(*args, save_dir=str(tmp_path) + "/", models=(None, None))


def test_file_writer_as_a_context_manager_reports_the_exception_leaving_its_own_block():
    """`with _FileWriter()`: a worker error surfaces on leaving the block, never replaces an exception raised inside it, and does
    surface when the block merely runs inside a caller's `except` (the exception leaving THIS block counts, not sys.exc_info())."""
    import time
    from autourdf_amd import mlp_reg

    def boom():
        raise ValueError("disk full")

    done = []
    with mlp_reg._FileWriter() as w:
        w.submit(done.append, 1)
    assert done == [1] and not w._t.is_alive()
    with pytest.raises(ValueError, match="disk full"):
        with mlp_reg._FileWriter() as w:
            w.submit(boom)
            time.sleep(0.2)
    assert not w._t.is_alive()
    with pytest.raises(KeyError):
        with mlp_reg._FileWriter() as w:
            w.submit(boom)
            time.sleep(0.2)
            raise KeyError("the frame loop's own error")
    assert not w._t.is_alive()
    with pytest.raises(ValueError, match="disk full"):
        try:
            raise RuntimeError("the caller is handling something else")
        except RuntimeError:
            with mlp_reg._FileWriter() as w:
                w.submit(boom)
                time.sleep(0.2)


def _frame0_globals(monkeypatch, tmp_path, segments):
    from autourdf_amd import mlp_reg
    monkeypatch.chdir(tmp_path)
    for name, v in dict(ROBOT="toy", NUM_SEG=3, STEP_SZIE=4, NUM_CAMERAS=20, NORMAL=False,
                        RAW_PATH_LIST=["data/raw/toy/4_deg_20_cams/V0000/", "data/raw/toy/4_deg_20_cams/V0001/"]).items():
        monkeypatch.setattr(mlp_reg, name, v, raising=False)
    monkeypatch.setattr(mlp_reg, "Segments", segments)
    return mlp_reg, "data/part/toy_3_seg/4_deg_20_cams/"


def _files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_frame0_state_is_reloaded_from_the_first_output_directory(monkeypatch, tmp_path):
    def no_segments(path):
        raise AssertionError("an existing output directory must be reloaded, not recomputed")

    mlp_reg, base = _frame0_globals(monkeypatch, tmp_path, no_segments)
    rng = np.random.default_rng(0)
    mats, clusters = rng.normal(size=(3, 4, 4)), [rng.normal(size=(n, 3)) for n in (5, 2, 7)]
    assert mlp_reg._out_dir() == base and mlp_reg._out_dir("data/raw/toy/4_deg_20_cams/V0001/") == base + "V0001/"
    mlp_reg._write_frame0(base + "V0001/", mats, clusters)
    os.makedirs(base + "V0002")                           # a later directory without a frame-0 state: the FIRST one is read
    before = _files_under(tmp_path)
    assert before == [base + "V0001/cluster/0000.npz", base + "V0001/matrix/0000.npy"]
    m, c = mlp_reg._frame0_state()
    np.testing.assert_array_equal(m, np.load(base + "V0001/matrix/0000.npy"))
    np.testing.assert_array_equal(m, mats)
    with np.load(base + "V0001/cluster/0000.npz") as z:
        assert list(z.keys()) == ["0", "1", "2"] and len(c) == 3
        for i in range(3):
            np.testing.assert_array_equal(c[i], z[str(i)])
            np.testing.assert_array_equal(c[i], clusters[i])
    mlp_reg._ensure_frame0("data/raw/toy/4_deg_20_cams/V0000/")
    assert _files_under(tmp_path) == before               # nothing written


def test_frame0_state_is_computed_from_the_first_raw_sequence_and_written_once(monkeypatch, tmp_path):
    made = []

    class StubSegments:
        def __init__(self, path):
            made.append(path)

        def k_means_cluster(self, idx, n_seg, normal):
            made.append((idx, n_seg, normal))
            self.init_matrix_list = [np.eye(4) * (i + 1) for i in range(n_seg)]
            self.init_segment_list = [np.full((i + 2, 3), float(i)) for i in range(n_seg)]

    mlp_reg, base = _frame0_globals(monkeypatch, tmp_path, StubSegments)
    m, c = mlp_reg._frame0_state()
    assert made == ["data/raw/toy/4_deg_20_cams/V0000/", (0, 3, False)] and _files_under(tmp_path) == []
    assert m.shape == (3, 4, 4) and m[2, 0, 0] == 3.0 and [x.shape[0] for x in c] == [2, 3, 4]
    mlp_reg._ensure_frame0("data/raw/toy/4_deg_20_cams/V0007/")      # written under the name of the sequence it is given
    assert _files_under(tmp_path) == [base + "V0007/cluster/0000.npz", base + "V0007/matrix/0000.npy"]
    np.testing.assert_array_equal(np.load(base + "V0007/matrix/0000.npy"), m)
    for a, b in zip(mlp_reg.load_pc_npz(base + "V0007/cluster/0000.npz"), c):
        np.testing.assert_array_equal(a, b)
    n_made = len(made)
    mlp_reg._ensure_frame0("data/raw/toy/4_deg_20_cams/V0008/")      # output exists now: neither computed nor written again
    assert len(made) == n_made and not os.path.exists(base + "V0008")


def _record(monkeypatch, ops, names):
    """Replace ops.<name> by recorders: calls = [(name, args, kwargs)], each returning (name, index of the call)."""
    calls = []
    for name in names:
        def rec(*a, _name=name, **kw):
            calls.append((_name, a, kw))
            return (_name, len(calls) - 1)
        monkeypatch.setattr(ops, name, rec)
    return calls


def test_kmeans_lloyd_each_takes_the_batch_launch_exactly_up_to_its_limits(monkeypatch):
    import torch
    from autourdf_amd import ops
    assert (ops.KMEANS_BATCH_MAX, ops.KMEANS_BATCH_MAX_N, ops.KMEANS_BATCH_MAX_K) == (16, 16384, 128)
    calls = _record(monkeypatch, ops.segment, ["kmeans_lloyd_batch", "kmeans_lloyd"])

    def case(B, n, k, ns=None):
        Xs = [torch.zeros(n if ns is None else ns[b], 3, dtype=torch.float64) for b in range(B)]
        inits = [torch.zeros(k, 3, dtype=torch.float64) for _ in range(B)]
        del calls[:]
        return Xs, inits, ops.kmeans_lloyd_each(Xs, inits)

    for B, n, k in ((16, 16384, 128), (1, 7, 1)):
        Xs, inits, out = case(B, n, k)
        assert out == ("kmeans_lloyd_batch", 0) and len(calls) == 1
        assert calls[0][1][0] is Xs and calls[0][1][1] is inits and calls[0][2] == {}
    for B, n, k, ns in ((17, 64, 4, None), (2, 16385, 4, None), (2, 64, 129, None), (2, None, 4, (64, 48))):
        Xs, inits, out = case(B, n, k, ns)
        assert out == [("kmeans_lloyd", b) for b in range(B)]
        for b, (name, a, kw) in enumerate(calls):
            assert name == "kmeans_lloyd" and a[0] is Xs[b] and a[1] is inits[b] and len(a) == 2 and kw == {}
    assert ops.kmeans_lloyd_each([], []) == []


def test_group_to_local_each_takes_the_batch_launch_exactly_up_to_its_limit(monkeypatch):
    import torch
    from autourdf_amd import ops
    assert ops.GROUP_BATCH_MAX == 16
    calls = _record(monkeypatch, ops.segment, ["group_to_local_batch", "group_to_local"])

    def case(ns, inverse):
        Xs = [torch.zeros(n, 3, dtype=torch.float64) for n in ns]
        labels = [torch.zeros(n, dtype=torch.int32) for n in ns]
        Ms = [torch.zeros(5, 4, 4, dtype=torch.float64) for _ in ns]
        del calls[:]
        return Xs, labels, Ms, ops.group_to_local_each(Xs, labels, Ms, m_is_inverse=inverse)

    for inverse in (False, True):
        Xs, labels, Ms, out = case([40] * 16, inverse)
        assert out == ("group_to_local_batch", 0) and len(calls) == 1
        assert [x is y for x, y in zip(calls[0][1], (Xs, labels, Ms))] == [True] * 3 and calls[0][2] == {"m_is_inverse": inverse}
        for ns in ([40] * 17, [40, 24]):
            Xs, labels, Ms, out = case(ns, inverse)
            assert out == [("group_to_local", b) for b in range(len(ns))]
            for b, (name, a, kw) in enumerate(calls):
                assert name == "group_to_local" and kw == {"m_is_inverse": inverse}
                assert len(a) == 3 and a[0] is Xs[b] and a[1] is labels[b] and a[2] is Ms[b]


def test_masked_icp_each_takes_the_batch_launch_exactly_up_to_its_limit(monkeypatch):
    import inspect
    import torch
    from autourdf_amd import ops
    assert ops.ICP_BATCH_MAX == 16
    signature = inspect.signature(ops.masked_icp)
    calls = _record(monkeypatch, ops.icp, ["masked_icp_batch", "masked_icp", "cluster_transform"])

    def problems(ns, world="given", woff=False):
        out = []
        for n in ns:
            p = (torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 3) if world == "given" else None,
                 torch.zeros(6, dtype=torch.int32), torch.zeros(50, 3, dtype=torch.float64), torch.ones(5, 4, 4, dtype=torch.float64))
            out.append(p + (torch.ones(6, dtype=torch.int32),) if woff else p)
        del calls[:]
        return out

    for world, woff in (("given", False), ("given", True), (None, False)):
        probs = problems([40] * 16, world, woff)
        assert ops.masked_icp_each(probs) == ("masked_icp_batch", 0)
        assert len(calls) == 1 and len(calls[0][1]) == 1 and calls[0][1][0] is probs and calls[0][2] == {}
    for ns in ([40] * 17, [40, 24]):
        # six-tuples (the --mlp_icp frame): world_offsets arrives in masked_icp's `world_offsets`, `scale` keeps its default
        probs = problems(ns, "given", True)
        assert ops.masked_icp_each(probs) == [("masked_icp", b) for b in range(len(ns))]
        for p, (name, a, kw) in zip(probs, calls):
            bound = signature.bind(*a, **kw)
            assert name == "masked_icp" and "scale" not in bound.arguments and bound.arguments["world_offsets"] is p[5]
            assert [bound.arguments[k] is v for k, v in zip(("local", "world", "offsets", "frame", "M"), p)] == [True] * 5
        # world None (BatchIcpRegistrar): the boxes are cluster_transform of the float32 casts, made right before each ICP
        probs = problems(ns, None)
        assert ops.masked_icp_each(probs) == [("masked_icp", 2 * b + 1) for b in range(len(ns))]
        assert [c[0] for c in calls] == ["cluster_transform", "masked_icp"] * len(ns)
        for b, p in enumerate(probs):
            (_, ta, tkw), (_, a, kw) = calls[2 * b], calls[2 * b + 1]
            assert tkw == {} and len(ta) == 3 and ta[1] is p[2]
            assert ta[0].dtype == torch.float32 and ta[0].shape == p[0].shape and ta[2].dtype == torch.float32 and torch.equal(ta[2], p[4].float())
            bound = signature.bind(*a, **kw)
            assert bound.arguments["world"] == ("cluster_transform", 2 * b) and bound.arguments.get("world_offsets") is None
            assert "scale" not in bound.arguments
            assert [bound.arguments[k] is p[i] for k, i in (("local", 0), ("offsets", 2), ("frame", 3), ("M", 4))] == [True] * 4


#: the public names of autourdf_amd/ops.py when it was one file: every one of them stays reachable as ops.<name>
OPS_PUBLIC = [
    "DQ_PARAM_ORDER", "GROUP_BATCH_MAX", "HULL_MAX_COORD", "HULL_STATUS", "ICP_BATCH_MAX", "JOINT_MAX_SAMPLES", "JOINT_THETA_MIN",
    "KMEANS_BATCH_MAX", "KMEANS_BATCH_MAX_K", "KMEANS_BATCH_MAX_N", "KMEANS_ND_MAX_K", "KMEANS_ND_MAX_N", "LINK_SWEEP_MAX_K",
    "MESH_CONTAIN_MAX_POINTS", "MESH_INERTIA_KEYS", "MESH_MAX_NEIGHBORS", "POSE_FIT_MAX_D", "Q_PARAM_ORDER", "TRAIN_HIDDEN_TILES",
    "TRAIN_ROT", "TrainPlan", "aabb_mask", "chamfer_distance", "cluster_transform", "coord_dist_map", "coord_mst", "depth_points",
    "dq_invert", "dq_multiply", "dq_to_quat_trans", "dq_to_se3", "dq_to_se3_bwd", "group_to_local", "group_to_local_batch",
    "group_to_local_each", "icp_nn_counters", "icp_p2p", "icp_p2p_batch", "joint_axes", "joint_axes_prepare", "joint_chains",
    "joint_positions", "joint_samples", "joint_slides", "joint_types", "kabsch", "kmeans_assign", "kmeans_lloyd", "kmeans_lloyd_batch",
    "kmeans_lloyd_each", "kmeans_lloyd_nd", "knn_normals", "lattice_hull", "link_clouds", "link_clouds_bytes", "link_clouds_prepare",
    "link_moments", "link_poses", "link_sweep", "masked_icp", "masked_icp_batch", "masked_icp_each", "masked_icp_regime",
    "matrix_to_quat", "mesh_clearance", "mesh_collide", "mesh_contain", "mesh_inertia", "motion_error", "nn_l1_bidir", "pack_clusters",
    "point_mesh_distance", "pose_coords", "pose_fit_system", "quat_to_matrix", "quat_trans_to_dq", "raster_depth", "sample_mesh",
    "se3_to_dq", "segment_plane", "statistical_outlier", "urdf_fk", "visibility", "voxel_layout", "voxel_mesh"]


def test_ops_package_keeps_the_one_file_surface():
    import types
    from autourdf_amd import ops
    assert len(OPS_PUBLIC) == 85 and OPS_PUBLIC == sorted(OPS_PUBLIC)
    public = sorted(n for n, v in vars(ops).items() if not n.startswith("_") and not isinstance(v, types.ModuleType))
    assert public == OPS_PUBLIC
    for private in ("_p", "_stream", "_need", "_morton_order"):                   # used from outside the package
        assert callable(getattr(ops, private))
    assert os.path.isdir(os.path.dirname(ops.__file__)) and os.path.basename(ops.__file__) == "__init__.py"
    assert not os.path.exists(os.path.join(ROOT, "autourdf_amd", "ops.py"))


def test_workspace_holds_the_bytes_asked_for_at_an_8_byte_boundary():
    import torch
    from autourdf_amd.ops._common import _workspace
    for nbytes in (0, 1, 4, 7, 8, 12, 257):
        ws = _workspace(torch.device("cpu"), nbytes)
        assert ws.dtype == torch.uint8 and ws.device.type == "cpu" and ws.is_contiguous()
        assert ws.numel() * ws.element_size() >= max(nbytes, 1) and ws.data_ptr() % 8 == 0
