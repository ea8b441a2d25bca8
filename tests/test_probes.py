"""Light probes (brt_bake_probes*, brt_probe_rays_device, brt_probe_project_device, brt_host_probe_*; DESIGN.md "Light probes").  CPU:
the exports, the direction table, the restatement (tests/probe_ref.py) against the closed-form sky and against float64, the host
evaluation, rejections.  GPU: the two kernels bitwise against the restatement on generated and synthetic lists; bakes bitwise against
radiance_ref + the restatement on both trees, both bases, both entry points and both radiance forms; one call against its three steps
under three chunkings; an empty sky against the analytic coefficients; refusals; streams; host queries growing the shared staging buffers behind a held bake; frames do not move; 32-bit descriptors."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import probe_ref as pr
import radiance_ref as rr
from bevyray_amd import _lib
from helpers import big_scene, big_view, cover as _cover, dev as _dev, l1_norm, make_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_host_probe_directions", "brt_host_probe_irradiance", "brt_probe_rays_device", "brt_probe_project_device",
           "brt_bake_probes_device", "brt_bake_probes")
F32 = np.float32
SH9, CUBE = brt.PROBE_SH9, brt.PROBE_AMBIENT_CUBE
PLAIN, STREAM = 1, 2          # values of the knob BRT_RADIANCE_FORM
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
W, H = 96, 54
SKY_BOUND = 1e-3              # |coefficient - analytic| of the N = 1024 sky record (the rule alone: 2.8e-4)
F64_TOLERANCE = 7.5e-7        # 4 x 1.86e-7, see test_the_f32_restatement_against_float64


def _make_probes(positions, seeds):
    positions = np.asarray(positions, F32).reshape(-1, 3)
    probes = np.zeros(len(positions), brt.PROBE_DTYPE)
    probes["position"] = positions
    probes["seed"] = seeds
    return probes


def _sky_record(n=1024, basis=SH9):
    d = brt.probe_directions(n)
    res = np.zeros(n, brt.RADIANCE_DTYPE)
    res["rgb"] = rr.sky_rgb(d)
    res["t"] = np.inf
    return pr.project(res, d, basis)[0]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in EXPORTS:
        assert f"int32_t {name}(" in header, name
        assert name in _lib.EXPORTS, name
        assert f"pub fn {name}(" in rust, name
        assert name in defined, name
    for record in ("pub struct brt_probe {", "pub struct brt_probe_record {"):
        assert record in rust, record
    assert _lib.load().brt_abi_version() == 6
    assert brt.PROBE_DTYPE.itemsize == 16 and brt.PROBE_RECORD_DTYPE.itemsize == 128
    assert [brt.PROBE_DTYPE.fields[f][1] for f in ("position", "seed")] == [0, 12]
    assert [brt.PROBE_RECORD_DTYPE.fields[f][1] for f in ("coeff", "hits", "status", "n_dirs", "basis", "reserved")] == [0, 108, 112, 116, 120, 124]
    assert (SH9, CUBE) == (0, 1) and "#define BRT_PROBE_SH9 0u" in header and "#define BRT_PROBE_AMBIENT_CUBE 1u" in header


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 65536])
def test_the_direction_table(n):
    d = brt.probe_directions(n)
    assert d.shape == (n, 3) and d.dtype == F32
    d64 = pr.directions64(n)
    k = np.arange(n, dtype=np.float64)
    assert np.array_equal(d[:, 1].view(np.uint32), (1.0 - (2.0 * k + 1.0) / n).astype(F32).view(np.uint32))
    for axis in (0, 2):
        ulp = np.spacing(np.maximum(np.abs(d[:, axis]), np.abs(d64[:, axis]).astype(F32))).astype(np.float64)
        assert (np.abs(d[:, axis].astype(np.float64) - d64[:, axis]) <= ulp).all(), axis
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 2e-7


def test_direction_counts_out_of_range_are_refused():
    lib = _lib.load()
    buf = np.zeros(3, F32)
    p = buf.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    assert lib.brt_host_probe_directions(0, p) == INVALID
    assert lib.brt_host_probe_directions(65537, p) == INVALID
    assert lib.brt_host_probe_directions(1, None) == INVALID
    assert (buf == 0).all()
    for n in (0, 65537):
        with pytest.raises(brt.BrtError):
            brt.probe_directions(n)


def test_the_restatement_projects_the_closed_form_sky():
    rec = _sky_record(1024, SH9)
    err = np.abs(rec["coeff"].reshape(9, 3).astype(np.float64) - pr.sky_sh9_analytic()).max()
    print(f"N = 1024 sky, largest |coefficient - analytic|: {err:.3e}")
    assert err <= SKY_BOUND / 2          # (the bound stands only while the restatement's own error is at most half of it)
    assert rec["hits"] == 0 and rec["status"] == 0 and rec["n_dirs"] == 1024 and rec["basis"] == SH9 and rec["reserved"] == 0
    for n in (1, 2, 3, 64, 1000):
        d = brt.probe_directions(n)
        res = np.zeros(2 * n, brt.RADIANCE_DTYPE)
        res["rgb"][:n], res["rgb"][n:] = np.sqrt(F32(0.37)), F32(0.9)
        cube = pr.project(res, d, CUBE)
        den = pr.cube_weights(d).sum(axis=0)
        for p, value in enumerate((float(np.sqrt(F32(0.37)) * np.sqrt(F32(0.37))), float(F32(0.9) * F32(0.9)))):
            faces = cube["coeff"][p][:18].reshape(6, 3)
            assert np.abs(faces[den > 0] - value).max() <= 1e-6, (n, p)
            assert (faces[den == 0] == 0).all() and (cube["coeff"][p][18:] == 0).all()
        if n >= 64:
            assert (den > 0).all()


def test_the_f32_restatement_against_float64():
    """Random colours in [0, 4], N in {64, 1000, 65536}, both bases, four probes each: the largest |f32 - float64| coefficient relative to
    the case's largest |coefficient| measured 1.86e-7 (N = 65536, ambient cube); the tolerance is 4 x that, 7.5e-7."""
    rng = np.random.default_rng(31)
    worst = 0.0
    for n in (64, 1000, 65536):
        d = brt.probe_directions(n)
        for basis in (SH9, CUBE):
            res = np.zeros(4 * n, brt.RADIANCE_DTYPE)
            res["rgb"] = rng.uniform(0, 4, size=(4 * n, 3)).astype(F32)
            rec = pr.project(res, d, basis)
            r64 = pr.project64(res["rgb"].reshape(4, n, 3), d, basis)
            rel = np.abs(rec["coeff"] - r64).max() / np.abs(r64).max()
            print(f"N {n} basis {basis}: {rel:.3e}")
            worst = max(worst, rel)
    assert worst <= F64_TOLERANCE


def test_host_irradiance_against_numpy():
    rng = np.random.default_rng(32)
    normals = rng.normal(size=(24, 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(F32)
    normals[:3] = np.eye(3, dtype=F32)
    normals[3:6] = -np.eye(3, dtype=F32)
    for basis in (SH9, CUBE):
        recs = np.zeros(8, brt.PROBE_RECORD_DTYPE)
        recs["basis"] = basis
        coeff = rng.uniform(-0.2, 0.2, size=(8, 27)).astype(F32)
        coeff[:, :3] = rng.uniform(1.0, 4.0, size=(8, 3))           # (a positive constant term: E stays away from 0)
        if basis == CUBE:
            coeff = rng.uniform(0.1, 4.0, size=(8, 27)).astype(F32)
            coeff[:, 18:] = 0
        recs["coeff"] = coeff
        for rec in recs:
            for n in normals:
                got, want = brt.probe_irradiance(rec, n), pr.irradiance64(rec, n)
                assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all(), (basis, n, got, want)
    sky = _sky_record(1024, SH9)
    A, B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])
    for n in normals:
        got, want = brt.probe_irradiance(sky, n), pr.irradiance64(sky, n)
        assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all()
        assert np.abs(got - (np.pi * A + (2.0 * np.pi / 3.0) * B * float(n[1]))).max() <= 2e-3, n
    bad = np.zeros(1, brt.PROBE_RECORD_DTYPE)
    bad["basis"] = 2
    with pytest.raises(brt.BrtError):
        brt.probe_irradiance(bad[0], normals[0])


def test_rejections_that_need_no_device():
    lib = _lib.load()
    probes = np.zeros(1, brt.PROBE_DTYPE)
    out = np.zeros(1, brt.PROBE_RECORD_DTYPE)
    p, o = probes.ctypes.data, out.ctypes.data
    assert lib.brt_bake_probes(None, p, 1, 64, 1, SH9, 0.0, o, None) == INVALID
    assert lib.brt_bake_probes_device(None, p, 1, 64, 1, SH9, 0.0, o, None, 0, None) == INVALID
    assert lib.brt_probe_rays_device(None, p, 1, 64, o, None, 0) == INVALID
    assert lib.brt_probe_project_device(None, p, 1, 64, SH9, o, None, 0) == INVALID
    assert b"null" in lib.brt_last_error(None)
    f3 = np.zeros(3, F32).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    assert lib.brt_host_probe_irradiance(None, f3, f3) == INVALID
    assert lib.brt_host_probe_irradiance(o, None, f3) == INVALID
    assert lib.brt_host_probe_irradiance(o, f3, None) == INVALID


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _gen_rays(plugin, probes, n_dirs, stream=None):
    import torch
    d_probes = _dev(probes)
    d_rays = torch.full((len(probes) * n_dirs * 32 + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    plugin.node.probe_rays_device(d_probes.data_ptr(), len(probes), n_dirs, d_rays.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = d_rays.cpu().numpy()
    assert (got[-32:] == 0xAB).all()
    return got[:-32].view(brt.RADIANCE_RAY_DTYPE)


def _project(plugin, results, n_probes, n_dirs, basis):
    """The projection step on a host list; the record behind the output is a guard."""
    import torch
    d_res = _dev(results)
    d_out = torch.full(((n_probes + 1) * 128,), 0xCD, dtype=torch.uint8, device="cuda")
    plugin.node.probe_project_device(d_res.data_ptr(), n_probes, n_dirs, basis, d_out.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n_probes * 128:] == 0xCD).all(), "the guard record was written"
    return got[: n_probes * 128].view(brt.PROBE_RECORD_DTYPE)


def _bake(plugin, probes, n_dirs, bounces, basis, form=None, device=False, stream=None, origin_bound=0.0, **knobs):
    import torch
    if form is not None:
        knobs["BRT_RADIANCE_FORM"] = form
    with plugin.tuning(**knobs):
        if not device:
            out = plugin.node.bake_probes(probes, n_dirs, bounces, basis, origin_bound)
        else:
            d_probes = _dev(probes)
            d_out = torch.full((len(probes) * 128 + 128,), 0xCD, dtype=torch.uint8, device="cuda")
            plugin.node.bake_probes((d_probes.data_ptr(), len(probes), d_out.data_ptr()), n_dirs, bounces, basis, origin_bound, device=True,
                                    stream=stream)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[-128:] == 0xCD).all(), "the guard record was written"
            out = got[:-128].view(brt.PROBE_RECORD_DTYPE)
        if form is not None:
            assert plugin.node.last_probe_stats["form"] == form - 1
    return out


def _steps(plugin, probes, n_dirs, bounces, basis):
    """The bake as its three steps: generate, brt_radiance_rays_device with samples = 1, project."""
    import torch
    n = len(probes) * n_dirs
    d_probes = _dev(probes)
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(len(probes) * 128, dtype=torch.uint8, device="cuda")
    plugin.node.probe_rays_device(d_probes.data_ptr(), len(probes), n_dirs, d_rays.data_ptr())
    plugin.node.radiance_rays((d_rays.data_ptr(), n, d_res.data_ptr()), 1, bounces, device=True)
    rad = dict(plugin.node.last_radiance_stats)
    plugin.node.probe_project_device(d_res.data_ptr(), len(probes), n_dirs, basis, d_out.data_ptr())
    torch.cuda.synchronize()
    return _host(d_out, brt.PROBE_RECORD_DTYPE), rad


@functools.lru_cache(maxsize=None)
def _cover_camera():
    return brt.cover_camera(W, H, 2, 4)


def _clear_of_spheres(models, p, margin):
    dist = np.linalg.norm(models["position"].astype(np.float64) - np.asarray(p, np.float64)[None, :], axis=1)
    return bool((dist > models["radius"] + margin).all())


@functools.lru_cache(maxsize=None)
def _cover_probes():
    """High above the scene, between the small spheres, inside the glass sphere, on the ground plane."""
    b = _cover()
    m, mats = b.models, b.materials
    small = m["radius"] < 0.5
    rng = np.random.default_rng(41)
    between = next(p for p in rng.uniform((-4, 0.2, -4), (4, 0.2, 4), size=(200, 3))
                   if _clear_of_spheres(m, p, 0.05) and np.sort(np.linalg.norm(m["position"][small] - p[None, :], axis=1))[1] < 1.2)
    glass = next(i for i in range(len(m)) if m["radius"][i] == 1.0 and mats[m["material_id"][i]]["specular_transmission"] > 0)
    ground = next(p for p in rng.uniform((-4, 0.0, -4), (4, 0.0, 4), size=(200, 3)) if _clear_of_spheres(m[m["radius"] < 100], p, 0.05))
    return _make_probes([(0.0, 30.0, 0.0), between, m["position"][glass], ground], [7, 0xFFFFFFF0, 123456789, 0])


_TREES = {}


def _upload_cover(plugin, tree):
    """The cover scene under the caller's PLOC tree, or under the callee's SAH tree with its reach raised (by a bake's origin_bound) to
    cover the probes.  -> (Buffers with the tree the GPU walks, the key of that tree)."""
    b = _cover()
    if tree == "caller":
        plugin.node.write_buffers(b)
        return b, "caller"
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    plugin.node.bake_probes(_cover_probes()[:1], 1, 0, SH9, origin_bound=40.0)
    reach = plugin.node.last_probe_stats["tree_reach"]
    assert plugin.node.query_origin_bound() >= 40.0
    key = f"callee@{reach!r}"
    _TREES.setdefault(key, brt.build_bvh_sah(b.models, reach))
    return brt.Buffers(b.models, b.materials, _TREES[key]), key


@functools.lru_cache(maxsize=None)
def _want_results(key, bounces, n_dirs=81):
    """radiance_ref's results and counts of the cover probes' entries under the tree `key`: once per module."""
    b = _cover()
    bvh = b.bvh if key == "caller" else _TREES[key]
    rays = pr.make_rays(_cover_probes(), brt.probe_directions(n_dirs))
    return rr.expected(b.models, b.materials, bvh, _cover_camera()[1], rays, 1, bounces)


@pytest.mark.gpu
def test_generated_rays_are_the_restatements(plugin):
    rng = np.random.default_rng(42)
    for n_probes in (1, 3, 64, 65):
        probes = _make_probes(rng.uniform(-50, 50, size=(n_probes, 3)), rng.integers(0, 2 ** 32, size=n_probes, dtype=np.uint32))
        probes["seed"][0] = 0xFFFFFFFF                                    # (the seeds wrap)
        if n_probes >= 3:
            probes["position"][1] = (np.nan, 1.0, -np.inf)
            probes["position"][2] = (np.inf, -0.0, 1e-42)
            probes["position"].view(np.uint32)[1, 0] = 0x7FC12345        # (a NaN with a payload: copied as bits)
        for n_dirs in (1, 2, 63, 64, 65, 256, 1000):
            got = _gen_rays(plugin, probes, n_dirs)
            want = pr.make_rays(probes, brt.probe_directions(n_dirs))
            assert got.tobytes() == want.tobytes(), (n_probes, n_dirs)


def _synthetic(n_probes, n_dirs, kind, rng):
    res = np.zeros((n_probes, n_dirs), brt.RADIANCE_DTYPE)
    res["rgb"] = rng.uniform(0, 2, size=(n_probes, n_dirs, 3)).astype(F32)
    res["t"] = rng.uniform(0.1, 9, size=(n_probes, n_dirs)).astype(F32)
    res["status"] = rng.integers(0, 2, size=(n_probes, n_dirs)) * 3       # miss, or hit | front face
    res["user"] = np.arange(n_dirs, dtype=np.uint32)[None, :]
    pick = rng.integers(0, n_dirs, size=n_probes)
    rows = np.arange(n_probes)
    if kind == "uniform":
        res["rgb"] = F32(0.8)
    elif kind == "nan":
        res["rgb"][rows, pick, 1] = np.nan
    elif kind == "inf":
        res["rgb"][rows, pick, 0] = np.inf
    elif kind == "overflow":
        res["rgb"][rows, pick, 2] = F32(3e38)
    elif kind == "negzero":
        res["rgb"] = F32(-0.0)
    elif kind == "denormal":
        res["rgb"] = rng.uniform(1e-23, 3e-19, size=(n_probes, n_dirs, 3)).astype(F32)     # (squares from below the denormals up into the normals)
        res["rgb"][:, ::3] = F32(1e-42)
    elif kind == "statuses":
        res["status"] = rng.choice(np.array([0, 1, 3, 4, 8, 12], np.uint32), size=(n_probes, n_dirs))
        res["status"][0, 0] = 0
        if n_probes > 1:
            res["status"][1, 0] = brt.QUERY_STATUS_INVALID
            res["status"][2, 0] = brt.QUERY_STATUS_OUT_OF_REACH
            res["status"][3, 0] = 3
    return res.reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("basis", [SH9, CUBE])
@pytest.mark.parametrize("n_dirs", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 65536])
def test_projection_of_synthetic_lists(plugin, n_dirs, basis):
    rng = np.random.default_rng(43 + n_dirs)
    dirs = brt.probe_directions(n_dirs)
    for n_probes in (1, 5):
        for kind in ("uniform", "nan", "inf", "overflow", "negzero", "denormal", "statuses"):
            res = _synthetic(n_probes, n_dirs, kind, rng)
            want = pr.project(res, dirs, basis)
            got = _project(plugin, res, n_probes, n_dirs, basis)
            pr.assert_records_equal(got, want, f"{kind} {n_probes} x {n_dirs} basis {basis}")
            if kind == "nan":
                assert np.isnan(want["coeff"]).any()
            if kind == "statuses" and n_probes > 1:
                assert list(want["status"][:4]) == [0, 4, 8, 0] and (want["coeff"][1:3] == 0).all() and (want["hits"][1:3] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["caller", "callee"])
def test_bakes_on_the_cover_scene_match_the_reference(plugin, tree):
    b, key = _upload_cover(plugin, tree)
    probes, n_dirs = _cover_probes(), 81
    dirs = brt.probe_directions(n_dirs)
    _, counts = _want_results(key, 8)
    print(counts)
    for k in ("metal", "glass", "diffuse", "miss_entries", "hit_entries"):
        assert counts[k] > 0, (k, counts)
    seen = set()
    for bounces in (0, 8):
        res, counts = _want_results(key, bounces)
        for basis in (SH9, CUBE):
            want = pr.project(res, dirs, basis)
            assert not np.isnan(want["coeff"]).any() and (want["status"] == 0).all()
            assert want["hits"].sum() == counts["hit_entries"] and (0 < want["hits"]).all() and (want["hits"] < n_dirs).all()
            for device in (False, True):
                for form in (PLAIN, STREAM):
                    got = _bake(plugin, probes, n_dirs, bounces, basis, form=form, device=device)
                    pr.assert_records_equal(got, want, f"{tree} bounces {bounces} basis {basis} device {device} form {form}")
                    st = plugin.node.last_probe_stats
                    assert (st["walks"], st["hits"], st["refused"], st["chunks"]) == (counts["raycasts"], counts["hit_entries"], 0, 1), st
            seen.add(want["coeff"].tobytes())
    assert len(seen) == 4


def _lattice(n, lo=(-5.0, 0.1, -5.0), hi=(5.0, 3.0, 5.0), seed=1):
    side = int(round(n ** (1.0 / 3.0)))
    assert side ** 3 == n
    g = [np.linspace(lo[a], hi[a], side) for a in range(3)]
    pos = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3)
    return _make_probes(pos, np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed))


@pytest.mark.gpu
def test_one_call_equals_its_three_steps_whatever_the_chunks(plugin):
    _upload_cover(plugin, "caller")
    probes, n_dirs = _lattice(1000), 256
    for basis in (SH9, CUBE):
        want, rad = _steps(plugin, probes, n_dirs, 4, basis)
        assert want["hits"].sum() == rad["hits"] > 0 and (want["status"] == 0).all() and len(set(want["coeff"][:, 0].tolist())) > 500
        for chunk_rays, chunks in ((2000, 143), (100, 1000), (None, 1)):
            knobs = {} if chunk_rays is None else {"BRT_PROBE_CHUNK_RAYS": chunk_rays}
            for device in (True, False) if basis == SH9 else (True,):
                got = _bake(plugin, probes, n_dirs, 4, basis, device=device, **knobs)
                assert got.tobytes() == want.tobytes(), (basis, chunk_rays, device)
                st = plugin.node.last_probe_stats
                assert st["chunks"] == chunks and (st["walks"], st["hits"], st["refused"]) == (rad["walks"], rad["hits"], 0), st
    assert plugin.get_tuning("BRT_PROBE_CHUNK_RAYS") == (1 << 21, 1 << 21)


@pytest.mark.gpu
def test_an_empty_sky_against_the_analytic_coefficients(plugin):
    b = make_buffers([((300.0, 400.0, 500.0), 0.01, brt.StandardMaterial())])
    plugin.node.write_buffers(b)
    probes = _make_probes([(0, 0, 0), (3, -2, 5), (-40, 10, 0.5)], [1, 2, 3])
    recs = _bake(plugin, probes, 1024, 8, SH9)
    assert (recs["hits"] == 0).all() and (recs["status"] == 0).all()
    pr.assert_records_equal(recs, np.repeat(_sky_record(1024, SH9), 3), "the sky's record, whatever the position and the seed")
    A, B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])
    for rec in recs:
        assert np.abs(rec["coeff"].reshape(9, 3) - pr.sky_sh9_analytic()).max() <= SKY_BOUND
        for n in ((0, 1, 0), (0, -1, 0), (0.6, 0.0, 0.8), (-0.48, 0.6, 0.64)):
            e = brt.probe_irradiance(rec, n)
            assert np.abs(e - (np.pi * A + (2.0 * np.pi / 3.0) * B * n[1])).max() <= 2e-3, n
    cube = _bake(plugin, probes, 1024, 8, CUBE)
    pr.assert_records_equal(cube, np.repeat(_sky_record(1024, CUBE), 3), "the sky's ambient cube")
    up, down = cube[0]["coeff"][6:9], cube[0]["coeff"][9:12]
    assert (up[:2] < down[:2]).all() and abs(up[2] - 1.0) < 1e-6          # (the zenith is bluer: less red and green from above)


@pytest.mark.gpu
def test_refused_probes_and_reach(plugin):
    b, key = _upload_cover(plugin, "callee")
    bound = plugin.node.query_origin_bound()
    assert 40.0 <= bound < np.inf
    n_dirs = 81
    dirs = brt.probe_directions(n_dirs)
    good = _cover_probes()
    probes = np.concatenate([good[:2], _make_probes([(np.nan, 1.0, 0.0), (0.0, 2.0 * bound, 0.0)], [5, 6]), good[2:]])
    res, _ = _want_results(key, 8)
    want = pr.project(res, dirs, SH9)
    for device in (False, True):
        got = _bake(plugin, probes, n_dirs, 8, SH9, device=device)
        assert list(got["status"]) == [0, 0, brt.QUERY_STATUS_INVALID, brt.QUERY_STATUS_OUT_OF_REACH, 0, 0]
        assert (got["coeff"][2:4].view(np.uint32) == 0).all() and (got["hits"][2:4] == 0).all()
        assert (got["n_dirs"] == n_dirs).all() and (got["basis"] == SH9).all() and (got["reserved"] == 0).all()
        pr.assert_records_equal(got[[0, 1, 4, 5]], want, "neighbours of refused probes")
        assert plugin.node.last_probe_stats["refused"] == 2 * n_dirs
    # a far probe with origin_bound given is answered on a tree of a longer reach, rebuilt once
    far = _make_probes([(13.0 * 60.0, 2.0 * 60.0, 3.0 * 60.0)], [9])
    out = _bake(plugin, far, n_dirs, 8, CUBE)
    assert out["status"][0] == brt.QUERY_STATUS_OUT_OF_REACH and (out["coeff"] == 0).all()
    l1 = l1_norm(far["position"][0])
    got = _bake(plugin, far, n_dirs, 8, CUBE, origin_bound=l1)
    st = plugin.node.last_probe_stats
    assert st["tree_rebuilt"] == 1 and st["tree_reach"] > 0 and plugin.node.query_origin_bound() >= l1
    twin = brt.build_bvh_sah(b.models, st["tree_reach"])
    res_far, _ = rr.expected(b.models, b.materials, twin, _cover_camera()[1], pr.make_rays(far, dirs), 1, 8)
    pr.assert_records_equal(got, pr.project(res_far, dirs, CUBE), "far probe")
    _bake(plugin, far, n_dirs, 8, CUBE, origin_bound=l1)
    assert plugin.node.last_probe_stats["tree_rebuilt"] == 0


@pytest.mark.gpu
def test_refused_calls_leave_the_context_usable(plugin):
    import torch
    _upload_cover(plugin, "caller")
    lib, ctx = plugin._lib, plugin._ctx
    probes, n_dirs = _cover_probes(), 81
    res, _ = _want_results("caller", 8)
    want = pr.project(res, brt.probe_directions(n_dirs), SH9)
    host = np.ascontiguousarray(probes)
    out = np.zeros(len(probes), brt.PROBE_RECORD_DTYPE)
    p, o = host.ctypes.data, out.ctypes.data
    d_buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    d_p, d_o, d_l = d_buf.data_ptr(), d_buf.data_ptr() + 4096, d_buf.data_ptr() + 8192

    def refused(code, call, what):
        assert call() == code, what
        pr.assert_records_equal(_bake(plugin, probes, n_dirs, 8, SH9), want, f"after {what}")

    refused(INVALID, lambda: lib.brt_bake_probes(ctx, p, 4, 0, 8, SH9, 0.0, o, None), "n_dirs 0")
    refused(INVALID, lambda: lib.brt_bake_probes(ctx, p, 4, 65537, 8, SH9, 0.0, o, None), "n_dirs 65537")
    refused(INVALID, lambda: lib.brt_bake_probes_device(ctx, d_p, 4, 0, 8, SH9, 0.0, d_o, None, 0, None), "n_dirs 0, device")
    refused(INVALID, lambda: lib.brt_bake_probes(ctx, p, 4, 81, 65536, SH9, 0.0, o, None), "bounces 65536")
    refused(INVALID, lambda: lib.brt_bake_probes(ctx, p, 4, 81, 8, 2, 0.0, o, None), "basis 2")
    refused(INVALID, lambda: lib.brt_bake_probes_device(ctx, d_p, 4, 81, 8, 2, 0.0, d_o, None, 0, None), "basis 2, device")
    refused(INVALID, lambda: lib.brt_bake_probes_device(ctx, d_p, 4, 81, 8, SH9, 0.0, d_o, None, brt.FLAG_DENOISE, None), "unknown flag")
    refused(INVALID, lambda: lib.brt_bake_probes_device(ctx, d_p, 4, 81, 8, SH9, 0.0, d_p + 48, None, 0, None), "overlapping buffers")
    refused(INVALID, lambda: lib.brt_probe_rays_device(ctx, d_p, 4, 81, d_p + 32, None, 0), "rays over the probes")
    refused(INVALID, lambda: lib.brt_probe_rays_device(ctx, d_p, 4, 0, d_l, None, 0), "step, n_dirs 0")
    refused(INVALID, lambda: lib.brt_probe_rays_device(ctx, d_p, 0x7FFF0000 // 64 + 1, 64, d_l, None, 0), "step, list too long")
    refused(INVALID, lambda: lib.brt_probe_rays_device(ctx, d_p, 4, 81, d_l, None, brt.FLAG_COUNTERS), "step, unknown flag")
    refused(INVALID, lambda: lib.brt_probe_project_device(ctx, d_l, 4, 81, SH9, d_l + 128, None, 0), "records over the results")
    refused(INVALID, lambda: lib.brt_probe_project_device(ctx, d_l, 4, 81, 2, d_o, None, 0), "step, basis 2")
    refused(INVALID, lambda: lib.brt_probe_project_device(ctx, d_l, 4, 65537, SH9, d_o, None, 0), "step, n_dirs 65537")
    refused(INVALID, lambda: lib.brt_probe_project_device(ctx, d_l, 0x7FFF0000 // 64 + 1, 64, SH9, d_o, None, 0), "step, list too long")
    assert lib.brt_bake_probes(ctx, None, 4, 81, 8, SH9, 0.0, o, None) == INVALID
    assert lib.brt_bake_probes(ctx, p, 4, 81, 8, SH9, 0.0, None, None) == INVALID
    assert lib.brt_bake_probes(ctx, p, 4, 81, 8, SH9, float("nan"), o, None) == INVALID
    assert lib.brt_bake_probes(ctx, p, 4, 81, 8, SH9, -1.0, o, None) == INVALID
    assert lib.brt_probe_rays_device(ctx, None, 4, 81, d_l, None, 0) == INVALID
    assert lib.brt_probe_project_device(ctx, d_l, 4, 81, SH9, None, None, 0) == INVALID
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert lib.brt_bake_probes(ctx, p, 4, 81, 8, SH9, 0.0, o, None) == UNSUPPORTED
        assert lib.brt_bake_probes_device(ctx, d_p, 4, 81, 8, SH9, 0.0, d_o, None, 0, None) == UNSUPPORTED
    finally:
        plugin.set_policy(0)
    # no probes: OK, nothing launched
    assert plugin.node.bake_probes(np.zeros(0, brt.PROBE_DTYPE), 81, 8).shape == (0,)
    assert plugin.node.last_probe_stats["chunks"] == 0
    pr.assert_records_equal(_bake(plugin, probes, n_dirs, 8, SH9), want, "after the refusals")
    with brt.RaytracePlugin([0]) as empty:
        with pytest.raises(brt.BrtError) as e:
            empty.node.bake_probes(probes, n_dirs, 8)
        assert e.value.code == NO_SCENE
        with pytest.raises(brt.BrtError) as e:
            empty.node.bake_probes((d_p, 4, d_o), n_dirs, 8, device=True)
        assert e.value.code == NO_SCENE
        empty.node.write_buffers(_cover())
        pr.assert_records_equal(empty.node.bake_probes(probes, n_dirs, 8), want, "after no scene")


@pytest.mark.gpu
def test_bakes_on_two_caller_streams_and_across_an_upload(plugin):
    import torch
    b, _ = _upload_cover(plugin, "caller")
    probes = _lattice(216)
    serial = {n: _bake(plugin, probes, n, 4, SH9, device=True).copy() for n in (64, 100)}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_probes = _dev(probes)
    d_out = {n: torch.zeros(len(probes) * 128, dtype=torch.uint8, device="cuda") for n in (64, 100)}
    torch.cuda.synchronize()

    def both():
        for n, s in ((64, s1), (100, s2)):
            st = plugin.node.bake_probes((d_probes.data_ptr(), len(probes), d_out[n].data_ptr()), n, 4, SH9, device=True, stream=s.cuda_stream)
            assert (st["walks"], st["hits"], st["refused"], st["chunks"]) == (0, 0, 0, 1)

    both()
    torch.cuda.synchronize()
    for n in (64, 100):
        assert _host(d_out[n], brt.PROBE_RECORD_DTYPE).tobytes() == serial[n].tobytes(), n
    # ... and with a scene upload between them: the first sees the old scene, the second the new one
    moved = b.models.copy()
    big = np.flatnonzero(moved["radius"] == 1.0)
    moved["position"][big] += np.array([0.0, 0.6, 0.0], F32)
    b2 = brt.Buffers(moved, b.materials, brt.build_bvh(moved))
    for t in d_out.values():
        t.zero_()
    torch.cuda.synchronize()
    plugin.node.bake_probes((d_probes.data_ptr(), len(probes), d_out[64].data_ptr()), 64, 4, SH9, device=True, stream=s1.cuda_stream)
    plugin.node.write_buffers(b2)
    plugin.node.bake_probes((d_probes.data_ptr(), len(probes), d_out[100].data_ptr()), 100, 4, SH9, device=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert _host(d_out[64], brt.PROBE_RECORD_DTYPE).tobytes() == serial[64].tobytes()
    after = _host(d_out[100], brt.PROBE_RECORD_DTYPE)
    assert after.tobytes() == _bake(plugin, probes, 100, 4, SH9, device=True).tobytes()
    assert after.tobytes() != serial[100].tobytes()


def _list_rays(n, dtype, seed):
    """n rays from inside the cover scene's box of probes, in the ray queries' or the radiance queries' record"""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype)
    rays["origin"] = rng.uniform((-5.0, 0.1, -5.0), (5.0, 3.0, 5.0), size=(n, 3)).astype(F32)
    d = rng.normal(size=(n, 3))
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    rays["user"] = np.arange(n, dtype=np.uint32)
    if "seed" in dtype.names:
        rays["seed"] = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    else:
        rays["t_max"] = np.inf
    return rays


@pytest.mark.gpu
def test_host_queries_behind_a_held_bake_grow_the_shared_staging_buffers(plugin):
    """d_qrays / d_qhits serve three families.  A device bake of 27 probes x 64 directions in chunks of 640 entries (three chunks, each
    staged in the pair: 20 480 bytes) is held on a caller's stream of a new context; with no host synchronisation the host ray query then
    stages 5 000 rays (160 000 bytes: the pair grows behind the held bake) and the host radiance query 1 234 entries (no growth).  The
    smallest sizes at which the new context must allocate and the bake must chunk.  Expectations: the same three calls one at a time on
    the module's context, whose buffers other tests have grown already."""
    import torch
    b, _ = _upload_cover(plugin, "caller")
    probes = _lattice(27)
    q_rays, r_rays = _list_rays(5000, brt.RAY_DTYPE, 61), _list_rays(1234, brt.RADIANCE_RAY_DTYPE, 62)
    want_bake = _bake(plugin, probes, 64, 4, SH9, device=True, BRT_PROBE_CHUNK_RAYS=640).copy()
    assert plugin.node.last_probe_stats["chunks"] == 3
    want_q = plugin.node.query_rays(q_rays).copy()
    want_r = plugin.node.radiance_rays(r_rays, 2, 4).copy()
    assert 0 < np.isfinite(want_q["t"]).sum() < 5000 and 0 < np.isfinite(want_r["t"]).sum() < 1234 and (want_r["rgb"] > 0).any()
    d_probes = _dev(probes)
    d_out = torch.zeros(len(probes) * 128, dtype=torch.uint8, device="cuda")
    sa = torch.cuda.Stream()
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.node.write_buffers(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                       # (a few ms: the held bake starts after the later calls have been made)
        with fresh.tuning(BRT_PROBE_CHUNK_RAYS=640):
            st = fresh.node.bake_probes((d_probes.data_ptr(), len(probes), d_out.data_ptr()), 64, 4, SH9, device=True, stream=sa.cuda_stream)
        assert st["chunks"] == 3
        got_q = fresh.node.query_rays(q_rays)
        assert got_q.tobytes() == want_q.tobytes() and fresh.node.last_query_stats["rays_walked"] == 5000
        got_r = fresh.node.radiance_rays(r_rays, 2, 4)                # (no growth: the buffers are reused)
        assert got_r.tobytes() == want_r.tobytes() and fresh.node.last_radiance_stats["refused"] == 0
        torch.cuda.synchronize()
        assert _host(d_out, brt.PROBE_RECORD_DTYPE).tobytes() == want_bake.tobytes()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_frames_do_not_move(plugin):
    b = _cover()
    w, h = 320, 180
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
    before = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=brt.FLAG_COUNTERS).copy()
    stats_before = dict(plugin.node.last_stats)
    probes = _lattice(125)
    for basis in (SH9, CUBE):
        _bake(plugin, probes, 96, 4, basis)
        _bake(plugin, probes, 96, 4, basis, device=True, BRT_PROBE_CHUNK_RAYS=1000)
    after = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for k in ("rays", "node_pops", "interior_visits", "sphere_tests", "hits", "kernel_variant", "n_workgroups", "scene_in_lds"):
        assert plugin.node.last_stats[k] == stats_before[k], k


@pytest.mark.gpu
def test_a_scene_with_32_bit_descriptors(plugin):
    s = big_scene(16383, 11)
    b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models))
    lvl, cam, win = big_view(W, H)
    plugin.node.run(lvl, cam, win, W, H, buffers=b)
    assert plugin.node.last_stats["scene_in_lds"] == 0
    centre = b.models["position"].astype(np.float64).mean(axis=0)
    rng = np.random.default_rng(44)
    probes = _make_probes(centre[None, :] + rng.uniform(-2, 2, size=(48, 3)), rng.integers(0, 2 ** 32, size=48, dtype=np.uint32))
    for basis in (SH9, CUBE):
        want, rad = _steps(plugin, probes, 128, 4, basis)
        assert rad["hits"] > 0 and rad["form"] == 0
        got = _bake(plugin, probes, 128, 4, basis, device=True, BRT_PROBE_CHUNK_RAYS=128 * 10)
        assert got.tobytes() == want.tobytes()
        st = plugin.node.last_probe_stats
        assert st["form"] == 0 and st["chunks"] == 5 and (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])     # (no LDS form: the plain kernel)
        with plugin.tuning(BRT_RADIANCE_FORM=STREAM):
            assert plugin.node.bake_probes(probes, 128, 4, basis).tobytes() == want.tobytes()
            assert plugin.node.last_probe_stats["form"] == 1
