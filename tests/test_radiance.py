"""Radiance queries (brt_radiance_rays*, DESIGN.md "Radiance queries"): path-traced colour for lists of the caller's rays.  CPU: the
exports, argument rejections, the reference (tests/radiance_ref.py: the numpy restatement of the shader) against the closed-form sky,
its independence of the list's order, and that the standard ray set reaches every class of segment.  GPU: every result bitwise against
that reference on the tree the GPU walked, both kernel forms, both entry points; the walk count; list lengths; long lists against ray
queries and the sky; refusals; streams; frames do not move; seeds."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import radiance_ref as rr
from bevyray_amd import _lib
from helpers import big_scene, big_view, l1_norm, single_leaf_bvh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_radiance_rays_device", "brt_radiance_rays")
F32 = np.float32
PLAIN, STREAM = 1, 2          # values of the knob BRT_RADIANCE_FORM
W, H = 96, 54
SAMPLES, BOUNCES = (1, 4), (0, 1, 8)
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7


@functools.lru_cache(maxsize=None)
def _cover():
    return brt.generate_scene(brt.SCENE_COVER, 1)


@functools.lru_cache(maxsize=None)
def _cover_camera():
    return brt.cover_camera(W, H, 2, 4)


@functools.lru_cache(maxsize=None)
def _standard():
    return rr.standard_rays(_cover_camera()[1][0]["position"])


_TREES = {}       # name -> the node array the reference walks (the callee's twin is known once the GPU has built its tree)


@functools.lru_cache(maxsize=None)
def _want(tree, samples, bounces):
    """The reference's records and counts of the standard set on the cover scene under `tree`: once per module."""
    b = _cover()
    bvh = b.bvh if tree == "caller" else _TREES[tree]
    return rr.expected(b.models, b.materials, bvh, _cover_camera()[1], _standard(), samples, bounces)


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
    for record in ("pub struct brt_radiance_ray {", "pub struct brt_radiance_result {"):
        assert record in rust, record
    assert _lib.load().brt_abi_version() == 6
    assert brt.RADIANCE_RAY_DTYPE.itemsize == 32 and brt.RADIANCE_DTYPE.itemsize == 32
    assert [brt.RADIANCE_RAY_DTYPE.fields[f][1] for f in ("origin", "seed", "direction", "user")] == [0, 12, 16, 28]
    assert [brt.RADIANCE_DTYPE.fields[f][1] for f in ("t", "rgb", "sphere", "material", "status", "user")] == [0, 4, 16, 20, 24, 28]


def test_rejections_that_need_no_device():
    lib = _lib.load()
    rays = np.zeros(1, brt.RADIANCE_RAY_DTYPE)
    out = np.zeros(1, brt.RADIANCE_DTYPE)
    assert lib.brt_radiance_rays(None, rays.ctypes.data, 1, 1, 1, 0.0, out.ctypes.data, None) == INVALID
    assert lib.brt_radiance_rays_device(None, rays.ctypes.data, 1, 1, 1, 0.0, out.ctypes.data, None, 0, None) == INVALID
    assert b"null" in lib.brt_last_error(None)


def test_a_miss_rays_reference_colour_is_the_closed_form_sky():
    b = _cover()
    rng = np.random.default_rng(5)
    d = rng.normal(size=(40, 3)).astype(F32)
    d[:, 1] = np.abs(d[:, 1]) + F32(0.05)                               # upwards from above the scene: nothing to hit
    d[:8] *= (10.0 ** rng.uniform(-20, 20, size=8)).astype(F32)[:, None]   # (unnormalised: the gradient normalises)
    rays = rr.make_rays(np.broadcast_to(np.array([0.0, 30.0, 0.0], F32), d.shape), d, rng.integers(0, 2 ** 32, size=len(d), dtype=np.uint32))
    want, counts = rr.expected(b.models, b.materials, b.bvh, _cover_camera()[1], rays, 1, 8)
    assert counts["miss_entries"] == len(rays) and counts["raycasts"] == len(rays)
    assert (want["status"] == brt.QUERY_STATUS_MISS).all() and np.isposinf(want["t"]).all()
    assert np.array_equal(want["rgb"].view(np.uint32), rr.sky_rgb(d).view(np.uint32))
    # straight up and along the horizon: sqrt of the gradient's two ends
    ends = rr.sky_rgb(np.array([[0, 2, 0], [3, 0, 0]], F32))
    assert np.array_equal(ends[0], np.sqrt(np.array([0.5, 0.7, 1.0], F32), dtype=F32))
    assert np.array_equal(ends[1], np.sqrt(np.array([0.75, 0.85, 1.0], F32), dtype=F32))


def test_the_reference_does_not_depend_on_the_lists_order():
    want, _ = _want("caller", 4, 8)
    perm = np.random.default_rng(9).permutation(len(want))
    b = _cover()
    shuffled, _ = rr.expected(b.models, b.materials, b.bvh, _cover_camera()[1], _standard()[perm], 4, 8)
    assert shuffled.tobytes() == want[perm].tobytes()


def test_the_standard_set_reaches_every_class():
    _, counts = _want("caller", 4, 8)
    print(counts)
    for k in ("metal", "glass", "diffuse", "absorbed", "bounce_limit", "miss_entries", "hit_entries"):
        assert counts[k] > 0, (k, counts)
    assert counts["miss_entries"] + counts["hit_entries"] == len(_standard()) == 96


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def _radiance(plugin, rays, samples, bounces, form, device=False, stream=None, origin_bound=0.0):
    """The list through the host-buffer or the device-buffer entry point, the kernel form forced by the knob."""
    import torch
    with plugin.tuning(BRT_RADIANCE_FORM=form):
        if not device:
            out = plugin.node.radiance_rays(rays, samples, bounces, origin_bound)
        else:
            d_rays = _dev(rays)
            d_out = torch.full((max(1, rays.size) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
            plugin.node.radiance_rays((d_rays.data_ptr() if rays.size else 0, rays.size, d_out.data_ptr() if rays.size else 0), samples, bounces,
                                      origin_bound, device=True, stream=stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()[: rays.size * 32].view(brt.RADIANCE_DTYPE)
        assert plugin.node.last_radiance_stats["form"] == form - 1 or rays.size == 0
    return out


def _same_bytes(a, b, what):
    assert a.tobytes() == b.tobytes(), what


def _walks_expected(want, counts, samples):
    """The reference walks an entry's own ray once per sample; the kernels once per entry."""
    return counts["raycasts"] - (samples - 1) * len(want)


def _check_against(plugin, rays, want, counts, models, samples, bounces, what):
    """Plain form, host buffers against the reference (fields, spheres, counts); the other three ways byte for byte against it."""
    got = _radiance(plugin, rays, samples, bounces, PLAIN)
    rr.assert_equal(got, want, f"{what} plain")
    rr.check_spheres(models, rays, got)
    for form, device in ((PLAIN, False), (STREAM, False), (PLAIN, True), (STREAM, True)):
        if (form, device) != (PLAIN, False):
            _same_bytes(_radiance(plugin, rays, samples, bounces, form, device=device), got, f"{what} form {form} device {device}")
        st = plugin.node.last_radiance_stats
        assert (st["walks"], st["hits"], st["refused"]) == (_walks_expected(want, counts, samples), counts["hit_entries"], 0), (what, form, device, st)
    return got


def _upload_cover(plugin, tree):
    """The cover scene resident under the caller's PLOC tree, or under the callee's SAH tree with its reach raised to cover the set, and
    one frame of the cover camera rendered.  -> (Buffers with the tree the GPU walks, the key of that tree for _want)."""
    b = _cover()
    lvl, cam, win = _cover_camera()
    if tree == "caller":
        plugin.node.run(lvl, cam, win, W, H, buffers=b)
        return b, "caller"
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    plugin.node.radiance_rays(_standard()[:1], 1, 0, origin_bound=20.0)      # (the set's origins have a 1-norm below 8 + 3 + 8)
    plugin.node.run(lvl, cam, win, W, H)
    reach = plugin.node.last_stats["tree_reach"]
    key = f"callee@{reach!r}"
    _TREES.setdefault(key, brt.build_bvh_sah(b.models, reach))
    assert plugin.node.query_origin_bound() >= 20.0
    return brt.Buffers(b.models, b.materials, _TREES[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["caller", "callee"])
def test_the_standard_set_matches_the_reference(plugin, tree):
    b, key = _upload_cover(plugin, tree)
    assert plugin.node.last_stats["scene_in_lds"] == 1                   # LDS-resident
    rays = _standard()
    seen = {}
    for samples in SAMPLES:
        for bounces in BOUNCES:
            want, counts = _want(key, samples, bounces)
            got = _check_against(plugin, rays, want, counts, b.models, samples, bounces, f"{tree} {samples} x {bounces}")
            seen[samples, bounces] = got["rgb"].tobytes()
    # every pair of parameters is its own image, but for bounces = 0: a sample is then the sky's colour or black, whatever the draws
    assert seen[1, 0] == seen[4, 0] and len(set(seen.values())) == len(seen) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stress_lds_top", "desc32_global"])
def test_scenes_beyond_the_lds(plugin, case):
    """The stress grid (top of the tree in LDS, spheres renumbered by the hot order) and a 16 383-sphere scene (32-bit descriptors, the
    scene in global memory): 64 rays against the reference, the path that ran asserted from the stats."""
    if case == "stress_lds_top":
        from test_query import _scene
        b, cam, win, _ = _scene(plugin, "stress")                          # (asserts scene_in_lds == 2 and hot_records > 0)
        targets = b.models["position"][np.random.default_rng(4).integers(0, len(b.models), size=64)]
        lds = 2
    else:
        s = big_scene(16383, 11)
        b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models))
        lvl, cam, win = big_view(W, H)
        plugin.node.run(lvl, cam, win, W, H, buffers=b)
        targets = b.models["position"][np.random.default_rng(4).integers(0, len(b.models), size=64)]
        lds = 0
    st = plugin.node.last_stats
    print(f"{case}: scene_in_lds {st['scene_in_lds']}, hot_records {st['hot_records']}")
    assert st["scene_in_lds"] == lds and (lds == 2 or st["hot_records"] == 0)
    rng = np.random.default_rng(6)
    o = np.broadcast_to(cam[0]["position"].astype(F32), (64, 3)).copy()
    d = (targets + rng.uniform(-0.3, 0.3, size=(64, 3)) - o).astype(F32)
    o[1::4] = (targets[1::4] + rng.uniform(-2, 2, size=(16, 3))).astype(F32)      # a quarter from inside the scene, anywhere
    d[1::4] = rng.normal(size=(16, 3)).astype(F32)
    rays = rr.make_rays(o, d, rng.integers(0, 2 ** 32, size=64, dtype=np.uint32))
    bound = plugin.node.query_origin_bound()
    rays = rays[np.array([l1_norm(r) for r in rays["origin"]]) <= bound]
    assert len(rays) >= 48
    want, counts = rr.expected(b.models, b.materials, b.bvh, cam, rays, 2, 4)
    assert counts["hit_entries"] > 8 and counts["raycasts"] > 2 * len(rays)
    _check_against(plugin, rays, want, counts, b.models, 2, 4, case)
    # the default rule: a list too short to stream takes the plain form; a long one streams only where the scene has an LDS form
    long_list = np.tile(rays, 1 + 1024 // len(rays))
    plugin.node.radiance_rays(rays, 1, 0)
    assert plugin.node.last_radiance_stats["form"] == 0
    plugin.node.radiance_rays(long_list, 1, 0)
    assert plugin.node.last_radiance_stats["form"] == (1 if lds else 0)
    if lds:
        assert plugin.node.last_radiance_stats["n_workgroups"] == -(-len(long_list) // 1024)
    with plugin.tuning(BRT_RADIANCE_FORM=STREAM):                        # forced, a global scene streams in 256-thread workgroups
        plugin.node.radiance_rays(long_list, 1, 0)
        assert plugin.node.last_radiance_stats["n_workgroups"] == -(-len(long_list) // (1024 if lds else 256))


@pytest.mark.gpu
def test_a_tree_deeper_than_the_stack(plugin):
    """raytrace.wgsl:320: a 40-deep caterpillar overflows the 32-entry stack and drops subtrees; both forms follow the rule (the plain
    form's stack is a column of LDS, the streaming form's a column of the wave's array)."""
    from test_query import _scene
    b, cam, win, _ = _scene(plugin, "overflow")
    rng = np.random.default_rng(8)
    targets = b.models["position"][rng.integers(0, len(b.models), size=48)] + rng.uniform(-0.45, 0.45, size=(48, 3))
    o = np.zeros((48, 3), F32)
    o[24:] = rng.uniform(-2, 2, size=(24, 3)).astype(F32)
    rays = rr.make_rays(o, (targets - o).astype(F32), rng.integers(0, 2 ** 32, size=48, dtype=np.uint32))
    want, counts = rr.expected(b.models, b.materials, b.bvh, cam, rays, 2, 3)
    brute, _ = rr.expected(b.models, b.materials, single_leaf_bvh(b.models), cam, rays, 1, 0)
    assert counts["hit_entries"] > 8 and (want["t"] != brute["t"]).any()       # (the overflow rule shows: some first hits are not the nearest sphere)
    _check_against(plugin, rays, want, counts, b.models, 2, 3, "overflow")


def _random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform((-8.0, 0.3, -8.0), (8.0, 3.0, 8.0), size=(n, 3)).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    return rr.make_rays(o, d, rng.integers(0, 2 ** 32, size=n, dtype=np.uint32))


@pytest.mark.gpu
def test_list_lengths_streaming_against_plain(plugin):
    import torch
    _upload_cover(plugin, "caller")
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 1024     # every lane of a streaming launch that fills the device
    rays = _random_rays(lanes + 1, 21)
    full = _radiance(plugin, rays, 2, 2, PLAIN, device=True)
    assert ((full["status"] & brt.QUERY_STATUS_HIT) != 0).any() and (full["status"] == brt.QUERY_STATUS_MISS).any()
    for n in (1, 63, 64, 65, 1023, 1024, 1025, lanes - 1, lanes, lanes + 1):
        got = _radiance(plugin, rays[:n], 2, 2, STREAM, device=True)
        _same_bytes(got, full[:n], f"list of {n}")
        if n <= 65:
            _same_bytes(_radiance(plugin, rays[:n], 2, 2, STREAM), full[:n], f"list of {n}, host buffers")
            _same_bytes(_radiance(plugin, rays[:n], 2, 2, PLAIN), full[:n], f"list of {n}, host buffers, plain")
    assert plugin.node.last_radiance_stats["n_workgroups"] == lanes // 1024


@pytest.mark.gpu
def test_a_long_list_against_ray_queries_and_the_sky(plugin):
    _upload_cover(plugin, "caller")
    n = 65536
    rays = _random_rays(n, 22)
    got = _radiance(plugin, rays, 1, 8, PLAIN)
    _same_bytes(_radiance(plugin, rays, 1, 8, STREAM), got, "forms")
    q = np.zeros(n, brt.RAY_DTYPE)
    q["origin"], q["direction"], q["user"], q["t_max"] = rays["origin"], rays["direction"], rays["user"], np.inf
    hits = plugin.node.query_rays(q)
    for f in ("t", "sphere", "material", "status", "user"):
        assert np.array_equal(got[f].view(np.uint32), hits[f].view(np.uint32)), f
    st = plugin.node.last_radiance_stats
    is_hit = (hits["status"] & brt.QUERY_STATUS_HIT) != 0
    assert st["hits"] == int(is_hit.sum()) and st["refused"] == 0 and st["walks"] >= n
    miss = ~is_hit
    assert miss.sum() > 1000 and is_hit.sum() > 1000
    assert np.array_equal(got["rgb"][miss].view(np.uint32), rr.sky_rgb(rays["direction"][miss]).view(np.uint32))
    # more samples of a miss ray: the same colour summed and divided, one walk each
    sky = rays[miss][:4096]
    many = _radiance(plugin, sky, 4, 8, STREAM)
    assert plugin.node.last_radiance_stats["walks"] == len(sky)
    c = rr.sky_rgb(sky["direction"])
    want = ((((c + c).astype(F32) + c).astype(F32) + c).astype(F32) / F32(4)).astype(F32)
    assert np.array_equal(many["rgb"].view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_refused_entries_and_reach(plugin):
    b = _cover()
    lvl, cam, win = _cover_camera()
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    plugin.node.radiance_rays(_standard()[:1], 1, 0, origin_bound=20.0)
    tree = brt.build_bvh_sah(b.models, plugin.node.last_radiance_stats["tree_reach"])
    bound = plugin.node.query_origin_bound()
    assert 20.0 <= bound < np.inf
    rays = _standard().copy()
    rays["user"] = np.arange(len(rays), dtype=np.uint32) ^ np.uint32(0xDEADBEEF)
    bad = {3: ("origin", (np.nan, 0, 0)), 40: ("origin", (0, np.inf, 0)), 41: ("direction", (0, 0, -np.inf)), 70: ("direction", (np.nan,) * 3),
           95: ("origin", (-np.inf, 0, 0))}
    far = {10: (np.nextafter(F32(bound), F32(np.inf)), 0, 0), 64: (0, -F32(bound) * 2, 0), 65: (3.0e38, 3.0e38, 3.0e38)}
    edge = {20: (F32(bound), 0, 0)}                                    # exactly at the bound: traced
    for i, (field, v) in bad.items():
        rays[field][i] = v
    for i, v in {**far, **edge}.items():
        rays["origin"][i] = v
    status = np.zeros(len(rays), np.uint32)
    status[list(bad)] = brt.QUERY_STATUS_INVALID
    status[list(far)] = brt.QUERY_STATUS_OUT_OF_REACH
    refused = status != 0
    want, counts = rr.expected(b.models, b.materials, tree, cam, rays[~refused], 2, 4)
    for form in (PLAIN, STREAM):
        for device in (False, True):
            got = _radiance(plugin, rays, 2, 4, form, device=device)
            assert np.array_equal(got["user"], rays["user"])
            assert np.array_equal(got["status"][refused], status[refused])
            assert np.isposinf(got["t"][refused]).all() and (got["rgb"][refused].view(np.uint32) == 0).all()
            assert (got["sphere"][refused] == brt.QUERY_NONE).all() and (got["material"][refused] == brt.QUERY_NONE).all()
            rr.assert_equal(got[~refused], want, f"neighbours of refused entries, form {form}")
            st = plugin.node.last_radiance_stats
            assert (st["refused"], st["hits"], st["walks"]) == (int(refused.sum()), counts["hit_entries"], _walks_expected(want, counts, 2))
    # a far origin with origin_bound given is answered on a tree of a longer reach, rebuilt once
    k = 60.0
    far_o = np.array([13.0 * k, 2.0 * k, 3.0 * k], F32)
    target = b.models["position"][:48].astype(F32)
    far_rays = rr.make_rays(np.broadcast_to(far_o, target.shape), target - far_o, np.arange(48, dtype=np.uint32) + 7)
    out = _radiance(plugin, far_rays, 2, 4, PLAIN)
    assert (out["status"] == brt.QUERY_STATUS_OUT_OF_REACH).all() and (out["rgb"] == 0).all() and np.array_equal(out["user"], far_rays["user"])
    l1 = l1_norm(far_o)
    got = _radiance(plugin, far_rays, 2, 4, PLAIN, origin_bound=l1)
    st = plugin.node.last_radiance_stats
    assert st["tree_rebuilt"] == 1 and st["tree_reach"] > 0 and plugin.node.query_origin_bound() >= l1
    twin = brt.build_bvh_sah(b.models, st["tree_reach"])
    want_far, counts_far = rr.expected(b.models, b.materials, twin, cam, far_rays, 2, 4)
    rr.assert_equal(got, want_far, "far origin")
    assert counts_far["hit_entries"] > 0
    _same_bytes(_radiance(plugin, far_rays, 2, 4, STREAM, origin_bound=l1), got, "far origin, streaming")
    assert plugin.node.last_radiance_stats["tree_rebuilt"] == 0            # (never lowered, not rebuilt twice)


def _oracle_frame_ok(plugin, oracle, b, what):
    lvl, cam, win = _cover_camera()
    frame = plugin.node.run(lvl, cam, win, W, H)
    ref, _ = oracle.render(b, lvl, cam, win, W, H)
    assert np.array_equal(frame.view(np.uint32), ref.view(np.uint32)), what


@pytest.mark.gpu
def test_refused_calls_leave_the_context_usable(plugin, oracle):
    import torch
    b, _ = _upload_cover(plugin, "caller")
    lib, ctx = plugin._lib, plugin._ctx
    rays = np.ascontiguousarray(_standard()[:8])
    out = np.zeros(8, brt.RADIANCE_DTYPE)
    r, o = rays.ctypes.data, out.ctypes.data
    d_buf = torch.zeros(8 * 32 * 2, dtype=torch.uint8, device="cuda")
    d_r, d_o = d_buf.data_ptr(), d_buf.data_ptr() + 8 * 32

    def refused(code, call, what):
        assert call() == code, what
        _oracle_frame_ok(plugin, oracle, b, what)

    refused(INVALID, lambda: lib.brt_radiance_rays(ctx, r, 8, 0, 4, 0.0, o, None), "samples 0")
    refused(INVALID, lambda: lib.brt_radiance_rays(ctx, r, 8, 65536, 4, 0.0, o, None), "samples 65536")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 0, 4, 0.0, d_o, None, 0, None), "samples 0, device")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 65536, 4, 0.0, d_o, None, 0, None), "samples 65536, device")
    refused(INVALID, lambda: lib.brt_radiance_rays(ctx, r, 8, 1, 65536, 0.0, o, None), "bounces 65536")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 1, 4, 0.0, d_o, None, brt.FLAG_DENOISE, None), "unknown flag")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 1, 4, 0.0, d_o, None, brt.FLAG_CALLER_STREAM | brt.FLAG_KERNEL_SIMPLE, None),
            "unknown flag beside a known one")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 1, 4, 0.0, d_r + 32 * 7, None, 0, None), "overlapping buffers")
    refused(INVALID, lambda: lib.brt_radiance_rays_device(ctx, d_r, 8, 1, 4, 0.0, d_r, None, 0, None), "the same buffer")
    assert lib.brt_radiance_rays(ctx, None, 8, 1, 4, 0.0, o, None) == INVALID
    assert lib.brt_radiance_rays(ctx, r, 8, 1, 4, 0.0, None, None) == INVALID
    assert lib.brt_radiance_rays(ctx, r, 8, 1, 4, float("nan"), o, None) == INVALID
    assert lib.brt_radiance_rays(ctx, r, 8, 1, 4, -1.0, o, None) == INVALID
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert lib.brt_radiance_rays(ctx, r, 8, 1, 4, 0.0, o, None) == UNSUPPORTED
        assert lib.brt_radiance_rays_device(ctx, d_r, 8, 1, 4, 0.0, d_o, None, 0, None) == UNSUPPORTED
    finally:
        plugin.set_policy(0)
    _oracle_frame_ok(plugin, oracle, b, "a non-default policy")
    # n_rays = 0 is OK and launches nothing; the bounds of samples and bounces are accepted
    assert plugin.node.radiance_rays(np.zeros(0, brt.RADIANCE_RAY_DTYPE), 1, 0).shape == (0,)
    assert plugin.node.last_radiance_stats["n_workgroups"] == 0
    want, _ = _want("caller", 4, 8)
    sky = np.ascontiguousarray(_standard()[want["status"] == brt.QUERY_STATUS_MISS][:1])      # (a miss: 65 535 samples of one walk)
    assert lib.brt_radiance_rays(ctx, sky.ctypes.data, 1, 65535, 65535, 0.0, o, None) == 0
    assert out[0]["status"] == brt.QUERY_STATUS_MISS and out[0]["user"] == sky[0]["user"] and (out[0]["rgb"] > 0).all()
    rr.assert_equal(plugin.node.radiance_rays(_standard(), 4, 8), want, "after the refusals")
    with brt.RaytracePlugin([0]) as empty:
        with pytest.raises(brt.BrtError) as e:
            empty.node.radiance_rays(rays, 1, 1)
        assert e.value.code == NO_SCENE
        with pytest.raises(brt.BrtError) as e:
            empty.node.radiance_rays((d_r, 8, d_o), 1, 1, device=True)
        assert e.value.code == NO_SCENE
        empty.node.write_buffers(b)
        rr.assert_equal(empty.node.radiance_rays(_standard(), 4, 8), want, "after no scene")


@pytest.mark.gpu
def test_lists_and_a_frame_on_two_caller_streams_and_across_an_upload(plugin):
    import torch
    b, _ = _upload_cover(plugin, "caller")
    lvl, cam, win = brt.cover_camera(160, 90, 4, 4)
    rays = _random_rays(6000, 23)
    serial_frame = plugin.node.run(lvl, cam, win, 160, 90).copy()
    serial = {form: _radiance(plugin, rays, 2, 4, form) for form in (PLAIN, STREAM)}
    _same_bytes(serial[PLAIN], serial[STREAM], "forms")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_frame = torch.zeros((90, 160, 4), dtype=torch.float32, device="cuda")
    d_rays = _dev(rays)
    d_out = [torch.zeros(rays.size * 32, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for i, form in enumerate((PLAIN, STREAM, PLAIN, STREAM)):
        with plugin.tuning(BRT_RADIANCE_FORM=form):
            if i == 1:
                plugin.node.render_device(lvl, cam, win, 160, 90, d_frame.data_ptr(), stream=s1.cuda_stream)
            st = plugin.node.radiance_rays((d_rays.data_ptr(), rays.size, d_out[i].data_ptr()), 2, 4, device=True,
                                           stream=(s2 if i % 2 else s1).cuda_stream)
            assert (st["walks"], st["hits"], st["refused"]) == (0, 0, 0) and st["form"] == form - 1
    torch.cuda.synchronize()
    assert np.array_equal(d_frame.cpu().numpy().view(np.uint32), serial_frame.view(np.uint32))
    for i in range(4):
        _same_bytes(d_out[i].cpu().numpy().view(brt.RADIANCE_DTYPE), serial[PLAIN], f"list {i} in flight")
    # a list enqueued before a re-upload that moves a sphere sees the old scene, one after it the new one
    moved = b.models.copy()
    target = int(serial[PLAIN]["sphere"][(serial[PLAIN]["status"] & brt.QUERY_STATUS_HIT) != 0][0])
    moved["position"][target] += np.array([0.0, 0.35, 0.0], F32)
    b2 = brt.Buffers(moved, b.materials, brt.build_bvh(moved))
    plugin.node.radiance_rays((d_rays.data_ptr(), rays.size, d_out[0].data_ptr()), 2, 4, device=True, stream=s1.cuda_stream)
    plugin.node.write_buffers(b2)
    plugin.node.radiance_rays((d_rays.data_ptr(), rays.size, d_out[1].data_ptr()), 2, 4, device=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    _same_bytes(d_out[0].cpu().numpy().view(brt.RADIANCE_DTYPE), serial[PLAIN], "before the upload")
    after = d_out[1].cpu().numpy().view(brt.RADIANCE_DTYPE)
    _same_bytes(after, _radiance(plugin, rays, 2, 4, PLAIN), "after the upload")
    assert after.tobytes() != serial[PLAIN].tobytes()
    sample = np.flatnonzero(after["sphere"] == target)[:24]
    assert len(sample) > 0
    want, _ = rr.expected(b2.models, b2.materials, b2.bvh, cam, rays[sample], 2, 4)
    rr.assert_equal(after[sample], want, "the moved sphere")


@pytest.mark.gpu
def test_frames_do_not_move(plugin):
    b = _cover()
    w, h = 320, 180
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
    before = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=brt.FLAG_COUNTERS).copy()
    stats_before = dict(plugin.node.last_stats)
    rays = _random_rays(5000, 24)
    for form in (PLAIN, STREAM):
        _radiance(plugin, rays, 2, 4, form)
        _radiance(plugin, rays, 2, 4, form, device=True)
    after = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for k in ("rays", "node_pops", "interior_visits", "sphere_tests", "hits", "kernel_variant", "n_workgroups", "scene_in_lds"):
        assert plugin.node.last_stats[k] == stats_before[k], k


@pytest.mark.gpu
def test_seeds(plugin):
    b, _ = _upload_cover(plugin, "caller")
    want, _ = _want("caller", 4, 8)
    diffuse = [i for i in np.flatnonzero((want["status"] & brt.QUERY_STATUS_HIT) != 0)
               if b.materials[want["material"][i]]["metallic"] == 0 and b.materials[want["material"][i]]["specular_transmission"] == 0]
    assert len(diffuse) >= 8
    rays = np.repeat(_standard()[diffuse[:8]], 3)                       # each ray three times: seed, seed, another seed
    rays["seed"][2::3] ^= np.uint32(0x9E3779B9)
    for form in (PLAIN, STREAM):
        got = _radiance(plugin, rays, 4, 8, form)
        a, same, other = got[0::3], got[1::3], got[2::3]
        _same_bytes(a, same, "the same ray twice in one list")
        for f in ("t", "sphere", "material", "status"):
            assert np.array_equal(a[f].view(np.uint32), other[f].view(np.uint32)), f
        assert (a["rgb"].view(np.uint32) != other["rgb"].view(np.uint32)).any(axis=1).all()
        rr.assert_equal(a, want[diffuse[:8]], "the standard entries")
