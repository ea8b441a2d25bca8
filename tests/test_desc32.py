"""Every kernel that walks the tree, on scenes that need 32-bit child descriptors (brt_layout.h Desc<D16>, DESIGN.md "Both descriptor
forms"): more than DESC16_MAX_INDEX = 16 382 spheres.  Such a scene is never LDS-resident, has no hot-record order, and takes the
`D16 = false` instantiation of the trace, bring-up, query, guide, coverage-guide and upscale kernels.  Three sizes of
helpers.big_scene: 16 382 (the last 16-bit scene), 16 383 (the first 32-bit one) and 24 001 (a third of the ids need more than 14
bits); four trees at 24 001: the callee's SAH tree, the caller's PLOC tree, a caller's tree with three-sphere leaves, and a 40-link
caterpillar over a median-split tree (deeper than the 32-entry stack: not a simple tree).

Every comparison is the one the kernel's own test file makes, with its reference and its bar: frames, counters, query records and
guides bitwise against the CPU oracle on the tree the GPU walked; the denoiser against denoise_ref64 (test_denoise_edges._check);
temporal frames against temporal_ref and blend-post frames against blend_post_ref at 1e-4; upsampling against upscale_ref at 1e-4
with bitwise sky.  Every test also asserts which path ran (last_stats["scene_in_lds"], ["hot_records"], the query form).

Measured where this file was written, 96x54, 2 spp, 4 bounces, 24 001 spheres: an oracle frame 0.45 s, the oracle's guides 0.9 s,
build_bvh_sah 0.09 s, build_bvh 0.10 s, median_split_bvh 0.3 s, temporal_ref.sphere_ids 0.6 s.  The oracle's share of the query
test (query_ref.ray_sets + expected, one call per ray, 2 000 rays per set) is 0.3 s on the PLOC tree and about 1 s on the callee's;
on the two median-split trees, which have no spatial order (about 10 000 node pops per ray), 2 000 rays per set would take 1.1 + 4.0 s
(three-sphere leaves) and 2.2 + 5.3 s (caterpillar), so there the sets hold 600 rays each, as in test_query.py's topology and overflow
cases: 2.0 s and 2.8 s.

The facts _assert_path asserts are also printed: run with -rP (or -s) to see scene_in_lds, hot_records and the query form per test."""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
import blend_post_ref as bp
import denoise_ref as dr
import denoise_ref64 as d64
import query_ref as qr
import temporal_ref as tr
import upscale_ref as ur
from helpers import (big_scene, big_view, chain_bvh, graft_bvh, l1_norm, median_split_bvh, resident_callee_tree, BIG_VIEW)
# the checkers and device plumbing of each kernel's own test file, imported rather than copied: the bars cannot drift apart, and a
# rename over there fails this file's collection loudly
from test_blend_post import _both_classes
from test_denoise_edges import _check as check_denoised, _denoise_dev
from test_parity_gpu import COUNTER_KEYS, assert_frames_equal
from test_query import PLAIN, STREAM, _query, _same_bytes, _with_tmax
from test_temporal import _compare_state, _rel
from test_upscale import _render_low, _render_upscaled, _same_bits, _upscale_dev

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
SEED = 11
W, H = 96, 54
LAST16, FIRST32, BIG = 16382, 16383, 24001
L1, L2 = brt.Raytracing.FallbackRaster, brt.Raytracing.FallbackRaytraced
BLEND, DENOISE, TEMPORAL = brt.FLAG_BLEND_POST, brt.FLAG_DENOISE, brt.FLAG_TEMPORAL
# (sphere count, tree): the two sizes at the switch-over on the callee's and the caller's tree, the large scene on all four
SCENES = [(LAST16, "callee"), (LAST16, "ploc"), (FIRST32, "callee"), (FIRST32, "ploc"),
          (BIG, "callee"), (BIG, "ploc"), (BIG, "median3"), (BIG, "caterpillar")]
SCENE_IDS = [f"{n}_{'desc16_lds2' if n <= LAST16 else 'desc32_global'}_{tree}" for n, tree in SCENES]


# ---- scenes, trees and references, made once per module ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene(n):
    return big_scene(n, SEED)


@functools.lru_cache(maxsize=None)
def _caller(n, tree):
    """The scene of `n` spheres with a caller's tree."""
    b = _scene(n)
    if tree == "ploc":
        return brt.Buffers(b.models, b.materials, brt.build_bvh(b.models))
    if tree == "median3":                        # general leaves: the leaf table under 32-bit descriptors
        return brt.Buffers(b.models, b.materials, median_split_bvh(b.models, 3))
    assert tree == "caterpillar"
    # the first 40 spheres one behind the other on the view axis (the `overflow` case of test_query.py), chained; the bottom link of
    # the chain holds sphere 0 and the root of a median-split tree over the other spheres, 40 levels down: deeper than the
    # 32-entry stack, so the tree is not a simple one and the overflow rule ends the walk of every ray through the chain's boxes
    models = b.models.copy()
    o, t = np.array(BIG_VIEW["pos"]), np.array(BIG_VIEW["target"])
    axis = (t - o) / np.linalg.norm(t - o)
    models["position"][:40] = (o + (5.0 + np.arange(40))[:, None] * axis).astype(F32)
    models["radius"][:40] = 0.5
    chain = chain_bvh(models[:40])
    nodes = graft_bvh(chain, len(chain) - 1, median_split_bvh(models[40:], 1), 40)
    assert brt.validate_scene(models, b.materials, nodes) > 40
    return brt.Buffers(models, b.materials, nodes)


_FRAMES = {}


def _oracle_frame(oracle, key, b, lvl, cam, win, w, h, raster=None, depth=None):
    """oracle.render, once per `key` (the tree, the view and the raster inputs by name)."""
    if key not in _FRAMES:
        _FRAMES[key] = oracle.render(b, lvl, cam, win, w, h, raster_rgba=raster, raster_depth=depth)
    return _FRAMES[key]


def _assert_path(plugin, n, what=""):
    """Which path the last frame took: the top of the tree in LDS at 16 382 spheres; from 16 383 on global memory, no hot order."""
    st = plugin.node.last_stats
    print(f"{what} n = {n}: scene_in_lds {st['scene_in_lds']}, hot_records {st['hot_records']}, kernel_variant {st['kernel_variant']}")
    if n <= LAST16:
        assert st["scene_in_lds"] == 2, st
    else:
        assert st["scene_in_lds"] == 0 and st["hot_records"] == 0, st


def _resident(plugin, n, tree, w=W, h=H, view=None):
    """Uploads the scene and renders one frame of `view`; -> (Buffers with the tree the GPU walks, (lvl, cam, win)).  The callee's tree
    is compared through its CPU twin at the reach the context reports."""
    plugin.set_denoise()
    plugin.set_temporal()
    lvl, cam, win = view or big_view(w, h)
    if tree == "callee":
        b, win, st = resident_callee_tree(plugin, _scene(n), lvl, cam, win, w, h)
        key = (n, tree, st["tree_reach"])
    else:
        b = _caller(n, tree)
        plugin.node.run(lvl, cam, win, w, h, buffers=b)
        key = (n, tree)
    _assert_path(plugin, n, tree)
    _assert_tree_kind(b, tree)
    return b, key, (lvl, cam, win)


def _assert_tree_kind(b, tree):
    """Which instantiation the tree reaches (brt_host.cpp: a simple tree has one-sphere leaves only and max leaf depth + 1 < 31): the
    callee's and the PLOC tree the simple one, three-sphere leaves and the caterpillar the general one."""
    depth = brt.validate_scene(b.models, b.materials, b.bvh)
    leaves = b.bvh["model_count"][b.bvh["model_count"] > 0]
    if tree in ("callee", "ploc"):           # measured: depth 28 (callee, every reach and size here), 19 .. 20 (PLOC)
        assert depth + 1 < 31 and leaves.max() == 1, (tree, depth, int(leaves.max()))
    elif tree == "median3":
        assert depth + 1 < 31 and leaves.max() == 3, (tree, depth, int(leaves.max()))
    else:
        assert depth > 40 and leaves.max() == 1, (tree, depth)


def _render_both(plugin, oracle, key, b, view, w, h, flags=brt.FLAG_COUNTERS, raster=None, depth=None, raster_key=None):
    """test_parity_gpu.render_both on the resident scene: the frame bitwise, the ray count, and all five counters under FLAG_COUNTERS."""
    lvl, cam, win = view
    got = plugin.node.run(lvl, cam, win, w, h, raster_rgba=raster, raster_depth=depth, flags=flags).copy()
    stats = dict(plugin.node.last_stats)
    seed = float(win[0]["random_seed"])
    want, cnt = _oracle_frame(oracle, (key, w, h, seed, int(lvl["level"][0]), cam.tobytes(), raster_key), b, lvl, cam, win, w, h, raster, depth)
    assert_frames_equal(got, want)
    assert stats["rays"] == cnt["rays"]
    if flags & brt.FLAG_COUNTERS:
        assert {k: stats[k] for k in COUNTER_KEYS} == cnt
    return got, stats


# the last sphere of the 16 383 (radius 0.07 .. 0.18 at a distance of 14 .. 44, where a pixel is 0.13 .. 0.41 wide) covers at most
# 3 x 3 pixel centres, and the paths of a few more pixels bounce into it: measured 1 differing pixel
CROPPED_MAX_PIXELS = 16


# ---- the inputs -------------------------------------------------------------------------------------------------------------------

def test_the_scenes_exercise_the_form(oracle):
    """The conditions on the inputs, from the oracle alone (its first hits on the caller's PLOC tree)."""
    lvl, cam, win = big_view(W, H)
    b = _caller(BIG, "ploc")
    g = dr.guides(oracle, b, cam, W, H)
    hit = g[..., 3] < np.inf
    sid, ties = tr.sphere_ids(g, tr.Camera(oracle, cam, W, H), b.models)
    ids = np.unique(sid[hit & ~ties])
    print(f"n = {BIG}: {len(ids)} distinct spheres, {(ids >= 16384).sum()} with an id >= 16384, sky {1 - hit.mean():.3f}, hits {hit.mean():.3f}")
    # measured: 3239 distinct spheres, 1049 of them with an id >= 16384; sky 0.153, hits 0.847 of the 5184 pixels
    assert len(ids) >= 300 and (ids >= 16384).sum() >= 60
    assert 1 - hit.mean() >= 0.10 and hit.mean() >= 0.30
    mid = g[..., 7].view(U32)
    # measured: all 48 materials; 296 pixels of a refracting one (a = 1), 99 of the one whose base colour is clamped (material 2)
    assert len(np.unique(mid[hit])) >= 40
    assert (g[..., 4:7][hit] == 1).all(-1).sum() >= 50 and (mid == 2).sum() >= 20
    assert (b.materials["base_color"][2] < 1e-3).any() and (g[..., 4:7][mid == 2].min() == np.sqrt(F32(1e-3)))
    # the switch-over: 16 382 spheres is the scene of 16 383 with its last sphere removed, a strict subset; the two oracle frames
    # differ in the few pixels that sphere touches (measured: see the bound below), so a form switch that loses a sphere cannot
    # hide behind "the scenes differ anyway"
    full, cropped = _scene(FIRST32), _scene(LAST16)
    assert np.array_equal(full.models[:-1].view(np.uint8), cropped.models.view(np.uint8))
    frames = []
    for n in (FIRST32, LAST16):
        bb = _caller(n, "ploc")
        frames.append(_oracle_frame(oracle, ((n, "ploc"), W, H, 0.5, 3, cam.tobytes(), None), bb, lvl, cam, win, W, H)[0])
        gg = dr.guides(oracle, bb, cam, W, H)
        # measured at both sizes: sky 0.281, hits 0.719
        assert 1 - (gg[..., 3] < np.inf).mean() >= 0.10 and (gg[..., 3] < np.inf).mean() >= 0.30
    # the caterpillar: the overflow rule fires.  The centre pixels look down the chain's axis, a sphere of radius 0.5 sits 5 units
    # away, and the oracle sees sky there because the walk ends at 32 stack entries; on a plain median split of the same spheres it
    # sees that sphere (measured: the guides of the two trees differ in 36 pixels)
    cat = _caller(BIG, "caterpillar")
    g_cat = dr.guides(oracle, cat, cam, W, H)
    g_flat = dr.guides(oracle, brt.Buffers(cat.models, cat.materials, brt.build_bvh(cat.models)), cam, W, H)
    assert g_cat[H // 2, W // 2, 3] == np.inf and abs(g_flat[H // 2, W // 2, 3] - 4.5) < 0.01
    assert 10 <= (g_cat.view(U32) != g_flat.view(U32)).any(-1).sum() <= 200
    differ = int((frames[0].view(U32) != frames[1].view(U32)).any(-1).sum())
    print(f"oracle frames of {FIRST32} and {LAST16} spheres differ in {differ} pixels")
    assert 1 <= differ <= CROPPED_MAX_PIXELS


# ---- trace ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tree", SCENES, ids=SCENE_IDS)
def test_trace_matches_the_oracle(plugin, oracle, n, tree):
    """The persistent kernel with and without the counters and the bring-up kernel: pixels and all five counters bitwise."""
    b, key, view = _resident(plugin, n, tree)
    _render_both(plugin, oracle, key, b, view, W, H)
    _assert_path(plugin, n, "persistent, counters")
    _render_both(plugin, oracle, key, b, view, W, H, flags=0)
    _assert_path(plugin, n, "persistent")
    _render_both(plugin, oracle, key, b, view, W, H, flags=brt.FLAG_COUNTERS | brt.FLAG_KERNEL_SIMPLE)
    if n == BIG:                                 # partial tiles
        small = big_view(33, 17, seed=0.25)
        _render_both(plugin, oracle, key, b, small, 33, 17)
        _render_both(plugin, oracle, key, b, small, 33, 17, flags=0)
        _assert_path(plugin, n, "33x17")


@pytest.mark.parametrize("tree", ["callee", "ploc"])
def test_steady_state_levels_and_parts(plugin, oracle, tree):
    import torch
    from bevyray_amd.parallel import frame_rows_of_part
    n = BIG
    b, key, view = _resident(plugin, n, tree)
    lvl, cam, _ = view
    # four frames, a new seed each: the steady state of a known view with the hot order off.  A scene walked from global memory has
    # no LEAN instantiation (brt_trace.h launch_persistent_md takes the LEAN template arguments only when MODE != SCENE_GLOBAL):
    # these frames run the same k_trace_persistent<SCENE_GLOBAL, 32-bit> as the first one, and last_stats["kernel_variant"] only
    # echoes the host's lean decision, so it is not asserted
    for seed in (0.125, 0.375, 0.625, 0.875):
        v = (lvl, cam, brt.WindowExtract.extract_component(H, seed))
        _render_both(plugin, oracle, key, b, v, W, H, flags=0)
        _assert_path(plugin, n, f"seed {seed}")
    # levels 1 and 2 with raster and depth inputs (the wall and the disc of blend_post_ref lie in front of the slab)
    raster, depth = bp.raster_inputs(W, H)
    for level in (L1, L2):
        v = big_view(W, H, level=level)
        got, _ = _render_both(plugin, oracle, key, b, v, W, H, raster=raster, depth=depth, raster_key="bp")
        _both_classes((got.view(U32) == raster.view(U32)).all(-1))
        _render_both(plugin, oracle, key, b, v, W, H, flags=0, raster=raster, depth=depth, raster_key="bp")
    # three parts assemble to the full frame
    full, cnt = _oracle_frame(oracle, (key, W, H, 0.5, 3, cam.tobytes(), None), b, *view, W, H)
    n_parts = 3
    rows = brt.tile_rows(H, n_parts)
    tiles = torch.zeros((n_parts, rows, W, 4), dtype=torch.float32, device="cuda")
    total = 0
    for p in range(n_parts):
        st = plugin.node.render_part_device(*view, W, H, p, n_parts, tiles[p].data_ptr())
        total += st["rays"]
        assert st["scene_in_lds"] == 0 and st["hot_records"] == 0
        fr = frame_rows_of_part(H, p, n_parts)
        assert_frames_equal(tiles[p].cpu().numpy()[fr >= 0], full[fr[fr >= 0]])
    assert total == cnt["rays"]
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    plugin.node.deinterleave_device(tiles.data_ptr(), n_parts, W, H, frame.data_ptr())
    torch.cuda.synchronize()
    assert_frames_equal(frame.cpu().numpy(), full)


def test_a_tunable_instantiation_and_a_far_camera(plugin, oracle):
    n = BIG
    b, key, view = _resident(plugin, n, "callee")
    # 512 threads with the hand-over pool forced on (a frame of this size runs without it by default)
    with plugin.tuning(BRT_BLOCK_THREADS=512, BRT_POOL_FORCE=1):
        _, st = _render_both(plugin, oracle, key, b, view, W, H)
        _, st0 = _render_both(plugin, oracle, key, b, view, W, H, flags=0)
        assert st["threads_per_workgroup"] == 512 and st0["threads_per_workgroup"] == 512 and st["scene_in_lds"] == 0
        with plugin.tuning(BRT_POOL_FORCE=0):
            plugin.node.run(*view, W, H)
            assert plugin.node.last_stats["lds_bytes"] < st0["lds_bytes"]          # the forced launches really carried a pool
    # a camera far behind the first one: the callee rebuilds its tree for the larger reach
    reach = plugin.node.last_stats["tree_reach"]
    far = big_view(W, H, pos=(12.0, 9.0, 160.0), fov=0.22, seed=0.75)
    got = plugin.node.run(*far, W, H, flags=brt.FLAG_COUNTERS).copy()
    st = dict(plugin.node.last_stats)
    assert st["tree_rebuilt"] == 1 and st["tree_reach"] > reach, (st, reach)
    _assert_path(plugin, n, "far camera")
    twin = brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, st["tree_reach"]))
    want, cnt = oracle.render(twin, *far, W, H)
    assert_frames_equal(got, want)
    assert {k: st[k] for k in COUNTER_KEYS} == cnt
    hit_share = (dr.guides(oracle, twin, far[1], W, H)[..., 3] < np.inf).mean()
    assert 0.05 <= hit_share <= 0.95, hit_share


# ---- queries ----------------------------------------------------------------------------------------------------------------------

def _assert_query_mode(plugin, n, n_rays):
    """The streaming form's launch: 256-thread workgroups when the scene is walked from global memory (32-bit descriptors), 1024 with
    the top of the tree in LDS (brt_api_query.cpp plan_query)."""
    st = plugin.node.last_query_stats
    assert st["form"] == 1
    assert st["n_workgroups"] == -(-n_rays // (1024 if n <= LAST16 else 256)), (st, n_rays)


@pytest.mark.parametrize("n,tree", SCENES, ids=SCENE_IDS)
def test_queries_match_the_oracle_raycast(plugin, oracle, n, tree):
    """test_query.test_queries_match_the_oracle_raycast on these scenes: both forms, both modes, both entry points, t_max around the
    hit, batch sizes around a wave."""
    b, _, (lvl, cam, win) = _resident(plugin, n, tree)
    rng = np.random.default_rng(7)
    sets = qr.ray_sets(oracle, b.models, b.bvh, cam, W, H, rng, n=600 if tree in ("median3", "caterpillar") else 2000)   # (see the docstring)
    bound = plugin.node.query_origin_bound()
    n_hits = high = 0
    for name, rays in sets.items():
        l1 = np.abs(rays["origin"]).astype(F32)
        rays = rays[((l1[:, 0] + l1[:, 1]) + l1[:, 2]) <= bound]              # (a callee's tree: the rays inside its reach)
        assert len(rays) >= 16, name
        want, t_unb = qr.expected(oracle, b.models, b.bvh, rays)
        got = _query(plugin, rays, PLAIN)
        qr.assert_hits_equal(got, want, f"{tree}/{name} plain")
        qr.check_spheres(oracle, b.models, rays, got)
        st = plugin.node.last_query_stats
        is_hit = (want["status"] & brt.QUERY_STATUS_HIT) != 0
        assert (st["rays_walked"], st["hits"], st["refused"]) == (len(rays), int(is_hit.sum()), 0)
        n_hits += int(is_hit.sum())
        high += int((got["sphere"][is_hit] >= 16384).sum())
        _same_bytes(_query(plugin, rays, STREAM), got, f"{tree}/{name} streaming form")
        if len(rays) > 1024:
            _assert_query_mode(plugin, n, len(rays))
        _same_bytes(_query(plugin, rays, PLAIN, device=True), got, f"{tree}/{name} device buffers, plain")
        _same_bytes(_query(plugin, rays, STREAM, device=True), got, f"{tree}/{name} device buffers, streaming")
        # t_max just below, at and just above the unbounded t: miss, miss, hit; ANY agrees with CLOSEST on every ray
        t = np.where(np.isfinite(t_unb), t_unb, F32(1.0)).astype(F32)
        for t_max in (np.nextafter(t, F32(0)), t, np.nextafter(t, F32(np.inf)), np.full(len(rays), np.inf, F32)):
            bounded_rays = _with_tmax(rays, t_max)
            for mode in (brt.QUERY_CLOSEST, brt.QUERY_ANY):
                want_b = qr.bounded(want, t_max, mode)
                got_p = _query(plugin, bounded_rays, PLAIN, mode)
                qr.assert_hits_equal(got_p, want_b, f"{tree}/{name} t_max mode {mode}")
                if mode == brt.QUERY_CLOSEST:
                    qr.check_spheres(oracle, b.models, bounded_rays, got_p)
                else:
                    assert (got_p["sphere"] == brt.QUERY_NONE).all()
                _same_bytes(_query(plugin, bounded_rays, STREAM, mode), got_p, f"{tree}/{name} t_max mode {mode} streaming")
        below = _query(plugin, _with_tmax(rays, np.nextafter(t, F32(0))), PLAIN)
        above = _query(plugin, _with_tmax(rays, np.nextafter(t, F32(np.inf))), PLAIN)
        assert not (below["status"] & brt.QUERY_STATUS_HIT).any()
        assert np.array_equal((above["status"] & brt.QUERY_STATUS_HIT) != 0, is_hit)
    assert n_hits > 0
    if n == BIG:
        assert high >= 60, high                  # spheres whose id does not fit 14 bits were hit and named
    rays = sets["shuffled"]
    full = _query(plugin, rays, PLAIN)
    for k in (1, 63, 64, 65, min(len(rays), 517)):
        for form in (PLAIN, STREAM):
            for device in (False, True):
                _same_bytes(_query(plugin, rays[:k], form, device=device), full[:k], f"{tree} batch of {k}, form {form}, device {device}")
    _assert_path(plugin, n, "after the queries")


@pytest.mark.parametrize("n", [LAST16, FIRST32, BIG])
def test_picking_equals_the_guide_buffer(plugin, n):
    b, _, (lvl, cam, win) = _resident(plugin, n, "callee")
    rays = np.concatenate([brt.pixel_ray(cam, win, W, H, x, y) for y in range(H) for x in range(W)])
    bound = l1_norm(cam[0]["position"])
    g = plugin.debug_denoise_guides(cam, win, W, H)
    for form in (PLAIN, STREAM):
        hits = _query(plugin, rays, form, origin_bound=bound).reshape(H, W)
        assert plugin.node.last_query_stats["tree_rebuilt"] == 0
        if form == STREAM:
            _assert_query_mode(plugin, n, len(rays))
        assert np.array_equal(hits["user"], np.arange(W * H, dtype=U32).reshape(H, W))
        assert np.array_equal(hits["t"].view(U32), g[..., 3].view(U32))
        assert np.array_equal(hits["normal"].view(U32), g[..., :3].view(U32))
        assert np.array_equal(hits["material"], g[..., 7].view(U32))
        is_hit = (hits["status"] & brt.QUERY_STATUS_HIT) != 0
        assert is_hit.any() and (hits["status"] == brt.QUERY_STATUS_MISS).any()
        assert np.array_equal(b.models["material_id"][hits["sphere"][is_hit]], hits["material"][is_hit])
        if n == BIG:
            assert (np.unique(hits["sphere"][is_hit]) >= 16384).sum() >= 60


# ---- guides -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tree", SCENES, ids=SCENE_IDS)
def test_guides_are_the_oracles_raycast(plugin, oracle, n, tree):
    b, _, (lvl, cam, win) = _resident(plugin, n, tree)
    for w, h in ((W, H), (33, 17)):
        _, cam_s, win_s = big_view(w, h)
        got = plugin.debug_denoise_guides(cam_s, win_s, w, h)
        want = dr.guides(oracle, b, cam_s, w, h)
        bad = (got.view(U32) != want.view(U32)).any(-1)
        assert not bad.any(), (w, h, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        hit = got[..., 3] < np.inf
        assert hit.any() and (~hit).any()
    if n == BIG and tree != "caterpillar":
        # the material id and `a` planes come from spheres with ids above 16 383 too
        g96 = plugin.debug_denoise_guides(cam, win, W, H)
        sid, ties = tr.sphere_ids(g96, tr.Camera(oracle, cam, W, H), b.models)
        high = (sid >= 16384) & (g96[..., 3] < np.inf) & ~ties
        assert high.sum() >= 300
        assert np.array_equal(g96[..., 7].view(U32)[high], b.models["material_id"][sid[high]])
        assert len(np.unique(g96[..., 4:7][high], axis=0)) >= 20


# ---- denoiser, temporal, blend-post -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tree", [(BIG, "ploc"), (BIG, "callee")], ids=["24001_ploc", "24001_callee"])
def test_denoiser_against_the_float64_reference(plugin, oracle, n, tree):
    b, _, (lvl, cam, win) = _resident(plugin, n, tree)
    frame = plugin.node.run(lvl, cam, win, W, H).copy()
    g = plugin.debug_denoise_guides(cam, win, W, H)
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, W, H)
    try:
        for it in (1, 5):
            plugin.set_denoise(it)
            got = _denoise_dev(plugin, cam, win, W, H, frame).view(F32)
            want = d64.denoise(frame, g, dirs, tan, spp=2, **{**dr.DEFAULTS, "iterations": it})
            live = ~d64.passes_through(frame, g)
            print(f"denoiser, {it} iterations: max rel err {d64.rel_err(got, want, live).max():.3g}")
            check_denoised(got, want, frame, g, (tree, it))
            assert np.abs(got - frame)[live].max() > 1e-4                  # (it did filter)
    finally:
        plugin.set_denoise()


def _orbit(i, step_deg=0.25):
    """The camera of big_view turned about its target by i steps."""
    a = np.radians(step_deg * i)
    o, t = np.array(BIG_VIEW["pos"]), np.array(BIG_VIEW["target"])
    d = o - t
    pos = t + np.array([d[0] * np.cos(a) - d[2] * np.sin(a), d[1], d[0] * np.sin(a) + d[2] * np.cos(a)])
    return big_view(W, H, pos=tuple(float(x) for x in pos), seed=0.5 + 0.0371 * i)


@pytest.mark.parametrize("denoise_on", [False, True])
def test_temporal_orbit_matches_the_restatement(plugin, oracle, denoise_on):
    """test_temporal.test_orbit_matches_the_restatement, three frames: the history keeps sphere ids that need more than 14 bits (the
    largest is 24 000), and with no hot order the resident numbering is the caller's (no map)."""
    n = BIG
    b, _, _ = _resident(plugin, n, "callee")
    plugin.reset_temporal()
    hist = tr.History()
    sph = tr.spheres_of(b.models)
    flags = TEMPORAL | (DENOISE if denoise_on else 0)
    n_ties = 0
    try:
        for i in range(3):
            lvl, cam, win = _orbit(i)
            plain = plugin.node.run(lvl, cam, win, W, H).copy()
            got = plugin.node.run(lvl, cam, win, W, H, flags=flags).copy()
            _assert_path(plugin, n, f"temporal frame {i}")
            g = plugin.debug_denoise_guides(cam, win, W, H)
            c = tr.Camera(oracle, cam, W, H)
            sid, ties = tr.sphere_ids(g, c, b.models)
            n_ties += int(ties.sum())
            want = tr.frame_step(hist, plain, g, sid, c, sph, 2, denoise_on)
            _compare_state(plugin.debug_temporal_state(W, H), tr.state(hist), ~ties)
            print(f"temporal frame {i}, denoise {denoise_on}: max rel err {_rel(got, want):.3g}")
            assert _rel(got, want) <= 1e-4
            if i > 0:
                kept = tr.state(hist)[..., 3] >= 2
                hit = g[..., 3] < np.inf
                assert kept.sum() > 0.5 * hit.sum()                        # (the orbit keeps most of the history)
                assert (sid[kept & hit & ~ties] >= 16384).any()            # ... on spheres whose id needs more than 14 bits
        assert n_ties <= 0.001 * W * H * 3 + 1
    finally:
        plugin.reset_temporal()


@pytest.mark.parametrize("mode", [DENOISE, TEMPORAL, DENOISE | TEMPORAL], ids=["denoise", "temporal", "denoise_temporal"])
def test_blend_post_matches_the_restatement(plugin, oracle, mode):
    """test_blend_post.test_modes_match_the_restatement on a level-1 frame: the coverage-guide kernel under 32-bit descriptors."""
    n = BIG
    b, _, _ = _resident(plugin, n, "median3")
    rgba, depth = bp.raster_inputs(W, H)
    sph = tr.spheres_of(b.models)
    hist = tr.History()
    plugin.reset_temporal()
    try:
        for i in range(2):
            lvl, cam, win = big_view(W, H, level=L1, seed=0.5 + 0.0371 * i)
            covf = plugin.node.run(lvl, cam, win, W, H, raster_depth=depth).copy()
            cov = bp.coverage(covf)
            _both_classes(cov)
            got = plugin.node.run(lvl, cam, win, W, H, raster_rgba=rgba, raster_depth=depth, flags=BLEND | mode).copy()
            _assert_path(plugin, n, f"blend-post frame {i}")
            g = plugin.debug_denoise_guides(cam, win, W, H)
            c = tr.Camera(oracle, cam, W, H)
            sid, ties = tr.sphere_ids(g, c, b.models)
            if mode == DENOISE:
                want = bp.denoise_frame(oracle, covf, g, cam, rgba)
            else:
                want = bp.frame_step(hist, covf, g, sid, c, sph, 2, bool(mode & DENOISE), rgba)
                st, ws = plugin.debug_temporal_state(W, H), tr.state(hist)
                check = ~ties
                assert np.array_equal(st[..., 3][check], ws[..., 3][check])
                assert np.array_equal(np.isnan(st[..., 6:8][check]), np.isnan(ws[..., 6:8][check]))
                assert (st[..., 3][cov] == 0).all() and np.isnan(st[..., 6:8][cov]).all()
            assert np.array_equal(got.view(U32)[cov], rgba.view(U32)[cov])
            assert not (bp.coverage(got) & ~cov).any()                     # (no uncovered pixel ends with alpha 0)
            with np.errstate(invalid="ignore"):
                err = float(np.nanmax(np.abs(got[~cov].astype(np.float64) - want[~cov]) / np.maximum(1.0, np.abs(want[~cov]))))
            print(f"blend-post mode {mode}, frame {i}: max rel err {err:.3g}")
            assert err <= 1e-4
            assert ((g[..., 3] < np.inf) & ~cov).sum() >= 0.2 * W * H        # (uncovered hit pixels: the filter had work)
    finally:
        plugin.reset_temporal()


# ---- upsampling -------------------------------------------------------------------------------------------------------------------

UPSCALES = [(BIG, "callee", (96, 54, 48, 27)), (BIG, "callee", (97, 55, 25, 14)), (BIG, "median3", (96, 54, 48, 27)),
            (LAST16, "callee", (96, 54, 48, 27)), (FIRST32, "callee", (96, 54, 48, 27)),
            (LAST16, "ploc", (96, 54, 48, 27)), (FIRST32, "ploc", (96, 54, 48, 27))]


@pytest.mark.parametrize("n,tree,size", UPSCALES, ids=[f"{n}_{t}_{s[0]}x{s[1]}_from_{s[2]}x{s[3]}" for n, t, s in UPSCALES])
def test_upscale_matches_the_restatement(plugin, oracle, n, tree, size):
    """test_upscale.test_kernel_matches_the_restatement: 1e-4, sky pixels bitwise; the low frame is the oracle's; one store format."""
    w, h, lw, lh = size
    view = big_view(w, h)
    lvl, cam, win = view
    lwin = brt.upscale_window(win, h, lh)
    b, key, _ = _resident(plugin, n, tree, lw, lh, view=(lvl, cam, lwin))
    low, _ = _render_both(plugin, oracle, key, b, (lvl, cam, lwin), lw, lh, flags=0)
    g_low, g_full = plugin.debug_denoise_guides(cam, lwin, lw, lh), plugin.debug_denoise_guides(cam, win, w, h)
    for got_g, (gw, gh) in ((g_low, (lw, lh)), (g_full, (w, h))):
        assert np.array_equal(got_g.view(U32), dr.guides(oracle, b, cam, gw, gh).view(U32))
    got = _upscale_dev(plugin, cam, win, lw, lh, low, w, h).view(F32)
    want, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    err = np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
    print(f"{n} {tree} {size}: max err {err.max():.3g}, stages {np.bincount(stage.ravel(), minlength=5).tolist()}")
    assert err.max() <= 1e-4, float(err.max())
    sky = stage == ur.SKY
    assert _same_bits(got[sky], want[sky])
    assert sky.any() and (stage == ur.STAGE_A).any()
    enc = oracle.encode_frame(got, "srgb8")
    got8 = _upscale_dev(plugin, cam, win, lw, lh, low, w, h, out_format=brt.FLAG_OUT_RGBA8_UNORM_SRGB)
    assert np.array_equal(got8.view(enc.dtype).reshape(enc.shape), enc)
    assert _same_bits(_render_upscaled(plugin, cam, win, lw, lh, w, h), got.view(np.uint8).reshape(h, w, -1))
    _assert_path(plugin, n, "one-call form")


def test_upscale_one_call_equals_the_two_step_form(plugin):
    """render_upscaled_device = render_device at the low size + denoise_device + upscale_device bit for bit, DENOISE | TEMPORAL, over
    three frames."""
    import torch
    from test_upscale import _host, _out_tensor
    w, h, lw, lh = 96, 54, 48, 27
    n = BIG
    _resident(plugin, n, "callee", lw, lh)
    flags = DENOISE | TEMPORAL

    def sequence(one_call):
        plugin.reset_temporal()
        frames = []
        for seed in (0.5, 0.25, 0.75):
            lvl, cam, win = big_view(w, h, seed=seed)
            if one_call:
                frames.append(_render_upscaled(plugin, cam, win, lw, lh, w, h, flags=flags))
                _assert_path(plugin, n, "one call")
                continue
            low = _render_low(plugin, lvl, cam, win, lw, lh, h)
            post = torch.empty_like(low)
            plugin.node.denoise_device(cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr(), post.data_ptr(), flags=flags)
            out = _out_tensor(w, h)
            plugin.node.upscale_device(cam, win, lw, lh, post.data_ptr(), w, h, out.data_ptr())
            frames.append(_host(out, h, w))
        return frames

    try:
        one, two = sequence(True), sequence(False)
        for k in range(3):
            assert _same_bits(one[k], two[k]), k
        assert not _same_bits(one[0], one[1])
    finally:
        plugin.reset_temporal()
