"""Radiance queries and probe bakes against the C oracle's caller-ray entry (oracle/bevyray_oracle.c oracle_radiance), at the scale the
numpy restatement cannot reach.  CPU: oracle_radiance byte for byte against tests/radiance_ref.py (two independently written statements of
the rule); the frame identity -- a one-sample Pure frame of the oracle is, pixel by pixel, the radiance of that pixel's first-sample ray
from the rng state after its jitter (oracle_first_sample_ray) --; order independence.  GPU: both kernel forms bitwise against the oracle
on 40 randomized scenes of test_parity_gpu's generator under three scene placements, with the table of kernel instantiations that ran; the edge
ray sets of tests/query_ref.py; whole frames; sample and bounce counts on lists of several workgroups; probe bakes."""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
import probe_ref as pr
import query_ref as qr
import radiance_ref as rr
import test_radiance as tr
from helpers import _random_case, big_scene, big_view, median_split_bvh

F32 = np.float32
PLAIN, STREAM = tr.PLAIN, tr.STREAM
HIT = brt.QUERY_STATUS_HIT
N_CASES, N_ENTRIES = 40, 2048
SETTINGS = {"default": {}, "lds_top": {"BRT_FORCE_LDS_TOP": 5}, "global": {"BRT_FORCE_GLOBAL_SCENE": 1}}
MODES = {1: "LDS", 2: "LDS_TOP", 0: "GLOBAL"}           # last_stats["scene_in_lds"] -> the streaming kernel's MODE
DESC16_MAX_INDEX = 0x3FFE                               # brt_layout.h


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cases():
    """40 consecutive draws of the frame tests' generator of randomized scenes (helpers._random_case) from default_rng(2024): fractional
    metallic and specular_transmission, ior below 1, giant ground spheres; PLOC, single-leaf, median-split and chain trees."""
    rng = np.random.default_rng(2024)
    return [_random_case(rng) for _ in range(N_CASES)]


def _entries(case, n=N_ENTRIES):
    """The entries of a randomized case: origins in [-8, 8]^3, normal directions, the even entries aimed into [-4, 4]^3."""
    r = np.random.default_rng(case)
    o = r.uniform(-8, 8, (n, 3)).astype(F32)
    d = r.normal(size=(n, 3)).astype(F32)
    d[0::2] = (r.uniform(-4, 4, (n // 2, 3)).astype(F32) - o[0::2]).astype(F32)
    return rr.make_rays(o, d, r.integers(0, 2 ** 32, n, dtype=np.uint32))


def _bounces(case):
    return int(_cases()[case][2][0]["bounce_count"])


_WANT = {}


def _want_case(oracle, case, n=N_ENTRIES, samples=3, bounces=None):
    """The oracle's records and counters of a randomized case's entries, once per module."""
    bounces = _bounces(case) if bounces is None else bounces
    key = (case, n, samples, bounces)
    if key not in _WANT:
        _WANT[key] = oracle.radiance(_cases()[case][0], _entries(case, n), samples, bounces)
    return _WANT[key]


def _is_hit(records):
    return (records["status"] & HIT) != 0


def _nan_entries(records):
    return np.isnan(records["rgb"]).any(axis=1)


def _pure_one_sample(lvl, cam):
    lvl, cam = lvl.copy(), cam.copy()
    lvl["level"] = int(brt.Raytracing.Pure)
    cam["sample_count"] = 1
    return lvl, cam


def _first_sample_list(oracle, cam, win, w, h):
    o, d, states = oracle.first_sample_rays(cam, win, w, h)
    return rr.make_rays(o, d, states, user=np.arange(w * h, dtype=np.uint32))


def _reachable(bvh):
    """The nodes the root reaches, with their depths (a node array may hold others: the upload encodes what the walk can visit)."""
    depth, todo = {0: 0}, [0]
    while todo:
        n = todo.pop()
        if bvh[n]["model_count"] == 0:
            for c in (int(bvh[n]["index"]), int(bvh[n]["index"]) + 1):
                depth[c] = depth[n] + 1
                todo.append(c)
    return depth


def tree_is_simple(bvh):
    """brt_host.cpp: every leaf holds one sphere and max leaf depth + 1 < 31 (the nodes the root reaches)."""
    depth = _reachable(bvh)
    leaves = [n for n in depth if bvh[n]["model_count"] > 0]
    return all(bvh[n]["model_count"] == 1 for n in leaves) and max(depth[n] for n in leaves) + 1 < 31


def tree_is_desc16(b):
    """brt_host.cpp: spheres, pair records (interior nodes) and multi-sphere leaves each number at most DESC16_MAX_INDEX."""
    counts = b.bvh["model_count"][sorted(_reachable(b.bvh))]
    interior, general = int((counts == 0).sum()), int((counts > 1).sum())
    return len(b.models) <= DESC16_MAX_INDEX and interior <= DESC16_MAX_INDEX and general <= DESC16_MAX_INDEX


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------

def test_the_oracle_equals_the_numpy_restatement_on_the_standard_set(oracle):
    b = tr._cover()
    for samples in tr.SAMPLES:
        for bounces in tr.BOUNCES:
            want, counts = tr._want("caller", samples, bounces)
            got, cnt = oracle.radiance(b, tr._standard(), samples, bounces)
            assert got.tobytes() == want.tobytes(), (samples, bounces)
            assert cnt["rays"] == counts["raycasts"], (samples, bounces, cnt, counts)
            assert int(_is_hit(got).sum()) == counts["hit_entries"]


def test_the_oracle_equals_the_numpy_restatement_on_randomized_scenes(oracle):
    kinds = dict.fromkeys(("metal", "glass", "diffuse", "hit_entries", "miss_entries"), 0)      # (absorbed paths: the standard set's)
    for case in range(5):
        b, _, cam, _, _, _ = _cases()[case]
        rays = _entries(case)[:24]
        want, counts = rr.expected(b.models, b.materials, b.bvh, cam, rays, 3, _bounces(case))
        got, cnt = oracle.radiance(b, rays, 3, _bounces(case))
        assert got.tobytes() == want.tobytes(), case
        assert cnt["rays"] == counts["raycasts"], (case, cnt, counts)
        for k in kinds:
            kinds[k] += counts[k]
    print(kinds)
    assert all(v > 0 for v in kinds.values()), kinds


def _frame_identity(oracle, b, lvl, cam, win, w, h):
    lvl, cam = _pure_one_sample(lvl, cam)
    frame, counters = oracle.render(b, lvl, cam, win, w, h, threads=1)
    rays = _first_sample_list(oracle, cam, win, w, h)
    got, cnt = oracle.radiance(b, rays, 1, int(cam[0]["bounce_count"]))
    assert np.array_equal(got["rgb"].view(np.uint32).reshape(h, w, 3), frame[..., :3].view(np.uint32))
    assert (frame[..., 3] == 1.0).all()
    assert cnt["rays"] == counters["rays"] and cnt == counters
    return got


def test_a_one_sample_frame_is_the_radiance_of_its_first_sample_rays(oracle):
    lvl, cam, win = brt.cover_camera(48, 27, 1, 4)
    got = _frame_identity(oracle, tr._cover(), lvl, cam, win, 48, 27)
    assert _is_hit(got).any() and (~_is_hit(got)).any()
    # a randomized scene with its own camera, window height and frame size: the first one whose frame shows spheres and sky
    for case in range(N_CASES):
        b, lvl, cam, win, w, h = _cases()[case]
        if w * h < 400 or _bounces(case) < 2:
            continue
        got = _frame_identity(oracle, b, lvl, cam, win, w, h)
        if _is_hit(got).sum() > 50 and (~_is_hit(got)).sum() > 50:
            break
    else:
        raise AssertionError("no randomized case shows spheres and sky")


def test_the_oracle_does_not_depend_on_the_lists_order(oracle):
    b = _cases()[1][0]
    rays = _entries(1)
    want, cnt = _want_case(oracle, 1)
    perm = np.random.default_rng(9).permutation(len(rays))
    got, cnt_p = oracle.radiance(b, rays[perm], 3, _bounces(1))
    assert got.tobytes() == want[perm].tobytes() and cnt_p == cnt
    assert len(np.unique(want["rgb"], axis=0)) > 100                  # (not one colour everywhere)


def test_the_randomized_entries_hit_and_miss(oracle):
    hits = nans = 0
    for case in range(N_CASES):
        want, _ = _want_case(oracle, case)
        hits += int(_is_hit(want).sum())
        nans += int(_nan_entries(want).sum())
    total = N_CASES * N_ENTRIES
    print(f"randomized scenes: {hits} hits, {total - hits} misses, {nans} NaN of {total}")
    assert hits >= total // 4 and total - hits >= total // 4 and nans == 0


def test_tree_is_simple_follows_the_upload_rule():
    from helpers import chain_bvh, make_buffers, median_split_bvh, single_leaf_bvh
    data = [((0.0, 0.0, -5.0 - i), 0.5, brt.StandardMaterial()) for i in range(40)]
    assert tree_is_simple(make_buffers(data[:30], chain_bvh).bvh)                  # 30 spheres: depth 29
    assert not tree_is_simple(make_buffers(data[:31], chain_bvh).bvh)              # depth 30
    assert not tree_is_simple(make_buffers(data[:2], single_leaf_bvh).bvh)
    assert tree_is_simple(make_buffers(data[:1], single_leaf_bvh).bvh)
    assert tree_is_simple(make_buffers(data, lambda m: median_split_bvh(m, 1)).bvh)
    assert not tree_is_simple(make_buffers(data, lambda m: median_split_bvh(m, 3)).bvh)
    assert tree_is_simple(make_buffers(data).bvh)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

def assert_equal(got, want, b, what):
    """rr.assert_equal, and: where the oracle's rgb component is NaN the kernel's is NaN (payload free), every other word equal; `sphere`
    is a caller's index of that material on hits and QUERY_NONE elsewhere."""
    assert got.shape == want.shape, what
    for f in ("t", "material", "status", "user"):
        bad = got[f].view(np.uint32) != want[f].view(np.uint32)
        assert not bad.any(), f"{what}: field {f}: {bad.sum()} of {len(got)} entries differ, first {np.flatnonzero(bad)[:4].tolist()}: got {got[bad][:2]}, want {want[bad][:2]}"
    wn = np.isnan(want["rgb"])
    assert np.isnan(got["rgb"][wn]).all(), f"{what}: a NaN of the oracle is a number: entries {np.flatnonzero((wn & ~np.isnan(got['rgb'])).any(axis=1))[:4].tolist()}"
    bad = ((got["rgb"].view(np.uint32) != want["rgb"].view(np.uint32)) & ~wn).any(axis=1)
    assert not bad.any(), f"{what}: rgb: {bad.sum()} of {len(got)} entries differ, first {np.flatnonzero(bad)[:4].tolist()}: got {got[bad][:2]}, want {want[bad][:2]}"
    hit = _is_hit(want)
    assert (got["sphere"][~hit] == brt.QUERY_NONE).all(), what
    assert (got["sphere"][hit] < len(b.models)).all() and (b.models["material_id"][got["sphere"][hit]] == got["material"][hit]).all(), what


def test_the_comparison_notices_one_bit(oracle):
    b = tr._cover()
    rays = tr._standard().copy()
    rays["direction"][5] *= F32(1e-30)                                  # (d . d underflows: the oracle's colour of this entry is NaN)
    want, _ = oracle.radiance(b, rays, 2, 4)
    assert _nan_entries(want)[5] and _is_hit(want).sum() > 10 and (~_is_hit(want)).sum() > 10
    good = want.copy()
    hit = np.flatnonzero(_is_hit(want))
    good["sphere"][hit] = [int(np.flatnonzero(b.models["material_id"] == m)[0]) for m in want["material"][hit]]
    nan = np.isnan(good["rgb"])
    good["rgb"].view(np.uint32)[nan] = 0xFFC12345                       # another NaN: the payload is free
    assert_equal(good, want, b, "the oracle's own records")
    edits = {"rgb bit": lambda r: r["rgb"].view(np.uint32).__setitem__((7, 1), r["rgb"].view(np.uint32)[7, 1] ^ 1),
             "t bit": lambda r: r["t"].view(np.uint32).__setitem__(hit[0], r["t"].view(np.uint32)[hit[0]] ^ 1),
             "status": lambda r: r["status"].__setitem__(hit[1], r["status"][hit[1]] ^ brt.QUERY_STATUS_FRONT_FACE),
             "user": lambda r: r["user"].__setitem__(0, 1), "material": lambda r: r["material"].__setitem__(hit[2], 0xFFFFFFFF),
             "a number for a NaN": lambda r: r["rgb"].__setitem__(nan, 0.5), "a NaN for a number": lambda r: r["rgb"].__setitem__((9, 0), np.nan),
             "sphere of a miss": lambda r: r["sphere"].__setitem__(np.flatnonzero(~_is_hit(want))[0], 3),
             "sphere out of range": lambda r: r["sphere"].__setitem__(hit[0], len(b.models))}
    for name, edit in edits.items():
        bad = good.copy()
        edit(bad)
        with pytest.raises(AssertionError):
            assert_equal(bad, want, b, name)


_TABLE = {}        # kernel instantiation -> the first hits of the lists it traced


def _ran(plugin, b, scene_in_lds, n, hits):
    """Enters the instantiation of the call that just returned: the form and the workgroup count from its stats, the placement from the
    stats of a frame of the same scene under the same knobs, descriptor width and tree class from the tree."""
    st = plugin.node.last_radiance_stats
    d16 = tree_is_desc16(b)
    if st["form"] == 0:
        assert st["n_workgroups"] == -(-n // 256), st
        key = ("k_radiance_plain", "D16" if d16 else "D32")
    else:
        mode = MODES[scene_in_lds]
        assert d16 or mode == "GLOBAL"
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        useful = -(-n // (256 if mode == "GLOBAL" else 1024))
        # plan_stream: a workgroup per 1024 (256: global) entries, at most one per CU where the scene or its top is staged (no
        # global-memory list here has more than a workgroup per CU)
        assert st["n_workgroups"] == min(useful, cus) and (mode != "GLOBAL" or useful <= cus), (mode, st)
        key = ("k_radiance_stream", mode, "D16" if d16 else "D32", "SIMPLE" if tree_is_simple(b.bvh) else "GENERAL")
    _TABLE[key] = _TABLE.get(key, 0) + hits
    return key


def _check(plugin, b, rays, want, cnt, samples, bounces, device, scene_in_lds, what):
    """PLAIN against the oracle, STREAM byte for byte against PLAIN, the stats of both."""
    n_hits = int(_is_hit(want).sum())
    stats = (cnt["rays"] - (samples - 1) * len(rays), n_hits, 0)
    got = tr._radiance(plugin, rays, samples, bounces, PLAIN, device=device)
    assert_equal(got, want, b, f"{what} plain")
    st = plugin.node.last_radiance_stats
    assert (st["walks"], st["hits"], st["refused"]) == stats, (what, "plain", st, stats)
    _ran(plugin, b, scene_in_lds, len(rays), n_hits)
    streamed = tr._radiance(plugin, rays, samples, bounces, STREAM, device=device)
    assert streamed.tobytes() == got.tobytes(), f"{what}: the streaming form differs from the plain one at {np.flatnonzero((streamed.view(np.uint32).reshape(-1, 8) != got.view(np.uint32).reshape(-1, 8)).any(axis=1))[:4].tolist()}"
    st = plugin.node.last_radiance_stats
    assert (st["walks"], st["hits"], st["refused"]) == stats, (what, "stream", st, stats)
    _ran(plugin, b, scene_in_lds, len(rays), n_hits)
    return got


def _upload(plugin, b, lvl, cam, win, w, h):
    """The scene resident under the caller's tree and one frame of it -> where that frame's kernel found the scene."""
    plugin.node.run(lvl, cam, win, w, h, buffers=b)
    return plugin.node.last_stats["scene_in_lds"]


_DONE = set()


def _randomized(plugin, oracle, setting):
    if setting in _DONE:
        return
    with plugin.tuning(**SETTINGS[setting]):
        for case in range(N_CASES):
            b, lvl, cam, win, w, h = _cases()[case]
            placed = _upload(plugin, b, lvl, cam, win, w, h)
            assert placed == {"default": 1, "lds_top": 2, "global": 0}[setting], (case, placed)
            want, cnt = _want_case(oracle, case)
            assert not _nan_entries(want).any()
            _check(plugin, b, _entries(case), want, cnt, 3, _bounces(case), case % 4 == 0, placed, f"{setting} case {case} ({len(b.models)} spheres, {len(b.bvh)} nodes)")
    _DONE.add(setting)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_randomized_scenes(plugin, oracle, setting):
    _randomized(plugin, oracle, setting)


def _desc32(plugin, oracle, tree):
    """The 16 383-sphere scene (32-bit descriptors, walked from global memory) under the PLOC tree with 4096 entries, or under a
    median-split tree of three-sphere leaves with 512 (its boxes overlap everywhere: the oracle pops 6000 nodes per ray)."""
    if ("desc32", tree) in _DONE:
        return
    s = big_scene(16383, 11)
    b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models) if tree == "ploc" else median_split_bvh(s.models, 3))
    assert not tree_is_desc16(b) and tree_is_simple(b.bvh) == (tree == "ploc")
    lvl, cam, win = big_view(tr.W, tr.H)
    placed = _upload(plugin, b, lvl, cam, win, tr.W, tr.H)
    assert placed == 0 and plugin.node.last_stats["hot_records"] == 0
    rng = np.random.default_rng(12)
    n = 4096 if tree == "ploc" else 512
    targets = b.models["position"][rng.integers(0, len(b.models), size=n)]
    o = np.broadcast_to(cam[0]["position"].astype(F32), (n, 3)).copy()
    o[1::4] = (targets[1::4] + rng.uniform(-2, 2, size=(n // 4, 3))).astype(F32)          # a quarter from inside the slab
    d = (targets + rng.uniform(-0.1, 0.1, size=(n, 3)) - o).astype(F32)
    rays = rr.make_rays(o, d, rng.integers(0, 2 ** 32, size=n, dtype=np.uint32))
    want, cnt = oracle.radiance(b, rays, 2, 4)
    assert not _nan_entries(want).any() and _is_hit(want).sum() > n // 2 and cnt["rays"] > 3 * n
    _check(plugin, b, rays, want, cnt, 2, 4, True, placed, f"16 383 spheres, {tree}")
    _DONE.add(("desc32", tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["ploc", "median3"])
def test_a_scene_with_32_bit_descriptors(plugin, oracle, tree):
    _desc32(plugin, oracle, tree)


@pytest.mark.gpu
def test_edge_rays(plugin, oracle):
    b = tr._cover()
    lvl, cam, win = tr._cover_camera()
    placed = _upload(plugin, b, lvl, cam, win, tr.W, tr.H)
    sets = qr.ray_sets(oracle, b.models, b.bvh, cam, tr.W, tr.H, np.random.default_rng(7), n=600)
    assert len(sets) == 8
    for name, q in sets.items():
        rays = rr.make_rays(q["origin"], q["direction"], np.arange(len(q), dtype=np.uint32) * np.uint32(747796405) + np.uint32(1), user=q["user"])
        want, cnt = oracle.radiance(b, rays, 2, 6)
        nans = int(_nan_entries(want).sum())
        print(f"{name}: {len(rays)} entries, {int(_is_hit(want).sum())} hits, {int((~_is_hit(want)).sum())} misses, {nans} NaN")
        if name == "scaled_directions":
            assert 0 < nans < len(rays)
        elif name != "zero_direction":
            assert nans == 0, name
        for device in (False, True):
            _check(plugin, b, rays, want, cnt, 2, 6, device, placed, f"{name} device {device}")


@pytest.mark.gpu
def test_a_frame_is_the_radiance_of_its_first_sample_rays(plugin, oracle):
    w, h = tr.W, tr.H
    b = tr._cover()
    lvl, cam, win = brt.cover_camera(w, h, 1, 4)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    plugin.node.radiance_rays(tr._standard()[:1], 1, 0, origin_bound=20.0)                 # (as test_radiance._upload_cover raises the reach)
    frame = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS).copy()
    st = dict(plugin.node.last_stats)
    twin = brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, st["tree_reach"]))
    ref, counters = oracle.render(twin, lvl, cam, win, w, h)
    assert np.array_equal(frame.view(np.uint32), ref.view(np.uint32)) and st["rays"] == counters["rays"]
    rays = _first_sample_list(oracle, cam, win, w, h)
    assert len(rays) == 5184
    want, cnt = oracle.radiance(twin, rays, 1, 4)
    assert cnt == counters and not _nan_entries(want).any()
    q = np.zeros(len(rays), brt.RAY_DTYPE)
    q["origin"], q["direction"], q["user"], q["t_max"] = rays["origin"], rays["direction"], rays["user"], np.inf
    closest = plugin.node.query_rays(q)
    for device in (False, True):
        got = _check(plugin, twin, rays, want, cnt, 1, 4, device, st["scene_in_lds"], f"frame list device {device}")
        assert np.array_equal(got["rgb"].view(np.uint32).reshape(h, w, 3), frame[..., :3].view(np.uint32))
        assert np.array_equal(got["t"].view(np.uint32), closest["t"].view(np.uint32))
        assert np.array_equal(got["sphere"], closest["sphere"])


@functools.lru_cache(maxsize=None)
def _three_kinds_case(oracle):
    """The first randomized case whose first hits meet a metal (metallic = 1), a glass (metallic = 0, specular_transmission = 1) and a
    diffuse (both 0) material, by the oracle."""
    for case in range(N_CASES):
        b = _cases()[case][0]
        want, _ = _want_case(oracle, case)
        m = b.materials[np.unique(want["material"][_is_hit(want)])]
        metal = (m["metallic"] == 1).any()
        glass = ((m["metallic"] == 0) & (m["specular_transmission"] == 1)).any()
        diffuse = ((m["metallic"] == 0) & (m["specular_transmission"] == 0)).any()
        if metal and glass and diffuse:
            return case
    raise AssertionError("no randomized case meets all three material kinds")


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 2, 5, 64])
def test_samples_and_bounces(plugin, oracle, samples):
    case = _three_kinds_case(oracle)
    b, lvl, cam, win, w, h = _cases()[case]
    placed = _upload(plugin, b, lvl, cam, win, w, h)
    rays = _entries(case, 4096)
    seen = set()
    for bounces in (0, 1, 8):
        want, cnt = _want_case(oracle, case, 4096, samples, bounces)
        assert not _nan_entries(want).any() and 400 < _is_hit(want).sum() < 3696
        _check(plugin, b, rays, want, cnt, samples, bounces, False, placed, f"case {case} samples {samples} bounces {bounces}")
        seen.add(want["rgb"].tobytes())
    assert len(seen) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1])
def test_a_list_longer_than_the_launch(plugin, oracle, case):
    """More entries than a streaming launch that fills the device has lanes, by 4098: every lane takes an entry at once, and the rest go
    to whichever lanes end first -- those whose entry missed -- while their neighbours are mid-path.  Case 0: a tree with multi-sphere
    leaves, 2 bounces; case 1: a PLOC tree (the hand-written walk loop), 10 bounces."""
    import torch
    b, lvl, cam, win, w, h = _cases()[case]
    assert tree_is_simple(b.bvh) == (case == 1)
    placed = _upload(plugin, b, lvl, cam, win, w, h)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 1024 + 4098
    want, cnt = _want_case(oracle, case, n)
    assert not _nan_entries(want).any() and n // 8 < _is_hit(want).sum() < n - n // 8
    _check(plugin, b, _entries(case, n), want, cnt, 3, _bounces(case), True, placed, f"case {case}, {n} entries")
    assert placed == 1 and plugin.node.last_radiance_stats["n_workgroups"] == cus
    del _WANT[case, n, 3, _bounces(case)]


def _probes(seed, n=64):
    rng = np.random.default_rng(seed)
    probes = np.zeros(n, brt.PROBE_DTYPE)
    probes["position"] = rng.uniform(-6, 6, (n, 3)).astype(F32)
    probes["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    probes["seed"][1], probes["seed"][2], probes["seed"][n - 1] = 0, 0xFFFFFFFF, 0xFFFFFFFF - 5      # seed + k * 0x9E3779B9 wraps from k = 1 on
    return probes


def _bake_checks(plugin, oracle, b, probes, what, chunked):
    for n_dirs in (1, 65, 256, 1000):
        dirs = brt.probe_directions(n_dirs)
        res, cnt = oracle.radiance(b, pr.make_rays(probes, dirs), 1, 8)
        bad = np.flatnonzero(_nan_entries(res))
        assert len(bad) == 0, f"{what} n_dirs {n_dirs}: the oracle's colour is NaN at (probe, direction) {[(int(i) // n_dirs, int(i) % n_dirs) for i in bad[:4]]}"
        for basis in (pr.SH9, pr.CUBE):
            want = pr.project(res, dirs, basis)
            assert not np.isnan(want["coeff"]).any(), (what, n_dirs, basis)
            knobs = {"BRT_PROBE_CHUNK_RAYS": 6000} if chunked and n_dirs == 256 else {}
            with plugin.tuning(**knobs):
                got = plugin.node.bake_probes(probes, n_dirs, 8, basis)
            pr.assert_records_equal(got, want, f"{what} n_dirs {n_dirs} basis {basis}")
            st = plugin.node.last_probe_stats
            assert (st["walks"], st["hits"], st["refused"]) == (cnt["rays"], int(want["hits"].sum()), 0), (what, n_dirs, basis, st)
            assert st["hits"] == int(_is_hit(res).sum())
            if knobs:
                assert st["chunks"] >= 3, st
            if n_dirs == 1000:
                assert 0 < want["hits"].sum() < len(probes) * n_dirs


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_probe_bakes_on_randomized_scenes(plugin, oracle, case):
    b = _cases()[case][0]
    plugin.node.write_buffers(b)
    _bake_checks(plugin, oracle, b, _probes(50 + case), f"case {case}", chunked=case == 0)


@pytest.mark.gpu
def test_probe_bakes_on_the_callees_tree(plugin, oracle):
    b = tr._cover()
    probes = _probes(54)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    plugin.node.bake_probes(probes[:1], 1, 0, pr.SH9, origin_bound=40.0)
    reach = plugin.node.last_probe_stats["tree_reach"]
    assert plugin.node.query_origin_bound() >= 18.0
    twin = brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, reach))
    _bake_checks(plugin, oracle, twin, probes, "cover, callee's tree", chunked=False)


INSTANTIATIONS = [("k_radiance_stream", mode, "D16", tree) for mode in ("LDS", "LDS_TOP", "GLOBAL") for tree in ("SIMPLE", "GENERAL")] + [
    ("k_radiance_stream", "GLOBAL", "D32", "SIMPLE"), ("k_radiance_stream", "GLOBAL", "D32", "GENERAL"),
    ("k_radiance_plain", "D16"), ("k_radiance_plain", "D32")]        # all eight of k_radiance_stream, both of k_radiance_plain


@pytest.mark.gpu
def test_every_instantiation_ran(plugin, oracle):
    """The table of the module: every instantiation of the two kernels that the public knobs reach traced a list with first hits.  (The
    tests above fill it; what has not run yet -- this test selected alone -- runs here.)"""
    for setting in SETTINGS:
        _randomized(plugin, oracle, setting)
    for tree in ("ploc", "median3"):
        _desc32(plugin, oracle, tree)
    for key in sorted(_TABLE):
        print(key, _TABLE[key])
    for key in INSTANTIATIONS:
        assert _TABLE.get(key, 0) > 0, (key, _TABLE)
