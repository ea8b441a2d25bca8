"""The tree the CALLEE builds against brute force, where its leaf boxes are tight (brt_sah.h sah_model_pad; docs/experiments.md "Grazing
rays against the tight boxes").  Every other parity test walks the oracle through the twin of the tree the GPU walked, so a leaf box
that is too tight loses the same hit on both sides.  Here the other side is one leaf of all spheres, and the rays graze a sphere
where it touches a face of its box, from a distance near the tree's reach, in scenes whose pads lie strictly between the rule's floor
and ceiling (tests/graze_cases.py).  CPU: the claim behind the pad as a property of pairs (sphere test, slab test) in numpy f32, and
the oracle's records in the callee's tree against its records in the single leaf.  GPU: ray queries, occlusion and radiance in the
callee's tree against the same kernels on the single leaf."""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
import graze_cases as gc
import query_ref as qr
from helpers import guarded, l1_norm, single_leaf_bvh

F32 = np.float32
LIVE, CEILING = sorted(gc.LIVE), sorted(gc.CEILING)
N_CPU, POOL_CPU = 12000, 400000            # rays per list the oracle walks one by one, out of a pool of grazing rays
N_GPU, POOL_GPU = 262144, 524288
PLAIN, STREAM = 1, 2                       # values of the knob BRT_QUERY_FORM


def _reach_of(models, rays):
    """The reach of the callee's tree for this list by the library's own rule: brt_host_tree_reach for a camera at the list's
    farthest origin -- without big spheres the rule of an origin bound (brt_api_query.cpp) is the same arithmetic, restated here.
    -> (reach the tree is built with, S, the need |o|_1 + S + L in float64 with L = 0)."""
    l1 = np.abs(rays["origin"].astype(np.float64)).sum(axis=1)
    far = rays["origin"][int(np.argmax(l1))]
    cam = brt.cover_camera(16, 9, 1, 1)[1].copy()
    cam["position"][0] = far
    S, level, reach = brt.tree_reach(models, cam)
    assert S == float(gc.scale_of(models))
    need = float(l1.max()) + S
    k = 0 if need <= 2.0 * S else max(1, int(np.ceil(4.0 * np.log2(need / (2.0 * S)))))
    restated = float(F32(2.0 * S * 2.0 ** (0.25 * k))) if k else 0.0
    # (the library lowers a level to 0 where its tree is the tree of the scene's own extent: the same bytes)
    assert reach == restated or (level == 0 and np.array_equal(brt.build_bvh_sah(models, restated).view(np.uint8),
                                                                 brt.build_bvh_sah(models).view(np.uint8))), (level, reach, restated)
    assert max(restated, 2.0 * S) >= need, (restated, S, need)
    return reach, S, need


def _pads_of_tree(models, nodes):
    """leaf half-width minus radius per sphere, from the nodes (y axis; exact up to the rounding of c -+ (r + pad))"""
    pads = np.zeros(len(models))
    for nd in nodes[nodes["model_count"] > 0]:
        pads[nd["index"]] = (float(nd["bounds_max"][1]) - float(nd["bounds_min"][1])) / 2 - float(models[nd["index"]]["radius"])
    return pads


def _assert_pads(name, models, reach, S):
    """The list's scene is what its name says at the reach the library chose: every pad strictly inside (0.01, 0.1), or every pad 0.1;
    and the library's tree has those pads."""
    pad, raw = gc.pad_of(models["radius"], reach, S)
    if name in gc.LIVE:
        assert (raw > gc.PAD_FLOOR).all() and (raw < gc.PAD_CEILING).all(), (name, raw.min(), raw.max())
    else:
        assert (raw > gc.PAD_CEILING).all(), (name, raw.min())
    got = _pads_of_tree(models, brt.build_bvh_sah(models, reach))
    assert np.allclose(got, pad, rtol=0, atol=2.0 ** -24 * 4 * (S + 100.0)), (name, np.abs(got - pad).max())


@functools.lru_cache(maxsize=None)
def _cpu_records(name):
    """-> (rays, beyond, reach, records in the single leaf, in the PLOC tree, in the callee's tree at the library's reach)"""
    import oracle_loader
    oracle = oracle_loader.load()
    models, _ = gc.scene(name)
    rays, idx, rho, beyond = gc.graze_list(name, 1 if name == "counter" else N_CPU, POOL_CPU)
    reach, S, _ = _reach_of(models, rays)
    brute = qr.expected(oracle, models, single_leaf_bvh(models), rays)[0]
    ploc = qr.expected(oracle, models, brt.build_bvh(models), rays)[0]
    callee = qr.expected(oracle, models, brt.build_bvh_sah(models, reach), rays)[0]
    return rays, beyond, reach, brute, ploc, callee


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_restatements_are_the_oracles_arithmetic(oracle):
    """hit_sphere and ray_bounding_dst in numpy f32 are bitwise the oracle's on a subsample of every pool (the boxes: the sphere's own
    at the pad of the rule, which the rays graze)."""
    for name in LIVE + CEILING:
        models, reach = gc.scene(name)
        rays, idx = gc.graze_rays(models, reach, 3000, 3)
        c, r = models["position"][idx], models["radius"][idx]
        t, _ = gc.hit_sphere_np(rays, c, r)
        assert np.array_equal(t.view(np.uint32), gc.oracle_hit_sphere(oracle, rays, c, r).view(np.uint32)), name
        lo, hi = gc.box_of(c, r, gc.pad_of(r, reach, gc.scale_of(models))[0])
        dst = gc.slab_np(rays, lo, hi)
        assert np.array_equal(dst.view(np.uint32), gc.oracle_slab(oracle, rays, lo, hi).view(np.uint32)), name
        assert (t != F32(-1.0)).any() and (t == F32(-1.0)).any() and (dst == qr.NO_HIT).any() and (dst != qr.NO_HIT).any(), name


def test_an_accepted_ray_passes_the_slab_test_of_its_spheres_box():
    """The claim behind the pad, where it is tight: over 2.4e6 grazing rays of the live scenes, a ray that the f32 sphere test accepts
    with t > 0.001 is not a miss of the f32 slab test of sah_model_box's box (the pad rule restated in f32: gc.pad_of).  Not vacuous:
    some accepted rays lie further outside their sphere than 2 * 2^-24 t^2 covers, the bound the rule was written for before (K > 2)."""
    n_rays = n_beyond = n_k2 = 0
    k_max = 0.0
    for name in LIVE:
        models, reach = gc.scene(name)
        S = gc.scale_of(models)
        rays, idx = gc.graze_rays(models, reach, 400000, 5)
        c, r = models["position"][idx], models["radius"][idx]
        pad, raw = gc.pad_of(r, reach, S)
        assert (raw > gc.PAD_FLOOR).all() and (raw < gc.PAD_CEILING).all(), name
        t, disc = gc.hit_sphere_np(rays, c, r)
        accepted = (disc >= F32(0.0)) & (t > F32(0.001))
        lo, hi = gc.box_of(c, r, pad)
        miss = gc.slab_np(rays, lo, hi) == qr.NO_HIT
        rho = gc.rho_of(rays, c, r)
        K = gc.k_of(rho, r, t)[accepted]
        # the bound brt_sah.h derives from hit_sphere's roundings holds for every accepted ray: rho^2 - r^2 <= u (15 D^2 + 2 rho D + r^2)
        D = np.linalg.norm(c.astype(np.float64) - rays["origin"].astype(np.float64), axis=1)
        r64 = r.astype(np.float64)
        assert (((rho - r64) * (rho + r64))[accepted] <= gc.U * (15.0 * D * D + 2.0 * rho * D + r64 * r64)[accepted]).all(), name
        print(f"{name}: {len(rays)} rays, {int(accepted.sum())} accepted, {int((K > 0).sum())} of them from outside, {int((K > 2).sum())} with "
              f"K > 2, largest K {K.max():.3f}, longest t {t[accepted].max():.1f} of reach {reach}; lost {int((accepted & miss).sum())}")
        assert not (accepted & miss).any(), (name, int((accepted & miss).sum()), rays[accepted & miss][:2])
        assert miss.any(), name                                   # (the rays do leave the boxes: delta runs to 3 pads)
        n_rays, n_beyond, n_k2, k_max = n_rays + len(rays), n_beyond + int((K > 0).sum()), n_k2 + int((K > 2).sum()), max(k_max, float(K.max()))
    print(f"{n_rays} rays, {n_beyond} accepted from outside their sphere, {n_k2} with K > 2, largest K {k_max:.3f}")
    assert n_rays >= 2000000 and n_k2 >= 100


@pytest.mark.parametrize("name", LIVE)
def test_reference_tree_equals_brute_force_on_the_live_lists(name):
    """On the reference alone: the 0.1-padded PLOC tree loses nothing on these lists (the seeds are kept for that), and the lists graze:
    at least 100 rays hit with their line outside the sphere they graze (rho > r in float64)."""
    rays, beyond, _, brute, ploc, _ = _cpu_records(name)
    qr.assert_hits_equal(ploc, brute, f"{name}: PLOC tree against the single leaf")
    hit = (brute["status"] & brt.QUERY_STATUS_HIT) != 0
    print(f"{name}: {len(rays)} rays, {int(hit.sum())} hit, {int((hit & beyond).sum())} of them accepted from outside the sphere they graze")
    assert int((hit & beyond).sum()) >= 100


@pytest.mark.parametrize("name", LIVE + ["counter"])
def test_callee_tree_equals_brute_force_in_the_oracle(name):
    """Every ray's oracle_raycast record in the callee's tree, built for the reach the library's rule gives the list, is bitwise its
    record in one leaf of all spheres.  No ray is excused."""
    models, _ = gc.scene(name)
    rays, beyond, reach, brute, _, callee = _cpu_records(name)
    if name in gc.LIVE:
        _assert_pads(name, models, reach, gc.scale_of(models))
    else:
        assert brt.tree_reach(models, _camera_at(rays["origin"][0]))[1] == 0 and brute["t"][0] == gc.COUNTER_T
        qr.assert_hits_equal(qr.expected(_oracle(), models, brt.build_bvh_sah(models), rays)[0], brute, "counter-example, reach 0")
    qr.assert_hits_equal(callee, brute, f"{name}: callee's tree (reach {reach}) against the single leaf")


@pytest.mark.parametrize("name", CEILING)
def test_callee_tree_equals_the_reference_tree_at_the_ceiling(name):
    """Where every pad is the reference's own 0.1 the callee's tree answers as the reference's PLOC tree does."""
    models, _ = gc.scene(name)
    rays, beyond, reach, brute, ploc, callee = _cpu_records(name)
    _assert_pads(name, models, reach, gc.scale_of(models))
    qr.assert_hits_equal(callee, ploc, f"{name}: callee's tree (reach {reach}) against the PLOC tree")
    assert int((((ploc["status"] & brt.QUERY_STATUS_HIT) != 0) & beyond).sum()) >= 100


def test_headline_trees_keep_the_floor():
    """Every ordinary leaf pad of the cover and the RTIOW scenes is the 0.01 floor at reach 0 -- the rule's constant does not reach
    the headline tree's bytes -- and their big spheres keep 0.1."""
    for kind in (brt.SCENE_COVER, brt.SCENE_RTIOW_FINAL):
        for seed in (1, 2, 3):
            m = brt.generate_scene(kind, seed).models
            ordinary = m["radius"] <= 100
            ap = np.abs(m["position"][ordinary]).astype(F32)
            S = F32((((ap[:, 0] + ap[:, 1]) + ap[:, 2]) + m["radius"][ordinary]).max())
            pad, raw = gc.pad_of(m["radius"][ordinary], 0.0, S)
            assert raw.max() < gc.PAD_FLOOR / F32(2.0) and (pad == gc.PAD_FLOOR).all(), (kind, seed, raw.max())
            nodes = brt.build_bvh_sah(m)
            for nd in nodes[nodes["model_count"] > 0]:
                c, r = m[nd["index"]]["position"], F32(m[nd["index"]]["radius"])
                half = r + (gc.PAD_FLOOR if r <= 100 else gc.PAD_CEILING)
                assert np.array_equal(nd["bounds_min"], c - half) and np.array_equal(nd["bounds_max"], c + half), (kind, seed, nd["index"])


def _oracle():
    import oracle_loader
    return oracle_loader.load()


def _camera_at(position):
    cam = brt.cover_camera(16, 9, 1, 1)[1].copy()
    cam["position"][0] = position
    return cam


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def _query(plugin, rays, form, mode=brt.QUERY_CLOSEST, device=False, origin_bound=0.0):
    import torch
    with plugin.tuning(BRT_QUERY_FORM=form):
        if not device:
            hits = plugin.node.query_rays(rays, mode, origin_bound)
        else:
            d_rays = _dev(rays)
            d_hits = guarded(rays.size * 32, 0, 0xAB)
            plugin.node.query_rays_device(d_rays.data_ptr(), rays.size, d_hits.data_ptr(), mode, origin_bound)
            torch.cuda.synchronize()
            hits = d_hits.cpu().numpy().view(brt.HIT_DTYPE)
        assert plugin.node.last_query_stats["form"] == form - 1
    return hits


def _radiance(plugin, rays, bounces, origin_bound):
    import torch
    d_rays = _dev(rays)
    d_out = guarded(rays.size * 32, 0, 0xAB)
    plugin.node.radiance_rays((d_rays.data_ptr(), rays.size, d_out.data_ptr()), 1, bounces, origin_bound, device=True)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(brt.RADIANCE_DTYPE)


def _gpu_list(name):
    models, _ = gc.scene(name)
    rays, idx, rho, beyond = gc.graze_list(name, N_GPU, POOL_GPU)
    l1 = gc.l1_f32(rays["origin"])
    bound = l1_norm(rays["origin"][int(np.argmax(l1))])
    assert bound == float(l1.max())
    return models, rays, beyond, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIVE + ["counter"] + CEILING)
def test_gpu_callee_tree_equals_gpu_brute_force(plugin, oracle, name):
    """262 144 grazing rays per scene through brt_query_rays / brt_query_rays_device, both forms, in the callee's tree (bvh = NULL,
    origin_bound = the list's largest 1-norm) against the same list through one leaf of all spheres uploaded as the caller's tree --
    brute force on the same kernel: t, normal, material, status and user of every ray bitwise, closest hit and occlusion.  The
    ceiling scenes: against the caller's PLOC tree.  2 000 rays of each side against oracle_raycast."""
    models, rays, beyond, bound = _gpu_list(name)
    mats = gc.materials()
    sub = np.arange(0, len(rays), len(rays) // 2000)[:2000]
    other = brt.build_bvh(models) if name in gc.CEILING else single_leaf_bvh(models)
    plugin.node.write_buffers(brt.Buffers(models, mats, other))
    want = _query(plugin, rays, PLAIN)
    assert plugin.node.last_query_stats["refused"] == 0
    assert _query(plugin, rays, STREAM, device=True).tobytes() == want.tobytes(), f"{name}: the other tree, streaming form"
    want_any = _query(plugin, rays, PLAIN, brt.QUERY_ANY)
    qr.assert_hits_equal(want[sub], qr.expected(oracle, models, other, rays[sub])[0], f"{name}: GPU in the other tree against the oracle")

    plugin.node.write_buffers(brt.Buffers(models, mats, None))
    got = _query(plugin, rays, PLAIN, origin_bound=bound)
    st = dict(plugin.node.last_query_stats)
    # the reach covers the list's need |o|_1 + S + L (float64, L = 0: no big sphere), the bound refuses nothing
    S = float(gc.scale_of(models))
    need = float(np.abs(rays["origin"].astype(np.float64)).sum(axis=1).max()) + S
    print(f"{name}: tree_reach {st['tree_reach']}, rebuilt {st['tree_rebuilt']}, need {need:.3f}, S {S}, origin bound {plugin.node.query_origin_bound()}"
          f" >= {bound}; form {st['form']}, {st['n_workgroups']} workgroups, {st['rays_walked']} rays walked, {st['hits']} hits, "
          f"{int(beyond.sum())} rays accepted from outside their sphere")
    assert max(st["tree_reach"], 2.0 * S) >= need and plugin.node.query_origin_bound() >= bound
    assert st["refused"] == 0 and st["rays_walked"] == len(rays) and not (got["status"] & ~np.uint32(3)).any()
    if name != "counter":
        _assert_pads(name, models, st["tree_reach"], gc.scale_of(models))
        assert int((((want["status"] & brt.QUERY_STATUS_HIT) != 0) & beyond).sum()) >= 100
    twin = brt.build_bvh_sah(models, st["tree_reach"])
    qr.assert_hits_equal(got[sub], qr.expected(oracle, models, twin, rays[sub])[0], f"{name}: GPU in the callee's tree against the oracle in its twin")
    qr.assert_hits_equal(got, want, f"{name}: callee's tree against the other tree, plain form")
    for form, device in ((STREAM, False), (PLAIN, True), (STREAM, True)):
        qr.assert_hits_equal(_query(plugin, rays, form, device=device, origin_bound=bound), want, f"{name}: form {form}, device {device}")
    for form in (PLAIN, STREAM):
        got_any = _query(plugin, rays, form, brt.QUERY_ANY, device=True, origin_bound=bound)
        assert np.array_equal(got_any["status"], want_any["status"]), f"{name}: occlusion, form {form}"
    assert np.array_equal((want_any["status"] & brt.QUERY_STATUS_HIT) != 0, (want["status"] & brt.QUERY_STATUS_HIT) != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIVE + ["counter"])
def test_gpu_radiance_in_the_callee_tree_equals_the_single_leaf(plugin, name):
    """brt_radiance_rays_device over the first 4096 rays of the list (where the rays accepted from outside their sphere are), one
    sample, 0 and 2 bounces: the records in the callee's tree are bitwise those in one leaf of all spheres."""
    models, rays, beyond, bound = _gpu_list(name)
    mats = gc.materials()
    rr = np.zeros(4096, brt.RADIANCE_RAY_DTYPE)
    rr["origin"], rr["direction"], rr["user"] = rays["origin"][:4096], rays["direction"][:4096], rays["user"][:4096]
    rr["seed"] = np.arange(4096, dtype=np.uint32) * np.uint32(747796405) + np.uint32(1)
    plugin.node.write_buffers(brt.Buffers(models, mats, single_leaf_bvh(models)))
    want = {b: _radiance(plugin, rr, b, 0.0) for b in (0, 2)}
    plugin.node.write_buffers(brt.Buffers(models, mats, None))
    for b in (0, 2):
        got = _radiance(plugin, rr, b, bound)
        st = plugin.node.last_radiance_stats
        assert st["refused"] == 0 and (name == "counter" or beyond[:4096].sum() >= 100)
        assert ((want[b]["status"] & brt.QUERY_STATUS_HIT) != 0).any()
        bad = (got.view(np.uint8).reshape(4096, 32) != want[b].view(np.uint8).reshape(4096, 32)).any(axis=1)
        assert not bad.any(), f"{name}, {b} bounces: {int(bad.sum())} records differ, first {np.flatnonzero(bad)[:4].tolist()}: {got[bad][:2]} / {want[b][bad][:2]}"
