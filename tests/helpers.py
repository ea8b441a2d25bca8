"""Shared test helpers: hand-made BVHs (single leaf, median split, caterpillar chain, a composer that grafts one onto another),
a seeded scene large enough for 32-bit tree descriptors with its camera, the upload of a scene whose tree the callee builds,
uniform builders, the generator of randomized scenes (materials, sizes, cameras, topologies), the generator of wild scenes that
scripts/fuzz_parity.py and tests/shade_cases.py share, the scene and view generators that scripts/sequence_soak.py and
tests/sequence_cases.py share, and a numpy-f32 restatement of the
camera/sky arithmetic for analytic checks; for the GPU tests of the bakes, device buffers and the upload of the cover scene."""
import functools
import os

import numpy as np

import bevyray_amd as brt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _padded_boxes(models):
    pos = models["position"].astype(np.float32)
    pad = (models["radius"].astype(np.float32) + F32(0.1))[:, None]   # Model::aabb, extract.rs:220-227
    return pos - pad, pos + pad


def single_leaf_bvh(models):
    """One leaf holding every model: the reference's own loop then tests all spheres
    (raytrace.wgsl:325-326,349) -- the brute-force truth."""
    lo, hi = _padded_boxes(models)
    nodes = np.zeros(1, brt.BVH_NODE_DTYPE)
    nodes[0]["bounds_min"], nodes[0]["bounds_max"] = lo.min(0), hi.max(0)
    nodes[0]["index"], nodes[0]["model_count"] = 0, len(models)
    return nodes


def median_split_bvh(models, leaf_size=2):
    """Splits the model ARRAY at its midpoint (no reordering, so leaves are contiguous model
    ranges); leaves hold up to leaf_size models -> exercises multi-model leaves."""
    lo, hi = _padded_boxes(models)
    nodes = [None]

    def build(slot, a, b):
        box = (lo[a:b].min(0), hi[a:b].max(0))
        if b - a <= leaf_size:
            nodes[slot] = (box, a, b - a)
            return
        first = len(nodes)
        nodes.extend([None, None])
        nodes[slot] = (box, first, 0)
        mid = (a + b) // 2
        build(first, a, mid)
        build(first + 1, mid, b)

    build(0, 0, len(models))
    out = np.zeros(len(nodes), brt.BVH_NODE_DTYPE)
    for i, (box, index, count) in enumerate(nodes):
        out[i]["bounds_min"], out[i]["bounds_max"] = box
        out[i]["index"], out[i]["model_count"] = index, count
    return out


def chain_bvh(models, far_first=False):
    """Caterpillar: level k has leaf `2k+1` (popped LAST, raytrace.wgsl:332-340) and interior
    `2k+2`; the bottom holds two leaves.  Leaf at level k = model n-1-k, so model 0 is at the
    bottom.  Every interior box is the union box.  Depth n-1."""
    n = len(models)
    assert n >= 2
    lo, hi = _padded_boxes(models)
    order = list(range(n - 1, -1, -1))
    if far_first:
        order = order[::-1]
    nodes = np.zeros(2 * n - 1, brt.BVH_NODE_DTYPE)
    union = (lo.min(0), hi.max(0))
    cur = 0
    for k in range(n - 1):
        nodes[cur]["bounds_min"], nodes[cur]["bounds_max"] = union
        nodes[cur]["index"], nodes[cur]["model_count"] = 2 * k + 1, 0
        m = order[k]
        leaf = 2 * k + 1
        nodes[leaf]["bounds_min"], nodes[leaf]["bounds_max"] = lo[m], hi[m]
        nodes[leaf]["index"], nodes[leaf]["model_count"] = m, 1
        cur = 2 * k + 2
    m = order[n - 1]
    nodes[cur]["bounds_min"], nodes[cur]["bounds_max"] = lo[m], hi[m]
    nodes[cur]["index"], nodes[cur]["model_count"] = m, 1
    return nodes


def graft_bvh(top, leaf_slot, sub, model_offset):
    """`top` with its leaf `leaf_slot` turned into an interior node over {that leaf, the root of `sub`}: a composer of node arrays.
    `sub` is a tree over models[model_offset:] numbered from 0; its leaves are moved by model_offset, its interior indices by where
    its nodes land (appended behind `top`, the two children of every interior node still adjacent).  Every interior box of the
    result is refitted bottom-up (children lie behind their parent in every array this module makes), so the boxes above the
    graft enclose the grafted spheres."""
    assert top[leaf_slot]["model_count"] > 0
    base = len(top) + 1                                      # where sub's node 0 lands
    out = np.zeros(len(top) + 1 + len(sub), brt.BVH_NODE_DTYPE)
    out[:len(top)] = top
    out[len(top)] = top[leaf_slot]
    moved = sub.copy()
    leaf = moved["model_count"] > 0
    moved["index"][leaf] += model_offset
    moved["index"][~leaf] += base
    out[base:] = moved
    out[leaf_slot]["index"], out[leaf_slot]["model_count"] = len(top), 0
    for i in range(len(out) - 1, -1, -1):
        if out[i]["model_count"] == 0:
            a, b = out[out[i]["index"]], out[out[i]["index"] + 1]
            out[i]["bounds_min"] = np.minimum(a["bounds_min"], b["bounds_min"])
            out[i]["bounds_max"] = np.maximum(a["bounds_max"], b["bounds_max"])
    return out


def big_scene(n, seed, n_materials=48):
    """-> Buffers(models, materials, None): `n` small spheres with uniform random centres in a slab in front of BIG_VIEW's camera,
    seeded numpy only.  From 16 383 spheres on the uploaded tree needs the 32-bit descriptor form (brt_layout.h DESC16_MAX_INDEX).
    The slab is wider than the view at its far end and thin enough (optical depth about 1) that a 96x54 frame shows sky, near
    spheres and far spheres.  Every sphere is an independent draw (centre, radius and material come from one row of one array), so
    big_scene(n, s).models[:k] is big_scene(k, s).models: a cropped scene is a strict subset.  Ids carry no spatial order.
    Materials: every third one metal, three refracting (specular_transmission = 1: the guides' `a` is 1), one diffuse with a
    base-colour channel below 1e-3 (the guides clamp it), the rest diffuse."""
    rng = np.random.default_rng(seed)
    mats = np.zeros(n_materials, brt.MATERIAL_DTYPE)
    for m in range(n_materials):
        colour = tuple(float(x) for x in rng.uniform(0.15, 0.95, 3))
        if m % 3 == 0:
            sm = brt.StandardMaterial(base_color=colour, metallic=1.0, perceptual_roughness=float(rng.uniform(0.0, 0.8)))
        elif m in (1, 13, 25):
            sm = brt.StandardMaterial(specular_transmission=1.0, ior=float(rng.uniform(1.2, 1.7)))
        elif m == 2:
            sm = brt.StandardMaterial(base_color=(0.6, 0.0, 0.35))
        else:
            sm = brt.StandardMaterial(base_color=colour, perceptual_roughness=float(rng.uniform(0.0, 1.0)))
        mats[m] = brt.RaytraceMaterial.prepare_asset(sm)[0]
    draw = np.random.default_rng([seed, 1]).random((n, 5))                # one row per sphere: x, y, z, radius, material
    models = np.zeros(n, brt.MODEL_DTYPE)
    lo, hi = np.array(BIG_SLAB[0]), np.array(BIG_SLAB[1])
    models["position"] = (lo + draw[:, :3] * (hi - lo)).astype(F32)
    models["radius"] = (0.07 + 0.11 * draw[:, 3]).astype(F32)
    models["material_id"] = np.minimum((draw[:, 4] * n_materials).astype(np.uint32), n_materials - 1)
    return brt.Buffers(models, mats, None)


BIG_SLAB = ((-17.0, -10.0, -44.0), (17.0, 10.0, -14.0))
BIG_VIEW = dict(pos=(0.75, 0.5, 0.0), target=(0.0, 0.0, -29.0), fov=0.5)


def big_view(w, h, spp=2, bounces=4, seed=0.5, level=brt.Raytracing.Pure, **kw):
    """The fixed camera of big_scene (the raster wall and disc of blend_post_ref.raster_inputs, at distances 9 and 6, lie in front
    of the slab)."""
    return uniforms(w, h, spp, bounces, seed=seed, level=level, **{**BIG_VIEW, **kw})


def l1_norm(v):
    v = np.abs(np.asarray(v, F32))
    return float((v[0] + v[1]) + v[2])


def resident_callee_tree(plugin, b, lvl, cam, win, w, h, seeds=()):
    """Uploads `b` without a tree, so the callee builds its SAH tree; a first query raises that tree's reach to the camera's 1-norm
    (the position-free rule asks for more than the camera's own); then one frame per seed.  -> (Buffers with the CPU twin of the
    resident tree, the last window, last_stats)."""
    none = brt.Buffers(b.models, b.materials, None)
    plugin.node.write_buffers(none)
    plugin.node.query_rays(brt.pixel_ray(cam, win, w, h, 0, 0), origin_bound=l1_norm(cam[0]["position"]))
    for seed in seeds:
        win = brt.WindowExtract.extract_component(h, seed)
        plugin.node.run(lvl, cam, win, w, h, buffers=none)
    if not seeds:
        plugin.node.run(lvl, cam, win, w, h)
    st = dict(plugin.node.last_stats)
    return brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, st["tree_reach"])), win, st


def dev(a):
    """The bytes of a host array in a device tensor of uint8."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(n_bytes, guard, fill):
    """A device buffer of n_bytes with `guard` bytes behind it, all of them `fill`.  The fill is a kernel on torch's stream and the
    context's own stream is non-blocking: the buffer is handed out once the fill has landed, so that it cannot overwrite what a call
    on the context's stream writes (seen once: a buffer of 48 bytes that came back all `fill`)."""
    import torch
    buf = torch.full((n_bytes + guard,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


@functools.lru_cache(maxsize=None)
def cover():
    return brt.generate_scene(brt.SCENE_COVER, 1)


def upload_cover(plugin, tree):
    """The cover scene under the caller's PLOC tree, or under the callee's SAH tree with its reach raised by a bake's origin_bound."""
    b = cover()
    if tree == "caller":
        plugin.node.write_buffers(b)
        return
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    one = np.zeros(1, brt.PROBE_DTYPE)
    one["position"] = (0.0, 30.0, 0.0)
    plugin.node.bake_probes(one, 1, 0, brt.PROBE_SH9, origin_bound=40.0)
    assert 40.0 <= plugin.node.query_origin_bound() < np.inf


def make_buffers(data, bvh_fn=None):
    """data = [(position, radius, StandardMaterial)] -> Buffers; bvh_fn(models) or the PLOC builder."""
    b = brt.prepare_buffers([(p, brt.RaytracedSphere(r), m) for p, r, m in data])
    if bvh_fn is not None:
        b = brt.Buffers(b.models, b.materials, bvh_fn(b.models))
    return b


def uniforms(w, h, spp, bounces, pos, target, fov, seed, level=brt.Raytracing.Pure, near=0.1, far=1000.0,
             up=(0.0, 1.0, 0.0), window_height=None):
    cam = brt.RaytracedCamera(level=level, sample_count=spp, bounces=bounces)
    proj = brt.PerspectiveProjection(fov=fov, aspect_ratio=w / h, near=near, far=far)
    lvl, cex = brt.CameraExtract.extract_component(cam, brt.Transform(pos, target, up), proj)
    return lvl, cex, brt.WindowExtract.extract_component(h if window_height is None else window_height, seed)


def _random_case(rng):
    n = int(rng.integers(1, 60))
    data = []
    for _ in range(n):
        kind = rng.random()
        mat = brt.StandardMaterial(base_color=tuple(float(x) for x in rng.random(3)),
                                   metallic=float(rng.choice([0.0, 1.0, rng.random()])),
                                   perceptual_roughness=float(rng.choice([0.0, 0.5, rng.random()])),
                                   ior=float(rng.uniform(0.5, 2.5)),
                                   specular_transmission=float(rng.choice([0.0, 1.0, rng.random()])))
        r = float(rng.uniform(0.05, 1.5)) if kind < 0.9 else float(rng.uniform(20, 200))
        pos = tuple(float(x) for x in rng.uniform(-4, 4, 3)) if kind < 0.9 else (float(rng.uniform(-3, 3)), -r - 1.0, float(rng.uniform(-3, 3)))
        data.append((pos, r, mat))
    topo = rng.integers(0, 4)
    bvh_fn = [None, single_leaf_bvh, lambda m: median_split_bvh(m, int(rng.integers(1, 5))), chain_bvh][topo]
    if bvh_fn is chain_bvh and n < 2:
        bvh_fn = single_leaf_bvh
    b = make_buffers(data, bvh_fn)
    w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    pos = tuple(float(x) for x in rng.uniform(-8, 8, 3))
    lvl, cam, win = uniforms(w, h, spp=int(rng.integers(1, 6)), bounces=int(rng.integers(0, 12)), pos=pos,
                             target=tuple(float(x) for x in rng.uniform(-1, 1, 3)), fov=float(rng.uniform(0.2, 1.5)),
                             seed=float(np.float32(rng.random())), level=brt.Raytracing(int(rng.integers(1, 4))),
                             window_height=int(rng.integers(1, 1200)))
    return b, lvl, cam, win, w, h


SPECIAL = [0.0, -0.0, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1e-38, 1e-45, 1.0, -1.0, 1e6, 1e-6]


def _special(rng):
    return float(SPECIAL[int(rng.integers(0, len(SPECIAL)))])


def _wild_material(rng, wild):
    def unit():
        if wild and rng.random() < 0.15:
            return _special(rng) if rng.random() < 0.5 else float(rng.uniform(-2, 3))
        return float(rng.choice([0.0, 1.0, rng.random()]))
    ior = float(rng.uniform(0.3, 3.0))
    if wild and rng.random() < 0.2:
        ior = _special(rng)
    return brt.StandardMaterial(base_color=tuple(float(x) for x in rng.random(3)), metallic=unit(),
                                perceptual_roughness=unit(), ior=ior, specular_transmission=unit())


def _wild_case(rng, wild=True, max_spheres=None, callee_trees=True):
    """The generator of scripts/fuzz_parity.py (which draws `wild` itself: half of its cases stay sane but structurally varied): the values
    the reference never guards against (raytrace.wgsl has no validation) -- zero / negative / huge / NaN / infinite radii and positions,
    coincident spheres (exact ties, raytrace.wgsl:353 strict `<`), materials outside [0, 1], ior 0 and inf, poisoned boxes, cameras inside
    spheres, degenerate up vectors, window height 0 (infinite jitter), NaN / huge / negative random_seed, sample_count 0, bounce counts
    past the stack size, hand-made trees deeper than the 32-entry stack, multi-sphere leaves.
    max_spheres: larger draws are folded below it (the suite's table: a case stays under a second on the oracle).
    callee_trees: topology 0 leaves the tree to the callee (buffers.bvh None); False: it is the caller's PLOC tree.
    -> dict(buffers, level, camera, window, w, h, raster, depth, wild, topo, mode, n_parts, far_cam)."""
    n = int(rng.choice([1, 2, 3, int(rng.integers(4, 40)), int(rng.integers(40, 400)), int(rng.integers(400, 3000)),
                        int(rng.integers(8200, 12000)),       # does not fit LDS: top-of-tree tile, 16-bit descriptors
                        int(rng.integers(16400, 18000))],     # > 16382 spheres: 32-bit descriptors, all from L2
                       p=[0.05, 0.05, 0.05, 0.45, 0.285, 0.1, 0.01, 0.005]))
    if max_spheres is not None and n > max_spheres:
        n = max_spheres - n % 64
    spread = float(rng.choice([0.5, 4.0, 30.0]))
    data = []
    for i in range(n):
        r = float(rng.uniform(0.05, 1.5)) if rng.random() < 0.9 else float(rng.uniform(20, 2000))
        pos = [float(x) for x in rng.uniform(-spread, spread, 3)]
        if r > 10:
            pos[1] = -r - 1.0
        data.append((tuple(pos), r, _wild_material(rng, wild)))
    if n >= 2 and rng.random() < 0.3:    # coincident spheres: exact ties in t
        for _ in range(int(rng.integers(1, 4))):
            a, b = rng.integers(0, n, 2)
            data[int(b)] = (data[int(a)][0], data[int(a)][1], data[int(b)][2])

    topo = int(rng.integers(0, 5))
    if n > 400 and topo in (1, 3):
        topo = 0                          # single leaf / chain of 1000s of spheres: too slow for the oracle
    bvh_fn = [None, single_leaf_bvh, lambda m: median_split_bvh(m, int(rng.integers(1, 9))), chain_bvh,
              lambda m: chain_bvh(m, far_first=True)][topo]
    if topo in (3, 4) and n < 2:
        bvh_fn = single_leaf_bvh
    if bvh_fn is None and not callee_trees:
        bvh_fn = brt.build_bvh
    b = brt.prepare_buffers([(p, brt.RaytracedSphere(r), m) for p, r, m in data])
    models = b.models.copy()
    if wild:
        for _ in range(int(rng.integers(0, 4))):
            i = int(rng.integers(0, n))
            if rng.random() < 0.5:
                models["radius"][i] = _special(rng)
            else:
                models["position"][i, int(rng.integers(0, 3))] = _special(rng)
    bvh = None if bvh_fn is None else bvh_fn(models)
    if bvh is not None and wild and rng.random() < 0.2:      # a poisoned box
        k = int(rng.integers(0, len(bvh)))
        bvh["bounds_min" if rng.random() < 0.5 else "bounds_max"][k, int(rng.integers(0, 3))] = _special(rng)
    b = brt.Buffers(models, b.materials, bvh)

    big = n > 400
    w, h = (int(rng.integers(1, 40)), int(rng.integers(1, 30))) if big else (int(rng.integers(1, 90)), int(rng.integers(1, 60)))
    if rng.random() < 0.1:
        h = int(rng.integers(60, 200))    # enough 8-row strips for every part of an 8-way split
    # (32+ samples: the first frame of a view runs a pre-pass, which for a scene walked from an LDS tile + L2 also re-numbers the tree's
    #  records by their use -- brt_api_order.cpp apply_hot_order)
    spp = int(rng.choice([0, 1, 2, 3, 5, 9, 33, 64], p=[0.03, 0.29, 0.24, 0.19, 0.11, 0.06, 0.05, 0.03]))
    bounces = int(rng.choice([0, 1, 3, 8, 20, 70], p=[0.1, 0.15, 0.3, 0.3, 0.1, 0.05]))
    per_ray = n if topo in (1, 3, 4) else 40          # sphere/box tests per ray, roughly
    while w * h * max(spp, 1) * (bounces + 1) * per_ray > 2e8 and w * h > 1:   # keep the oracle under about a second
        w, h = max(1, w // 2), max(1, (h * 2) // 3)
    pos = tuple(float(x) for x in rng.uniform(-8, 8, 3))
    far_cam = rng.random() < 0.35
    if far_cam:                           # a camera far outside the scene: distance log-uniform in [1, 2000] (the callee's tree must follow it:
        dist = float(np.exp(rng.uniform(0.0, np.log(2000.0))))        # brt_sah.h "leaf boxes")
        v = rng.standard_normal(3)
        pos = tuple(float(x) for x in dist * v / np.linalg.norm(v))
    if rng.random() < 0.15:               # camera inside (or on) a sphere
        i = int(rng.integers(0, n))
        pos = tuple(float(x) for x in np.nan_to_num(models["position"][i], nan=0.0, posinf=9.0, neginf=-9.0))
    target = tuple(float(x) for x in rng.uniform(-1, 1, 3))
    up = (0.0, 1.0, 0.0)
    if wild and rng.random() < 0.1:
        up = tuple(float(x) for x in rng.uniform(-1, 1, 3))
    fov = float(rng.uniform(0.2, 1.5))
    if far_cam:                           # ... looking at the scene through a field of view as narrow as 1e-3
        fov = float(np.exp(rng.uniform(np.log(1e-3), np.log(1.5))))
    if wild and rng.random() < 0.15:
        fov = float(rng.choice([1e-4, 3.1, 3.14159274, 0.0, 6.0]))
    seed = float(np.float32(rng.random()))
    if wild and rng.random() < 0.2:
        seed = float(rng.choice([0.0, 1.0, -0.5, 1e9, np.nan, np.inf, 1e-30]))
    window_height = int(rng.integers(1, 2400))
    if wild and rng.random() < 0.05:
        window_height = 0
    near, far = 0.1, 1000.0
    if wild and rng.random() < 0.1:
        near, far = float(rng.choice([0.0, 5.0, 1e4])), float(rng.choice([0.0, 1.0, 1e30]))
    lvl, cam, win = uniforms(w, h, spp=spp, bounces=bounces, pos=pos, target=target, fov=fov, seed=seed,
                             level=brt.Raytracing(int(rng.integers(0, 4))), near=near, far=far, up=up,
                             window_height=window_height)
    raster = depth = None
    if rng.random() < 0.4:
        raster = rng.random((h, w, 4), dtype=np.float32)
        depth = rng.random((h, w), dtype=np.float32) * np.float32(rng.choice([0.05, 1.0]))
        if wild and rng.random() < 0.3:
            depth[rng.random((h, w)) < 0.1] = np.float32(_special(rng))
    mode = str(rng.choice(["run", "multi", "parts", "simple"], p=[0.6, 0.15, 0.15, 0.1]))
    return dict(buffers=b, level=lvl, camera=cam, window=win, w=w, h=h, raster=raster, depth=depth, wild=wild, topo=topo,
                mode=mode, n_parts=int(rng.choice([2, 3, 5, 8])), far_cam=far_cam)


def random_scene(rng, max_spheres=6000):
    """The scene generator of scripts/sequence_soak.py and tests/sequence_cases.py: 70 .. max_spheres spheres (log-uniform) in a cube of
    half-edge `spread`, half the scenes over a ground sphere.  -> (Buffers under the caller's PLOC tree, spread)."""
    n = int(np.exp(rng.uniform(np.log(70), np.log(max_spheres))))
    spread = float(rng.choice([3.0, 12.0, 40.0]))
    data = []
    ground = rng.random() < 0.5
    for i in range(n):
        if i == 0 and ground:
            data.append(((0.0, -1000.0, 0.0), 1000.0, brt.StandardMaterial(base_color=(0.5, 0.5, 0.5))))
            continue
        r = float(rng.uniform(0.05, 0.6)) * (spread / 12.0) ** 0.5
        pos = rng.uniform(-spread, spread, 3)
        if ground:
            pos[1] = r if rng.random() < 0.7 else float(rng.uniform(r, spread / 3))
        u = rng.random()
        mat = brt.StandardMaterial(base_color=tuple(float(x) for x in rng.random(3)), metallic=1.0 if u < 0.2 else 0.0,
                                   perceptual_roughness=float(rng.random()), ior=float(rng.uniform(1.1, 2.4)),
                                   specular_transmission=1.0 if 0.2 <= u < 0.35 else 0.0)
        data.append((tuple(float(x) for x in pos), r, mat))
    b = brt.prepare_buffers([(p, brt.RaytracedSphere(r), m) for p, r, m in data])
    return b, spread


def random_view(rng, spread, w, h, spp, bounces, far=False, near_to=None):
    """A camera of random_scene's scene: a jump, with `far` x 5 .. x 300 the scene's extent (field of view narrowed to match), or with
    near_to (the description a former call returned) a small move.  -> ((level, camera, window), (pos, target, fov, seed))."""
    if near_to is not None:                # a small move: a few percent of the distance
        pos, target, fov, seed = near_to
        d = float(np.linalg.norm(np.subtract(pos, target)))
        pos = tuple(float(x) for x in np.add(pos, rng.normal(0.0, 0.01 * d, 3)))
    else:
        dist = spread * (float(np.exp(rng.uniform(np.log(5.0), np.log(300.0)))) if far else float(rng.uniform(0.3, 2.5)))
        v = rng.standard_normal(3)
        v[1] = abs(v[1]) * 0.5 + 0.05
        pos = tuple(float(x) for x in dist * v / np.linalg.norm(v))
        target = tuple(float(x) for x in rng.uniform(-0.3, 0.3, 3) * spread)
        fov = float(rng.uniform(0.3, 1.2)) if not far else float(min(1.2, rng.uniform(1.0, 3.0) * spread / dist))
        seed = float(np.float32(rng.random()))
    lvl, cam, win = uniforms(w, h, spp=spp, bounces=bounces, pos=pos, target=target, fov=fov, seed=seed,
                             level=brt.Raytracing(int(rng.choice([1, 2, 3], p=[0.15, 0.15, 0.7]))))
    return (lvl, cam, win), (pos, target, fov, seed)


def fixture_buffers():
    z = np.load(os.path.join(GOLDEN, "cover_64x36.npz"))
    b = brt.Buffers(z["models"].view(brt.MODEL_DTYPE), z["materials"].view(brt.MATERIAL_DTYPE), z["bvh"].view(brt.BVH_NODE_DTYPE))
    return (b, z["level"].view(brt.LEVEL_DTYPE), z["camera"].view(brt.CAMERA_DTYPE), z["window"].view(brt.WINDOW_DTYPE),
            z["frame"], [int(x) for x in z["counters"]])


def sky_color(oracle, cam, win, w, h, spp):
    """Expected frame when EVERY ray misses, restated in numpy f32 from raytrace.wgsl:95,
    139-156,161-170,198-201,223,364-369 (RNG draws taken from the pinned oracle RNG)."""
    c = cam[0]
    seed = F32(win[0]["random_seed"])
    height = F32(win[0]["height"])
    aspect = F32(c["aspect"])
    width = height * aspect
    cd, cu = c["direction"].astype(F32), c["up"].astype(F32)
    right = np.array([cd[1] * cu[2] - cd[2] * cu[1], cd[2] * cu[0] - cd[0] * cu[2], cd[0] * cu[1] - cd[1] * cu[0]], F32)
    scale = F32(oracle.lib.oracle_tan_half_fov(float(c["fov"])))
    out = np.zeros((h, w, 3), F32)
    for py in range(h):
        for px in range(w):
            uvx = (F32(px) + F32(0.5)) / F32(w)
            uvy = (F32(py) + F32(0.5)) / F32(h)
            state = oracle.lib.oracle_seed(float(seed), px, py, w, h)
            total = np.zeros(3, F32)
            for _ in range(spp):
                r, state = oracle.rng_floats(state, 2)
                rx, ry = r[0] - F32(0.5), r[1] - F32(0.5)
                du, dv = (F32(1.0) / width) * rx, (F32(1.0) / height) * ry
                ndc_x = (uvx * F32(2.0) - F32(1.0)) + du
                ndc_y = (F32(1.0) - uvy * F32(2.0)) + dv
                d = (cd + (ndc_x * aspect * scale) * right) + (ndc_y * scale) * cu
                d = d.astype(F32)
                ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=F32)
                rd = (d / ln).astype(F32)                     # ray direction, raytrace.wgsl:153
                ln2 = np.sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2], dtype=F32)
                u = (rd / ln2).astype(F32)                   # background_gradient normalises again, :365
                a = F32(0.5) * (u[1] + F32(1.0))
                col = (F32(1.0) - a) * np.ones(3, F32) + a * np.array([0.5, 0.7, 1.0], F32)
                total = (total + np.sqrt(col.astype(F32), dtype=F32)).astype(F32)
            out[py, px] = total / F32(spp)
    return out


def tiny_frame_cases():
    """Frames rendered by the independent numpy restatement (tests/golden/numpy_restatement.py)."""
    z = np.load(os.path.join(GOLDEN, "tiny_frames.npz"))
    names = sorted({k.split(".")[0] for k in z.files})
    for name in names:
        g = lambda k: z[f"{name}.{k}"]
        b = brt.Buffers(g("models").view(brt.MODEL_DTYPE), g("materials").view(brt.MATERIAL_DTYPE), g("bvh").view(brt.BVH_NODE_DTYPE))
        w, h = (int(x) for x in g("size"))
        raster = g("raster") if f"{name}.raster" in z.files else None
        depth = g("depth") if f"{name}.depth" in z.files else None
        yield (name, b, g("level").view(brt.LEVEL_DTYPE), g("camera").view(brt.CAMERA_DTYPE), g("window").view(brt.WINDOW_DTYPE),
               w, h, raster, depth, g("frame"), int(g("rays")[0]))
