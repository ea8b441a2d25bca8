"""Reference side of tests/test_query.py: the expected result of a ray query from the CPU oracle's `oracle_raycast` (one call per ray),
a numpy f32 restatement of the pixel-centre ray (camera_ray_dir_center and the camera terms of the frame parameters), and the ray sets."""
import ctypes as C

import numpy as np

import bevyray_amd as brt

F32 = np.float32
NO_HIT = F32(3.40282347e+38)      # const.wgsl:2: the reference's INF
INF = F32(np.inf)


def pixel_ray_np(oracle, cam, win, w, h, px, py):
    """(origin (3,), direction (3,)) f32 of the pixel-centre ray of pixel (px, py), in the kernel's order of operations."""
    c = cam[0]
    aspect = F32(c["aspect"])
    heightf = F32(win[0]["height"])
    widthf = heightf * aspect
    with np.errstate(all="ignore"):
        inv_w, inv_h = F32(1.0) / widthf, F32(1.0) / heightf
    cd, cu = c["direction"].astype(F32), c["up"].astype(F32)
    right = np.array([cd[1] * cu[2] - cd[2] * cu[1], cd[2] * cu[0] - cd[0] * cu[2], cd[0] * cu[1] - cd[1] * cu[0]], F32)
    scale = F32(oracle.lib.oracle_tan_half_fov(float(c["fov"])))
    uvx = (F32(px) + F32(0.5)) / F32(w)
    uvy = (F32(py) + F32(0.5)) / F32(h)
    ndc_x = (uvx * F32(2.0) - F32(1.0)) + inv_w * F32(0.0)
    ndc_y = (F32(1.0) - uvy * F32(2.0)) + inv_h * F32(0.0)
    sx = (ndc_x * aspect) * scale
    sy = ndc_y * scale
    d = ((cd + sx * right) + sy * cu).astype(F32)
    ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=F32)
    return c["position"].astype(F32), (d / ln).astype(F32)


def make_rays(origins, directions, t_max=np.inf, user=None):
    origins = np.asarray(origins, F32).reshape(-1, 3)
    directions = np.asarray(directions, F32).reshape(-1, 3)
    n = max(len(origins), len(directions))
    rays = np.zeros(n, brt.RAY_DTYPE)
    rays["origin"] = origins
    rays["direction"] = directions
    rays["t_max"] = t_max
    rays["user"] = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) if user is None else user
    return rays


def pixel_rays(oracle, cam, w, h):
    """The pixel-centre rays of a w x h frame in raster order (tests/denoise_ref.py pixel_center_rays: the same arithmetic, vectorised)."""
    import denoise_ref as dr
    o, dirs, _ = dr.pixel_center_rays(oracle, cam, w, h)
    return make_rays(np.broadcast_to(o, (w * h, 3)), dirs.reshape(-1, 3))


def expected(oracle, models, bvh, rays, mode=brt.QUERY_CLOSEST):
    """HIT_DTYPE records of valid, in-reach rays by the oracle (sphere left at QUERY_NONE: see check_spheres), and the unbounded t."""
    models = np.ascontiguousarray(models)
    bvh = np.ascontiguousarray(bvh)
    out = np.zeros(len(rays), brt.HIT_DTYPE)
    t_unbounded = np.zeros(len(rays), F32)
    o3, d3, r7 = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 7)()
    mid, front = C.c_uint32(0), C.c_int(0)
    for i, r in enumerate(rays):
        o3[0], o3[1], o3[2] = (float(v) for v in r["origin"])
        d3[0], d3[1], d3[2] = (float(v) for v in r["direction"])
        oracle.lib.oracle_raycast(models.ctypes.data, len(models), bvh.ctypes.data, len(bvh), o3, d3, r7, C.byref(mid), C.byref(front))
        t = F32(r7[0])
        t_unbounded[i] = INF if t == NO_HIT else t
        hit = t != NO_HIT and t < r["t_max"]
        out[i]["user"] = r["user"]
        out[i]["sphere"] = brt.QUERY_NONE
        if not hit or mode == brt.QUERY_ANY:          # the miss form (the oracle's own miss is its INF constant with material 0)
            out[i]["t"] = INF
            out[i]["material"] = brt.QUERY_NONE
            out[i]["status"] = brt.QUERY_STATUS_HIT if hit else brt.QUERY_STATUS_MISS
            continue
        out[i]["t"] = t
        out[i]["normal"] = (r7[4], r7[5], r7[6])
        out[i]["material"] = mid.value
        out[i]["status"] = brt.QUERY_STATUS_HIT | (brt.QUERY_STATUS_FRONT_FACE if front.value else 0)
    return out, t_unbounded


def assert_hits_equal(got, want, what=""):
    """Bitwise, every field but `sphere`."""
    assert got.shape == want.shape
    for f in ("t", "normal", "material", "status", "user"):
        g = got[f].view(np.uint32).reshape(len(got), -1)
        w = want[f].view(np.uint32).reshape(len(want), -1)
        bad = (g != w).any(axis=1)
        assert not bad.any(), f"{what}: field {f}: {bad.sum()} of {len(got)} rays differ, first {np.flatnonzero(bad)[:4].tolist()}: got {got[bad][:2]}, want {want[bad][:2]}"


def check_spheres(oracle, models, rays, hits):
    """`sphere` of every CLOSEST hit is a caller's index whose sphere reproduces t through oracle_hit_sphere and carries that material;
    QUERY_NONE everywhere else."""
    is_hit = (hits["status"] & brt.QUERY_STATUS_HIT) != 0
    full = is_hit & (hits["material"] != brt.QUERY_NONE)
    assert (hits["sphere"][~full] == brt.QUERY_NONE).all()
    assert (hits["sphere"][full] < len(models)).all()
    o3, d3, c3 = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    for i in np.flatnonzero(full):
        m = models[hits["sphere"][i]]
        assert m["material_id"] == hits["material"][i], i
        o3[0], o3[1], o3[2] = (float(v) for v in rays["origin"][i])
        d3[0], d3[1], d3[2] = (float(v) for v in rays["direction"][i])
        c3[0], c3[1], c3[2] = (float(v) for v in m["position"])
        t = F32(oracle.lib.oracle_hit_sphere(o3, d3, c3, float(m["radius"])))
        assert t.view(np.uint32) == hits["t"][i].view(np.uint32), (i, t, hits["t"][i])


def ray_sets(oracle, models, bvh, cam, w, h, rng, n=1500):
    """name -> rays: the issue's sets, `n` rays each (the oracle is called per ray)."""
    px = pixel_rays(oracle, cam, w, h)
    pick = rng.choice(len(px), size=min(n, len(px)), replace=False)
    sets = {"pixel_centre": px[np.sort(pick)], "shuffled": px[pick]}
    # from hit points into random directions: origins on a surface
    base, _ = expected(oracle, models, bvh, sets["pixel_centre"])
    on = (base["status"] & brt.QUERY_STATUS_HIT) != 0
    src = sets["pixel_centre"][on]
    pos = (src["origin"] + base["t"][on][:, None] * src["direction"]).astype(F32)
    dirs = rng.normal(size=(len(pos), 3)).astype(F32)
    sets["bounce"] = make_rays(pos, dirs)
    # origins inside spheres (the centre plus less than the radius)
    k = rng.integers(0, len(models), size=n // 3)
    off = (rng.uniform(-0.5, 0.5, size=(len(k), 3)) * models["radius"][k][:, None]).astype(F32)
    sets["inside"] = make_rays(models["position"][k] + off, rng.normal(size=(len(k), 3)).astype(F32))
    # axis-parallel directions (zero components) from around the scene
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, 1]], F32)
    o = (models["position"][rng.integers(0, len(models), size=n // 3)] + rng.uniform(-3, 3, size=(n // 3, 3))).astype(F32)
    sets["axis_parallel"] = make_rays(o, axes[rng.integers(0, len(axes), size=len(o))])
    # origins on slab planes: a coordinate of the origin equal to a box plane of the tree, some directions inside that plane
    nodes = bvh[rng.integers(0, len(bvh), size=n // 3)]
    o = (0.5 * (nodes["bounds_min"] + nodes["bounds_max"])).astype(F32)
    ax = rng.integers(0, 3, size=len(o))
    side = rng.integers(0, 2, size=len(o))
    o[np.arange(len(o)), ax] = np.where((side == 0)[:, None], nodes["bounds_min"], nodes["bounds_max"])[np.arange(len(o)), ax]
    d = rng.normal(size=(len(o), 3)).astype(F32)
    flat = rng.integers(0, 2, size=len(o)) == 0
    d[np.flatnonzero(flat), ax[flat]] = 0.0
    finite = np.isfinite(o).all(axis=1)
    sets["slab_planes"] = make_rays(o[finite], d[finite])
    # unnormalised and tiny directions, and d = 0
    s = sets["shuffled"][: n // 3].copy()
    scale = (10.0 ** rng.uniform(-30, 6, size=len(s))).astype(F32)
    s["direction"] = (s["direction"] * scale[:, None]).astype(F32)
    sets["scaled_directions"] = s
    z = sets["shuffled"][:64].copy()
    z["direction"] = 0.0
    sets["zero_direction"] = z
    return sets


def bounded(want, t_max, mode=brt.QUERY_CLOSEST):
    """The expected records of the same rays under `t_max` (scalar or per ray) and `mode`, from their unbounded CLOSEST records."""
    out = want.copy()
    t_max = np.broadcast_to(np.asarray(t_max, F32), want.shape)
    hit = ((want["status"] & brt.QUERY_STATUS_HIT) != 0) & (want["t"] < t_max)
    blank = ~hit if mode == brt.QUERY_CLOSEST else np.ones(len(want), bool)
    out["t"][blank] = INF
    out["normal"][blank] = 0
    out["material"][blank] = brt.QUERY_NONE
    out["sphere"][blank] = brt.QUERY_NONE
    out["status"][blank] = np.where(hit[blank], brt.QUERY_STATUS_HIT, brt.QUERY_STATUS_MISS)
    return out
