"""Reference side of tests/test_radiance.py: the expected result of a radiance query from the numpy restatement of the shader
(tests/golden/numpy_restatement.py, written from the WGSL): Rng(seed), `samples` calls of Shader.raytrace(o, d, rng) at level 3 with
camera.bounce_count = bounces, summed in f32 and divided by f32(samples); the first-hit fields from Shader.raycast.  It also counts what
the paths met, so that a test can say its ray set reaches every class of segment."""
import os
import sys

import numpy as np

import bevyray_amd as brt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import numpy_restatement as npr  # noqa: E402

F32 = np.float32
NO_HIT = npr.INF                  # const.wgsl:2: the reference's INF
INF = F32(np.inf)
COUNT_KEYS = ("raycasts", "metal", "glass", "diffuse", "absorbed", "bounce_limit", "miss_entries", "hit_entries")


def make_rays(origins, directions, seeds, user=None):
    origins = np.asarray(origins, F32).reshape(-1, 3)
    directions = np.asarray(directions, F32).reshape(-1, 3)
    n = max(len(origins), len(directions))
    rays = np.zeros(n, brt.RADIANCE_RAY_DTYPE)
    rays["origin"] = origins
    rays["direction"] = directions
    rays["seed"] = seeds
    rays["user"] = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) if user is None else user
    return rays


def standard_rays(camera_position, n=96, seed=3, box=6.0):
    """The standard set: even entries start at the camera and aim at uniform random targets in [-box, box] x [0, 1.2] x [-box, box];
    odd entries start at uniform random origins in [-8, 8] x [0.3, 3] x [-8, 8] with normal-distributed directions.  Seeds, targets,
    origins and directions from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    targets = rng.uniform((-box, 0.0, -box), (box, 1.2, box), size=(n, 3)).astype(F32)
    origins = rng.uniform((-8.0, 0.3, -8.0), (8.0, 3.0, 8.0), size=(n, 3)).astype(F32)
    dirs = rng.normal(size=(n, 3)).astype(F32)
    cam = np.asarray(camera_position, F32)
    even = (np.arange(n) % 2) == 0
    o = np.where(even[:, None], cam[None, :], origins).astype(F32)
    d = np.where(even[:, None], (targets - cam[None, :]).astype(F32), dirs).astype(F32)
    return make_rays(o, d, seeds)


class _Counting(npr.Shader):
    """Shader whose scatter says which branch a segment took (from the draws the branch itself makes: random.wgsl, raytrace.wgsl:231-299)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.counts = dict.fromkeys(COUNT_KEYS, 0)
        self.sample_scatters = 0

    def scatter(self, d, hit, rng):
        mat = self.materials[hit["material"]]
        probe = npr.Rng(rng.state)
        if probe.next_float() < F32(mat["metallic"]):
            kind = "metal"
        elif probe.next_float() < F32(mat["specular_transmission"]):
            kind = "glass"
        else:
            kind = "diffuse"
        self.counts[kind] += 1
        out = super().scatter(d, hit, rng)
        if out[0]:
            self.counts["absorbed"] += 1
        else:
            self.sample_scatters += 1
        return out


def shader(models, materials, bvh, camera, bounces):
    cam = np.array(camera[0] if getattr(camera, "shape", ()) else camera).copy()
    cam["bounce_count"] = bounces
    return _Counting(models, materials, bvh, cam, None, 3)


def expected(models, materials, bvh, camera, rays, samples, bounces):
    """-> (RADIANCE_DTYPE records of valid, in-reach entries -- sphere left at QUERY_NONE: see check_spheres --, counts).  counts:
    COUNT_KEYS; "raycasts" are those of the paths alone (`samples` per entry for the entry's own ray included)."""
    sh = shader(models, materials, bvh, camera, bounces)
    out = np.zeros(len(rays), brt.RADIANCE_DTYPE)
    for i, r in enumerate(rays):
        o, d = r["origin"].astype(F32), r["direction"].astype(F32)
        first = sh.raycast(o, d)
        out[i]["user"] = r["user"]
        out[i]["sphere"] = brt.QUERY_NONE
        if first["distance"] == NO_HIT:
            out[i]["t"] = INF
            out[i]["material"] = brt.QUERY_NONE
            out[i]["status"] = brt.QUERY_STATUS_MISS
            sh.counts["miss_entries"] += 1
        else:
            out[i]["t"] = first["distance"]
            out[i]["material"] = first["material"]
            out[i]["status"] = brt.QUERY_STATUS_HIT | (brt.QUERY_STATUS_FRONT_FACE if first["front_face"] else 0)
            sh.counts["hit_entries"] += 1
        sh.rays = 0
        rng = npr.Rng(int(r["seed"]))
        total = npr.v3(0, 0, 0)
        for _ in range(samples):
            sh.sample_scatters = 0
            color, _ = sh.raytrace(o, d, rng)
            if sh.sample_scatters == bounces + 1:
                sh.counts["bounce_limit"] += 1
            total = (total + color).astype(F32)
        out[i]["rgb"] = (total / F32(samples)).astype(F32)
        sh.counts["raycasts"] += sh.rays
    return out, dict(sh.counts)


def sky_rgb(directions):
    """The colour of a miss ray in closed form: sqrt of the sky gradient of the normalised direction (raytrace.wgsl:198-201, :223,
    :364-369), every operation a separately rounded f32 operation, vectorised.  `samples` equal colours summed and divided give the
    colour itself only for samples = 1 in general; callers use one sample."""
    d = np.asarray(directions, F32).reshape(-1, 3)
    ln = np.sqrt(((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32) + (d[:, 2] * d[:, 2]).astype(F32), dtype=F32)
    uy = (d[:, 1] / ln).astype(F32)
    a = (F32(0.5) * (uy + F32(1.0)).astype(F32)).astype(F32)
    b = (F32(1.0) - a).astype(F32)
    top = np.array([0.5, 0.7, 1.0], F32)
    col = ((b[:, None] * np.ones(3, F32)[None, :]).astype(F32) + (a[:, None] * top[None, :]).astype(F32)).astype(F32)
    return np.sqrt(col, dtype=F32)


def assert_equal(got, want, what=""):
    """Bitwise, every field but `sphere`."""
    assert got.shape == want.shape
    for f in ("t", "rgb", "material", "status", "user"):
        g = got[f].view(np.uint32).reshape(len(got), -1)
        w = want[f].view(np.uint32).reshape(len(want), -1)
        bad = (g != w).any(axis=1)
        assert not bad.any(), f"{what}: field {f}: {bad.sum()} of {len(got)} entries differ, first {np.flatnonzero(bad)[:4].tolist()}: got {got[bad][:2]}, want {want[bad][:2]}"


def check_spheres(models, rays, got):
    """`sphere` of every hit is a caller's index whose sphere reproduces t through the restatement's hit_sphere and carries that material;
    QUERY_NONE everywhere else."""
    sh = npr.Shader(models, None, None, dict(fov=F32(1.0)), None, 3)
    is_hit = (got["status"] & brt.QUERY_STATUS_HIT) != 0
    assert (got["sphere"][~is_hit] == brt.QUERY_NONE).all()
    assert (got["sphere"][is_hit] < len(models)).all()
    for i in np.flatnonzero(is_hit):
        m = models[got["sphere"][i]]
        assert m["material_id"] == got["material"][i], i
        t = sh.hit_sphere(m, rays["origin"][i].astype(F32), rays["direction"][i].astype(F32))
        assert F32(t).view(np.uint32) == got["t"][i].view(np.uint32), (i, t, got["t"][i])
