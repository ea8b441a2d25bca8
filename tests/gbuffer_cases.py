"""The cases of tests/test_gbuffer.py: the random and special-valued inputs of the host twin, and the GPU cases -- scenes, cameras,
previous cameras, moved spheres, coverage frames -- each of which the CPU tests first hold to the oracle alone (non-vacuity)."""
import functools

import numpy as np

import bevyray_amd as brt
from helpers import big_scene, big_view, uniforms

F32 = np.float32
SPECIAL = [np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1e-42, -1e-45, -0.0, 0.0]
SIZES = [(1, 1), (1, 7), (7, 1), (17, 9), (33, 31), (96, 54)]


def _camera(rng, special):
    cam = np.zeros(1, brt.CAMERA_DTYPE)
    d = rng.normal(size=3)
    cam["sample_count"], cam["bounce_count"] = 1, 1
    cam["near"], cam["far"] = rng.choice([0.1, 0.5, 1e-3]), rng.choice([1000.0, 50.0, 10.0])
    cam["fov"], cam["aspect"] = rng.uniform(0.1, 2.0), rng.uniform(0.3, 3.0)
    cam["position"] = rng.uniform(-20, 20, 3)
    cam["direction"] = d / np.linalg.norm(d) * (1.0 if rng.random() < 0.8 else rng.uniform(0.2, 5.0))
    cam["up"] = rng.normal(size=3)                       # any up
    if special:
        f = str(rng.choice(["near", "far", "fov", "aspect", "position", "direction", "up"]))
        v = F32(SPECIAL[int(rng.integers(0, len(SPECIAL)))])
        if cam[f].ndim == 2:
            cam[f][0, int(rng.integers(0, 3))] = v
        else:
            cam[f] = v
    return cam


def twin_cases(n=3000, seed=29):
    """n x (cam, prev_cam or None, win, W, H, px, py, depth_mode, motion_format, t, sn, so or None, finite): positions in [-20, 20]^3, any
    up, fov 0.1 .. 2, aspect 0.3 .. 3, hits in front of the camera on spheres of radius 0.05 .. 3 -- unmoved, moved, resized -- misses, an
    identical / a nearby / an unrelated previous camera; every fourth case carries a special value (NaN, +-INF, 3e38, denormals, -0.0) in
    one field of a camera, of a sphere, or in t.  finite: no special value in it (the float64 compare takes those)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        special = i % 4 == 3
        where = int(rng.integers(0, 4)) if special else -1
        cam = _camera(rng, where == 0)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            prev = None
        elif kind == 1:
            prev = cam.copy()
        elif kind == 2:                                  # a small move and turn: most pixels stay in the previous frame
            prev = cam.copy()
            prev["position"] += rng.normal(0, 0.2, 3).astype(F32)
            prev["direction"] += rng.normal(0, 0.03, 3).astype(F32)
            if rng.random() < 0.3:
                prev["fov"] *= F32(rng.uniform(0.9, 1.1))
        else:
            prev = _camera(rng, where == 1)
        win = np.zeros(1, brt.WINDOW_DTYPE)
        win["random_seed"], win["height"] = 0.5, int(rng.integers(1, 2000))
        W, H = (int(x) for x in rng.choice([1, 7, 17, 96, 640, 1920, 32768], 2))
        px, py = int(rng.integers(0, W)), int(rng.integers(0, H))
        miss = rng.random() < 0.15
        t = F32(np.inf) if miss else F32(np.exp(rng.uniform(np.log(0.05), np.log(200.0))))
        r = F32(rng.uniform(0.05, 3.0))
        # a sphere through the hit point, more or less: the rule does not ask that it is
        with np.errstate(all="ignore"):
            c = cam["position"][0] + rng.normal(size=3).astype(F32) * r + F32(t if not miss else 1.0) * cam["direction"][0]
        sn = np.array([c[0], c[1], c[2], r * r], F32)
        mk = int(rng.integers(0, 4))
        so = None
        if mk == 1:
            so = sn.copy()
        elif mk == 2:
            so = sn.copy()
            so[:3] += rng.normal(0, 0.3, 3).astype(F32)
        elif mk == 3:
            so = sn.copy()
            so[3] = F32(rng.uniform(0.05, 3.0)) ** 2
        if where == 2:
            (sn if so is None or rng.random() < 0.5 else so)[int(rng.integers(0, 4))] = F32(SPECIAL[int(rng.integers(0, len(SPECIAL)))])
        if where == 3:
            t = F32(SPECIAL[int(rng.integers(0, len(SPECIAL)))])
        out.append((cam, prev, win, W, H, px, py, int(rng.integers(0, 3)), int(rng.integers(0, 3)), t, sn, so, not special))
    return out


# ---- GPU cases ----------------------------------------------------------------------------------------------------------------------

def orbit(cam, angle, lift=0.0):
    """`cam` turned by `angle` about the y axis through the origin, still looking at the origin (the cover and RTIOW views do)."""
    from bevyray_amd import CameraExtract, PerspectiveProjection, RaytracedCamera, Transform
    c = cam[0]
    p = c["position"].astype(np.float64)
    ca, sa = np.cos(angle), np.sin(angle)
    q = (ca * p[0] + sa * p[2], p[1] + lift, -sa * p[0] + ca * p[2])
    rc = RaytracedCamera(level=brt.Raytracing.Pure, sample_count=int(c["sample_count"]), bounces=int(c["bounce_count"]))
    proj = PerspectiveProjection(fov=float(c["fov"]), aspect_ratio=float(c["aspect"]), near=float(c["near"]), far=float(c["far"]))
    return CameraExtract.extract_component(rc, Transform(tuple(float(x) for x in q), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), proj)[1]


def turned(cam, w, h, yaw):
    """`cam` at its place, its target swung by `yaw` radians about the y axis through the camera: pixels leave the frame on one side."""
    from bevyray_amd import CameraExtract, PerspectiveProjection, RaytracedCamera, Transform
    c = cam[0]
    p = c["position"].astype(np.float64)
    d = c["direction"].astype(np.float64)
    ca, sa = np.cos(yaw), np.sin(yaw)
    d2 = np.array([ca * d[0] + sa * d[2], d[1], -sa * d[0] + ca * d[2]])
    rc = RaytracedCamera(level=brt.Raytracing.Pure, sample_count=int(c["sample_count"]), bounces=int(c["bounce_count"]))
    proj = PerspectiveProjection(fov=float(c["fov"]), aspect_ratio=float(c["aspect"]), near=float(c["near"]), far=float(c["far"]))
    return CameraExtract.extract_component(rc, Transform(tuple(p), tuple(p + 10.0 * d2), (0.0, 1.0, 0.0)), proj)[1]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "cover":
        return brt.generate_scene(brt.SCENE_COVER, 1)
    if name == "rtiow":
        return brt.generate_scene(brt.SCENE_RTIOW_FINAL, 1)
    if name == "stress":
        return brt.generate_scene(brt.SCENE_STRESS_GRID, 1)
    if name == "mirrored":                               # the cover scene, its small spheres mirrored in x: another frame in every plane
        c = brt.generate_scene(brt.SCENE_COVER, 1)
        m = c.models.copy()
        m["position"][m["radius"] < 10.0, 0] *= F32(-1.0)
        m["position"][m["radius"] < 10.0, 2] += F32(0.37)
        return brt.Buffers(m, c.materials, brt.build_bvh(m))
    if name == "big":
        b = big_scene(16383, 5)                          # (32-bit tree descriptors: brt_layout.h DESC16_MAX_INDEX)
        return brt.Buffers(b.models, b.materials, brt.build_bvh(b.models))
    raise ValueError(name)


def view(name, w, h):
    """(level, camera, window) of a scene's test view at w x h."""
    if name == "rtiow":
        return brt.rtiow_camera(w, h, 2, 4)
    if name == "big":
        return big_view(w, h)
    if name == "inside":                                 # the camera inside the cover scene's glass sphere at (0, 1, 0), radius 1
        return uniforms(w, h, 1, 2, pos=(0.2, 1.1, 0.1), target=(4.0, 1.0, 0.0), fov=1.2, seed=0.5)
    if name == "graze":
        # A back-face hit.  The reference's hit_sphere returns the NEAR root alone (raytrace.wgsl:373-384), so a camera inside a sphere
        # does not hit it at all, and the near root faces the ray -- except where a ray grazes and dot(d, n) rounds to >= 0.  This view of
        # the cover scene at 33 x 31, found by search on the oracle, has one such pixel on the ground sphere's horizon.
        return uniforms(w, h, 1, 2, pos=(-0.654, 0.447, 1.804), target=(3.895, 0.2915, 3.88), fov=0.69, seed=0.5)
    return brt.cover_camera(w, h, 64 if name == "stress" else 2, 4)


def moved_models(models, centre_of_view):
    """The previous frame of a re-upload: three spheres near the view's centre moved, one resized.  -> (previous models, indices)."""
    prev = models.copy()
    small = np.flatnonzero(models["radius"] < 10.0)
    d = np.linalg.norm(models["position"][small] - np.asarray(centre_of_view, F32), axis=1)
    pick = small[np.argsort(d)[:4]]
    for k, i in enumerate(pick[:3]):
        prev["position"][i] += np.array([(0.15, 0.0, -0.1), (-0.1, 0.05, 0.1), (0.0, 0.1, 0.2)][k], F32)
    prev["radius"][pick[3]] *= F32(0.8)
    return prev, pick


def coverage_frame(w, h, kind):
    """An RGBA32F coverage frame: alpha exactly +0.0 is covered.  "blocks": a pattern that covers whole waves (4 rows of a 16-wide tile
    column), parts of waves and single pixels on both sides of wave boundaries; "all": every pixel covered."""
    cov = np.ones((h, w, 4), F32)
    if kind == "all":
        cov[..., 3] = 0.0
        return cov
    yy, xx = np.mgrid[0:h, 0:w]
    wave = (yy // 4 + xx // 16) % 3 == 0                 # whole waves
    part = ((yy % 4 == 1) & (xx % 5 == 0)) | ((yy % 8 == 3) & (xx % 16 >= 12))
    cov[..., 3] = np.where(wave | part, F32(0.0), F32(1.0))
    cov[0, 0, 3] = -0.0                                  # (-0.0 is NOT covered: the test is of the bits)
    return cov
