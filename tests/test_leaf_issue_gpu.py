"""The leaf step, the outer head and the sampler's bookkeeping of the hand-written loops after their pass in the instruction currency
(BRT_LEAF_ISSUE, brt_device.h: BRT_LEAF_TAIL without its upper range guards, the accept rule by two v_cmpx, the leaf lanes from the head's
masks, ball_loop_asm's masks): small frames bit for bit against the C oracle with equal ray counts, the rays and scenes at and one float
beyond the bounds that replace the guards (through the streaming closest-hit query, which walks in walk_wave_lds_asm /
walk_wave_top_asm), the accept rule at its two strict compares, and the bound itself evaluated on the CPU."""
import numpy as np
import pytest

import bevyray_amd as brt
import query_ref as qr
from helpers import make_buffers, uniforms

F32 = np.float32
STREAM = 2                    # value of the knob BRT_QUERY_FORM: the streaming form (walk_run's wave-level loops)
LANES = (5, 63, 0, 31)        # where the edge ray sits in the four waves of a 256-ray batch

# the bounds of brt_layout.h (kLeafOriginMax, kLeafCentreMax, kLeafR2Max, kLeafAHi, and kLeafALo of brt_device.h)
B_O, B_C, B_R, A_HI, A_LO = 2.0 ** 24, 2.0 ** 24, 2.0 ** 50, 2.0 ** 8, 2.0 ** -29


def up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


# ---- 4. the bound itself (CPU) ----------------------------------------------------------------------------------------------------------

def test_bounds_keep_the_discriminant_and_n_inside_the_short_forms_ranges():
    """The derivation above BRT_LEAF_TAIL as arithmetic, in f64 at the corner of the admitted box: every f32 operation of the leaf step is
    taken at its largest magnitude times (1 + u), u = 2^-23 (one rounding, generously: round-to-nearest is within 2^-24), and nothing
    cancels.  |disc| must stay below 2^80 and |n| below 2^40, the ranges in which sqrt_rsq and div_plain are the compiler's forms."""
    u = 2.0 ** -23
    r = 1.0 + u
    oc = (B_C + B_O) * r                                   # |centre_i - o_i|
    occ = 3.0 * (oc * oc * r) * r * r                      # dot(oc, oc): three squares, two sums
    c = (occ + B_R) * r                                    # |dot(oc, oc) - r^2|
    # a = fl(fl(dx^2 + dy^2) + dz^2) <= A_HI with every term non-negative: each dx^2 <= a (1 + u)^3 exactly
    d = np.sqrt(A_HI * r ** 3)
    h = 3.0 * (d * oc * r) * r * r                         # |dot(d, oc)|: three products, two sums
    hh = h * h * r
    ac = A_HI * c * r
    disc = (hh + ac) * r
    n = (h + np.sqrt(disc) * r) * r
    assert oc <= 2.0 ** 25 * r and occ < 2.0 ** 52 and c < 2.0 ** 53 and h < 2.0 ** 31, (oc, occ, c, h)
    assert disc < 2.0 ** 63 < 2.0 ** 80, disc
    assert n < 2.0 ** 33 < 2.0 ** 40, n
    # ... and the divide's lower end: with a >= 2^-29 a lane with |n| < 2^-40 is rejected by t > 0.001 in either form (brt_device.h)
    assert 2.0 ** -40 / A_LO * (1.0 + 2.0 ** -21) < 0.001


# ---- everything below needs the GPU -----------------------------------------------------------------------------------------------------

def _mat(k=0):
    return (brt.StandardMaterial(base_color=(0.7, 0.6, 0.5)),
            brt.StandardMaterial(base_color=(0.8, 0.8, 0.9), metallic=1.0, perceptual_roughness=0.4),
            brt.StandardMaterial(specular_transmission=1.0, ior=1.5))[k % 3]


def _assert_frame(got, want, what):
    got = np.asarray(got, F32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"


# ---- 1. small frames --------------------------------------------------------------------------------------------------------------------

def _three(kind):
    """Three spheres of one material kind on a large diffuse or metal ground-less stage: every hit lane is in the sampler, with two balls
    per lane (diffuse) or one (rough metal)."""
    m = (brt.StandardMaterial(base_color=(0.7, 0.6, 0.5)) if kind == "diffuse"
         else brt.StandardMaterial(base_color=(0.8, 0.8, 0.9), metallic=1.0, perceptual_roughness=0.6))
    b = make_buffers([((1.1 * k - 1.1, 0.0, -4.0 - 0.3 * k), 0.5, m) for k in range(3)])
    return (b, *uniforms(32, 16, spp=8, bounces=8, pos=(0.0, 0.2, 0.0), target=(0.0, 0.0, -4.0), fov=0.6, seed=0.37), 32, 16, {})


FRAMES = {
    "cover_32x16": lambda: (brt.generate_scene(brt.SCENE_COVER, 1), *brt.cover_camera(32, 16, 4, 8), 32, 16, {}),
    "grid_lds_top": lambda: (brt.generate_scene(brt.SCENE_STRESS_GRID, 1), *brt.cover_camera(32, 16, 4, 8), 32, 16, {"BRT_FORCE_LDS_TOP": 64}),
    "all_diffuse": lambda: _three("diffuse"),
    "all_rough_metal": lambda: _three("metal"),
}


@pytest.fixture(scope="module", params=list(FRAMES))
def frame_case(request, oracle):
    b, lvl, cam, win, w, h, knobs = FRAMES[request.param]()
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    return request.param, b, lvl, cam, win, w, h, knobs, np.asarray(want, F32), cnt["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("live", [False, True], ids=["production", "knobs_live"])
def test_small_frames_match_the_oracle(plugin, frame_case, live):
    """production: no flags (LEAN 1 at this size: the hand-written loops and sampler); knobs_live: BRT_TUNABLE."""
    name, b, lvl, cam, win, w, h, knobs, want, rays = frame_case
    with plugin.tuning(**knobs, **({"BRT_TUNABLE": 1} if live else {})):
        got = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=0)
        st = dict(plugin.node.last_stats)
        assert (st["kernel_variant"] & 16) if live else st["kernel_variant"] == 1, st["kernel_variant"]
        if "BRT_FORCE_LDS_TOP" in knobs:
            assert st["scene_in_lds"] == 2
        assert st["rays"] == rays, (name, st["rays"], rays)
        _assert_frame(got, want, f"{name} variant {st['kernel_variant']}")


@pytest.mark.gpu
def test_steady_state_instantiation_matches_the_oracle(plugin, oracle):
    """LEAN 2 is chosen by the frame's size, not by a knob: it needs more than twice a pixel's longest chain of rays per lane of the GPU,
    which no 32 x 16 frame has.  The smallest view that runs in it is the one tests/test_interior_step_gpu.py uses -- the cover scene at
    1920 x 1080, one sample -- here with two bounces (at most 3 rays per pixel); its third frame runs in LEAN 2."""
    w, h = 1920, 1080
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(w, h, 1, 2)
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    want = np.asarray(want, F32)
    for frame in range(3):
        got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
        st = dict(plugin.node.last_stats)
        assert st["rays"] == cnt["rays"], (frame, st["rays"], cnt["rays"])
    assert st["kernel_variant"] == 2, st["kernel_variant"]
    _assert_frame(got, want, "third frame, LEAN 2")


# ---- 2. precondition edges --------------------------------------------------------------------------------------------------------------

def _leaf_terms(o, d, centre, radius):
    """(a, disc, n, r2) of hit_sphere (raytrace.wgsl:371-383) in the kernel's order of f32 operations; n = h - sqrt(disc) (NaN: disc < 0)."""
    o, d, c = (np.asarray(v, F32) for v in (o, d, centre))
    oc = c - o
    h = (d[0] * oc[0] + d[1] * oc[1]) + d[2] * oc[2]
    r2 = F32(radius) * F32(radius)
    cc = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - r2
    a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    with np.errstate(all="ignore"):
        disc = h * h - a * cc
        n = h - np.sqrt(disc, dtype=F32)
    return float(a), float(disc), float(n), float(r2)


def _inside(o, d, spheres):
    """What walk_run and the upload decide: (the ray is inside its bounds, the scene is inside its bounds)."""
    o = np.asarray(o, F32)
    a = _leaf_terms(o, d, (0, 0, 0), 1.0)[0]
    ray = bool((np.abs(o) <= F32(B_O)).all()) and A_LO <= a <= A_HI
    scene = all(bool((np.abs(np.asarray(c, F32)) <= F32(B_C)).all()) and float(F32(r) * F32(r)) <= B_R for c, r in spheres)
    return ray, scene


S3 = 1.0 / np.sqrt(3.0)
NEAR = [((0.0, 0.0, 5.0), 1.0), ((2.0, 0.0, 6.0), 1.0)]      # two ordinary spheres in front of the ordinary rays
R25 = 2.0 ** 25                                              # radius whose square is B_R exactly

# name -> (spheres [(centre, radius)], the edge ray (o, d, index of the sphere it is aimed at), claim(ray inside, scene inside, a, r2, hit))
# The claim is asserted on the f32 terms before anything runs.  `r2`: r^2 is the square of the radius a caller passes, so the next r^2
# above the bound that a scene can have is the square of the next radius above 2^25 (two floats above 2^50).
EDGES = {
    "origin_at_bound": ([((16777000.0, 0.0, 0.0), 50.0)] + NEAR[:1], ((B_O, 0, 0), (-1, 0, 0), 0),
                        lambda ray, scene, o, a, r2: ray and scene and o[0] == B_O),
    "origin_above_bound": ([((16777000.0, 0.0, 0.0), 50.0)] + NEAR[:1], ((up(B_O), 0, 0), (-1, 0, 0), 0),
                           lambda ray, scene, o, a, r2: not ray and scene and o[0] == up(B_O)),
    "a_at_bound": (NEAR, ((0, 0, 0), (0, 0, 16.0), 0), lambda ray, scene, o, a, r2: ray and scene and a == A_HI),
    "a_above_bound": (NEAR, ((0, 0, 0), (0, 0.005, 16.0), 0), lambda ray, scene, o, a, r2: not ray and scene and a == up(A_HI)),
    "centre_at_bound": ([((B_C, 0.0, 0.0), 50.0)] + NEAR[:1], ((B_C - 200.0, 0, 0), (1, 0, 0), 0),
                        lambda ray, scene, o, a, r2: ray and scene),
    "centre_above_bound": ([((up(B_C), 0.0, 0.0), 50.0)] + NEAR[:1], ((B_C - 200.0, 0, 0), (1, 0, 0), 0),
                           lambda ray, scene, o, a, r2: ray and not scene),
    "r2_at_bound": ([((-B_C, -B_C, -B_C), R25)] + NEAR, ((B_O, B_O, B_O), (-S3, -S3, -S3), 0),
                    lambda ray, scene, o, a, r2: ray and scene and r2 == B_R),
    "r2_above_bound": ([((-B_C, -B_C, -B_C), up(R25))] + NEAR, ((B_O, B_O, B_O), (-S3, -S3, -S3), 0),
                       lambda ray, scene, o, a, r2: ray and not scene and B_R < r2 <= up(up(B_R))),
    "lone_sphere_at_both_bounds": ([((B_C, -B_C, B_C), R25)], ((-B_O, B_O, -B_O), (S3, -S3, S3), 0),
                                   lambda ray, scene, o, a, r2: ray and scene and r2 == B_R),
}


def _ordinary_rays(spheres, rng, n=256):
    """Rays from around the origin towards points in and around the scene's spheres: most hit, some graze, some miss."""
    o = rng.uniform(-1, 1, size=(n, 3)).astype(F32)
    k = rng.integers(0, len(spheres), size=n)
    centres = np.array([s[0] for s in spheres], np.float64)[k]
    radii = np.array([s[1] for s in spheres], np.float64)[k]
    d = centres + rng.uniform(-1.3, 1.3, size=(n, 3)) * radii[:, None] - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return qr.make_rays(o, d.astype(F32))


@pytest.fixture(scope="module", params=list(EDGES))
def edge_case(request, oracle):
    """(name, buffers, ordinary rays and their expected records, the edge ray and its expected record): once per case, shared by the tree modes."""
    spheres, (o, d, k), claim = EDGES[request.param]
    a, disc, n, r2 = _leaf_terms(o, d, *spheres[k])
    ray, scene = _inside(o, d, spheres)
    assert claim(ray, scene, [float(F32(v)) for v in o], a, r2), (request.param, ray, scene, a, disc, n, r2)
    assert 0.0 < disc < 2.0 ** 63 and 0.0 < n < 2.0 ** 33, (request.param, disc, n)      # a hit, inside what the derivation promises
    b = make_buffers([(c, r, _mat(i)) for i, (c, r) in enumerate(spheres)])
    ordinary = _ordinary_rays(spheres, np.random.default_rng(23))
    want, _ = qr.expected(oracle, b.models, b.bvh, ordinary)
    edge = qr.make_rays([o], [d], user=np.array([0xE06E], np.uint32))
    want_edge, _ = qr.expected(oracle, b.models, b.bvh, edge)
    assert want_edge["status"][0] & brt.QUERY_STATUS_HIT, request.param
    return request.param, b, ordinary, want, edge, want_edge


def _query_among_and_alone(plugin, oracle, b, ordinary, want_ordinary, edges, want_edges, places, what):
    rays, want = ordinary.copy(), want_ordinary.copy()
    for e, at in enumerate(places):
        rays[at] = edges[e % len(edges)]
        want[at] = want_edges[e % len(edges)]
    got = plugin.node.query_rays(rays)
    assert plugin.node.last_query_stats["form"] == STREAM - 1
    qr.assert_hits_equal(got, want, f"{what} among ordinary rays")
    qr.check_spheres(oracle, b.models, rays, got)
    alone = plugin.node.query_rays(edges)
    qr.assert_hits_equal(alone, want_edges, f"{what} alone")
    qr.check_spheres(oracle, b.models, edges, alone)
    return got, alone


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"BRT_FORCE_LDS_TOP": 1}], ids=["lds", "lds_top"])
def test_rays_and_scenes_at_the_bounds_match_the_oracle(plugin, oracle, edge_case, knobs):
    """Each edge ray once per wave of a 256-ray batch among 63 ordinary rays, and alone: at a bound it walks in the hand-written loop,
    one float beyond it (the ray, or the whole scene) in the compiler's; t, normal, material and status equal the oracle's either way."""
    name, b, ordinary, want_ordinary, edge, want_edge = edge_case
    lvl, cam, win = uniforms(8, 8, spp=1, bounces=1, pos=(0, 0, 0), target=(0, 0, 1), fov=0.5, seed=0.5)
    plugin.node.run(lvl, cam, win, 8, 8, buffers=b)                  # makes the scene resident
    assert plugin.node.query_origin_bound() >= 3.0 * up(B_O)
    with plugin.tuning(BRT_QUERY_FORM=STREAM, **knobs):
        _query_among_and_alone(plugin, oracle, b, ordinary, want_ordinary, edge, want_edge, [64 * w + lane for w, lane in enumerate(LANES)],
                               f"{name} {knobs}")


# ---- 3. the accept rule -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"BRT_FORCE_LDS_TOP": 1}], ids=["lds", "lds_top"])
def test_coincident_spheres_the_first_one_reached_wins(plugin, oracle, knobs):
    """Two spheres of the same centre and radius in different leaves give the same t: t < closest is strict, so the one the walk reaches
    first keeps the hit.  Their materials differ, so the oracle's material names its sphere."""
    spheres = [((0.0, 0.0, 5.0), 1.0), ((0.0, 0.0, 5.0), 1.0), ((3.0, 0.0, 6.0), 1.0)]
    b = make_buffers([(c, r, _mat(i)) for i, (c, r) in enumerate(spheres)])
    ids = b.models["material_id"]
    assert len(set(int(v) for v in ids)) == 3
    rays = _ordinary_rays(spheres, np.random.default_rng(5))
    want, _ = qr.expected(oracle, b.models, b.bvh, rays)
    lvl, cam, win = uniforms(8, 8, spp=1, bounces=1, pos=(0, 0, 0), target=(0, 0, 1), fov=0.5, seed=0.5)
    plugin.node.run(lvl, cam, win, 8, 8, buffers=b)
    with plugin.tuning(BRT_QUERY_FORM=STREAM, **knobs):
        got = plugin.node.query_rays(rays)
    qr.assert_hits_equal(got, want, f"coincident {knobs}")
    hit = (want["status"] & brt.QUERY_STATUS_HIT) != 0
    twins = hit & np.isin(want["material"], ids[:2])
    assert twins.sum() > 64, int(twins.sum())
    assert (ids[got["sphere"][hit]] == want["material"][hit]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"BRT_FORCE_LDS_TOP": 1}], ids=["lds", "lds_top"])
def test_accept_threshold_sweep_matches_the_oracle(plugin, oracle, knobs):
    """Origins at (1 + k ulp) * 0.001 from a sphere's surface along its normal, k = -8 .. 8, looking at it: t lands within a few ulp of
    0.001 on both sides of the strict t > 0.001.  The sphere is small (radius 2^-10, its surface through the origin) so that an ulp of
    the origin is an ulp of t; a rejected ray goes on to the sphere behind.  Both outcomes must occur, and each equals the oracle's."""
    R = 2.0 ** -10
    spheres = [((0.0, 0.0, R), R), ((0.0, 0.0, 5.0), 1.0)]
    b = make_buffers([(c, r, _mat(i)) for i, (c, r) in enumerate(spheres)])
    eps = F32(0.001)
    s = (eps.view(np.uint32) + np.arange(-8, 9)).astype(np.uint32).view(F32)
    o = np.zeros((17, 3), F32)
    o[:, 2] = -s
    sweep = qr.make_rays(o, np.tile(np.array([0, 0, 1], F32), (17, 1)), user=np.arange(17, dtype=np.uint32) + np.uint32(0xACC0))
    want_sweep, _ = qr.expected(oracle, b.models, b.bvh, sweep)
    near = want_sweep["t"] < F32(0.01)
    assert near.any() and (~near).any(), want_sweep["t"]           # accepted by the small sphere resp. rejected and caught by the far one
    assert ((want_sweep["status"] & brt.QUERY_STATUS_HIT) != 0).all()
    ordinary = _ordinary_rays(spheres[1:], np.random.default_rng(9))
    want, _ = qr.expected(oracle, b.models, b.bvh, ordinary)
    lvl, cam, win = uniforms(8, 8, spp=1, bounces=1, pos=(0, 0, 0), target=(0, 0, 1), fov=0.5, seed=0.5)
    plugin.node.run(lvl, cam, win, 8, 8, buffers=b)
    with plugin.tuning(BRT_QUERY_FORM=STREAM, **knobs):
        _query_among_and_alone(plugin, oracle, b, ordinary, want, sweep, want_sweep, [(15 * j) % 256 for j in range(17)], f"sweep {knobs}")
