"""The short correctly rounded forms of the leaf step and the shading (sqrt_rsq, BRT_LEAF_TAIL, brt_device.h): sqrt_rsq -- Newton on v_rsq_f32 --
on every float of its range, the guarded tail of the hand-written leaf step on the rays at and beyond the edges of its guards (through
the streaming ray query, which walks in walk_wave_lds_asm / walk_wave_top_asm), and small frames, all bit for bit against the compiler's
forms resp. the CPU oracle."""
import numpy as np
import pytest

import bevyray_amd as brt
import query_ref as qr
from helpers import make_buffers, uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
DBG_SQRT_SWEEP = 8
STREAM = 2                    # value of the knob BRT_QUERY_FORM: the streaming form (walk_run's wave-level loops)
LANES = (5, 63, 0, 31)        # where the edge ray sits in the four waves of a 256-ray batch


def test_rsq_sqrt_is_the_compilers_sqrt_on_every_float_of_its_range(plugin):
    """sqrt_rsq against __builtin_sqrtf on EVERY float in [2^-80, 2^80] (1.34e9 values), bit for bit.  v_rsq_f32 is specified to
    1 ulp only: what the form returns depends on the hardware's actual outputs, and this sweep is what settles it."""
    lo = int(F32(2.0 ** -80).view(np.uint32))
    hi = int(F32(2.0 ** 80).view(np.uint32))
    per = 65536
    n = (hi - lo) // per + 2
    inp = np.zeros((n, 16), F32)
    inp[:, 0] = np.full(n, lo - 3, np.uint32).view(F32)            # element i covers [lo - 3 + i * per, +per)
    inp[:, 1] = float(per)
    inp[:, 2] = 1.0                                                 # the rsq form (strictly positive arguments, no +-0)
    out = plugin.debug_eval(DBG_SQRT_SWEEP, inp)
    assert out[:, 0].sum() == 0, f"{int(out[:, 0].sum())} mismatches, first argument bits {out[out[:, 0] > 0][:1, 1].view(np.uint32)}"


# ---- the leaf step's edges ------------------------------------------------------------------------------------------------------------

def _leaf_terms(o, d, centre, radius):
    """(a, disc, n) of hit_sphere (raytrace.wgsl:371-383) in the kernel's order of f32 operations; n = h - sqrt(disc) (NaN: disc < 0)."""
    o, d, c = (np.asarray(v, F32) for v in (o, d, centre))
    oc = c - o
    h = (d[0] * oc[0] + d[1] * oc[1]) + d[2] * oc[2]
    cc = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - F32(radius) * F32(radius)
    a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    with np.errstate(all="ignore"):
        disc = h * h - a * cc
        n = h - np.sqrt(disc, dtype=F32)
    return F32(a), F32(disc), F32(n)


def _mat():
    return brt.StandardMaterial(base_color=(0.7, 0.6, 0.5))


P2 = lambda e: float(2.0 ** e)  # noqa: E731

# scene name -> (spheres [(centre, radius)], length scale of the ordinary rays, edge rays [(name, o, d, sphere index, regime)])
# regime(a, disc, n) states what makes the ray an edge of the guarded tail; it is asserted on the f32 terms before anything runs.
PLAIN_A = lambda a: 2.0 ** -29 <= a <= 2.0 ** 40  # noqa: E731
SCENES = {
    "unit": ([((1.0, 0.0, 5.0), 1.0)], 1.0, [
        ("tangent", (0, 0, 0), (0, 0, 1), 0, lambda a, disc, n: disc == 0 and PLAIN_A(a)),
        ("tangent_d_2^-25", (0, 0, 0), (0, 0, P2(-25)), 0, lambda a, disc, n: a == 2.0 ** -50),
        ("tangent_d_2^25", (0, 0, 0), (0, 0, P2(25)), 0, lambda a, disc, n: a == 2.0 ** 50),
        ("centre_d_2^-25", (0, 0, 0), (0.2 * P2(-25), 0, P2(-25)), 0, lambda a, disc, n: a < 2.0 ** -49 and disc > 0),
        ("centre_d_2^25", (0, 0, 0), (0.2 * P2(25), 0, P2(25)), 0, lambda a, disc, n: a > 2.0 ** 49 and disc > 0),
        ("miss_negative_discriminant", (0, 0, 0), (0, 1, 0), 0, lambda a, disc, n: disc < 0 and np.isnan(n)),
        ("miss_without_nan", (0, 0, 0), (-0.2, 0, -1), 0, lambda a, disc, n: disc > 0 and n < 0),
    ]),
    "on_surface": ([((0.0, 0.0, 1.0), 1.0), ((3.0, 0.0, 5.0), 1.0)], 1.0, [
        ("inward_from_the_surface", (0, 0, 0), (0, 0, 1), 0, lambda a, disc, n: n == 0 and PLAIN_A(a) and disc == 1),
    ]),
    "tiny_n": ([((0.0, 0.0, P2(-30)), P2(-30)), ((P2(-28), 0.0, P2(-28)), P2(-30))], P2(-29), [
        ("n_tiny_positive", (0, 0, -P2(-52)), (0, 0, 1), 0, lambda a, disc, n: 0 < n < 2.0 ** -40 and 2.0 ** -80 <= disc <= 2.0 ** 80 and a == 1),
    ]),
    "tiny_discriminant": ([((P2(-21), 0.0, 5 * P2(-21)), P2(-21))], P2(-21), [
        ("discriminant_below_2^-80", (0, 0, 0), (P2(-28), 0, P2(-14)), 0, lambda a, disc, n: 0 < disc < 2.0 ** -80 and PLAIN_A(a)),
    ]),
    "huge": ([((0.0, 0.0, 1e13), 1e12), ((0.0, 0.0, -1e13), 4e12), ((0.0, 2.0, 0.0), 0.5)], 1.0, [
        ("radius_1e12_at_1e13", (0, 0, 0), (0, 0, 1), 0, lambda a, disc, n: disc > 2.0 ** 79 and n > 2.0 ** 40 and a == 1),
        ("discriminant_above_2^80", (0, 0, 0), (0, 0, -1), 1, lambda a, disc, n: disc > 2.0 ** 80 and a == 1),
    ]),
}


def _ordinary_rays(spheres, scale, rng, n=256):
    """Rays from around the origin towards points in and around the scene's spheres: most hit, some graze, some miss."""
    o = (rng.uniform(-1, 1, size=(n, 3)) * scale).astype(F32)
    k = rng.integers(0, len(spheres), size=n)
    centres = np.array([s[0] for s in spheres], np.float64)[k]
    radii = np.array([s[1] for s in spheres], np.float64)[k]
    target = centres + rng.uniform(-1.3, 1.3, size=(n, 3)) * radii[:, None]
    d = target - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return qr.make_rays(o, d.astype(F32))


@pytest.fixture(scope="module", params=list(SCENES))
def edge_scene(request, plugin, oracle):
    """(name, buffers, ordinary rays, their expected records): computed once per scene and shared by the tree modes."""
    spheres, scale, edges = SCENES[request.param]
    for name, o, d, k, regime in edges:
        a, disc, n = _leaf_terms(o, d, *spheres[k])
        assert regime(float(a), float(disc), float(n)), (request.param, name, a, disc, n)
    b = make_buffers([(c, r, _mat()) for c, r in spheres])
    ordinary = _ordinary_rays(spheres, scale, np.random.default_rng(11))
    want, _ = qr.expected(oracle, b.models, b.bvh, ordinary)
    return request.param, b, ordinary, want


@pytest.mark.parametrize("knobs", [{}, {"BRT_FORCE_LDS_TOP": 1}], ids=["lds", "lds_top"])
def test_leaf_step_edge_rays_match_the_oracle(plugin, oracle, edge_scene, knobs):
    """Every edge ray of the scene through the hand-written walk (streaming closest-hit query; scene in LDS: walk_wave_lds_asm, forced
    top-of-tree tile: walk_wave_top_asm): once per wave of a 256-ray batch among 63 ordinary rays, so that the out-of-line full forms
    run with other lanes live, and alone in a wave.  t, normal, material and status equal the oracle's bit for bit; the sphere's index
    reproduces t."""
    name, b, ordinary, want_ordinary = edge_scene
    lvl, cam, win = uniforms(8, 8, spp=1, bounces=1, pos=(0, 0, 0), target=(0, 0, 1), fov=0.5, seed=0.5)
    plugin.node.run(lvl, cam, win, 8, 8, buffers=b)                  # makes the scene resident
    assert plugin.node.query_origin_bound() >= 4.0
    with plugin.tuning(BRT_QUERY_FORM=STREAM, **knobs):
        for ename, o, d, _, _ in SCENES[name][2]:
            edge = qr.make_rays([o], [d], user=np.array([0xE06E], np.uint32))
            want_edge, _ = qr.expected(oracle, b.models, b.bvh, edge)
            rays, want = ordinary.copy(), want_ordinary.copy()
            for w, lane in enumerate(LANES):
                rays[64 * w + lane] = edge[0]
                want[64 * w + lane] = want_edge[0]
            got = plugin.node.query_rays(rays)
            assert plugin.node.last_query_stats["form"] == STREAM - 1
            qr.assert_hits_equal(got, want, f"{name}/{ename} among ordinary rays {knobs}")
            qr.check_spheres(oracle, b.models, rays, got)
            alone = plugin.node.query_rays(edge)
            qr.assert_hits_equal(alone, want_edge, f"{name}/{ename} alone {knobs}")
            qr.check_spheres(oracle, b.models, edge, alone)


# ---- small frames ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,bounces", [(brt.SCENE_COVER, 8), (brt.SCENE_RTIOW_FINAL, 50)], ids=["cover", "rtiow_glass"])
def test_small_frames_match_the_oracle(plugin, oracle, kind, bounces):
    """64 x 40, 8 samples per pixel in the production instantiation (no counters): pixels and ray count equal the oracle's."""
    w, h = 64, 40
    b = brt.generate_scene(kind, 1)
    lvl, cam, win = (brt.rtiow_camera if kind == brt.SCENE_RTIOW_FINAL else brt.cover_camera)(w, h, 8, bounces)
    got = np.asarray(plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=0), F32)
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    want = np.asarray(want, F32)
    assert plugin.node.last_stats["rays"] == cnt["rays"]
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"
