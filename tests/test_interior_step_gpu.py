"""The interior step of the hand-written walk loops (BRT_WIDE_INT_STEP, brt_device.h: walk_wave_lds_asm, walk_wave_top_asm) on the shipped
build: small frames at which a slip in the push / pop rule, the stack pointer or a record address shows, as `uint32` and with their
ray counts against the C oracle, in the production instantiations (LEAN 1, LEAN 2) and in the knobs-live one.  The oracle frame of a
case is computed once and shared by the instantiations."""
import numpy as np
import pytest

import bevyray_amd as brt
from helpers import chain_bvh, make_buffers, uniforms

pytestmark = pytest.mark.gpu


def _mat(k):
    return (brt.StandardMaterial(base_color=(0.7, 0.6, 0.5)),
            brt.StandardMaterial(base_color=(0.8, 0.8, 0.9), metallic=1.0, perceptual_roughness=0.1),
            brt.StandardMaterial(specular_transmission=1.0, ior=1.5))[k % 3]


def _few(n):
    """n spheres side by side: the root is a leaf (1), one record (2), two records (3)."""
    b = make_buffers([((1.1 * k - 0.55 * (n - 1), 0.0, -4.0 - 0.3 * k), 0.5, _mat(k)) for k in range(n)])
    return (b, *uniforms(16, 8, spp=2, bounces=4, pos=(0.0, 0.2, 0.0), target=(0.0, 0.0, -4.0), fov=0.6, seed=0.37), 16, 8, {})


def _deep_chain(knobs):
    """30 collinear spheres under a caterpillar tree of depth 29 -- the deepest the simple-tree rule takes (max leaf depth + 1 < 31) --
    seen along their line: the interior child is walked first, so a central ray stacks one leaf per level before it pops any."""
    n = 30
    b = make_buffers([((0.0, 0.0, -3.0 - 1.2 * k), 0.5, _mat(k)) for k in range(n)], chain_bvh)
    return (b, *uniforms(16, 8, spp=2, bounces=8, pos=(0.0, 0.05, 2.0), target=(0.0, 0.0, -20.0), fov=0.3, seed=0.61), 16, 8, knobs)


def _cover(w, h, spp=4, bounces=4):
    return (brt.generate_scene(brt.SCENE_COVER, 1), *brt.cover_camera(w, h, spp, bounces), w, h, {})


def _cover_along(pos, target, up=(0.0, 1.0, 0.0)):
    """The cover scene seen along one axis: the camera rays read one sign granule of every record, the bounces the others."""
    return (brt.generate_scene(brt.SCENE_COVER, 1),
            *uniforms(24, 12, spp=2, bounces=4, pos=pos, target=target, fov=0.5, seed=0.83, up=up), 24, 12, {})


def _grid_lds_top():
    """The 10 004-sphere grid with a top-of-tree tile of 64 records: steps whose lanes are all in the tile (the common step of
    walk_wave_top_asm), all in the global array, and mixed (its out-of-line step)."""
    return (brt.generate_scene(brt.SCENE_STRESS_GRID, 1), *brt.cover_camera(32, 16, 4, 4), 32, 16, {"BRT_FORCE_LDS_TOP": 64})


CASES = {
    "one_sphere": lambda: _few(1),
    "two_spheres": lambda: _few(2),
    "three_spheres": lambda: _few(3),
    "deep_chain": lambda: _deep_chain({}),
    "deep_chain_lds_top": lambda: _deep_chain({"BRT_FORCE_LDS_TOP": 3}),
    "cover_1x1": lambda: _cover(1, 1),
    "cover_13x9": lambda: _cover(13, 9),
    "cover_64x32": lambda: _cover(64, 32),
    "grid_lds_top": _grid_lds_top,
    "along_minus_x": lambda: _cover_along((13.0, 1.0, 0.0), (0.0, 1.0, 0.0)),
    "along_minus_y": lambda: _cover_along((0.0, 15.0, 0.0), (0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0)),
    "along_minus_z": lambda: _cover_along((0.0, 1.0, 13.0), (0.0, 1.0, 0.0)),
    "along_plus_xyz": lambda: _cover_along((-10.0, 0.5, -10.0), (0.0, 3.0, 0.0)),
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, oracle):
    b, lvl, cam, win, w, h, knobs = CASES[request.param]()
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    return request.param, b, lvl, cam, win, w, h, knobs, np.asarray(want, np.float32), cnt["rays"]


def _assert_frame(got, want, what):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("live", [False, True], ids=["production", "knobs_live"])
def test_small_frames_match_the_oracle(plugin, case, live):
    """production: no flags, two frames of the view (LEAN instantiation: kernel_variant 1 or 2, the hand-written loops);
    knobs_live: BRT_TUNABLE (kernel_variant bit 4)."""
    name, b, lvl, cam, win, w, h, knobs, want, rays = case
    with plugin.tuning(**knobs, **({"BRT_TUNABLE": 1} if live else {})):
        for frame in range(1 if live else 2):
            got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
            st = dict(plugin.node.last_stats)
            assert (st["kernel_variant"] & 16) if live else st["kernel_variant"] in (1, 2), st["kernel_variant"]
            if "BRT_FORCE_LDS_TOP" in knobs:
                assert st["scene_in_lds"] == 2
            assert st["rays"] == rays, (name, frame, st["rays"], rays)
            _assert_frame(got, want, f"{name} frame {frame} variant {st['kernel_variant']}")


def test_steady_state_instantiation_matches_the_oracle(plugin, oracle):
    """LEAN = 2 needs a frame with more than twice a pixel's longest chain of rays per lane of the GPU: the cover scene at 1920 x 1080,
    one sample, one bounce (at most 2 rays per pixel, at least 2.07 M in the frame, 7 per lane of 256 CUs); the third frame of the view
    runs in it."""
    w, h = 1920, 1080
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(w, h, 1, 1)
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    want = np.asarray(want, np.float32)
    for frame in range(3):
        got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
        st = dict(plugin.node.last_stats)
        assert st["rays"] == cnt["rays"], (frame, st["rays"], cnt["rays"])
        _assert_frame(got, want, f"frame {frame} variant {st['kernel_variant']}")
    assert st["kernel_variant"] == 2, st["kernel_variant"]
