"""Temporal accumulation (BRT_FLAG_TEMPORAL) on the GPU against the restatement (tests/temporal_ref.py) on the paths the orbit and the
moving-sphere tests do not take: the hot order's renumbered spheres (rmap) through recounts, reused and dropped numberings; zoom, roll,
dolly, a turn in place and a far camera whose tree is rebuilt; history limits around kTemporalConverged; odd shapes; accumulated frames
in every store format; a new material count; frames on two caller streams.  State: n and the rejections exact, x', y' within 1e-4 px
(_compare_state); frames within 1e-4 max(1, |ref|)."""
import numpy as np
import pytest

import bevyray_amd as brt
import temporal_ref as tr
from helpers import uniforms
from test_temporal import _compare_state, _device_frame, _orbit, _rel, _seed

F32 = np.float32
COVER_POS = (13.0, 2.0, 3.0)


class Seq:
    """Runs temporal frames on a context and the restatement side by side: each step renders the plain frame (the restatement's input),
    the temporal frame, reads the guides and the history state, and compares."""

    def __init__(self, p, oracle, models, w, h, spp, denoise_on, max_history=32):
        self.p, self.oracle, self.w, self.h, self.spp, self.denoise_on = p, oracle, w, h, spp, denoise_on
        self.flags = brt.FLAG_TEMPORAL | (brt.FLAG_DENOISE if denoise_on else 0)
        self.hist = tr.History(max_history)
        self.models = models
        self.ties = 0
        p.set_temporal(max_history)

    def step(self, lvl, cam, win, buffers=None):
        p, w, h = self.p, self.w, self.h
        if buffers is not None:
            self.models = buffers.models
        plain = p.node.run(lvl, cam, win, w, h, buffers=buffers).copy()
        self.plain_stats = dict(p.node.last_stats)
        got = p.node.run(lvl, cam, win, w, h, flags=self.flags).copy()
        self.stats = dict(p.node.last_stats)
        g = p.debug_denoise_guides(cam, win, w, h)
        c = tr.Camera(self.oracle, cam, w, h)
        sid, ties = tr.sphere_ids(g, c, self.models)
        self.ties += int(ties.sum())
        want = tr.frame_step(self.hist, plain, g, sid, c, tr.spheres_of(self.models), self.spp, self.denoise_on)
        st = p.debug_temporal_state(w, h)
        _compare_state(st, tr.state(self.hist), ~ties)
        assert _rel(got, want) <= 1e-4
        self.plain, self.g, self.state = plain, g, st
        return got


@pytest.fixture
def fresh(plugin):
    plugin.set_temporal()
    plugin.set_denoise()
    plugin.node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    yield plugin
    plugin.set_temporal()


def _hit(g):
    return g[..., 3] < np.inf


# ---- the hot order (the renumbered resident spheres) --------------------------------------------------------------------------------

def _hot_sequence(oracle, hot):
    """The stress grid at 64 spp through the five phases; returns the temporal frames and states, and asserts hot_records per phase
    (hot = False: the same sequence with BRT_HOT_RECORDS = 0, where nothing is renumbered)."""
    b = brt.generate_scene(brt.SCENE_STRESS_GRID, 1)
    w, h, spp = 160, 90, 64
    out = []
    A = brt.cover_camera(w, h, spp, 4, brt.Raytracing.Pure, _seed(0))
    B = uniforms(w, h, spp, 4, (11.0, 5.0, -6.0), (0.0, 0.0, 0.0), 0.4, _seed(1))

    def view(base, i):
        lvl, cam, win = base
        return lvl, cam, brt.WindowExtract.extract_component(h, _seed(i))

    def more(expect):
        assert (s.stats["hot_records"] > 1000) == expect, (len(out), s.stats)

    with brt.RaytracePlugin([0]) as p:
        if not hot:
            p.set_tuning("BRT_HOT_RECORDS", 0)
        s = Seq(p, oracle, b.models, w, h, spp, True)
        # 1. still frames: counted on the first (the pre-pass), the spheres renumbered
        for i in range(3):
            out.append((s.step(*view(A, i), buffers=brt.Buffers(b.models, b.materials, None) if i == 0 else None), s.state))
            more(hot)
        assert s.stats["scene_in_lds"] == 2
        # 2. a camera jump: hot_stale, counted and renumbered again (the pre-pass runs); the history does not survive the jump
        for i in range(3, 5):
            out.append((s.step(*view(B, i)), s.state))
            more(hot)
            if i == 3 and hot:
                assert s.plain_stats["prepass_ms"] > 0.0
        reach = s.stats["tree_reach"]
        # 3. an animated upload: a few spheres move by less than the tree's pads, the caller's tree keeps its shape -- the numbering is
        # reused at once (no pre-pass) and the motion term reads the spheres through rmap
        moving = b.models.copy()
        hit_ids = np.flatnonzero(np.isin(b.models["material_id"], s.g[..., 7].view(np.uint32)[_hit(s.g)]))   # (one sphere per material)
        for k in hit_ids[:: max(1, len(hit_ids) // 40)]:
            moving["position"][k] += np.array([0.01, 0.0, -0.008], F32)
        same_shape = brt.Buffers(moving, b.materials, brt.build_bvh_sah(b.models, reach))
        out.append((s.step(*view(B, 5), buffers=same_shape), s.state))
        assert (s.plain_stats["hot_records"] > 1000) == hot and s.plain_stats["prepass_ms"] == 0.0
        kept = s.state[..., 3] >= 2
        assert kept.sum() > 0.5 * _hit(s.g).sum()                     # (the moved spheres keep their history through the map)
        out.append((s.step(*view(B, 6)), s.state))
        # 4. an upload in which spheres translate and one changes radius: the callee's tree changes shape and the numbering is not
        # reused -- the frame after it runs in the encoder's numbering (rmap drops out) or in one counted afresh by a pre-pass
        moved = moving.copy()
        for k in hit_ids[1:: max(1, len(hit_ids) // 10)]:
            moved["position"][k] += np.array([0.0, 3.0, 0.0], F32)          # (out of the grid's layer: other leaves)
        moved["radius"][hit_ids[0]] *= F32(1.25)
        out.append((s.step(*view(B, 7), buffers=brt.Buffers(moved, b.materials, None)), s.state))
        assert s.plain_stats["hot_records"] == 0 or s.plain_stats["prepass_ms"] > 0.0, s.plain_stats
        # 5. still frames until the order is counted again (the scene's second still frame)
        for i in range(8, 10):
            out.append((s.step(*view(B, i)), s.state))
        more(hot)
        assert s.ties == 0
    return out


@pytest.mark.gpu
def test_hot_order_phases(oracle):
    hot = _hot_sequence(oracle, True)
    cold = _hot_sequence(oracle, False)
    for i, ((fh, sh), (fc, sc)) in enumerate(zip(hot, cold)):
        assert np.array_equal(fh.view(np.uint32), fc.view(np.uint32)), i
        assert np.array_equal(sh.view(np.uint32), sc.view(np.uint32)), i


# ---- camera paths ---------------------------------------------------------------------------------------------------------------------

def _path(kind, w, h, i):
    a = np.radians(i)
    if kind == "zoom":
        return uniforms(w, h, 4, 8, COVER_POS, (0.0, 0.0, 0.0), 0.4 - 0.012 * i, _seed(i))
    if kind == "roll":
        return uniforms(w, h, 4, 8, COVER_POS, (0.0, 0.0, 0.0), 0.4, _seed(i), up=(float(np.sin(a)), float(np.cos(a)), 0.0))
    if kind == "dolly":
        k = 1.0 - 0.02 * i
        return uniforms(w, h, 4, 8, (13.0 * k, 2.0 * k, 3.0 * k), (0.0, 0.0, 0.0), 0.4, _seed(i))
    if kind == "turn":                       # the cover view, then the view straight back from the same point
        target = (0.0, 0.0, 0.0) if i % 2 == 0 else (26.0, 4.0, 6.0)
        return uniforms(w, h, 4, 8, COVER_POS, target, 0.4, _seed(i))
    k = (4.0, 8.0, 8.0)[i]                   # far: the cover view from 4x and 8x (the callee's tree is rebuilt for its reach; from 20x on every pad is 0.1)
    return uniforms(w, h, 4, 8, (13.0 * k, 2.0 * k, 3.0 * k), (0.0, 0.0, 0.0), 0.4 / k, _seed(i), far=1.0e5)


@pytest.mark.gpu
@pytest.mark.parametrize("denoise_on", [False, True], ids=["temporal", "temporal_denoise"])
@pytest.mark.parametrize("kind", ["zoom", "roll", "dolly", "turn", "far"])
def test_camera_paths(fresh, oracle, kind, denoise_on):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 200, 120
    if kind == "far":
        p.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    s = Seq(p, oracle, b.models, w, h, 4, denoise_on)
    p.reset_temporal()
    for i in range(3):
        lvl, cam, win = _path(kind, w, h, i)
        got = s.step(lvl, cam, win)
        n = s.state[..., 3][_hit(s.g)]
        if kind == "turn" and i > 0:
            # every point of the turned view lies behind the previous camera (z <= 0): n = 1 everywhere, a first frame bit for bit
            assert (n == 1).all() and np.isnan(s.state[..., 6]).all()
            first = p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE if denoise_on else 0)
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
        elif kind == "far" and i == 1:
            assert s.plain_stats["tree_rebuilt"] == 1
            assert (n == 2).mean() > 0.5
        elif i > 0:
            assert (n == i + 1).mean() > 0.5, (kind, i, float((n == i + 1).mean()))
    assert s.ties <= 0.001 * w * h * 3


@pytest.mark.gpu
def test_a_sphere_that_grows_keeps_its_history(fresh, oracle):
    """A big sphere's radius grows by 5 % between uploads, centre fixed: X_prev = c + (X - c) r_old / r_new puts its pixels back on the
    old surface, so they keep their history, and x' follows the restatement (without the ratio it would be off by ~1 px)."""
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 200, 120
    big = int(np.argsort(-b.models["radius"], kind="stable")[1])
    grown = b.models.copy()
    grown["radius"][big] *= F32(1.05)
    s = Seq(p, oracle, b.models, w, h, 4, False)
    s.step(*brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(0)), buffers=brt.Buffers(b.models, b.materials, None))
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(1))
    s.step(lvl, cam, win, buffers=brt.Buffers(grown, b.materials, None))
    sid, _ = tr.sphere_ids(s.g, tr.Camera(oracle, cam, w, h), grown)
    mine = sid == big
    assert mine.sum() > 500
    assert (s.state[..., 3][mine] == 2).mean() > 0.9
    gy, gx = np.mgrid[0:h, 0:w]
    off = np.hypot(s.state[..., 6] - gx, s.state[..., 7] - gy)[mine & (s.state[..., 3] == 2)]
    assert np.median(off) > 0.05                                        # (the ratio moves x', y' off the pixel itself)
    p.node.write_buffers(b)


# ---- history length, shapes, formats --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("max_history", [1, 2, 3, 4, 5])
def test_history_limit_with_denoise(fresh, oracle, max_history):
    """8 still frames with DENOISE: n climbs to max_history and stays; from n = kTemporalConverged = 4 on the variance comes from the
    moments and sigma_l is unscaled."""
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 120, 72
    s = Seq(p, oracle, b.models, w, h, 4, True, max_history)
    for i in range(8):
        s.step(*brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(i)))
        hit = _hit(s.g) & np.isfinite(s.plain).all(-1)
        assert (s.state[..., 3][hit] == min(i + 1, max_history)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (17, 15), (641, 361)], ids=["1x1", "17x15", "641x361"])
def test_orbit_shapes(fresh, oracle, w, h):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    for denoise_on in (False, True):
        s = Seq(p, oracle, b.models, w, h, 4, denoise_on)
        for i in range(3):
            s.step(*_orbit(w, h, 4, i, 0.25))


@pytest.mark.gpu
def test_accumulated_frames_in_every_format(fresh, oracle):
    """The third of three still frames (n = 3) in each store format equals oracle.encode_frame of the same frame in RGBA32F."""
    p = fresh
    w, h = 57, 43
    for flags in (brt.FLAG_TEMPORAL, brt.FLAG_TEMPORAL | brt.FLAG_DENOISE):
        def third(fmt):
            p.reset_temporal()
            for i in range(3):
                lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(i))
                out = _device_frame(p, lvl, cam, win, w, h, flags, fmt if i == 2 else brt.FLAG_OUT_RGBA32F)
            return out, cam, win
        f32, cam, win = third(brt.FLAG_OUT_RGBA32F)
        f32 = f32.view(F32)
        hit = _hit(p.debug_denoise_guides(cam, win, w, h))
        assert (p.debug_temporal_state(w, h)[..., 3][hit] == 3).all()
        for fmt, name in ((brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"), (brt.FLAG_OUT_RGBA16F, "f16")):
            got, _, _ = third(fmt)
            want = oracle.encode_frame(f32, name)
            assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), (flags, name)


# ---- lifecycle, streams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_new_material_count_resets_the_history(fresh):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 160, 96
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(0))
    lvl2, cam2, win2 = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(1))
    more = np.concatenate([b.materials, b.materials[:1]])
    assert len(more) == len(b.materials) + 1
    for flags in (brt.FLAG_TEMPORAL, brt.FLAG_TEMPORAL | brt.FLAG_DENOISE):
        p.node.write_buffers(b)
        first = p.node.run(lvl2, cam2, win2, w, h, flags=flags & ~brt.FLAG_TEMPORAL).copy()
        p.reset_temporal()
        p.node.run(lvl, cam, win, w, h, flags=flags)
        p.node.write_buffers(brt.Buffers(b.models, more, b.bvh))      # same spheres, one more material
        got = p.node.run(lvl2, cam2, win2, w, h, flags=flags).copy()
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), flags
        g = p.debug_denoise_guides(cam2, win2, w, h)
        assert (p.debug_temporal_state(w, h)[..., 3][_hit(g)] == 1).all()
        # (and a re-upload with the same counts keeps it)
        p.node.write_buffers(b)
        p.reset_temporal()
        p.node.run(lvl, cam, win, w, h, flags=flags)
        p.node.write_buffers(b)
        p.node.run(lvl2, cam2, win2, w, h, flags=flags)
        assert (p.debug_temporal_state(w, h)[..., 3][_hit(g)] == 2).mean() > 0.9
    p.node.write_buffers(b)


@pytest.mark.gpu
def test_frames_on_two_streams(fresh):
    """Six temporal frames on caller streams A and B in turn, each into its own buffer, no host sync between them: the same bits as the
    six frames run one after another with a sync each (one temporal frame per context in flight, behind ev_dn)."""
    import torch
    p = fresh
    w, h = 160, 96
    views = [_orbit(w, h, 4, i, 0.5) for i in range(6)]
    for flags in (brt.FLAG_TEMPORAL, brt.FLAG_TEMPORAL | brt.FLAG_DENOISE):
        p.reset_temporal()
        want = []
        for lvl, cam, win in views:
            frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            p.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=flags)
            torch.cuda.synchronize()
            want.append(frame.cpu().numpy())
        p.reset_temporal()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda") for _ in views]
        torch.cuda.synchronize()
        for i, (lvl, cam, win) in enumerate(views):
            s = streams[i % 2]
            with torch.cuda.stream(s):
                p.node.render_device(lvl, cam, win, w, h, outs[i].data_ptr(), stream=s.cuda_stream, flags=flags)
        for s in streams:
            s.synchronize()
        for i in range(len(views)):
            assert np.array_equal(outs[i].cpu().numpy().view(np.uint32), want[i].view(np.uint32)), (flags, i)
