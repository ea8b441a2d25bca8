"""The sparse pixel tracer (brt_render_pixels*, DESIGN.md "Refined upsampling").  CPU: the exports and the argument checks.  GPU: every
entry bitwise the pixel of the oracle's frame -- every pixel of a small frame in a shuffled order on five scenes, both kernel forms and
both entry points with the form that ran asserted; edge lists; plain against stream; streams; refusals.  Lists around the streaming
launch's lane count, no samples, no bounces, one-row and one-column frames, a window of another height, a camera beyond the callee tree's
reach; a host-entry list whose staging buffers grow behind a list held on a caller's stream."""
import os
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
from helpers import big_scene, big_view, resident_callee_tree, uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_render_pixels_device", "brt_render_pixels", "brt_upscale_refine_device", "brt_render_upscaled_refined_device",
           "brt_upscale_refine_mask_device")
ERR_INVALID, ERR_NO_SCENE, ERR_UNSUPPORTED = -1, -7, -8
STREAM_FORM, PLAIN_FORM = 32, 33          # brt_stats::kernel_variant of the two forms
W, H = 96, 54


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in EXPORTS:
        assert f"int32_t {name}(" in header, name
        assert name in _lib.EXPORTS, name
        assert f"pub fn {name}(" in rust, name
        assert name in defined, name
    assert "#define BRT_REFINE_EDGES 1u" in header and "#define BRT_REFINE_SPECULAR 2u" in header
    assert (brt.REFINE_EDGES, brt.REFINE_SPECULAR) == (1, 2)
    assert _lib.load().brt_abi_version() == 6


def test_argument_checks_without_a_context():
    lib = _lib.load()
    cam, win = np.zeros(80, np.uint8), np.zeros(16, np.uint8)
    px, out = np.zeros(4, np.uint32), np.zeros(16, np.float32)
    c, w = cam.ctypes.data, win.ctypes.data
    assert lib.brt_render_pixels(None, c, w, 8, 8, px.ctypes.data, 4, out.ctypes.data, 0, None) == ERR_INVALID
    assert lib.brt_render_pixels_device(None, c, w, 8, 8, 4096, 4, 8192, None, 0, None) == ERR_INVALID
    assert lib.brt_upscale_refine_device(None, c, w, 4, 4, 4096, 8, 8, 8192, 3, None, None, 0, None) == ERR_INVALID
    assert lib.brt_render_upscaled_refined_device(None, c, w, 4, 4, 8, 8, 8192, 3, None, None, 0, None) == ERR_INVALID
    assert lib.brt_upscale_refine_mask_device(None, c, w, 4, 4, 4096, 8, 8, 8192, None, 0) == ERR_INVALID
    assert b"null" in lib.brt_last_error(None)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def _pixels_dev(plugin, cam, win, w, h, pixels, flags=0, stream=None):
    """(n, 4) f32 of brt_render_pixels_device, the output pre-filled with a pattern the call must overwrite."""
    import torch
    pixels = np.ascontiguousarray(pixels, np.uint32)
    d_px = _dev(pixels)
    out = torch.full((max(pixels.size, 1), 4), 7.5, dtype=torch.float32, device="cuda")
    plugin.node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), pixels.size, out.data_ptr(), stream=stream, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:pixels.size]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scene(plugin, case):
    """-> (Buffers the oracle walks, level, camera, window, expected scene_in_lds of the streaming form) with the scene resident."""
    if case == "big32":
        lvl, cam, win = big_view(W, H)
        b, win, st = resident_callee_tree(plugin, big_scene(16383, 7), lvl, cam, win, W, H)
        return b, lvl, cam, win, 0
    kind = {"rtiow": brt.SCENE_RTIOW_FINAL, "stress": brt.SCENE_STRESS_GRID}.get(case, brt.SCENE_COVER)
    b = brt.generate_scene(kind, 1)
    lvl, cam, win = (brt.rtiow_camera if case == "rtiow" else brt.cover_camera)(W, H, 2, 4)
    if case == "cover_callee":
        b, win, st = resident_callee_tree(plugin, b, lvl, cam, win, W, H)
    else:
        plugin.node.write_buffers(b)
    return b, lvl, cam, win, 2 if case == "stress" else 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cover_callee", "cover_caller", "rtiow", "stress", "big32"])
def test_every_pixel_of_a_small_frame(plugin, oracle, case):
    """The list of every pixel of a 96x54 frame, shuffled: scattered back, the output is the oracle's frame bit for bit and the ray count
    the oracle's; both forms, host and device entry points."""
    b, lvl, cam, win, in_lds = _scene(plugin, case)
    want, cnt = oracle.render(b, lvl, cam, win, W, H)
    order = np.random.default_rng(5).permutation(W * H).astype(np.uint32)
    for flags, variant in ((0, STREAM_FORM), (brt.FLAG_KERNEL_SIMPLE, PLAIN_FORM)):
        for entry in ("device", "host"):
            got = _pixels_dev(plugin, cam, win, W, H, order, flags) if entry == "device" else plugin.node.render_pixels(cam, win, W, H, order, flags)
            st = plugin.node.last_stats
            frame = np.zeros((H * W, 4), np.float32)
            frame[order] = got
            assert _same_bits(frame.reshape(H, W, 4), want), (case, flags, entry)
            assert st["rays"] == cnt["rays"] and st["reserved"] == 0 and st["paths"] == W * H * 2, (case, flags, entry, st)
            assert st["kernel_variant"] == variant, st
            if variant == STREAM_FORM:
                assert st["scene_in_lds"] == in_lds, (case, st)
    print(f"{case}: stream form scene_in_lds {in_lds}, rays {cnt['rays']}")


@pytest.fixture(scope="module")
def cover(plugin, oracle):
    """The cover scene resident (caller's tree) and the oracle's 96x54 frame at 4 spp, 4 bounces: shared, never written."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(W, H, 4, 4)
    want, _ = oracle.render(b, lvl, cam, win, W, H)
    want.setflags(write=False)
    return b, lvl, cam, win, want


def _resident(plugin, cover):
    plugin.node.write_buffers(cover[0])       # (an unchanged scene is not re-sent)
    return cover[2], cover[3], cover[4].reshape(-1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_list_lengths(plugin, cover, n):
    cam, win, want = _resident(plugin, cover)
    px = np.random.default_rng(n).integers(0, W * H, n).astype(np.uint32)
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        assert _same_bits(_pixels_dev(plugin, cam, win, W, H, px, flags), want[px]), (n, flags)
        assert plugin.node.last_stats["paths"] == n * 4


@pytest.mark.gpu
def test_repeats_sky_only_and_longest_only(plugin, oracle, cover):
    cam, win, want = _resident(plugin, cover)
    b, lvl = cover[0], cover[1]
    p = (H * 2 // 3) * W + W // 2
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        got = _pixels_dev(plugin, cam, win, W, H, np.full(70, p, np.uint32), flags)
        assert _same_bits(got, np.broadcast_to(want[p], (70, 4)).copy())                      # one pixel 70 times: the same bytes
    # per-pixel ray counts from the oracle, a row at a time: the sky pixels (one ray per sample) and the longest pixels
    rays = np.array([oracle.render(b, lvl, cam, win, W, H, rows=(y, y + 1))[1]["rays"] for y in range(H)])
    sky_rows = np.flatnonzero(rays == W * 4)
    assert sky_rows.size > 0
    sky = (sky_rows[:, None] * W + np.arange(W)[None, :]).ravel().astype(np.uint32)
    long_row = int(np.argmax(rays))
    longest = (long_row * W + np.arange(W)).astype(np.uint32)
    for px in (sky, longest, np.concatenate([sky[:40], longest, sky[40:90]])):            # lanes end at very different times
        for flags in (0, brt.FLAG_KERNEL_SIMPLE):
            assert _same_bits(_pixels_dev(plugin, cam, win, W, H, px, flags), want[px])
    assert plugin.node.render_pixels(cam, win, W, H, sky).shape == (sky.size, 4) and plugin.node.last_stats["rays"] == sky.size * 4


@pytest.mark.gpu
def test_out_of_range_entries(plugin, cover):
    cam, win, want = _resident(plugin, cover)
    px = np.random.default_rng(3).integers(0, W * H, 200).astype(np.uint32)
    bad = np.array([0, 7, 63, 64, 130, 199])
    px[bad] = [W * H, W * H + 1, 0xFFFFFFFF, 1 << 31, W * H, W * H + 12345]
    ok = np.ones(200, bool)
    ok[bad] = False
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        for got in (_pixels_dev(plugin, cam, win, W, H, px, flags), plugin.node.render_pixels(cam, win, W, H, px, flags)):
            assert plugin.node.last_stats["reserved"] == bad.size and plugin.node.last_stats["paths"] == (200 - bad.size) * 4
            assert not got[bad].view(np.uint32).any()                                         # four zeros
            assert _same_bits(got[ok], want[px[ok]])                                          # neighbours untouched


@pytest.mark.gpu
def test_plain_against_stream(plugin, cover):
    cam, win, want = _resident(plugin, cover)
    px = np.random.default_rng(11).integers(0, W * H, 500).astype(np.uint32)
    a, b = _pixels_dev(plugin, cam, win, W, H, px, 0), _pixels_dev(plugin, cam, win, W, H, px, brt.FLAG_KERNEL_SIMPLE)
    assert _same_bits(a, b) and _same_bits(a, want[px])
    with plugin.tuning(BRT_PIXELS_FORM=1):                      # the knob forces a form whatever the flag
        plugin.node.render_pixels(cam, win, W, H, px)
        assert plugin.node.last_stats["kernel_variant"] == PLAIN_FORM
    with plugin.tuning(BRT_FORCE_GLOBAL_SCENE=1):
        assert _same_bits(plugin.node.render_pixels(cam, win, W, H, px), want[px]) and plugin.node.last_stats["scene_in_lds"] == 0
    with plugin.tuning(BRT_FORCE_LDS_TOP=64):
        assert _same_bits(plugin.node.render_pixels(cam, win, W, H, px), want[px]) and plugin.node.last_stats["scene_in_lds"] == 2


@pytest.mark.gpu
def test_streams(plugin, cover):
    import torch
    cam, win, want = _resident(plugin, cover)
    rng = np.random.default_rng(17)
    lists = [rng.integers(0, W * H, 700).astype(np.uint32) for _ in range(3)]
    d_px = [_dev(p) for p in lists]
    outs = [torch.zeros((700, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    # two calls in flight on two caller streams, a third on the default stream under FLAG_CALLER_STREAM
    plugin.node.render_pixels_device(cam, win, W, H, d_px[0].data_ptr(), 700, outs[0].data_ptr(), stream=s1.cuda_stream)
    plugin.node.render_pixels_device(cam, win, W, H, d_px[1].data_ptr(), 700, outs[1].data_ptr(), stream=s2.cuda_stream, flags=brt.FLAG_KERNEL_SIMPLE)
    plugin.node.render_pixels_device(cam, win, W, H, d_px[2].data_ptr(), 700, outs[2].data_ptr(), stream=0)
    assert plugin.node.last_stats["rays"] == 0                  # (a caller's stream is not synchronised: nothing counted)
    torch.cuda.synchronize()
    for o, p in zip(outs, lists):
        assert _same_bits(o.cpu().numpy(), want[p])


def _both_forms(plugin, oracle, b, lvl, cam, win, w, h, order, tag):
    """The list `order` of a w x h frame in both forms on the device entry point: entries, rays and paths against the oracle."""
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    rays = oracle.pixel_rays(b, cam, win, w, h).reshape(-1)
    assert int(rays.sum()) == cnt["rays"]
    spp = int(cam[0]["sample_count"])
    for flags, variant in ((0, STREAM_FORM), (brt.FLAG_KERNEL_SIMPLE, PLAIN_FORM)):
        got = _pixels_dev(plugin, cam, win, w, h, order, flags)
        st = plugin.node.last_stats
        assert st["kernel_variant"] == variant and st["reserved"] == 0, (tag, st)
        assert _same_bits(got, want.reshape(-1, 4)[order]), (tag, flags)
        assert st["rays"] == int(rays[order].sum(dtype=np.int64)) and st["paths"] == order.size * spp, (tag, flags, st)
    return want


@pytest.mark.gpu
def test_lists_around_the_launch_lane_count(plugin, oracle):
    """k_list_stream's exit test (`base >= n || n - base <= cnt`) at lists of L - 1, L, L + 1, 2 L and 2 L + 63 entries, L the
    lanes of the launch, at 1 spp with the longest pixels of the frame in a run at the end, so that the last fetch happens while lanes are
    busy.  L is read twice: from a list of 1000 entries (the launch is as wide as the list needs: one workgroup) and from one that is
    longer than the widest launch (every CU's workgroups).  The second L is above 70 000 on an MI355X and no knob plan_stream honours
    lowers it (BRT_FORCE_GLOBAL_SCENE and BRT_FORCE_LDS_TOP change the workgroup's size and the workgroups per CU, whose product stays
    1024 lanes per CU), so those lists are that long; at 1 spp each is a few milliseconds."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(W, H, 1, 4)
    plugin.node.write_buffers(b)
    want, cnt = oracle.render(b, lvl, cam, win, W, H)
    want = want.reshape(-1, 4)
    rays = oracle.pixel_rays(b, cam, win, W, H).reshape(-1).astype(np.int64)
    assert int(rays.sum()) == cnt["rays"]
    longest = np.argsort(rays, kind="stable")[-192:].astype(np.uint32)
    assert rays[longest].min() > rays.mean()
    rng = np.random.default_rng(23)
    lanes = []
    for probe in (1000, 1 << 20):
        _pixels_dev(plugin, cam, win, W, H, rng.integers(0, W * H, probe).astype(np.uint32))
        st = plugin.node.last_stats
        assert st["kernel_variant"] == STREAM_FORM
        lanes.append(st["n_workgroups"] * st["threads_per_workgroup"])
    assert lanes[0] >= 1000 and lanes[1] < (1 << 20), lanes          # (the second launch was capped by the device, not by its list)
    print(f"lanes of the launch: {lanes[0]} for 1000 entries, {lanes[1]} at most")
    for L in lanes:
        for n in (L - 1, L, L + 1, 2 * L, 2 * L + 63):
            px = np.concatenate([rng.integers(0, W * H, n - longest.size).astype(np.uint32), longest])
            for flags in (0, brt.FLAG_KERNEL_SIMPLE):
                got = _pixels_dev(plugin, cam, win, W, H, px, flags)
                st = plugin.node.last_stats
                assert _same_bits(got, want[px]), (L, n, flags)
                assert st["rays"] == int(rays[px].sum()) and st["paths"] == n and st["reserved"] == 0, (L, n, flags, st)


@pytest.mark.gpu
def test_sample_count_zero(plugin):
    """No sample: every entry is the pixel of brt_render_device's 0-spp frame (0 / 0 in the colour channels, alpha 1), no ray cast; the
    streaming form's branch of its own, the plain form and the host entry point."""
    import torch
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(W, H, 0, 4)
    plugin.node.write_buffers(b)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    plugin.node.render_device(lvl, cam, win, W, H, frame.data_ptr())
    want = frame.cpu().numpy().reshape(-1, 4)
    assert np.isnan(want[:, :3]).all() and (want[:, 3] == 1.0).all()
    px = np.random.default_rng(29).permutation(W * H).astype(np.uint32)[:3001]
    for flags, variant in ((0, STREAM_FORM), (brt.FLAG_KERNEL_SIMPLE, PLAIN_FORM)):
        for got in (_pixels_dev(plugin, cam, win, W, H, px, flags), plugin.node.render_pixels(cam, win, W, H, px, flags)):
            st = plugin.node.last_stats
            assert st["kernel_variant"] == variant and st["rays"] == 0 and st["paths"] == 0 and st["reserved"] == 0, st
            assert _same_bits(got, want[px]), flags


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 1])
def test_no_bounce_and_one_bounce_at_one_sample(plugin, oracle, bounces):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(W, H, 1, bounces)
    plugin.node.write_buffers(b)
    order = np.random.default_rng(31).permutation(W * H).astype(np.uint32)
    _both_forms(plugin, oracle, b, lvl, cam, win, W, H, order, bounces)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 37), (37, 1), (97, 3)], ids=lambda s: "%dx%d" % s)
def test_one_column_one_row_and_thin_frames(plugin, oracle, size):
    w, h = size
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(w, h, 2, 4)
    plugin.node.write_buffers(b)
    order = np.random.default_rng(37).permutation(w * h).astype(np.uint32)
    _both_forms(plugin, oracle, b, lvl, cam, win, w, h, order, size)


@pytest.mark.gpu
def test_window_of_another_height(plugin, oracle):
    """The jitter of a sample is sized by the window's height, not the frame's (raytrace.wgsl:139-147)."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, _ = brt.cover_camera(W, H, 2, 4)
    win = brt.WindowExtract.extract_component(2 * H, 0.25)
    plugin.node.write_buffers(b)
    order = np.random.default_rng(41).permutation(W * H).astype(np.uint32)
    want = _both_forms(plugin, oracle, b, lvl, cam, win, W, H, order, "window")
    same_height = oracle.render(b, lvl, cam, brt.WindowExtract.extract_component(H, 0.25), W, H)[0]
    assert not _same_bits(want, same_height)                    # (the case is real: the window's height changes the frame)


@pytest.mark.gpu
def test_camera_beyond_the_callee_trees_reach(plugin, oracle):
    """The list is the call that meets the far camera: it rebuilds the callee's tree (with_tree_reach), and its entries are the oracle's
    in the CPU twin of the tree the context reports; the other form and a plain frame behind it use that tree as it is."""
    import torch
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = uniforms(W, H, 2, 4, (13.0 * 25, 2.0 * 25, 3.0 * 25), (0.0, 0.0, 0.0), 0.4 / 25, 0.5, far=1.0e5)
    plugin.node.write_buffers(brt.generate_scene(brt.SCENE_RTIOW_FINAL, 1))      # (another scene first: the upload below is a real one)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    order = np.random.default_rng(43).permutation(W * H).astype(np.uint32)
    got = _pixels_dev(plugin, cam, win, W, H, order)
    st = dict(plugin.node.last_stats)
    assert st["tree_rebuilt"] == 1 and st["tree_reach"] == brt.tree_reach(b.models, cam)[2] > 0, st
    twin = brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, st["tree_reach"]))
    want, cnt = oracle.render(twin, lvl, cam, win, W, H)
    assert _same_bits(got, want.reshape(-1, 4)[order]) and st["rays"] == cnt["rays"] and st["kernel_variant"] == STREAM_FORM
    got = _pixels_dev(plugin, cam, win, W, H, order, brt.FLAG_KERNEL_SIMPLE)
    st2 = plugin.node.last_stats
    assert st2["tree_rebuilt"] == 0 and st2["tree_reach"] == st["tree_reach"] and st2["rays"] == cnt["rays"], st2
    assert _same_bits(got, want.reshape(-1, 4)[order])
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st3 = plugin.node.render_device(lvl, cam, win, W, H, frame.data_ptr())
    assert st3["tree_rebuilt"] == 0 and st3["tree_reach"] == st["tree_reach"] and st3["rays"] == cnt["rays"], st3
    assert _same_bits(frame.cpu().numpy(), want)


@pytest.mark.gpu
def test_a_host_list_behind_a_held_one_grows_the_staging_buffers(oracle, cover):
    """A device-entry list of 700 is held on a caller's stream; the host entry point then stages 5 000 entries, which a new context has
    no room for: the host forms' staging buffer is allocated behind the held list (whose control words the new one shares).  No host
    synchronisation between the two calls; the held list's output is read last."""
    import torch
    b, lvl, cam, win, want = cover
    want = want.reshape(-1, 4)
    rng = np.random.default_rng(47)
    held, later = rng.integers(0, W * H, 700).astype(np.uint32), rng.integers(0, W * H, 5000).astype(np.uint32)
    d_held = _dev(held)
    out = torch.full((700, 4), 7.5, dtype=torch.float32, device="cuda")
    sa = torch.cuda.Stream()
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.node.write_buffers(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                       # (a few ms: the held list starts after the second call has been made)
        fresh.node.render_pixels_device(cam, win, W, H, d_held.data_ptr(), 700, out.data_ptr(), stream=sa.cuda_stream)
        got = fresh.node.render_pixels(cam, win, W, H, later)
        st = fresh.node.last_stats
        assert _same_bits(got, want[later]) and st["paths"] == 5000 * 4 and st["reserved"] == 0
        again = fresh.node.render_pixels(cam, win, W, H, later[:1234], brt.FLAG_KERNEL_SIMPLE)      # (no growth: the buffers are reused)
        assert _same_bits(again, want[later[:1234]])
        torch.cuda.synchronize()
        assert _same_bits(out.cpu().numpy(), want[held])
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(plugin, oracle, cover):
    import torch
    cam, win, want = _resident(plugin, cover)
    lib, ctx = plugin._lib, plugin._ctx
    px = np.arange(64, dtype=np.uint32)
    d_px, out = _dev(px), torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    host_out = np.zeros((64, 4), np.float32)
    c, w = cam.ctypes.data, win.ctypes.data

    def dev(cam_p=c, win_p=w, width=W, height=H, pixels=d_px.data_ptr(), n=64, o=out.data_ptr(), flags=0):
        return lib.brt_render_pixels_device(ctx, cam_p, win_p, width, height, pixels, n, o, None, flags, None)

    assert dev(cam_p=None) == ERR_INVALID and dev(win_p=None) == ERR_INVALID
    assert dev(pixels=None) == ERR_INVALID and dev(o=None) == ERR_INVALID
    assert dev(width=0) == ERR_INVALID and dev(height=32769) == ERR_INVALID
    for flags in (brt.FLAG_COUNTERS, brt.FLAG_DENOISE, brt.FLAG_OUT_RGBA16F, brt.FLAG_TEMPORAL, 256):
        assert dev(flags=flags) == ERR_INVALID, flags
    assert lib.brt_render_pixels(ctx, c, w, W, H, px.ctypes.data, 64, host_out.ctypes.data, brt.FLAG_CALLER_STREAM, None) == ERR_INVALID
    assert dev(n=0, pixels=None, o=None) == 0                                                # an empty list: BRT_OK, nothing written
    ortho = cam.copy()
    ortho["projection"] = 1
    assert dev(cam_p=ortho.ctypes.data) == ERR_UNSUPPORTED
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert dev() == ERR_UNSUPPORTED
        assert lib.brt_render_pixels(ctx, c, w, W, H, px.ctypes.data, 64, host_out.ctypes.data, 0, None) == ERR_UNSUPPORTED
    finally:
        plugin.set_policy(0)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                                        # no refused call wrote anything
    fresh = brt.RaytracePlugin([0])
    try:
        assert fresh._lib.brt_render_pixels_device(fresh._ctx, c, w, W, H, d_px.data_ptr(), 64, out.data_ptr(), None, 0, None) == ERR_NO_SCENE
    finally:
        fresh.close()
    # the context is usable: the list, and a following frame, are still the oracle's
    assert _same_bits(_pixels_dev(plugin, cam, win, W, H, px), want[px])
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    plugin.node.render_device(cover[1], cam, win, W, H, frame.data_ptr())
    assert _same_bits(frame.cpu().numpy().reshape(-1, 4), want)
