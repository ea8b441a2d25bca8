"""The cases the rules of the sparse pixel tracer (brt_pixels_dev.h: WholePixel under PinholeStart and LensStart, ProgStart) route through
the hooks of the one kernel pair, each in BOTH forms by the knob (BRT_PIXELS_FORM 1: plain, 2: streaming) on the cover scene, bitwise
against the oracle: a pixel that begins ended (no sample to run under the whole-pixel rules; a record already at the target under the
progressive rule), the pads of the tile order, and a count word below the list's capacity under the progressive rule."""
import numpy as np
import pytest

import bevyray_amd as brt
from test_progressive import REC, Planes, _bytes, _check_step, _cover_view, _dev, _same_bytes

FORMS = (1, 2)                      # BRT_PIXELS_FORM
T = 3                               # the progressive cases' target


def _variant(base, form):
    """brt_stats::kernel_variant: the streaming form's is the family's base, the plain form's one more."""
    return base + (1 if form == 1 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rule", ["pinhole", "thin_lens"])
def test_a_whole_pixel_without_samples_begins_ended(plugin, oracle, rule, form):
    """sample_count 0 on a 4x4 frame, five entries, the third out of range: the four pixels are the average of nothing (the oracle's 0-spp
    frame: NaN colour, alpha 1; bitwise the 0-spp frame of brt_render_device), the refused entry is four zeros and counted, no ray."""
    import torch
    w = h = 4
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(w, h, 0, 4)
    plugin.node.write_buffers(b)
    want, cnt = oracle.render(b, lvl, cam, win, w, h)
    want = want.reshape(-1, 4)
    assert cnt["rays"] == 0 and np.isnan(want[:, :3]).all() and (want[:, 3] == 1.0).all()
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr())
    whole = frame.cpu().numpy().reshape(-1, 4)
    px = np.array([5, 0, w * h, 15, 9], np.uint32)
    ok = px < w * h
    d_px = _dev(px)
    out = torch.full((px.size, 4), 7.5, dtype=torch.float32, device="cuda")
    with plugin.tuning(BRT_PIXELS_FORM=form):
        if rule == "pinhole":
            st = plugin.node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), px.size, out.data_ptr())
        else:
            st = plugin.node.render_lens_pixels_device(cam, win, brt.lens(0.5, 10.0), w, h, d_px.data_ptr(), px.size, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert st["kernel_variant"] == _variant(32 if rule == "pinhole" else 34, form), st
    assert st["rays"] == 0 and st["paths"] == 0 and st["reserved"] == 1, st
    assert np.array_equal(np.isnan(got[ok]), np.isnan(want[px[ok]])) and _same_bytes(got[ok, 3], want[px[ok], 3])
    assert _same_bytes(got[ok], whole[px[ok]])
    assert not got[~ok].view(np.uint32).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_record_at_the_target_begins_ended(plugin, oracle, form):
    """9x7, a null list to 3 samples: every third pixel's record is at 3 already, the others at 0 and at 1.  The finished records are
    byte-identical afterwards and their values written; the others are the oracle's at 3; paths counts only the samples run."""
    w, h = 9, 7
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    with plugin.tuning(BRT_PIXELS_FORM=form):
        at_1, at_t = Planes(w, h), Planes(w, h)
        at_1.sample(plugin, view.cam, view.win, 1)
        at_t.sample(plugin, view.cam, view.win, T)
        _check_step(oracle, view, at_1, 1, "to 1")
        _check_step(oracle, view, at_t, T, "to the target")
        kind = (np.arange(w * h) % 3).reshape(h, w)              # 0: finished, 1: no sample yet, 2: one sample
        state = np.zeros((h, w), REC)
        state[kind == 0] = at_t.state()[kind == 0]
        state[kind == 2] = at_1.state()[kind == 2]
        planes = Planes(w, h, state=state)
        st = planes.sample(plugin, view.cam, view.win, T)
    rays_1, rays_t = view.want(1)[1].astype(np.int64), view.want(T)[1].astype(np.int64)
    assert st["kernel_variant"] == _variant(36, form) and st["reserved"] == 0, st
    assert st["paths"] == T * int((kind == 1).sum()) + (T - 1) * int((kind == 2).sum()), st
    assert st["rays"] == int(rays_t[kind != 0].sum() - rays_1[kind == 2].sum()), st
    got = planes.state()
    assert _same_bytes(got[kind == 0], state[kind == 0])
    assert _same_bytes(got, at_t.state())                          # (a continued record is the record of a pixel traced in one go)
    _check_step(oracle, view, planes, T, "mixed")                  # n, rays and every value of the frame, the finished pixels' included


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("size", [(9, 7), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_the_pads_of_a_null_list(plugin, oracle, size, order, form):
    """Neither size is a multiple of 8: the tile order (BRT_PROGRESSIVE_ORDER 1) has slots outside the frame, which are passed over and
    not refused; the raster order has none.  Every pixel is the oracle's."""
    w, h = size
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    planes = Planes(w, h)
    with plugin.tuning(BRT_PIXELS_FORM=form, BRT_PROGRESSIVE_ORDER=order):
        st = planes.sample(plugin, view.cam, view.win, T)
    assert st["kernel_variant"] == _variant(36, form) and st["reserved"] == 0 and st["paths"] == T * w * h, st
    assert st["rays"] == int(view.want(T)[1].astype(np.int64).sum()), st
    _check_step(oracle, view, planes, T, (size, order, form))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_count_word_below_the_capacity_under_the_progressive_rule(plugin, oracle, form):
    """A list of 8 entries whose device count word says 3: the first three pixels are the oracle's at the target, the entries past the
    count and every pixel not listed are untouched, records and frame."""
    w, h = 9, 7
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    listed = np.random.default_rng(8).permutation(w * h)[:8].astype(np.uint32)
    d_list, d_count = _dev(listed), _dev(np.array([3], np.uint32))
    planes = Planes(w, h)
    with plugin.tuning(BRT_PIXELS_FORM=form):
        st = planes.sample(plugin, view.cam, view.win, T, d_list.data_ptr(), listed.size, d_count.data_ptr())
    frame_t, rays_t = view.want(T)
    hit = np.zeros(w * h, bool)
    hit[listed[:3]] = True
    hit = hit.reshape(h, w)
    assert st["kernel_variant"] == _variant(36, form) and st["reserved"] == 0 and st["paths"] == T * 3, st
    assert st["rays"] == int(rays_t[hit].astype(np.int64).sum()), st
    got, fr = planes.state(), planes.frame()
    assert (got["n"][hit] == T).all() and np.array_equal(got["rays"][hit], rays_t[hit])
    assert not got[~hit].view(np.uint8).any() and (fr[~hit] == 0xCD).all()
    assert np.array_equal(fr[hit], _bytes(oracle, frame_t, planes.fmt)[hit])
