"""k_adaptive_select on base frames the tracer never renders (tests/adaptive_synth.py): NaN, +-INF, overflowing, negative, -0.0 and
denormal values; frame edges on, before and after a 16-pixel tile edge; waves with no, one and 64 selected lanes.  CPU: the numpy
restatement against the compiled rule pixel by pixel, and the conditions that make the frames exercise what they are made for.  GPU:
the mask against the restatement, and the refined frame in all four store formats -- the count word, the oracle's full frame where a
pixel has a class, the store of the base value everywhere else, a guard row behind the frame.  Tolerance 0 throughout."""
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import adaptive_synth as sy
import bevyray_amd as brt

F32 = np.float32
FORMATS = {brt.FLAG_OUT_RGBA32F: None, brt.FLAG_OUT_RGBA8_UNORM_SRGB: "srgb8", brt.FLAG_OUT_RGBA16F: "f16", brt.FLAG_OUT_RGBA8_UNORM: "unorm8"}
CASES = [(kind, size) for kind in sy.FRAMES for size in sy.SIZES]
CASE_IDS = [f"{kind}-{sy.size_id(size)}" for kind, size in CASES]


def _pairs(kind):
    return sy.PAIRS + ((sy.OWN_PAIR[kind],) if kind in sy.OWN_PAIR and sy.OWN_PAIR[kind] not in sy.PAIRS else ())


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def _conditions(kind, w, h, base, info, g, masks):
    """What makes a frame exercise what it is made for, under the restatement alone.  masks: {(threshold, min_taps): class mask}.
    Sizes that are exempt from a condition, all for want of pixels: the cover view has 35 hit pixels at 1x40, 12 at 40x1 and 4 at 2x2.
      noise      the two 5 % shares need 200 hit pixels, as the issue sets: 15x15 (185), 257x3 (100), 1x40, 40x1 and 2x2 are exempt
      nonfinite  a classed neighbour of a poisoned hit pixel needs 20 hit pixels: 40x1 and 2x2 are exempt (at 2x2 every pixel is poisoned)
      lanes_all  a wave of 64 selected lanes needs a 16x4 block of hit pixels: asserted at 31x33, 32x32 and 48x20; the frames of
                 15 or 17 rows or columns have one in some views only, 257x3, 1x40, 40x1 and 2x2 have no 16x4 block at all
      huge       a pixel whose counted taps (at least 6) all lie in its own region exists in every region at 31x33, 32x32 and 48x20;
                 the smaller frames have bands of 5 pixels or fewer with sky in one of them, 257x3 hits the scene in its middle band only.
                 Where such pixels exist, at whatever size, their classes are asserted."""
    hit = sy.hit_of(g)
    n_hit = int(hit.sum())
    n, pure = sy.tap_counts(base, g)
    if kind == "noise":
        m = masks[(0.4, 6)]
        if n_hit >= 200:
            assert (m[hit] == ar.NOISY).mean() >= 0.05 and (m[hit] == 0).mean() >= 0.05, ((m[hit] == ar.NOISY).mean(), (m[hit] == 0).mean())
        if (w, h) in ((17, 17), (257, 3)):      # a wave whose only appended lane is NOISY (the lanes_one frames append SPARSE lanes only)
            m, blocks = masks[(0.1, 1)], sy.wave_blocks(w, h)
            per_wave = np.bincount(blocks[m != 0], minlength=int(blocks.max()) + 1)
            noisy = np.bincount(blocks[m == ar.NOISY], minlength=int(blocks.max()) + 1)
            assert ((per_wave == 1) & (noisy == 1)).any()
    elif kind == "flat":
        assert not any((m == ar.NOISY).any() for m in masks.values())
        m = masks[(0.4, 25)]            # a hit pixel within 2 of a frame edge or of a material boundary has fewer than 25 taps
        assert (m[hit & (n < 25)] == ar.SPARSE).all() and not m[hit & (n == 25)].any() and not m[~hit].any()
        y, x = np.mgrid[0:h, 0:w]
        edge = (x < 2) | (y < 2) | (x >= w - 2) | (y >= h - 2)
        assert (m[hit & edge] == ar.SPARSE).all()
    elif kind.startswith("lanes"):
        sel = masks[sy.OWN_PAIR[kind]] != 0
        assert np.array_equal(sel, info["selected"]), int((sel != info["selected"]).sum())
        per_wave = np.bincount(sy.wave_blocks(w, h)[sel], minlength=int(sy.wave_blocks(w, h).max()) + 1)
        waves_hit = np.unique(sy.wave_blocks(w, h)[hit])
        if kind == "lanes_one":
            assert set(per_wave) <= {0, 1} and int(per_wave.sum()) == waves_hit.size
        elif kind == "lanes_alternate":
            assert set(per_wave) <= {0, 1} and not per_wave[1::2].any() and int(per_wave.sum()) == int((waves_hit % 2 == 0).sum())
        elif (w, h) in ((32, 32), (48, 20), (31, 33)):
            assert per_wave.max() == 64 and np.array_equal(sel, hit)         # a wave whose 64 lanes all append
    elif kind == "nonfinite":
        bad, ids, m = info["poisoned"], sy.ids_of(g), masks[(0.4, 6)]
        assert not np.isfinite(ar.luma(base)[bad]).any() and all(not mk[bad].any() for mk in masks.values())
        for c in sy._special(w):
            assert bad[:, c].any(), c
        for r in sy._special(h):
            assert bad[r, :].any(), r
        # a poisoned hit pixel (no class) inside the window of a same-material pixel that has one
        seen = False
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                q_bad = ar._shift(bad & hit, dx, dy, False) & (ar._shift(ids, dx, dy, np.uint32(0)) == ids)
                seen = seen or bool((q_bad & (m != 0)).any())
        if n_hit >= 20:
            assert seen
    elif kind == "huge":
        region, m = info["region"], masks[(0.4, 6)]
        l = ar.luma(base)
        assert np.isfinite(l).all()       # (the weights sum to 1: a finite colour's luminance does not overflow; at 3e38 l * l does)
        full = hit & pure & (n >= 6)
        # S2 = +INF from the fourth tap on, m * m = 1e38: v = +INF > thr * thr, NOISY.  S2 and m * m both +INF: INF - INF = NaN, v = 0
        assert (m[full & (region == 0)] == ar.NOISY).all() and not m[full & (region != 0)].any()
        if (w, h) in ((32, 32), (48, 20), (31, 33)):
            assert all((full & (region == k)).any() for k in range(3)), [(int((full & (region == k)).sum())) for k in range(3)]
    elif kind == "signed":
        assert (base[..., :3] < 0).any() and np.signbit(base[base == 0]).any()
        assert ((np.abs(base) > 0) & (np.abs(base) < np.finfo(F32).tiny)).any()


@pytest.mark.parametrize("kind,size", CASES, ids=CASE_IDS)
def test_restatement_equals_the_host_rule_and_the_frames_do_their_work(oracle, kind, size):
    w, h = size
    g = sy.cpu_guides(oracle, w, h)
    base, info = sy.frame(kind, w, h, g)
    pairs = _pairs(kind)
    host = sy.host_masks(base, g, pairs)
    masks = {}
    for pair, hm in zip(pairs, host):
        masks[pair] = ar.class_mask(base, g, *pair)
        assert np.array_equal(masks[pair], hm), (kind, size, pair, int((masks[pair] != hm).sum()))
    _conditions(kind, w, h, base, info, g, masks)


def test_s2_overflow_alone_is_noisy():
    """brt_adaptive.h: where S2 overflows and m * m does not, v is +INF and the class is NOISY (luminances of about 3.7e18 to 1.8e19
    over a flat 25-tap window) as long as thr * thr is finite; where both overflow, S2 / n - m * m is NaN, v is 0 and nothing is selected."""
    inside, ids = np.ones(25, bool), np.zeros(25, np.uint32)
    for value, want in ((3.6e18, 0), (3.8e18, ar.NOISY), (1e19, ar.NOISY), (1.8e19, ar.NOISY), (1.9e19, 0), (1e20, 0), (3e38, 0)):
        cols = np.full((25, 3), value, F32)
        for thr in (0.4, brt.ADAPT_DEFAULT_THRESHOLD, 1e-30):
            assert brt.adaptive_class(1.0, 0, cols[12], inside, ids, cols, thr, 6) == want, (value, thr)
            assert ar.class_from_taps(1.0, 0, ar.luma(cols[12]), inside, ids, ar.luma(cols), thr, 6) == want, (value, thr)
    # a threshold whose thr * thr overflows too: +INF > +INF is false.  2 x 3.8e18 squared is 5.8e37, 2 x 1e19 squared is +INF
    for value, thr, want in ((3.8e18, 2.0, ar.NOISY), (1e19, 2.0, 0), (1.8e19, 2.0, 0), (3.8e18, 1e10, 0), (1e19, 1e10, 0)):
        cols = np.full((25, 3), value, F32)
        assert brt.adaptive_class(1.0, 0, cols[12], inside, ids, cols, thr, 6) == want, (value, thr)
        assert ar.class_from_taps(1.0, 0, ar.luma(cols[12]), inside, ids, ar.luma(cols), thr, 6) == want, (value, thr)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _full(oracle, w, h):
    """The oracle's frame at the camera's own sample count: shared, never written."""
    b, lvl, cam, win = sy.view(w, h)
    full, _ = oracle.render(b, lvl, cam, win, w, h)
    full.setflags(write=False)
    return full


@pytest.fixture
def adaptive(plugin):
    plugin.set_adaptive(sy.BASE_SPP, brt.ADAPT_DEFAULT_THRESHOLD, 6)
    yield plugin
    plugin.set_adaptive(8, brt.ADAPT_DEFAULT_THRESHOLD, 6)


def _gpu_case(plugin, kind, w, h):
    b, lvl, cam, win = sy.view(w, h)
    plugin.node.write_buffers(b)
    g = plugin.debug_denoise_guides(cam, win, w, h)
    base, info = sy.frame(kind, w, h, g)
    return cam, win, g, base


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", CASES, ids=CASE_IDS)
def test_mask_equals_the_restatement(adaptive, kind, size):
    import torch
    plugin, (w, h) = adaptive, size
    cam, win, g, base = _gpu_case(plugin, kind, w, h)
    d_base = _device(base)
    for thr, mt in _pairs(kind):
        plugin.set_adaptive(sy.BASE_SPP, thr, mt)
        m = torch.full((h + 1, w), 0x55, dtype=torch.uint8, device="cuda")          # (a guard row behind the mask)
        plugin.node.adaptive_mask_device(cam, win, w, h, d_base.data_ptr(), m.data_ptr())
        torch.cuda.synchronize()
        got, want = m.cpu().numpy(), ar.class_mask(base, g, thr, mt)
        assert np.array_equal(got[:h], want), (kind, size, thr, mt, int((got[:h] != want).sum()))
        assert (got[h] == 0x55).all()


def _same_nan_class_f16(got, want):
    """f16 bits (.., 4) u16: equal, or both NaN (the payload of a NaN is not pinned, its class and a non-zero payload are)."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    nan_w = ((want & 0x7c00) == 0x7c00) & ((want & 0x3ff) != 0)
    nan_g = ((got & 0x7c00) == 0x7c00) & ((got & 0x3ff) != 0)
    return np.array_equal(nan_g, nan_w) and np.array_equal(got[~nan_w], want[~nan_w])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", CASES, ids=CASE_IDS)
def test_refined_frame_and_count(adaptive, oracle, kind, size):
    """The count word is the number of classed pixels, every one of them holds the oracle's full frame (so the list lost none), every
    other pixel the store of its base value; the row behind the frame is untouched."""
    import torch
    plugin, (w, h) = adaptive, size
    cam, win, g, base = _gpu_case(plugin, kind, w, h)
    full = _full(oracle, w, h)
    d_base = _device(base)
    forms = (0, 1) if kind == "noise" or kind.startswith("lanes") else (0,)
    # (noise at (0.1, 1): at 17x17 and 257x3 a wave appends one lane only, and that lane is NOISY)
    for (thr, mt), fmt in [(sy.OWN_PAIR.get(kind, (0.4, 6)), f) for f in FORMATS] + ([((0.1, 1), brt.FLAG_OUT_RGBA32F)] if kind == "noise" else []):
        name = FORMATS[fmt]
        plugin.set_adaptive(sy.BASE_SPP, thr, mt)
        sel = ar.class_mask(base, g, thr, mt) != 0
        words = brt.OUT_PIXEL_BYTES[fmt] // 4
        want_base = base if name is None else oracle.encode_frame(base, name)
        want_full = full if name is None else oracle.encode_frame(full, name)
        for form in forms:
            out = torch.full((h + 1, w * words), 0x11111111, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            with plugin.tuning(BRT_PIXELS_FORM=form):
                plugin.node.adaptive_refine_device(cam, win, w, h, d_base.data_ptr(), out.data_ptr(), count.data_ptr(), out_format=fmt)
            torch.cuda.synchronize()
            raw = out.cpu().numpy()
            assert (raw[h] == 0x11111111).all(), (kind, size, name, form, "guard row")
            assert int(count.cpu()[0]) == int(sel.sum()), (kind, size, name, form)
            got = raw[:h].view(want_base.dtype).reshape(h, w, 4)
            assert np.array_equal(got[sel].view(np.uint8), np.ascontiguousarray(want_full[sel]).view(np.uint8)), (kind, size, name, form, "selected")
            if name == "f16":
                assert _same_nan_class_f16(got[~sel], want_base[~sel]), (kind, size, name, form, "base")
            else:
                assert np.array_equal(got[~sel].view(np.uint8), np.ascontiguousarray(want_base[~sel]).view(np.uint8)), (kind, size, name, form, "base")
