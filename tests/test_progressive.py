"""Progressive frames (brt_set_progressive, brt_progressive_sample*, brt_progressive_select_device, brt_render_progressive*,
brt_host_progressive_accumulate / _class; DESIGN.md "Progressive frames").  CPU: the exports in all four places, the refusals that need
no context, the host twins bitwise against the numpy restatement (tests/progressive_ref.py) on random records and the board of special
ones, the stand-alone twin under the sanitizers, the one-call test's condition on the model, the quality table.  GPU: continuation is
exact (frames in four formats, rays), moments are exact, lists (one longer than its launch has lanes), the one-call form, sequences and
surroundings (streams, uploads, a held call whose buffers a later call grows, refusals, plain / temporal / denoised frames and the
dispatch tile order untouched), the context's own default settings.  The selecting kernel on
synthetic planes: tests/test_progressive_synthetic.py."""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
import progressive_ref as pr
from helpers import big_scene, big_view, resident_callee_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_set_progressive", "brt_progressive_sample_device", "brt_progressive_sample", "brt_progressive_select_device",
           "brt_render_progressive_device", "brt_render_progressive", "brt_host_progressive_accumulate", "brt_host_progressive_class")
ERR_INVALID, ERR_NO_SCENE, ERR_UNSUPPORTED = -1, -7, -8
STREAM_FORM, PLAIN_FORM = 36, 37          # brt_stats::kernel_variant of the two forms
FORMS = ((0, STREAM_FORM), (brt.FLAG_KERNEL_SIMPLE, PLAIN_FORM))
FORMATS = {brt.FLAG_OUT_RGBA32F: None, brt.FLAG_OUT_RGBA8_UNORM_SRGB: "srgb8", brt.FLAG_OUT_RGBA16F: "f16", brt.FLAG_OUT_RGBA8_UNORM: "unorm8"}
REC = brt.PROG_PIXEL_DTYPE
GRID = (0.0125, 0.025, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6)
# Quality (test_quality_table): R at the default threshold 0.05, radius 1, on the MODEL of progressive_ref.CoverModel, recorded in
# DESIGN.md section 26; the bar is section 17's margin of 1.1 on it
R_RECORDED = 0.7870
ONE_CALL = dict(first=8, max_spp=64, threshold=0.1, radius=1)      # the one-call GPU test's settings


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_cpp_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "bevyray_amd", "host", "raytracing.hpp")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in EXPORTS:
        assert f"int32_t {name}(" in header, name
        assert name in _lib.EXPORTS, name
        assert f"pub fn {name}(" in rust, name
        assert name in defined, name
        if "host" not in name:
            assert f"{name}(ctx_" in hpp, name
    assert "#define BRT_PROG_SELECTED 1u" in header and "pub const BRT_PROG_SELECTED: u32 = 1;" in rust and brt.PROG_SELECTED == 1
    assert REC.itemsize == 32 and [REC.fields[k][1] for k in ("sum", "m1", "m2", "rng", "n", "rays")] == [0, 12, 16, 20, 24, 28]
    assert f"(default {brt.PROG_DEFAULT_THRESHOLD:g})" in header
    assert _lib.load().brt_abi_version() == 6


def test_calls_without_a_context_and_twins_with_null_pointers():
    lib = _lib.load()
    cam, win = np.zeros(80, np.uint8), np.zeros(16, np.uint8)
    c, w = cam.ctypes.data, win.ctypes.data
    assert lib.brt_set_progressive(None, 8, 64, 0.1, 1) == ERR_INVALID
    assert lib.brt_progressive_sample_device(None, c, w, 8, 8, 4096, None, 64, None, 4, None, None, 0, None) == ERR_INVALID
    assert lib.brt_progressive_sample(None, c, w, 8, 8, 4096, None, 64, 4, None, 0, None) == ERR_INVALID
    assert lib.brt_progressive_select_device(None, 8, 8, 4096, 4, 8192, 12288, None, None, 0) == ERR_INVALID
    assert lib.brt_render_progressive_device(None, c, w, 8, 8, 4096, 8192, None, 0, None) == ERR_INVALID
    assert lib.brt_render_progressive(None, c, w, 8, 8, 4096, 8192, 0, None) == ERR_INVALID
    rec, rgb, cls = np.zeros(9, REC), np.zeros(3, np.float32), np.zeros(1, np.uint32)
    inside = np.ones(9, np.uint32)
    assert lib.brt_host_progressive_accumulate(None, rgb.ctypes.data) == ERR_INVALID
    assert lib.brt_host_progressive_accumulate(rec.ctypes.data, None) == ERR_INVALID
    assert lib.brt_host_progressive_class(None, inside.ctypes.data, 4, 0.1, 1, cls.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32))) == ERR_INVALID
    assert lib.brt_host_progressive_class(rec.ctypes.data, inside.ctypes.data, 4, 0.1, 2, cls.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32))) == ERR_INVALID


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _twin_classes(state, target, threshold, radius):
    h, w = state.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = brt.progressive_class(*pr.window(state, x, y), target, threshold, radius)
    return out


def test_accumulate_twin_is_bitwise_the_restatement():
    rng = np.random.default_rng(7)
    board = pr.special_board().reshape(-1)
    colours = [rng.uniform(0, 2, 3).astype(np.float32) for _ in range(40)]
    colours += [np.array(c, np.float32) for c in ((np.nan, 0.5, 0.5), (0.5, np.inf, 0.1), (0.1, 0.2, -np.inf), (3e38, 3e38, 3e38), (1e-42, -0.0, 1e-45),
                                                  (-0.0, -0.0, -0.0), (2e19, 2e19, 2e19), (-3e38, 1.0, 3e38))]
    n = 0
    for i, rec in enumerate(board):
        for c in colours[i % 5::5] + colours[-8:]:
            got, want = brt.progressive_accumulate(rec, c), pr.accumulate(rec, c)
            assert _same_bytes(got, want), (rec, c, got, want)
            n += 1
    # a chain: eight samples into a zero record
    rec = np.zeros(1, REC)
    want = rec.copy()
    for c in colours[:8]:
        rec, want = brt.progressive_accumulate(rec, c), pr.accumulate(want, c)
    assert _same_bytes(rec, want) and rec["n"][0] == 8
    print(f"{n} record / colour pairs")


def test_class_twin_is_bitwise_the_restatement_on_the_board_and_on_random_planes():
    """Every pixel of the special board (windows clipped at every frame edge) and of the ten synthetic planes, at radius 0 and 1."""
    board = pr.special_board()
    own = pr.noisy(board, 0.1)
    assert own.any() and not own.all()
    # what the header says of non-finite moments, on the restatement: NaN anywhere in the moments is quiet; both overflowing is quiet;
    # m2 alone overflowing is noisy
    flat = board.reshape(-1)
    assert not own.reshape(-1)[np.isnan(flat["m1"]) | np.isnan(flat["m2"])].any()
    assert not own.reshape(-1)[np.isposinf(flat["m1"]) & np.isposinf(flat["m2"])].any()
    alone = np.isposinf(flat["m2"]) & np.isfinite(flat["m1"]) & (flat["n"] >= 2) & (flat["m1"] < 1e30)
    assert alone.any() and own.reshape(-1)[alone].all()
    for target in (2, 15, 16, 17):
        for threshold, radius in ((0.1, 1), (0.1, 0), (1e-3, 1), (30.0, 1)):
            assert np.array_equal(_twin_classes(board, target, threshold, radius), pr.classes(board, target, threshold, radius)), (target, threshold, radius)
    for k, (w, h) in enumerate(pr.SIZES):
        plane = pr.synthetic_plane(w, h, k)
        for radius in (0, 1):
            want = pr.classes(plane, 16, 0.1, radius)
            assert pr.non_vacuous(want), (w, h, radius, pr.wave_counts(want))
            if k % 3 == 0:
                assert np.array_equal(_twin_classes(plane, 16, 0.1, radius), want), (w, h, radius)


def test_the_stand_alone_twin_under_sanitizers(tmp_path):
    """tests/tools/progressive_twin_main.hip: the record and the rule alone in a program of its own, built with the address and
    undefined-behaviour sanitizers and run on the CPU over the board, read from odd addresses; its output is the restatement's."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "progressive_twin_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "bevyray_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "progressive_twin_main.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    board = pr.special_board()
    h, w = board.shape
    cols = np.array([(0.25, 0.5, 0.75), (np.nan, 1.0, 1.0), (3e38, 3e38, 3e38), (1e-42, -0.0, 0.5)], np.float32)
    for target, threshold, radius in ((16, 0.1, 1), (2, 0.05, 0)):
        head = np.array([w, h, target, radius, 0, len(cols)], np.uint32)
        head[4:5] = np.array([threshold], np.float32).view(np.uint32)
        src, dst = tmp_path / "board.bin", tmp_path / "out.bin"
        src.write_bytes(head.tobytes() + board.tobytes() + cols.tobytes())
        run = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
        out = dst.read_bytes()
        assert np.array_equal(np.frombuffer(out[:w * h], np.uint8).reshape(h, w), pr.classes(board, target, threshold, radius))
        want = board.reshape(-1).copy()
        for i in range(want.size):
            r = want[i:i + 1]
            for c in cols:
                r = pr.accumulate(r, c)
            want[i] = r[0]
        assert out[w * h:] == want.tobytes()


@pytest.fixture(scope="module")
def model(oracle):
    """The cover scene at 96x54, 8 bounces on the oracle with its prefix frames to 64 samples: shared, never written."""
    return pr.CoverModel(oracle, 64)


def test_the_one_call_tests_condition_holds_on_the_model(model):
    """A MODEL (progressive_ref.CoverModel): the settings of the GPU one-call test put pixels at three or more of the four counts."""
    n = model.counts(ONE_CALL["first"], pr.targets_of(ONE_CALL["first"], ONE_CALL["max_spp"]), ONE_CALL["threshold"], ONE_CALL["radius"])
    ok, shares = pr.distribution_ok(n, ONE_CALL["first"], ONE_CALL["max_spp"])
    print("model shares", {k: round(v, 4) for k, v in shares.items()})
    assert ok, shares


def test_quality_table(model, oracle):
    """A MODEL, not the f32 rule on the kernel's own colours: cover scene, 96x54, 8 bounces, first 8, targets doubling to 64, against 1024
    spp of another window seed.  Per (radius, threshold) the samples spent per pixel and R = MSE(progressive) / MSE(uniform at ceil(spent)
    spp) as in DESIGN.md section 17; and R of today's brt_adaptive at its default against the same reference.  Asserted: the default
    threshold is the grid point of lowest R at the default radius, and R there <= 1.1 x the recorded value.  Reported, not asserted:
    whether it is below the adaptive rule's."""
    import adaptive_ref as ar
    import denoise_ref as dr
    w, h = model.W, model.H
    lvl, cam_r, win_r = model.view(1024, 0.25)
    ref, _ = oracle.render(model.buffers, lvl, cam_r, win_r, w, h)
    ratios = {}
    for radius in (1, 0):
        for thr in GRID:
            n = model.counts(8, pr.targets_of(8, 64), thr, radius)
            spent = float(n.mean())
            k = math.ceil(spent)
            ratios[radius, thr] = pr.mse(model.progressive_frame(n), ref) / pr.mse(model.frame(k), ref)
            shares = pr.distribution_ok(n, 8, 64)[1]
            print(f"radius {radius} threshold {thr:g}: spent {spent:.2f} spp, uniform {k} spp, R {ratios[radius, thr]:.4f}, shares "
                  + " / ".join(f"{100 * s:.1f} %" for s in shares.values()))
    mask = ar.class_mask(model.frame(8), dr.guides(oracle, model.buffers, cam_r, w, h), brt.ADAPT_DEFAULT_THRESHOLD, 6)
    s = float((mask != 0).mean())
    r_adaptive = ar.mse(ar.adaptive(model.frame(8), model.frame(64), mask), ref) / ar.mse(model.frame(math.ceil(8 + 64 * s)), ref)
    best = min(GRID, key=lambda t: ratios[1, t])
    print(f"brt_adaptive at its default: share {s:.4f}, spent {8 + 64 * s:.2f} spp, R {r_adaptive:.4f}; progressive at {best:g}: "
          f"R {ratios[1, best]:.4f} -- {'below' if ratios[1, best] < r_adaptive else 'NOT below'} the adaptive rule's")
    assert brt.PROG_DEFAULT_THRESHOLD == best, ratios
    assert ratios[1, best] <= 1.1 * R_RECORDED, ratios


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

GUARD = 4096


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Planes:
    """A zeroed state plane and a frame on the device, each with a guard row of 0xCD behind it."""

    def __init__(self, w, h, fmt=brt.FLAG_OUT_RGBA32F, state=None):
        import torch
        self.w, self.h, self.fmt = w, h, fmt
        self.state_bytes, self.frame_bytes = w * h * 32, w * h * brt.OUT_PIXEL_BYTES[fmt]
        self.d_state = torch.zeros(self.state_bytes + GUARD, dtype=torch.uint8, device="cuda")
        if state is not None:
            self.d_state[:self.state_bytes] = _dev(state)
        self.d_state[self.state_bytes:] = 0xCD
        self.d_frame = torch.full((self.frame_bytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def state(self):
        import torch
        torch.cuda.synchronize()
        raw = self.d_state.cpu().numpy()
        assert (raw[self.state_bytes:] == 0xCD).all(), "the guard row behind the state was written"
        return raw[:self.state_bytes].view(REC).reshape(self.h, self.w).copy()

    def frame(self):
        import torch
        torch.cuda.synchronize()
        raw = self.d_frame.cpu().numpy()
        assert (raw[self.frame_bytes:] == 0xCD).all(), "the guard row behind the frame was written"
        return raw[:self.frame_bytes].reshape(self.h, self.w, -1).copy()

    def sample(self, plugin, cam, win, target, d_pixels=0, n_pixels=None, d_count=0, flags=0, stream=None, frame=True):
        return plugin.node.progressive_sample_device(cam, win, self.w, self.h, self.d_state.data_ptr(), target, d_pixels, n_pixels, d_count,
                                                     self.d_frame.data_ptr() if frame else 0, stream=stream, out_format=self.fmt, flags=flags)


def _bytes(oracle, frame, fmt):
    f = frame if FORMATS[fmt] is None else oracle.encode_frame(frame, FORMATS[fmt])
    h, w = frame.shape[:2]
    return np.ascontiguousarray(f).view(np.uint8).reshape(h, w, -1)


class View:
    """A scene with a view on it and the oracle's frames and per-pixel ray counts by sample count, computed once."""

    def __init__(self, oracle, buffers, view_of, w, h):
        self.oracle, self.b, self.view_of, self.w, self.h = oracle, buffers, view_of, w, h
        self.lvl, self.cam, self.win = view_of(1)

    @functools.lru_cache(maxsize=None)
    def want(self, n):
        lvl, cam, win = self.view_of(n)
        frame, _ = self.oracle.render(self.b, lvl, cam, self.win, self.w, self.h)
        rays = self.oracle.pixel_rays(self.b, cam, self.win, self.w, self.h)
        frame.setflags(write=False)
        rays.setflags(write=False)
        return frame, rays


@functools.lru_cache(maxsize=None)
def _cover_view(oracle, w, h, bounces=4):
    return View(oracle, brt.generate_scene(brt.SCENE_COVER, 1), lambda n: brt.cover_camera(w, h, n, bounces), w, h)


def _check_step(oracle, view, planes, n, where):
    frame, rays = view.want(n)
    st = planes.state()
    assert (st["n"] == n).all(), where
    assert np.array_equal(st["rays"], rays), where
    assert np.array_equal(planes.frame(), _bytes(oracle, frame, planes.fmt)), where


SEQUENCES = ((1, 2, 3), (3, 8), (8, 16, 64), (64,))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["caller", "callee"])
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (33, 17), (64, 40)], ids=lambda s: "%dx%d" % s)
def test_continuation_is_exact(plugin, oracle, tree, size):
    """After every step of every target sequence the frame is bitwise the oracle's at that sample count in the four store formats, and
    `rays` the oracle's per-pixel ray count; both kernel forms, both entry points; a guard row behind the frame and the state."""
    w, h = size
    view = _cover_view(oracle, w, h)
    if tree == "caller":
        plugin.node.write_buffers(view.b)
        v = view
    else:
        b, win, _ = resident_callee_tree(plugin, view.b, view.lvl, view.cam, view.win, w, h)
        v = View(oracle, b, view.view_of, w, h)
    for flags, variant in FORMS:
        for seq in SEQUENCES:
            fmts = list(FORMATS)
            planes = Planes(w, h, fmts[len(seq) % 4])
            host_state, host_frame = np.zeros((h, w), REC), np.full((h, w, 4), 7.5, np.float32)
            for n in seq:
                st = planes.sample(plugin, v.cam, v.win, n, flags=flags)
                assert st["kernel_variant"] == variant and st["reserved"] == 0, st
                assert st["rays"] == int(v.want(n)[1].astype(np.int64).sum()) - int(planes_prev_rays(v, seq, n)), (seq, n, st)
                _check_step(oracle, v, planes, n, (tree, size, flags, seq, n))
                # the other formats: a second call to the same target leaves the records byte for byte and still stores the values
                before = planes.state()
                for fmt in fmts:
                    other = Planes(w, h, fmt, before)
                    st2 = other.sample(plugin, v.cam, v.win, n, flags=flags)
                    assert st2["rays"] == 0 and st2["paths"] == 0, st2
                    assert _same_bytes(other.state(), before) and np.array_equal(other.frame(), _bytes(oracle, v.want(n)[0], fmt)), (seq, n, fmt)
                plugin.node.progressive_sample(v.cam, v.win, w, h, host_state, n, frame=host_frame, flags=flags)
                assert plugin.node.last_stats["kernel_variant"] == variant
                assert _same_bytes(host_state, before) and _same_bytes(host_frame, v.want(n)[0]), (tree, size, flags, seq, n, "host")


def planes_prev_rays(view, seq, n):
    """The rays of the steps of `seq` before the step to n."""
    i = seq.index(n)
    return view.want(seq[i - 1])[1].astype(np.int64).sum() if i else 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stress_lds_top", "big32"])
def test_continuation_on_the_other_scene_paths(plugin, oracle, case):
    """The stress grid with the top of the tree in LDS, and a 16 383-sphere scene that needs 32-bit descriptors: the path that ran is
    asserted."""
    w, h = 33, 17
    if case == "big32":
        lvl, cam, win = big_view(w, h)
        b, win, _ = resident_callee_tree(plugin, big_scene(16383, 7), lvl, cam, win, w, h)
        view = View(oracle, b, lambda n: big_view(w, h, spp=n), w, h)
        view.win = win
        in_lds = 0
    else:
        b = brt.generate_scene(brt.SCENE_STRESS_GRID, 1)
        plugin.node.write_buffers(b)
        view = View(oracle, b, lambda n: brt.cover_camera(w, h, n, 4), w, h)
        in_lds = 2
    for flags, variant in FORMS:
        planes = Planes(w, h)
        for n in (3, 8):
            st = planes.sample(plugin, view.cam, view.win, n, flags=flags)
            assert st["kernel_variant"] == variant, st
            if variant == STREAM_FORM:
                assert st["scene_in_lds"] == in_lds, (case, st)
            _check_step(oracle, view, planes, n, (case, flags, n))
    if case == "big32":
        assert len(b.models) > 16382                                # (DESC16_MAX_INDEX: the first scene of test_desc32 that needs 32 bits)


@pytest.mark.gpu
def test_moments_are_exact(plugin, oracle):
    """One sample per call for six calls at 33x17: every step's colour is recomputed by the oracle's radiance entry (one sample) from the
    ray the record's own rng yields under the pinhole rule (the lens tests' host twin), and sum, m1, m2, n are bitwise the restated
    accumulation.  With the 6-sample frame being the oracle's this pins every intermediate rng."""
    w, h = 33, 17
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    planes = Planes(w, h)
    pinhole = brt.lens(0.0)
    want = np.zeros((h, w), REC)
    for step in range(1, 7):
        before = planes.state()
        entries = np.zeros(w * h, brt.RADIANCE_RAY_DTYPE)
        for p in range(w * h):
            px, py = p % w, p // w
            state = int(before[py, px]["rng"]) if step > 1 else brt.lens_seed(view.win, w, h, px, py)
            o, d, after = brt.lens_ray(view.cam, view.win, pinhole, w, h, px, py, state)
            entries[p]["origin"], entries[p]["direction"], entries[p]["seed"] = o, d, after
        rgb = oracle.radiance(view.b, entries, 1, int(view.cam[0]["bounce_count"]))[0]["rgb"]
        planes.sample(plugin, view.cam, view.win, step, flags=FORMS[step % 2][0])
        got = planes.state()
        for p in range(w * h):
            want[p // w, p % w] = pr.accumulate(want[p // w, p % w], rgb[p])[0]
        for k in ("sum", "m1", "m2", "n"):
            assert _same_bytes(got[k], want[k]), (step, k)
    _check_step(oracle, view, planes, 6, "six single samples")
    assert pr.noisy(planes.state(), 0.1).any() and not pr.noisy(planes.state(), 0.1).all()


@pytest.mark.gpu
def test_lists(plugin, oracle):
    """A shuffled half of the frame; the count word; lengths 1, 63, 64, 65 and around one workgroup's lane count (the whole launch's:
    test_a_list_longer_than_the_launch_has_lanes); out-of-range entries at places 0 / 31 / 32 / 63 / 64; records with n >= target and pixels not listed are byte-identical afterwards."""
    import torch
    w, h = 64, 40
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    rng = np.random.default_rng(3)
    f3, r3 = view.want(3)
    f8, r8 = view.want(8)

    def check(planes, listed, base_state, n_to, where):
        """The listed pixels are at n_to, everything else is as it was."""
        st = planes.state()
        hit = np.zeros(w * h, bool)
        hit[listed] = True
        hit = hit.reshape(h, w)
        assert _same_bytes(st[~hit], base_state[~hit]), where
        moved = hit & (base_state["n"] < n_to)
        assert (st["n"][moved] == n_to).all() and np.array_equal(st["rays"][moved], view.want(n_to)[1][moved]), where
        assert _same_bytes(st[hit & ~moved], base_state[hit & ~moved]), where
        fr = planes.frame().view(np.float32).reshape(h, w, 4)
        assert _same_bytes(fr[moved], view.want(n_to)[0][moved]), where
        assert (fr[~hit].view(np.uint8) == 0xCD).all(), where

    probe = Planes(w, h)
    block = probe.sample(plugin, view.cam, view.win, 1)["threads_per_workgroup"]      # one workgroup's lane count
    lengths = sorted({1, 63, 64, 65, block - 1, block, block + 1, 2 * block + 1, w * h // 2})
    for flags, variant in FORMS:
        for n in lengths:
            planes = Planes(w, h)
            listed = rng.permutation(w * h)[:n].astype(np.uint32)
            s = planes.sample(plugin, view.cam, view.win, 3, _dev(listed).data_ptr(), n, flags=flags)
            assert s["kernel_variant"] == variant and s["paths"] == 3 * n, (n, s)
            check(planes, listed, np.zeros((h, w), REC), 3, (flags, n))
        # the count word: a capacity of the whole frame, 700 entries counted; then the same list to 8 with some pixels already there
        planes = Planes(w, h)
        listed = rng.permutation(w * h).astype(np.uint32)
        d_list, d_count = _dev(listed), _dev(np.array([700], np.uint32))
        planes.sample(plugin, view.cam, view.win, 3, d_list.data_ptr(), w * h, d_count.data_ptr(), flags=flags)
        check(planes, listed[:700], np.zeros((h, w), REC), 3, (flags, "count"))
        base = planes.state()
        planes.d_frame[:] = 0xCD
        torch.cuda.synchronize()
        mixed = np.concatenate([listed[500:700], listed[700:900]])           # 200 at 3 samples, 200 at none
        planes.sample(plugin, view.cam, view.win, 8, _dev(mixed).data_ptr(), mixed.size, flags=flags)
        check(planes, mixed, base, 8, (flags, "mixed"))
        base = planes.state()
        planes.d_frame[:] = 0xCD
        torch.cuda.synchronize()
        s = planes.sample(plugin, view.cam, view.win, 3, _dev(mixed).data_ptr(), mixed.size, flags=flags)      # every record has n >= 3
        assert s["rays"] == 0 and s["paths"] == 0
        assert _same_bytes(planes.state(), base)
        fr = planes.frame().view(np.float32).reshape(-1, 4)
        assert _same_bytes(fr[mixed], f8.reshape(-1, 4)[mixed])                 # ... and its value is still stored
        # out-of-range entries
        planes = Planes(w, h)
        listed = rng.permutation(w * h)[:130].astype(np.uint32)
        bad = np.array([0, 31, 32, 63, 64])
        listed[bad] = [w * h, 0xFFFFFFFF, 1 << 31, w * h + 1, w * h + 12345]
        ok = np.ones(listed.size, bool)
        ok[bad] = False
        s = planes.sample(plugin, view.cam, view.win, 3, _dev(listed).data_ptr(), listed.size, flags=flags)
        assert s["reserved"] == bad.size and s["paths"] == 3 * int(ok.sum()), s
        check(planes, listed[ok], np.zeros((h, w), REC), 3, (flags, "refused"))
    assert r3.sum() < r8.sum() and not _same_bytes(f3, f8)


@pytest.mark.gpu
def test_a_list_longer_than_the_launch_has_lanes(plugin, oracle):
    """The streaming launch's grid is capped by the device, not by the list: on a frame with more pixels than the launch has lanes every
    lane takes further entries from the batch counter while its neighbours are in flight, and the record it carries (m1, m2, rays) starts
    again with each.  Lists of lanes - 1, lanes + 1 entries and the whole frame, to 2 and on to 3 samples: the frame and the rays are the
    oracle's, and the records are bitwise the plain form's, which never refills."""
    w, h = 1024, 768
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    stream, plain = Planes(w, h), Planes(w, h)
    st = stream.sample(plugin, view.cam, view.win, 2)
    lanes = st["n_workgroups"] * st["threads_per_workgroup"]
    assert st["kernel_variant"] == STREAM_FORM and lanes + 1 < w * h, (st, "the frame must outnumber the launch's lanes")
    plain.sample(plugin, view.cam, view.win, 2, flags=brt.FLAG_KERNEL_SIMPLE)
    _check_step(oracle, view, stream, 2, "whole frame, streaming form")
    assert _same_bytes(stream.state(), plain.state())
    order = np.random.default_rng(9).permutation(w * h).astype(np.uint32)
    d_order = _dev(order)
    for n in (lanes - 1, lanes + 1):
        a, b = Planes(w, h), Planes(w, h)
        sa = a.sample(plugin, view.cam, view.win, 2, d_order.data_ptr(), n)
        b.sample(plugin, view.cam, view.win, 2, d_order.data_ptr(), n, flags=brt.FLAG_KERNEL_SIMPLE)
        assert sa["kernel_variant"] == STREAM_FORM and sa["paths"] == 2 * n
        got = a.state()
        assert _same_bytes(got, b.state())
        listed = np.zeros(w * h, bool)
        listed[order[:n]] = True
        assert _same_bytes(got.reshape(-1)[listed], stream.state().reshape(-1)[listed]) and not got.reshape(-1)[~listed].view(np.uint8).any()
    stream.sample(plugin, view.cam, view.win, 3, d_order.data_ptr(), w * h)      # records with n > 0 carried on, in a shuffled order
    plain.sample(plugin, view.cam, view.win, 3, flags=brt.FLAG_KERNEL_SIMPLE)
    _check_step(oracle, view, stream, 3, "carried on")
    assert _same_bytes(stream.state(), plain.state())


def _select(plugin, w, h, d_state, target, mask=True):
    """(sorted list, count, mask) of brt_progressive_select_device."""
    import torch
    d_list = torch.full((w * h + 16,), 0xCDCDCDCD - (1 << 32), dtype=torch.int32, device="cuda")
    d_count = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    d_mask = torch.full((w * h + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plugin.node.progressive_select_device(w, h, d_state.data_ptr(), target, d_list.data_ptr(), d_count.data_ptr(), d_mask.data_ptr() if mask else 0)
    torch.cuda.synchronize()
    cnt = d_count.cpu().numpy().view(np.uint32)
    lst = d_list.cpu().numpy().view(np.uint32)
    msk = d_mask.cpu().numpy()
    n = int(cnt[0])
    assert (cnt[1:] == 77).all() and (lst[n:] == 0xCDCDCDCD).all() and (msk[w * h:] == 0xCD).all()
    return np.sort(lst[:n]), n, msk[:w * h].reshape(h, w), d_list, d_count


@pytest.mark.gpu
def test_one_call(plugin, oracle, model):
    """Cover scene 96x54, first 8, max 64, radius 1, threshold 0.1.  On the GPU's own state: every n is a target and at least three
    counts hold >= 3 % of the pixels (the model says 26 / 5 / 12 / 56 %); frame[p] is bitwise the oracle's n_p-sample frame at p; the
    one-call form equals its steps; calling again with max 128 equals a fresh call at 128 from a zeroed plane.  Both kernel forms, both
    entry points."""
    w, h = model.W, model.H
    plugin.node.write_buffers(model.buffers)
    lvl, cam, win = model.view(1)
    first, max_spp, thr, radius = (ONE_CALL[k] for k in ("first", "max_spp", "threshold", "radius"))
    try:
        plugin.set_progressive(first, max_spp, thr, radius)
        ref_state = None
        for flags, variant in FORMS:
            planes = Planes(w, h)
            st = plugin.node.render_progressive_device(cam, win, w, h, planes.d_state.data_ptr(), planes.d_frame.data_ptr(), flags=flags)
            state = planes.state()
            ok, shares = pr.distribution_ok(state["n"], first, max_spp)
            print("GPU shares", {k: round(v, 4) for k, v in shares.items()}, "variant", st["kernel_variant"])
            assert ok, shares
            assert st["kernel_variant"] == variant
            want = model.progressive_frame(state["n"])
            assert _same_bytes(planes.frame().view(np.float32).reshape(h, w, 4), want)
            assert st["paths"] == int(state["n"].sum()) and st["rays"] == int(state["rays"].astype(np.int64).sum()), st
            # the host entry
            hs, hf = np.zeros((h, w), REC), np.zeros((h, w, 4), np.float32)
            plugin.node.render_progressive(cam, win, w, h, hs, hf, flags=flags)
            assert _same_bytes(hs, state) and _same_bytes(hf, want)
            # its steps
            steps = Planes(w, h)
            steps.sample(plugin, cam, win, first, flags=flags)
            for t in pr.targets_of(first, max_spp):
                lst, n, mask, d_list, d_count = _select(plugin, w, h, steps.d_state, t)
                assert np.array_equal(mask, pr.classes(steps.state(), t, thr, radius)) and n == int((mask != 0).sum())
                steps.sample(plugin, cam, win, t, d_list.data_ptr(), w * h, d_count.data_ptr(), flags=flags)
            assert _same_bytes(steps.state(), state) and _same_bytes(steps.frame(), planes.frame())
            if ref_state is None:
                ref_state = state
            assert _same_bytes(state, ref_state)                      # both forms: the same bytes
        # carried on to 128 against a fresh call at 128
        plugin.set_progressive(first, 128, thr, radius)
        plugin.node.render_progressive_device(cam, win, w, h, planes.d_state.data_ptr(), planes.d_frame.data_ptr())
        fresh = Planes(w, h)
        plugin.node.render_progressive_device(cam, win, w, h, fresh.d_state.data_ptr(), fresh.d_frame.data_ptr())
        assert (fresh.state()["n"] == 128).any()
        assert _same_bytes(planes.state(), fresh.state()) and _same_bytes(planes.frame(), fresh.frame())
    finally:
        plugin.set_progressive()


@pytest.mark.gpu
def test_setter_and_refusals_each_followed_by_a_correct_call(plugin, oracle):
    import torch
    w, h = 33, 17
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    lib, ctx = plugin._lib, plugin._ctx
    planes = Planes(w, h)
    cam, win = view.cam, view.win
    c, wn, ds, df = cam.ctypes.data, win.ctypes.data, planes.d_state.data_ptr(), planes.d_frame.data_ptr()

    def good(n):
        planes.sample(plugin, cam, win, n)
        _check_step(oracle, view, planes, n, n)

    # the setter: every bad value, and the settings stay as they were
    plugin.set_progressive(4, 32, 0.2, 0)
    for bad in ((1, 64, 0.1, 1), (0, 64, 0.1, 1), (9, 8, 0.1, 1), (8, 65536, 0.1, 1), (8, 64, 0.0, 1), (8, 64, -1.0, 1), (8, 64, float("nan"), 1),
                (8, 64, float("inf"), 1), (8, 64, 0.1, 2), (8, 64, 0.1, 0xFFFFFFFF)):
        assert lib.brt_set_progressive(ctx, *bad) == ERR_INVALID, bad
    p2 = Planes(w, h)
    plugin.node.render_progressive_device(cam, win, w, h, p2.d_state.data_ptr(), p2.d_frame.data_ptr())
    assert set(np.unique(p2.state()["n"])) <= {4, 8, 16, 32} and (p2.state()["n"] >= 4).all()
    plugin.set_progressive(2, 2, 1e-30, 1)
    plugin.set_progressive(65535, 65535, 3e38, 0)
    plugin.set_progressive()
    n = 0
    refusals = [
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, None, wn, w, h, ds, None, w * h, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, None, w, h, ds, None, w * h, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, None, None, w * h, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 0, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 65536, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, 0, h, ds, None, 0, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, 32769, ds, None, w * 32769, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h - 1, None, 2, df, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 2, ds + 32, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 2, df, None, brt.FLAG_DENOISE, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 2, df, None, brt.FLAG_TEMPORAL, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 2, df, None, brt.FLAG_COUNTERS, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive_device(ctx, c, wn, w, h, ds, None, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive_device(ctx, c, wn, w, h, ds, ds, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive_device(ctx, c, wn, w, h, ds, df, None, brt.FLAG_DENOISE, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, None, 4, df, df + 8192, None, None, 0)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, ds, 0, df, df + 8192, None, None, 0)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, ds, 4, df, None, None, None, 0)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, ds, 4, None, None, None, None, 0)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, ds, 4, ds, ds + 64, None, None, 0)),
        (ERR_INVALID, lambda: lib.brt_progressive_select_device(ctx, w, h, ds, 4, df, df + 8192, None, None, brt.FLAG_KERNEL_SIMPLE)),
    ]
    hs, hf = np.zeros((h, w), REC), np.zeros((h, w, 4), np.float32)
    hsp, hfp = hs.ctypes.data, hf.ctypes.data
    refusals += [
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, hsp, None, w * h, 2, hfp, brt.FLAG_CALLER_STREAM, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, hsp, None, w * h, 2, hfp, brt.FLAG_DENOISE, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, None, None, w * h, 2, hfp, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, hsp, None, w * h - 1, 2, hfp, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, hsp, None, w * h, 0, hfp, 0, None)),
        (ERR_INVALID, lambda: lib.brt_progressive_sample(ctx, c, wn, w, h, hsp, None, w * h, 2, hsp + 64, 0, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive(ctx, c, wn, w, h, hsp, hfp, brt.FLAG_CALLER_STREAM, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive(ctx, c, wn, w, h, hsp, hfp, brt.FLAG_TEMPORAL, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive(ctx, c, wn, w, h, hsp, None, 0, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive(ctx, c, wn, w, h, None, hfp, 0, None)),
        (ERR_INVALID, lambda: lib.brt_render_progressive(ctx, c, wn, 0, h, hsp, hfp, 0, None)),
    ]
    for code, call in refusals:
        assert call() == code, refusals.index((code, call))
        n += 1
        good(n)
    assert not hs.view(np.uint8).any() and not hf.any()              # (a refused host call writes nothing)
    ortho = cam.copy()
    ortho["projection"] = 1
    assert lib.brt_progressive_sample_device(ctx, ortho.ctypes.data, wn, w, h, ds, None, w * h, None, 40, df, None, 0, None) == ERR_UNSUPPORTED
    good(n + 1)
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert lib.brt_progressive_sample_device(ctx, c, wn, w, h, ds, None, w * h, None, 40, df, None, 0, None) == ERR_UNSUPPORTED
        assert lib.brt_render_progressive_device(ctx, c, wn, w, h, ds, df, None, 0, None) == ERR_UNSUPPORTED
    finally:
        plugin.set_policy(0)
    good(n + 2)
    with brt.RaytracePlugin([0]) as fresh:
        assert fresh._lib.brt_progressive_sample_device(fresh._ctx, c, wn, w, h, ds, None, w * h, None, 2, df, None, 0, None) == ERR_NO_SCENE
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_streams_uploads_held_calls_and_plain_frames_around(plugin, oracle):
    """Two caller streams with an upload of another scene between them, and a host call of a larger frame behind them; plain, denoised and
    temporal frames and the dispatch tile order (brt_debug_tile_order) are the same before and after: bitwise, same rays, same
    kernel_variant.  (The held call whose buffers a later call grows: test_a_larger_call_behind_a_held_one_grows_the_buffers.)"""
    import torch
    w, h = 64, 40
    view = _cover_view(oracle, w, h)
    plugin.node.write_buffers(view.b)
    lvl8, cam8, win = brt.cover_camera(w, h, 8, 4)

    def plain_frames():
        out = []
        for flags in (0, brt.FLAG_DENOISE, brt.FLAG_DENOISE | brt.FLAG_TEMPORAL):
            plugin.reset_temporal()
            f = plugin.node.run(lvl8, cam8, win, w, h, flags=flags)
            out.append((f.copy(), plugin.node.last_stats["rays"], plugin.node.last_stats["kernel_variant"]))
        # the dispatch order the context builds on the GPU from per-tile ray counts (as tests/test_gbuffer.py observes it)
        n_tiles = 24
        ray_sum = (np.arange(n_tiles, dtype=np.uint32) * 37) % 101 + 1
        longest = (np.arange(n_tiles, dtype=np.uint32) * 13) % 17 + 1
        order, info = np.zeros(n_tiles, np.uint32), np.zeros(5, np.uint32)
        _lib.check(plugin._lib.brt_debug_tile_order(plugin._ctx, ray_sum.ctypes.data, longest.ctypes.data, n_tiles, 2, 4096, 1, 0, 0,
                                                    order.ctypes.data, info.ctypes.data), plugin._ctx)
        out.append((np.concatenate([order, info]), 0, 0))
        return out

    plain_frames()                                                   # (the view's first frames measure its dispatch order)
    before = plain_frames()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b2 = Planes(w, h), Planes(w, h)
    torch.cuda.synchronize()
    a.sample(plugin, view.cam, view.win, 8, stream=s1.cuda_stream)
    a.sample(plugin, view.cam, view.win, 16, stream=s2.cuda_stream)
    other = brt.generate_scene(brt.SCENE_RTIOW_FINAL, 1)
    plugin.node.write_buffers(other)                                 # (an upload waits for the lists of the context)
    oview = View(oracle, other, lambda n: brt.rtiow_camera(w, h, n, 4), w, h)
    b2.sample(plugin, oview.cam, oview.win, 3, stream=s2.cuda_stream)
    b2.sample(plugin, oview.cam, oview.win, 8, stream=s1.cuda_stream)
    W2, H2 = 96, 54
    big = View(oracle, other, lambda n: brt.rtiow_camera(W2, H2, n, 4), W2, H2)
    hs, hf = np.zeros((H2, W2), REC), np.zeros((H2, W2, 4), np.float32)
    plugin.node.progressive_sample(big.cam, big.win, W2, H2, hs, 2, frame=hf)
    assert _same_bytes(hf, big.want(2)[0]) and np.array_equal(hs["rays"], big.want(2)[1])
    _check_step(oracle, view, a, 16, "two streams")
    _check_step(oracle, oview, b2, 8, "behind the upload")
    plugin.node.write_buffers(view.b)
    after = plain_frames()
    assert len(before) == len(after) == 4 and before[3][0].any()
    for (f0, r0, v0), (f1, r1, v1) in zip(before, after):
        assert _same_bytes(f0, f1) and r0 == r1 and v0 == v1
    assert plugin.get_tuning("BRT_PROGRESSIVE_ORDER")[0] == 1         # (whole-frame passes above started in 8x8 tiles)
    with plugin.tuning(BRT_PROGRESSIVE_ORDER=0):                     # the knob's raster order: the same bytes
        t = Planes(w, h)
        t.sample(plugin, view.cam, view.win, 3)
        _check_step(oracle, view, t, 3, "raster order")
        t7 = Planes(7, 5)
        v7 = _cover_view(oracle, 7, 5)
        t7.sample(plugin, v7.cam, v7.win, 2, flags=brt.FLAG_KERNEL_SIMPLE)
        _check_step(oracle, v7, t7, 2, "raster order, plain form")


@pytest.mark.gpu
def test_a_larger_call_behind_a_held_one_grows_the_buffers(plugin, oracle):
    """A NEW context, whose buffers are all unallocated or minimal, and its own default settings (no setter call).  Every device buffer of
    the test is allocated first; from the hold to the last assertion on it nothing synchronises the device.  Stream A is held
    (test_caller_streams.Streams.hold) and takes a one-call device form at 64x40 -- its list lives in the context's list buffer --; a
    sample call that needs no larger buffer goes to stream B, and the hold is asserted to be still on behind both.  Then a one-call
    device form at 96x54 has to grow the list buffer and the host forms have to allocate the staging buffers: the context waits for the
    held call on the host before it frees or allocates, so those calls return only once the hold has ended (that wait is why the hold
    cannot be asserted behind THEM).  The held call's planes are read last.  Every result is what the session's context gives under
    PROG_DEFAULT_THRESHOLD, first 8, max 64, radius 1 stated explicitly, and the fresh context's selection is the restatement's."""
    import torch
    from test_caller_streams import Streams
    w, h, W2, H2 = 64, 40, 96, 54
    small, large = _cover_view(oracle, w, h), _cover_view(oracle, W2, H2)
    plugin.node.write_buffers(small.b)

    def one_call(p, view, planes, stream=None):
        p.node.render_progressive_device(view.cam, view.win, planes.w, planes.h, planes.d_state.data_ptr(), planes.d_frame.data_ptr(), stream=stream)

    try:
        plugin.set_progressive(8, 64, brt.PROG_DEFAULT_THRESHOLD, 1)
        ws, wl = Planes(w, h), Planes(W2, H2)
        one_call(plugin, small, ws)
        one_call(plugin, large, wl)
        want_small, want_large = (ws.state(), ws.frame()), (wl.state(), wl.frame())
    finally:
        plugin.set_progressive()
    assert len(np.unique(want_small[0]["n"])) >= 2 and len(np.unique(want_large[0]["n"])) >= 2
    streams = Streams()
    held, side, later = Planes(w, h), Planes(w, h), Planes(W2, H2)
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.node.write_buffers(small.b)
        torch.cuda.synchronize()
        hold = streams.hold(streams.a)
        one_call(fresh, small, held, stream=streams.a.cuda_stream)
        side.sample(fresh, small.cam, small.win, 2, stream=streams.b.cuda_stream)      # (the control words alone: nothing to grow)
        done = torch.cuda.Event()
        done.record(streams.a)
        assert not hold.query() and not done.query()            # (both were enqueued while A was held: the held call has not begun)
        one_call(fresh, large, later)                           # (grows the list buffer: waits on the host for the held call)
        assert done.query()                                     # (... so the held call has ended when this one returns)
        hs, hf = np.zeros((H2, W2), REC), np.zeros((H2, W2, 4), np.float32)
        fresh.node.render_progressive(large.cam, large.win, W2, H2, hs, hf)      # (allocates the staging buffers)
        half = np.random.default_rng(5).permutation(W2 * H2)[:W2 * H2 // 2].astype(np.uint32)
        hs2 = np.zeros((H2, W2), REC)
        fresh.node.progressive_sample(large.cam, large.win, W2, H2, hs2, 3, pixels=half)      # (... and the host list)
        assert fresh.node.last_stats["paths"] == 3 * half.size
        fresh.node.progressive_sample(large.cam, large.win, W2, H2, hs2, 3, pixels=np.zeros(0, np.uint32))      # an empty list: nothing
        assert fresh.node.last_stats["paths"] == 0
        assert _same_bytes(later.state(), want_large[0]) and _same_bytes(later.frame(), want_large[1])
        assert _same_bytes(hs, want_large[0]) and _same_bytes(hf.view(np.uint8).reshape(H2, W2, -1), want_large[1])
        assert np.array_equal(np.flatnonzero(hs2["n"].reshape(-1) == 3), np.sort(half))
        # the context's own defaults against the restatement
        _, n, mask, _, _ = _select(fresh, W2, H2, later.d_state, 128)
        assert np.array_equal(mask, pr.classes(want_large[0], 128, brt.PROG_DEFAULT_THRESHOLD, 1)) and 0 < n < W2 * H2
        assert not np.array_equal(mask, pr.classes(want_large[0], 128, brt.PROG_DEFAULT_THRESHOLD, 0))
        _check_step(oracle, small, side, 2, "behind the held call")
        assert _same_bytes(held.state(), want_small[0]) and _same_bytes(held.frame(), want_small[1])
    finally:
        fresh.close()
