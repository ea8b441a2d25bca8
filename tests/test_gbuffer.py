"""The G-buffer of a frame (brt_render_gbuffer*, DESIGN.md "G-buffer").  CPU: the exports; the host twin against the numpy restatement
(tests/gbuffer_ref.py) bit for bit and against its float64 form; properties of the rule in float64; the two encodings; refusals; the rule
alone under the sanitizers; every GPU case held to the oracle alone first.  GPU: the planes bitwise against oracle_raycast on the tree
the GPU walked, against the guide buffer and the ray queries, against the twin applied to the oracle's hits; motion, the tie to the temporal
pass, coverage, null planes, streams, refusals, and the other calls undisturbed."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import gbuffer_cases as gc
import gbuffer_ref as gr
import query_ref as qr
from bevyray_amd import _lib
from helpers import dev as _dev, guarded as _guarded, resident_callee_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_render_gbuffer_device", "brt_render_gbuffer", "brt_host_gbuffer_pixel")
F32, F64 = np.float32, np.float64
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
PLANES = brt.GBUFFER_PLANES


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _canon(a):
    """The bits of f32 values with every NaN the same NaN: which NaN an operation returns (sign, payload) is the machine's choice."""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    for name in EXPORTS:
        assert f"int32_t {name}(" in header and name in _lib.EXPORTS and f"pub fn {name}(" in rust and f" T {name}\n" in out, name
    for struct in ("brt_gbuffer", "brt_gbuffer_pixel"):
        assert f"typedef struct {struct} {{" in header and f"pub struct {struct} {{" in rust
    assert brt.GBUFFER_DTYPE.itemsize == 32 and brt.GBUFFER_DTYPE.names == ("depth_mode", "normal_format", "motion_format", "reserved")
    assert brt.GBUFFER_PIXEL_DTYPE.itemsize == 64
    for name, value in (("DEPTH_VIEW", 0), ("DEPTH_SHADER", 1), ("DEPTH_DISTANCE", 2), ("NORMAL_RGBA32F", 0), ("NORMAL_RGB10A2", 1),
                        ("MOTION_UV32F", 0), ("MOTION_UV16F", 1), ("MOTION_PIXEL", 2), ("STATUS_HIT", 1), ("STATUS_FRONT_FACE", 2),
                        ("STATUS_MOVED", 4), ("STATUS_NO_PREVIOUS", 8)):
        assert f"#define BRT_GBUFFER_{name} {value}u" in header and getattr(brt, "GBUFFER_" + name) == value
    assert _lib.load().brt_abi_version() == 6


@functools.lru_cache(maxsize=None)
def _twin_cases():
    return gc.twin_cases()


def _twin(case):
    cam, prev, win, W, H, px, py, dm, mf, t, sn, so, _ = case
    return brt.gbuffer_pixel(cam, win, W, H, px, py, brt.gbuffer(dm, int(mf != 1), mf), float(t), sn, so, prev)


def test_the_host_twin_against_the_restatement():
    """brt_host_gbuffer_pixel is gbuffer_ref.pixel (f32) bit for bit over the ~3 000 cases of gbuffer_cases.twin_cases -- every field of
    the record: depth, status, both normal forms, the motion words of the case's format, (x', y'), the direction.  NaNs compare as NaNs."""
    seen = {"hit": 0, "miss": 0, "moved": 0, "noprev": 0, "identity": 0, "special": 0, "nan_normal": 0}
    for case in _twin_cases():
        cam, prev, win, W, H, px, py, dm, mf, t, sn, so, finite = case
        got = _twin(case)
        r = gr.pixel(cam, win, W, H, px, py, dm, t, sn, so, prev)
        want = gr.record(r, dm, mf)
        for f in ("depth", "normal", "xy_prev", "direction"):
            assert np.array_equal(_canon(got[f]), _canon(want[f])), (f, got[f], want[f], case)
        assert got["status"][0] == want["status"][0], (got, want, case)
        if mf == 1:
            assert np.array_equal(got["motion"], want["motion"]), (got, want, case)
        else:
            assert np.array_equal(_canon(got["motion"].view(F32)), _canon(want["motion"].view(F32))), (got, want, case)
        assert got["normal_rgb10a2"][0] == want["normal_rgb10a2"][0], (got, want, case)      # (a NaN channel encodes as 0 on both sides)
        seen["nan_normal"] += bool(np.isnan(want["normal"]).any())
        s = int(got["status"][0])
        seen["hit" if s & gr.HIT else "miss"] += 1
        seen["moved"] += bool(s & gr.MOVED)
        seen["noprev"] += bool(s & gr.NO_PREVIOUS)
        seen["identity"] += bool(not s & gr.NO_PREVIOUS and got["xy_prev"][0, 0] == px and got["xy_prev"][0, 1] == py)
        seen["special"] += not finite
    assert min(v for k, v in seen.items() if k != "nan_normal") >= 100 and seen["nan_normal"] >= 50, seen


# The bounds of the f32 rule against its float64 restatement over the finite cases of twin_cases (positions up to 20, hits up to t = 200,
# frames up to 32768 wide, previous cameras related and unrelated).  Two kinds of case are left out: those with a special value in a field
# (there is no error to measure against a NaN), and those either precision calls NO_PREVIOUS (no position to compare; at the frame's
# edge the two may fall on different sides).  Measured maxima, as the test prints them: (x', y') 1.02e-4 of the
# frame size, motion 1.02e-4 uv (both at a point a previous camera sees at a flat angle: z small against |v|), VIEW depth 8.19e-6
# relative (a ray nearly perpendicular to fwd, dot(d, fwd) = -0.006, which a camera with a skewed `up` casts: the dot's rounding error is
# relative to its terms, not to their sum).  Asserted: four times the measured maximum rounded up to one digit.
BOUND_XY_REL, BOUND_MOTION, BOUND_DEPTH_REL = 5e-4, 5e-4, 4e-5


def test_f32_against_float64():
    """(x', y'), the uv motion and the VIEW depth of the finite cases against the float64 restatement.  (x', y') is measured relative to
    the frame size (the error of a pixel position grows with the position), the depth relative to its value."""
    worst = {"xy": 0.0, "motion": 0.0, "depth": 0.0}
    n = 0
    for case in _twin_cases():
        cam, prev, win, W, H, px, py, dm, mf, t, sn, so, finite = case
        if not finite:
            continue
        lo = gr.pixel(cam, win, W, H, px, py, gr.DEPTH_VIEW, t, sn, so, prev, T=F32)
        hi = gr.pixel(cam, win, W, H, px, py, gr.DEPTH_VIEW, t, sn, so, prev, T=F64)
        if (lo["status"] | hi["status"]) & gr.NO_PREVIOUS:
            continue             # (a position at the frame's edge may fall on either side)
        n += 1
        worst["xy"] = max(worst["xy"], abs(float(lo["xp"]) - float(hi["xp"])) / W, abs(float(lo["yp"]) - float(hi["yp"])) / H)
        worst["motion"] = max(worst["motion"], abs(float(lo["mu"]) - float(hi["mu"])), abs(float(lo["mv"]) - float(hi["mv"])))
        if hi["hit"]:
            worst["depth"] = max(worst["depth"], abs(float(lo["depth"]) - float(hi["depth"])) / abs(float(hi["depth"])))
    print(f"f32 against float64 over {n} cases: max |x' - x'_64| / size = {worst['xy']:.3g}, max |motion - motion_64| = "
          f"{worst['motion']:.3g} uv, max relative VIEW depth error = {worst['depth']:.3g}")
    assert n >= 1000
    assert worst["xy"] <= BOUND_XY_REL and worst["motion"] <= BOUND_MOTION and worst["depth"] <= BOUND_DEPTH_REL, worst


def _simple_cam(pos, target, w, h, fov=0.8):
    from helpers import uniforms
    return uniforms(w, h, 1, 1, pos=pos, target=target, fov=fov, seed=0.5)[1:]


def test_properties_in_float64():
    w, h = 64, 36
    cam, win = _simple_cam((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), w, h)
    sn = np.array([0.0, 0.0, 0.0, 1.0], F32)
    # the identity: exactly (px, py) and motion +0.0, in f32 and in float64, hit or miss, with or without an unmoved previous record
    for T in (F32, F64):
        for px, py, t in ((0, 0, np.inf), (31, 17, 4.0), (63, 35, 4.5)):
            for so in (None, sn.copy()):
                for prev in (None, cam.copy()):
                    r = gr.pixel(cam, win, w, h, px, py, 0, t, sn, so, prev, T=T)
                    assert (r["xp"], r["yp"]) == (px, py) and not r["status"] & (gr.MOVED | gr.NO_PREVIOUS)
                    assert np.array([r["mu"], r["mv"]], F64).tobytes() == np.zeros(2, F64).tobytes()      # +0.0, not -0.0
    # a sideways translation by b: a hit at view depth z moves by the parallax b / (z tan_half aspect) * W / 2 pixels, no vertical part
    ct = gr.camera_terms(cam, F64)
    b = 0.25
    prev = cam.copy()
    prev["position"][0, 0] += b                    # the camera was further right: the point appears further left, x' < px
    for px, py, t in ((31, 17, 4.0), (40, 10, 7.5), (12, 30, 2.0)):
        r = gr.pixel(cam, win, w, h, px, py, 0, t, sn, None, prev, T=F64, same=False)
        z = float(t) * float(np.dot(r["d"], gr.view_terms(ct, ct, F64)["fwd"]))
        shift = b / (z * float(ct["tan_half"]) * float(ct["aspect"])) * w / 2
        assert abs(float(r["xp"]) - (px - shift)) < 1e-9 and abs(float(r["yp"]) - py) < 1e-9, (r, shift)
        assert abs(float(r["mu"]) - shift / w) < 1e-12          # current minus previous, uv units
    # a pure rotation: sky and hit pixels move alike in the limit of far hits
    prev = gc.turned(cam, w, h, 0.05)
    prev["position"] = cam["position"]
    for px, py in ((31, 17), (10, 30)):
        sky = gr.pixel(cam, win, w, h, px, py, 0, np.inf, None, None, prev, T=F64)
        near = gr.pixel(cam, win, w, h, px, py, 0, 3.0, sn, None, prev, T=F64)
        far = gr.pixel(cam, win, w, h, px, py, 0, 1e7, sn, None, prev, T=F64)
        assert abs(float(sky["xp"]) - px) > 1.0                  # (the rotation does move the pixel)
        assert abs(float(far["xp"]) - float(sky["xp"])) < 1e-5 and abs(float(far["yp"]) - float(sky["yp"])) < 1e-5
        assert abs(float(near["xp"]) - float(sky["xp"])) < 1e-9  # (no translation: the depth plays no part)
    # DEPTH_SHADER at the centre ray is near / t, with the far rule; the miss is the test on far - 1
    c32 = gr.camera_terms(cam, F32)
    for t in (0.5, 4.0, 999.0, 1000.0, 1000.5, 1e30):
        r = gr.pixel(cam, win, w, h, 31, 17, gr.DEPTH_SHADER, t, sn, None, None)
        want = F32(-1.0) if F32(t) > c32["far"] else F32(c32["near"] / F32(t))
        assert _bits(F32(r["depth"])) == _bits(want), (t, r["depth"], want)
        twin = brt.gbuffer_pixel(cam, win, w, h, 31, 17, brt.gbuffer(gr.DEPTH_SHADER), t, sn)
        assert _bits(twin["depth"])[0] == _bits(want)
    miss = brt.gbuffer_pixel(cam, win, w, h, 31, 17, brt.gbuffer(gr.DEPTH_SHADER), np.inf)
    assert _bits(miss["depth"])[0] == _bits(F32(c32["near"] / F32(c32["far"] - F32(1.0))))
    assert brt.gbuffer_pixel(cam, win, w, h, 31, 17, brt.gbuffer(gr.DEPTH_DISTANCE), np.inf)["depth"][0] == np.inf
    assert _bits(brt.gbuffer_pixel(cam, win, w, h, 31, 17, brt.gbuffer(gr.DEPTH_VIEW), np.inf)["depth"])[0] == 0


def test_motion_fetch_lands_on_the_same_sphere(oracle):
    """uv - motion, fetched in the previous frame, is the same sphere there: oracle_raycast on both frames of every motion case."""
    for name in ("orbit", "moved"):
        case = _gpu_case(oracle, name)
        w, h = case["w"], case["h"]
        cur, prev = case["oracle_cur"], case["oracle_prev"]
        pb = prev["b"]
        pt = gr.camera_terms(case["prev_cam"], F64)
        keep = [int(p) for p in np.flatnonzero(cur["hit"]) if not case["twin"][p]["status"] & gr.NO_PREVIOUS]
        # the previous camera's ray through (x', y') itself (a fractional pixel position: the fetch is bilinear), by the oracle
        dirs = np.array([gr.direction(pt, case["win"][0]["height"], w, h, float(case["twin"][p]["xp"]), float(case["twin"][p]["yp"]), F64)
                         for p in keep], F32)
        rays = qr.make_rays(np.broadcast_to(case["prev_cam"][0]["position"], (len(keep), 3)), dirs)
        there = _hits_of_rays(oracle, pb, rays)
        same = there["hit"] & (there["sphere"] == cur["sphere"][keep])
        moved = np.array([bool(case["twin"][p]["status"] & gr.MOVED) for p in keep])
        # a point seen now may have been hidden then: the previous ray meets ANOTHER sphere before it reaches X_prev
        dist = np.array([case["twin"][p]["dist_prev"] for p in keep])
        hidden = ~same & there["hit"] & (there["t"].astype(F64) < dist * (1.0 - 1e-4))
        print(f"{name}: of {len(keep)} fetches {same.sum()} land on the same sphere, {hidden.sum()} were hidden behind another one then, "
              f"{(~same & ~hidden).sum()} neither ({moved.sum()} on moved spheres, {same[moved].sum()} of them the same)")
        assert len(keep) >= 1000 and same.sum() >= 0.9 * len(keep) and (name != "moved" or same[moved].sum() >= 10)
        # (neither: (x', y') in f32 at a silhouette may fall just beside the sphere -- a few pixels at most)
        assert (~same & ~hidden).sum() <= 0.002 * len(keep), (name, int((~same & ~hidden).sum()), len(keep))


def _sphere_with_normal(cam, win, w, h, px, py, t, m, r=1.0):
    """{centre, r^2} of the sphere whose normal at the hit of pixel (px, py) at distance t is the unit vector m: c = X - r m, with X as the
    rule computes it (f32)."""
    d = np.array(gr.direction(gr.camera_terms(cam), win[0]["height"], w, h, px, py), F32)
    x = (cam[0]["position"].astype(F32) + F32(t) * d).astype(F32)
    c = (x.astype(F64) - r * np.asarray(m, F64)).astype(F32)
    return np.array([c[0], c[1], c[2], F32(r) * F32(r)], F32)


def test_rgb10a2_against_numpy():
    """The compiled encoder (brt_host_gbuffer_pixel's packed word) against numpy: every one of the 1024 levels of every channel, reached by
    a sphere crafted so that the channel's normal component is the level's value; NaN normals (a centre at INF: the channel encodes as 0);
    a miss (a zero word); random normals all around a sphere.  The clamp branches no unit normal reaches are driven in
    tests/tools/gbuffer_twin_main.hip, which calls the encoder itself over the edge table below with these expected words."""
    _, cam, win = brt.cover_camera(16, 9, 1, 1)
    levels = np.arange(1024, dtype=np.uint32)
    centre = ((levels.astype(F64) / 1023.0) * 2.0 - 1.0)
    assert np.array_equal(gr.unorm10(centre.astype(F32)), levels)            # (the restatement on the levels' own values)
    edge = np.array([-1.0, 1.0, -1.5, 1.5, np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38, -3e38, 1e-45], F32)
    assert gr.unorm10(edge).tolist() == [0, 1023, 0, 1023, 0, 1023, 0, 512, 512, 1023, 0, 512]
    desc = brt.gbuffer(0, 1, 0)
    for k in range(3):
        reached = set()
        for lv in range(1024):
            v = float(centre[lv])
            rest = np.sqrt(max(0.0, 1.0 - v * v))
            m = np.zeros(3)
            m[k], m[(k + 1) % 3], m[(k + 2) % 3] = v, 0.6 * rest, -0.8 * rest
            px, py, t = lv % 16, lv % 9, 2.0 + (lv % 7)
            got = brt.gbuffer_pixel(cam, win, 16, 9, px, py, desc, t, _sphere_with_normal(cam, win, 16, 9, px, py, t, m))
            word = int(got["normal_rgb10a2"][0])
            assert word == int(gr.rgb10a2(got["normal"][0, :3])) and word >> 30 == 3, (k, lv, got)
            assert (word >> (10 * k)) & 1023 == lv, (k, lv, got["normal"], hex(word))
            reached.add((word >> (10 * k)) & 1023)
        assert len(reached) == 1024
    # NaN normals: a centre at INF in one coordinate gives n = (NaN, 0 or NaN, ..); every NaN channel is 0, alpha stays 3
    for k in range(3):
        sn = np.array([0.0, 0.0, 0.0, 1.0], F32)
        sn[k] = np.inf
        got = brt.gbuffer_pixel(cam, win, 16, 9, 3, 4, desc, 5.0, sn)
        n = got["normal"][0, :3]
        assert np.isnan(n[k])
        word = int(got["normal_rgb10a2"][0])
        assert word == int(gr.rgb10a2(n)) and word >> 30 == 3 and (word >> (10 * k)) & 1023 == 0, (n, hex(word))
    got = brt.gbuffer_pixel(cam, win, 16, 9, 3, 4, desc, 5.0, np.array([np.nan, np.nan, np.nan, 1.0], F32))
    assert int(got["normal_rgb10a2"][0]) == 3 << 30
    # random normals all around a sphere, word for word
    rng = np.random.default_rng(3)
    for i in range(500):
        px, py = int(rng.integers(0, 16)), int(rng.integers(0, 9))
        t = F32(rng.uniform(0.5, 30.0))
        m = rng.normal(size=3)
        got = brt.gbuffer_pixel(cam, win, 16, 9, px, py, desc, t, _sphere_with_normal(cam, win, 16, 9, px, py, t, m / np.linalg.norm(m), 0.7))
        assert got["normal_rgb10a2"][0] == gr.rgb10a2(got["normal"][0, :3])
    assert brt.gbuffer_pixel(cam, win, 16, 9, 0, 0, desc, np.inf)["normal_rgb10a2"][0] == 0


def test_rg16f_against_numpy_float16():
    """The twin's f32 -> f16 conversion against numpy.float16 bitwise: the motion a sideways camera move of chosen size gives spans
    ordinary values, values that round to f16 subnormals and to zero; the conversion itself is then driven over every f16 boundary by
    gbuffer_twin_main (every f32 whose low 13 bits are 0x0fff, 0x1000 or 0x1001: ties and their neighbours)."""
    w, h = 64, 36
    cam, win = _simple_cam((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), w, h)
    sn = np.array([0.0, 0.0, 0.0, 1.0], F32)
    classes = {"normal": 0, "subnormal": 0, "zero": 0}
    for k in range(400):
        b = 10.0 ** (-9 + k * 0.025)                     # 1e-9 .. 10: motion from far below the smallest f16 subnormal upwards
        prev = cam.copy()
        prev["position"][0, 0] += F32(b)
        prev["position"][0, 1] -= F32(b * 0.37)
        for px, py, t in ((31, 17, 4.0), (3, 30, 6.0)):
            uv = brt.gbuffer_pixel(cam, win, w, h, px, py, brt.gbuffer(0, 0, 0), t, sn, None, prev)
            pk = brt.gbuffer_pixel(cam, win, w, h, px, py, brt.gbuffer(0, 0, 1), t, sn, None, prev)
            if uv["status"][0] & gr.NO_PREVIOUS:
                continue
            m = uv["motion"].view(F32)[0]
            assert pk["motion"][0, 0] == gr.f16_pair(m[0], m[1]) and pk["motion"][0, 1] == 0, (m, pk["motion"])
            a = abs(float(np.float16(m[0])))
            classes["zero" if a == 0 else "subnormal" if a < 6.104e-5 else "normal"] += 1
    assert min(classes.values()) >= 20, classes


def test_rejections_that_need_no_device():
    lib = _lib.load()
    _, cam, win = brt.cover_camera(16, 9, 1, 1)
    desc = brt.gbuffer()
    out = np.zeros(1, brt.GBUFFER_PIXEL_DTYPE)
    sn = np.array([0, 0, 0, 1], F32)

    def call(cam_=cam, win_=win, w=16, h=9, px=0, py=0, desc_=desc, prev=None, t=1.0, sn_=sn, out_=out):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.brt_host_gbuffer_pixel(p(cam_), p(win_), w, h, px, py, p(desc_), p(prev), C.c_float(t), p(sn_), None, p(out_))

    assert call() == 0
    for kw, word in ((dict(cam_=None), b"camera"), (dict(win_=None), b"window"), (dict(desc_=None), b"gbuffer is null"),
                     (dict(out_=None), b"out_pixel64"), (dict(px=16), b"pixel outside"), (dict(py=9), b"pixel outside"),
                     (dict(w=0), b"width/height"), (dict(h=32769), b"width/height"), (dict(sn_=None), b"sphere_new4")):
        assert call(**kw) == INVALID, kw
        assert word in lib.brt_last_error(None), (kw, lib.brt_last_error(None))
    assert call(sn_=None, t=np.inf) == 0                   # (a miss needs no sphere)
    for field, bad, word in (("reserved", 1, b"reserved"), ("depth_mode", 3, b"depth_mode"), ("normal_format", 2, b"normal_format"),
                             ("motion_format", 3, b"motion_format")):
        d = brt.gbuffer()
        if field == "reserved":
            d["reserved"][0, 4] = bad
        else:
            d[field] = bad
        assert call(desc_=d) == INVALID and word in lib.brt_last_error(None), field
    ortho = cam.copy()
    ortho["projection"] = 1
    assert call(cam_=ortho) == UNSUPPORTED and lib.brt_last_error(None).startswith(b"camera.projection_type")
    assert call(prev=ortho) == UNSUPPORTED and lib.brt_last_error(None).startswith(b"prev_camera.projection_type")
    planes = [None] * 5
    assert lib.brt_render_gbuffer(None, cam.ctypes.data, win.ctypes.data, 16, 9, desc.ctypes.data, None, None, None, *planes, None) == INVALID
    assert lib.brt_render_gbuffer_device(None, cam.ctypes.data, win.ctypes.data, 16, 9, desc.ctypes.data, None, None, None, *planes,
                                         None, 0, None) == INVALID
    assert b"null" in lib.brt_last_error(None)


def test_the_rule_alone_under_the_sanitizers(tmp_path):
    """tests/tools/gbuffer_twin_main.hip: the rule alone in a program of its own, built with the address and undefined-behaviour
    sanitizers and run on the CPU over special values read from odd addresses; it also holds the f16 conversion to the compiler's own
    over every rounding boundary."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "gbuffer_twin_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "bevyray_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "gbuffer_twin_main.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr


# ---- the GPU cases, on the oracle alone -------------------------------------------------------------------------------------------

def _oracle_hits(oracle, b, cam, w, h, models=None):
    """The first hits of the pixel-centre rays of a w x h frame by the oracle on b's tree -> dict of (w * h) arrays: hit, t, n, material,
    front, sphere (the caller's index: the sphere of that material that reproduces t through oracle_hit_sphere, nearest first)."""
    return _hits_of_rays(oracle, b, qr.pixel_rays(oracle, cam, w, h))


def _hits_of_rays(oracle, b, rays):
    want, _ = qr.expected(oracle, b.models, b.bvh, rays)
    hit = (want["status"] & brt.QUERY_STATUS_HIT) != 0
    sphere = np.full(len(rays), brt.QUERY_NONE, np.uint32)
    m = b.models
    for i in np.flatnonzero(hit):
        x = rays["origin"][i].astype(F64) + F64(want["t"][i]) * rays["direction"][i].astype(F64)
        err = np.abs(np.linalg.norm(m["position"].astype(F64) - x, axis=1) - m["radius"].astype(F64))
        err[m["material_id"] != want["material"][i]] = np.inf
        sphere[i] = int(np.argmin(err))
    return dict(b=b, rays=rays, hit=hit, t=want["t"], n=want["normal"], material=want["material"],
                front=(want["status"] & brt.QUERY_STATUS_FRONT_FACE) != 0, sphere=sphere, want=want)


def _sphere4(models, idx):
    m = models[idx]
    return np.array([m["position"][0], m["position"][1], m["position"][2], F32(m["radius"]) * F32(m["radius"])], F32)


def _twin_planes(cam, win, w, h, hits, models, prev_cam=None, prev_models=None):
    """`pixel` (f32 restatement == the host twin, test_the_host_twin_against_the_restatement) on the oracle's hits -> a list of dicts."""
    out = []
    for p in range(w * h):
        py, px = divmod(p, w)
        if hits["hit"][p]:
            s = int(hits["sphere"][p])
            sn = _sphere4(models, s)
            so = None if prev_models is None else _sphere4(prev_models, s)
            out.append(gr.pixel(cam, win, w, h, px, py, 0, hits["t"][p], sn, so, prev_cam))
        else:
            out.append(gr.pixel(cam, win, w, h, px, py, 0, np.inf, None, None, prev_cam))
    return out


GPU_CASES = {
    # name: (scene, view, w, h, previous camera, previous models, coverage)
    "static": ("cover", "cover", 96, 54, None, False, None),
    "orbit": ("cover", "cover", 96, 54, "orbit", False, None),
    "moved": ("cover", "cover", 96, 54, "orbit", True, None),
    "turned": ("cover", "cover", 96, 54, "turned", False, None),
    "graze": ("cover", "graze", 33, 31, "orbit", False, None),
    "coverage": ("cover", "cover", 96, 54, "orbit", False, "blocks"),
}


@functools.lru_cache(maxsize=None)
def _gpu_case_cached(name):
    import oracle_loader
    oracle = oracle_loader.load()
    scene, view, w, h, prev_kind, moved, cov = GPU_CASES[name]
    b = gc.scene(scene)
    lvl, cam, win = gc.view(view, w, h)
    prev_cam = None if prev_kind is None else gc.orbit(cam, 0.04, 0.1) if prev_kind == "orbit" else gc.turned(cam, w, h, 0.12)
    prev_models, picked = (gc.moved_models(b.models, (0.0, 0.5, 0.0)) if moved else (None, None))
    cur = _oracle_hits(oracle, b, cam, w, h)
    case = dict(name=name, b=b, lvl=lvl, cam=cam, win=win, w=w, h=h, prev_cam=prev_cam, prev_models=prev_models, picked=picked,
                cov=None if cov is None else gc.coverage_frame(w, h, cov), oracle_cur=cur)
    case["twin"] = _twin_planes(cam, win, w, h, cur, b.models, prev_cam, prev_models)
    if prev_cam is not None:
        pb = b if prev_models is None else brt.Buffers(prev_models, b.materials, brt.build_bvh(prev_models))
        case["oracle_prev"] = _oracle_hits(oracle, pb, prev_cam, w, h)
    return case


def _gpu_case(oracle, name):
    return _gpu_case_cached(name)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_are_not_vacuous_on_the_oracle(oracle, name):
    case = _gpu_case(oracle, name)
    cur, w, h = case["oracle_cur"], case["w"], case["h"]
    status = np.array([r["status"] for r in case["twin"]])
    share = cur["hit"].mean()
    print(f"{name}: hit share {share:.3f}, moved {np.count_nonzero(status & gr.MOVED)}, no-previous {np.count_nonzero(status & gr.NO_PREVIOUS)}, "
          f"front {np.count_nonzero(cur['hit'] & cur['front'])}, back {np.count_nonzero(cur['hit'] & ~cur['front'])}")
    assert 0.10 < share < 0.95, share
    assert (cur["hit"] & cur["front"]).any()
    if name == "graze":
        # A back-face hit.  A camera INSIDE a sphere gives none: the reference's hit_sphere returns the near root alone, which lies
        # behind such a camera (asserted here on the glass sphere of the cover scene); a grazing ray whose dot(d, n) rounds to >= 0 does.
        assert (cur["hit"] & ~cur["front"]).sum() >= 1
        _, icam, _ = gc.view("inside", w, h)
        inside = _oracle_hits(oracle, case["b"], icam, w, h)
        glass = int(np.flatnonzero((case["b"].models["position"] == (0.0, 1.0, 0.0)).all(axis=1))[0])
        assert inside["hit"].any() and inside["front"][inside["hit"]].all() and not (inside["sphere"][inside["hit"]] == glass).any()
    if name == "moved":
        assert np.count_nonzero(status & gr.MOVED) >= 10
        moved_spheres = set(cur["sphere"][(status & gr.MOVED) != 0].tolist())
        assert moved_spheres <= set(case["picked"].tolist()) and len(moved_spheres) >= 2
    else:
        assert not (status & gr.MOVED).any()
    if name == "turned":
        assert np.count_nonzero(status & gr.NO_PREVIOUS) >= 50 and np.count_nonzero(~(status & gr.NO_PREVIOUS).astype(bool)) >= 50
        assert (status[~cur["hit"]] & gr.NO_PREVIOUS).any() and (status[cur["hit"]] & gr.NO_PREVIOUS).any()      # sky and hit pixels
    if name == "static":
        assert not (status & gr.NO_PREVIOUS).any()
        assert all(r["xp"] == p % w and r["yp"] == p // w for p, r in enumerate(case["twin"]))
    if case["cov"] is not None:
        covered = _bits(case["cov"][..., 3]) == 0
        assert covered[0, 0] == False and _bits(case["cov"][..., 3])[0, 0] == 0x80000000      # noqa: E712  (-0.0 is not covered)
        waves = covered.reshape(-1)          # a wave: 4 rows x 16 columns of a 16 x 16 tile
        yy, xx = np.mgrid[0:h, 0:w]
        wave_id = ((yy // 4) * ((w + 15) // 16) + xx // 16).reshape(-1)
        full = [waves[wave_id == k].all() for k in np.unique(wave_id)]
        mixed = [waves[wave_id == k].any() and not waves[wave_id == k].all() for k in np.unique(wave_id)]
        assert sum(full) >= 5 and sum(mixed) >= 5 and not all(full)
        # covered and uncovered pixels on both sides of a wave boundary (rows 3 | 4 of a tile column)
        assert (covered[3, :] & ~covered[4, :]).any() and (~covered[3, :] & covered[4, :]).any()
        assert (covered & cur["hit"].reshape(h, w)).any() and (~covered & cur["hit"].reshape(h, w)).any()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

GUARD = 256
FILL = 0xCD


def _plane_bytes(desc, plane, n):
    return n * {"depth": 4, "normal": 16 if desc["normal_format"][0] == 0 else 4, "motion": 4 if desc["motion_format"][0] == 1 else 8,
                "ids": 16, "albedo": 16}[plane]


def _device(plugin, cam, win, w, h, desc, planes=PLANES, prev_cam=None, prev_models=None, cov=None, stream=None, bufs=None):
    """brt_render_gbuffer_device into guarded buffers filled with FILL -> {plane: host array}; the guard rows are checked."""
    import torch
    n = w * h
    own = bufs is None
    if own:
        bufs = {k: _guarded(_plane_bytes(desc, k, n), GUARD, FILL) for k in planes}
    d_prev = None if prev_models is None else _dev(prev_models)
    d_cov = None if cov is None else _dev(cov)
    st = plugin.node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev_cam,
                                           d_prev_models=0 if d_prev is None else d_prev.data_ptr(),
                                           d_coverage=0 if d_cov is None else d_cov.data_ptr(), stream=stream,
                                           **{"d_" + k: bufs[k].data_ptr() for k in planes})
    torch.cuda.synchronize()
    out = {}
    for k in planes:
        raw = bufs[k].cpu().numpy()
        size = _plane_bytes(desc, k, n)
        assert (raw[size:] == FILL).all(), f"plane {k}: the guard behind it was written"
        shape = brt.gbuffer_plane(desc, k, w, h)
        out[k] = raw[:size].view(shape.dtype).reshape(shape.shape).copy()
    return out, st


def _expected_planes(case, desc, b_twin=None, hits=None):
    """The planes of a case in the formats of `desc` from the oracle's hits and the rule."""
    w, h = case["w"], case["h"]
    hits = case["oracle_cur"] if hits is None else hits
    dm, nf, mf = (int(desc[k][0]) for k in ("depth_mode", "normal_format", "motion_format"))
    twin = case["twin"]
    models, mats = case["b"].models, case["b"].materials
    n = w * h
    depth = np.zeros(n, F32)
    for p in range(n):
        py, px = divmod(p, w)
        if dm == 0:
            depth[p] = twin[p]["depth"]
        else:
            r = twin[p]
            sn = _sphere4(models, int(hits["sphere"][p])) if hits["hit"][p] else None
            depth[p] = brt.gbuffer_pixel(case["cam"], case["win"], w, h, px, py, brt.gbuffer(dm), hits["t"][p] if hits["hit"][p] else np.inf, sn)["depth"][0]
    nrm = np.array([r["n"] for r in twin], F32)
    hit = hits["hit"]
    out = {"depth": depth.reshape(h, w)}
    if nf == 0:
        out["normal"] = np.concatenate([nrm, hit[:, None].astype(F32)], axis=1).reshape(h, w, 4)
    else:
        out["normal"] = gr.rgb10a2(nrm, hit).reshape(h, w)
    mu, mv = (np.array([r[k] for r in twin], F32) for k in ("mu", "mv"))
    xp, yp = (np.array([r[k] for r in twin], F32) for k in ("xp", "yp"))
    out["motion"] = (np.stack([mu, mv], 1).reshape(h, w, 2) if mf == 0 else gr.f16_pair(mu, mv).reshape(h, w) if mf == 1
                     else np.stack([xp, yp], 1).reshape(h, w, 2))
    ids = np.zeros(n, brt.GBUFFER_IDS_DTYPE)
    ids["sphere"] = hits["sphere"]
    ids["material"] = np.where(hit, hits["material"], brt.QUERY_NONE)
    ids["status"] = [r["status"] for r in twin]
    out["ids"] = ids.reshape(h, w)
    alb = np.zeros((n, 4), F32)
    mm = mats[hits["material"][hit]]
    alb[hit, :3] = mm["base_color"]
    alb[hit, 3] = mm["metallic"]
    out["albedo"] = alb.reshape(h, w, 4)
    return out


def _assert_planes(got, want, what, mask=None):
    for k in got:
        g, w_ = got[k], want[k]
        gb = g.view(np.uint32).reshape(g.shape[0], g.shape[1], -1)
        wb = np.ascontiguousarray(w_).view(np.uint32).reshape(g.shape[0], g.shape[1], -1)
        if k in ("depth", "motion", "normal") and g.dtype == F32:
            gb, wb = _canon(g).reshape(gb.shape), _canon(np.ascontiguousarray(w_)).reshape(gb.shape)
        bad = (gb != wb).any(axis=2)
        if mask is not None:
            bad &= mask
        assert not bad.any(), f"{what}: plane {k}: {bad.sum()} pixels differ, first {np.argwhere(bad)[:3].tolist()}: got {g[bad][:2]}, want {np.asarray(w_)[bad][:2]}"


DESCS = [(0, 0, 0), (1, 1, 1), (2, 0, 2)]


def _upload(plugin, case, tree="caller"):
    """The case's scene resident under the caller's tree (-> its Buffers) or the callee's (-> Buffers with the CPU twin of that tree)."""
    b = case["b"]
    if tree == "caller":
        plugin.node.write_buffers(b)
        return b
    twin, _, _ = resident_callee_tree(plugin, b, case["lvl"], case["cam"], case["win"], case["w"], case["h"])
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["static", "orbit", "moved", "turned", "graze"])
def test_planes_against_the_oracle_and_the_twin(plugin, oracle, name):
    """Every plane in all three depth modes, both normal formats and all three motion formats, bitwise: the hit planes (t as DISTANCE
    depth, normal, sphere, material, FRONT_FACE, albedo) are the oracle's raycast, the derived ones the rule on the oracle's hits.  Both
    entry points give the same bytes, and the counts are the oracle's."""
    case = _gpu_case(oracle, name)
    _upload(plugin, case)
    w, h, cam, win = case["w"], case["h"], case["cam"], case["win"]
    for dm, nf, mf in DESCS:
        desc = brt.gbuffer(dm, nf, mf)
        want = _expected_planes(case, desc)
        got, st = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"], prev_models=case["prev_models"])
        _assert_planes(got, want, f"{name} {dm}{nf}{mf} device")
        status = want["ids"]["status"]
        assert (st["cast"], st["hits"], st["covered"]) == (w * h, int(case["oracle_cur"]["hit"].sum()), 0)
        assert (st["moved"], st["no_previous"]) == (int(np.count_nonzero(status & gr.MOVED)), int(np.count_nonzero(status & gr.NO_PREVIOUS)))
        host = plugin.node.render_gbuffer(cam, win, w, h, desc, prev_camera=case["prev_cam"], prev_models=case["prev_models"])
        for k in PLANES:
            assert host[k].tobytes() == got[k].tobytes(), f"{name} {dm}{nf}{mf}: host and device entry points differ in {k}"
    if name == "static":
        m = _device(plugin, cam, win, w, h, brt.gbuffer(0, 0, 0))[0]
        assert not m["motion"].view(np.uint32).any() and not (m["ids"]["status"] & (gr.MOVED | gr.NO_PREVIOUS)).any()
        m2 = _device(plugin, cam, win, w, h, brt.gbuffer(0, 0, 0), prev_cam=cam.copy(), prev_models=case["b"].models)[0]
        assert all(m2[k].tobytes() == m[k].tobytes() for k in PLANES)


SCENES = [("cover", "caller", 96, 54), ("cover", "callee", 96, 54), ("rtiow", "caller", 96, 54), ("stress", "callee", 96, 54),
          ("big", "caller", 33, 31), ("cover", "caller", 1, 1), ("cover", "caller", 1, 7), ("cover", "caller", 7, 1),
          ("cover", "callee", 17, 9), ("cover", "caller", 33, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,tree,w,h", SCENES)
def test_hit_planes_on_every_scene_and_size(plugin, oracle, scene, tree, w, h):
    """The hit planes on the cover scene in both trees, RTIOW final, the stress grid with the hot order live (the sphere renumbering
    asserted) and a 16 383-sphere scene (32-bit descriptors), at the edge sizes: against oracle_raycast on the tree the GPU walked,
    against brt_debug_denoise_guides and against brt_query_rays on brt_host_pixel_ray's rays."""
    b = gc.scene(scene)
    lvl, cam, win = gc.view(scene, w, h)
    if tree == "callee":
        twin, win, st = resident_callee_tree(plugin, b, lvl, cam, win, w, h, seeds=(0.5, 0.25, 0.75) if scene == "stress" else ())
        if scene == "stress":
            assert st["scene_in_lds"] == 2 and st["hot_records"] > 0        # top of the tree in LDS, spheres renumbered
    else:
        plugin.node.write_buffers(b)
        twin = b
    if scene == "big":
        # the path, as tests/test_desc32.py asserts it: past 16 382 spheres the tree needs 32-bit descriptors, which are walked from
        # global memory with no hot order (k_gbuffer<false, ...> is the instantiation launch_gbuffer picks for such a scene)
        plugin.node.run(lvl, cam, win, w, h)
        st = plugin.node.last_stats
        assert len(b.models) == 16383 and st["scene_in_lds"] == 0 and st["hot_records"] == 0, st
    desc = brt.gbuffer(brt.GBUFFER_DEPTH_DISTANCE, 0, 2)
    got, st = _device(plugin, cam, win, w, h, desc)
    rays = qr.pixel_rays(oracle, cam, w, h)
    want, _ = qr.expected(oracle, twin.models, twin.bvh, rays)
    hit = (want["status"] & brt.QUERY_STATUS_HIT) != 0
    ids = got["ids"].reshape(-1)
    assert np.array_equal(_bits(got["depth"]).reshape(-1), _bits(want["t"]))
    assert np.array_equal(_bits(got["normal"][..., :3]).reshape(-1, 3), _bits(want["normal"]))
    assert np.array_equal(got["normal"][..., 3].reshape(-1), hit.astype(F32))
    assert np.array_equal(ids["material"], want["material"])
    assert np.array_equal(ids["status"] & 3, want["status"] & 3)
    assert not ids["reserved"].any()
    # the sphere: the caller's index, which reproduces t and carries the material (the oracle names no sphere)
    as_hits = np.zeros(len(rays), brt.HIT_DTYPE)
    as_hits["t"], as_hits["sphere"], as_hits["material"], as_hits["status"] = want["t"], ids["sphere"], ids["material"], ids["status"] & 3
    qr.check_spheres(oracle, b.models, rays, as_hits)
    alb = got["albedo"].reshape(-1, 4)
    mm = b.materials[want["material"][hit]]
    assert np.array_equal(_bits(alb[hit, :3]), _bits(mm["base_color"])) and np.array_equal(_bits(alb[hit, 3]), _bits(mm["metallic"]))
    assert not _bits(alb[~hit]).any()
    assert (st["cast"], st["hits"]) == (w * h, int(hit.sum()))
    # ... the existing exports
    q = plugin.node.query_rays(rays)
    assert np.array_equal(_bits(q["t"]), _bits(got["depth"]).reshape(-1)) and np.array_equal(q["sphere"], ids["sphere"])
    assert np.array_equal(q["material"], ids["material"]) and np.array_equal(_bits(q["normal"]), _bits(got["normal"][..., :3]).reshape(-1, 3))
    for px, py in {(0, 0), (w - 1, h - 1), (w // 2, h // 2)}:
        r = brt.pixel_ray(cam, win, w, h, px, py)
        assert r["direction"].tobytes() == rays[py * w + px]["direction"].tobytes()
    guides = np.zeros((h, w, 8), F32)
    _lib.check(plugin._lib.brt_debug_denoise_guides(plugin._ctx, cam.ctypes.data, win.ctypes.data, w, h, guides.ctypes.data), plugin._ctx)
    g = guides.reshape(-1, 8)
    assert np.array_equal(_bits(g[:, 3]), _bits(got["depth"]).reshape(-1))
    assert np.array_equal(_bits(g[:, :3]), _bits(got["normal"][..., :3]).reshape(-1, 3))
    assert np.array_equal(_bits(g[:, 7]), ids["material"])


@pytest.mark.gpu
def test_the_tie_to_the_temporal_pass(plugin, oracle):
    """After two BRT_FLAG_TEMPORAL frames of an orbit with a moved sphere, brt_debug_temporal_state's (x', y') on the hit pixels it
    kept equal motion format 2 bitwise; where it says NaN for a hit pixel, the position was outside the frame: NO_PREVIOUS."""
    import torch
    case = _gpu_case(oracle, "moved")
    w, h, b = case["w"], case["h"], case["b"]
    lvl, cam, win = case["lvl"], case["cam"], case["win"]
    prev_b = brt.Buffers(case["prev_models"], b.materials, None)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    _lib.check(plugin._lib.brt_reset_temporal(plugin._ctx), plugin._ctx)
    for bufs, c in ((prev_b, case["prev_cam"]), (brt.Buffers(b.models, b.materials, None), cam)):
        plugin.node.write_buffers(bufs)
        plugin.node.render_device(lvl, c, win, w, h, frame.data_ptr(), flags=brt.FLAG_TEMPORAL)
    state = np.zeros((h, w, 8), F32)
    _lib.check(plugin._lib.brt_debug_temporal_state(plugin._ctx, w, h, state.ctypes.data), plugin._ctx)
    got, _ = _device(plugin, cam, win, w, h, brt.gbuffer(2, 0, 2), prev_cam=case["prev_cam"], prev_models=case["prev_models"])
    xy = state[..., 6:8]
    hit = (got["ids"]["status"] & gr.HIT) != 0
    noprev = (got["ids"]["status"] & gr.NO_PREVIOUS) != 0
    kept = hit & ~np.isnan(xy[..., 0])
    assert kept.sum() >= 500 and (got["ids"]["status"][kept] & gr.MOVED).any()
    assert np.array_equal(_bits(xy[kept]), _bits(got["motion"][kept]))
    assert not noprev[kept].any()
    # the temporal pass says NaN for a position outside the frame AND for one whose taps it all rejected; the first kind is NO_PREVIOUS:
    # every NO_PREVIOUS hit pixel is a NaN there
    assert (hit & noprev).sum() >= 20 and np.isnan(xy[..., 0])[hit & noprev].all()
    _lib.check(plugin._lib.brt_reset_temporal(plugin._ctx), plugin._ctx)


@pytest.mark.gpu
def test_coverage(plugin, oracle):
    """With a coverage frame bound, covered pixels keep the sentinel in every plane, the others equal the call without coverage; a fully
    covered frame writes nothing; the host entry point keeps the caller's values."""
    case = _gpu_case(oracle, "coverage")
    _upload(plugin, case)
    w, h, cam, win = case["w"], case["h"], case["cam"], case["win"]
    covered = _bits(case["cov"][..., 3]) == 0
    for dm, nf, mf in DESCS:
        desc = brt.gbuffer(dm, nf, mf)
        free, _ = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"])
        got, st = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"], cov=case["cov"])
        assert (st["cast"], st["covered"]) == (int((~covered).sum()), int(covered.sum()))
        for k in PLANES:
            gb = got[k].view(np.uint8).reshape(h, w, -1)
            assert (gb[covered] == FILL).all(), f"plane {k}: a covered pixel was written"
            assert np.array_equal(gb[~covered], free[k].view(np.uint8).reshape(h, w, -1)[~covered]), k
        none, st = _device(plugin, cam, win, w, h, desc, cov=gc.coverage_frame(w, h, "all"))
        assert st["cast"] == 0 and st["covered"] == w * h
        assert all((none[k].view(np.uint8) == FILL).all() for k in PLANES)
        into = {k: brt.gbuffer_plane(desc, k, w, h) for k in PLANES}
        for k in PLANES:
            into[k].view(np.uint8)[...] = 0x5A
        host = plugin.node.render_gbuffer(cam, win, w, h, desc, prev_camera=case["prev_cam"], coverage=case["cov"], into=into)
        for k in PLANES:
            hb = host[k].view(np.uint8).reshape(h, w, -1)
            assert (hb[covered] == 0x5A).all() and np.array_equal(hb[~covered], free[k].view(np.uint8).reshape(h, w, -1)[~covered]), k


@pytest.mark.gpu
def test_null_planes_and_refusals(plugin, oracle):
    case = _gpu_case(oracle, "orbit")
    _upload(plugin, case)
    w, h, cam, win = case["w"], case["h"], case["cam"], case["win"]
    desc = brt.gbuffer(0, 1, 1)
    full, _ = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"])
    # each plane alone, and none
    for k in PLANES:
        one, _ = _device(plugin, cam, win, w, h, desc, planes=(k,), prev_cam=case["prev_cam"])
        assert one[k].tobytes() == full[k].tobytes(), k
    st = plugin.node.render_gbuffer_device(cam, win, w, h, desc)
    assert st["cast"] == 0
    assert plugin.node.render_gbuffer(cam, win, w, h, desc, planes=()) == {}
    n = w * h
    # the scene-dependent refusals, each followed by a correct call
    node = plugin.node
    d = _guarded(n * 4, GUARD, FILL)

    def refused(code, word, **kw):
        args = dict(camera=cam, window=win, width=w, height=h, desc=desc, d_depth=d.data_ptr())
        args.update(kw)
        with pytest.raises(brt.BrtError) as e:
            node.render_gbuffer_device(args.pop("camera"), args.pop("window"), args.pop("width"), args.pop("height"), args.pop("desc"), **args)
        assert e.value.code == code and word in e.value.text, e.value
        ok, _ = _device(plugin, cam, win, w, h, desc, planes=("depth",))
        assert ok["depth"].tobytes() == full["depth"].tobytes()

    bad = brt.gbuffer(0, 1, 1)
    bad["reserved"][0, 2] = 7
    refused(INVALID, "reserved", desc=bad)
    refused(INVALID, "depth_mode", desc=brt.gbuffer(9, 0, 0))
    refused(INVALID, "width/height", width=0)
    refused(INVALID, "width/height", height=40000)
    refused(INVALID, "BRT_FLAG_CALLER_STREAM only", flags=brt.FLAG_DENOISE)
    refused(INVALID, "16-byte aligned", d_depth=d.data_ptr() + 4)
    ortho = cam.copy()
    ortho["projection"] = 1
    refused(UNSUPPORTED, "camera.projection_type", camera=ortho)
    refused(UNSUPPORTED, "prev_camera.projection_type", prev_camera=ortho)
    many = cam.copy()
    many["bounce_count"] = 0x7fffffff                       # (the rule reads no count of the previous camera: no refusal in its name)
    ok, _ = _device(plugin, cam, win, w, h, desc, prev_cam=many)
    assert all(ok[k].tobytes() == _device(plugin, cam, win, w, h, desc, prev_cam=cam.copy())[0][k].tobytes() for k in PLANES)
    plugin.set_policy(brt.POLICY_MINMAX_SELECT)
    try:
        refused_code = None
        with pytest.raises(brt.BrtError) as e:
            node.render_gbuffer_device(cam, win, w, h, desc, d_depth=d.data_ptr())
        refused_code = e.value.code
    finally:
        plugin.set_policy(0)
    assert refused_code == UNSUPPORTED
    fresh = brt.RaytracePlugin([0])
    try:
        with pytest.raises(brt.BrtError) as e:
            fresh.node.render_gbuffer_device(cam, win, w, h, desc, d_depth=d.data_ptr())
        assert e.value.code == NO_SCENE
    finally:
        fresh.close()
    ok, _ = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"])
    assert all(ok[k].tobytes() == full[k].tobytes() for k in PLANES)


def _fresh_bufs(desc, n, planes=PLANES):
    return {k: _guarded(_plane_bytes(desc, k, n), GUARD, FILL) for k in planes}


def _enqueue(plugin, cam, win, w, h, desc, bufs, prev_cam=None, stream=None):
    """brt_render_gbuffer_device into `bufs` on a caller's stream: nothing is waited for."""
    return plugin.node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev_cam, stream=stream,
                                             **{"d_" + k: t.data_ptr() for k, t in bufs.items()})


def _read(bufs, desc, w, h):
    out = {}
    for k, t in bufs.items():
        raw, size = t.cpu().numpy(), _plane_bytes(desc, k, w * h)
        assert (raw[size:] == FILL).all(), f"plane {k}: the guard behind it was written"
        shape = brt.gbuffer_plane(desc, k, w, h)
        out[k] = raw[:size].view(shape.dtype).reshape(shape.shape).copy()
    return out


def _same_planes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in PLANES)


@pytest.mark.gpu
def test_two_caller_streams_with_an_upload_in_between(plugin, oracle):
    """A G-buffer call held on stream A, an upload of another scene, a G-buffer call on stream B: A holds the planes of the scene that was
    resident when it was called (the upload waited for it), B those of the new scene.  Nothing is synchronised before the end."""
    import torch
    from test_caller_streams import Streams
    case = _gpu_case(oracle, "orbit")
    w, h, cam, win, prev = case["w"], case["h"], case["cam"], case["win"], case["prev_cam"]
    desc = brt.gbuffer(0, 1, 1)
    other = gc.scene("mirrored")
    plugin.node.write_buffers(other)
    want_other, _ = _device(plugin, cam, win, w, h, desc, prev_cam=prev)
    _upload(plugin, case)
    want_first, _ = _device(plugin, cam, win, w, h, desc, prev_cam=prev)
    assert not any(want_first[k].tobytes() == want_other[k].tobytes() for k in PLANES)      # (the two scenes differ in every plane)
    streams = Streams()
    bufs_a, bufs_b = _fresh_bufs(desc, w * h), _fresh_bufs(desc, w * h)
    torch.cuda.synchronize()
    held = streams.hold(streams.a)
    st = _enqueue(plugin, cam, win, w, h, desc, bufs_a, prev, stream=streams.a.cuda_stream)
    assert st["cast"] == 0 and not held.query()                # (a caller's stream is not waited for: nothing counted, the hold still on)
    plugin.node.write_buffers(other)                           # (waits for the held call: uploads wait for the context's lists)
    _enqueue(plugin, cam, win, w, h, desc, bufs_b, prev, stream=streams.b.cuda_stream)
    torch.cuda.synchronize()
    assert _same_planes(_read(bufs_a, desc, w, h), want_first)
    assert _same_planes(_read(bufs_b, desc, w, h), want_other)


@pytest.mark.gpu
def test_a_held_call_with_its_buffers_reused_behind_it(plugin, oracle):
    """Call 1 is held on stream A; call 2, of another camera, goes to stream B into THE SAME buffers, and call 3 to B into fresh ones.  The
    context runs its G-buffer calls one behind the other whatever streams they come on, so the shared buffers end with call 2's planes:
    had call 2 run while A was held, call 1 would have overwritten them."""
    import torch
    from test_caller_streams import Streams
    case = _gpu_case(oracle, "orbit")
    _upload(plugin, case)
    w, h, cam, win, prev = case["w"], case["h"], case["cam"], case["win"], case["prev_cam"]
    desc = brt.gbuffer(2, 0, 2)
    want1, _ = _device(plugin, cam, win, w, h, desc, prev_cam=prev)
    want2, _ = _device(plugin, prev, win, w, h, desc, prev_cam=cam)
    assert not any(want1[k].tobytes() == want2[k].tobytes() for k in PLANES)
    streams = Streams()
    shared, fresh = _fresh_bufs(desc, w * h), _fresh_bufs(desc, w * h)
    torch.cuda.synchronize()
    held = streams.hold(streams.a)
    _enqueue(plugin, cam, win, w, h, desc, shared, prev, stream=streams.a.cuda_stream)
    _enqueue(plugin, prev, win, w, h, desc, shared, cam, stream=streams.b.cuda_stream)
    _enqueue(plugin, cam, win, w, h, desc, fresh, prev, stream=streams.b.cuda_stream)
    assert not held.query()                                    # (all three were enqueued while call 1 was held)
    torch.cuda.synchronize()
    assert _same_planes(_read(shared, desc, w, h), want2)
    assert _same_planes(_read(fresh, desc, w, h), want1)


@pytest.mark.gpu
def test_other_calls_are_undisturbed(plugin, oracle):
    """A Pure frame, a temporal sequence, a denoised frame and brt_debug_tile_order with G-buffer calls in between are, byte for byte,
    what they are without."""
    import torch
    case = _gpu_case(oracle, "orbit")
    w, h, cam, win, lvl = case["w"], case["h"], case["cam"], case["win"], case["lvl"]
    cams = [case["prev_cam"], cam, gc.orbit(cam, -0.04)]
    desc = brt.gbuffer(1, 1, 2)

    def sequence(interleave):
        _upload(plugin, case)
        _lib.check(plugin._lib.brt_reset_temporal(plugin._ctx), plugin._ctx)
        out = []
        frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")

        def g():
            if interleave:
                _device(plugin, cam, win, w, h, desc, prev_cam=cams[0], cov=gc.coverage_frame(w, h, "blocks"))
                plugin.node.render_gbuffer(cams[2], win, w, h, desc, prev_camera=cam)

        g()
        out.append(plugin.node.run(lvl, cam, win, w, h).tobytes())
        g()
        for c in cams:
            plugin.node.render_device(lvl, c, win, w, h, frame.data_ptr(), flags=brt.FLAG_TEMPORAL)
            torch.cuda.synchronize()
            out.append(frame.cpu().numpy().tobytes())
            g()
        state = np.zeros((h, w, 8), F32)
        _lib.check(plugin._lib.brt_debug_temporal_state(plugin._ctx, w, h, state.ctypes.data), plugin._ctx)
        out.append(state.tobytes())
        g()
        plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=brt.FLAG_DENOISE)
        torch.cuda.synchronize()
        out.append(frame.cpu().numpy().tobytes())
        g()
        n_tiles = 24
        ray_sum = (np.arange(n_tiles, dtype=np.uint32) * 37) % 101 + 1
        longest = (np.arange(n_tiles, dtype=np.uint32) * 13) % 17 + 1
        order, info = np.zeros(n_tiles, np.uint32), np.zeros(5, np.uint32)
        _lib.check(plugin._lib.brt_debug_tile_order(plugin._ctx, ray_sum.ctypes.data, longest.ctypes.data, n_tiles, 2, 4096, 1, 0, 0,
                                                    order.ctypes.data, info.ctypes.data), plugin._ctx)
        out.append(order.tobytes() + info.tobytes())
        _lib.check(plugin._lib.brt_reset_temporal(plugin._ctx), plugin._ctx)
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed) == 7
    for i, (a, c) in enumerate(zip(plain, mixed)):
        assert a == c, f"step {i} of the sequence changed under interleaved G-buffer calls"
