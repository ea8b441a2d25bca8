#!/usr/bin/env python3
"""Cost and quality of the guide-buffer upsampling on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up
and 30 timed calls each, cover scene, 1920x1080, 64 spp, 8 bounces:
  (a) the full frame through brt_render_device;
  (b) brt_render_upscaled_device from 960x540 and from 1280x720;
  (c) brt_upscale_device alone, from both low sizes (the call also casts the low frame's guides: k_upscale by itself is its row of the
      kernel split);
  (d) brt_denoise_device at 1080p, for scale.
Also the quality ratio at 480x270 from 240x135 for 4 and 64 spp: MSE over the full-size hit pixels of the upsampled frame / of the plain
bilinear upsampling of the same low frame, against a 1024-spp full-size frame of another seed.  Prints one JSON document; --out writes it
to a file.  Per-kernel split: run this under `rocprofv3 --kernel-trace --stats -- python scripts/upscale_time.py --quick`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bevyray_amd as brt  # noqa: E402
import denoise_ref as dr  # noqa: E402


def bilinear(low, w, h):
    """Plain bilinear upsampling of the colour of `low` to w x h, pixel centres aligned and edges clamped: the baseline of the quality
    ratio (tests/test_upscale.py holds the same few lines for its bars)."""
    lh, lw = low.shape[:2]
    xs = np.clip((np.arange(w) + 0.5) * lw / w - 0.5, 0, lw - 1)
    ys = np.clip((np.arange(h) + 0.5) * lh / h - 0.5, 0, lh - 1)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    x1, y1 = np.minimum(x0 + 1, lw - 1), np.minimum(y0 + 1, lh - 1)
    fx, fy = (xs - x0)[None, :, None], (ys - y0)[:, None, None]
    c = low[..., :3].astype(np.float64)
    out = (c[y0][:, x0] * (1 - fx) + c[y0][:, x1] * fx) * (1 - fy) + (c[y1][:, x0] * (1 - fx) + c[y1][:, x1] * fx) * fy
    return out.astype(np.float32)


def time_calls(call, warmup, timed):
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(s):
        for _ in range(warmup):
            call(s.cuda_stream)
        s.synchronize()
        ms = []
        for _ in range(timed):
            ev[0].record(s)
            call(s.cuda_stream)
            ev[1].record(s)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="3 warm-up and 5 timed calls, no quality (for the rocprofv3 kernel split)")
    a = ap.parse_args()
    warmup, timed = (3, 5) if a.quick else (10, 30)
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash(), "warmup": warmup, "timed": timed}
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h, spp, bounces = 1920, 1080, 64, 8
    with brt.RaytracePlugin([0]) as plugin:
        node = plugin.node
        lvl, cam, win = brt.cover_camera(w, h, spp, bounces, brt.Raytracing.Pure, 0.5)
        frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        out = torch.empty_like(frame)
        node.write_buffers(b)
        res["size"], res["spp"], res["bounces"] = [w, h], spp, bounces
        res["a_render_device"] = time_calls(lambda s: node.render_device(lvl, cam, win, w, h, frame.data_ptr(), stream=s), warmup, timed)
        res["b_render_upscaled_device"], res["c_upscale_device"] = {}, {}
        for lw, lh in ((960, 540), (1280, 720)):
            key = f"{lw}x{lh}"
            low = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
            lwin = brt.upscale_window(win, h, lh)
            res["low_render_device_" + key] = time_calls(lambda s: node.render_device(lvl, cam, lwin, lw, lh, low.data_ptr(), stream=s),
                                                         warmup, timed)
            res["b_render_upscaled_device"][key] = time_calls(
                lambda s: node.render_upscaled_device(cam, win, lw, lh, w, h, out.data_ptr(), stream=s), warmup, timed)
            res["b_render_upscaled_device"][key]["over_a"] = res["b_render_upscaled_device"][key]["median_ms"] / res["a_render_device"]["median_ms"]
            res["c_upscale_device"][key] = time_calls(
                lambda s: node.upscale_device(cam, win, lw, lh, low.data_ptr(), w, h, out.data_ptr(), stream=s), warmup, timed)
        res["d_denoise_device"] = time_calls(lambda s: node.denoise_device(cam, win, w, h, frame.data_ptr(), out.data_ptr(), stream=s),
                                             warmup, timed)
        if not a.quick:
            qw, qh, ql, qk = 480, 270, 240, 135
            _, cam_r, win_r = brt.cover_camera(qw, qh, 1024, bounces, brt.Raytracing.Pure, 0.25)
            ref = node.run(lvl, cam_r, win_r, qw, qh).copy()
            res["quality_480x270_from_240x135"] = {}
            for q in (4, 64):
                lq, cq, wq = brt.cover_camera(qw, qh, q, bounces, brt.Raytracing.Pure, 0.5)
                low = node.run(lq, cq, brt.upscale_window(wq, qh, qk), ql, qk).copy()
                up = torch.empty((qh, qw, 4), dtype=torch.float32, device="cuda")
                node.render_upscaled_device(cq, wq, ql, qk, qw, qh, up.data_ptr())
                g = plugin.debug_denoise_guides(cq, wq, qw, qh)
                m_up, m_bi = dr.hit_mse(up.cpu().numpy(), ref, g), dr.hit_mse(bilinear(low, qw, qh), ref, g)
                res["quality_480x270_from_240x135"][f"{q}spp"] = {"mse_upsampled": m_up, "mse_bilinear": m_bi, "ratio": m_up / m_bi}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
