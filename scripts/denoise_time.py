#!/usr/bin/env python3
"""Cost of the denoiser (brt_denoise_device: guides + demodulation + variance + the a-trous passes) on one MI355X, timed with HIP
events around the call on a torch stream: 10 warm-up and 30 timed calls per setting, at 1920x1080 on the cover scene, for the
default settings and for iterations 1..6.  Also the quality ratio (MSE over the hit pixels of the denoised frame / of the noisy one,
against a 1024-spp frame of another seed) at 480x270 for 4 and 64 spp.  Prints one JSON document; --out writes it to a file.
Per-kernel split: run this under `rocprofv3 --kernel-trace --stats -- python scripts/denoise_time.py --quick`."""
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


def time_calls(plugin, cam, win, w, h, d_in, d_out, warmup, timed):
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(s):
        for _ in range(warmup):
            plugin.node.denoise_device(cam, win, w, h, d_in.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
        ms = []
        for _ in range(timed):
            ev[0].record(s)
            plugin.node.denoise_device(cam, win, w, h, d_in.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
            ev[1].record(s)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="defaults only, no quality (for the rocprofv3 kernel split)")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash()}
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 1920, 1080
    with brt.RaytracePlugin([0]) as plugin:
        lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
        frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        out = torch.empty_like(frame)
        plugin.node.write_buffers(b)
        plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr())
        res["size"] = [w, h]
        res["default"] = time_calls(plugin, cam, win, w, h, frame, out, 10, 30)
        if not a.quick:
            res["iterations"] = {}
            for it in range(1, 7):
                plugin.set_denoise(iterations=it)
                res["iterations"][str(it)] = time_calls(plugin, cam, win, w, h, frame, out, 10, 30)
            plugin.set_denoise()
            qw, qh = 480, 270
            _, cam_r, win_r = brt.cover_camera(qw, qh, 1024, 8, brt.Raytracing.Pure, 0.25)
            ref = plugin.node.run(lvl, cam_r, win_r, qw, qh, buffers=b).copy()
            res["quality_480x270"] = {}
            for spp in (4, 64):
                lq, cq, wq = brt.cover_camera(qw, qh, spp, 8, brt.Raytracing.Pure, 0.5)
                noisy = plugin.node.run(lq, cq, wq, qw, qh).copy()
                den = plugin.node.run(lq, cq, wq, qw, qh, flags=brt.FLAG_DENOISE).copy()
                g = plugin.debug_denoise_guides(cq, wq, qw, qh)
                res["quality_480x270"][f"{spp}spp"] = {"mse_noisy": dr.hit_mse(noisy, ref, g), "mse_denoised": dr.hit_mse(den, ref, g),
                                                      "ratio": dr.hit_mse(den, ref, g) / dr.hit_mse(noisy, ref, g)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
