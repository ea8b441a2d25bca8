#!/usr/bin/env python3
"""Cost of the upsampling of blended (level 1 / 2) frames on one MI355X, timed with HIP events around the calls on a torch stream: 10
warm-up and 30 timed calls each, medians.  Cover scene, the camera and the raster fixture of tests/test_upscale_blend.py at 1920x1080
from 960x540, 4 spp, 4 bounces (the reference's shipping settings at level 2).

  --mode kernel   brt_upscale_device (the unblended k_upscale) and brt_upscale_blend_device at level 2 on the same Pure low frame, with
                  the fixture's depth, with a depth of zeros (nothing covered: the added reads alone) and with a depth that covers the
                  whole frame (every wave branches over the gather).  With --parent only the first: for a library of the parent commit,
                  named by BRT_LIB_PATH, which lacks the blended exports.  Run the two builds alternately, a process each; the calls also
                  cast the low frame's guides, the same in both, so k_upscale by itself is its row of the kernel split
                  (rocprofv3 --kernel-trace --stats -- python scripts/upscale_blend_time.py --mode kernel --quick).
  --mode frame    brt_render_upscaled_blend_device at level 2 from 960x540 against plain brt_render_device at level 2 at full size with
                  the same raster inputs.

Prints one JSON document; --out writes it to a file."""
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
from bevyray_amd import _lib  # noqa: E402
import upscale_blend_ref as ubr  # noqa: E402
from helpers import uniforms  # noqa: E402
from upscale_time import time_calls  # noqa: E402

NEW_EXPORTS = ("brt_upscale_blend_device", "brt_render_upscaled_blend_device", "brt_host_blend_covered")


def view(w, h, level):
    return uniforms(w, h, 4, 4, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0), 0.5, 0.5, level=level)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "frame"), required=True)
    ap.add_argument("--parent", action="store_true", help="the library of BRT_LIB_PATH is the parent commit's: unblended calls only")
    ap.add_argument("--quick", action="store_true", help="3 warm-up and 5 timed calls (for the rocprofv3 kernel split)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parent:
        assert a.mode == "kernel" and os.environ.get("BRT_LIB_PATH")
        for name in NEW_EXPORTS:
            _lib._PROTOTYPES.pop(name)
    warmup, timed = (3, 5) if a.quick else (10, 30)
    w, h, lw, lh = 1920, 1080, 960, 540
    res = {"device": torch.cuda.get_device_name(0), "library": "parent" if a.parent else "this tree",
           "kernel_code_hash": _lib.kernel_code_hash(), "warmup": warmup, "timed": timed, "size": [w, h], "low_size": [lw, lh]}
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl3, cam, win = view(w, h, brt.Raytracing.Pure)
    lvl2, _, _ = view(w, h, brt.Raytracing.FallbackRaytraced)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rgba = dev(ubr.raster_rgba(w, h))
    depths = {"fixture": dev(ubr.raster_depth(w, h)), "nothing_covered": torch.zeros((h, w), dtype=torch.float32, device="cuda"),
              "all_covered": torch.full((h, w), 1.0e6, dtype=torch.float32, device="cuda")}
    with brt.RaytracePlugin([0]) as plugin:
        node = plugin.node
        node.write_buffers(brt.Buffers(b.models, b.materials, None))
        out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        low = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
        node.render_device(lvl3, cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr())
        t = plugin.debug_denoise_guides(cam, win, w, h)[..., 3]
        res["covered_share"] = {k: float(np.mean(ubr.covered(cam, 2, t, d.cpu().numpy()))) for k, d in depths.items()}
        if a.mode == "kernel":
            res["upscale_device"] = time_calls(
                lambda s: node.upscale_device(cam, win, lw, lh, low.data_ptr(), w, h, out.data_ptr(), stream=s), warmup, timed)
            if not a.parent:
                res["upscale_blend_device_level2"] = {}
                for key, d in depths.items():
                    res["upscale_blend_device_level2"][key] = time_calls(
                        lambda s: node.upscale_blend_device(lvl2, cam, win, lw, lh, low.data_ptr(), w, h, out.data_ptr(),
                                                            d_raster_rgba=rgba.data_ptr(), d_raster_depth=d.data_ptr(), stream=s),
                        warmup, timed)
        else:
            d = depths["fixture"]
            res["render_device_level2_full"] = time_calls(
                lambda s: node.render_device(lvl2, cam, win, w, h, out.data_ptr(), d_raster_rgba=rgba.data_ptr(),
                                             d_raster_depth=d.data_ptr(), stream=s), warmup, timed)
            res["render_upscaled_blend_device_level2"] = time_calls(
                lambda s: node.render_upscaled_blend_device(lvl2, cam, win, lw, lh, w, h, out.data_ptr(), d_raster_rgba=rgba.data_ptr(),
                                                            d_raster_depth=d.data_ptr(), stream=s), warmup, timed)
            res["render_upscaled_blend_device_level2"]["over_full"] = (res["render_upscaled_blend_device_level2"]["median_ms"] /
                                                                       res["render_device_level2_full"]["median_ms"])
            res["render_device_pure_low"] = time_calls(
                lambda s: node.render_device(lvl3, cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr(), stream=s), warmup, timed)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
