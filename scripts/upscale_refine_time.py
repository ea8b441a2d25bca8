#!/usr/bin/env python3
"""Cost of the refined upsampling and of the sparse pixel tracer on one MI355X, timed with HIP events around the calls on a torch stream:
10 warm-up and 30 timed calls each, medians; cover scene, 1920x1080, 64 spp, 8 bounces, from 960x540:
  (a) the refined share of pixels per class (brt_upscale_refine_mask_device);
  (b) brt_render_upscaled_refined_device (each class mask) against brt_render_upscaled_device and against the full frame
      (brt_render_device); the parent commit's brt_render_upscaled_device is the same call on a library built from it (BRT_LIB_PATH);
  (c) the sparse tracer by itself: brt_render_pixels_device over the list of ALL 1080p pixels (row-major, and shuffled) against
      brt_render_device -- its cost per pixel relative to the persistent kernel on identical work;
  (d) the streaming form against the plain form (BRT_PIXELS_FORM) on the refinement's own list.
Prints one JSON document; --out writes it to a file (default profiles/upscale_refine/upscale_refine_time.json).  Per-kernel split: run
this under `rocprofv3 --kernel-trace --stats -- python scripts/upscale_refine_time.py --quick`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bevyray_amd as brt  # noqa: E402


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
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls, 8 spp (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale_refine", "upscale_refine_time.json"))
    args = ap.parse_args()
    warmup, timed, spp = (2, 3, 8) if args.quick else (10, 30, 64)
    w, h, lw, lh = 1920, 1080, 960, 540
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    low = torch.zeros((lh, lw, 4), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    res = {"scene": "cover", "size": [w, h], "low": [lw, lh], "spp": spp, "bounces": 8, "warmup": warmup, "timed": timed,
           "library": os.environ.get("BRT_LIB_PATH", "tree")}
    # the steady state of the persistent kernel's dispatch order: a few synchronous frames of each size first
    for _ in range(4):
        node.render_device(lvl, cam, win, w, h, frame.data_ptr())
        node.render_device(lvl, cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr())
    res["full_frame"] = time_calls(lambda s: node.render_device(lvl, cam, win, w, h, frame.data_ptr(), stream=s), warmup, timed)
    res["upscaled"] = time_calls(lambda s: node.render_upscaled_device(cam, win, lw, lh, w, h, frame.data_ptr(), stream=s), warmup, timed)
    if hasattr(node, "upscale_refine_mask_device") and "brt_upscale_refine_mask_device" in brt._lib.EXPORTS and not os.environ.get("BRT_LIB_PATH"):
        node.upscale_refine_mask_device(cam, win, lw, lh, low.data_ptr(), w, h, mask.data_ptr())
        torch.cuda.synchronize()
        m = mask.cpu().numpy()
        res["share"] = {"edges": float(((m & 1) != 0).mean()), "specular": float(((m & 2) != 0).mean()), "both": float((m != 0).mean())}
        for name, classes in (("edges", 1), ("specular", 2), ("both", 3)):
            res["refined_" + name] = time_calls(lambda s: node.render_upscaled_refined_device(cam, win, lw, lh, w, h, frame.data_ptr(), classes,
                                                                                             count.data_ptr(), stream=s), warmup, timed)
            res["refined_" + name]["pixels"] = int(count.cpu()[0])
        # the refinement by itself on its own list: both forms
        for name, form in (("stream", 2), ("plain", 1)):
            with plugin.tuning(BRT_PIXELS_FORM=form):
                res["refine_step_" + name] = time_calls(lambda s: node.upscale_refine_device(cam, win, lw, lh, low.data_ptr(), w, h, frame.data_ptr(), 3,
                                                                                            0, stream=s), warmup, timed)
        res["upscale_step"] = time_calls(lambda s: node.upscale_device(cam, win, lw, lh, low.data_ptr(), w, h, frame.data_ptr(), stream=s), warmup, timed)
        # the sparse tracer over every pixel of the frame
        rng = np.random.default_rng(1)
        for name, order in (("row_major", np.arange(w * h, dtype=np.uint32)), ("shuffled", rng.permutation(w * h).astype(np.uint32))):
            d_px = torch.from_numpy(order.view(np.int32)).cuda()
            for fname, form in (("stream", 2), ("plain", 1)):
                with plugin.tuning(BRT_PIXELS_FORM=form):
                    res[f"all_pixels_{name}_{fname}"] = time_calls(
                        lambda s: node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), w * h, frame.data_ptr(), stream=s), warmup, timed)
        full = res["full_frame"]["median_ms"]
        res["ratios"] = {"refined_both_over_upscaled": res["refined_both"]["median_ms"] / res["upscaled"]["median_ms"],
                         "refined_both_over_full": res["refined_both"]["median_ms"] / full,
                         "upscaled_over_full": res["upscaled"]["median_ms"] / full,
                         "all_pixels_row_major_stream_over_full": res["all_pixels_row_major_stream"]["median_ms"] / full,
                         "all_pixels_shuffled_stream_over_full": res["all_pixels_shuffled_stream"]["median_ms"] / full}
    plugin.close()
    doc = json.dumps(res, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
