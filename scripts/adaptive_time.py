#!/usr/bin/env python3
"""Cost of adaptive sampling on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up and 30 timed calls
each, medians; cover scene, 1920x1080, 64 spp, 8 bounces (the headline configuration), base_spp 8, default threshold and min_taps:
  (a) the selected share of pixels per class (brt_adaptive_mask_device on the base frame);
  (b) brt_render_adaptive_device against brt_render_device at 64 spp and at the base 8 spp on the same build;
  (c) its steps behind a base frame: brt_adaptive_refine_device (guides + selection + re-trace) in both pixel-tracer forms, and with a
      threshold that selects nothing (guides + selection alone);
  (d) the plain frame alone -- run the script with --root <a checkout of the parent commit with its library built> --out <other file>
      to compare it with the parent's (a package without the adaptive exports: only `full_frame` is measured).
Prints one JSON document; --out writes it to a file (default profiles/adaptive/adaptive_time.json).  The selection kernel alone: run this
under `rocprofv3 --kernel-trace --stats -- python scripts/adaptive_time.py --quick` (k_adaptive_select in the kernel statistics)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PACKAGE_ROOT)

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
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose bevyray_amd package is timed (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "adaptive_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (10, 30)
    w, h, spp, base_spp = 1920, 1080, 64, 8
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5)
    _, cam_base, _ = brt.cover_camera(w, h, base_spp, 8, brt.Raytracing.Pure, 0.5)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    base = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    res = {"scene": "cover", "size": [w, h], "spp": spp, "base_spp": base_spp, "bounces": 8, "warmup": warmup, "timed": timed,
           "package": "tree" if PACKAGE_ROOT == ROOT else "other checkout", "kernel_code_hash": brt._lib.kernel_code_hash()}
    for _ in range(4):      # the steady state of the persistent kernel's dispatch order
        node.render_device(lvl, cam, win, w, h, frame.data_ptr())
    res["full_frame"] = time_calls(lambda s: node.render_device(lvl, cam, win, w, h, frame.data_ptr(), stream=s), warmup, timed)
    if "brt_render_adaptive_device" in brt._lib.EXPORTS:
        thr = brt.ADAPT_DEFAULT_THRESHOLD
        plugin.set_adaptive(base_spp, thr, 6)
        res["threshold"], res["min_taps"] = thr, 6
        res["base_frame"] = time_calls(lambda s: node.render_device(lvl, cam_base, win, w, h, base.data_ptr(), stream=s), warmup, timed)
        node.render_device(lvl, cam_base, win, w, h, base.data_ptr())
        node.adaptive_mask_device(cam, win, w, h, base.data_ptr(), mask.data_ptr())
        torch.cuda.synchronize()
        m = mask.cpu().numpy()
        res["share"] = {"sparse": float((m == brt.ADAPT_SPARSE).mean()), "noisy": float((m == brt.ADAPT_NOISY).mean()),
                        "selected": float((m != 0).mean())}
        for _ in range(3):
            node.render_adaptive_device(cam, win, w, h, frame.data_ptr(), count.data_ptr())
        res["steady_prepass_ms"] = node.last_stats["prepass_ms"]
        res["adaptive"] = time_calls(lambda s: node.render_adaptive_device(cam, win, w, h, frame.data_ptr(), count.data_ptr(), stream=s),
                                     warmup, timed)
        res["adaptive"]["pixels"] = int(count.cpu()[0])
        for name, form in (("stream", 2), ("plain", 1)):
            with plugin.tuning(BRT_PIXELS_FORM=form):
                res["refine_step_" + name] = time_calls(
                    lambda s: node.adaptive_refine_device(cam, win, w, h, base.data_ptr(), frame.data_ptr(), 0, stream=s), warmup, timed)
        plugin.set_adaptive(base_spp, 1e30, 1)
        res["select_step"] = time_calls(lambda s: node.adaptive_refine_device(cam, win, w, h, base.data_ptr(), frame.data_ptr(), 0, stream=s),
                                        warmup, timed)
        plugin.set_adaptive(base_spp, thr, 6)
        full, n = res["full_frame"]["median_ms"], max(res["adaptive"]["pixels"], 1)
        retrace = res["refine_step_stream"]["median_ms"] - res["select_step"]["median_ms"]
        res["ratios"] = {"adaptive_over_full": res["adaptive"]["median_ms"] / full,
                         "base_over_full": res["base_frame"]["median_ms"] / full,
                         "retrace_ns_per_selected_pixel": 1e6 * retrace / n,
                         "full_frame_ns_per_pixel": 1e6 * full / (w * h),
                         "selected_share_x_retrace_cost_over_full_cost": (n / (w * h)) * (retrace / n) / (full / (w * h))}
    plugin.close()
    doc = json.dumps(res, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
