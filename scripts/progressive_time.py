#!/usr/bin/env python3
"""Cost of progressive frames on one MI355X, timed with HIP events around the calls on a torch stream: 5 warm-up and 15 timed calls
each, medians; cover scene, 1920x1080, 8 bounces.  Every timed call starts from a zeroed state plane (the memset is inside the timing:
63 MiB, reported on its own as `state_memset`):
  (a) the whole-frame pass to 8 samples in raster order and in tile order (BRT_PROGRESSIVE_ORDER 0 / 1), against brt_render_pixels_device
      over the identity list and brt_render_device at 8 spp;
  (b) the one-call form at the defaults (first 8, max 64, default threshold and radius) in both orders, against brt_render_adaptive_device
      at (8, 64) and brt_render_device at 64 spp, with the share of pixels at each count;
  (c) the selecting kernel alone (brt_progressive_select_device on the state the one-call form left, target 64).
Prints one JSON document; --out writes it to a file (default profiles/progressive/progressive_time.json)."""
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
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive", "progressive_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (5, 15)
    w, h, first, max_spp = 1920, 1080, 8, 64
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam8, win = brt.cover_camera(w, h, first, 8, brt.Raytracing.Pure, 0.5)
    _, cam64, _ = brt.cover_camera(w, h, max_spp, 8, brt.Raytracing.Pure, 0.5)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    packed = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    state = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
    identity = torch.arange(w * h, dtype=torch.int32, device="cuda")
    lst = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {"scene": "cover", "size": [w, h], "first_spp": first, "max_spp": max_spp, "bounces": 8, "warmup": warmup, "timed": timed,
           "threshold": brt.PROG_DEFAULT_THRESHOLD, "radius": 1, "kernel_code_hash": brt._lib.kernel_code_hash()}

    def zero(s):
        with torch.cuda.stream(torch.cuda.ExternalStream(s)):
            state.zero_()

    res["state_memset"] = time_calls(zero, warmup, timed)
    for spp, cam, key in ((first, cam8, "frame_8spp"), (max_spp, cam64, "frame_64spp")):
        for _ in range(4):      # the steady state of the persistent kernel's dispatch order
            node.render_device(lvl, cam, win, w, h, frame.data_ptr())
        res[key] = time_calls(lambda s: node.render_device(lvl, cam, win, w, h, frame.data_ptr(), stream=s), warmup, timed)
    res["pixels_identity_8spp"] = time_calls(
        lambda s: node.render_pixels_device(cam8, win, w, h, identity.data_ptr(), w * h, packed.data_ptr(), stream=s), warmup, timed)
    plugin.set_adaptive(first, brt.ADAPT_DEFAULT_THRESHOLD, 6)
    for _ in range(3):
        node.render_adaptive_device(cam64, win, w, h, frame.data_ptr(), count.data_ptr())
    res["adaptive_8_64"] = time_calls(lambda s: node.render_adaptive_device(cam64, win, w, h, frame.data_ptr(), count.data_ptr(), stream=s),
                                      warmup, timed)
    res["adaptive_8_64"]["selected_share"] = float(int(count.cpu()[0]) / (w * h))
    plugin.set_progressive(first, max_spp, brt.PROG_DEFAULT_THRESHOLD, 1)
    for order, name in ((0, "raster"), (1, "tile")):
        with plugin.tuning(BRT_PROGRESSIVE_ORDER=order):
            def first_pass(s):
                zero(s)
                node.progressive_sample_device(cam8, win, w, h, state.data_ptr(), first, d_frame=frame.data_ptr(), stream=s)

            def one_call(s):
                zero(s)
                node.render_progressive_device(cam8, win, w, h, state.data_ptr(), frame.data_ptr(), stream=s)
            res["pass_8spp_" + name] = time_calls(first_pass, warmup, timed)
            res["one_call_" + name] = time_calls(one_call, warmup, timed)
    torch.cuda.synchronize()
    n = state.cpu().numpy().view(brt.PROG_PIXEL_DTYPE)["n"]
    res["share_by_count"] = {str(int(k)): float((n == k).mean()) for k in np.unique(n)}
    res["samples_per_pixel"] = float(n.mean())
    res["select_alone"] = time_calls(
        lambda s: node.progressive_select_device(w, h, state.data_ptr(), max_spp, lst.data_ptr(), count.data_ptr(), stream=s), warmup, timed)
    best = min(res["one_call_raster"]["median_ms"], res["one_call_tile"]["median_ms"])
    res["ratios"] = {"pass_raster_over_frame_8spp": res["pass_8spp_raster"]["median_ms"] / res["frame_8spp"]["median_ms"],
                     "pass_tile_over_frame_8spp": res["pass_8spp_tile"]["median_ms"] / res["frame_8spp"]["median_ms"],
                     "pass_raster_over_pixels_identity": res["pass_8spp_raster"]["median_ms"] / res["pixels_identity_8spp"]["median_ms"],
                     "one_call_over_frame_64spp": best / res["frame_64spp"]["median_ms"],
                     "one_call_over_adaptive": best / res["adaptive_8_64"]["median_ms"],
                     "one_call_ns_per_sample": 1e6 * best / (res["samples_per_pixel"] * w * h),
                     "frame_64spp_ns_per_sample": 1e6 * res["frame_64spp"]["median_ms"] / (max_spp * w * h)}
    plugin.close()
    doc = json.dumps(res, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
