#!/usr/bin/env python3
"""Cost of the post-passes on a blended (level 2) frame on one MI355X, timed with HIP events around the call on a torch stream: 10
warm-up and 30 timed calls per series, at 1920x1080 on the cover scene with the synthetic raster inputs of tests/blend_post_ref.py
(wall + disc), still camera.
  (a) brt_blend_post_device on the level-2 coverage frame in the three modes (DENOISE, TEMPORAL, both);
  (b) brt_denoise_device on the Pure-level frame of the same camera in the same three modes -- in the same process, the calls of (a) and
      (b) interleaved, so that the shared machine's drift hits both;
  (c) the whole brt_render_device frame at level 2, 4 spp, 4 bounces (the configuration the reference ships), without and with the
      post-passes (BRT_FLAG_BLEND_POST).
Prints one JSON document; --out writes it to a file (default profiles/blend_post/blend_post_time.json).  Per-kernel split: run this
under `rocprofv3 --kernel-trace --stats -- python scripts/blend_post_time.py --quick` (--quick: 3 warm-up + 10 timed calls, no file)."""
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
import blend_post_ref as bp  # noqa: E402

MODES = {"denoise": brt.FLAG_DENOISE, "temporal": brt.FLAG_TEMPORAL, "temporal_denoise": brt.FLAG_TEMPORAL | brt.FLAG_DENOISE}


def summary(ms):
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def time_interleaved(calls, warmup, timed):
    """calls: {name: f(stream)}; every round runs each call once, in turn, each between its own pair of events."""
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in calls}
    with torch.cuda.stream(s):
        for i in range(warmup + timed):
            for name, f in calls.items():
                ev[0].record(s)
                f(s.cuda_stream)
                ev[1].record(s)
                ev[1].synchronize()
                if i >= warmup:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_post", "blend_post_time.json"))
    ap.add_argument("--quick", action="store_true", help="3 warm-up + 10 timed calls, nothing written (for the rocprofv3 kernel split)")
    a = ap.parse_args()
    warmup, timed = (3, 10) if a.quick else (10, 30)
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash(), "warmup": warmup, "timed": timed}
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 1920, 1080
    rgba, depth = bp.raster_inputs(w, h)
    d_rgba, d_depth = torch.from_numpy(rgba).cuda(), torch.from_numpy(depth).cuda()
    # (b) runs on a context of its own: a history of its own in the temporal modes
    with brt.RaytracePlugin([0]) as plugin, brt.RaytracePlugin([0]) as plugin_b:
        node = plugin.node
        node.write_buffers(b)
        plugin_b.node.write_buffers(b)
        lvl2, cam, win = brt.cover_camera(w, h, 4, 4, brt.Raytracing.FallbackRaytraced, 0.5)
        lvl3, _, _ = brt.cover_camera(w, h, 4, 4, brt.Raytracing.Pure, 0.5)
        cov = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        pure = torch.empty_like(cov)
        out = torch.empty_like(cov)
        node.render_device(lvl2, cam, win, w, h, cov.data_ptr(), 0, d_depth.data_ptr())
        node.render_device(lvl3, cam, win, w, h, pure.data_ptr())
        torch.cuda.synchronize()
        res["size"] = [w, h]
        res["covered_share"] = float((cov[..., 3] == 0).float().mean().item())
        # (a) against (b), mode by mode: the two calls alternate on one stream (still camera: in the temporal modes every pixel with a
        # history reprojects onto itself)
        res["blend_post_device"], res["denoise_device"] = {}, {}
        for name, mode in MODES.items():
            plugin.reset_temporal()
            plugin_b.reset_temporal()
            r = time_interleaved({
                "a": lambda s, m=mode: node.blend_post_device(cam, win, w, h, cov.data_ptr(), out.data_ptr(), d_rgba.data_ptr(), stream=s, flags=m),
                "b": lambda s, m=mode: plugin_b.node.denoise_device(cam, win, w, h, pure.data_ptr(), out.data_ptr(), stream=s, flags=m),
            }, warmup, timed)
            res["blend_post_device"][name], res["denoise_device"][name] = r["a"], r["b"]
        # (c) the whole level-2 frame
        plugin.reset_temporal()
        frames = {"plain": 0}
        frames.update({k: brt.FLAG_BLEND_POST | m for k, m in MODES.items()})
        res["render_device_level2_4spp_4bounces"] = time_interleaved({
            k: (lambda s, f=f: node.render_device(lvl2, cam, win, w, h, out.data_ptr(), d_rgba.data_ptr(), d_depth.data_ptr(), stream=s, flags=f))
            for k, f in frames.items()}, warmup, timed)
    text = json.dumps(res, indent=1)
    print(text)
    if not a.quick:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
