#!/usr/bin/env python3
"""Cost of the radiance queries on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up and 30 timed calls
each, medians; cover scene, the pixel-centre rays of a 1920x1080 frame (brt_host_pixel_ray, one seed per pixel), 16 samples, 8 bounces:
  (a) brt_radiance_rays_device in both kernel forms (BRT_RADIANCE_FORM), rays in row-major order and shuffled;
  (b) brt_render_pixels_device over all pixels of the same frame at 16 spp in both of its forms: the nearest kernel there was before
      (the same paths per pixel up to the jitter of the camera ray; it walks the camera ray of every sample);
  (c) the walks each of them performed (synchronous calls on the context's own stream).
Prints one JSON document; --out writes it to a file (default profiles/radiance/radiance_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/radiance_time.py --quick`."""
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


def pixel_centre_rays(cam, win, w, h):
    """RADIANCE_RAY_DTYPE records of the frame's pixel-centre rays in raster order: brt_host_pixel_ray per pixel, then a seed in the
    t_max slot (user stays py * width + px)."""
    lib = brt._lib.load()
    rays = np.zeros(w * h, brt.RAY_DTYPE)
    base, c, wn = rays.ctypes.data, cam.ctypes.data, win.ctypes.data
    for py in range(h):
        for px in range(w):
            lib.brt_host_pixel_ray(c, wn, w, h, px, py, base + 32 * (py * w + px))
    out = rays.view(brt.RADIANCE_RAY_DTYPE)
    out["seed"] = np.arange(w * h, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance", "radiance_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (10, 30)
    w, h = (int(x) for x in args.size.split("x"))
    spp, bounces = 16, 8
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces, brt.Raytracing.Pure, 0.5)
    n = w * h
    rays = pixel_centre_rays(cam, win, w, h)
    order = np.random.default_rng(1).permutation(n)
    res = {"scene": "cover", "size": [w, h], "rays": n, "samples": spp, "bounces": bounces, "warmup": warmup, "timed": timed}
    d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    ref_bytes = None
    for name, host in (("row_major", rays), ("shuffled", rays[order])):
        d_rays = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8)).cuda()
        for fname, form in (("stream", 2), ("plain", 1)):
            with plugin.tuning(BRT_RADIANCE_FORM=form):
                st = node.radiance_rays((d_rays.data_ptr(), n, d_out.data_ptr()), spp, bounces, device=True)
                got = d_out.cpu().numpy().view(brt.RADIANCE_DTYPE)
                got = got if name == "row_major" else got[np.argsort(order)]
                if ref_bytes is None:
                    ref_bytes = got.tobytes()
                assert got.tobytes() == ref_bytes, (name, fname)           # (the bytes depend on neither the form nor the order)
                key = f"radiance_{name}_{fname}"
                res[key] = time_calls(lambda s: node.radiance_rays((d_rays.data_ptr(), n, d_out.data_ptr()), spp, bounces, device=True, stream=s),
                                      warmup, timed)
                res[key].update(walks=st["walks"], hit_entries=st["hits"], workgroups=st["n_workgroups"])
        d_px = torch.from_numpy((np.arange(n, dtype=np.uint32) if name == "row_major" else order.astype(np.uint32)).view(np.int32)).cuda()
        for fname, form in (("stream", 2), ("plain", 1)):
            with plugin.tuning(BRT_PIXELS_FORM=form):
                walks = int(node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, frame.data_ptr())["rays"])
                key = f"pixels_{name}_{fname}"
                res[key] = time_calls(lambda s: node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, frame.data_ptr(), stream=s), warmup, timed)
                res[key]["walks"] = walks
    res["ratios"] = {f"radiance_over_pixels_{name}_{fname}": res[f"radiance_{name}_{fname}"]["median_ms"] / res[f"pixels_{name}_{fname}"]["median_ms"]
                     for name in ("row_major", "shuffled") for fname in ("stream", "plain")}
    res["ratios"]["radiance_plain_over_stream_row_major"] = res["radiance_row_major_plain"]["median_ms"] / res["radiance_row_major_stream"]["median_ms"]
    plugin.close()
    doc = json.dumps(res, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
