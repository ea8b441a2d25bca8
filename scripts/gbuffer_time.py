#!/usr/bin/env python3
"""Cost of a G-buffer call on one MI355X, timed with HIP events on a torch stream: 5 warm-up calls, then 15 timed samples, each sample
REPS calls enqueued back to back between two events and divided by REPS (the host's issue path -- Python, ctypes, the entry point -- of
a call then overlaps the GPU's work of the call before it; one call between two events would count it); median [min, max]; the cover
scene and the 10 004-sphere stress grid at 1920 x 1080, each after a rendered frame:
  (a) brt_render_gbuffer_device with all five planes (depth VIEW, normal RGBA32F, motion UV32F against an orbited previous camera);
  (b) the same with each plane alone, and with the packed formats (normal RGB10A2, motion UV16F);
  (c) brt_query_rays_device in the plain form over the same pixel-centre rays (64 bytes per pixel through memory): the first yardstick;
  (d) a device copy of as many bytes as the planes of (a) hold, between random-filled buffers, rotating over four source / destination
      pairs (1 GB in all, so that no copy finds its lines in the 256 MB last-level cache): the second.
Prints one JSON document with the ratios (a) / (c) and (a) / (d); --out writes it to a file (default profiles/gbuffer/gbuffer_time.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


REPS = 10


def time_calls(call, warmup, timed, reps=REPS):
    import numpy as np
    import torch
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(s):
        for _ in range(warmup):
            call(s.cuda_stream)
        s.synchronize()
        ms = []
        for _ in range(timed):
            ev[0].record(s)
            for _ in range(reps):
                call(s.cuda_stream)
            ev[1].record(s)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]) / reps)
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


PLANE_BYTES = {"depth": 4, "normal": 16, "motion": 8, "ids": 16, "albedo": 16}


def measure_scene(plugin, name, warmup, timed, w, h):
    import numpy as np
    import torch

    import bevyray_amd as brt
    import gbuffer_cases as gc
    node = plugin.node
    b = brt.generate_scene(brt.SCENE_COVER if name == "cover" else brt.SCENE_STRESS_GRID, 1)
    lvl, cam, win = brt.cover_camera(w, h, 1, 2)
    node.write_buffers(b)
    frame = torch.zeros(w * h * 16, dtype=torch.uint8, device="cuda")
    node.render_device(lvl, cam, win, w, h, frame.data_ptr())            # (the tree's reach settled, the hot order applied)
    prev = gc.orbit(cam, 0.01)
    n = w * h
    bufs = {k: torch.zeros(n * v, dtype=torch.uint8, device="cuda") for k, v in PLANE_BYTES.items()}
    ptr = {"d_" + k: t.data_ptr() for k, t in bufs.items()}
    desc = brt.gbuffer(brt.GBUFFER_DEPTH_VIEW, brt.GBUFFER_NORMAL_RGBA32F, brt.GBUFFER_MOTION_UV32F)
    packed = brt.gbuffer(brt.GBUFFER_DEPTH_VIEW, brt.GBUFFER_NORMAL_RGB10A2, brt.GBUFFER_MOTION_UV16F)
    st = dict(node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev, **ptr))
    res = {"scene": name, "spheres": int(len(b.models)), "width": w, "height": h, "cast": st["cast"], "hits": st["hits"],
           "no_previous": st["no_previous"], "plane_bytes_per_pixel": sum(PLANE_BYTES.values())}
    res["all_planes"] = time_calls(lambda s: node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev, stream=s, **ptr), warmup, timed)
    res["all_planes_packed"] = time_calls(lambda s: node.render_gbuffer_device(cam, win, w, h, packed, prev_camera=prev, stream=s, **ptr), warmup, timed)
    for k in PLANE_BYTES:
        one = {"d_" + k: bufs[k].data_ptr()}
        res[k + "_alone"] = time_calls(lambda s: node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev, stream=s, **one), warmup, timed)
    # the yardsticks: the plain query form over the same rays, and a copy of the planes' bytes
    rays = np.zeros(n, brt.RAY_DTYPE)
    import denoise_ref as dr                             # (brt_host_pixel_ray's arithmetic, vectorised)
    import oracle_loader
    o, dirs, _ = dr.pixel_center_rays(oracle_loader.load(), cam, w, h)
    rays["origin"], rays["direction"], rays["t_max"] = o, dirs.reshape(-1, 3), np.inf
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    with plugin.tuning(BRT_QUERY_FORM=1):
        q = dict(node.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr()))
        assert q["hits"] == st["hits"], (q, st)          # (the same rays, the same hits)
        res["query_plain"] = time_calls(lambda s: node.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=s), warmup, timed)
    total = n * sum(PLANE_BYTES.values())
    pairs = [(torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")) for _ in range(4)]
    turn = [0]

    def copy(s):
        src, dst = pairs[turn[0] % 4]
        turn[0] += 1
        dst.copy_(src, non_blocking=True)

    res["device_copy_of_the_planes_bytes"] = time_calls(copy, warmup, timed)
    del pairs
    res["all_planes_again"] = time_calls(lambda s: node.render_gbuffer_device(cam, win, w, h, desc, prev_camera=prev, stream=s, **ptr), warmup, timed)
    best = min(res["all_planes"]["median_ms"], res["all_planes_again"]["median_ms"])
    res["all_planes_over_query_plain"] = best / res["query_plain"]["median_ms"]
    res["all_planes_over_copy"] = best / res["device_copy_of_the_planes_bytes"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer", "gbuffer_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (5, 15)
    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    doc = {"warmup": warmup, "timed_samples": timed, "calls_per_sample": REPS, "scenes": [measure_scene(plugin, name, warmup, timed, args.width, args.height) for name in ("cover", "stress")]}
    plugin.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
