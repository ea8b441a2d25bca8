#!/usr/bin/env python3
"""Cost of the batched ray queries (brt_query_rays_device) on one MI355X: HIP events around the call on a torch stream, 10 warm-up and
30 timed calls per series, the plain and the streaming form alternating call by call in one process; median (min .. max) ms.
1920x1080 = 2 073 600 rays of the cover scene and of the 10 004-sphere grid:
  (a) pixel-centre rays in raster order   (b) the same shuffled   (c) one diffuse bounce from the hits of (a), shuffled
  (d) ANY mode on (c)                     (e) a batch of 1 and of 64 rays (the pick): wall time of the whole synchronous call, in us
and, beside (a), the guide kernel of the same camera (brt_denoise_device with one pass is not a fair partner, so the guides are taken
from a kernel trace: run this under `rocprofv3 --kernel-trace --stats -- python scripts/query_time.py --quick`).
Prints one JSON document; --out writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bevyray_amd as brt  # noqa: E402

PLAIN, STREAM = 1, 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def summary(ms):
    ms = np.array(ms)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def time_forms(plugin, d_rays, n, d_hits, mode, warmup, timed):
    """-> {"plain": .., "stream": ..} ms, the two forms alternating."""
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {PLAIN: [], STREAM: []}
    with torch.cuda.stream(s):
        for i in range(warmup + timed):
            for form in (PLAIN, STREAM):
                plugin.set_tuning("BRT_QUERY_FORM", form)
                ev[0].record(s)
                plugin.node.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), mode, stream=s.cuda_stream)
                ev[1].record(s)
                ev[1].synchronize()
                if i >= warmup:
                    ms[form].append(ev[0].elapsed_time(ev[1]))
    plugin.set_tuning("BRT_QUERY_FORM", 0)
    return {"plain": summary(ms[PLAIN]), "stream": summary(ms[STREAM])}


def time_pick(plugin, rays, warmup, timed):
    """wall time (us) of the whole synchronous host-buffer call, the two forms alternating"""
    us = {PLAIN: [], STREAM: []}
    for i in range(warmup + timed):
        for form in (PLAIN, STREAM):
            plugin.set_tuning("BRT_QUERY_FORM", form)
            t0 = time.perf_counter()
            plugin.node.query_rays(rays)
            if i >= warmup:
                us[form].append((time.perf_counter() - t0) * 1e6)
    plugin.set_tuning("BRT_QUERY_FORM", 0)
    return {"plain_us": summary(us[PLAIN]), "stream_us": summary(us[STREAM])}


def pixel_rays(cam, win, w, h):
    """the pixel-centre rays in raster order, vectorised in numpy (2 M calls of brt_host_pixel_ray would take minutes): the same formula
    with tan evaluated by numpy, so a direction may differ from the picking ray's in the last bit -- of no consequence for a time"""
    first = brt.pixel_ray(cam, win, w, h, 0, 0)                     # (the library's own ray fixes origin and t_max)
    c = cam[0]
    f32 = np.float32
    cd, cu = c["direction"].astype(f32), c["up"].astype(f32)
    right = np.array([cd[1] * cu[2] - cd[2] * cu[1], cd[2] * cu[0] - cd[0] * cu[2], cd[0] * cu[1] - cd[1] * cu[0]], f32)
    scale = f32(np.tan(np.float64(f32(c["fov"]) * f32(0.5))))
    uvx = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    uvy = (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    ndc_x = (uvx * f32(2.0) - f32(1.0))[None, :, None]
    ndc_y = (f32(1.0) - uvy * f32(2.0))[:, None, None]
    d = (cd + ((ndc_x * f32(c["aspect"])) * scale) * right) + (ndc_y * scale) * cu
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    rays = np.zeros(w * h, brt.RAY_DTYPE)
    rays["origin"] = first["origin"][0]
    rays["t_max"] = np.inf
    rays["direction"] = (d / ln).astype(f32).reshape(-1, 3)
    rays["user"] = np.arange(w * h, dtype=np.uint32)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="series (a) of the cover scene and its guide kernel only (for the rocprofv3 kernel split)")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash(), "unit": "ms (picks: us)"}
    w, h = 1920, 1080
    rng = np.random.default_rng(3)
    with brt.RaytracePlugin([0]) as plugin:
        for name, kind in (("cover", brt.SCENE_COVER), ("stress_grid", brt.SCENE_STRESS_GRID)):
            if a.quick and name != "cover":
                break
            b = brt.generate_scene(kind, 1)
            lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
            frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
            for seed in (0.5, 0.25):                                 # frames first: the resident numbering is the steady-state one
                plugin.node.render_device(lvl, cam, brt.WindowExtract.extract_component(h, seed), w, h, frame.data_ptr())
            bound = float(np.abs(cam[0]["position"]).sum())
            ra = pixel_rays(cam, win, w, h)
            n = len(ra)
            d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_a = dev(ra)
            plugin.node.query_rays_device(d_a.data_ptr(), n, d_hits.data_ptr(), origin_bound=bound)     # (raises the reach once, if needed)
            r = {"rays": n, "stats": plugin.node.last_query_stats}
            r["a_raster"] = time_forms(plugin, d_a, n, d_hits, brt.QUERY_CLOSEST, 10, 30)
            if a.quick:
                out = torch.empty_like(frame)
                for _ in range(5):
                    plugin.node.denoise_device(cam, win, w, h, frame.data_ptr(), out.data_ptr())   # (its k_denoise_guides is the partner of (a))
                res[name] = r
                break
            hits_a = d_hits.cpu().numpy().view(brt.HIT_DTYPE).copy()
            perm = rng.permutation(n)
            d_b = dev(ra[perm])
            r["b_shuffled"] = time_forms(plugin, d_b, n, d_hits, brt.QUERY_CLOSEST, 10, 30)
            # one diffuse bounce from the hits of (a): origin on the surface, direction normal + a unit-ball point; misses keep their ray
            on = (hits_a["status"] & brt.QUERY_STATUS_HIT) != 0
            rc = ra.copy()
            pos = ra["origin"] + hits_a["t"][:, None] * ra["direction"]
            ball = rng.normal(size=(n, 3))
            ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)
            rc["origin"][on] = pos[on].astype(np.float32)
            rc["direction"][on] = (hits_a["normal"][on] + ball[on]).astype(np.float32)
            d_c = dev(rc[perm])
            r["hit_share_of_a"] = float(on.mean())
            r["c_bounce_shuffled"] = time_forms(plugin, d_c, n, d_hits, brt.QUERY_CLOSEST, 10, 30)
            r["d_any_on_c"] = time_forms(plugin, d_c, n, d_hits, brt.QUERY_ANY, 10, 30)
            r["e_pick_1"] = time_pick(plugin, ra[n // 2 + w // 2: n // 2 + w // 2 + 1], 10, 30)
            r["e_pick_64"] = time_pick(plugin, ra[perm[:64]], 10, 30)
            res[name] = r
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
