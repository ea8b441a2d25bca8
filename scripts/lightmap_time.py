#!/usr/bin/env python3
"""Cost of a lightmap bake on one MI355X, timed with HIP events around the calls on a torch stream: 5 warm-up and 15 timed calls each,
medians; cover scene, the 256 x 128 latitude-longitude chart of one of its unit spheres, 256 directions, 8 bounces, 4 passes:
  (a) brt_bake_lightmap_device (per chunk generate -> radiance -> resolve, then the passes, in one call);
  (b) brt_radiance_rays_device over the same entry list, generated beforehand by brt_lightmap_rays_device: what there was before;
  (c) the steps alone: generate, resolve, and 8 dilation passes over a 1024 x 1024 image beside a device copy of the bytes one pass
      reads and writes at least (source image + destination image).
Prints one JSON document; --out writes it to a file (default profiles/lightmap/lightmap_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/lightmap_time.py --quick`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_calls(call, warmup, timed):
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
            call(s.cuda_stream)
            ev[1].record(s)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def measure(warmup, timed, width, height, n_dirs, bounces, passes, big, big_passes):
    import hashlib

    import numpy as np
    import torch

    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    node.write_buffers(b)
    i = int(np.flatnonzero(b.models["radius"] == np.float32(1.0))[0])
    pts = brt.lightmap_sphere_points(b.models["position"][i], 1.0, width, height, seed=12345, offset=1e-3)
    n = width * height

    def zeros(n_bytes):
        return torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")

    d_pts = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy()).cuda()
    d_rays, d_res = zeros(n * n_dirs * 32), zeros(n * n_dirs * 32)
    d_img, d_steps, d_bake, d_info = zeros(n * 16), zeros(n * 16), zeros(n * 16), zeros(n * 8)
    pp, pr, ps, pi, pc, pb, pn = (t.data_ptr() for t in (d_pts, d_rays, d_res, d_img, d_steps, d_bake, d_info))

    node.lightmap_rays_device(pp, n, n_dirs, pr)
    rad = dict(node.radiance_rays((pr, n * n_dirs, ps), 1, bounces, device=True))
    node.lightmap_resolve_device(ps, pp, n, n_dirs, pi)
    node.lightmap_dilate_device(pi, width, height, passes, True, pc)
    st = dict(node.bake_lightmap((pp, width, height, pb, pn), n_dirs, bounces, passes, True, device=True))
    torch.cuda.synchronize()
    steps, bake = d_steps.cpu().numpy(), d_bake.cpu().numpy()
    assert steps.tobytes() == bake.tobytes()                     # (the one call is its steps)
    assert (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])
    res = {"scene": "cover", "width": width, "height": height, "n_dirs": n_dirs, "entries": n * n_dirs, "bounces": bounces, "passes": passes,
           "warmup": warmup, "timed": timed, "walks": st["walks"], "hit_entries": st["hits"], "radiance_form": st["form"],
           "chunks": st["chunks"], "image_sha": hashlib.sha256(bake.tobytes()).hexdigest()[:16]}
    bake_call = lambda s: node.bake_lightmap((pp, width, height, pb, pn), n_dirs, bounces, passes, True, device=True, stream=s)
    res["bake"] = time_calls(bake_call, warmup, timed)
    res["radiance_alone"] = time_calls(lambda s: node.radiance_rays((pr, n * n_dirs, ps), 1, bounces, device=True, stream=s), warmup, timed)
    res["generate_alone"] = time_calls(lambda s: node.lightmap_rays_device(pp, n, n_dirs, pr, stream=s), warmup, timed)
    res["resolve_alone"] = time_calls(lambda s: node.lightmap_resolve_device(ps, pp, n, n_dirs, pi, stream=s), warmup, timed)
    res["dilate_alone"] = time_calls(lambda s: node.lightmap_dilate_device(pi, width, height, passes, True, pc, stream=s), warmup, timed)
    res["bake_again"] = time_calls(bake_call, warmup, timed)
    res["bake_over_radiance"] = min(res["bake"]["median_ms"], res["bake_again"]["median_ms"]) / res["radiance_alone"]["median_ms"]
    # the passes at a texture's size: a checkerboard of 8 x 8 charts, so that half the texels gather
    yy, xx = np.mgrid[0:big, 0:big]
    atlas = np.random.default_rng(5).uniform(0, 1, size=(big, big, 4)).astype(np.float32)
    atlas[..., 3] = ((xx // 8 + yy // 8) % 2).astype(np.float32)
    d_a, d_o, d_c = torch.from_numpy(atlas.view(np.uint8).reshape(-1)).cuda(), zeros(big * big * 16), zeros(big * big * 16)
    res["dilate_big"] = {"size": big, "passes": big_passes, "bytes_moved_per_pass": 2 * big * big * 16,
                         "passes_time": time_calls(lambda s: node.lightmap_dilate_device(d_a.data_ptr(), big, big, big_passes, False, d_o.data_ptr(), stream=s), warmup, timed),
                         "device_copy_of_one_image": time_calls(lambda s: d_c.copy_(d_a, non_blocking=True), warmup, timed)}
    res["dilate_big"]["pass_over_copy"] = res["dilate_big"]["passes_time"]["median_ms"] / big_passes / res["dilate_big"]["device_copy_of_one_image"]["median_ms"]
    plugin.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--dirs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap", "lightmap_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (5, 15)
    doc = measure(warmup, timed, args.width, args.height, args.dirs, 8, 4, 1024, 8)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
