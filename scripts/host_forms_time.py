#!/usr/bin/env python3
"""Cost of the host-buffer forms on one MI355X: wall time around the whole synchronous call (the copies in, the kernels, the copies
out), warm-up calls first so that no first allocation is counted, then timed calls; median (min .. max) ms.  One series per export
that stages a caller's host buffers, the cover scene, each at the shape its family's own script times the device form at:
  query_rays          the pixel-centre rays of a 1920x1080 frame (query_time.py (a))
  radiance_rays       the same rays, 16 samples, 8 bounces (radiance_time.py (a))
  sample_volume       1920 x 1080 random points in a 16^3 lattice, SH9 (volume_time.py (a))
  bake_probes         the 16^3 lattice's probes x 256 directions, 8 bounces, SH9 (probe_time.py (a))
  bake_lightmap       the 256 x 128 chart of a unit sphere, 256 directions, 8 bounces, 4 passes, with the info plane (lightmap_time.py (a))
  render_pixels       every pixel of the 1920x1080 frame in raster order, 64 spp, 8 bounces (lens_time.py pixels_identity)
  progressive_sample  the whole-frame pass of a zeroed 1920x1080 state plane to 8 samples, with a frame (progressive_time.py (a))
  render_progressive  the one-call form at the defaults, from a zeroed state plane (progressive_time.py (b))
  render_gbuffer      all five planes at 1920x1080 against an orbited previous camera (gbuffer_time.py (a))
For a comparison of two builds run it once per build and process, the builds alternating: BRT_LIB_PATH=<library> python
scripts/host_forms_time.py --out <file>.  Prints one JSON document; --out writes it to a file."""
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
from query_time import pixel_rays  # noqa: E402

W, H = 1920, 1080
HEAVY = ("radiance_rays", "bake_probes", "bake_lightmap", "render_pixels", "render_progressive")     # (fewer calls: --heavy)


def time_calls(call, warmup, timed):
    ms = []
    for i in range(warmup + timed):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "calls": timed}


def series(plugin):
    """-> [(name, call)]"""
    node = plugin.node
    rng = np.random.default_rng(5)
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    node.write_buffers(b)                                                   # (the caller's tree: it serves every origin)
    lvl, cam, win = brt.cover_camera(W, H, 4, 8, brt.Raytracing.Pure, 0.5)
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    node.render_device(lvl, cam, win, W, H, frame.data_ptr())              # (the resident numbering is the steady-state one)
    rays = pixel_rays(cam, win, W, H)
    rrays = np.zeros(len(rays), brt.RADIANCE_RAY_DTYPE)
    rrays["origin"], rrays["direction"], rrays["user"] = rays["origin"], rays["direction"], rays["user"]
    rrays["seed"] = rng.integers(0, 2 ** 32, len(rays), dtype=np.uint32)
    volume = brt.make_volume((-8.0, 0.25, -8.0), (1.0, 0.5, 1.0), (16, 16, 16), brt.PROBE_SH9, 7, 0)
    probes = brt.volume_probes(volume)
    records = node.bake_volume(volume, 16, 2)
    points = np.zeros(W * H, brt.VOLUME_POINT_DTYPE)
    points["position"] = rng.uniform((-9.0, -0.25, -9.0), (8.0, 8.25, 8.0), (W * H, 3)).astype(np.float32)
    nrm = rng.standard_normal((W * H, 3))
    points["normal"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    unit = int(np.flatnonzero(b.models["radius"] == np.float32(1.0))[0])
    chart = brt.lightmap_sphere_points(b.models["position"][unit], 1.0, 256, 128, seed=3, offset=1e-3)
    cam64 = brt.cover_camera(W, H, 64, 8, brt.Raytracing.Pure, 0.5)[1]
    every = np.arange(W * H, dtype=np.uint32)
    state = np.zeros((H, W), brt.PROG_PIXEL_DTYPE)
    out = np.zeros((H, W, 4), np.float32)
    desc = brt.gbuffer()
    prev_cam = brt.cover_camera(W, H, 4, 8, brt.Raytracing.Pure, 0.25)[1]
    prev_cam["position"][0][:3] += np.float32(0.05)
    planes = {k: brt.gbuffer_plane(desc, k, W, H) for k in brt.GBUFFER_PLANES}

    def zeroed(call):
        def run():
            state.view(np.uint8)[...] = 0
            call()
        return run
    return [
        ("query_rays", lambda: node.query_rays(rays)),
        ("radiance_rays", lambda: node.radiance_rays(rrays, 16, 8)),
        ("sample_volume", lambda: node.sample_volume(volume, records, points)),
        ("bake_probes", lambda: node.bake_probes(probes, 256, 8)),
        ("bake_lightmap", lambda: node.bake_lightmap(chart, 256, 8, passes=4)),
        ("render_pixels", lambda: node.render_pixels(cam64, win, W, H, every)),
        ("progressive_sample", zeroed(lambda: node.progressive_sample(cam, win, W, H, state, 8, frame=out))),
        ("render_progressive", zeroed(lambda: node.render_progressive(cam, win, W, H, state, out))),
        ("render_gbuffer", lambda: node.render_gbuffer(cam, win, W, H, desc, prev_camera=prev_cam, into=planes)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timed", type=int, default=15)
    ap.add_argument("--heavy", type=int, nargs=2, default=(2, 8), metavar=("WARMUP", "TIMED"), help="of the series that trace for long")
    ap.add_argument("--only", default=None, help="comma-separated series")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash(), "unit": "ms of wall time per call",
           "series": {}}
    with brt.RaytracePlugin([0]) as plugin:
        for name, call in series(plugin):
            if a.only and name not in a.only.split(","):
                continue
            res["series"][name] = time_calls(call, *(a.heavy if name in HEAVY else (a.warmup, a.timed)))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
