#!/usr/bin/env python3
"""Cost of irradiance volumes on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up and 30 timed calls
each, medians and min - max; cover scene, a 16^3 lattice:
  (a) brt_sample_volume_device over 1920 x 1080 points, both bases, with and without BRT_VOLUME_WRAP, for two lists: `gbuffer` (pixel
      (x, y) lies at (x, y) of a wavy sheet through the lattice: neighbouring points share their eight records) and `random` (uniform
      positions in the lattice's box grown by one cell: the least sharing a list can have);
  (b) the floor the kernel is read against: a plain device copy that moves the same 48 bytes per point (24 read, 24 written);
  (c) brt_bake_volume_device against brt_bake_probes_device over the same probes (256 directions, 8 bounces, SH9), which differ by one
      launch of k_volume_probes.
Prints one JSON document; --out writes it to a file (default profiles/volume/volume_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/volume_time.py --quick`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from probe_time import time_calls  # noqa: E402


def measure(warmup, timed, side, width, height, n_dirs, bounces):
    import numpy as np
    import torch

    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lo, hi = np.array((-6.0, 0.1, -6.0)), np.array((6.0, 3.0, 6.0))
    spacing = (hi - lo) / (side - 1)
    n_points = width * height
    rng = np.random.default_rng(7)
    lists = {}
    gx, gy = np.meshgrid(np.linspace(0.0, 1.0, width), np.linspace(0.0, 1.0, height))
    sheet = np.stack([lo[0] + gx * (hi[0] - lo[0]), lo[1] + (0.5 + 0.45 * np.sin(9.0 * gx) * np.cos(7.0 * gy)) * (hi[1] - lo[1]),
                      lo[2] + gy * (hi[2] - lo[2])], axis=-1).reshape(-1, 3)
    lists["gbuffer"] = sheet
    lists["random"] = rng.uniform(lo - spacing, hi + spacing, size=(n_points, 3))
    normals = rng.normal(size=(n_points, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    d_points = {}
    for name, pos in lists.items():
        pts = np.zeros(n_points, brt.VOLUME_POINT_DTYPE)
        pts["position"], pts["normal"] = pos, normals
        d_points[name] = torch.from_numpy(pts.view(np.uint8).reshape(-1)).cuda()
    d_out = torch.zeros(n_points * 16, dtype=torch.uint8, device="cuda")
    n_probes = side ** 3
    d_rec = {b: torch.zeros(n_probes * 128, dtype=torch.uint8, device="cuda") for b in (brt.PROBE_SH9, brt.PROBE_AMBIENT_CUBE)}
    res = {"side": side, "probes": n_probes, "points": n_points, "n_dirs": n_dirs, "bounces": bounces, "warmup": warmup, "timed": timed}

    def volume(basis, flags=0):
        return brt.make_volume(lo, spacing, (side, side, side), basis, 12345, flags)

    for basis in d_rec:
        node.bake_volume(volume(basis), n_dirs, bounces, d_records=d_rec[basis].data_ptr())
    torch.cuda.synchronize()
    # (a) the sampling kernel
    import hashlib
    for basis, bname in ((brt.PROBE_SH9, "sh9"), (brt.PROBE_AMBIENT_CUBE, "cube")):
        for flags, fname in ((0, "plain"), (brt.VOLUME_WRAP, "wrap")):
            vol = volume(basis, flags)
            for lname, d_pts in d_points.items():
                args = (vol, d_rec[basis].data_ptr(), (d_pts.data_ptr(), n_points, d_out.data_ptr()))
                node.sample_volume(*args, device=True)
                got = d_out.cpu().numpy().view(brt.VOLUME_SAMPLE_DTYPE)
                t = time_calls(lambda s: node.sample_volume(*args, device=True, stream=s), warmup, timed)
                t["clamped"] = float(np.mean((got["status"] & brt.VOLUME_STATUS_CLAMPED) != 0))
                t["mean_rgb"] = [float(x) for x in got["rgb"].mean(axis=0)]
                t["samples_sha"] = hashlib.sha256(got.tobytes()).hexdigest()[:16]
                t["bytes_per_ns"] = 48.0 * n_points / (t["median_ms"] * 1e6)
                res[f"sample_{bname}_{fname}_{lname}"] = t
    # (b) the floor: 24 bytes read and 24 written per point
    src = torch.zeros(n_points * 24, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n_points * 24, dtype=torch.uint8, device="cuda")
    res["copy_48_bytes_per_point"] = time_calls(lambda s: dst.copy_(src, non_blocking=True), warmup, timed)
    # (c) the bake against the bake of the same probes
    vol = volume(brt.PROBE_SH9)
    d_probes = torch.from_numpy(brt.volume_probes(vol).view(np.uint8).reshape(-1)).cuda()
    d_a = torch.zeros(n_probes * 128, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(n_probes * 128, dtype=torch.uint8, device="cuda")
    st = dict(node.bake_volume(vol, n_dirs, bounces, d_records=d_a.data_ptr()))
    node.bake_probes((d_probes.data_ptr(), n_probes, d_b.data_ptr()), n_dirs, bounces, brt.PROBE_SH9, device=True)
    torch.cuda.synchronize()
    assert d_a.cpu().numpy().tobytes() == d_b.cpu().numpy().tobytes()          # (the volume's bake is the bake of its probes)
    res["bake_stats"] = st
    bake_v = lambda s: node.bake_volume(vol, n_dirs, bounces, d_records=d_a.data_ptr(), stream=s)
    bake_p = lambda s: node.bake_probes((d_probes.data_ptr(), n_probes, d_b.data_ptr()), n_dirs, bounces, brt.PROBE_SH9, device=True, stream=s)
    res["bake_volume"] = time_calls(bake_v, warmup, timed)
    res["bake_probes"] = time_calls(bake_p, warmup, timed)
    res["bake_volume_again"] = time_calls(bake_v, warmup, timed)
    res["bake_volume_over_bake_probes"] = min(res["bake_volume"]["median_ms"], res["bake_volume_again"]["median_ms"]) / res["bake_probes"]["median_ms"]
    plugin.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--dirs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume", "volume_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (10, 30)
    doc = {"scene": "cover", **measure(warmup, timed, args.side, args.width, args.height, args.dirs, 8)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
