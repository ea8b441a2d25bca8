#!/usr/bin/env python3
"""Cost of a reflection-probe bake on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up and 30 timed
calls each, medians; cover scene, a 256 x 256 x 6 cube with its 9 levels, 1 sample, 8 bounces, 64 taps:
  (a) brt_bake_envmap_device (generate -> radiance -> resolve, then per level box -> filter, in one call);
  (b) brt_radiance_rays_device over the same list, generated beforehand by brt_envmap_rays_device: what there was before;
  (c) the steps alone: generate, resolve, and per level the box kernel and k_envmap_filter, the filter beside a device copy of the
      bytes it reads and writes (source cube + table + destination cube).
Prints one JSON document; --out writes it to a file (default profiles/envmap/envmap_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/envmap_time.py --quick`."""
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


def measure(warmup, timed, size, samples, bounces, n_taps):
    import hashlib

    import numpy as np
    import torch

    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    position, seed = (2.5, 1.5, 3.5), 12345
    levels = size.bit_length()
    offs = brt.envmap_level_offsets(size, levels)
    n = offs[1]
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(offs[-1] * 16, dtype=torch.uint8, device="cuda")
    d_bake = torch.zeros(offs[-1] * 16, dtype=torch.uint8, device="cuda")
    d_box = [None] + [torch.zeros(6 * (size >> l) ** 2 * 16, dtype=torch.uint8, device="cuda") for l in range(1, levels)]
    d_taps = [None] + [torch.from_numpy(brt.envmap_taps(brt.ENVMAP_TAPS_GGX, np.float32(l) / np.float32(levels - 1), n_taps).view(np.uint8).reshape(-1)).cuda()
                       for l in range(1, levels)]
    pr, ps, pc, pb = (t.data_ptr() for t in (d_rays, d_res, d_steps, d_bake))

    def box_of(l):
        return pc if l == 0 else d_box[l].data_ptr()

    node.envmap_rays_device(position, seed, size, pr)
    rad = dict(node.radiance_rays((pr, n, ps), samples, bounces, device=True))
    node.envmap_resolve_device(ps, size, pc)
    for l in range(1, levels):
        node.envmap_downsample_device(box_of(l - 1), size >> (l - 1), box_of(l))
        node.envmap_filter_device(box_of(l), size >> l, d_taps[l].data_ptr(), n_taps, size >> l, pc + offs[l] * 16)
    st = dict(node.bake_envmap(position, size, levels, samples, bounces, n_taps, seed, d_out=pb))
    torch.cuda.synchronize()
    steps, bake = d_steps.cpu().numpy(), d_bake.cpu().numpy()
    assert steps.tobytes() == bake.tobytes()                     # (the one call is its steps)
    assert (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])
    res = {"scene": "cover", "size": size, "levels": levels, "texels": n, "samples": samples, "bounces": bounces, "n_taps": n_taps,
           "warmup": warmup, "timed": timed, "walks": st["walks"], "hit_entries": st["hits"], "radiance_form": st["form"],
           "chunks": st["chunks"], "chain_sha": hashlib.sha256(bake.tobytes()).hexdigest()[:16]}
    bake_call = lambda s: node.bake_envmap(position, size, levels, samples, bounces, n_taps, seed, d_out=pb, stream=s)
    res["bake"] = time_calls(bake_call, warmup, timed)
    res["radiance_alone"] = time_calls(lambda s: node.radiance_rays((pr, n, ps), samples, bounces, device=True, stream=s), warmup, timed)
    res["generate_alone"] = time_calls(lambda s: node.envmap_rays_device(position, seed, size, pr, stream=s), warmup, timed)
    res["resolve_alone"] = time_calls(lambda s: node.envmap_resolve_device(ps, size, pc, stream=s), warmup, timed)
    res["filter_levels"] = []
    for l in range(1, levels):
        s_l = size >> l
        moved = 2 * 6 * s_l * s_l * 16 + n_taps * 16                 # source cube + destination cube + table
        d_a = torch.zeros(moved, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(moved, dtype=torch.uint8, device="cuda")

        def copy(s, a=d_a, b=d_b):
            b.copy_(a, non_blocking=True)                           # (on the current stream: time_calls made it current)

        one = {"level": l, "edge": s_l, "bytes_moved": moved,
               "downsample": time_calls(lambda s, l=l: node.envmap_downsample_device(box_of(l - 1), size >> (l - 1), box_of(l), stream=s), warmup, timed),
               "filter": time_calls(lambda s, l=l, s_l=s_l: node.envmap_filter_device(box_of(l), s_l, d_taps[l].data_ptr(), n_taps, s_l, pc + offs[l] * 16, stream=s), warmup, timed),
               "device_copy_of_its_bytes": time_calls(copy, warmup, timed)}
        one["filter_over_copy"] = one["filter"]["median_ms"] / one["device_copy_of_its_bytes"]["median_ms"]
        res["filter_levels"].append(one)
    res["bake_again"] = time_calls(bake_call, warmup, timed)
    res["bake_over_radiance"] = min(res["bake"]["median_ms"], res["bake_again"]["median_ms"]) / res["radiance_alone"]["median_ms"]
    plugin.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--taps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envmap", "envmap_time.json"))
    args = ap.parse_args()
    warmup, timed = (2, 3) if args.quick else (10, 30)
    doc = measure(warmup, timed, args.size, 1, 8, args.taps)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
