#!/usr/bin/env python3
"""Cost of a light-probe bake on one MI355X, timed with HIP events around the calls on a torch stream: 10 warm-up and 30 timed calls
each, medians; cover scene, a 16^3 lattice of probes x 256 directions, 8 bounces, SH9:
  (a) brt_bake_probes_device (generate -> radiance -> project in one call);
  (b) brt_radiance_rays_device with samples = 1 over the same list, generated beforehand by brt_probe_rays_device: what there was before;
  (c) the two new steps alone (brt_probe_rays_device, brt_probe_project_device).
The list layout (brt_probe.h kProbeLayout) is a constant of the build and a run reports the one it finds: for the other layout run again
with BRT_LIB_PATH set to a variant (scripts/build_variant.sh NAME "-DBRT_PROBE_LAYOUT=1"), then --merge the two documents.
Prints one JSON document; --out writes it to a file (default profiles/probes/probe_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/probe_time.py --quick`."""
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


def measure(warmup, timed, side, n_dirs, bounces):
    import numpy as np
    import torch

    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    g = [np.linspace(lo, hi, side) for lo, hi in ((-6.0, 6.0), (0.1, 3.0), (-6.0, 6.0))]
    probes = np.zeros(side ** 3, brt.PROBE_DTYPE)
    probes["position"] = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3)
    probes["seed"] = np.arange(len(probes), dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    n_probes, n = len(probes), len(probes) * n_dirs
    d_probes = torch.from_numpy(probes.view(np.uint8)).cuda()
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(n_probes * 128, dtype=torch.uint8, device="cuda")
    d_bake = torch.zeros(n_probes * 128, dtype=torch.uint8, device="cuda")
    pp, pr, ps, pc, pb = (t.data_ptr() for t in (d_probes, d_rays, d_res, d_rec, d_bake))
    # which layout this build generates: entry 1 of a 2 x 2 list is direction 1 of probe 0, or direction 0 of probe 1
    node.probe_rays_device(pp, 2, 2, pr)
    layout = "probe_major" if int(d_rays[:64].cpu().numpy().view(brt.RADIANCE_RAY_DTYPE)[1]["user"]) == 1 else "direction_major"
    node.probe_rays_device(pp, n_probes, n_dirs, pr)
    rad = dict(node.radiance_rays((pr, n, ps), 1, bounces, device=True))
    node.probe_project_device(ps, n_probes, n_dirs, brt.PROBE_SH9, pc)
    st = dict(node.bake_probes((pp, n_probes, pb), n_dirs, bounces, brt.PROBE_SH9, device=True))
    torch.cuda.synchronize()
    steps, bake = d_rec.cpu().numpy(), d_bake.cpu().numpy()
    assert steps.tobytes() == bake.tobytes()                     # (the one call is its three steps)
    res = {"layout": layout, "probes": n_probes, "n_dirs": n_dirs, "entries": n, "bounces": bounces, "basis": "SH9", "warmup": warmup,
           "timed": timed, "walks": st["walks"], "hit_entries": st["hits"], "radiance_form": st["form"], "chunks": st["chunks"],
           "records_sha": __import__("hashlib").sha256(bake.tobytes()).hexdigest()[:16]}
    assert (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])
    res["bake"] = time_calls(lambda s: node.bake_probes((pp, n_probes, pb), n_dirs, bounces, brt.PROBE_SH9, device=True, stream=s), warmup, timed)
    res["radiance_alone"] = time_calls(lambda s: node.radiance_rays((pr, n, ps), 1, bounces, device=True, stream=s), warmup, timed)
    res["generate_alone"] = time_calls(lambda s: node.probe_rays_device(pp, n_probes, n_dirs, pr, stream=s), warmup, timed)
    res["project_alone"] = time_calls(lambda s: node.probe_project_device(ps, n_probes, n_dirs, brt.PROBE_SH9, pc, stream=s), warmup, timed)
    res["bake_again"] = time_calls(lambda s: node.bake_probes((pp, n_probes, pb), n_dirs, bounces, brt.PROBE_SH9, device=True, stream=s), warmup, timed)
    res["bake_over_radiance"] = min(res["bake"]["median_ms"], res["bake_again"]["median_ms"]) / res["radiance_alone"]["median_ms"]
    plugin.close()
    return res


def merge(paths):
    """The documents of two runs (one per layout) as one; the records of both are the same bytes."""
    doc = {"scene": "cover"}
    for path in paths:
        with open(path) as f:
            one = json.load(f)
        one.pop("scene")
        assert not set(one) & set(doc), "two runs of the same layout"
        doc.update(one)
    assert doc["probe_major"]["records_sha"] == doc["direction_major"]["records_sha"]      # (the records do not depend on the layout)
    doc["bake_direction_major_over_probe_major"] = doc["direction_major"]["bake"]["median_ms"] / doc["probe_major"]["bake"]["median_ms"]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 warm-up and 3 timed calls (for a profiler run)")
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--dirs", type=int, default=256)
    ap.add_argument("--merge", nargs=2, metavar="JSON", help="no measurement: the documents of two runs, one per layout, as one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes", "probe_time.json"))
    args = ap.parse_args()
    if args.merge:
        doc = merge(args.merge)
    else:
        warmup, timed = (2, 3) if args.quick else (10, 30)
        one = measure(warmup, timed, args.side, args.dirs, 8)
        doc = {"scene": "cover", one["layout"]: one}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
