#!/usr/bin/env python3
"""Cost of a lens frame on one MI355X, timed with HIP events around the calls on a torch stream (warm-up calls, then timed ones;
medians and the spread): the cover scene at 1920 x 1080, 64 spp, 8 bounces.
  pixels_identity   brt_render_pixels_device over the list of every pixel in raster order: the nearest kernel there was before.  With
                    --baseline-root DIR (a checkout of the parent commit with its library built) it is also timed on that build, in
                    processes of their own, in turn with this tree's: pixels_identity_baseline.
  render_device     brt_render_device, the persistent kernel, for scale.
  lens_r0           brt_render_lens_device at radius 0 (the same frame as the two above, bit for bit -- checked);
  lens_r0.05, lens_r0.5   ... with the book's aperture and a wide one, focused on the cover target;
  lens_ortho        ... with an orthographic camera that shows about the same part of the scene;
  *_plain           the same under BRT_FLAG_KERNEL_SIMPLE (the one-thread-per-pixel form), with --plain.
Prints one JSON document; --out writes it to a file (default profiles/lens/lens_time.json).  Per-kernel split: run this under
`rocprofv3 --kernel-trace --stats -- python scripts/lens_time.py --quick`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--root DIR, the child processes of --baseline-root: the package of another checkout)
sys.path.insert(0, sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT)


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


def measure(warmup, timed, w, h, spp, bounces, only_pixels, plain):
    """The rows of one process (one library: BRT_LIB_PATH, else this tree's)"""
    import numpy as np
    import torch

    import bevyray_amd as brt
    plugin = brt.RaytracePlugin([0])
    node = plugin.node
    node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces)
    n = w * h
    d_px = torch.arange(n, dtype=torch.int32, device="cuda")
    frames = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    res = {"rays": int(node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, frames[0].data_ptr())["rays"])}
    res["pixels_identity"] = time_calls(lambda s: node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, frames[0].data_ptr(), stream=s), warmup, timed)
    if only_pixels:
        plugin.close()
        return res
    res["render_device"] = time_calls(lambda s: node.render_device(lvl, cam, win, w, h, frames[1].data_ptr(), stream=s), warmup, timed)
    focus = float(np.sqrt(np.float32(182.0)))
    ortho = cam.copy()
    ortho["projection"] = 1
    # the perspective view is 2 tan(0.2) * 13.5 = 5.5 units high at the target
    views = {"lens_r0": (cam, brt.lens(0.0)), "lens_r0.05": (cam, brt.lens(0.05, focus)), "lens_r0.5": (cam, brt.lens(0.5, focus)),
             "lens_ortho": (ortho, brt.lens(0.0, 1.0, 5.5))}
    for name, (c, lens) in views.items():
        for flags, tag in ((0, ""), (brt.FLAG_KERNEL_SIMPLE, "_plain"))[:2 if plain else 1]:
            st = dict(node.render_lens_device(c, win, lens, w, h, frames[2].data_ptr(), flags=flags))
            res[name + tag] = time_calls(lambda s, c=c, lens=lens, flags=flags: node.render_lens_device(c, win, lens, w, h, frames[2].data_ptr(), stream=s, flags=flags),
                                         warmup, timed)
            res[name + tag].update(rays=int(st["rays"]), kernel_variant=st["kernel_variant"], scene_in_lds=st["scene_in_lds"],
                                   n_workgroups=st["n_workgroups"], threads_per_workgroup=st["threads_per_workgroup"])
            if name == "lens_r0":
                torch.cuda.synchronize()
                assert torch.equal(frames[2].view(torch.int32), frames[0].view(torch.int32)), "the radius-0 lens frame is not the pixel tracer's"
    res["pixels_identity_again"] = time_calls(lambda s: node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, frames[0].data_ptr(), stream=s), warmup, timed)
    plugin.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1 warm-up and 2 timed calls (for a profiler run)")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--plain", action="store_true", help="also time the plain form of every lens row")
    ap.add_argument("--baseline-root", help="a built checkout of the parent commit: its pixels_identity, in processes of their own, in turn with this tree's")
    ap.add_argument("--root", help="(the child processes of --baseline-root) the checkout whose package is imported")
    ap.add_argument("--rounds", type=int, default=2, help="processes per library of the baseline comparison")
    ap.add_argument("--only-pixels", action="store_true", help="(the child processes of --baseline-root) pixels_identity alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens", "lens_time.json"))
    args = ap.parse_args()
    warmup, timed = (1, 2) if args.quick else (5, 30)
    w, h = (int(x) for x in args.size.split("x"))
    if args.only_pixels:
        print(json.dumps(measure(warmup, timed, w, h, args.spp, args.bounces, True, False)))
        return
    doc = {"scene": "cover", "width": w, "height": h, "spp": args.spp, "bounces": args.bounces, "warmup": warmup, "timed": timed}
    if args.baseline_root:
        # one build per process (the library is chosen at import): parent, this tree, parent, this tree, ...
        rows = {"pixels_identity_baseline": [], "pixels_identity_this_tree": []}
        for _ in range(args.rounds):
            for key, root in (("pixels_identity_baseline", os.path.abspath(args.baseline_root)), ("pixels_identity_this_tree", ROOT)):
                env = dict(os.environ, BRT_LIB_PATH=os.path.join(root, "bevyray_amd", "libbevyray_amd.so"))
                cmd = [sys.executable, os.path.abspath(__file__), "--only-pixels", "--root", root, "--size", args.size, "--spp", str(args.spp),
                       "--bounces", str(args.bounces)]
                out = subprocess.run(cmd + (["--quick"] if args.quick else []), env=env, capture_output=True, text=True, check=True, timeout=600).stdout
                rows[key].append(json.loads(out.strip().splitlines()[-1])["pixels_identity"])
        doc.update(rows)
    doc.update(measure(warmup, timed, w, h, args.spp, args.bounces, False, args.plain))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
