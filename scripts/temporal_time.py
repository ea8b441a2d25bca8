#!/usr/bin/env python3
"""Cost of the temporal accumulation on one MI355X: brt_denoise_device on a rendered 1920x1080 cover-scene frame
at 4 spp, timed with HIP events around the call on a torch stream, 10 warm-up and 30 timed calls per setting, for FLAG_DENOISE,
FLAG_DENOISE | FLAG_TEMPORAL and FLAG_TEMPORAL alone, on a still camera (one frame, the history converges) and on a slow orbit (a new
camera and frame every call, 0.05 degrees per frame).  Writes profiles/temporal/temporal_time.json (--out to change) and prints it.
Per-kernel split: run this under `rocprofv3 --kernel-trace --stats -- python scripts/temporal_time.py --quick`."""
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
from helpers import uniforms  # noqa: E402

MODES = {"denoise": brt.FLAG_DENOISE, "denoise_temporal": brt.FLAG_DENOISE | brt.FLAG_TEMPORAL, "temporal": brt.FLAG_TEMPORAL}


def orbit(w, h, i, step_deg=0.05):
    a = np.radians(step_deg * i)
    x, z = 13.0 * np.cos(a) - 3.0 * np.sin(a), 13.0 * np.sin(a) + 3.0 * np.cos(a)
    return uniforms(w, h, 4, 8, (float(x), 2.0, float(z)), (0.0, 0.0, 0.0), 0.4, 0.5 + 0.0371 * i)


def time_calls(plugin, views, frames, out, flags, warmup, timed):
    """views[i], frames[i]: the camera / window and the rendered frame of call i (one of each: a still camera)."""
    plugin.reset_temporal()
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    with torch.cuda.stream(s):
        for i in range(warmup + timed):
            cam, win = views[i % len(views)]
            d_in = frames[i % len(frames)]
            ev[0].record(s)
            plugin.node.denoise_device(cam, win, out.shape[1], out.shape[0], d_in.data_ptr(), out.data_ptr(), stream=s.cuda_stream,
                                       flags=flags)
            ev[1].record(s)
            ev[1].synchronize()
            if i >= warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "temporal_time.json"))
    ap.add_argument("--quick", action="store_true", help="still camera only, nothing written (for the rocprofv3 kernel split)")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernel_code_hash": brt._lib.kernel_code_hash(), "calls": "10 warm-up + 30 timed"}
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 1920, 1080
    res["size"] = [w, h]
    with brt.RaytracePlugin([0]) as plugin:
        plugin.node.write_buffers(b)
        lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
        still = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        plugin.node.render_device(lvl, cam, win, w, h, still.data_ptr())
        out = torch.empty_like(still)
        cases = {"still": ([(cam, win)], [still])}
        if not a.quick:
            views, frames = [], []
            for i in range(40):
                lo, co, wo = orbit(w, h, i)
                f = torch.empty_like(still)
                plugin.node.render_device(lo, co, wo, w, h, f.data_ptr())
                views.append((co, wo))
                frames.append(f)
            cases["orbit"] = (views, frames)
        for case, (views, frames) in cases.items():
            res[case] = {m: time_calls(plugin, views, frames, out, f, 10, 30) for m, f in MODES.items()}
            st = plugin.debug_temporal_state(w, h)           # (after the last "temporal" call)
            n = st[..., 3]
            res[case]["history_after_40_calls"] = {"n_median": float(np.median(n[n > 0])), "rejected_fraction": float(np.isnan(st[..., 6]).mean())}
    text = json.dumps(res, indent=1)
    print(text)
    if not a.quick:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
