#!/usr/bin/env python3
"""The child process of tests/test_hand_loops_gpu.py and tests/test_shade_production_gpu.py: renders every case of a case module -- its
second argument, tests/hand_loops_cases.py by default; a module has SMALL, LARGE, MODES, SMALL_FRAMES, LARGE_FRAMES and large_size -- in
the library that BRT_LIB_PATH names -- the -DBRT_ASM_COUNT build, in which the hand-written loops count their own executions and active
lanes -- and writes what it saw to the directory given as its first argument:
    records.json        case / mode / frame -> {stats (last_stats of the production launch), asm and order (last_asm_counts and
                        last_order_meta of that launch),
                        counting (last_stats of the FLAG_COUNTERS frame that follows it), profile (its debug_profile())}
    frames.npz          the production frames of the small cases under the same keys
    <case>.npy          the recorded (third) production frame of a large case
It asserts nothing: the parent does.  A HIP error raises out of the binding and ends the process with a non-zero status.
    BRT_LIB_PATH=ab/libasmcount.so python tests/tools/hand_loops_child.py OUT_DIR [CASE_MODULE]"""
import importlib
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import bevyray_amd as brt  # noqa: E402


def _record(p, lvl, cam, win, w, h):
    """What the production launch that has just run left behind, then a counting frame of the same view (the compiler's loops)."""
    stats = dict(p.node.last_stats)
    p.debug_profile()
    asm = dict(p.last_asm_counts)
    order = dict(p.last_order_meta)
    p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    counting = dict(p.node.last_stats)
    profile = p.debug_profile()
    return {"stats": stats, "asm": asm, "order": order, "counting": counting, "profile": profile}


def main():
    out_dir = sys.argv[1]
    hl = importlib.import_module(sys.argv[2] if len(sys.argv) > 2 else "hand_loops_cases")
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    records, frames = {"lib": os.environ.get("BRT_LIB_PATH", ""), "n_cus": n_cus}, {}
    with brt.RaytracePlugin([0]) as p:
        for name, make in hl.SMALL.items():
            b, lvl, cam, win, w, h, knobs = make()
            for mode, extra in hl.MODES.items():
                with p.tuning(**knobs, **extra):
                    for frame in range(hl.SMALL_FRAMES):
                        got = p.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
                        key = f"{name}/{mode}/{frame}"
                        frames[key] = np.array(got, np.float32)
                        records[key] = _record(p, lvl, cam, win, w, h)
        w, h = hl.large_size(n_cus)
        for name, (make, _) in hl.LARGE.items():
            b, lvl, cam, win, w, h, knobs = make(w, h)
            with p.tuning(**knobs):
                for frame in range(hl.LARGE_FRAMES):
                    got = p.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
                np.save(os.path.join(out_dir, f"{name}.npy"), np.asarray(got, np.float32))
                records[f"{name}/production/{hl.LARGE_FRAMES - 1}"] = _record(p, lvl, cam, win, w, h)
            print(name, flush=True)
    np.savez(os.path.join(out_dir, "frames.npz"), **frames)
    with open(os.path.join(out_dir, "records.json"), "w") as f:
        json.dump(records, f)
    print(f"{len(records) - 2} records", flush=True)


if __name__ == "__main__":
    main()
