#!/usr/bin/env python3
"""Drives each of the twelve device entry points on a whole frame behind the tracer once -- post-passes, upsampling, adaptive sampling;
the blended calls at levels 1 and 2 -- on the three-sphere scene of tests/post_refusal_cases.py, 8x4 low and 16x8 full, on the context's
own stream or on a stream of the caller's, and prints one line per call with the CRC of everything the calls have written so far.  For
comparing the work of two builds (BRT_LIB_PATH selects the library), one fresh process per run:

  rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python scripts/post_plumbing_drive.py --stream own|caller
  python scripts/post_plumbing_drive.py --list DIR/.../NAME_kernel_trace.csv      # kernel (without its argument list), grid, block per dispatch, in order

profiles/post_plumbing/kernel_sequence.txt holds the lists of the commit before the entry points were folded onto one skeleton and of
the fold, and their (empty) difference."""
import argparse
import csv
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _without_arguments(name):
    """a demangled kernel name without its trailing argument list (the template arguments stay; list_trace keeps 160 characters)"""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def list_trace(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print(_without_arguments(r["Kernel_Name"])[:160], "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], "block", r["Workgroup_Size_X"],
              r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])


def drive(stream_kind):
    import torch

    import bevyray_amd as brt
    import post_refusal_cases as prc
    from bevyray_amd import _lib

    arena = torch.zeros(prc.ARENA_BYTES, dtype=torch.uint8, device="cuda")
    arena[:prc.ARENA["depth"][0]] = torch.arange(prc.ARENA["depth"][0], device="cuda") % 61       # (inputs that are no zeros; finite as f32)
    syms, _keep = prc.symbols(arena.data_ptr(), spp=16)                     # (above the default base_spp: adaptive sampling selects)
    stream = torch.cuda.Stream() if stream_kind == "caller" else None
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(prc.scene())
        for export, entry in prc.TABLE.items():
            names = [k for k, _ in entry["base"]]
            for level in ((1, 2) if "level" in names else (None,)):
                args = dict(entry["base"], ctx=p._ctx)
                if level is not None:
                    args["level"] = level
                if stream is not None:
                    args["stream"], args["flags"] = stream.cuda_stream, brt.FLAG_CALLER_STREAM
                _lib.check(getattr(p._lib, export)(*[v if k == "ctx" or not isinstance(v, str) else syms[v] for k, v in args.items()]), p._ctx)
                torch.cuda.synchronize()
                print(export, "" if level is None else f"level {level}", f"crc {zlib.crc32(arena.cpu().numpy().tobytes()):08x}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", choices=("own", "caller"), default="own")
    ap.add_argument("--list", default=None, help="print the kernel list of a rocprofv3 kernel trace (csv) instead of driving anything")
    a = ap.parse_args()
    if a.list:
        list_trace(a.list)
    else:
        drive(a.stream)


if __name__ == "__main__":
    main()
