#!/usr/bin/env python3
"""Are the kernels of two builds of one .hip file the same instructions?  Takes two device assembly files
(hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> -S --cuda-device-only -o X.s X.hip, e.g. of a parent checkout and of this tree)
and prints, per kernel of the first, SAME or DIFF with the instruction counts (gone: the second has no such kernel); kernels only the second has
are listed as new.  Comments,
directives and the numbering of local labels are ignored; an empty template parameter pack in a mangled name counts as no pack (the
instantiation of a kernel template that gained an optional trailing argument), and a seventh argument `false` of k_trace_persistent
counts as no argument (the template lost that parameter; its `true` instantiation has no namesake and is reported missing).  Exit
status 1 if a kernel differs or is missing."""
import re
import sys


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1).replace("EJEEEv", "EEEv").replace("DpT1_", "")
            cur = re.sub(r"(k_trace_persistentI(?:L[ib]\dE){6})Lb0E(EEv)", r"\1\2", cur)
            out[cur] = []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            s = ln.split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):
                out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k, body in a.items():
        same = body == b.get(k)
        bad += not same
        print(f"{'SAME' if same else 'DIFF' if k in b else 'gone'} {len(body):6d} {len(b.get(k, [])):6d}  {k}")
    for k in b:
        if k not in a:
            print(f"new  {'':6s} {len(b[k]):6d}  {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
