#!/usr/bin/env python3
"""Are the kernels of two builds of one .hip file the same instructions?  Takes two device assembly files
(hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> -S --cuda-device-only -o X.s X.hip, e.g. of a parent checkout and of this tree)
and prints, per kernel of the first, SAME, REGS or DIFF with the instruction counts (gone: the second has no such kernel); kernels only the second has
are listed as new.  REGS: not the same, but as many instructions, the same mnemonics and the same operands wherever an operand is no
register, and the same "Kernel info" block behind the kernel (the figures -Rpass-analysis=kernel-resource-usage prints: registers,
scratch, LDS, occupancy): the register allocator named the same values differently.  Comments,
directives and the numbering of local labels are ignored; an empty template parameter pack in a mangled name counts as no pack (the
instantiation of a kernel template that gained an optional trailing argument), and a seventh argument `false` of k_trace_persistent
counts as no argument (the template lost that parameter; its `true` instantiation has no namesake and is reported missing), and
k_trace_pixels_{plain,stream}<...> and k_lens_{plain,stream}<LENS, ...> count as their namesakes k_list_*<PinholeStart, ...> and
k_list_*<LensStart<LENS>, ..., LensView> (the two families became one pair of templates under a start rule), and k_prog_plain<D16> and
k_prog_stream<MODE, D16, SIMPLE> as k_list_*<ProgStart, ..., ProgSample> (the progressive kernels became a third rule of that pair).  Exit
status 1 if a kernel is DIFF or missing."""
import re
import sys


REG = re.compile(r"\b[vsa](?:\d+|\[\d+:\d+\])|\bvcc(?:_lo|_hi)?\b")


def kernels(path, info=None):
    """kernel -> its instructions; info (if given): kernel -> the lines of the "Kernel info" block behind it"""
    out, cur, last, block = {}, None, None, None
    for ln in open(path):
        if ln.startswith("; Kernel info:") and info is not None:
            block = info.setdefault(last, [])
            continue
        if block is not None:
            if ln.startswith("; "):
                block.append(ln.strip())
                continue
            block = None
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = re.sub(r"DpT\d_", "", m.group(1).replace("EJEEEv", "EEEv"))
            cur = re.sub(r"(k_trace_persistentI(?:L[ib]\dE){6})Lb0E(EEv)", r"\1\2", cur)
            cur = re.sub(r"\d\dk_trace_pixels_(plain|stream)I", lambda g: f"{len(g.group(1)) + 7}k_list_{g.group(1)}INS_12PinholeStartE", cur)
            cur = re.sub(r"k_lens_(plain|stream)I(Lj\dE)((?:L[ib]\dE)+)EEv(\w+)NS_8LensViewE$", r"k_list_\1INS_9LensStartI\2EE\3JNS_8LensViewEEEEv\4", cur)
            cur = re.sub(r"12_GLOBAL__N_1\d\dk_prog_(plain|stream)I((?:L[ib]\dE)+)EEv(\w+)NS_10ProgSampleE$",
                         lambda g: f"{len(g.group(1)) + 7}k_list_{g.group(1)}INS_9ProgStartE{g.group(2)}JNS_10ProgSampleEEEEv{g.group(3)}", cur)
            out[cur] = []
            last = cur
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            s = ln.split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):
                out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    ia, ib = {}, {}
    a, b = kernels(sys.argv[1], ia), kernels(sys.argv[2], ib)
    bad = 0
    for k, body in a.items():
        same = body == b.get(k)
        regs = not same and k in b and ia.get(k) == ib.get(k) and [REG.sub("r", x) for x in body] == [REG.sub("r", x) for x in b[k]]
        bad += not (same or regs)
        print(f"{'SAME' if same else 'REGS' if regs else 'DIFF' if k in b else 'gone'} {len(body):6d} {len(b.get(k, [])):6d}  {k}")
    for k in b:
        if k not in a:
            print(f"new  {'':6s} {len(b[k]):6d}  {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
