#!/usr/bin/env python3
"""Writes integration/bevyray_amd_sys/src/lib.rs from include/bevyray_amd.h: one `extern "C"` declaration per export, the
constants and `brt_stats`, so that the Rust binding nobody here can compile at least cannot drift from the header
(tests/test_abi_binding.py compares the two).  Run after every change of the header:  python scripts/gen_rust_ffi.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import abi_parse  # noqa: E402

DOCS = {
    "brt_create": "replaces RaytracingPipeline::from_world (pipeline.rs:233-331)",
    "brt_upload_scene": "replaces model_buffer / material_buffer / bvh_buffer .write_buffer (pipeline.rs:136-138); bvh_nodes null: the callee builds the tree on the GPU (extract.rs:315-332 is then not needed)",
    "brt_render": "replaces set_bind_group x2 + draw(0..3, 0..1) (pipeline.rs:160-217) and the fragment() grid (raytrace.wgsl:93-123)",
    "brt_render_part_device": "one rank's strips into a device tile (row tiling over N GPUs, SURVEY 8(e))",
    "brt_render_device": "the whole frame of an N-device context, assembled on its first device (peer copies over xGMI + one copy kernel); replaces the pass on post_process.destination (pipeline.rs:191-217) for a single-process node",
    "brt_gather_rccl": "the ONE collective of the path for a host that runs one process per GPU: ncclGather of the tiles to rank 0 (rccl.h:745) + the de-interleave kernel (SURVEY 8(e))",
    "brt_rccl_unique_id": "ncclGetUniqueId through the library's own librccl (dlopen): on one rank, the 128 bytes go to the others by the host's means",
    "brt_rccl_comm_create": "ncclCommInitRank on the context's first device; every rank calls it",
    "brt_import_frame_fd": "maps the memory behind the host's colour target (a Vulkan opaque-fd export, or a dma-buf) so that the frame is written where the next pass reads it (pipeline.rs:191-203)",
    "brt_build_bvh": "replaces obvhs::ploc::build_ploc::<24> + flatten (extract.rs:315-332)",
    "brt_build_bvh_sah": "binned-SAH tree for the same node contract, CPU statement of what brt_upload_scene builds on the GPU when bvh_nodes is null",
    "brt_build_bvh_sah_device": "the same tree built on the GPU (byte-identical), with the kernel time",
    "brt_set_denoise": "the denoiser's settings: iterations 1..6, sigma_luminance / sigma_normal / sigma_depth (defaults 5, 4, 128, 1)",
    "brt_denoise_device": "the guide-buffer a-trous denoiser on an RGBA f32 device frame the caller holds (the root's frame after brt_gather_rccl); brt_render* denoise with BRT_FLAG_DENOISE",
    "brt_blend_post_device": "brt_denoise_device for a level-1 / level-2 coverage frame (rendered without the raster colour): covered pixels become the raster texels, the rest is denoised / accumulated; brt_render* do it with BRT_FLAG_BLEND_POST",
    "brt_debug_denoise_guides": "diagnostic: the denoiser's guide buffer (normal, t, demodulation factor, material id per pixel) in host memory",
    "brt_set_temporal": "the temporal history's max_history (1..65535, default 32; 1: no accumulation); empties the history",
    "brt_reset_temporal": "empties the temporal history (a camera cut)",
    "brt_query_rays_device": "batched ray queries (closest hit / occlusion) against the resident scene: 32-byte rays in, 32-byte hits out, DEVICE buffers; the reference offers none (a host would rebuild a CPU BVH per frame, extract.rs:315-332)",
    "brt_query_rays": "the same for host buffers, synchronous",
    "brt_query_origin_bound": "the largest origin 1-norm the resident tree covers (+INF: any)",
    "brt_upscale_device": "guide-buffer upsampling of a low-resolution Pure DEVICE frame the caller holds to the colour target's size: every output pixel casts its own centre ray, so silhouettes, base colour and sky are at full sharpness",
    "brt_render_upscaled_device": "trace at low_width x low_height (brt_render_device's frame, every device of the context), post-passes on the low frame, upsampling into the full-size target: the pass on post_process.destination (pipeline.rs:191-217) at a fraction of the rays",
    "brt_host_upscale_window": "host arithmetic: the WindowExtract a low frame is traced with (height scaled in integer arithmetic, at least 1)",
    "brt_upscale_blend_device": "brt_upscale_device for a frame of level 1 / 2: the low frame is a Pure frame, the raster blend (raytrace.wgsl:104-120) is decided per output pixel against the full-size raster depth and colour",
    "brt_render_upscaled_blend_device": "brt_render_upscaled_device for a frame of level 1 / 2: trace low at level 3, present full with the raster blend -- the pass of the shipping level (FallbackRaytraced) at a fraction of the rays",
    "brt_host_blend_covered": "host arithmetic: whether the raster wins a pixel whose centre ray hits at distance t (+INF: a miss) against a raster depth, the blend rule of the two calls above",
    "brt_host_pixel_ray": "host arithmetic: the pixel-centre ray of a pixel (raytrace.wgsl:139-156 without the jitter), for picking",
    "brt_debug_temporal_state": "diagnostic: the temporal history per pixel (h.rgb, n, m1, m2, reprojected x', y') in host memory",
}


def main():
    H = abi_parse.parse_header(os.path.join(ROOT, "include", "bevyray_amd.h"))
    lines = []
    for name, (ret, args) in H["functions"].items():
        if name in DOCS:
            lines.append(f"    /// {DOCS[name]}")
        parts = [f"{n}: {t}" for n, t in args]
        sig = f"    pub fn {name}({', '.join(parts)}) -> {ret};"
        if len(sig) > 118:
            cur = f"    pub fn {name}("
            indent, out = " " * len(cur), []
            for i, pz in enumerate(parts):
                piece = pz + (", " if i < len(parts) - 1 else "")
                if len(cur) + len(piece) > 116:
                    out.append(cur.rstrip())
                    cur = indent + piece
                else:
                    cur += piece
            out.append(cur + f") -> {ret};")
            sig = "\n".join(out)
        lines.append(sig)
    c = H["constants"]

    def grp(prefix):
        return [(k, v) for k, v in c.items() if k.startswith(prefix)]

    rs = f'''//! UNVERIFIED SOURCE: written against `include/bevyray_amd.h` (BRT_ABI_VERSION {c["BRT_ABI_VERSION"]}), never compiled (no Rust
//! toolchain in the build environment).  GENERATED by `scripts/gen_rust_ffi.py` from the header; what IS checked mechanically:
//! `tests/test_abi_binding.py` parses this file and the C header and compares every export (name, argument count, argument and
//! return types), every constant, the field order and types of `brt_stats` and the ABI version.  What is compiled and tested
//! against the same ABI: the ctypes binding `bevyray_amd/_lib.py` (every GPU test goes through it) and the C++ host
//! `bevyray_amd/host/raytracing.hpp`.
//!
//! One declaration per export of the header; the doc comment of each names the reference code it replaces.
#![allow(non_camel_case_types)]
use std::os::raw::{{c_char, c_void}};

pub const BRT_ABI_VERSION: u32 = {c["BRT_ABI_VERSION"]};
pub const BRT_STRIP_ROWS: u32 = {c["BRT_STRIP_ROWS"]};

pub const BRT_OK: i32 = 0;
'''
    for k, v in grp("BRT_ERR_"):
        rs += f"pub const {k}: i32 = {v};\n"
    for title, prefix in (("Raytracing level, reference src/raytracing/mod.rs:94-101 (#[repr(u32)])", "BRT_LEVEL_"), ("brt_render* flags", "BRT_FLAG_"),
                          ("brt_set_policy: the WGSL-spec (short-circuit) reading of `||` in raytrace.wgsl:269; default 0 = both operands evaluated", "BRT_POLICY_"),
                          ("brt_import_frame_fd handle types", "BRT_EXTMEM_"), ("brt_scene_generate kinds", "BRT_SCENE_"), ("brt_query_rays*: modes, status bits, the \"no sphere\" index", "BRT_QUERY_"), ("brt_debug_eval op codes", "BRT_DBG_")):
        rs += f"\n/// {title}\n"
        for k, v in grp(prefix):
            rs += f"pub const {k}: u32 = {v};\n"
    rs += "\n#[repr(C)]\npub struct brt_ctx { _private: [u8; 0] }\n\n#[repr(C)]\n#[derive(Default, Debug, Clone, Copy)]\npub struct brt_stats {\n"
    for n, t in H["stats"]:
        rs += f"    pub {n}: {t},\n"
    rs += "}\n\nextern \"C\" {\n" + "\n".join(lines) + "\n}\n"
    rs += '''
/// Text of the last error as an owned String (ctx may be null).
pub unsafe fn last_error(ctx: *const brt_ctx) -> String {
    let p = brt_last_error(ctx);
    if p.is_null() { String::new() } else { std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned() }
}
'''
    open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs"), "w").write(rs)
    print("wrote integration/bevyray_amd_sys/src/lib.rs:", len(H["functions"]), "exports")


if __name__ == "__main__":
    main()
