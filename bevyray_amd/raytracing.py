"""Host-side mirror of bevyray's plugin surface for the ray-tracing pass.

Names, fields and error behaviour follow the reference's Rust (reference
src/raytracing/mod.rs, extract.rs, pipeline.rs) so that tests read like tests of the
reference would; the arithmetic lives in the C++/HIP library behind the C ABI
(include/bevyray_amd.h).  Nothing here traces rays.

    RaytracePlugin            mod.rs:24-84      owns the GPU context (RaytracingPipeline::from_world)
    RaytracedCamera           mod.rs:86-91      {level, sample_count, bounces}
    Raytracing                mod.rs:94-101     Skip/FallbackRaster/FallbackRaytraced/Pure = 0..3
    RaytracedSphere           mod.rs:103-106    {radius}
    StandardMaterial          bevy 0.14 defaults of the fields extract.rs:200-207 reads
    CameraExtract / WindowExtract / RaytraceLevelExtract / RaytraceMaterial / Model / BVHNode
                              extract.rs:56-237 byte layouts (numpy structured dtypes)
    prepare_buffers           extract.rs:280-337
    RayTracingNode.run        pipeline.rs:58-220
"""
from __future__ import annotations

import ctypes as C
import enum
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import BrtError, BrtStats

# ---- wire formats (extract.rs:56-61, 83-104, 181-189, 213-218, 229-237) ---------------------

MODEL_DTYPE = np.dtype({"names": ["position", "radius", "material_id"],
                        "formats": [("<f4", 3), "<f4", "<u4"], "offsets": [0, 12, 16], "itemsize": 32})
MATERIAL_DTYPE = np.dtype({"names": ["base_color", "metallic", "roughness", "reflectance", "ior", "specular_transmission"],
                           "formats": [("<f4", 3), "<f4", "<f4", "<f4", "<f4", "<f4"],
                           "offsets": [0, 12, 16, 20, 24, 28], "itemsize": 32})
BVH_NODE_DTYPE = np.dtype({"names": ["bounds_min", "bounds_max", "index", "model_count"],
                           "formats": [("<f4", 3), ("<f4", 3), "<u4", "<u4"], "offsets": [0, 16, 28, 32], "itemsize": 48})
CAMERA_DTYPE = np.dtype({"names": ["sample_count", "bounce_count", "projection", "near", "far", "fov", "aspect",
                                   "position", "direction", "up"],
                         "formats": ["<u4", "<u4", "<u4", "<f4", "<f4", "<f4", "<f4", ("<f4", 3), ("<f4", 3), ("<f4", 3)],
                         "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 48, 64], "itemsize": 80})
WINDOW_DTYPE = np.dtype({"names": ["random_seed", "height"], "formats": ["<f4", "<u4"], "offsets": [0, 4], "itemsize": 16})
LEVEL_DTYPE = np.dtype({"names": ["level"], "formats": ["<u4"], "offsets": [0], "itemsize": 32})

STRIP_ROWS = 8
FLAG_COUNTERS = 1
FLAG_KERNEL_SIMPLE = 2
POLICY_OR_SHORT_CIRCUIT = 1   # brt_set_policy: the WGSL-spec reading of `||` in raytrace.wgsl:269 (default: both operands evaluated)
POLICY_MINMAX_SELECT = 2      # ... min / max by compare-select (default: minNum / maxNum)
POLICY_POW_EXP2_LOG2 = 4      # ... pow(x, 5) as exp2(5 log2 x) (default: multiplies)
EXTMEM_OPAQUE_FD, EXTMEM_DMABUF_FD = 1, 2   # brt_import_frame_fd handle types
FLAG_CALLER_STREAM = 4   # device entry points: `stream` is the caller's stream even when its handle is 0
FLAG_DENOISE = 32        # brt_render / brt_render_device (level 3): the frame is denoised (RaytracePlugin.set_denoise) before it is written
FLAG_TEMPORAL = 64       # ... and brt_denoise_device: the frame is accumulated into the context's temporal history (set_temporal)
FLAG_BLEND_POST = 128    # brt_render / brt_render_device at levels 1 / 2, with FLAG_DENOISE and / or FLAG_TEMPORAL: the post-passes run on the
                         # ray-traced pixels, the raster-covered ones are written as their raster texels (level 3 ignores the flag)
# format of an assembled DEVICE frame (render_device, gather_rccl, deinterleave_device): the colour target's own (pipeline.rs:311-315)
FLAG_OUT_RGBA32F, FLAG_OUT_RGBA8_UNORM_SRGB, FLAG_OUT_RGBA16F, FLAG_OUT_RGBA8_UNORM = 0, 8, 16, 24
OUT_PIXEL_BYTES = {FLAG_OUT_RGBA32F: 16, FLAG_OUT_RGBA8_UNORM_SRGB: 4, FLAG_OUT_RGBA16F: 8, FLAG_OUT_RGBA8_UNORM: 4}

SCENE_COVER, SCENE_RTIOW_FINAL, SCENE_STRESS_GRID = 0, 1, 2


class Raytracing(enum.IntEnum):
    """mod.rs:94-101, #[repr(u32)]"""
    Skip = 0
    FallbackRaster = 1
    FallbackRaytraced = 2
    Pure = 3


@dataclass
class RaytracedCamera:
    """mod.rs:86-91"""
    level: Raytracing = Raytracing.FallbackRaytraced
    sample_count: int = 4
    bounces: int = 4


@dataclass
class RaytracedSphere:
    """mod.rs:103-106"""
    radius: float = 1.0


@dataclass
class StandardMaterial:
    """The StandardMaterial fields extract.rs:200-207 reads, with bevy 0.14's defaults.
    base_color is sRGB (Color::srgb), decoded to linear by RaytraceMaterial.prepare_asset."""
    base_color: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    metallic: float = 0.0
    perceptual_roughness: float = 0.5
    reflectance: float = 0.5
    ior: float = 1.5
    specular_transmission: float = 0.0


@dataclass
class PerspectiveProjection:
    fov: float = math.pi / 4.0
    aspect_ratio: float = 1.0
    near: float = 0.1
    far: float = 1000.0


@dataclass
class OrthographicProjection:
    """Unsupported by the reference: CameraExtract returns None (extract.rs:148)."""
    scale: float = 1.0


@dataclass
class Transform:
    """Transform::from_translation(t).looking_at(target, up)"""
    translation: Tuple[float, float, float] = (0.0, 0.0, 5.0)
    target: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    up: Tuple[float, float, float] = (0.0, 1.0, 0.0)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _trim(arr: np.ndarray, n: int) -> np.ndarray:
    """First n records as an owned array, copied bytewise (padding bytes stay zero)."""
    raw = arr.view(np.uint8).reshape(len(arr), arr.dtype.itemsize)[:n].copy()
    return raw.view(arr.dtype).reshape(n)


def _stream_args(stream: Optional[int], flags: int = 0):
    """The (hip_stream, flags) pair of a device entry point: stream=None is the context's own stream, a handle (0 = the default
    stream) the caller's, with FLAG_CALLER_STREAM added to `flags`."""
    return stream or None, flags | (0 if stream is None else FLAG_CALLER_STREAM)


def _stats8(words, names) -> dict:
    """The out_stats8 words of a list call; names: the keys of word 0 and of word 6, which differ by family."""
    return {names[0]: int(words[0]), "hits": int(words[1]), "refused": int(words[2]), "tree_rebuilt": int(words[3]),
            "tree_reach": float(np.array([words[4]], np.uint64).astype(np.uint32).view(np.float32)[0]),
            "form": int(words[5]), names[1]: int(words[6])}


def _bake_call(node, export, *args) -> dict:
    """One brt_bake_* export of `node`: export(ctx, *args, out_stats8), checked -> the call's stats, kept in node.last_probe_stats."""
    p = node._p
    words = (C.c_uint64 * 8)()
    _lib.check(export(p._ctx, *args, words), p._ctx)
    node.last_probe_stats = _stats8(words, ("walks", "chunks"))
    return node.last_probe_stats


class CameraExtract:
    """extract.rs:83-158"""

    @staticmethod
    def extract_component(camera: RaytracedCamera, transform: Transform, projection):
        if not isinstance(projection, PerspectiveProjection):
            return None  # extract.rs:148
        lib = _lib.load()
        cam = np.zeros(1, CAMERA_DTYPE)
        _lib.check(lib.brt_host_camera_extract(_f3(transform.translation), _f3(transform.target), _f3(transform.up),
                                               projection.fov, projection.aspect_ratio, projection.near, projection.far,
                                               int(camera.sample_count), int(camera.bounces), cam.ctypes.data))
        level = np.zeros(1, LEVEL_DTYPE)
        level["level"] = int(camera.level)
        return level, cam


class WindowExtract:
    """extract.rs:56-81.  The reference draws random_seed from thread_rng every frame; here
    it is an explicit input."""

    @staticmethod
    def extract_component(physical_height: int, random_seed: float):
        lib = _lib.load()
        win = np.zeros(1, WINDOW_DTYPE)
        _lib.check(lib.brt_host_window_extract(float(random_seed), int(physical_height), win.ctypes.data))
        return win


class RaytraceMaterial:
    """extract.rs:181-209"""

    @staticmethod
    def prepare_asset(source: StandardMaterial) -> np.ndarray:
        lib = _lib.load()
        out = np.zeros(1, MATERIAL_DTYPE)
        _lib.check(lib.brt_host_material(_f3(source.base_color), source.metallic, source.perceptual_roughness,
                                         source.reflectance, source.ior, source.specular_transmission, out.ctypes.data))
        return out


def build_bvh(models: np.ndarray) -> np.ndarray:
    """The build_ploc call + flatten of extract.rs:315-332 (native PLOC builder)."""
    lib = _lib.load()
    models = np.ascontiguousarray(models, MODEL_DTYPE)
    n = len(models)
    cap = max(1, 2 * n)
    nodes = np.zeros(cap, BVH_NODE_DTYPE)
    out_n = C.c_uint32(0)
    _lib.check(lib.brt_build_bvh(models.ctypes.data, n, nodes.ctypes.data, cap, C.byref(out_n)))
    return _trim(nodes, out_n.value)


def build_bvh_sah(models: np.ndarray, reach: float = 0.0) -> np.ndarray:
    """The binned-SAH tree that brt_upload_scene builds when the caller passes no BVH (brt_build_bvh_sah); reach: what the
    leaf pads cover (0 = the scene's own extent; tree_reach(models, camera) for a camera further out)."""
    lib = _lib.load()
    models = np.ascontiguousarray(models, MODEL_DTYPE)
    n = len(models)
    cap = max(1, 2 * n)
    nodes = np.zeros(cap, BVH_NODE_DTYPE)
    out_n = C.c_uint32(0)
    _lib.check(lib.brt_build_bvh_sah(models.ctypes.data, n, float(reach), nodes.ctypes.data, cap, C.byref(out_n)))
    return _trim(nodes, out_n.value)


def tree_reach(models: np.ndarray, camera: np.ndarray):
    """brt_host_tree_reach: (scene scale S, level, reach) the callee-built SAH tree needs for this camera."""
    lib = _lib.load()
    models = np.ascontiguousarray(models, MODEL_DTYPE)
    s, lvl, r = C.c_float(0), C.c_uint32(0), C.c_float(0)
    _lib.check(lib.brt_host_tree_reach(models.ctypes.data, len(models), camera.ctypes.data, C.byref(s), C.byref(lvl), C.byref(r)))
    return float(s.value), int(lvl.value), float(r.value)


def srgb_thresholds() -> np.ndarray:
    """brt_host_srgb_thresholds: the 255 f32 decision thresholds of the exact 8-bit sRGB encode (code = thresholds <= c)."""
    out = np.zeros(255, np.float32)
    _lib.check(_lib.load().brt_host_srgb_thresholds(out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def validate_scene(models, materials, bvh) -> int:
    """Returns the maximum leaf depth; raises BrtError for what brt_upload_scene would reject."""
    lib = _lib.load()
    models = np.ascontiguousarray(models, MODEL_DTYPE)
    materials = np.ascontiguousarray(materials, MATERIAL_DTYPE)
    bvh = np.ascontiguousarray(bvh, BVH_NODE_DTYPE)
    depth = C.c_uint32(0)
    _lib.check(lib.brt_validate_scene(models.ctypes.data, len(models), materials.ctypes.data, len(materials),
                                      bvh.ctypes.data, len(bvh), C.byref(depth)))
    return depth.value


@dataclass
class Buffers:
    """ModelBuffer / MaterialBuffer / BVHBuffer (extract.rs:252-262)."""
    models: np.ndarray
    materials: np.ndarray
    bvh: np.ndarray


def prepare_buffers(data: Sequence[Tuple[Tuple[float, float, float], RaytracedSphere, StandardMaterial]]) -> Buffers:
    """extract.rs:280-337: one Model + one material entry per sphere (material_id = enumerate
    index), AABBs padded by 0.1, PLOC BVH, flattened nodes."""
    n = len(data)
    models = np.zeros(n, MODEL_DTYPE)
    materials = np.zeros(n, MATERIAL_DTYPE)
    for i, (position, sphere, material) in enumerate(data):
        materials[i] = RaytraceMaterial.prepare_asset(material)[0]
        models[i]["position"] = position
        models[i]["radius"] = sphere.radius
        models[i]["material_id"] = i
    return Buffers(models, materials, build_bvh(models))


def generate_scene(kind: int, seed: int = 1) -> Buffers:
    """Seeded version of the demo scene setup (main.rs:49-240) and the other benchmark scenes."""
    lib = _lib.load()
    cap = 16384
    models = np.zeros(cap, MODEL_DTYPE)
    materials = np.zeros(cap, MATERIAL_DTYPE)
    n = C.c_uint32(0)
    _lib.check(lib.brt_scene_generate(kind, seed, models.ctypes.data, materials.ctypes.data, cap, C.byref(n)))
    models, materials = _trim(models, n.value), _trim(materials, n.value)
    return Buffers(models, materials, build_bvh(models))


def cover_camera(width: int, height: int, sample_count: int, bounces: int,
                 level: Raytracing = Raytracing.Pure, seed: float = 0.5):
    """The 'cover' view: position (13,2,3) looking at the origin, fov 0.4 rad,
    near 0.1, far 1000.  Returns (level, camera, window) extracts."""
    cam = RaytracedCamera(level=level, sample_count=sample_count, bounces=bounces)
    proj = PerspectiveProjection(fov=0.4, aspect_ratio=width / height, near=0.1, far=1000.0)
    lvl, cex = CameraExtract.extract_component(cam, Transform((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), proj)
    return lvl, cex, WindowExtract.extract_component(height, seed)


def rtiow_camera(width: int, height: int, sample_count: int, bounces: int,
                 level: Raytracing = Raytracing.Pure, seed: float = 0.5):
    """The book's final-scene view for BASELINE.json configs 3 and 4: lookfrom (13,2,3),
    lookat the origin, vfov 20 degrees = 0.34906585 rad, no defocus (the shader has none)."""
    cam = RaytracedCamera(level=level, sample_count=sample_count, bounces=bounces)
    proj = PerspectiveProjection(fov=0.34906585, aspect_ratio=width / height, near=0.1, far=1000.0)
    lvl, cex = CameraExtract.extract_component(cam, Transform((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), proj)
    return lvl, cex, WindowExtract.extract_component(height, seed)


def blend_covered(camera, level, t, raster_depth) -> np.ndarray:
    """brt_host_blend_covered per element of the broadcast of t (distance of a pixel's centre ray, inf: a miss) and raster_depth: whether
    the raster wins the pixel in a frame of `level` (LEVEL_DTYPE or int) upsampled by upscale_blend_device."""
    lib = _lib.load()
    lvl = int(level["level"][0]) if isinstance(level, np.ndarray) else int(level)
    t, d = np.broadcast_arrays(np.asarray(t, np.float32), np.asarray(raster_depth, np.float32))
    out = np.zeros(t.shape, bool)
    c = C.c_uint32(0)
    for i in np.ndindex(t.shape):
        _lib.check(lib.brt_host_blend_covered(camera.ctypes.data, lvl, float(t[i]), float(d[i]), C.byref(c)))
        out[i] = c.value != 0
    return out


# adaptive sampling: brt_*adaptive* (include/bevyray_amd.h): the classes of the pixels that are traced again at the camera's sample count
ADAPT_SPARSE, ADAPT_NOISY = 1, 2
ADAPT_DEFAULT_THRESHOLD = 0.025


def adaptive_class(t, material_id, rgb, taps_inside, taps_id, taps_rgb, threshold: float = ADAPT_DEFAULT_THRESHOLD, min_taps: int = 6) -> int:
    """brt_host_adaptive_class: the ADAPT_* class of one pixel (distance t of its centre ray, inf: sky; material id; base colour rgb) from
    its 25 taps in the rule's order (dy outer, dx inner, -2 .. 2): inside the frame or not, material ids, base colours (25, 3)."""
    inside = np.ascontiguousarray(taps_inside, np.uint32).reshape(25)
    ids = np.ascontiguousarray(taps_id, np.uint32).reshape(25)
    cols = np.ascontiguousarray(taps_rgb, np.float32).reshape(75)
    own = np.ascontiguousarray(rgb, np.float32).reshape(-1)[:3].copy()
    c = C.c_uint32(0)
    _lib.check(_lib.load().brt_host_adaptive_class(float(t), int(material_id), own.ctypes.data, inside.ctypes.data, ids.ctypes.data,
                                                   cols.ctypes.data, float(threshold), int(min_taps), C.byref(c)))
    return int(c.value)


# progressive frames: brt_*progressive* (include/bevyray_amd.h): the 32-byte record of a pixel between two of its samples
PROG_SELECTED = 1
PROG_DEFAULT_THRESHOLD = 0.05
PROG_PIXEL_DTYPE = np.dtype([("sum", np.float32, 3), ("m1", np.float32), ("m2", np.float32), ("rng", np.uint32), ("n", np.uint32),
                             ("rays", np.uint32)])
assert PROG_PIXEL_DTYPE.itemsize == 32


def progressive_accumulate(record, rgb) -> np.ndarray:
    """brt_host_progressive_accumulate: one PROG_PIXEL_DTYPE record with one more sample of colour rgb (a new array; rng and rays stay)."""
    rec = np.array(record, PROG_PIXEL_DTYPE).reshape(1).copy()
    col = np.ascontiguousarray(rgb, np.float32).reshape(-1)[:3].copy()
    _lib.check(_lib.load().brt_host_progressive_accumulate(rec.ctypes.data, col.ctypes.data))
    return rec


def progressive_class(records9, inside9, target: int, threshold: float = PROG_DEFAULT_THRESHOLD, radius: int = 1) -> int:
    """brt_host_progressive_class: PROG_SELECTED or 0 for one pixel from the PROG_PIXEL_DTYPE records of its 3x3 window (dy outer, dx
    inner, -1 .. 1: the pixel itself is records9[4]) and whether each lies inside the frame."""
    recs = np.ascontiguousarray(records9, PROG_PIXEL_DTYPE).reshape(9)
    inside = np.ascontiguousarray(inside9, np.uint32).reshape(9)
    c = C.c_uint32(0)
    _lib.check(_lib.load().brt_host_progressive_class(recs.ctypes.data, inside.ctypes.data, int(target), float(threshold), int(radius),
                                                      C.byref(c)))
    return int(c.value)


def upscale_window(window, height: int, low_height: int) -> np.ndarray:
    """brt_host_upscale_window: the window a low_height frame is traced with when it is to be upsampled to `height` rows -- the seed of
    `window`, its height scaled to max(1, window.height * low_height // height).  Host arithmetic."""
    out = np.zeros(1, WINDOW_DTYPE)
    _lib.check(_lib.load().brt_host_upscale_window(window.ctypes.data, int(height), int(low_height), out.ctypes.data))
    return out


def tile_rows(height: int, n_parts: int) -> int:
    return int(_lib.load().brt_tile_rows(height, n_parts))


# ray queries: brt_query_rays* (include/bevyray_amd.h)
QUERY_CLOSEST, QUERY_ANY = 0, 1
QUERY_STATUS_MISS, QUERY_STATUS_HIT, QUERY_STATUS_FRONT_FACE, QUERY_STATUS_INVALID, QUERY_STATUS_OUT_OF_REACH = 0, 1, 2, 4, 8
QUERY_NONE = 0xFFFFFFFF
# refined upsampling: brt_upscale_refine* (include/bevyray_amd.h): the classes of output pixels that are traced at full size
REFINE_EDGES, REFINE_SPECULAR = 1, 2
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_max", np.float32), ("direction", np.float32, 3), ("user", np.uint32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("normal", np.float32, 3), ("sphere", np.uint32), ("material", np.uint32),
                      ("status", np.uint32), ("user", np.uint32)])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32
# radiance queries: brt_radiance_rays* (include/bevyray_amd.h): the query ray with `seed` where t_max is, the query hit with the colour
# where the normal is
RADIANCE_RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("seed", np.uint32), ("direction", np.float32, 3), ("user", np.uint32)])
RADIANCE_DTYPE = np.dtype([("t", np.float32), ("rgb", np.float32, 3), ("sphere", np.uint32), ("material", np.uint32),
                           ("status", np.uint32), ("user", np.uint32)])
assert RADIANCE_RAY_DTYPE.itemsize == 32 and RADIANCE_DTYPE.itemsize == 32
# light probes: brt_bake_probes* (include/bevyray_amd.h): a position with the seed of its first entry; the record of one probe
PROBE_SH9, PROBE_AMBIENT_CUBE = 0, 1
PROBE_DTYPE = np.dtype([("position", np.float32, 3), ("seed", np.uint32)])
PROBE_RECORD_DTYPE = np.dtype([("coeff", np.float32, 27), ("hits", np.uint32), ("status", np.uint32), ("n_dirs", np.uint32),
                               ("basis", np.uint32), ("reserved", np.uint32)])
assert PROBE_DTYPE.itemsize == 16 and PROBE_RECORD_DTYPE.itemsize == 128


def probe_directions(n_dirs: int) -> np.ndarray:
    """brt_host_probe_directions: the (n_dirs, 3) f32 direction table of a probe.  Host arithmetic."""
    n = int(n_dirs)
    out = np.zeros((n if 0 < n <= 65536 else 0, 3), np.float32)       # (a count out of range is refused before anything is written)
    _lib.check(_lib.load().brt_host_probe_directions(n, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def probe_irradiance(record, normal) -> np.ndarray:
    """brt_host_probe_irradiance: one PROBE_RECORD_DTYPE record evaluated for a unit normal -> rgb (f32 x 3).  Host arithmetic."""
    rec = np.ascontiguousarray(record, PROBE_RECORD_DTYPE).reshape(1)
    n = np.ascontiguousarray(normal, np.float32).reshape(3)
    out = np.zeros(3, np.float32)
    _lib.check(_lib.load().brt_host_probe_irradiance(rec.ctypes.data, n.ctypes.data_as(C.POINTER(C.c_float)),
                                                     out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


# irradiance volumes: brt_bake_volume* / brt_sample_volume* (include/bevyray_amd.h): a lattice of probes, the points lit from it, the samples
VOLUME_WRAP = 1
VOLUME_STATUS_CLAMPED, VOLUME_STATUS_INVALID, VOLUME_STATUS_NO_PROBE = 1, 4, 8
VOLUME_DTYPE = np.dtype([("origin", np.float32, 3), ("seed", np.uint32), ("spacing", np.float32, 3), ("basis", np.uint32),
                         ("count", np.uint32, 3), ("flags", np.uint32)])
VOLUME_POINT_DTYPE = np.dtype([("position", np.float32, 3), ("ignored0", np.uint32), ("normal", np.float32, 3), ("ignored1", np.uint32)])
VOLUME_SAMPLE_DTYPE = np.dtype([("rgb", np.float32, 3), ("status", np.uint32)])
assert VOLUME_DTYPE.itemsize == 48 and VOLUME_POINT_DTYPE.itemsize == 32 and VOLUME_SAMPLE_DTYPE.itemsize == 16


def make_volume(origin, spacing, count, basis: int = PROBE_SH9, seed: int = 0, flags: int = 0) -> np.ndarray:
    """One VOLUME_DTYPE descriptor (shape (1,)); nothing is checked here: the library refuses a bad one."""
    v = np.zeros(1, VOLUME_DTYPE)
    v["origin"], v["spacing"], v["count"] = origin, spacing, count
    v["seed"], v["basis"], v["flags"] = seed, basis, flags
    return v


def _volume_probe_count(volume) -> int:
    c = [int(x) for x in volume["count"].reshape(3)]
    n = c[0] * c[1] * c[2]
    return n if all(1 <= x <= 1024 for x in c) and n <= 1 << 20 else 0      # (a bad descriptor is refused before anything is written)


def volume_probes(volume) -> np.ndarray:
    """brt_host_volume_probes: the PROBE_DTYPE records of the lattice, in index order.  Host arithmetic."""
    v = np.ascontiguousarray(volume, VOLUME_DTYPE).reshape(1)
    out = np.zeros(_volume_probe_count(v), PROBE_DTYPE)
    _lib.check(_lib.load().brt_host_volume_probes(v.ctypes.data, out.ctypes.data if out.size else None))
    return out


def volume_sample_host(volume, records, points) -> np.ndarray:
    """brt_host_volume_sample: the sampling rule over VOLUME_POINT_DTYPE points on the host -> VOLUME_SAMPLE_DTYPE.  The compiled twin
    of the kernel behind RayTracingNode.sample_volume."""
    v = np.ascontiguousarray(volume, VOLUME_DTYPE).reshape(1)
    records = np.ascontiguousarray(records, PROBE_RECORD_DTYPE)
    points = np.ascontiguousarray(points, VOLUME_POINT_DTYPE)
    out = np.zeros(points.shape, VOLUME_SAMPLE_DTYPE)
    _lib.check(_lib.load().brt_host_volume_sample(v.ctypes.data, records.ctypes.data if records.size else None,
                                                  points.ctypes.data if points.size else None, points.size,
                                                  out.ctypes.data if points.size else None))
    return out


# reflection probes: brt_bake_envmap* / brt_envmap_*_device (include/bevyray_amd.h): a cube map [face][y][x] of RGBA f32 texels, its
# roughness mip chain, and the tap tables of the filter
ENVMAP_TAPS_GGX, ENVMAP_TAPS_COSINE = 0, 1
ENVMAP_TEXEL_DTYPE = np.dtype([("rgba", np.float32, 4)])
ENVMAP_TEXEL16_DTYPE = np.dtype([("rgba", np.float16, 4)])
ENVMAP_TAP_DTYPE = np.dtype([("l", np.float32, 3), ("w", np.float32)])
assert ENVMAP_TEXEL_DTYPE.itemsize == 16 and ENVMAP_TEXEL16_DTYPE.itemsize == 8 and ENVMAP_TAP_DTYPE.itemsize == 16


def envmap_level_offsets(size: int, levels: int) -> list:
    """The texel offsets of the levels of a chain, level 0 first, and the chain's total as the last entry (levels + 1 entries): level l
    has edge size >> l and begins at the sum over j < l of 6 * (size >> j) ** 2."""
    offs = [0]
    for l in range(int(levels)):
        offs.append(offs[-1] + 6 * (int(size) >> l) ** 2)
    return offs


def envmap_directions(size: int) -> np.ndarray:
    """brt_host_envmap_directions: the (6, size, size, 3) f32 texel directions of a cube, faces +X, -X, +Y, -Y, +Z, -Z.  Host arithmetic."""
    s = int(size)
    out = np.zeros((6, s, s, 3) if 0 < s <= 4096 else (0, 3), np.float32)   # (a size out of range is refused before anything is written)
    _lib.check(_lib.load().brt_host_envmap_directions(s, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def envmap_taps(kind: int, roughness: float, n_taps: int) -> np.ndarray:
    """brt_host_envmap_taps: the (n_taps, 4) f32 table {lx, ly, lz, w} of ENVMAP_TAPS_GGX at `roughness` or of ENVMAP_TAPS_COSINE."""
    n = int(n_taps)
    out = np.zeros((n if 0 < n <= 4096 else 0, 4), np.float32)
    _lib.check(_lib.load().brt_host_envmap_taps(int(kind), float(roughness), n, out.ctypes.data if out.size else None))
    return out


def envmap_downsample_host(src) -> np.ndarray:
    """brt_host_envmap_downsample: the box level of a (6, S, S, 4) f32 cube -> (6, S / 2, S / 2, 4).  Host arithmetic."""
    src = np.ascontiguousarray(src, np.float32)
    s = src.shape[1]
    out = np.zeros((6, s // 2, s // 2, 4), np.float32)
    _lib.check(_lib.load().brt_host_envmap_downsample(src.ctypes.data, s, out.ctypes.data if out.size else None))
    return out


def envmap_filter_host(src, taps, dst_size: int) -> np.ndarray:
    """brt_host_envmap_filter: the filter rule on the host, a (6, S, S, 4) f32 cube and an (n, 4) table -> (6, dst_size, dst_size, 4).
    The compiled twin of the kernel behind RayTracingNode.envmap_filter_device."""
    src = np.ascontiguousarray(src, np.float32)
    taps = np.ascontiguousarray(taps, np.float32).reshape(-1, 4)
    d = int(dst_size)
    out = np.zeros((6, d, d, 4) if 0 < d <= 4096 else (0, 4), np.float32)
    _lib.check(_lib.load().brt_host_envmap_filter(src.ctypes.data, src.shape[1], taps.ctypes.data if taps.size else None, len(taps), d,
                                                  out.ctypes.data if out.size else None))
    return out


# lightmaps: brt_bake_lightmap* / brt_lightmap_*_device (include/bevyray_amd.h): one surface point per texel of a chart, the texels
# (mean linear radiance over the hemisphere: irradiance = pi * rgb; a = 1 traced, 0.5 dilated, 0 neither) and the optional info records
LIGHTMAP_STATUS_EMPTY = 16
LIGHTMAP_POINT_DTYPE = np.dtype([("position", np.float32, 3), ("seed", np.uint32), ("normal", np.float32, 3), ("offset", np.float32)])
LIGHTMAP_INFO_DTYPE = np.dtype([("hits", np.uint32), ("status", np.uint32)])
assert LIGHTMAP_POINT_DTYPE.itemsize == 32 and LIGHTMAP_INFO_DTYPE.itemsize == 8


def lightmap_directions(n_dirs: int) -> np.ndarray:
    """brt_host_lightmap_directions: the (n_dirs, 3) f32 cosine-weighted hemisphere directions about +z.  Host arithmetic."""
    n = int(n_dirs)
    out = np.zeros((n if 0 < n <= 65536 else 0, 3), np.float32)       # (a count out of range is refused before anything is written)
    _lib.check(_lib.load().brt_host_lightmap_directions(n, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def lightmap_ray(point, n_dirs: int, k: int) -> np.ndarray:
    """brt_host_lightmap_ray: entry k of one LIGHTMAP_POINT_DTYPE point as one RADIANCE_RAY_DTYPE record.  The compiled twin of the
    kernel behind RayTracingNode.lightmap_rays_device."""
    pt = np.ascontiguousarray(point, LIGHTMAP_POINT_DTYPE).reshape(1)
    ray = np.zeros(1, RADIANCE_RAY_DTYPE)
    _lib.check(_lib.load().brt_host_lightmap_ray(pt.ctypes.data, int(n_dirs), int(k), ray.ctypes.data))
    return ray


def lightmap_sphere_points(centre, radius: float, width: int, height: int, seed: int = 0, offset: float = 0.0) -> np.ndarray:
    """brt_host_lightmap_sphere_points: the (height, width) LIGHTMAP_POINT_DTYPE points of the latitude-longitude chart of one sphere
    (azimuth about +Y along x, polar angle from +Y along y).  One parameterisation: a host with other UVs makes its own points."""
    w, h = int(width), int(height)
    out = np.zeros((h, w) if 0 < w <= 16384 and 0 < h <= 16384 else (0, 0), LIGHTMAP_POINT_DTYPE)
    _lib.check(_lib.load().brt_host_lightmap_sphere_points(_f3(centre), float(radius), int(seed), float(offset), w, h,
                                                           out.ctypes.data if out.size else None))
    return out


def lightmap_dilate_host(texels, passes: int, wrap_u: bool = False) -> np.ndarray:
    """brt_host_lightmap_dilate: `passes` dilation passes over an (H, W, 4) f32 image.  The compiled twin of the kernel behind
    RayTracingNode.lightmap_dilate_device."""
    src = np.ascontiguousarray(texels, np.float32)
    h, w = src.shape[:2]
    out = np.zeros(src.shape, np.float32)
    _lib.check(_lib.load().brt_host_lightmap_dilate(src.ctypes.data, w, h, int(passes), int(wrap_u), out.ctypes.data))
    return out


def pixel_ray(camera, window, width: int, height: int, px: int, py: int) -> np.ndarray:
    """brt_host_pixel_ray: the pixel-centre ray of pixel (px, py) as one RAY_DTYPE record (t_max = inf, user = py * width + px): the
    ray the guide buffer casts for that pixel.  Host arithmetic; for picking through RayTracingNode.query_rays."""
    ray = np.zeros(1, RAY_DTYPE)
    _lib.check(_lib.load().brt_host_pixel_ray(camera.ctypes.data, window.ctypes.data, int(width), int(height), int(px), int(py),
                                              ray.ctypes.data))
    return ray


# brt_lens (include/bevyray_amd.h "lens frames"): the descriptor of brt_render_lens*
LENS_DTYPE = np.dtype([("aperture_radius", np.float32), ("focus_distance", np.float32), ("ortho_height", np.float32),
                       ("reserved", np.uint32, 5)])
assert LENS_DTYPE.itemsize == 32


def lens(aperture_radius: float = 0.0, focus_distance: float = 1.0, ortho_height: float = 0.0) -> np.ndarray:
    """One LENS_DTYPE record.  aperture_radius 0: a pinhole; > 0: a thin lens focused on the plane at focus_distance along the camera's
    direction.  ortho_height: the height of the view volume of an orthographic camera (camera["projection_type"] = 1)."""
    d = np.zeros(1, LENS_DTYPE)
    d["aperture_radius"] = aperture_radius
    d["focus_distance"] = focus_distance
    d["ortho_height"] = ortho_height
    return d


def lens_seed(window, width: int, height: int, px: int, py: int) -> int:
    """brt_host_lens_seed: the RNG seed of pixel (px, py) of a width x height frame (raytrace.wgsl:95)."""
    seed = C.c_uint32()
    _lib.check(_lib.load().brt_host_lens_seed(window.ctypes.data, int(width), int(height), int(px), int(py), C.byref(seed)))
    return seed.value


def lens_ray(camera, window, lens_desc, width: int, height: int, px: int, py: int, state: int):
    """brt_host_lens_ray: the lens rule for one sample of pixel (px, py) on the RNG state `state` -> (origin (3,) f32, direction (3,)
    f32, the state behind the rule's draws).  The compiled twin of the kernels behind RayTracingNode.render_lens*."""
    st = C.c_uint32(int(state))
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    _lib.check(_lib.load().brt_host_lens_ray(camera.ctypes.data, window.ctypes.data, lens_desc.ctypes.data, int(width), int(height),
                                             int(px), int(py), C.byref(st), o.ctypes.data, d.ctypes.data))
    return o, d, st.value


def lens_origin_bound(camera, lens_desc) -> float:
    """brt_host_lens_origin_bound: a 1-norm no origin of the lens rule exceeds for this camera and lens (inf: none)."""
    out = C.c_float()
    _lib.check(_lib.load().brt_host_lens_origin_bound(camera.ctypes.data, lens_desc.ctypes.data, C.byref(out)))
    return out.value


# brt_gbuffer (include/bevyray_amd.h "G-buffer"): the descriptor of brt_render_gbuffer*, its modes and formats, the status bits of the
# ids plane, and the record brt_host_gbuffer_pixel returns
GBUFFER_DEPTH_VIEW, GBUFFER_DEPTH_SHADER, GBUFFER_DEPTH_DISTANCE = 0, 1, 2
GBUFFER_NORMAL_RGBA32F, GBUFFER_NORMAL_RGB10A2 = 0, 1
GBUFFER_MOTION_UV32F, GBUFFER_MOTION_UV16F, GBUFFER_MOTION_PIXEL = 0, 1, 2
GBUFFER_STATUS_HIT, GBUFFER_STATUS_FRONT_FACE, GBUFFER_STATUS_MOVED, GBUFFER_STATUS_NO_PREVIOUS = 1, 2, 4, 8
GBUFFER_DTYPE = np.dtype([("depth_mode", np.uint32), ("normal_format", np.uint32), ("motion_format", np.uint32), ("reserved", np.uint32, 5)])
GBUFFER_PIXEL_DTYPE = np.dtype([("depth", np.float32), ("status", np.uint32), ("normal_rgb10a2", np.uint32), ("reserved0", np.uint32),
                                ("normal", np.float32, 4), ("motion", np.uint32, 2), ("xy_prev", np.float32, 2),
                                ("direction", np.float32, 3), ("reserved1", np.uint32)])
GBUFFER_IDS_DTYPE = np.dtype([("sphere", np.uint32), ("material", np.uint32), ("status", np.uint32), ("reserved", np.uint32)])
assert GBUFFER_DTYPE.itemsize == 32 and GBUFFER_PIXEL_DTYPE.itemsize == 64 and GBUFFER_IDS_DTYPE.itemsize == 16
GBUFFER_PLANES = ("depth", "normal", "motion", "ids", "albedo")


def gbuffer(depth_mode: int = GBUFFER_DEPTH_VIEW, normal_format: int = GBUFFER_NORMAL_RGBA32F,
            motion_format: int = GBUFFER_MOTION_UV32F) -> np.ndarray:
    """One GBUFFER_DTYPE record: the depth mode (GBUFFER_DEPTH_*) and the normal and motion formats of a G-buffer call."""
    d = np.zeros(1, GBUFFER_DTYPE)
    d["depth_mode"] = depth_mode
    d["normal_format"] = normal_format
    d["motion_format"] = motion_format
    return d


def gbuffer_plane(desc, plane: str, width: int, height: int) -> np.ndarray:
    """An empty host array of `plane` (GBUFFER_PLANES) of a width x height frame in the formats of `desc`."""
    nf, mf = int(desc["normal_format"][0]), int(desc["motion_format"][0])
    if plane == "depth":
        return np.zeros((height, width), np.float32)
    if plane == "normal":
        return np.zeros((height, width, 4), np.float32) if nf == GBUFFER_NORMAL_RGBA32F else np.zeros((height, width), np.uint32)
    if plane == "motion":
        return np.zeros((height, width), np.uint32) if mf == GBUFFER_MOTION_UV16F else np.zeros((height, width, 2), np.float32)
    if plane == "ids":
        return np.zeros((height, width), GBUFFER_IDS_DTYPE)
    if plane == "albedo":
        return np.zeros((height, width, 4), np.float32)
    raise ValueError(plane)


def gbuffer_pixel(camera, window, width: int, height: int, px: int, py: int, desc, t: float, sphere_new=None, sphere_old=None,
                  prev_camera=None) -> np.ndarray:
    """brt_host_gbuffer_pixel: the G-buffer rule for pixel (px, py) whose pixel-centre ray hits at t (inf: a miss) the sphere
    {centre, radius * radius} = sphere_new, which was sphere_old (None: not moved) in the frame of prev_camera (None: this camera)
    -> one GBUFFER_PIXEL_DTYPE record.  The compiled twin of the kernel behind RayTracingNode.render_gbuffer*."""
    out = np.zeros(1, GBUFFER_PIXEL_DTYPE)
    sn = None if sphere_new is None else np.ascontiguousarray(sphere_new, np.float32)
    so = None if sphere_old is None else np.ascontiguousarray(sphere_old, np.float32)
    _lib.check(_lib.load().brt_host_gbuffer_pixel(camera.ctypes.data, window.ctypes.data, int(width), int(height), int(px), int(py),
                                                  desc.ctypes.data, None if prev_camera is None else prev_camera.ctypes.data,
                                                  C.c_float(t), None if sn is None else sn.ctypes.data,
                                                  None if so is None else so.ctypes.data, out.ctypes.data))
    return out


def _gbuffer_stats(words) -> dict:
    return {"cast": int(words[0]), "hits": int(words[1]), "covered": int(words[2]), "tree_rebuilt": int(words[3]),
            "tree_reach": float(np.array([words[4]], np.uint64).astype(np.uint32).view(np.float32)[0]),
            "moved": int(words[5]), "no_previous": int(words[6])}


class RaytracePlugin:
    """mod.rs:24-84.  build()/finish() create the GPU context (the reference queues the
    render pipeline in RaytracingPipeline::from_world, pipeline.rs:233-331)."""

    def __init__(self, device_ids: Sequence[int] = (0,)):
        lib = _lib.load()
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        ctx = C.c_void_p()
        _lib.check(lib.brt_create(ids, len(device_ids), C.byref(ctx)))
        self._lib = lib
        self._ctx = ctx
        self.node = RayTracingNode(self)

    def close(self):
        if self._ctx:
            self._lib.brt_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_policy(self, flags: int) -> None:
        """brt_set_policy: POLICY_OR_SHORT_CIRCUIT or 0 (the reading of `||` in raytrace.wgsl:269; changes pixels)."""
        _lib.check(self._lib.brt_set_policy(self._ctx, flags), self._ctx)

    def set_tuning(self, name: str, value: int) -> None:
        """brt_set_tuning: a scheduling / launch-shape knob of this context (never changes a pixel)."""
        _lib.check(self._lib.brt_set_tuning(self._ctx, name.encode(), int(value)), self._ctx)

    def get_tuning(self, name: str):
        """(value, default) of a knob."""
        v, d = C.c_uint32(0), C.c_uint32(0)
        _lib.check(self._lib.brt_get_tuning(self._ctx, name.encode(), C.byref(v), C.byref(d)), self._ctx)
        return int(v.value), int(d.value)

    def tuning(self, **knobs):
        """Context manager: `with plugin.tuning(BRT_LEAF_VOTE=8): ...` sets knobs and restores the previous values."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_tuning(k)[0] for k in knobs}
            for k, v in knobs.items():
                self.set_tuning(k, v)
            try:
                yield self
            finally:
                for k, v in old.items():
                    self.set_tuning(k, v)
        return cm()

    def set_denoise(self, iterations: int = 5, sigma_luminance: float = 4.0, sigma_normal: float = 128.0,
                    sigma_depth: float = 1.0) -> None:
        """brt_set_denoise: the denoiser's settings (iterations 1..6, sigmas finite and > 0); applies to FLAG_DENOISE frames and
        RayTracingNode.denoise_device.  Invalid values raise BrtError and leave the settings as they were."""
        _lib.check(self._lib.brt_set_denoise(self._ctx, int(iterations), float(sigma_luminance), float(sigma_normal),
                                             float(sigma_depth)), self._ctx)

    def set_adaptive(self, base_spp: int = 8, threshold: float = ADAPT_DEFAULT_THRESHOLD, min_taps: int = 6) -> None:
        """brt_set_adaptive: the settings of RayTracingNode.render_adaptive_device & co. (base_spp 1..65535, threshold finite and > 0,
        min_taps 1..25).  Invalid values raise BrtError and leave the settings as they were."""
        _lib.check(self._lib.brt_set_adaptive(self._ctx, int(base_spp), float(threshold), int(min_taps)), self._ctx)

    def set_progressive(self, first_spp: int = 8, max_spp: int = 64, threshold: float = PROG_DEFAULT_THRESHOLD, radius: int = 1) -> None:
        """brt_set_progressive: the settings of RayTracingNode.render_progressive* and progressive_select_device (2 <= first_spp <=
        max_spp <= 65535, threshold finite and > 0, radius 0 or 1).  Invalid values raise BrtError and leave the settings as they were."""
        _lib.check(self._lib.brt_set_progressive(self._ctx, int(first_spp), int(max_spp), float(threshold), int(radius)), self._ctx)

    def debug_denoise_guides(self, camera, window, width: int, height: int) -> np.ndarray:
        """brt_debug_denoise_guides: (height, width, 8) f32 -- normal.xyz, t (inf: sky), a.rgb, material id as bits
        (0xFFFFFFFF: sky) of every pixel-centre ray on the resident scene."""
        out = np.empty((height, width, 8), np.float32)
        _lib.check(self._lib.brt_debug_denoise_guides(self._ctx, camera.ctypes.data, window.ctypes.data, width, height,
                                                      out.ctypes.data), self._ctx)
        return out

    def set_temporal(self, max_history: int = 32) -> None:
        """brt_set_temporal: the history length FLAG_TEMPORAL frames accumulate up to (1..65535; 1: no accumulation); empties the
        history.  An invalid value raises BrtError and changes nothing."""
        _lib.check(self._lib.brt_set_temporal(self._ctx, int(max_history)), self._ctx)

    def reset_temporal(self) -> None:
        """brt_reset_temporal: empties the temporal history (call it on a camera cut)."""
        _lib.check(self._lib.brt_reset_temporal(self._ctx), self._ctx)

    def debug_temporal_state(self, width: int, height: int) -> np.ndarray:
        """brt_debug_temporal_state: (height, width, 8) f32 -- h.rgb, n, m1, m2, x', y' of the history after the last FLAG_TEMPORAL
        frame (x', y': the reprojected position; NaN where the history was rejected)."""
        out = np.empty((height, width, 8), np.float32)
        _lib.check(self._lib.brt_debug_temporal_state(self._ctx, width, height, out.ctypes.data), self._ctx)
        return out

    def alloc_frame(self, width: int, height: int) -> np.ndarray:
        """Page-locked (height, width, 4) f32 frame owned by the context (brt_host_alloc): passing it
        as `out` to RayTracingNode.run lets the library DMA straight into it."""
        nbytes = width * height * 16
        ptr = C.c_void_p()
        _lib.check(self._lib.brt_host_alloc(self._ctx, nbytes, C.byref(ptr)), self._ctx)
        buf = (C.c_float * (width * height * 4)).from_address(ptr.value)
        return np.frombuffer(buf, np.float32).reshape(height, width, 4)

    def build_bvh(self, models: np.ndarray):
        """GPU PLOC build (brt_build_bvh_device): returns (nodes, kernel ms); same bytes as build_bvh()."""
        models = np.ascontiguousarray(models, MODEL_DTYPE)
        n = len(models)
        cap = max(1, 2 * n)
        nodes = np.zeros(cap, BVH_NODE_DTYPE)
        out_n = C.c_uint32(0)
        ms = C.c_double(0.0)
        _lib.check(self._lib.brt_build_bvh_device(self._ctx, models.ctypes.data, n, nodes.ctypes.data, cap, C.byref(out_n),
                                                  C.byref(ms)), self._ctx)
        return _trim(nodes, out_n.value), ms.value

    def build_bvh_sah(self, models: np.ndarray, reach: float = 0.0):
        """GPU binned-SAH build (brt_build_bvh_sah_device): returns (nodes, kernel ms); same bytes as build_bvh_sah()."""
        models = np.ascontiguousarray(models, MODEL_DTYPE)
        n = len(models)
        cap = max(1, 2 * n)
        nodes = np.zeros(cap, BVH_NODE_DTYPE)
        out_n = C.c_uint32(0)
        ms = C.c_double(0.0)
        _lib.check(self._lib.brt_build_bvh_sah_device(self._ctx, models.ctypes.data, n, float(reach), nodes.ctypes.data, cap, C.byref(out_n),
                                                      C.byref(ms)), self._ctx)
        return _trim(nodes, out_n.value), ms.value

    # -- frame targets in another API's memory (brt_import_frame_fd) --------------------------------------------------
    def import_frame_fd(self, fd: int, nbytes: int, handle_type: int = 2) -> int:
        """brt_import_frame_fd: maps the memory behind a file descriptor (EXTMEM_OPAQUE_FD = 1: a Vulkan opaque-fd export;
        EXTMEM_DMABUF_FD = 2: a dma-buf of a HIP virtual-memory allocation) and returns the device pointer."""
        ptr = C.c_void_p()
        _lib.check(self._lib.brt_import_frame_fd(self._ctx, int(fd), int(nbytes), int(handle_type), C.byref(ptr)), self._ctx)
        return int(ptr.value)

    def release_frame(self, d_frame: int) -> None:
        _lib.check(self._lib.brt_release_frame(self._ctx, d_frame), self._ctx)

    def debug_export_frame_fd(self, nbytes: int):
        """(fd, device pointer) of a fresh exportable allocation on the first device (the other side of import_frame_fd in tests)."""
        fd, ptr = C.c_int32(-1), C.c_void_p()
        _lib.check(self._lib.brt_debug_export_frame_fd(self._ctx, int(nbytes), C.byref(fd), C.byref(ptr)), self._ctx)
        return int(fd.value), int(ptr.value)

    def debug_copy_to_host(self, d_src: int, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype)
        _lib.check(self._lib.brt_debug_copy_to_host(self._ctx, d_src, out.ctypes.data, out.nbytes), self._ctx)
        return out

    # -- strips by measured cost (one process per GPU) --------------------------------------------------------------------
    def set_strip_table(self, n_parts: int, part_of_strip) -> None:
        """brt_set_strip_table: part_of_strip[s] = the part that renders frame strip s (a permutation of the parts inside every group of
        n_parts consecutive strips); None: back to s % n_parts.  Every rank sets the same table."""
        if part_of_strip is None:
            _lib.check(self._lib.brt_set_strip_table(self._ctx, int(n_parts), 0, None), self._ctx)
            return
        t = np.ascontiguousarray(part_of_strip, np.uint32)
        _lib.check(self._lib.brt_set_strip_table(self._ctx, int(n_parts), len(t), t.ctypes.data), self._ctx)

    def plan_strips(self, level, camera, window, width: int, height: int, n_parts: int, probe_spp: int = 4) -> np.ndarray:
        """brt_plan_strips: renders the frame once at probe_spp samples per pixel with the per-tile ray counts on, deals the strips of
        every group of n_parts out by cost, installs the table and returns it (deterministic: every rank gets the same one)."""
        t = np.zeros((height + STRIP_ROWS - 1) // STRIP_ROWS, np.uint32)
        _lib.check(self._lib.brt_plan_strips(self._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]), width, height,
                                             int(n_parts), int(probe_spp), t.ctypes.data), self._ctx)
        return t

    # -- the RCCL gather behind the C ABI (one process per GPU) -----------------------------------------------------------
    @staticmethod
    def rccl_unique_id() -> bytes:
        """brt_rccl_unique_id (ncclGetUniqueId): on one rank; the 128 bytes go to the other ranks by the host's own means."""
        buf = (C.c_char * 128)()
        _lib.check(_lib.load().brt_rccl_unique_id(buf))
        return bytes(buf.raw)

    def rccl_comm_create(self, unique_id: bytes, rank: int, world: int) -> int:
        assert len(unique_id) == 128
        comm = C.c_void_p()
        _lib.check(self._lib.brt_rccl_comm_create(self._ctx, unique_id, rank, world, C.byref(comm)), self._ctx)
        return int(comm.value)

    def rccl_comm_destroy(self, comm: int) -> None:
        _lib.check(self._lib.brt_rccl_comm_destroy(self._ctx, comm), self._ctx)

    def debug_profile(self) -> dict:
        """Lane-utilisation profile of the last FLAG_COUNTERS launch: section -> (executions, lanes)."""
        raw = (C.c_uint64 * 64)()
        _lib.check(self._lib.brt_debug_profile(self._ctx, raw), self._ctx)
        self.last_raw = [int(x) for x in raw]
        # -DBRT_ASM_COUNT builds: executions / active lanes of the hand-written loops of the last production launch (else zeros)
        self.last_asm_counts = {"interior": (int(raw[33]), int(raw[34])), "leaf": (int(raw[35]), int(raw[36])), "ball": (int(raw[37]), int(raw[38])),
                                "repairing_loop_lanes": (int(raw[39]), int(raw[43])), "rows_interior_exec": int(raw[44]), "rows_calls": int(raw[5]),
                                "rows_cycles": int(raw[6]), "wide_cycles": int(raw[7]), "leaf_slow_exec": int(raw[4])}
        names = ["interior", "leaf", "camera", "scatter", "sky", "ball", "camera_top", "round"]
        prof = {n: (int(raw[8 + 2 * k]), int(raw[9 + 2 * k])) for k, n in enumerate(names)}
        # wave time stamps (100 MHz wall clock): first start, first / last "pixel queue empty", last end
        self.last_order_meta = {"critical_tiles": int(raw[40]), "longest_pixel_rays": int(raw[41]), "split_tiles": int(raw[42]),
                                "second_halves_taken": int(raw[62]), "second_halves_left": int(raw[63])}
        t0 = (~int(raw[24])) & (2**64 - 1)
        if raw[29]:
            first_empty = ((~int(raw[25])) & (2**64 - 1)) if raw[25] else 0
            self.last_timeline = {
                "waves": int(raw[29]),
                "first_empty_ms": (first_empty - t0) / 1e5 if first_empty else None,
                "last_empty_ms": (int(raw[26]) - t0) / 1e5 if raw[26] else None,
                "end_ms": (int(raw[27]) - t0) / 1e5,
                "mean_wave_drain_ms": int(raw[28]) / 1e5 / int(raw[29]),
                "mean_wave_life_ms": int(raw[45]) / 1e5 / int(raw[29]),       # against end_ms: what the tail of the launch leaves idle
                "wave_life_hist_0.33ms": [(int(raw[46 + (b >> 2)]) >> (16 * (b & 3))) & 0xffff for b in range(64)],
                "drain_rounds": int(raw[31]),
                "drain_live_lanes_per_round": int(raw[30]) / max(1, int(raw[31])),
                # mean per wave, ms: pixel refill | walk loop | shading (of which the rejection-sampler loop) | drain
                # logic + camera ray + walk begin
                "wave_ms_refill_walk_shade_ball_pre": [int(raw[5]) / 1e5 / int(raw[29]), int(raw[6]) / 1e5 / int(raw[29]),
                                                       int(raw[7]) / 1e5 / int(raw[29]), int(raw[44]) / 1e5 / int(raw[29]),
                                                       int(raw[43]) / 1e5 / int(raw[29])],
            }
        return prof

    def debug_eval(self, op: int, inputs: np.ndarray) -> np.ndarray:
        inputs = np.ascontiguousarray(inputs, np.float32)
        assert inputs.ndim == 2 and inputs.shape[1] == 16
        out = np.zeros((inputs.shape[0], 8), np.float32)
        _lib.check(self._lib.brt_debug_eval(self._ctx, op, inputs.ctypes.data, out.ctypes.data, inputs.shape[0]), self._ctx)
        return out


class RayTracingNode:
    """pipeline.rs:29-221.  `run` uploads the three storage buffers and draws the frame."""

    def __init__(self, plugin: RaytracePlugin):
        self._p = plugin
        self.last_stats: Optional[dict] = None
        self.last_query_stats: Optional[dict] = None
        self.last_radiance_stats: Optional[dict] = None
        self.last_probe_stats: Optional[dict] = None
        self.last_gbuffer_stats: Optional[dict] = None

    def write_buffers(self, buffers: Buffers) -> None:
        """pipeline.rs:136-138"""
        p = self._p
        models = np.ascontiguousarray(buffers.models, MODEL_DTYPE)
        materials = np.ascontiguousarray(buffers.materials, MATERIAL_DTYPE)
        bvh = None if buffers.bvh is None else np.ascontiguousarray(buffers.bvh, BVH_NODE_DTYPE)
        _lib.check(p._lib.brt_upload_scene(p._ctx, models.ctypes.data, len(models), materials.ctypes.data, len(materials),
                                           None if bvh is None else bvh.ctypes.data, 0 if bvh is None else len(bvh)), p._ctx)

    def run(self, level, camera, window, width: int, height: int, buffers: Optional[Buffers] = None,
            raster_rgba: Optional[np.ndarray] = None, raster_depth: Optional[np.ndarray] = None,
            flags: int = 0, out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """Returns the RGBA f32 frame (height, width, 4), or None when the pass is skipped the
        way the reference skips it (missing camera extract, empty buffers)."""
        if camera is None or window is None or level is None:
            return None  # pipeline.rs:88-102
        p = self._p
        if buffers is not None:
            try:
                self.write_buffers(buffers)
            except BrtError as e:
                if e.code == -6:  # BRT_ERR_EMPTY_SCENE: no binding -> skip (pipeline.rs:141-151)
                    return None
                raise
        if out is None:
            out = np.empty((height, width, 4), np.float32)
        assert out.shape == (height, width, 4) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        stats = BrtStats()
        rr = None if raster_rgba is None else np.ascontiguousarray(raster_rgba, np.float32)
        rd = None if raster_depth is None else np.ascontiguousarray(raster_depth, np.float32)
        if rr is not None:
            assert rr.shape == (height, width, 4)
        if rd is not None:
            assert rd.shape == (height, width)
        _lib.check(p._lib.brt_render(p._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]), width, height,
                                     None if rr is None else rr.ctypes.data, None if rd is None else rd.ctypes.data,
                                     out.ctypes.data, flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return out

    # -- device-pointer entry points (used by bench.py with torch tensors) ------------------------

    def render_part_device(self, level, camera, window, width: int, height: int, part: int, n_parts: int,
                           d_out_tile: int, d_raster_rgba: int = 0, d_raster_depth: int = 0, stream: Optional[int] = None,
                           flags: int = 0) -> dict:
        """stream=None: the context's own stream, synchronous, full stats.  stream=<hipStream_t handle>
        (0 = the default stream): asynchronous on that stream (FLAG_CALLER_STREAM is added)."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_part_device(p._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]),
                                                 width, height, part, n_parts, d_raster_rgba or None,
                                                 d_raster_depth or None, d_out_tile, *_stream_args(stream, flags),
                                                 C.byref(stats)), p._ctx)
        return stats.as_dict()

    def render_device(self, level, camera, window, width: int, height: int, d_frame: int, d_raster_rgba: int = 0,
                      d_raster_depth: int = 0, stream: Optional[int] = None, flags: int = 0) -> dict:
        """brt_render_device: the frame of an N-device context assembled on its first device (tiles by peer copy, then
        the de-interleave kernel).  d_frame / d_raster_*: device pointers on the first device.  Stream rule as for
        render_part_device."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_device(p._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]), width, height,
                                            d_raster_rgba or None, d_raster_depth or None, d_frame, *_stream_args(stream, flags),
                                            C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def denoise_device(self, camera, window, width: int, height: int, d_frame: int, d_out: int, stream: Optional[int] = None,
                       out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_denoise_device: the context's denoiser on the RGBA f32 device frame d_frame (rendered with camera / window on the
        resident scene) into d_out (out_format: FLAG_OUT_*; may be d_frame).  Stream rule as for render_part_device.  flags:
        FLAG_TEMPORAL accumulates into the temporal history instead, and FLAG_TEMPORAL | FLAG_DENOISE filters the accumulation."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_denoise_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_frame, d_out,
                                             *_stream_args(stream, out_format | flags),
                                             C.byref(stats)), p._ctx)
        return stats.as_dict()

    def blend_post_device(self, camera, window, width: int, height: int, d_coverage: int, d_out: int, d_raster_rgba: int = 0,
                          stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_blend_post_device: denoise_device for a level-1 / level-2 frame.  d_coverage: the RGBA f32 device frame of that level
        rendered with the raster depth and no raster colour (alpha exactly 0: covered); d_raster_rgba: the raster colour on the first
        device (0: zeros).  Covered pixels of d_out (out_format; may be d_coverage) are the raster texels, the others are denoised,
        or with FLAG_TEMPORAL (| FLAG_DENOISE) accumulated (and filtered).  Stream rule as for render_part_device."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_blend_post_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_coverage,
                                                d_raster_rgba or None, d_out,
                                                *_stream_args(stream, out_format | flags), C.byref(stats)), p._ctx)
        return stats.as_dict()

    # -- guide-buffer upsampling (include/bevyray_amd.h "guide-buffer upsampling") ------------------

    def upscale_device(self, camera, window, low_width: int, low_height: int, d_low: int, width: int, height: int, d_out: int,
                       stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F) -> dict:
        """brt_upscale_device: the RGBA f32 low_width x low_height Pure device frame d_low (rendered with camera and
        upscale_window(window, height, low_height) on the resident scene; denoised / accumulated or not) upsampled into d_out
        (width x height, out_format: FLAG_OUT_*; must not overlap d_low).  Stream rule as for render_part_device."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_upscale_device(p._ctx, camera.ctypes.data, window.ctypes.data, low_width, low_height, d_low or None, width,
                                             height, d_out or None, *_stream_args(stream, out_format), C.byref(stats)), p._ctx)
        return stats.as_dict()

    def render_upscaled_device(self, camera, window, low_width: int, low_height: int, width: int, height: int, d_frame: int,
                               stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_upscaled_device: a Pure frame traced at low_width x low_height (render_device with upscale_window(window, height,
        low_height)), with flags FLAG_DENOISE and / or FLAG_TEMPORAL post-processed at that size, and upsampled into d_frame
        (width x height, out_format).  Pure only: there is no level.  Stream rule as for render_part_device; last_stats: the low
        frame's, total_ms of the whole call."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_upscaled_device(p._ctx, camera.ctypes.data, window.ctypes.data, low_width, low_height, width, height,
                                                     d_frame or None, *_stream_args(stream, out_format | flags),
                                                     C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    # -- upsampling blended frames (include/bevyray_amd.h "upsampling blended frames") -------------

    def upscale_blend_device(self, level, camera, window, low_width: int, low_height: int, d_low: int, width: int, height: int,
                             d_out: int, d_raster_rgba: int = 0, d_raster_depth: int = 0, stream: Optional[int] = None,
                             out_format: int = FLAG_OUT_RGBA32F) -> dict:
        """brt_upscale_blend_device: upscale_device for a frame of `level` (LEVEL_DTYPE; 1 / 2 blend, 3 is upscale_device).  d_low is a
        Pure low frame; d_raster_rgba / d_raster_depth: the full-size raster colour (RGBA f32) and reverse-Z depth on the first device
        (0: zeros), neither overlapping d_out.  An output pixel the raster depth wins (blend_covered) is its raster texel."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_upscale_blend_device(p._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]), low_width,
                                                   low_height, d_low or None, width, height, d_raster_rgba or None, d_raster_depth or None,
                                                   d_out or None, *_stream_args(stream, out_format), C.byref(stats)), p._ctx)
        return stats.as_dict()

    def render_upscaled_blend_device(self, level, camera, window, low_width: int, low_height: int, width: int, height: int, d_frame: int,
                                     d_raster_rgba: int = 0, d_raster_depth: int = 0, stream: Optional[int] = None,
                                     out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_upscaled_blend_device: render_upscaled_device for a frame of `level`: the low frame is traced at level 3 (post-passes
        of `flags` on it), the raster blend is decided per output pixel against the full-size raster inputs.  last_stats: the low
        frame's, total_ms of the whole call."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_upscaled_blend_device(p._ctx, camera.ctypes.data, window.ctypes.data, int(level["level"][0]), low_width,
                                                           low_height, width, height, d_raster_rgba or None, d_raster_depth or None,
                                                           d_frame or None, *_stream_args(stream, out_format | flags),
                                                           C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    # -- sparse pixel tracer and refined upsampling (include/bevyray_amd.h) -------------------------

    def render_pixels(self, camera, window, width: int, height: int, pixels: np.ndarray, flags: int = 0) -> np.ndarray:
        """brt_render_pixels: the uint32 list `pixels` (p = py * width + px, host memory) -> (n, 4) f32, entry i the value the Pure
        width x height frame holds at pixels[i] (an entry >= width * height: zeros, counted in last_stats["reserved"]).  flags:
        FLAG_KERNEL_SIMPLE (the one-thread-per-entry form; same bytes)."""
        p = self._p
        pixels = np.ascontiguousarray(pixels, np.uint32)
        out = np.zeros((pixels.size, 4), np.float32)
        stats = BrtStats()
        _lib.check(p._lib.brt_render_pixels(p._ctx, camera.ctypes.data, window.ctypes.data, width, height,
                                            pixels.ctypes.data if pixels.size else None, pixels.size,
                                            out.ctypes.data if pixels.size else None, flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return out

    def render_pixels_device(self, camera, window, width: int, height: int, d_pixels: int, n_pixels: int, d_out: int,
                             stream: Optional[int] = None, flags: int = 0) -> dict:
        """brt_render_pixels_device: n_pixels uint32 entries at d_pixels -> n_pixels RGBA f32 values at d_out (device pointers on the
        first device).  Stream rule as for render_part_device; the counts of last_stats only on the own stream."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_pixels_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_pixels or None,
                                                   int(n_pixels), d_out or None, *_stream_args(stream, flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    # -- lens frames: depth of field and orthographic projection (include/bevyray_amd.h) ------------

    def render_lens(self, camera, window, lens_desc, width: int, height: int, flags: int = 0) -> np.ndarray:
        """brt_render_lens: the Pure width x height frame under the lens rule (LENS_DTYPE, lens()) -> (height, width, 4) f32.  flags:
        FLAG_KERNEL_SIMPLE (the one-thread-per-pixel form; same bytes)."""
        p = self._p
        out = np.zeros((height, width, 4) if 0 < width <= 32768 and 0 < height <= 32768 else (1, 1, 4), np.float32)
        stats = BrtStats()
        _lib.check(p._lib.brt_render_lens(p._ctx, camera.ctypes.data, window.ctypes.data, lens_desc.ctypes.data, width, height,
                                          out.ctypes.data, flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return out

    def render_lens_device(self, camera, window, lens_desc, width: int, height: int, d_frame: int, stream: Optional[int] = None,
                           out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_lens_device: the same frame into d_frame (a device pointer on the first device) in `out_format` (FLAG_OUT_*).
        Stream rule as for render_part_device; the counts of last_stats only on the own stream."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_lens_device(p._ctx, camera.ctypes.data, window.ctypes.data, lens_desc.ctypes.data, width, height,
                                                 d_frame or None, *_stream_args(stream, out_format | flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def render_lens_pixels(self, camera, window, lens_desc, width: int, height: int, pixels: np.ndarray, flags: int = 0) -> np.ndarray:
        """brt_render_lens_pixels: render_pixels under the lens rule: entry i is the value render_lens holds at pixels[i]."""
        p = self._p
        pixels = np.ascontiguousarray(pixels, np.uint32)
        out = np.zeros((pixels.size, 4), np.float32)
        stats = BrtStats()
        _lib.check(p._lib.brt_render_lens_pixels(p._ctx, camera.ctypes.data, window.ctypes.data, lens_desc.ctypes.data, width, height,
                                                 pixels.ctypes.data if pixels.size else None, pixels.size,
                                                 out.ctypes.data if pixels.size else None, flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return out

    def render_lens_pixels_device(self, camera, window, lens_desc, width: int, height: int, d_pixels: int, n_pixels: int, d_out: int,
                                  stream: Optional[int] = None, flags: int = 0) -> dict:
        """brt_render_lens_pixels_device: render_pixels_device under the lens rule."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_lens_pixels_device(p._ctx, camera.ctypes.data, window.ctypes.data, lens_desc.ctypes.data, width,
                                                        height, d_pixels or None, int(n_pixels), d_out or None,
                                                        *_stream_args(stream, flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    # -- G-buffer: depth, normal, motion, ids, albedo of a frame (include/bevyray_amd.h) ------------

    def render_gbuffer(self, camera, window, width: int, height: int, desc, planes: Sequence[str] = GBUFFER_PLANES, prev_camera=None,
                       prev_models=None, coverage=None, into: Optional[dict] = None) -> dict:
        """brt_render_gbuffer: the planes named in `planes` (GBUFFER_PLANES) of the width x height frame -> {name: array} (gbuffer_plane's
        shapes).  prev_camera / prev_models (MODEL_DTYPE, the caller's order): the previous frame's, for the motion plane; coverage: an
        (height, width, 4) f32 coverage frame whose covered pixels (alpha +0.0) keep what `into` holds.  last_gbuffer_stats: the counts."""
        p = self._p
        ok = 0 < width <= 32768 and 0 < height <= 32768
        out = {k: (into[k] if into is not None and k in into else gbuffer_plane(desc, k, *((width, height) if ok else (1, 1)))) for k in planes}
        pm = None if prev_models is None else np.ascontiguousarray(prev_models, MODEL_DTYPE)
        cov = None if coverage is None else np.ascontiguousarray(coverage, np.float32)
        words = (C.c_uint64 * 8)()
        ptr = [out[k].ctypes.data if k in out else None for k in GBUFFER_PLANES]
        _lib.check(p._lib.brt_render_gbuffer(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, desc.ctypes.data,
                                             None if prev_camera is None else prev_camera.ctypes.data,
                                             None if pm is None else pm.ctypes.data, None if cov is None else cov.ctypes.data,
                                             *ptr, words), p._ctx)
        self.last_gbuffer_stats = _gbuffer_stats(words)
        return out

    def render_gbuffer_device(self, camera, window, width: int, height: int, desc, d_depth: int = 0, d_normal: int = 0, d_motion: int = 0,
                              d_ids: int = 0, d_albedo: int = 0, prev_camera=None, d_prev_models: int = 0, d_coverage: int = 0,
                              stream: Optional[int] = None, flags: int = 0) -> dict:
        """brt_render_gbuffer_device: the planes whose device pointer (on the first device) is not 0.  Stream rule as for
        render_part_device; the counts of the returned stats only on the own stream."""
        p = self._p
        words = (C.c_uint64 * 8)()
        _lib.check(p._lib.brt_render_gbuffer_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, desc.ctypes.data,
                                                    None if prev_camera is None else prev_camera.ctypes.data, d_prev_models or None,
                                                    d_coverage or None, d_depth or None, d_normal or None, d_motion or None,
                                                    d_ids or None, d_albedo or None, *_stream_args(stream, flags), words), p._ctx)
        self.last_gbuffer_stats = _gbuffer_stats(words)
        return self.last_gbuffer_stats

    def upscale_refine_device(self, camera, window, low_width: int, low_height: int, d_low: int, width: int, height: int, d_out: int,
                              classes: int = REFINE_EDGES | REFINE_SPECULAR, d_refined_count: int = 0, stream: Optional[int] = None,
                              out_format: int = FLAG_OUT_RGBA32F) -> dict:
        """brt_upscale_refine_device: upscale_device with the output pixels of `classes` (REFINE_*) traced at full size.  `window` is the
        FULL-SIZE window; d_refined_count: a device uint32 that receives the number of refined pixels (0: none)."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_upscale_refine_device(p._ctx, camera.ctypes.data, window.ctypes.data, low_width, low_height, d_low or None,
                                                    width, height, d_out or None, int(classes), d_refined_count or None,
                                                    *_stream_args(stream, out_format), C.byref(stats)), p._ctx)
        return stats.as_dict()

    def render_upscaled_refined_device(self, camera, window, low_width: int, low_height: int, width: int, height: int, d_frame: int,
                                       classes: int = REFINE_EDGES | REFINE_SPECULAR, d_refined_count: int = 0,
                                       stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_upscaled_refined_device: the low trace of render_upscaled_device, then upscale_refine_device.  No post-pass flags."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_upscaled_refined_device(p._ctx, camera.ctypes.data, window.ctypes.data, low_width, low_height, width,
                                                             height, d_frame or None, int(classes), d_refined_count or None,
                                                             *_stream_args(stream, out_format | flags),
                                                             C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def upscale_refine_mask_device(self, camera, window, low_width: int, low_height: int, d_low: int, width: int, height: int,
                                   d_mask: int, stream: Optional[int] = None) -> None:
        """brt_upscale_refine_mask_device: the REFINE_* class bits of every output pixel into the width x height bytes at d_mask."""
        p = self._p
        _lib.check(p._lib.brt_upscale_refine_mask_device(p._ctx, camera.ctypes.data, window.ctypes.data, low_width, low_height,
                                                         d_low or None, width, height, d_mask or None, *_stream_args(stream)), p._ctx)

    # -- adaptive sampling (include/bevyray_amd.h "adaptive sampling") -------------------------------

    def render_adaptive_device(self, camera, window, width: int, height: int, d_frame: int, d_selected_count: int = 0,
                               stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_adaptive_device: a base frame at the context's base_spp (RaytracePlugin.set_adaptive), the pixels its rule selects
        traced again at the camera's sample_count.  d_selected_count: a device uint32 that receives their number (0: none).  No
        post-pass flags.  last_stats: the base trace's, rays with the re-trace's on the own stream, total_ms of the whole call."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_adaptive_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_frame or None,
                                                     d_selected_count or None,
                                                     *_stream_args(stream, out_format | flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def adaptive_refine_device(self, camera, window, width: int, height: int, d_base: int, d_out: int, d_selected_count: int = 0,
                               stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F) -> dict:
        """brt_adaptive_refine_device: render_adaptive_device for a base frame (RGBA f32, width x height) the caller holds at d_base."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_adaptive_refine_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_base or None,
                                                     d_out or None, d_selected_count or None,
                                                     *_stream_args(stream, out_format), C.byref(stats)), p._ctx)
        return stats.as_dict()

    def adaptive_mask_device(self, camera, window, width: int, height: int, d_base: int, d_mask: int, stream: Optional[int] = None) -> None:
        """brt_adaptive_mask_device: the ADAPT_* class of every pixel into the width x height bytes at d_mask; traces nothing."""
        p = self._p
        _lib.check(p._lib.brt_adaptive_mask_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_base or None,
                                                   d_mask or None, *_stream_args(stream)), p._ctx)

    # -- progressive frames (include/bevyray_amd.h "progressive frames") -----------------------------

    def progressive_sample_device(self, camera, window, width: int, height: int, d_state: int, target: int, d_pixels: int = 0,
                                  n_pixels: Optional[int] = None, d_count: int = 0, d_frame: int = 0, stream: Optional[int] = None,
                                  out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_progressive_sample_device: the listed pixels (d_pixels 0: every pixel) of the state plane at d_state (PROG_PIXEL_DTYPE,
        width x height) continued to `target` samples; their values scattered into the frame at d_frame (0: none).  A pixel may be
        named at most once per call.  flags: FLAG_KERNEL_SIMPLE for the plain form."""
        p = self._p
        stats = BrtStats()
        n = width * height if n_pixels is None else int(n_pixels)
        _lib.check(p._lib.brt_progressive_sample_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_state or None,
                                                        d_pixels or None, n, d_count or None, int(target), d_frame or None,
                                                        *_stream_args(stream, out_format | flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def progressive_sample(self, camera, window, width: int, height: int, state: np.ndarray, target: int, pixels=None,
                           frame: Optional[np.ndarray] = None, out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_progressive_sample: progressive_sample_device for host arrays, in place: `state` (PROG_PIXEL_DTYPE, height x width,
        C-contiguous), `pixels` (uint32 or None: every pixel) and `frame` (or None)."""
        p = self._p
        stats = BrtStats()
        assert state.dtype == PROG_PIXEL_DTYPE and state.size == width * height and state.flags.c_contiguous
        lst = None if pixels is None else np.ascontiguousarray(pixels, np.uint32)
        if lst is not None and lst.size == 0:       # (a null list means every pixel: an empty one is nothing to do)
            self.last_stats = BrtStats().as_dict()
            return self.last_stats
        n = width * height if lst is None else lst.size
        _lib.check(p._lib.brt_progressive_sample(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, state.ctypes.data,
                                                 None if lst is None else lst.ctypes.data, n, int(target),
                                                 None if frame is None else frame.ctypes.data, out_format | flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def progressive_select_device(self, width: int, height: int, d_state: int, target: int, d_list: int = 0, d_count: int = 0,
                                  d_mask: int = 0, stream: Optional[int] = None) -> None:
        """brt_progressive_select_device: the pixels of the state plane that `target` is still worth under the context's threshold and
        radius (RaytracePlugin.set_progressive): appended to d_list with their number in d_count, class bytes to d_mask (0: none)."""
        p = self._p
        _lib.check(p._lib.brt_progressive_select_device(p._ctx, width, height, d_state or None, int(target), d_list or None, d_count or None,
                                                        d_mask or None, *_stream_args(stream)), p._ctx)

    def render_progressive_device(self, camera, window, width: int, height: int, d_state: int, d_frame: int, stream: Optional[int] = None,
                                  out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_progressive_device: the one-call form -- every pixel to first_spp, then selection and continuation for the targets
        doubling up to max_spp (RaytracePlugin.set_progressive).  The state at d_state is not cleared."""
        p = self._p
        stats = BrtStats()
        _lib.check(p._lib.brt_render_progressive_device(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, d_state or None,
                                                        d_frame or None, *_stream_args(stream, out_format | flags), C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    def render_progressive(self, camera, window, width: int, height: int, state: np.ndarray, frame: np.ndarray,
                           out_format: int = FLAG_OUT_RGBA32F, flags: int = 0) -> dict:
        """brt_render_progressive: render_progressive_device for host arrays, in place."""
        p = self._p
        stats = BrtStats()
        assert state.dtype == PROG_PIXEL_DTYPE and state.size == width * height and state.flags.c_contiguous
        _lib.check(p._lib.brt_render_progressive(p._ctx, camera.ctypes.data, window.ctypes.data, width, height, state.ctypes.data,
                                                 frame.ctypes.data, out_format | flags, C.byref(stats)), p._ctx)
        self.last_stats = stats.as_dict()
        return self.last_stats

    # -- ray queries (include/bevyray_amd.h "ray queries") ------------------------------------------

    def query_rays(self, rays: np.ndarray, mode: int = QUERY_CLOSEST, origin_bound: float = 0.0) -> np.ndarray:
        """brt_query_rays: a batch of RAY_DTYPE records (host memory) against the resident scene -> HIT_DTYPE records.  mode:
        QUERY_CLOSEST / QUERY_ANY; origin_bound > 0 first raises the tree's reach for origins of that 1-norm.  last_query_stats holds
        the call's counts."""
        p = self._p
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.empty(rays.shape, HIT_DTYPE)
        words = (C.c_uint64 * 8)()
        _lib.check(p._lib.brt_query_rays(p._ctx, rays.ctypes.data if rays.size else None, rays.size, int(mode), float(origin_bound),
                                         hits.ctypes.data if rays.size else None, words), p._ctx)
        self.last_query_stats = _stats8(words, ("rays_walked", "n_workgroups"))
        return hits

    def query_rays_device(self, d_rays: int, n_rays: int, d_hits: int, mode: int = QUERY_CLOSEST, origin_bound: float = 0.0,
                          stream: Optional[int] = None) -> dict:
        """brt_query_rays_device: n_rays 32-byte rays at d_rays -> 32-byte hits at d_hits (device pointers on the first device).
        Stream rule as for render_part_device; on a caller's stream the three counts of the returned stats are 0."""
        p = self._p
        words = (C.c_uint64 * 8)()
        _lib.check(p._lib.brt_query_rays_device(p._ctx, d_rays or None, int(n_rays), int(mode), float(origin_bound), d_hits or None,
                                                *_stream_args(stream), words), p._ctx)
        self.last_query_stats = _stats8(words, ("rays_walked", "n_workgroups"))
        return self.last_query_stats

    def query_origin_bound(self) -> float:
        """brt_query_origin_bound: the largest origin 1-norm the resident tree covers (inf: any)."""
        p = self._p
        b = C.c_float(0.0)
        _lib.check(p._lib.brt_query_origin_bound(p._ctx, C.byref(b)), p._ctx)
        return float(b.value)

    # -- radiance queries (include/bevyray_amd.h "radiance queries") --------------------------------

    def radiance_rays(self, rays, samples: int, bounces: int, origin_bound: float = 0.0, device: bool = False,
                      stream: Optional[int] = None):
        """brt_radiance_rays*: path-traced colour for a list of rays -- per entry, seed -> rng_state, `samples` paths of at most
        `bounces` bounces on (origin, direction), averaged.  device=False: `rays` is an array of RADIANCE_RAY_DTYPE records in host
        memory -> RADIANCE_DTYPE records (synchronous).  device=True: `rays` is (d_rays, n_rays, d_out), device pointers on the first
        device -> the call's stats; stream rule as for query_rays_device (on a caller's stream the three counts are 0).
        origin_bound > 0 first raises the tree's reach for origins of that 1-norm.  last_radiance_stats holds the call's stats."""
        p = self._p
        words = (C.c_uint64 * 8)()
        if device:
            d_rays, n_rays, d_out = rays
            _lib.check(p._lib.brt_radiance_rays_device(p._ctx, d_rays or None, int(n_rays), int(samples), int(bounces), float(origin_bound),
                                                       d_out or None, *_stream_args(stream), words),
                       p._ctx)
            self.last_radiance_stats = _stats8(words, ("walks", "n_workgroups"))
            return self.last_radiance_stats
        rays = np.ascontiguousarray(rays, RADIANCE_RAY_DTYPE)
        out = np.empty(rays.shape, RADIANCE_DTYPE)
        _lib.check(p._lib.brt_radiance_rays(p._ctx, rays.ctypes.data if rays.size else None, rays.size, int(samples), int(bounces),
                                            float(origin_bound), out.ctypes.data if rays.size else None, words), p._ctx)
        self.last_radiance_stats = _stats8(words, ("walks", "n_workgroups"))
        return out

    # -- light probes (include/bevyray_amd.h "light probes") ----------------------------------------

    def bake_probes(self, probes, n_dirs: int, bounces: int, basis: int = PROBE_SH9, origin_bound: float = 0.0, device: bool = False,
                    stream: Optional[int] = None):
        """brt_bake_probes*: irradiance records for a list of probes -- per probe n_dirs radiance entries of one sample and at most
        `bounces` bounces, made linear and projected onto `basis` (PROBE_SH9 / PROBE_AMBIENT_CUBE).  device=False: `probes` is an array
        of PROBE_DTYPE records in host memory -> PROBE_RECORD_DTYPE records (synchronous).  device=True: `probes` is (d_probes,
        n_probes, d_out), device pointers on the first device -> the call's stats; stream rule as for radiance_rays.
        last_probe_stats holds the call's stats."""
        lib = self._p._lib
        if device:
            d_probes, n_probes, d_out = probes
            return _bake_call(self, lib.brt_bake_probes_device, d_probes or None, int(n_probes), int(n_dirs), int(bounces), int(basis),
                              float(origin_bound), d_out or None, *_stream_args(stream))
        probes = np.ascontiguousarray(probes, PROBE_DTYPE)
        out = np.empty(probes.shape, PROBE_RECORD_DTYPE)
        _bake_call(self, lib.brt_bake_probes, probes.ctypes.data if probes.size else None, probes.size, int(n_dirs), int(bounces),
                   int(basis), float(origin_bound), out.ctypes.data if probes.size else None)
        return out

    def probe_rays_device(self, d_probes: int, n_probes: int, n_dirs: int, d_rays: int, stream: Optional[int] = None):
        """brt_probe_rays_device: the generation step alone -> n_probes * n_dirs RADIANCE_RAY_DTYPE entries at d_rays, probe-major."""
        p = self._p
        _lib.check(p._lib.brt_probe_rays_device(p._ctx, d_probes or None, int(n_probes), int(n_dirs), d_rays or None,
        *_stream_args(stream)), p._ctx)

    def probe_project_device(self, d_results: int, n_probes: int, n_dirs: int, basis: int, d_out: int, stream: Optional[int] = None):
        """brt_probe_project_device: the projection step alone, n_probes * n_dirs RADIANCE_DTYPE results (probe-major) ->
        n_probes PROBE_RECORD_DTYPE records at d_out."""
        p = self._p
        _lib.check(p._lib.brt_probe_project_device(p._ctx, d_results or None, int(n_probes), int(n_dirs), int(basis), d_out or None,
                                                   *_stream_args(stream)), p._ctx)

    # -- irradiance volumes (include/bevyray_amd.h "irradiance volumes") ----------------------------

    def volume_probes_device(self, volume, d_probes: int, stream: Optional[int] = None):
        """brt_volume_probes_device: the generation kernel alone -> the lattice's PROBE_DTYPE records at d_probes."""
        p = self._p
        v = np.ascontiguousarray(volume, VOLUME_DTYPE).reshape(1)
        _lib.check(p._lib.brt_volume_probes_device(p._ctx, v.ctypes.data, d_probes or None, *_stream_args(stream)), p._ctx)

    def bake_volume(self, volume, n_dirs: int, bounces: int, origin_bound: float = 0.0, d_records: Optional[int] = None,
                    stream: Optional[int] = None):
        """brt_bake_volume*: the records of the lattice `volume` (VOLUME_DTYPE), baked as bake_probes bakes the lattice's probes.
        d_records=None: -> PROBE_RECORD_DTYPE records in host memory (synchronous).  d_records=<device pointer>: the records are written
        there -> the call's stats; stream rule as for bake_probes.  last_probe_stats holds the call's stats."""
        lib = self._p._lib
        v = np.ascontiguousarray(volume, VOLUME_DTYPE).reshape(1)
        if d_records is not None:
            return _bake_call(self, lib.brt_bake_volume_device, v.ctypes.data, int(n_dirs), int(bounces), float(origin_bound),
                              d_records or None, *_stream_args(stream))
        out = np.empty(max(_volume_probe_count(v), 1), PROBE_RECORD_DTYPE)
        _bake_call(self, lib.brt_bake_volume, v.ctypes.data, int(n_dirs), int(bounces), float(origin_bound), out.ctypes.data)
        return out

    def sample_volume(self, volume, records, points, device: bool = False, stream: Optional[int] = None):
        """brt_sample_volume*: irradiance at {position, normal} points from the baked records of `volume`.  device=False: `records`
        (PROBE_RECORD_DTYPE) and `points` (VOLUME_POINT_DTYPE) are host arrays -> VOLUME_SAMPLE_DTYPE (synchronous).  device=True:
        `records` is a device pointer and `points` is (d_points, n_points, d_out); stream rule as for bake_probes."""
        p = self._p
        v = np.ascontiguousarray(volume, VOLUME_DTYPE).reshape(1)
        if device:
            d_points, n_points, d_out = points
            _lib.check(p._lib.brt_sample_volume_device(p._ctx, v.ctypes.data, records or None, d_points or None, int(n_points), d_out or None,
                                                       *_stream_args(stream)), p._ctx)
            return None
        records = np.ascontiguousarray(records, PROBE_RECORD_DTYPE)
        points = np.ascontiguousarray(points, VOLUME_POINT_DTYPE)
        out = np.zeros(points.shape, VOLUME_SAMPLE_DTYPE)
        _lib.check(p._lib.brt_sample_volume(p._ctx, v.ctypes.data, records.ctypes.data if records.size else None,
                                            points.ctypes.data if points.size else None, points.size,
                                            out.ctypes.data if points.size else None), p._ctx)
        return out

    # -- reflection probes (include/bevyray_amd.h "reflection probes") ------------------------------

    def bake_envmap(self, position, size: int, levels: int, samples: int, bounces: int, n_taps: int = 64, seed: int = 0,
                    origin_bound: float = 0.0, d_out: Optional[int] = None, stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F):
        """brt_bake_envmap*: the cube map seen from `position` (edge `size`, a power of two) and its `levels` roughness levels, the
        levels concatenated (envmap_level_offsets).  d_out=None: -> the chain's texels in host memory, (n, 4) f32 or, with
        out_format=FLAG_OUT_RGBA16F, f16 (synchronous).  d_out=<device pointer>: the chain is written there -> the call's stats; stream
        rule as for bake_probes.  last_probe_stats holds the call's stats."""
        lib = self._p._lib
        args = (_f3(position), int(seed), int(size), int(levels), int(samples), int(bounces), int(n_taps), float(origin_bound))
        if d_out is not None:
            return _bake_call(self, lib.brt_bake_envmap_device, *args, d_out or None, *_stream_args(stream, int(out_format)))
        n = envmap_level_offsets(size, levels)[-1] if 0 < int(size) <= 1024 and 0 < int(levels) <= 11 else 1
        out = np.zeros((max(n, 1), 4), np.float16 if out_format == FLAG_OUT_RGBA16F else np.float32)
        _bake_call(self, lib.brt_bake_envmap, *args, out.ctypes.data, int(out_format))
        return out

    def envmap_rays_device(self, position, seed: int, size: int, d_rays: int, stream: Optional[int] = None):
        """brt_envmap_rays_device: the generation step alone -> the 6 * size * size RADIANCE_RAY_DTYPE entries of a cube at d_rays."""
        p = self._p
        _lib.check(p._lib.brt_envmap_rays_device(p._ctx, _f3(position), int(seed), int(size), d_rays or None, *_stream_args(stream)), p._ctx)

    def envmap_resolve_device(self, d_results: int, size: int, d_out: int, stream: Optional[int] = None):
        """brt_envmap_resolve_device: 6 * size * size RADIANCE_DTYPE results -> the level-0 texels (linear rgb, alpha = hit) at d_out."""
        p = self._p
        _lib.check(p._lib.brt_envmap_resolve_device(p._ctx, d_results or None, int(size), d_out or None, *_stream_args(stream)), p._ctx)

    def envmap_downsample_device(self, d_src: int, src_size: int, d_out: int, stream: Optional[int] = None):
        """brt_envmap_downsample_device: the box level of the cube at d_src (edge src_size, even) -> d_out (edge src_size / 2)."""
        p = self._p
        _lib.check(p._lib.brt_envmap_downsample_device(p._ctx, d_src or None, int(src_size), d_out or None, *_stream_args(stream)), p._ctx)

    def envmap_filter_device(self, d_src: int, src_size: int, d_taps: int, n_taps: int, dst_size: int, d_out: int,
                             stream: Optional[int] = None):
        """brt_envmap_filter_device: the filter rule, the cube at d_src and the table at d_taps -> the cube of edge dst_size at d_out.  A
        cosine table (envmap_taps(ENVMAP_TAPS_COSINE, ...)) gives the diffuse map."""
        p = self._p
        _lib.check(p._lib.brt_envmap_filter_device(p._ctx, d_src or None, int(src_size), d_taps or None, int(n_taps), int(dst_size),
                                                   d_out or None, *_stream_args(stream)), p._ctx)

    # -- lightmaps (include/bevyray_amd.h "lightmaps") ----------------------------------------------

    def bake_lightmap(self, points, n_dirs: int, bounces: int, passes: int = 0, wrap_u: bool = False, origin_bound: float = 0.0,
                      device: bool = False, stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F, info: bool = True):
        """brt_bake_lightmap*: per surface point n_dirs radiance entries of one sample and at most `bounces` bounces over the hemisphere
        of its normal, made linear and averaged into a texel, then `passes` dilation passes.  device=False: `points` is an (H, W) array of
        LIGHTMAP_POINT_DTYPE in host memory -> (the (H, W, 4) texels, f32 or with out_format=FLAG_OUT_RGBA16F f16, and the (H, W)
        LIGHTMAP_INFO_DTYPE records or None) (synchronous).  device=True: `points` is (d_points, width, height, d_out, d_info or 0),
        device pointers on the first device -> the call's stats; stream rule as for bake_probes.  last_probe_stats holds the stats."""
        lib = self._p._lib
        tail = (int(n_dirs), int(bounces), int(passes), int(wrap_u), float(origin_bound))
        if device:
            d_points, width, height, d_out, d_info = points
            return _bake_call(self, lib.brt_bake_lightmap_device, d_points or None, int(width), int(height), *tail, d_out or None,
                              d_info or None, *_stream_args(stream, int(out_format)))
        points = np.ascontiguousarray(points, LIGHTMAP_POINT_DTYPE)
        h, w = points.shape
        out = np.zeros((h, w, 4), np.float16 if out_format == FLAG_OUT_RGBA16F else np.float32)
        rec = np.zeros((h, w), LIGHTMAP_INFO_DTYPE) if info else None
        _bake_call(self, lib.brt_bake_lightmap, points.ctypes.data if points.size else None, w, h, *tail,
                   out.ctypes.data if out.size else None, rec.ctypes.data if info and rec.size else None, int(out_format))
        return out, rec

    def lightmap_rays_device(self, d_points: int, n_points: int, n_dirs: int, d_rays: int, stream: Optional[int] = None):
        """brt_lightmap_rays_device: the generation step alone -> n_points * n_dirs RADIANCE_RAY_DTYPE entries at d_rays, point-major."""
        p = self._p
        _lib.check(p._lib.brt_lightmap_rays_device(p._ctx, d_points or None, int(n_points), int(n_dirs), d_rays or None,
                                                   *_stream_args(stream)), p._ctx)

    def lightmap_resolve_device(self, d_results: int, d_points: int, n_points: int, n_dirs: int, d_out: int, d_info: int = 0,
                                stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F):
        """brt_lightmap_resolve_device: the resolve step alone, n_points * n_dirs RADIANCE_DTYPE results (point-major) and their points
        -> n_points texels at d_out and, with d_info, LIGHTMAP_INFO_DTYPE records."""
        p = self._p
        _lib.check(p._lib.brt_lightmap_resolve_device(p._ctx, d_results or None, d_points or None, int(n_points), int(n_dirs),
                                                      d_out or None, d_info or None, *_stream_args(stream, int(out_format))), p._ctx)

    def lightmap_dilate_device(self, d_texels: int, width: int, height: int, passes: int, wrap_u: bool, d_out: int,
                               stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F):
        """brt_lightmap_dilate_device: `passes` dilation passes over the RGBA32F image at d_texels -> d_out (passes = 0 copies)."""
        p = self._p
        _lib.check(p._lib.brt_lightmap_dilate_device(p._ctx, d_texels or None, int(width), int(height), int(passes), int(wrap_u),
                                                     d_out or None, *_stream_args(stream, int(out_format))), p._ctx)

    def deinterleave_device(self, d_tiles: int, n_parts: int, width: int, height: int, d_frame: int,
                            stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F):
        """stream=None: own stream, synchronous.  stream=<handle> (0 = default stream): asynchronous there --
        pass the stream the gather was enqueued on so that the copy kernel runs behind it.  out_format: FLAG_OUT_*."""
        p = self._p
        _lib.check(p._lib.brt_deinterleave_device(p._ctx, d_tiles, n_parts, width, height, d_frame,
        *_stream_args(stream, out_format)), p._ctx)

    def gather_rccl(self, comm: int, rank: int, world: int, d_tile: int, d_tiles_on_root: int, width: int, height: int,
                    d_frame_on_root: int = 0, stream: Optional[int] = None, out_format: int = FLAG_OUT_RGBA32F):
        """brt_gather_rccl: ONE ncclGather of every rank's tile to rank 0 and, there, the de-interleave kernel behind it on the
        same stream.  Stream rule as for render_part_device."""
        p = self._p
        _lib.check(p._lib.brt_gather_rccl(p._ctx, comm, rank, world, d_tile, d_tiles_on_root or None, width, height,
                                          d_frame_on_root or None, *_stream_args(stream, out_format)), p._ctx)
