"""bevyray_amd -- MI355X-native path-tracing render node behind bevyray's plugin surface.

Only the hot path of GrandmasterB42/bevyray is here: the per-pixel ray loop
(assets/shaders/*.wgsl) as hand-written HIP kernels for gfx950, behind the C ABI declared in
include/bevyray_amd.h, plus the host-side mirror of the plugin types that feed it.
Importing the package builds/loads the HIP library; without it nothing renders.
"""
from . import _lib
from ._lib import BrtError, build, load
from .raytracing import (  # noqa: F401
    BVH_NODE_DTYPE, CAMERA_DTYPE, EXTMEM_DMABUF_FD, EXTMEM_OPAQUE_FD, FLAG_CALLER_STREAM, FLAG_COUNTERS, FLAG_DENOISE, FLAG_KERNEL_SIMPLE, FLAG_TEMPORAL, FLAG_BLEND_POST, FLAG_OUT_RGBA16F, FLAG_OUT_RGBA32F, FLAG_OUT_RGBA8_UNORM, FLAG_OUT_RGBA8_UNORM_SRGB, OUT_PIXEL_BYTES, POLICY_MINMAX_SELECT, POLICY_OR_SHORT_CIRCUIT, POLICY_POW_EXP2_LOG2, LEVEL_DTYPE, MATERIAL_DTYPE, MODEL_DTYPE,
    SCENE_COVER, SCENE_RTIOW_FINAL, SCENE_STRESS_GRID, STRIP_ROWS, WINDOW_DTYPE, Buffers, CameraExtract,
    OrthographicProjection, PerspectiveProjection, RaytracedCamera, RaytracedSphere, RaytraceMaterial, RaytracePlugin,
    Raytracing, RayTracingNode, StandardMaterial, Transform, WindowExtract, build_bvh, build_bvh_sah, cover_camera, generate_scene, tree_reach,
    PROG_DEFAULT_THRESHOLD, PROG_PIXEL_DTYPE, PROG_SELECTED, progressive_accumulate, progressive_class,
    ADAPT_DEFAULT_THRESHOLD, ADAPT_NOISY, ADAPT_SPARSE, HIT_DTYPE, REFINE_EDGES, REFINE_SPECULAR, adaptive_class, QUERY_ANY, QUERY_CLOSEST, QUERY_NONE, QUERY_STATUS_FRONT_FACE, QUERY_STATUS_HIT, QUERY_STATUS_INVALID, QUERY_STATUS_MISS,
    QUERY_STATUS_OUT_OF_REACH, RADIANCE_DTYPE, RADIANCE_RAY_DTYPE, RAY_DTYPE, pixel_ray,
    PROBE_AMBIENT_CUBE, PROBE_DTYPE, PROBE_RECORD_DTYPE, PROBE_SH9, probe_directions, probe_irradiance,
    VOLUME_DTYPE, VOLUME_POINT_DTYPE, VOLUME_SAMPLE_DTYPE, VOLUME_STATUS_CLAMPED, VOLUME_STATUS_INVALID, VOLUME_STATUS_NO_PROBE, VOLUME_WRAP,
    make_volume, volume_probes, volume_sample_host,
    ENVMAP_TAP_DTYPE, ENVMAP_TAPS_COSINE, ENVMAP_TAPS_GGX, ENVMAP_TEXEL16_DTYPE, ENVMAP_TEXEL_DTYPE, envmap_directions,
    envmap_downsample_host, envmap_filter_host, envmap_level_offsets, envmap_taps,
    LIGHTMAP_INFO_DTYPE, LIGHTMAP_POINT_DTYPE, LIGHTMAP_STATUS_EMPTY, lightmap_dilate_host, lightmap_directions, lightmap_ray,
    lightmap_sphere_points,
    LENS_DTYPE, lens, lens_origin_bound, lens_ray, lens_seed,
    GBUFFER_DEPTH_DISTANCE, GBUFFER_DEPTH_SHADER, GBUFFER_DEPTH_VIEW, GBUFFER_DTYPE, GBUFFER_IDS_DTYPE, GBUFFER_MOTION_PIXEL,
    GBUFFER_MOTION_UV16F, GBUFFER_MOTION_UV32F, GBUFFER_NORMAL_RGB10A2, GBUFFER_NORMAL_RGBA32F, GBUFFER_PIXEL_DTYPE, GBUFFER_PLANES,
    GBUFFER_STATUS_FRONT_FACE, GBUFFER_STATUS_HIT, GBUFFER_STATUS_MOVED, GBUFFER_STATUS_NO_PREVIOUS, gbuffer, gbuffer_pixel, gbuffer_plane,
    blend_covered, prepare_buffers, rtiow_camera, srgb_thresholds, tile_rows, upscale_window, validate_scene,
)

__all__ = [n for n in dir() if not n.startswith("_")]
