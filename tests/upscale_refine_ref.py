"""numpy restatement of the refined upsampling (DESIGN.md "Refined upsampling", brt_upscale_refine*) on top of tests/upscale_ref.py: the two
class tests of an output pixel, and the refined frame as "the upsampled frame with the selected pixels replaced by the full-size frame's".
Both tests are exact: with guides that are bitwise the kernel's, the selected set is the kernel's."""
import numpy as np

import upscale_ref as ur

EDGES, SPECULAR = 1, 2          # BRT_REFINE_EDGES, BRT_REFINE_SPECULAR


def class_mask(stage, g_full, materials):
    """(h, w) u8 of class bits.  stage: upscale_ref.upscale's stage plane; g_full: the full-size guides (h, w, 8); materials: the scene's
    MATERIAL_DTYPE array in the caller's order (the guides hold the caller's material ids).
    EDGES: a hit pixel that stage A does not serve (no tap of its 2x2 footprint is eligible).  SPECULAR: a hit pixel whose material
    has metallic > 0 or specular_transmission > 0.  The sky has no class."""
    hit = g_full[..., 3] < ur.INF
    mid = np.ascontiguousarray(g_full[..., 7]).view(np.uint32)
    mats = np.asarray(materials)
    spec_of = (mats["metallic"].astype(np.float32) > 0) | (mats["specular_transmission"].astype(np.float32) > 0)
    spec = np.zeros(hit.shape, bool)
    spec[hit] = spec_of[mid[hit]]
    edges = hit & (stage != ur.STAGE_A)
    return (edges.astype(np.uint8) * EDGES) | (spec.astype(np.uint8) * SPECULAR)


def selected(mask, classes):
    return (mask & np.uint8(classes)) != 0


def refine(upscaled, full, mask, classes):
    """The refined frame: `upscaled` (h, w, c) with the pixels selected under `classes` replaced by those of `full` (same shape and
    dtype: both already in the store format)."""
    out = upscaled.copy()
    sel = selected(mask, classes)
    out[sel] = full[sel]
    return out


def selected_mse(frame, ref, sel):
    d = frame[..., :3][sel].astype(np.float64) - ref[..., :3][sel].astype(np.float64)
    return float(np.mean(d * d))
