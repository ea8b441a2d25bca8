"""The refused calls of the twelve device entry points that work on a whole frame behind the tracer (brt_api_post.cpp, brt_api_upscale.cpp,
brt_api_adaptive.cpp), as a table: tests/test_post_refusals.py replays it against tests/golden/post_refusals.json, which
scripts/record_post_refusals.py recorded on the commit before the entry points were folded onto one skeleton.  Nothing here needs a GPU.

An entry point is described by its arguments in order with a valid value each (TABLE[export]["base"]) and by its checks in the order the
library makes them (TABLE[export]["checks"]): a check holds the variants of its fault, a variant the arguments it overrides and the
state of the context it needs.  cases() is every variant alone, and per entry point every pair of ADJACENT checks violated together
(the first variant of each): the text that comes back says which of the two the library looks at first.

Values are symbols the replay resolves (run): "cam" / "win" the perspective camera and the window, "ortho" / "bounces" a camera with
projection_type 1 / bounce_count 0x7fffffff ("ortho_bounces": both), a buffer name an address inside one zeroed device arena (never read or written: every case
is refused before anything is enqueued, and the replay checks that the arena is still zero), None a null pointer, an int itself.
States: "null" (no context), "noscene" (a context without a scene), "policy" (brt_set_policy(1) for the call).

Left out, because the refusal comes only after something was enqueued: a non-perspective camera or an oversized bounce count at the
entry points that trace a frame or zero the selection list first (brt_render_upscaled*, brt_upscale_refine_device,
brt_render_upscaled_refined_device, brt_upscale_refine_mask_device; brt_render_adaptive_device for the bounce count)."""
import bevyray_amd as brt
from helpers import make_buffers, uniforms

LOW, FULL = (8, 4), (16, 8)
OUT_FLAGS = brt.FLAG_CALLER_STREAM | brt.FLAG_OUT_RGBA8_UNORM
POST_FLAGS = OUT_FLAGS | brt.FLAG_DENOISE | brt.FLAG_TEMPORAL
# the arena: name -> (offset, bytes); an overlap is made by passing the output's name for the input (or the count) as well
ARENA = {"low": (0, 512), "base": (1024, 2048), "raster": (4096, 2048), "depth": (6144, 512), "out": (8192, 2048), "mask": (10240, 128),
         "count": (10496, 4)}
ARENA_BYTES = 12288


def _v(label, state=None, **over):
    return (label, over, state)


def _flag_bits(allowed):
    return [_v(f"flag_bit{b}", flags=1 << b) for b in range(32) if not (1 << b) & allowed]


CTX = ("ctx", [_v("ctx_null", "null")])
CAMWIN = ("camwin", [_v("cam_null", cam=None), _v("win_null", win=None)])
NOSCENE = ("noscene", [_v("no_scene", "noscene")])
POLICY = ("policy", [_v("policy", "policy")])
ORTHO = ("projection", [_v("ortho", cam="ortho")])
BOUNCES = ("bounces", [_v("bounces", cam="bounces")])
SIZE = ("size", [_v("w0", w=0), _v("h0", h=0), _v("w32769", w=32769), _v("h32769", h=32769)])
SIZES = ("sizes", [_v("lw0", lw=0), _v("lh0", lh=0), _v("lw_above_w", lw=17), _v("lh_above_h", lh=9), _v("w32769", w=32769, lw=16384),
                   _v("h32769", h=32769, lh=16384), _v("w_above_4lw", lw=3), _v("h_above_4lh", lh=1)])
LEVEL = ("level", [_v("level0", level=0), _v("level4", level=4), _v("level_huge", level=0xffffffff)])
CLASSES = ("classes", [_v("classes0", classes=0), _v("classes4", classes=4), _v("classes7", classes=7)])


def _nulls(*names):
    return ("nulls", [_v(f"{n}_null", **{n: None}) for n in names])


def _flags(allowed):
    return ("flags", _flag_bits(allowed))


def _overlap(name, a, b):
    return (name, [_v(name, **{a: b})])


_DENOISE_TAIL = [NOSCENE, CAMWIN, SIZE, ORTHO, BOUNCES]
_ADAPTIVE = [CAMWIN, SIZE, NOSCENE, ORTHO, POLICY]
_REFINE = [CAMWIN, CLASSES, SIZES, NOSCENE, POLICY]
_W, _H, _LW, _LH = FULL + LOW

TABLE = {
    "brt_denoise_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("w", _W), ("h", _H), ("frame", "base"), ("out", "out"), ("stream", None),
                 ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("frame", "out"), _flags(POST_FLAGS)] + _DENOISE_TAIL},
    "brt_blend_post_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("w", _W), ("h", _H), ("frame", "base"), ("raster", "raster"),
                 ("out", "out"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("frame", "out"), _flags(POST_FLAGS)] + _DENOISE_TAIL},
    "brt_upscale_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("lw", _LW), ("lh", _LH), ("low", "low"), ("w", _W), ("h", _H),
                 ("out", "out"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, CAMWIN, _nulls("low", "out"), _flags(OUT_FLAGS), SIZES, _overlap("out_on_low", "low", "out"), NOSCENE, ORTHO, BOUNCES]},
    "brt_upscale_blend_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("level", 1), ("lw", _LW), ("lh", _LH), ("low", "low"), ("w", _W),
                 ("h", _H), ("raster", "raster"), ("depth", "depth"), ("out", "out"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, CAMWIN, _nulls("low", "out"), _flags(OUT_FLAGS), LEVEL, SIZES, _overlap("out_on_low", "low", "out"),
                   _overlap("out_on_raster", "raster", "out"), _overlap("out_on_depth", "depth", "out"), NOSCENE, ORTHO, BOUNCES]},
    "brt_render_upscaled_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("lw", _LW), ("lh", _LH), ("w", _W), ("h", _H), ("out", "out"),
                 ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, CAMWIN, _nulls("out"), _flags(POST_FLAGS), SIZES, NOSCENE]},
    "brt_render_upscaled_blend_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("level", 1), ("lw", _LW), ("lh", _LH), ("w", _W), ("h", _H),
                 ("raster", "raster"), ("depth", "depth"), ("out", "out"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, CAMWIN, _nulls("out"), _flags(POST_FLAGS), LEVEL, SIZES, _overlap("out_on_raster", "raster", "out"),
                   _overlap("out_on_depth", "depth", "out"), NOSCENE]},
    "brt_upscale_refine_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("lw", _LW), ("lh", _LH), ("low", "low"), ("w", _W), ("h", _H),
                 ("out", "out"), ("classes", 3), ("count", "count"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("low", "out"), _flags(OUT_FLAGS)] + _REFINE + [_overlap("out_on_low", "low", "out"),
                                                                               _overlap("count_in_out", "count", "out")]},
    "brt_render_upscaled_refined_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("lw", _LW), ("lh", _LH), ("w", _W), ("h", _H), ("out", "out"),
                 ("classes", 3), ("count", "count"), ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("out"), _flags(OUT_FLAGS)] + _REFINE + [_overlap("count_in_out", "count", "out")]},
    "brt_upscale_refine_mask_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("lw", _LW), ("lh", _LH), ("low", "low"), ("w", _W), ("h", _H),
                 ("mask", "mask"), ("stream", None), ("flags", 0)],
        "checks": [CTX, _nulls("low", "mask"), _flags(brt.FLAG_CALLER_STREAM)] + [c for c in _REFINE if c is not CLASSES]
                  + [_overlap("mask_on_low", "low", "mask")]},
    "brt_render_adaptive_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("w", _W), ("h", _H), ("out", "out"), ("count", "count"), ("stream", None),
                 ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("out"), _flags(OUT_FLAGS)] + _ADAPTIVE + [_overlap("count_in_out", "count", "out")]},
    "brt_adaptive_refine_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("w", _W), ("h", _H), ("frame", "base"), ("out", "out"), ("count", "count"),
                 ("stream", None), ("flags", 0), ("stats", None)],
        "checks": [CTX, _nulls("frame", "out"), _flags(OUT_FLAGS)] + _ADAPTIVE + [_overlap("out_on_base", "frame", "out"),
                                                                                 _overlap("count_in_out", "count", "out"), BOUNCES]},
    "brt_adaptive_mask_device": {
        "base": [("ctx", "ctx"), ("cam", "cam"), ("win", "win"), ("w", _W), ("h", _H), ("frame", "base"), ("mask", "mask"), ("stream", None),
                 ("flags", 0)],
        "checks": [CTX, _nulls("frame", "mask"), _flags(brt.FLAG_CALLER_STREAM)] + _ADAPTIVE + [_overlap("mask_on_base", "frame", "mask"), BOUNCES]},
}
EXPORTS = tuple(TABLE)


def _states(*states):
    """the states of the variants of one case; "null" beside another state: there is no context to be in that state"""
    s = sorted({x for x in states if x})
    return ["null"] if "null" in s else s


def cases():
    """-> [{"id", "export", "faults" (1 or 2), "args" (in order, symbolic), "states"}], ids unique"""
    out = []
    for export, entry in TABLE.items():
        base = dict(entry["base"])

        def case(cid, n, over, states):
            args = dict(base, **over)
            out.append({"id": f"{export}:{cid}", "export": export, "faults": n, "args": [args[k] for k, _ in entry["base"]], "states": states})

        checks = entry["checks"]
        for name, variants in checks:
            for label, over, state in variants:
                case(label, 1, over, _states(state))
        for (_, va), (_, vb) in zip(checks, checks[1:]):
            (la, oa, sa), (lb, ob, sb) = va[0], vb[0]
            both = dict(oa, **ob)
            for k in set(oa) & set(ob):                         # (two faults of one camera: the camera that has both)
                assert k == "cam", (export, la, lb)
                both[k] = f"{oa[k]}_{ob[k]}"
            case(f"{la}+{lb}", 2, both, _states(sa, sb))
    assert len({c["id"] for c in out}) == len(out)
    return out


def scene():
    """the three spheres every case is refused over (a caller-built tree: no call has a reach to settle)"""
    m = brt.StandardMaterial(base_color=(0.8, 0.3, 0.3))
    return make_buffers([((0.0, 0.0, 0.0), 1.0, m), ((2.5, 0.0, -1.0), 1.0, m), ((-2.5, 0.5, 1.0), 1.5, m)])


def symbols(arena_ptr, spp=4):
    """what the symbolic values of a case stand for (the arrays are returned to keep them alive) -> ({symbol: address}, arrays)"""
    _, cam, win = uniforms(FULL[0], FULL[1], spp=spp, bounces=3, pos=(0.0, 1.0, 8.0), target=(0.0, 0.0, 0.0), fov=0.8, seed=0.5)
    ortho, bounces, both = cam.copy(), cam.copy(), cam.copy()
    ortho["projection"] = both["projection"] = 1
    bounces["bounce_count"] = both["bounce_count"] = 0x7fffffff
    arrays = {"cam": cam, "win": win, "ortho": ortho, "bounces": bounces, "ortho_bounces": both}
    out = {k: a.ctypes.data for k, a in arrays.items()}
    out.update({k: arena_ptr + off for k, (off, _) in ARENA.items()})
    return out, arrays


def run(lib, ctx_scene, ctx_noscene, arena_ptr, table=None):
    """Every case on the two contexts (raw pointers) -> {id: [return code, brt_last_error text]}"""
    syms, _keep = symbols(arena_ptr)
    got = {}
    for c in cases() if table is None else table:
        states = c["states"]
        ctx = None if "null" in states else ctx_noscene if "noscene" in states else ctx_scene
        args = [ctx if a == "ctx" else syms[a] if isinstance(a, str) else a for a in c["args"]]
        if "policy" in states:
            assert lib.brt_set_policy(ctx, brt.POLICY_OR_SHORT_CIRCUIT) == 0
        try:
            rc = getattr(lib, c["export"])(*args)
            text = lib.brt_last_error(ctx)
        finally:
            if "policy" in states:
                assert lib.brt_set_policy(ctx, 0) == 0
        got[c["id"]] = [int(rc), (text or b"").decode("utf-8", "replace")]
    return got


def pack(got):
    """{id: [code, text]} -> the golden file's form: the distinct answers once, and per export {case: index of its answer}"""
    answers = sorted({(rc, text) for rc, text in got.values()}, key=lambda a: (-a[0], a[1]))
    cases = {}
    for cid, (rc, text) in got.items():
        export, label = cid.split(":", 1)
        cases.setdefault(export, {})[label] = answers.index((rc, text))
    return {"answers": [list(a) for a in answers], "cases": cases}


def unpack(doc):
    return {f"{export}:{label}": list(doc["answers"][i]) for export, table in doc["cases"].items() for label, i in table.items()}


def run_on_gpu():
    """run() on two fresh contexts of the loaded library; the arena must come back untouched"""
    import torch
    arena = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    with brt.RaytracePlugin([0]) as with_scene, brt.RaytracePlugin([0]) as without:
        with_scene.node.write_buffers(scene())
        got = run(with_scene._lib, with_scene._ctx, without._ctx, arena.data_ptr())
        torch.cuda.synchronize()
    assert not bool(arena.any()), "a refused call wrote to a buffer"
    return got
