"""Sequences of calls over ONE context, and what each call must return: the generator and the CPU model of tests/test_call_sequences.py
(and of scripts/sequence_soak.py --families).  Nothing here needs a GPU.

A step is one call of one of twelve entry-point families (FAMILIES); an event (EVENTS) may sit in front of it.  Every shape, form and
stream of a step is drawn from the step's own seed, so a step's description does not depend on what a GPU answered.  The sequences:
  * covering: an Eulerian circuit of the complete directed graph on the families, self-loops included (144 edges: every ordered pair of
    families adjacent exactly once), drawn by seed and cut into 12 chunks of 13 steps that overlap by one step;
  * random: RANDOM_SEEDS sequences of 10 steps, families uniform, an event before every step.
The model (expect) states, bit for bit and from the CPU references alone, what a call of the families in LAYER_A returns on the tree
the context reports (`tree_reach` of the call's stats; the origin bound the context reports decides which list entries are refused).
The families in LAYER_B (post-processed, upscaled and adaptive frames) need guides and history: the test replays them on a control
context instead, which sees of a step of another family only the request that step makes of the tree's reach."""
import functools
import zlib

import numpy as np

import bevyray_amd as brt
import envmap_ref as er
import lens_ref
import lightmap_ref as lm
import probe_ref as pr
import query_ref as qr
import radiance_ref as rr
import volume_ref as vr
from helpers import random_scene, random_view, uniforms

F32 = np.float32
FAMILIES = ("frame", "post", "upscaled", "adaptive", "pixels", "lens", "query", "radiance", "probes", "volume", "envmap", "lightmap")
LAYER_B = ("post", "upscaled", "adaptive")
LAYER_A = tuple(f for f in FAMILIES if f not in LAYER_B)
EVENTS = ("same", "move", "jump", "far", "animate", "add")
CAMERA_FAMILIES = ("frame", "post", "upscaled", "adaptive", "pixels", "lens")     # their camera decides the tree's reach
COVERING_SEED = 68
RANDOM_SEEDS = (1101, 1102, 1103, 1104, 1105, 1106)
N_CHUNKS, CHUNK_STEPS, RANDOM_STEPS = 12, 13, 10
BOUNCES, BAKE_BOUNCES = 3, 2
LENS_SIZE, ADAPTIVE_SIZE = (48, 27), (64, 36)
UPSCALE_PAIRS = ((64, 36, 32, 18), (33, 31, 9, 8))         # (width, height, low width, low height); the odd pair: test_upscale_synthetic.py
FORMATS = {"f32": brt.FLAG_OUT_RGBA32F, "f16": brt.FLAG_OUT_RGBA16F, "unorm8": brt.FLAG_OUT_RGBA8_UNORM, "srgb8": brt.FLAG_OUT_RGBA8_UNORM_SRGB}
STREAMS = ("own", "s1", "s2")
REFUSED_BITS = brt.QUERY_STATUS_INVALID | brt.QUERY_STATUS_OUT_OF_REACH


# ---- the walk ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def covering_walk(seed=COVERING_SEED):
    """The vertices of an Eulerian circuit of the complete digraph on len(FAMILIES) vertices with self-loops (Hierholzer over edge lists
    shuffled by `seed`): 145 entries, the first equal to the last."""
    n = len(FAMILIES)
    rng = np.random.default_rng(seed)
    out = [[int(v) for v in rng.permutation(n)] for _ in range(n)]
    stack, walk = [int(rng.integers(n))], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return tuple(walk)


def specs():
    """-> [(name, kind, seed, the families of its steps, the chance of an event before a step)]"""
    walk = covering_walk()
    out = []
    for c in range(N_CHUNKS):
        fams = tuple(FAMILIES[v] for v in walk[c * (CHUNK_STEPS - 1): c * (CHUNK_STEPS - 1) + CHUNK_STEPS])
        out.append((f"cover{c:02d}", "covering", COVERING_SEED * 100 + c, fams, 1.0 / 3.0))
    for s in RANDOM_SEEDS:
        out.append(random_spec(s))
    return out


def random_spec(seed):
    rng = np.random.default_rng([seed, 7])
    return (f"random{seed}", "random", seed, tuple(FAMILIES[int(v)] for v in rng.integers(0, len(FAMILIES), RANDOM_STEPS)), 1.0)


# ---- the generator ----------------------------------------------------------------------------------------------------------------

class Step:
    """One call: `event` in front of it (or None), `upload` (the models to upload first, or None), `models` (the caller's models the call
    sees), `vdesc` (pos, target, fov, seed of the view), `v` (the drawn variant: plain values) and `inp` (the drawn arrays)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def describe(self):
        return f"step {self.index} {self.family} {self.v} stream {self.stream} event {self.event}"


class Sequence:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def view(self, step, w=None, h=None, spp=None, level=3):
        """(level, camera, window) of a step's view for a frame of w x h (the sequence's own size by default)"""
        w, h = (self.w, self.h) if w is None else (w, h)
        pos, target, fov, seed = step.vdesc
        return uniforms(w, h, spp=self.spp if spp is None else spp, bounces=BOUNCES, pos=pos, target=target, fov=fov, seed=seed,
                        level=brt.Raytracing(level))

    def buffers(self, step, bvh):
        return brt.Buffers(step.models, self.materials, bvh)


def _pick(rng, options):
    return options[int(rng.integers(len(options)))]


def _balanced(family, key, options, occurrence):
    """The value of a variant key for the `occurrence`-th step of `family` over all committed sequences: the options in one random
    permutation after another (seeded by family and key), so that every option is drawn once in len(options) steps of the family and
    the keys stay independent of one another."""
    n = len(options)
    perm = np.random.default_rng([FAMILIES.index(family), zlib.crc32(key.encode()), occurrence // n]).permutation(n)
    return options[int(perm[occurrence % n])]


def _occurrence_base(name, seed):
    """How many steps of each family the committed sequences in front of sequence `name` hold (another sequence: a base from its seed)"""
    base = dict.fromkeys(FAMILIES, 0)
    for spec in specs():
        if spec[0] == name:
            return base
        for f in spec[3]:
            base[f] += 1
    return dict.fromkeys(FAMILIES, 7 * seed)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F32)


def _far_origin(rng, spread, k):
    """An origin no tree of the scene's own extent reaches, further out with every use (k), so that a request for it raises the reach"""
    d = _unit(rng, 1)[0].astype(np.float64)
    return (d * spread * 60.0 * 1.6 ** k).astype(F32)


def l1(origins):
    a = np.abs(np.asarray(origins, F32).reshape(-1, 3))
    return ((a[:, 0] + a[:, 1]) + a[:, 2]).astype(F32)


def _inside(rng, spread, n, ground):
    """n positions in the middle of the scene (above the ground where there is one)"""
    p = rng.uniform(-0.4 * spread, 0.4 * spread, (n, 3))
    if ground:
        p[:, 1] = rng.uniform(0.05 * spread, 0.4 * spread, n)
    return p.astype(F32)


def _draw(seq, step, rng, oracle, state, occurrence):
    """The variant and the inputs of a step of its family, from the step's own rng"""
    fam, spread, models = step.family, seq.spread, step.models
    v, inp = {}, {}
    bal = lambda key, options: _balanced(fam, key, options, occurrence)          # noqa: E731
    ground = bool(abs(float(models["radius"][0])) > 100.0)
    if fam == "frame":
        target = bal("target", ("run",) + tuple(FORMATS))                # brt_render stores f32 alone
        v["call"], v["format"] = ("run", "f32") if target == "run" else ("render_device", target)
        v["level"] = int(bal("level", (1, 2, 3)))
        v["counters"] = bool(bal("counters", (True, False)))
    elif fam == "post":
        v["flags"] = bal("flags", ("denoise", "temporal", "denoise+temporal"))
    elif fam == "upscaled":
        kind = bal("call", ("plain", "refined", "blend1", "blend2"))           # (a blended frame at level 1 or 2)
        v["call"] = kind.rstrip("12")
        v["pair"] = bal("pair", (UPSCALE_PAIRS[0], UPSCALE_PAIRS[0], UPSCALE_PAIRS[1]))
        v["level"] = int(kind[-1]) if v["call"] == "blend" else 3
        if v["call"] == "blend":
            w, h = v["pair"][:2]
            inp["raster"] = rng.random((h, w, 4), dtype=np.float32)
            inp["depth"] = rng.random((h, w), dtype=np.float32) * np.float32(0.05)
    elif fam == "adaptive":
        pass
    elif fam == "pixels":
        v["call"] = bal("call", ("host", "device"))
        v["form"] = int(bal("form", (1, 2)))
        inp["pixels"] = rng.permutation(seq.w * seq.h)[:300].astype(np.uint32)
    elif fam == "lens":
        v["call"] = bal("call", ("render_lens", "render_lens_pixels", "render_lens_pixels_device"))
        v["mode"] = bal("mode", ("thin", "ortho"))
        pos, target = np.asarray(step.vdesc[0]), np.asarray(step.vdesc[1])
        dist = float(np.linalg.norm(pos - target))
        v["lens"] = (round(0.02 * dist, 6), round(dist, 6), 0.0) if v["mode"] == "thin" else (0.0, 1.0, round(1.5 * spread, 6))
        inp["pixels"] = rng.permutation(LENS_SIZE[0] * LENS_SIZE[1])[:200].astype(np.uint32)
        inp["spot"] = rng.permutation(200)[:3]                         # the entries the restated lens pixel is computed for
    elif fam in ("query", "radiance"):
        v["call"] = bal("call", ("host", "device"))
        raise_reach = bool(bal("origin_bound", (True, False)))
        far = _far_origin(rng, spread, state["far_uses"])
        state["far_uses"] += 1
        v["origin_bound"] = float(l1(far)[0]) if raise_reach else 0.0
        targets = models["position"][rng.integers(0, len(models), 16)].astype(F32)
        if fam == "query":
            v["mode"] = bal("mode", ("closest", "occlusion"))
            _, cam, _ = seq.view(step)
            tree = brt.build_bvh_sah(models, 0.0)
            sets = qr.ray_sets(oracle, models, tree, cam, seq.w, seq.h, rng, n=96)
            rays = np.concatenate([sets[k] for k in sorted(sets)] + [qr.make_rays(np.broadcast_to(far, targets.shape), targets - far)])
            rays["user"] = np.arange(len(rays), dtype=np.uint32) * np.uint32(2654435761)
            inp["rays"] = rays
        else:
            v["form"] = int(bal("form", (1, 2)))
            n = 496
            cam_pos = np.asarray(step.vdesc[0], F32)
            aim = rng.uniform(-spread, spread, (n // 2, 3)).astype(F32)
            o = np.concatenate([np.broadcast_to(cam_pos, aim.shape), rng.uniform(-spread, spread, (n // 2, 3)).astype(F32),
                                np.broadcast_to(far, targets.shape)])
            d = np.concatenate([aim - cam_pos, _unit(rng, n // 2), targets - far])
            inp["rays"] = rr.make_rays(o, d, rng.integers(0, 2 ** 32, size=len(o), dtype=np.uint32))
            v["samples"] = 2
    elif fam == "probes":
        v["call"] = bal("call", ("host", "device"))
        v["basis"] = bal("basis", ("sh9", "cube"))
        v["n_dirs"] = int(bal("n_dirs", (16, 64)))
        probes = np.zeros(8, brt.PROBE_DTYPE)
        probes["position"] = _inside(rng, spread, 8, ground)
        probes["seed"] = rng.integers(0, 2 ** 32, size=8, dtype=np.uint32)
        inp["probes"] = probes
    elif fam == "volume":
        v["bake"] = bal("bake", ("host", "device"))
        v["sample"] = bal("sample", ("host", "device"))
        v["basis"] = bal("basis", ("sh9", "cube"))
        v["n_dirs"] = int(bal("n_dirs", (16, 64)))
        lo = _inside(rng, spread, 1, ground)[0] * F32(0.5)
        space = float(0.3 * spread)
        inp["volume"] = brt.make_volume(tuple(float(x) for x in lo), (space, space, space), (2, 2, 2),
                                        brt.PROBE_SH9 if v["basis"] == "sh9" else brt.PROBE_AMBIENT_CUBE, int(rng.integers(2 ** 32)), 0)
        pts = np.zeros(100, brt.VOLUME_POINT_DTYPE)
        pts["position"] = (lo[None, :] + rng.uniform(-0.2, 1.2, (100, 3)) * space).astype(F32)
        pts["normal"] = _unit(rng, 100)
        inp["points"] = pts
    elif fam == "envmap":
        v["call"] = bal("call", ("host", "device"))
        v["levels"], v["n_taps"] = bal("levels", ((3, 16), (4, 8)))
        v["format"] = bal("format", ("f32", "f16"))
        v["chunk_rays"] = int(bal("chunk_rays", (0, 128)))                    # 0: the default; 128: the 384 entries in three chunks
        v["position"] = tuple(float(x) for x in _inside(rng, spread, 1, ground)[0] * F32(0.5))
        v["seed"] = int(rng.integers(2 ** 32))
    elif fam == "lightmap":
        v["call"] = bal("call", ("host", "device"))
        v["n_dirs"] = int(bal("n_dirs", (16, 64)))
        v["passes"] = int(bal("passes", (0, 2)))
        v["wrap_u"] = bool(bal("wrap_u", (True, False)))
        v["format"] = bal("format", ("f32", "f16"))
        near = np.argsort(np.abs(models["position"].astype(np.float64)).sum(axis=1) + np.where(np.abs(models["radius"]) > 100.0, 1e9, 0.0))
        i = int(near[int(rng.integers(min(8, len(near))))])
        r = float(models["radius"][i])
        pts = brt.lightmap_sphere_points(models["position"][i], r, 16, 8, seed=int(rng.integers(2 ** 32)), offset=1e-3 * r).copy()
        pts["normal"][2] = 0                                           # an EMPTY row: the dilation has something to fill
        inp["points"] = pts
    return v, inp


def generate(spec, oracle):
    """The sequence of `spec` (an entry of specs()): a pure function of the spec (the oracle is used for the hit points that
    query_ref.ray_sets starts rays from)."""
    name, kind, seed, fams, p_event = spec
    rng = np.random.default_rng([seed, 1])
    b, spread = random_scene(rng, max_spheres=600)
    models = b.models.copy()
    w, h = _pick(rng, ((61, 35), (64, 36)))
    spp = int(_pick(rng, (32, 8)))
    n_pairs = len(models) - 1
    tile = int(rng.integers(8, max(9, n_pairs // 2))) if rng.integers(2) else 0
    raster = rng.random((h, w, 4), dtype=np.float32)
    depth = rng.random((h, w), dtype=np.float32) * np.float32(0.05)
    seq = Sequence(name=name, kind=kind, seed=seed, spread=spread, materials=b.materials, w=w, h=h, spp=spp, tile=tile, raster=raster,
                   depth=depth, steps=[])
    _, vdesc = random_view(rng, spread, w, h, spp, BOUNCES)
    state = {"far_uses": 0}
    occurrence = _occurrence_base(name, seed)
    upload = models
    for i, fam in enumerate(fams):
        event = _pick(rng, EVENTS) if (i > 0 and rng.random() < p_event) else None
        if event == "move":
            _, vdesc = random_view(rng, spread, w, h, spp, BOUNCES, near_to=vdesc)
        elif event in ("jump", "far"):
            _, vdesc = random_view(rng, spread, w, h, spp, BOUNCES, far=event == "far")
        elif event == "animate":
            models = models.copy()
            for k in rng.integers(0, len(models), int(rng.integers(1, 6))):
                if abs(float(models["radius"][k])) < 100.0:
                    models["position"][k] += rng.normal(0.0, float(_pick(rng, (1e-3, 0.05))), 3).astype(np.float32)
            upload = models
        elif event == "add":
            if rng.random() < 0.5 and len(models) > 80:
                models = np.delete(models, int(rng.integers(1, len(models))))
            else:
                models = np.concatenate([models, models[-1:]])
                models["position"][-1] += np.float32(0.37)
            raw = np.zeros(len(models), brt.MODEL_DTYPE)               # (delete / concatenate re-pack the padded record)
            for f in brt.MODEL_DTYPE.names:
                raw[f] = models[f]
            models = upload = raw
        step = Step(index=i, family=fam, event=event, upload=upload, models=models, vdesc=vdesc,
                    stream=_pick(np.random.default_rng([seed, 3, i]), STREAMS))
        step.v, step.inp = _draw(seq, step, np.random.default_rng([seed, 2, i]), oracle, state, occurrence[fam])
        occurrence[fam] += 1
        seq.steps.append(step)
        upload = None
    return seq


# ---- what the contexts' buffers of the frame-level calls see ----------------------------------------------------------------------
ADAPTIVE_BASE_SPP = 8           # RaytracePlugin.set_adaptive's default: a sequence of spp <= 8 traces the plain frame, no base frame


def _context_frame_bytes(step):
    """what a step needs of the frame the context keeps between two stages of a call (the low frame of an upscaled step, the base frame
    of an adaptive one; brt_frame.h context_frame)"""
    if step.family == "upscaled":
        return step.v["pair"][2] * step.v["pair"][3] * 16
    return ADAPTIVE_SIZE[0] * ADAPTIVE_SIZE[1] * 16 if step.family == "adaptive" else 0


def frame_grows_on_a_caller_stream(seq):
    """-> the adaptive steps on a caller's stream at which the context's frame, last used by an upscaled step, has to grow"""
    if seq.spp <= ADAPTIVE_BASE_SPP:
        return []
    out, have, last = [], 0, None
    for s in seq.steps:
        need = _context_frame_bytes(s)
        if need:
            if s.family == "adaptive" and last == "upscaled" and need > have and s.stream != "own":
                out.append(s.index)
            have, last = max(have, need), s.family
    return out


def refined_follows_adaptive(seq):
    """-> the refined upscaled steps behind an adaptive step that selected: the selection list (DeviceCtx::d_pxbuf) serves both tails"""
    if seq.spp <= ADAPTIVE_BASE_SPP:
        return []
    first = next((s.index for s in seq.steps if s.family == "adaptive"), None)
    return [s.index for s in seq.steps if first is not None and s.index > first and s.family == "upscaled" and s.v["call"] == "refined"]


def fixed_frame_grows(oracle):
    """One fixed sequence at the module's sizes, which the drawn ones lack: an upscaled frame (low frame 32x18) on one caller stream, the
    adaptive frame (base frame 64x36: the context's frame grows) on another, then a refined upscaled frame on the first."""
    seq = generate(("fixed_frame_grows", "fixed", 4242, ("upscaled", "adaptive", "upscaled"), 0.0), oracle)
    seq.spp = 32
    for s, stream, v in zip(seq.steps, ("s1", "s2", "s1"), ({"call": "plain"}, {}, {"call": "refined"})):
        s.stream = stream
        if v:
            s.v, s.inp = dict(v, pair=UPSCALE_PAIRS[0], level=3), {}
    return seq


def description(seq):
    """The whole sequence as bytes-comparable text: the determinism test compares two of these"""
    lines = [f"{seq.name} {seq.w}x{seq.h} spp {seq.spp} tile {seq.tile} spread {seq.spread}"]
    for s in seq.steps:
        lines.append(s.describe() + f" upload {None if s.upload is None else len(s.upload)} view {s.vdesc} "
                     + " ".join(f"{k}:{np.ascontiguousarray(a).tobytes().hex()[:64]}:{np.ascontiguousarray(a).size}" for k, a in sorted(s.inp.items())))
    return "\n".join(lines)


# ---- the model --------------------------------------------------------------------------------------------------------------------

_TWINS = {}


def twin(models, reach):
    """The CPU twin of the callee's tree over `models` at the reach a call reported"""
    key = (models.tobytes(), float(reach))
    if key not in _TWINS:
        if len(_TWINS) > 64:
            _TWINS.clear()
        _TWINS[key] = brt.build_bvh_sah(models, float(reach))
    return _TWINS[key]


def needed_reach(seq, step):
    """The reach brt_host_tree_reach asks for a camera-driven step's camera (None: the family has no camera)"""
    if step.family not in CAMERA_FAMILIES:
        return None
    return brt.tree_reach(step.models, seq.view(step)[1])[2]


def radiance_expected(oracle, b, rays, samples, bounces, bound):
    """The records of a radiance list on the tree of `b`: entries with a non-finite word are INVALID, origins beyond `bound` (the
    1-norm the context reports it covers) OUT_OF_REACH, both stored as brt_radiance.hip radiance_store_refused stores them; the others
    are the C oracle's."""
    rays = np.ascontiguousarray(rays, brt.RADIANCE_RAY_DTYPE).reshape(-1)
    out = np.zeros(len(rays), brt.RADIANCE_DTYPE)
    finite = np.isfinite(rays["origin"]).all(axis=1) & np.isfinite(rays["direction"]).all(axis=1)
    with np.errstate(invalid="ignore"):
        far = finite & (l1(rays["origin"]) > F32(bound))
    ok = finite & ~far
    out["t"], out["sphere"], out["material"], out["user"] = np.inf, brt.QUERY_NONE, brt.QUERY_NONE, rays["user"]
    out["status"] = np.where(far, brt.QUERY_STATUS_OUT_OF_REACH, brt.QUERY_STATUS_INVALID)
    if ok.any():
        res, _ = oracle.radiance(b, rays[ok], samples, bounces)
        out[ok] = res
    return out, ok


def lens_of(seq, step):
    """(camera, window, lens descriptor) of a lens step: one sample per pixel (the restated lens pixel runs in Python)"""
    _, cam, win = seq.view(step, *LENS_SIZE, spp=1)
    if step.v["mode"] == "ortho":
        cam = cam.copy()
        cam["projection"] = 1
    return cam, win, brt.lens(*step.v["lens"])


def lens_rays(cam, win, lens, pixels):
    w, h = LENS_SIZE
    rays = np.zeros(len(pixels), brt.RADIANCE_RAY_DTYPE)
    for i, p in enumerate(pixels):
        px, py = int(p) % w, int(p) // w
        o, d, state = brt.lens_ray(cam, win, lens, w, h, px, py, brt.lens_seed(win, w, h, px, py))
        rays[i]["origin"], rays[i]["direction"], rays[i]["seed"], rays[i]["user"] = o, d, state, p
    return rays


def expect(seq, step, reach, bound, oracle):
    """What a Layer A step returns on the callee's tree of `reach`, whose origins reach to `bound` -> a dict of arrays (and "counters" /
    "hits" where the family reports counts).  From the CPU references alone."""
    fam, v, inp = step.family, step.v, step.inp
    b = seq.buffers(step, twin(step.models, reach))
    out = {}
    if fam == "frame":
        lvl, cam, win = seq.view(step, level=v["level"])
        blend = v["level"] in (1, 2)
        frame, cnt = oracle.render(b, lvl, cam, win, seq.w, seq.h, raster_rgba=seq.raster if blend else None,
                                   raster_depth=seq.depth if blend else None)
        out["frame"] = frame if v["format"] == "f32" else oracle.encode_frame(frame, v["format"])
        out["counters"] = cnt
    elif fam == "pixels":
        lvl, cam, win = seq.view(step)
        frame, _ = oracle.render(b, lvl, cam, win, seq.w, seq.h)
        out["pixels"] = frame.reshape(-1, 4)[inp["pixels"]]
    elif fam == "lens":
        cam, win, lens = lens_of(seq, step)
        w, h = LENS_SIZE
        pixels = np.arange(w * h) if v["call"] == "render_lens" else inp["pixels"]
        res, _ = oracle.radiance(b, lens_rays(cam, win, lens, pixels), 1, BOUNCES)
        out["pixels"] = np.concatenate([res["rgb"], np.ones((len(pixels), 1), F32)], axis=1)
        # ... and the restated lens pixel (lens_ref.pixel over the restated shader) on a few of them
        c = cam[0].copy()
        sh = rr.shader(b.models, b.materials, b.bvh, c, BOUNCES)
        spot = [int(k) for k in inp["spot"]]
        out["spot"] = spot
        out["spot_pixels"] = np.array([lens_ref.pixel(sh, cam, win, lens, w, h, int(pixels[k]) % w, int(pixels[k]) // w) for k in spot], F32)
    elif fam == "query":
        rays = inp["rays"]
        mode = brt.QUERY_CLOSEST if v["mode"] == "closest" else brt.QUERY_ANY
        far = l1(rays["origin"]) > F32(bound)
        want = np.zeros(len(rays), brt.HIT_DTYPE)
        want["t"], want["sphere"], want["material"], want["user"] = np.inf, brt.QUERY_NONE, brt.QUERY_NONE, rays["user"]
        want["status"] = brt.QUERY_STATUS_OUT_OF_REACH
        if (~far).any():
            want[~far] = qr.expected(oracle, b.models, b.bvh, rays[~far], mode)[0]
        out["hits"], out["walked"] = want, ~far
    elif fam == "radiance":
        out["results"], out["walked"] = radiance_expected(oracle, b, inp["rays"], v["samples"], BOUNCES, bound)
    elif fam in ("probes", "volume"):
        probes = inp["probes"] if fam == "probes" else vr.probes(inp["volume"])
        dirs = brt.probe_directions(v["n_dirs"])
        res, _ = radiance_expected(oracle, b, pr.make_rays(probes, dirs), 1, BAKE_BOUNCES, bound)
        out["records"] = pr.project(res, dirs, brt.PROBE_SH9 if v["basis"] == "sh9" else brt.PROBE_AMBIENT_CUBE)
        out["entries"] = res
        if fam == "volume":
            out["samples"] = vr.sample(inp["volume"], out["records"], inp["points"])
    elif fam == "envmap":
        size, n = 8, 6 * 8 * 8
        rays = rr.make_rays(np.broadcast_to(np.array(v["position"], F32), (n, 3)), er.directions(size).reshape(n, 3),
                            er.seeds(v["seed"], size), np.arange(n, dtype=np.uint32))
        res, _ = radiance_expected(oracle, b, rays, 1, BAKE_BOUNCES, bound)
        level0 = er.resolve(res["rgb"], res["status"])
        tables = [brt.envmap_taps(brt.ENVMAP_TAPS_GGX, er.level_roughness(k, v["levels"]), v["n_taps"]) for k in range(1, v["levels"])]
        chain = er.chain(level0.reshape(6, size, size, 4), v["levels"], tables)
        out["chain"] = chain.astype(np.float16) if v["format"] == "f16" else chain
        out["entries"] = res
    elif fam == "lightmap":
        pts = inp["points"]
        res, _ = radiance_expected(oracle, b, lm.make_rays(pts, brt.lightmap_directions(v["n_dirs"])), 1, BAKE_BOUNCES, bound)
        img, info = lm.resolve(res, pts.reshape(-1), v["n_dirs"])
        img = img.reshape(8, 16, 4)
        texels = lm.dilate(img, v["passes"], v["wrap_u"]) if v["passes"] else img
        out["texels"] = texels.astype(np.float16) if v["format"] == "f16" else texels
        out["info"] = info.reshape(8, 16)
        out["entries"] = res
    else:
        raise AssertionError(f"{fam} is not a Layer A family")
    return out


def non_trivial(seq, step, oracle):
    """The conditions on the reference-only inputs, with the oracle alone (the tree of reach 0; a reach beyond every origin): every list
    has hits and misses, every bake has texels or records of both kinds"""
    if step.family not in ("query", "radiance", "probes", "volume", "envmap", "lightmap"):
        return
    want = expect(seq, step, 0.0, np.inf, oracle)
    res = want["hits"] if step.family == "query" else want["results"] if step.family == "radiance" else want["entries"]
    hit = (res["status"] & brt.QUERY_STATUS_HIT) != 0
    traced = (res["status"] & REFUSED_BITS) == 0
    assert hit.any() and (traced & ~hit).any(), f"{seq.name} {step.describe()}: {int(hit.sum())} hits of {int(traced.sum())} entries"
    if step.family in ("probes", "volume"):
        h = want["records"]["hits"]
        assert (h > 0).any() and (h < step.v["n_dirs"]).any(), (seq.name, step.describe(), h)
    if step.family == "lightmap":
        info = want["info"]
        assert (info["status"] == brt.LIGHTMAP_STATUS_EMPTY).any() and (info["hits"] > 0).any() and (info["hits"] < step.v["n_dirs"]).any()
    if step.family == "envmap":
        a = want["chain"][:384, 3]
        assert (a > 0).any() and (a == 0).any(), (seq.name, step.describe())
