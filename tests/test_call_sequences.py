"""Every entry-point family driven in covering sequences over ONE context (tests/sequence_cases.py has the generator and the CPU model).

What a context carries from a call of one family into a call of another -- the shared staging buffers, the tables cached by key, the one
ordering event of the list families, the resident tree with its reach and its numbering, the per-view memory -- is tested here:
12 covering chunks (every ordered pair of the twelve families adjacent once) and 6 random sequences, each run twice:
  * stepwise: synchronise and compare after every step.  Layer A (plain frames, pixel lists, lens, ray and radiance lists, the four
    bakes and the volume sampler) against the CPU references on the CPU twin of the tree the context reports, bit for bit.  Layer B
    (post-processed, upscaled and adaptive frames) against a control context per family that sees the same uploads and the same reach
    requests but no call of another family, byte for byte;
  * in flight: device forms on the context's own stream or one of two caller streams, host forms in between, uploads in the middle,
    every device output in its own guarded buffer, ONE synchronisation at the end: the bytes of the stepwise run, guards intact.
Every comparison is bitwise or an exact count.  Entries beyond the tree's reach are expected outcomes: their refused records are part of
the expectation.  The CPU tests hold the generator to its conditions (pairs, variants, events, non-trivial inputs, determinism).

Lens steps trace one sample per pixel: their reference for every pixel is the host twin's ray under the C oracle's radiance, and
lens_ref.pixel (Python) states three pixels of each list.

Times on one MI355X (docs/experiments.md "Call sequences over one context"): the module whole (36 sequence runs, 39 CPU tests, the
sum-up) 5.5 s; a stepwise or in-flight test 0.06 .. 0.08 s (the first one about 0.4 s: it starts the runtime); generating the 18
sequences 1.6 s, once; the 18 stepwise runs 1.26 s together, 0.37 s of it (29 %) in the CPU model (42 % over 400 soak sequences).

Run the module whole: the last GPU test sums what the sequences reported (hot orders, rebuilds by a list call's origin_bound)."""
import functools
import time

import numpy as np
import pytest

import bevyray_amd as brt
import lightmap_ref as lm
import oracle_loader
import probe_ref as pr
import query_ref as qr
import radiance_ref as rr
import sequence_cases as sc
import volume_ref as vr
from helpers import dev, guarded

SPECS = sc.specs()
NAMES = [s[0] for s in SPECS]
COUNTER_KEYS = ("rays", "node_pops", "interior_visits", "sphere_tests", "hits")
GUARD, FILL = 256, 0xCD
MODEL_SECONDS = [0.0]  # wall time spent in the CPU model (sequence_cases.expect) so far
REPORTS = {}          # sequence name -> what its stepwise run reported (the last GPU test sums them)


@functools.lru_cache(maxsize=None)
def _sequence(name):
    return sc.generate(SPECS[NAMES.index(name)], oracle_loader.load())


# ---- CPU: the generator's conditions ----------------------------------------------------------------------------------------------

def test_the_covering_chunks_hold_every_ordered_pair_once():
    pairs = {}
    for name, kind, _, fams, _ in SPECS:
        if kind == "covering":
            assert len(fams) == sc.CHUNK_STEPS
            for a, b in zip(fams, fams[1:]):
                pairs[a, b] = pairs.get((a, b), 0) + 1
    assert len(pairs) == 144 and set(pairs.values()) == {1}
    assert sum(1 for s in SPECS if s[1] == "covering") == 12 and sum(1 for s in SPECS if s[1] == "random") == 6
    assert all(len(s[3]) == sc.RANDOM_STEPS for s in SPECS if s[1] == "random")


VARIANTS = {
    "frame": {"call": ("run", "render_device"), "level": (1, 2, 3), "format": ("f32", "f16", "unorm8", "srgb8"), "counters": (True, False)},
    "post": {"flags": ("denoise", "temporal", "denoise+temporal")},
    "upscaled": {"call": ("plain", "refined", "blend"), "pair": sc.UPSCALE_PAIRS, "level": (1, 2, 3)},
    "pixels": {"call": ("host", "device"), "form": (1, 2)},
    "lens": {"call": ("render_lens", "render_lens_pixels", "render_lens_pixels_device"), "mode": ("thin", "ortho")},
    "query": {"call": ("host", "device"), "mode": ("closest", "occlusion")},
    "radiance": {"call": ("host", "device"), "form": (1, 2)},
    "probes": {"call": ("host", "device"), "basis": ("sh9", "cube"), "n_dirs": (16, 64)},
    "volume": {"bake": ("host", "device"), "sample": ("host", "device"), "basis": ("sh9", "cube"), "n_dirs": (16, 64)},
    "envmap": {"call": ("host", "device"), "levels": (3, 4), "format": ("f32", "f16"), "chunk_rays": (0, 128)},
    "lightmap": {"call": ("host", "device"), "n_dirs": (16, 64), "passes": (0, 2), "wrap_u": (True, False), "format": ("f32", "f16")},
}


def test_every_variant_and_every_event_is_drawn():
    seen, events, size, spp, tiles = {}, {}, {}, {}, 0
    for name in NAMES:
        seq = _sequence(name)
        size[seq.w, seq.h] = size.get((seq.w, seq.h), 0) + 1
        spp[seq.spp] = spp.get(seq.spp, 0) + 1
        tiles += seq.tile > 0
        assert 70 <= len(seq.steps[0].models) <= 600
        for s in seq.steps:
            events[s.event] = events.get(s.event, 0) + 1
            for k, val in s.v.items():
                seen[s.family, k, val] = seen.get((s.family, k, val), 0) + 1
            if s.family in ("query", "radiance"):
                key = (s.family, "origin_bound", s.v["origin_bound"] > 0)
                seen[key] = seen.get(key, 0) + 1
            seen[s.family, "stream", s.stream] = seen.get((s.family, "stream", s.stream), 0) + 1
    for fam, table in VARIANTS.items():
        for k, values in table.items():
            for val in values:
                assert seen.get((fam, k, val), 0) >= 2, (fam, k, val, seen.get((fam, k, val), 0))
    for fam in ("query", "radiance"):
        assert seen.get((fam, "origin_bound", True), 0) >= 2 and seen.get((fam, "origin_bound", False), 0) >= 2
    for e in sc.EVENTS:
        assert events.get(e, 0) >= 5, (e, events)
    assert min(size.get(k, 0) for k in ((61, 35), (64, 36))) >= 2 and min(spp.get(k, 0) for k in (32, 8)) >= 2, (size, spp)
    assert 6 <= tiles <= 12                                              # about half the sequences force a small LDS tile
    raises = sum(1 for n in NAMES for s in _sequence(n).steps if s.family in ("query", "radiance") and s.v["origin_bound"] > 0)
    assert raises >= 4


def test_the_context_frame_and_the_selection_list_are_reused_across_families(oracle):
    """Two reuses of the buffers the frame-level calls share (brt_frame.h context_frame, refine_list): the context's frame grows between
    an upscaled and an adaptive call on a caller's stream -- no drawn sequence has that, so one fixed sequence adds it -- and a refined
    call follows an adaptive one."""
    drawn = [_sequence(n) for n in NAMES]
    fixed = sc.fixed_frame_grows(oracle)
    assert not any(sc.frame_grows_on_a_caller_stream(q) for q in drawn)      # (if a drawn one gains it, the fixed one can go)
    assert sc.frame_grows_on_a_caller_stream(fixed) == [1]
    assert sum(1 for q in drawn if sc.refined_follows_adaptive(q)) >= 1 and sc.refined_follows_adaptive(fixed) == [2]
    assert sc.description(fixed) == sc.description(sc.fixed_frame_grows(oracle))
    assert [(s.family, s.stream, s.event) for s in fixed.steps] == [("upscaled", "s1", None), ("adaptive", "s2", None), ("upscaled", "s1", None)]


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_only_inputs_are_non_trivial(oracle, name):
    seq = _sequence(name)
    for s in seq.steps:
        sc.non_trivial(seq, s, oracle)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@pytest.mark.parametrize("name", NAMES)
def test_the_model_is_deterministic(oracle, name):
    spec = SPECS[NAMES.index(name)]
    a, b = sc.generate(spec, oracle), sc.generate(spec, oracle)
    assert sc.description(a) == sc.description(b) == sc.description(_sequence(name))
    n = 0
    for sa, sb in zip(a.steps, b.steps):
        if sa.family in sc.LAYER_A:
            assert _same(sc.expect(a, sa, 0.0, np.inf, oracle), sc.expect(b, sb, 0.0, np.inf, oracle)), sa.describe()
            n += 1
    assert n == sum(1 for s in a.steps if s.family in sc.LAYER_A)


def test_every_description_is_reproducible(oracle):
    for spec in SPECS:
        assert sc.description(sc.generate(spec, oracle)) == sc.description(_sequence(spec[0])), spec[0]


# ---- GPU: one call of a step ------------------------------------------------------------------------------------------------------

class _Out:
    """A device output in its own guarded buffer"""

    def __init__(self, n_bytes, dtype, shape=None):
        self.n, self.dtype, self.shape = n_bytes, dtype, shape
        self.buf = guarded(n_bytes, GUARD, FILL)
        self.ptr = self.buf.data_ptr()

    def read(self, what):
        raw = self.buf.cpu().numpy()
        assert (raw[self.n:] == FILL).all(), f"{what}: the guard behind a device output was written"
        a = raw[:self.n].copy().view(self.dtype)
        return a if self.shape is None else a.reshape(self.shape)


def _flags_of(v):
    return {"denoise": brt.FLAG_DENOISE, "temporal": brt.FLAG_TEMPORAL, "denoise+temporal": brt.FLAG_DENOISE | brt.FLAG_TEMPORAL}[v["flags"]]


def _frame_dtype(fmt):
    return {"f32": np.float32, "f16": np.uint16, "unorm8": np.uint8, "srgb8": np.uint8}[fmt]


class _Call:
    """One step on one context: prepare() makes its device buffers (before anything is in flight), launch(stream) makes the call(s),
    collect() reads the outputs after a synchronisation -> {name: array}.  stats: what the synchronous forms reported."""

    def __init__(self, p, seq, step):
        self.p, self.seq, self.step = p, seq, step
        self.dev, self.out, self.host, self.stats, self.refused = {}, {}, {}, None, None

    def prepare(self):
        seq, s, v, inp = self.seq, self.step, self.step.v, self.step.inp
        fam = s.family
        if fam == "frame":
            if v["level"] in (1, 2) and v["call"] == "render_device":
                self.dev["raster"], self.dev["depth"] = dev(seq.raster), dev(seq.depth)
            if v["call"] == "render_device":
                self.out["frame"] = _Out(seq.w * seq.h * brt.OUT_PIXEL_BYTES[sc.FORMATS[v["format"]]], _frame_dtype(v["format"]), (seq.h, seq.w, 4))
        elif fam == "post":
            self.out["frame"] = _Out(seq.w * seq.h * 16, np.float32, (seq.h, seq.w, 4))
        elif fam == "upscaled":
            w, h = v["pair"][:2]
            self.out["frame"] = _Out(w * h * 16, np.float32, (h, w, 4))
            if v["call"] == "refined":
                self.out["count"] = _Out(4, np.uint32)
            if v["call"] == "blend":
                self.dev["raster"], self.dev["depth"] = dev(inp["raster"]), dev(inp["depth"])
        elif fam == "adaptive":
            w, h = sc.ADAPTIVE_SIZE
            self.out["frame"], self.out["count"] = _Out(w * h * 16, np.float32, (h, w, 4)), _Out(4, np.uint32)
        elif fam in ("pixels", "lens"):
            if v["call"].endswith("device"):
                self.dev["pixels"] = dev(inp["pixels"])
                self.out["pixels"] = _Out(len(inp["pixels"]) * 16, np.float32, (len(inp["pixels"]), 4))
        elif fam in ("query", "radiance"):
            if v["call"] == "device":
                self.dev["rays"] = dev(inp["rays"])
                self.out["hits" if fam == "query" else "results"] = _Out(len(inp["rays"]) * 32, brt.HIT_DTYPE if fam == "query" else brt.RADIANCE_DTYPE)
        elif fam == "probes":
            if v["call"] == "device":
                self.dev["probes"] = dev(inp["probes"])
                self.out["records"] = _Out(8 * 128, brt.PROBE_RECORD_DTYPE)
        elif fam == "volume":
            if v["bake"] == "device":
                self.out["records"] = _Out(8 * 128, brt.PROBE_RECORD_DTYPE)
            if v["sample"] == "device":
                self.dev["points"] = dev(inp["points"])
                self.dev["records_in"] = dev(np.zeros(8, brt.PROBE_RECORD_DTYPE))       # (where a host bake's records go for the sampler)
                self.out["samples"] = _Out(100 * 16, brt.VOLUME_SAMPLE_DTYPE)
        elif fam == "envmap":
            if v["call"] == "device":
                n = brt.envmap_level_offsets(8, v["levels"])[-1]
                self.out["chain"] = _Out(n * (8 if v["format"] == "f16" else 16), np.float16 if v["format"] == "f16" else np.float32, (n, 4))
        elif fam == "lightmap":
            if v["call"] == "device":
                self.dev["points"] = dev(inp["points"])
                self.out["texels"] = _Out(128 * (8 if v["format"] == "f16" else 16), np.float16 if v["format"] == "f16" else np.float32, (8, 16, 4))
                self.out["info"] = _Out(128 * 8, brt.LIGHTMAP_INFO_DTYPE, (8, 16))

    def launch(self, stream):
        """stream: None (the context's own stream: synchronous) or a torch stream of the caller's.  A call the context refuses as a
        whole leaves its code in `refused` (the stepwise run says which refusals the model expects)."""
        try:
            self._launch(stream)
        except brt.BrtError as e:
            self.refused = e.code

    def _launch(self, stream):
        import torch
        node, seq, s, v, inp = self.p.node, self.seq, self.step, self.step.v, self.step.inp
        fam = s.family
        sh = None if stream is None else stream.cuda_stream
        ptr = lambda k: self.dev[k].data_ptr()                              # noqa: E731
        if fam == "frame":
            lvl, cam, win = seq.view(s, level=v["level"])
            blend = v["level"] in (1, 2)
            flags = brt.FLAG_COUNTERS if v["counters"] else 0
            if v["call"] == "run":
                self.host["frame"] = node.run(lvl, cam, win, seq.w, seq.h, raster_rgba=seq.raster if blend else None,
                                              raster_depth=seq.depth if blend else None, flags=flags)
                self.stats = dict(node.last_stats)
            else:
                st = node.render_device(lvl, cam, win, seq.w, seq.h, self.out["frame"].ptr, ptr("raster") if blend else 0,
                                        ptr("depth") if blend else 0, stream=sh, flags=flags | sc.FORMATS[v["format"]])
                self.stats = dict(st) if sh is None else None
        elif fam == "post":
            lvl, cam, win = seq.view(s)
            st = node.render_device(lvl, cam, win, seq.w, seq.h, self.out["frame"].ptr, stream=sh, flags=_flags_of(v))
            self.stats = dict(st) if sh is None else None
        elif fam == "upscaled":
            w, h, lw, lh = v["pair"]
            lvl, cam, win = seq.view(s, w, h, level=v["level"])
            if v["call"] == "plain":
                st = node.render_upscaled_device(cam, win, lw, lh, w, h, self.out["frame"].ptr, stream=sh)
            elif v["call"] == "refined":
                st = node.render_upscaled_refined_device(cam, win, lw, lh, w, h, self.out["frame"].ptr, d_refined_count=self.out["count"].ptr, stream=sh)
            else:
                st = node.render_upscaled_blend_device(lvl, cam, win, lw, lh, w, h, self.out["frame"].ptr, ptr("raster"), ptr("depth"), stream=sh)
            self.stats = dict(st) if sh is None else None
        elif fam == "adaptive":
            w, h = sc.ADAPTIVE_SIZE
            _, cam, win = seq.view(s, w, h)
            st = node.render_adaptive_device(cam, win, w, h, self.out["frame"].ptr, self.out["count"].ptr, stream=sh)
            self.stats = dict(st) if sh is None else None
        elif fam == "pixels":
            _, cam, win = seq.view(s)
            with self.p.tuning(BRT_PIXELS_FORM=v["form"]):
                if v["call"] == "host":
                    self.host["pixels"] = node.render_pixels(cam, win, seq.w, seq.h, inp["pixels"])
                    self.stats = dict(node.last_stats)
                else:
                    st = node.render_pixels_device(cam, win, seq.w, seq.h, ptr("pixels"), len(inp["pixels"]), self.out["pixels"].ptr, stream=sh)
                    self.stats = dict(st) if sh is None else None
        elif fam == "lens":
            cam, win, lens = sc.lens_of(seq, s)
            w, h = sc.LENS_SIZE
            if v["call"] == "render_lens":
                self.host["pixels"] = node.render_lens(cam, win, lens, w, h).reshape(-1, 4)
                self.stats = dict(node.last_stats)
            elif v["call"] == "render_lens_pixels":
                self.host["pixels"] = node.render_lens_pixels(cam, win, lens, w, h, inp["pixels"])
                self.stats = dict(node.last_stats)
            else:
                st = node.render_lens_pixels_device(cam, win, lens, w, h, ptr("pixels"), len(inp["pixels"]), self.out["pixels"].ptr, stream=sh)
                self.stats = dict(st) if sh is None else None
        elif fam == "query":
            mode = brt.QUERY_CLOSEST if v["mode"] == "closest" else brt.QUERY_ANY
            if v["call"] == "host":
                self.host["hits"] = node.query_rays(inp["rays"], mode, v["origin_bound"])
                self.stats = dict(node.last_query_stats)
            else:
                st = node.query_rays_device(ptr("rays"), len(inp["rays"]), self.out["hits"].ptr, mode, v["origin_bound"], stream=sh)
                self.stats = dict(st) if sh is None else None
        elif fam == "radiance":
            with self.p.tuning(BRT_RADIANCE_FORM=v["form"]):
                if v["call"] == "host":
                    self.host["results"] = node.radiance_rays(inp["rays"], v["samples"], sc.BOUNCES, v["origin_bound"])
                    self.stats = dict(node.last_radiance_stats)
                else:
                    st = node.radiance_rays((ptr("rays"), len(inp["rays"]), self.out["results"].ptr), v["samples"], sc.BOUNCES, v["origin_bound"],
                                            device=True, stream=sh)
                    self.stats = dict(st) if sh is None else None
        elif fam == "probes":
            basis = brt.PROBE_SH9 if v["basis"] == "sh9" else brt.PROBE_AMBIENT_CUBE
            if v["call"] == "host":
                self.host["records"] = node.bake_probes(inp["probes"], v["n_dirs"], sc.BAKE_BOUNCES, basis)
                self.stats = dict(node.last_probe_stats)
            else:
                st = node.bake_probes((ptr("probes"), 8, self.out["records"].ptr), v["n_dirs"], sc.BAKE_BOUNCES, basis, device=True, stream=sh)
                self.stats = dict(st) if sh is None else None
        elif fam == "volume":
            vol = inp["volume"]
            if v["bake"] == "host":
                records = self.host["records"] = node.bake_volume(vol, v["n_dirs"], sc.BAKE_BOUNCES)
                self.stats = dict(node.last_probe_stats)
            else:
                st = node.bake_volume(vol, v["n_dirs"], sc.BAKE_BOUNCES, d_records=self.out["records"].ptr, stream=sh)
                self.stats = dict(st) if sh is None else None
                records = None
            if v["sample"] == "host":
                if records is None:                                        # the host sampler reads the records: this caller waits for its own bake
                    (torch.cuda.current_stream() if stream is None else stream).synchronize()
                    records = self.out["records"].buf.cpu().numpy()[:8 * 128].view(brt.PROBE_RECORD_DTYPE)
                self.host["samples"] = node.sample_volume(vol, records, inp["points"])
            else:
                d_records = self.out["records"].ptr if records is None else ptr("records_in")
                if records is not None:
                    self.dev["records_in"].copy_(torch.from_numpy(records.view(np.uint8).reshape(-1)))
                    torch.cuda.current_stream().synchronize()
                node.sample_volume(vol, d_records, (ptr("points"), 100, self.out["samples"].ptr), device=True, stream=sh)
        elif fam == "envmap":
            knobs = {"BRT_PROBE_CHUNK_RAYS": v["chunk_rays"]} if v["chunk_rays"] else {}
            fmt = sc.FORMATS[v["format"]]
            with self.p.tuning(**knobs):
                if v["call"] == "host":
                    self.host["chain"] = node.bake_envmap(v["position"], 8, v["levels"], 1, sc.BAKE_BOUNCES, v["n_taps"], v["seed"], out_format=fmt)
                    self.stats = dict(node.last_probe_stats)
                else:
                    st = node.bake_envmap(v["position"], 8, v["levels"], 1, sc.BAKE_BOUNCES, v["n_taps"], v["seed"], d_out=self.out["chain"].ptr,
                                          stream=sh, out_format=fmt)
                    self.stats = dict(st) if sh is None else None
        elif fam == "lightmap":
            fmt = sc.FORMATS[v["format"]]
            if v["call"] == "host":
                self.host["texels"], self.host["info"] = node.bake_lightmap(inp["points"], v["n_dirs"], sc.BAKE_BOUNCES, v["passes"], v["wrap_u"],
                                                                            out_format=fmt)
                self.stats = dict(node.last_probe_stats)
            else:
                st = node.bake_lightmap((ptr("points"), 16, 8, self.out["texels"].ptr, self.out["info"].ptr), v["n_dirs"], sc.BAKE_BOUNCES,
                                        v["passes"], v["wrap_u"], device=True, stream=sh, out_format=fmt)
                self.stats = dict(st) if sh is None else None

    def collect(self):
        got = dict(self.host)
        if self.refused is not None:
            got["refused"] = self.refused
        for k, o in self.out.items():
            got[k] = o.read(f"{self.seq.name} {self.step.describe()} output {k}")
        return got


def _reach_request(p, seq, step):
    """What a control context sees of a step of ANOTHER family: the request that step makes of the resident tree's reach, and nothing
    else of it.  A camera-driven step asks through its camera (a one-pixel list under the same camera, and for a lens step the same lens:
    the rule looks at the camera and the lens, not at the size); a list call with an origin_bound asks through a one-ray query with that
    origin_bound.  The bakes of a sequence ask for nothing."""
    one = np.zeros(1, np.uint32)
    if step.family == "lens":
        cam, win, lens = sc.lens_of(seq, step)
        p.node.render_lens_pixels(cam, win, lens, *sc.LENS_SIZE, one)
    elif step.family in sc.CAMERA_FAMILIES:
        size = step.v["pair"][:2] if step.family == "upscaled" else sc.ADAPTIVE_SIZE if step.family == "adaptive" else (seq.w, seq.h)
        _, cam, win = seq.view(step, *size)
        p.node.render_pixels(cam, win, *size, one)
    elif step.family in ("query", "radiance") and step.v["origin_bound"] > 0:
        p.node.query_rays(step.inp["rays"][:1], origin_bound=step.v["origin_bound"])


def _context(seq):
    p = brt.RaytracePlugin([0])
    p.set_tuning("BRT_FORCE_LDS_TOP", seq.tile if seq.tile else 100000)
    p.set_denoise()
    p.set_temporal()
    p.set_adaptive()
    return p


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"


def _ids(what, check):
    """check_spheres of a list family, its failure named: a hit's `sphere` is the caller's index of a sphere that gives the hit's t and
    material (the resident numbering mapped back)"""
    try:
        check()
    except AssertionError as e:
        raise AssertionError(f"{what}: a hit's sphere id is not in the caller's numbering (entry {e})") from e


def _compare_layer_a(seq, step, got, st, reach, bound, oracle, what):
    """A Layer A step against the CPU model; st: the call's stats (every step of a stepwise run has them)"""
    fam, v, inp = step.family, step.v, step.inp
    t0 = time.perf_counter()
    want = sc.expect(seq, step, reach, bound, oracle)
    MODEL_SECONDS[0] += time.perf_counter() - t0
    if fam == "frame":
        _bits_equal(got["frame"], want["frame"], what)
        assert st["rays"] == want["counters"]["rays"], (what, st["rays"], want["counters"])
        if v["counters"]:
            assert {k: st[k] for k in COUNTER_KEYS} == want["counters"], (what, st, want["counters"])
    elif fam == "pixels":
        _bits_equal(got["pixels"], want["pixels"], what)
        assert st["reserved"] == 0 and st["paths"] == 300 * seq.spp, (what, st)
    elif fam == "lens":
        _bits_equal(got["pixels"], want["pixels"], what)
        _bits_equal(got["pixels"][want["spot"]], want["spot_pixels"], what + ", the restated lens pixel")
    elif fam == "query":
        qr.assert_hits_equal(got["hits"], want["hits"], what)
        walked = want["walked"]
        assert (got["hits"]["sphere"][~walked] == brt.QUERY_NONE).all(), what
        _ids(what, lambda: qr.check_spheres(oracle, step.models, inp["rays"][walked], got["hits"][walked]))
        assert st["refused"] == int((~walked).sum()) and st["rays_walked"] == int(walked.sum()), (what, st)
    elif fam == "radiance":
        rr.assert_equal(got["results"], want["results"], what)
        walked = want["walked"]
        assert (got["results"]["sphere"][~walked] == brt.QUERY_NONE).all(), what
        _ids(what, lambda: rr.check_spheres(step.models, inp["rays"][walked], got["results"][walked]))
        hit = (want["results"]["status"] & brt.QUERY_STATUS_HIT) != 0
        assert (st["refused"], st["hits"], st["form"]) == (int((~walked).sum()), int(hit.sum()), v["form"] - 1), (what, st)
    elif fam in ("probes", "volume"):
        pr.assert_records_equal(got["records"], want["records"], what)
        if fam == "volume":
            vr.assert_samples_equal(got["samples"], want["samples"], what + ", samples")
    elif fam == "envmap":
        lm.assert_texels_equal(got["chain"], want["chain"], what)
        if v["chunk_rays"]:
            assert st["chunks"] == 3, (what, st)
    elif fam == "lightmap":
        lm.assert_texels_equal(got["texels"], want["texels"], what)
        assert got["info"].tobytes() == want["info"].tobytes(), what
    if fam in ("probes", "volume", "envmap", "lightmap"):
        res = want["entries"]
        refused = (res["status"] & sc.REFUSED_BITS) != 0
        hit = (res["status"] & brt.QUERY_STATUS_HIT) != 0
        assert (st["refused"], st["hits"]) == (int(refused.sum()), int(hit.sum())), (what, st)
        return int(refused.sum())
    return 0


def _run_stepwise(seq, oracle):
    """-> (the outputs of every step, the report).  Compares every step."""
    import torch
    t_start, model_start = time.perf_counter(), MODEL_SECONDS[0]
    mixed = _context(seq)
    controls = {f: _context(seq) for f in sc.LAYER_B if any(s.family == f for s in seq.steps)}
    everyone = [mixed] + list(controls.values())
    report = dict(hot=False, bound_rebuilds=0, compared=0, rebuilds=0, refused_calls=0, refused_entries=0)
    outputs = []
    try:
        calls = [_Call(mixed, seq, s) for s in seq.steps]
        twins = {s.index: _Call(controls[s.family], seq, s) for s in seq.steps if s.family in controls}
        for c in calls + list(twins.values()):
            c.prepare()
        torch.cuda.synchronize()
        prev = None
        for s, call in zip(seq.steps, calls):
            what = f"{seq.name} (seed {seq.seed}) {s.describe()} after {prev}"
            if s.upload is not None:
                for p in everyone:
                    p.node.write_buffers(brt.Buffers(s.upload, seq.materials, None))
            call.launch(None)
            torch.cuda.synchronize()
            got, st = call.collect(), call.stats
            if s.family == "envmap" and sc.l1(s.v["position"])[0] > np.float32(mixed.node.query_origin_bound()):
                # a cube beyond the tree's bound is refused whole (brt_api_envmap.cpp position_reach_check): the code, and nothing written
                assert got.get("refused") == -1 and not call.host, (what, got.keys())
                assert all((o.buf.cpu().numpy() == FILL).all() for o in call.out.values()), what
                report["compared"] += 1
                report["refused_calls"] += 1
                outputs.append(got)
                prev = f"{s.family} {s.v} (refused)"
                for f, p in controls.items():
                    _reach_request(p, seq, s)
                continue
            assert call.refused is None and st is not None, (what, call.refused)
            reach, bound = st["tree_reach"], mixed.node.query_origin_bound()
            report["rebuilds"] += st["tree_rebuilt"]
            report["hot"] |= st.get("hot_records", 0) > 0
            if s.family in ("frame", "pixels"):                           # as the soak: the reported reach covers what this camera needs
                need = sc.needed_reach(seq, s)
                assert reach >= need or sc.twin(s.models, reach).tobytes() == sc.twin(s.models, need).tobytes(), (what, reach, need)
            if s.family in ("query", "radiance") and s.v["origin_bound"] > 0:
                assert bound >= s.v["origin_bound"], (what, bound)
                report["bound_rebuilds"] += st["tree_rebuilt"]
            if s.family in sc.LAYER_A:
                report["refused_entries"] += _compare_layer_a(seq, s, got, st, reach, bound, oracle, what)
            else:
                twin = twins[s.index]
                twin.launch(None)
                torch.cuda.synchronize()
                want = twin.collect()
                assert twin.stats["tree_reach"] == reach, (what, "the control's tree has another reach", twin.stats["tree_reach"], reach)
                assert got.keys() == want.keys()
                for k in got:
                    _bits_equal(got[k], want[k], f"{what}: {k} against the control context")
                assert twin.stats["rays"] == st["rays"] and twin.stats["paths"] == st["paths"], (what, st, twin.stats)
            for f, p in controls.items():
                if f != s.family:
                    _reach_request(p, seq, s)
            report["compared"] += 1
            outputs.append(got)
            prev = f"{s.family} {s.v}"
    finally:
        torch.cuda.synchronize()
        for p in everyone:
            p.close()
    assert report["compared"] == len(seq.steps)
    report["seconds"], report["model_seconds"] = round(time.perf_counter() - t_start, 3), round(MODEL_SECONDS[0] - model_start, 3)
    return outputs, report


@functools.lru_cache(maxsize=None)
def _stepwise(name):
    outputs, report = _run_stepwise(_sequence(name), oracle_loader.load())
    REPORTS[name] = report
    return outputs


def _run_in_flight(seq):
    """Every step enqueued on its drawn stream (host forms and uploads in between), ONE synchronisation at the end -> the outputs"""
    import torch
    p = _context(seq)
    try:
        streams = {"own": None, "s1": torch.cuda.Stream(), "s2": torch.cuda.Stream()}
        calls = [_Call(p, seq, s) for s in seq.steps]
        for c in calls:
            c.prepare()
        torch.cuda.synchronize()
        for s, call in zip(seq.steps, calls):
            if s.upload is not None:
                p.node.write_buffers(brt.Buffers(s.upload, seq.materials, None))
            call.launch(streams[s.stream])
        torch.cuda.synchronize()
        return [c.collect() for c in calls]
    finally:
        torch.cuda.synchronize()
        p.close()


# ---- GPU: the sequences -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_stepwise(oracle, name):
    outputs = _stepwise(name)
    print(name, REPORTS[name])
    assert len(outputs) == len(_sequence(name).steps) and REPORTS[name]["compared"] == len(outputs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_in_flight(oracle, name):
    seq = _sequence(name)
    want = _stepwise(name)
    _compare_in_flight(seq, want)


def _compare_in_flight(seq, want):
    got = _run_in_flight(seq)
    compared = 0
    for s, g, w in zip(seq.steps, got, want):
        assert g.keys() == w.keys(), s.describe()
        for k in g:
            _bits_equal(g[k], w[k], f"{seq.name} (seed {seq.seed}) in flight, {s.describe()}: {k} against the stepwise run")
        compared += 1
    assert compared == len(seq.steps)


@pytest.mark.gpu
def test_the_fixed_sequence_stepwise_and_in_flight(oracle):
    """sequence_cases.fixed_frame_grows: every step bit for bit against its control context, then in flight against the stepwise run"""
    seq = sc.fixed_frame_grows(oracle)
    want, report = _run_stepwise(seq, oracle)
    assert report["compared"] == len(want) == 3
    _compare_in_flight(seq, want)


@pytest.mark.gpu
def test_what_the_sequences_reported():
    """Over all sequences: at least a third renumbered the tree's records by use on some frame, and at least four trees were rebuilt for
    a list call's origin_bound."""
    assert sorted(REPORTS) == sorted(NAMES), "run the module whole: this test sums what every stepwise run reported"
    hot = sum(1 for r in REPORTS.values() if r["hot"])
    rebuilt = sum(r["bound_rebuilds"] for r in REPORTS.values())
    print(f"{hot} of {len(REPORTS)} sequences with hot records; {rebuilt} rebuilds by a list call's origin_bound; "
          f"{sum(r['rebuilds'] for r in REPORTS.values())} rebuilds in all; {sum(r['refused_calls'] for r in REPORTS.values())} bakes refused "
          f"whole, {sum(r['refused_entries'] for r in REPORTS.values())} bake entries refused; stepwise runs {sum(r['seconds'] for r in REPORTS.values()):.2f} s "
          f"in all, {sum(r['model_seconds'] for r in REPORTS.values()):.2f} s of them in the CPU model")
    assert 3 * hot >= len(REPORTS), (hot, REPORTS)
    assert rebuilt >= 4, rebuilt
