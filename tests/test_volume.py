"""Irradiance volumes (brt_bake_volume*, brt_sample_volume*, brt_volume_probes_device, brt_host_volume_*; DESIGN.md "Irradiance volumes").
CPU: the exports, the lattice against the restatement (tests/volume_ref.py), every descriptor refusal, the host twin bitwise against the
restatement on synthetic records and points of every category, the same-records identity, the tie to brt_host_probe_irradiance.  GPU:
both kernels bitwise against the host exports and the restatement; the bake against brt_bake_probes_device over the lattice's probes on
both trees; a G-buffer-like list end to end; an empty sky against the analytic irradiance; streams, uploads, frames and refusals."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import probe_ref as pr
import volume_ref as vr
from bevyray_amd import _lib
from helpers import cover as _cover, dev as _dev, guarded as _guarded, make_buffers, upload_cover as _upload_cover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_host_volume_probes", "brt_host_volume_sample", "brt_volume_probes_device", "brt_bake_volume_device", "brt_bake_volume",
           "brt_sample_volume_device", "brt_sample_volume")
F32 = np.float32
SH9, CUBE, WRAP = brt.PROBE_SH9, brt.PROBE_AMBIENT_CUBE, brt.VOLUME_WRAP
CLAMPED, BAD, NO_PROBE = brt.VOLUME_STATUS_CLAMPED, brt.VOLUME_STATUS_INVALID, brt.VOLUME_STATUS_NO_PROBE
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
LATTICES = [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2), (5, 4, 3), (3, 1, 7)]
ORIGIN, SPACING = (-1.5, 0.25, -2.0), (0.7, 1.3, 0.9)        # (0.7 * i - 1.5 rounds in f32: the multiply and the add are both seen)
KINDS = ("nan", "inf", "3e38", "denormal", "negzero", "status4", "status8", "basis", "plain")
# |f32 rule - float64 rule| relative to max(1, |E|): 4 x the largest seen (7.41e-7) over the random points of the 5x4x3 lattice with
# identical records, both bases, both flag values (test_the_f32_rule_against_float64 prints each; DESIGN.md section 20 records them)
SAME_TOLERANCE = 4 * 7.5e-7
HOST_EXPORT_TOLERANCE = 1e-5      # relative: what tests/test_probes.py asks of brt_host_probe_irradiance against probe_ref.irradiance64
SKY_E_BOUND = 2e-3                # |E(n) - analytic| of an N = 1024 sky record: section 19's bound in tests/test_probes.py


def _volume(count, basis=SH9, flags=0, origin=ORIGIN, spacing=SPACING, seed=0xFFFFFF00):
    return brt.make_volume(origin, spacing, count, basis, seed, flags)


def _points(position, normal):
    position = np.asarray(position, F32).reshape(-1, 3)
    pts = np.zeros(len(position), brt.VOLUME_POINT_DTYPE)
    pts["position"] = position
    pts["normal"] = np.broadcast_to(np.asarray(normal, F32), position.shape)
    pts["ignored0"], pts["ignored1"] = 0xDEADBEEF, 0x7FC00000       # (the ignored words are ignored)
    return pts


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F32)


def _variants(count):
    n = count[0] * count[1] * count[2]
    return 1 if n >= 18 else -(-len(KINDS) // n)


def _special(rec, kind, basis, rng):
    if kind == "nan":
        rec["coeff"][rng.integers(0, 18)] = np.nan
    elif kind == "inf":
        rec["coeff"][rng.integers(0, 18)] = np.inf if rng.random() < 0.5 else -np.inf
    elif kind == "3e38":
        rec["coeff"][:18] = rng.choice([F32(3e38), F32(-3e38)], size=18)
    elif kind == "denormal":
        rec["coeff"][:] = rng.uniform(-1e-40, 1e-40, size=27).astype(F32)
    elif kind == "negzero":
        rec["coeff"][:] = F32(-0.0)
    elif kind == "status4":
        rec["status"] = brt.QUERY_STATUS_INVALID
        rec["coeff"][:] = np.nan                                     # (a refused record's coefficients reach nothing)
    elif kind == "status8":
        rec["status"] = brt.QUERY_STATUS_OUT_OF_REACH
    elif kind == "basis":
        rec["basis"] = 1 - basis


@functools.lru_cache(maxsize=None)
def _records(count, basis, variant):
    """Synthetic records of a lattice: random coefficients in [-2, 4]; NaN, INF, 3e38, denormal and -0.0 coefficients, refused statuses
    and a wrong basis word on some.  Small lattices take the kinds in turn over `_variants(count)` variants; larger ones carry all at
    once, ten of their records refused."""
    n = count[0] * count[1] * count[2]
    rng = np.random.default_rng([51, n, basis, variant])
    rec = np.zeros(n, brt.PROBE_RECORD_DTYPE)
    rec["coeff"] = rng.uniform(-2, 4, size=(n, 27)).astype(F32)
    if basis == CUBE:
        rec["coeff"][:, 18:] = 0
    rec["hits"], rec["n_dirs"], rec["basis"] = rng.integers(0, 64, size=n), 64, basis
    if n >= 18:
        kinds = ["status4"] * 4 + ["status8"] * 3 + ["basis"] * 3 + ["nan", "inf", "3e38", "denormal", "negzero"]
        where = rng.permutation(n)[:len(kinds)]
    else:
        kinds = [KINDS[(i + variant * n) % len(KINDS)] for i in range(n)]
        where = np.arange(n)
    for i, kind in zip(where, kinds):
        _special(rec[i], kind, basis, rng)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def _fixture_points(count):
    """Points of every category for the lattice `count` at ORIGIN / SPACING."""
    vol = _volume(count)
    rng = np.random.default_rng([52, *count])
    o, s, c = np.array(ORIGIN), np.array(SPACING), np.array(count)
    nodes = vr.probes(vol)["position"]
    parts = [_points(nodes, _unit(rng, len(nodes)))]                                         # every node exactly (len2 == 0 under WRAP)
    for shift in ((.5, 0, 0), (0, .5, 0), (0, 0, .5), (.5, .5, 0), (.5, 0, .5), (0, .5, .5), (.5, .5, .5)):  # edge, face and cell midpoints
        mid = nodes.astype(np.float64) + np.array(shift) * s
        parts.append(_points(mid, _unit(rng, len(mid))))
    g = [o[a] + s[a] * np.arange(-2.0, c[a] + 1.01, 0.5) for a in range(3)]                  # up to two cells outside on every side
    grid = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3)
    parts.append(_points(grid, _unit(rng, len(grid))))
    parts.append(_points(nodes[-1:], (0.0, 1.0, 0.0)))                                        # the far corner exactly
    inside = o + s * (c - 1) * 0.37
    for a in range(3):
        for value in (3e38, -3e38, 1e-42, -1e-42, -0.0):                                      # huge, denormal and -0.0 components
            p = inside.copy()
            p[a] = value
            parts.append(_points(p, _unit(rng, 1)))
            nrm = _unit(rng, 1)
            nrm[0, a] = value
            parts.append(_points(inside, nrm))
        for value in (np.nan, np.inf, -np.inf):                                               # refused: each of the six components
            p = inside.copy()
            p[a] = value
            parts.append(_points(p, (0.0, 1.0, 0.0)))
            nrm = np.array([0.6, 0.0, 0.8])
            nrm[a] = value
            parts.append(_points(inside, nrm))
    few = rng.uniform(o - s, o + s * c, size=(64, 3))
    parts.append(_points(few, rng.uniform(-3, 3, size=(64, 3))))                              # non-unit normals
    parts.append(_points(few[:8], (0.0, 0.0, 0.0)))                                           # zero normals
    rand = rng.uniform(o - 1.5 * s, o + s * (c - 1 + 1.5), size=(20000, 3))
    parts.append(_points(rand, _unit(rng, 20000)))                                            # 20 000 uniform random points (the last 20 000)
    pts = np.concatenate(parts)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _want(count, basis, flags, variant):
    """The restatement's samples of a fixture and what it saw on the way: once per process."""
    detail = {}
    out = vr.sample(_volume(count, basis, flags), _records(count, basis, variant), _fixture_points(count), detail=detail)
    out.setflags(write=False)
    return out, detail


def _cases(count):
    return [(basis, flags, variant) for basis in (SH9, CUBE) for flags in (0, WRAP) for variant in range(_variants(count))]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in EXPORTS:
        assert f"int32_t {name}(" in header, name
        assert name in _lib.EXPORTS, name
        assert f"pub fn {name}(" in rust, name
        assert name in defined, name
    for record in ("pub struct brt_volume {", "pub struct brt_volume_point {", "pub struct brt_volume_sample {"):
        assert record in rust, record
    assert _lib.load().brt_abi_version() == 6
    assert (brt.VOLUME_DTYPE.itemsize, brt.VOLUME_POINT_DTYPE.itemsize, brt.VOLUME_SAMPLE_DTYPE.itemsize) == (48, 32, 16)
    assert [brt.VOLUME_DTYPE.fields[f][1] for f in ("origin", "seed", "spacing", "basis", "count", "flags")] == [0, 12, 16, 28, 32, 44]
    assert [brt.VOLUME_POINT_DTYPE.fields[f][1] for f in ("position", "normal")] == [0, 16]
    assert [brt.VOLUME_SAMPLE_DTYPE.fields[f][1] for f in ("rgb", "status")] == [0, 12]
    assert (WRAP, CLAMPED, BAD, NO_PROBE) == (1, 1, 4, 8)
    for text in ("#define BRT_VOLUME_WRAP 1u", "#define BRT_VOLUME_STATUS_CLAMPED 1u", "#define BRT_VOLUME_STATUS_INVALID 4u",
                 "#define BRT_VOLUME_STATUS_NO_PROBE 8u"):
        assert text in header, text


@pytest.mark.parametrize("count", LATTICES + [(1024, 1, 1), (64, 128, 128)])
def test_the_lattice_against_the_restatement(count):
    for seed in (0, 0xFFFFFF00, 0xFFFFFFFF):                       # (seed + i * 0x85EBCA6B wraps)
        vol = _volume(count, seed=seed)
        got, want = brt.volume_probes(vol), vr.probes(vol)
        assert got.tobytes() == want.tobytes(), (count, seed)
    n = count[0] * count[1] * count[2]
    if n > 1:
        assert want["seed"][1] == (0xFFFFFFFF + 0x85EBCA6B) % 2 ** 32 and want["seed"][-1] == (0xFFFFFFFF + (n - 1) * 0x85EBCA6B) % 2 ** 32
    if count[0] >= 5:                                              # the multiply-add rounds: the exact node differs from the f32 one
        exact = ORIGIN[0] + np.arange(count[0]) * float(F32(SPACING[0]))
        assert (want["position"][:count[0], 0].astype(np.float64) != exact).any()
        two_steps = (F32(ORIGIN[0]) + (np.arange(count[0]).astype(F32) * F32(SPACING[0])).astype(F32)).astype(F32)
        assert np.array_equal(want["position"][:count[0], 0], two_steps)


def test_every_descriptor_refusal():
    lib = _lib.load()
    good = _volume((2, 2, 2))
    out = np.zeros(8, brt.PROBE_DTYPE)
    recs = np.zeros(8, brt.PROBE_RECORD_DTYPE)
    pts = _points([(0, 0, 0)], (0, 1, 0))
    smp = np.full(1, 7, brt.VOLUME_SAMPLE_DTYPE)
    assert lib.brt_host_volume_probes(good.ctypes.data, out.ctypes.data) == 0
    assert lib.brt_host_volume_sample(good.ctypes.data, recs.ctypes.data, pts.ctypes.data, 1, smp.ctypes.data) == 0

    def bad(**change):
        v = good.copy()
        for k, (index, value) in change.items():
            if index is None:
                v[k] = value
            else:
                v[k][0, index] = value
        return v

    cases = {"count 0": bad(count=(1, 0)), "count 1025": bad(count=(2, 1025)), "product above 1 << 20": bad(count=(None, (1024, 1024, 2))),
             "product just above 1 << 20": bad(count=(None, (1024, 513, 2))),
             "spacing 0": bad(spacing=(0, 0.0)), "spacing negative": bad(spacing=(1, -1.0)), "spacing nan": bad(spacing=(2, np.nan)),
             "spacing inf": bad(spacing=(0, np.inf)), "origin nan": bad(origin=(1, np.nan)), "origin inf": bad(origin=(2, np.inf)),
             "origin -inf": bad(origin=(0, -np.inf)), "basis 2": bad(basis=(None, 2)), "flags 2": bad(flags=(None, 2)),
             "flags 3": bad(flags=(None, 3)), "flags high": bad(flags=(None, 0x80000001))}
    for what, v in cases.items():
        out[:] = 0
        smp[:] = 7
        assert lib.brt_host_volume_probes(v.ctypes.data, out.ctypes.data) == INVALID, what
        assert lib.brt_host_volume_sample(v.ctypes.data, recs.ctypes.data, pts.ctypes.data, 1, smp.ctypes.data) == INVALID, what
        assert b"volume" in lib.brt_last_error(None), what
        assert not out.view(np.uint8).any() and (smp["status"] == 7).all(), what
        with pytest.raises(brt.BrtError):
            brt.volume_probes(v)
    assert lib.brt_host_volume_probes(_volume((1024, 1024, 1)).ctypes.data, None) == INVALID      # (the largest lattice is valid; null out)
    assert lib.brt_host_volume_probes(None, out.ctypes.data) == INVALID
    g = good.ctypes.data
    assert lib.brt_host_volume_sample(None, recs.ctypes.data, pts.ctypes.data, 1, smp.ctypes.data) == INVALID
    assert lib.brt_host_volume_sample(g, None, pts.ctypes.data, 1, smp.ctypes.data) == INVALID
    assert lib.brt_host_volume_sample(g, recs.ctypes.data, None, 1, smp.ctypes.data) == INVALID
    assert lib.brt_host_volume_sample(g, recs.ctypes.data, pts.ctypes.data, 1, None) == INVALID
    assert lib.brt_host_volume_sample(g, recs.ctypes.data, pts.ctypes.data, 1, pts.ctypes.data + 16) == INVALID       # out over the points
    assert lib.brt_host_volume_sample(g, recs.ctypes.data, pts.ctypes.data, 1, recs.ctypes.data + 1008) == INVALID    # out over the records
    assert lib.brt_host_volume_sample(g, recs.ctypes.data, pts.ctypes.data, 0x7FFF0001, smp.ctypes.data) == INVALID
    assert lib.brt_host_volume_sample(g, None, None, 0, None) == 0                                                    # no points: OK
    # the exports that own a context refuse a null one
    assert lib.brt_volume_probes_device(None, g, out.ctypes.data, None, 0) == INVALID
    assert lib.brt_bake_volume_device(None, g, 64, 1, 0.0, recs.ctypes.data, None, 0, None) == INVALID
    assert lib.brt_bake_volume(None, g, 64, 1, 0.0, recs.ctypes.data, None) == INVALID
    assert lib.brt_sample_volume_device(None, g, recs.ctypes.data, pts.ctypes.data, 1, smp.ctypes.data, None, 0) == INVALID
    assert lib.brt_sample_volume(None, g, recs.ctypes.data, pts.ctypes.data, 1, smp.ctypes.data) == INVALID
    assert b"null" in lib.brt_last_error(None)


@pytest.mark.parametrize("count", LATTICES)
def test_the_host_twin_is_the_restatement(count):
    pts = _fixture_points(count)
    seen, negative, nans = set(), 0, 0
    for basis, flags, variant in _cases(count):
        want, detail = _want(count, basis, flags, variant)
        got = brt.volume_sample_host(_volume(count, basis, flags), _records(count, basis, variant), pts)
        vr.assert_samples_equal(got, want, f"{count} basis {basis} flags {flags} variant {variant}")
        # this fixture is not vacuous: refused points, clamped and unclamped ones; a refused record is seen as NO_PROBE at its node
        st = set(want["status"].tolist())
        assert BAD in st and {x & CLAMPED for x in st if x != BAD} == {0, CLAMPED}, (count, basis, flags, variant, st)
        rec = _records(count, basis, variant)
        if ((rec["status"] != 0) | (rec["basis"] != basis)).any():
            assert NO_PROBE in st, (count, basis, flags, variant, st)
        assert (want["rgb"][want["status"] == BAD] == 0).all() and (want["rgb"][(want["status"] & NO_PROBE) != 0] == 0).all()
        seen |= st
        lit = ~detail["bad"] & (detail["sw"] > 0)
        with np.errstate(invalid="ignore"):
            negative += int((detail["raw"][lit] < 0).sum())
        nans += int(np.isnan(want["rgb"]).sum())
        if flags == WRAP:                        # the len2 == 0 branch: a node with its own valid record and any normal is lit
            n_nodes = count[0] * count[1] * count[2]
            valid = (rec["status"] == 0) & (rec["basis"] == basis)
            assert ((want["status"][:n_nodes] & NO_PROBE) == 0)[valid].all()
    # every status combination that can occur, a sample that was negative before the clamp, a NaN output
    assert seen == {0, CLAMPED, BAD, NO_PROBE, CLAMPED | NO_PROBE}, seen
    assert negative > 0 and nans > 0, (negative, nans)
    if count == (5, 4, 3):
        want, detail = _want(count, SH9, 0, 0)
        tail = slice(len(pts) - 20000, None)
        lit = detail["sw"][tail] > 0
        print(f"5x4x3, 20 000 random points: clamped {np.mean((want['status'][tail] & CLAMPED) != 0):.3f}, NO_PROBE "
              f"{np.mean((want['status'][tail] & NO_PROBE) != 0):.4f}, smallest positive sw {detail['sw'][tail][lit].min():.3e}")


def test_the_host_twin_reads_buffers_at_any_address():
    """Host buffers that are only byte-aligned give the bytes of aligned ones (the device needs 16-byte alignment and checks it)."""
    lib = _lib.load()
    count = (5, 4, 3)
    pts = _fixture_points(count)[-2000:]
    for basis, flags in ((SH9, WRAP), (CUBE, 0)):
        vol, rec = _volume(count, basis, flags), _records(count, basis, 0)
        want = brt.volume_sample_host(vol, rec, pts)
        for shift in (1, 4, 9):
            raw = [np.zeros(a.nbytes + 16, np.uint8) for a in (rec, pts, want)]
            for r, a in zip(raw[:2], (rec, pts)):
                r[shift: shift + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            at = [r.ctypes.data + shift for r in raw]
            assert lib.brt_host_volume_sample(np.ascontiguousarray(vol).ctypes.data, at[0], at[1], len(pts), at[2]) == 0
            assert raw[2][shift: shift + want.nbytes].tobytes() == want.tobytes(), (basis, flags, shift)
            assert not raw[2][:shift].any() and not raw[2][shift + want.nbytes:].any()


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def _one_record(basis):
    rng = np.random.default_rng(53 + basis)
    one = np.zeros(1, brt.PROBE_RECORD_DTYPE)
    one["coeff"] = rng.uniform(-2, 4, size=27).astype(F32)
    if basis == CUBE:
        one["coeff"][0, 18:] = 0
    one["n_dirs"], one["basis"] = 64, basis
    one.setflags(write=False)
    return one


def test_the_f32_rule_against_float64():
    """The restatement in f32 against the same rule in float64 on the 20 000 random points of the 5x4x3 lattice, every record the same
    valid one with coefficients in [-2, 4] (the configuration of the same-records test below), relative to max(1, |E|).  Measured:
    SH9 6.49e-7, SH9 with BRT_VOLUME_WRAP 7.41e-7, cube 3.10e-7, cube with BRT_VOLUME_WRAP 3.76e-7; SAME_TOLERANCE is 4 x 7.5e-7.
    For information, not asserted: with sixty different records, ten of them refused, the two differ by up to 1.4e-5, at points whose
    lit corners weigh 1e-3 together: f = t - f32(i0) carries t's rounding, which is as large as such a weight's last digits."""
    count, worst = (5, 4, 3), 0.0
    pts = _fixture_points(count)[-20000:]
    for basis in (SH9, CUBE):
        for flags in (0, WRAP):
            vol, rec = _volume(count, basis, flags), np.repeat(_one_record(basis), 60)
            d32, d64 = {}, {}
            vr.sample(vol, rec, pts, detail=d32)
            vr.sample(vol, rec, pts, ft=np.float64, detail=d64)
            assert (d32["sw"] > 0).all() and (d64["sw"] > 0).all() and (d64["raw"] < 0).any()
            rel = _rel(d32["rgb"].astype(np.float64), d64["rgb"]).max()
            print(f"basis {basis} flags {flags}: {rel:.3e}")
            worst = max(worst, rel)
    assert worst <= SAME_TOLERANCE / 4, worst


@pytest.mark.parametrize("basis", [SH9, CUBE])
@pytest.mark.parametrize("flags", [0, WRAP])
def test_eight_identical_records_give_that_records_own_evaluation(basis, flags):
    count = (5, 4, 3)
    pts = _fixture_points(count)[-20000:]
    one = _one_record(basis)
    got = brt.volume_sample_host(_volume(count, basis, flags), np.repeat(one, 60), pts)
    assert ((got["status"] & ~np.uint32(CLAMPED)) == 0).all()
    own = vr.evaluate(np.repeat(one["coeff"], len(pts), axis=0), pts["normal"], basis).astype(np.float64)
    assert (own < 0).any() and (own > 1).any()
    want = np.where(own < 0, 0.0, own)
    rel = _rel(got["rgb"].astype(np.float64), want).max()
    print(f"basis {basis} flags {flags}: {rel:.3e}")
    assert rel <= SAME_TOLERANCE
    # ... and that evaluation is the existing export's: brt_host_probe_irradiance / probe_ref.irradiance64 on the record
    pick = np.flatnonzero((np.abs(own) > 0.5).all(axis=1))[:64]
    assert len(pick) == 64
    for i in pick:
        e64 = pr.irradiance64(one[0], pts["normal"][i])
        assert (np.abs(own[i] - e64) <= HOST_EXPORT_TOLERANCE * np.abs(e64)).all(), (i, own[i], e64)
        lit = np.where(e64 < 0, 0.0, e64)
        assert (np.abs(got["rgb"][i] - lit) <= HOST_EXPORT_TOLERANCE * np.abs(e64) + SAME_TOLERANCE * np.maximum(1.0, np.abs(e64))).all()
        assert (np.abs(brt.probe_irradiance(one[0], pts["normal"][i]) - e64) <= HOST_EXPORT_TOLERANCE * np.abs(e64)).all()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _sample_device(plugin, vol, d_records, pts, stream=None):
    """brt_sample_volume_device on a host list; the sample behind the output is a guard."""
    import torch
    d_pts = _dev(pts)
    d_out = _guarded(len(pts) * 16, 16, 0xCD)
    plugin.node.sample_volume(vol, d_records.data_ptr(), (d_pts.data_ptr(), len(pts), d_out.data_ptr()), device=True, stream=stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[len(pts) * 16:] == 0xCD).all(), "the guard sample was written"
    return got[:len(pts) * 16].view(brt.VOLUME_SAMPLE_DTYPE)


@pytest.mark.gpu
@pytest.mark.parametrize("count", LATTICES + [(1024, 1, 1)])
def test_generated_probes_are_the_host_exports(plugin, count):
    import torch
    n = count[0] * count[1] * count[2]
    for seed in (0xFFFFFF00, 5):
        vol = _volume(count, seed=seed)
        d_probes = _guarded(n * 16, 16, 0xAB)
        plugin.node.volume_probes_device(vol, d_probes.data_ptr())
        torch.cuda.synchronize()
        got = d_probes.cpu().numpy()
        assert (got[n * 16:] == 0xAB).all(), "the guard probe was written"
        assert got[:n * 16].tobytes() == brt.volume_probes(vol).tobytes() == vr.probes(vol).tobytes(), (count, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("count", LATTICES)
@pytest.mark.parametrize("flags", [0, WRAP])
@pytest.mark.parametrize("basis", [SH9, CUBE])
def test_the_kernel_is_the_host_twin_and_the_restatement(plugin, basis, flags, count):
    pts = _fixture_points(count)
    vol = _volume(count, basis, flags)
    for variant in range(_variants(count)):
        rec = _records(count, basis, variant)
        want, _ = _want(count, basis, flags, variant)
        twin = brt.volume_sample_host(vol, rec, pts)
        d_rec = _dev(rec)
        got = _sample_device(plugin, vol, d_rec, pts)
        what = f"{count} basis {basis} flags {flags} variant {variant}"
        vr.assert_samples_equal(got, want, what)
        assert got.tobytes() == twin.tobytes(), what                  # (the two compiled forms agree in every bit, NaN payloads included)
        if variant == 0:
            host = plugin.node.sample_volume(vol, rec, pts)
            assert host.tobytes() == twin.tobytes(), what + ", host entry point"
    if count == (5, 4, 3):
        rec, d_rec = _records(count, basis, 0), _dev(_records(count, basis, 0))
        want, _ = _want(count, basis, flags, 0)
        tail = len(pts) - 20001
        for n in (1, 63, 64, 65, 255, 256, 257, 20001):
            got = _sample_device(plugin, vol, d_rec, pts[tail: tail + n])
            vr.assert_samples_equal(got, want[tail: tail + n], f"list of {n}")
            if n <= 257:
                assert plugin.node.sample_volume(vol, rec, pts[tail: tail + n]).tobytes() == got.tobytes(), n


COVER_COUNT = (4, 3, 4)


def _cover_volume(basis, flags=0):
    return brt.make_volume((-4.5, 0.3, -4.5), (3.0, 1.2, 3.0), COVER_COUNT, basis, 0xFFFFFFF0, flags)


def _bake_probes_device(plugin, probes, n_dirs, bounces, basis, **knobs):
    import torch
    d_probes, d_out = _dev(probes), _guarded(len(probes) * 128, 128, 0xCD)
    with plugin.tuning(**knobs):
        st = dict(plugin.node.bake_probes((d_probes.data_ptr(), len(probes), d_out.data_ptr()), n_dirs, bounces, basis, device=True))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:len(probes) * 128].view(brt.PROBE_RECORD_DTYPE), st


def _bake_volume_device(plugin, vol, n_dirs, bounces, stream=None, **knobs):
    import torch
    n = vr.n_probes(vol)
    d_out = _guarded(n * 128, 128, 0xCD)
    with plugin.tuning(**knobs):
        st = dict(plugin.node.bake_volume(vol, n_dirs, bounces, d_records=d_out.data_ptr(), stream=stream))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n * 128:] == 0xCD).all(), "the guard record was written"
    return got[:n * 128].view(brt.PROBE_RECORD_DTYPE), st, d_out


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["caller", "callee"])
def test_a_baked_volume_is_the_bake_of_its_probes(plugin, tree):
    _upload_cover(plugin, tree)
    three_chunks = {"BRT_PROBE_CHUNK_RAYS": 16 * 64}             # 48 probes x 64 directions in chunks of 16 probes
    for basis in (SH9, CUBE):
        vol = _cover_volume(basis)
        probes = brt.volume_probes(vol)
        want, st_want = _bake_probes_device(plugin, probes, 64, 8, basis)
        assert (want["status"] == 0).all() and want["hits"].sum() > 0 and len(set(want["coeff"][:, 0].tolist())) > 40
        got, st, _ = _bake_volume_device(plugin, vol, 64, 8)
        assert got.tobytes() == want.tobytes(), (tree, basis)
        assert st == st_want and st["chunks"] == 1, (st, st_want)
        host = plugin.node.bake_volume(vol, 64, 8)
        assert host.tobytes() == want.tobytes(), (tree, basis, "host")
        assert plugin.node.last_probe_stats == st_want
        _, st_want3 = _bake_probes_device(plugin, probes, 64, 8, basis, **three_chunks)
        got3, st3, _ = _bake_volume_device(plugin, vol, 64, 8, **three_chunks)
        assert got3.tobytes() == want.tobytes() and st3 == st_want3 and st3["chunks"] == 3, (st3, st_want3)
        with plugin.tuning(**three_chunks):
            assert plugin.node.bake_volume(vol, 64, 8).tobytes() == want.tobytes()
            assert plugin.node.last_probe_stats["chunks"] == 3
    if tree == "callee":
        # one probe beyond the tree's bound: its record is refused, and samples beside it carry the renormalised weight of the other
        bound = plugin.node.query_origin_bound()
        vol = brt.make_volume((-1.0, 0.5, 0.25), (2.0 * bound, 1.0, 1.0), (2, 1, 1), SH9, 9, 0)
        probes = brt.volume_probes(vol)
        rec, st, d_rec = _bake_volume_device(plugin, vol, 64, 8)
        want, _ = _bake_probes_device(plugin, probes, 64, 8, SH9)
        assert rec.tobytes() == want.tobytes() and list(rec["status"]) == [0, brt.QUERY_STATUS_OUT_OF_REACH] and st["refused"] == 64
        rng = np.random.default_rng(54)
        pts = _points(np.stack([rng.uniform(-1.0, 2.0 * bound - 1.0, 200), np.full(200, 0.5), np.full(200, 0.25)], axis=1), _unit(rng, 200))
        got = _sample_device(plugin, vol, d_rec, pts)
        vr.assert_samples_equal(got, vr.sample(vol, rec, pts), "beside a refused probe")
        assert (got["status"] == 0).all()
        own = vr.evaluate(np.repeat(rec["coeff"][:1], 200, axis=0), pts["normal"], SH9).astype(np.float64)
        assert _rel(got["rgb"].astype(np.float64), np.where(own < 0, 0.0, own)).max() <= SAME_TOLERANCE
        far = _points([(3.0 * bound, 0.5, 0.25)], (0.0, 1.0, 0.0))                           # clamped onto the refused node: no probe
        assert _sample_device(plugin, vol, d_rec, far)["status"][0] == CLAMPED | NO_PROBE


@pytest.mark.gpu
def test_a_g_buffer_list_end_to_end(plugin):
    _upload_cover(plugin, "caller")
    w = h = 64
    lvl, cam, win = brt.cover_camera(w, h, 1, 1)
    rays = np.concatenate([brt.pixel_ray(cam, win, w, h, px, py) for py in range(h) for px in range(w)])
    hits = plugin.node.query_rays(rays, brt.QUERY_CLOSEST)
    hit = (hits["status"] & brt.QUERY_STATUS_HIT) != 0
    print(f"{hit.sum()} of 4096 pixel rays hit")
    assert hit.sum() > 500
    with np.errstate(all="ignore"):
        pos = (rays["origin"] + (hits["t"][:, None] * rays["direction"]).astype(F32)).astype(F32)    # (a miss: t = INF, a refused point)
    pts = _points(pos, hits["normal"])
    for basis, flags in ((SH9, 0), (SH9, WRAP), (CUBE, 0), (CUBE, WRAP)):
        vol = _cover_volume(basis, flags)
        rec, _, d_rec = _bake_volume_device(plugin, vol, 64, 8)
        got = _sample_device(plugin, vol, d_rec, pts)
        vr.assert_samples_equal(got, vr.sample(vol, rec, pts), f"basis {basis} flags {flags}")
        assert ((got["status"] == BAD) == ~hit).all()
        lit = got["rgb"][hit]
        assert (lit >= 0).all() and lit.mean() > 0.05 and len(np.unique(lit[:, 0])) > 400
        assert (got["status"][hit] & NO_PROBE == 0).all() and ((got["status"][hit] & CLAMPED) != 0).any() and (got["status"][hit] == 0).any()


@pytest.mark.gpu
def test_an_empty_sky_against_the_analytic_irradiance(plugin):
    plugin.node.write_buffers(make_buffers([((300.0, 400.0, 500.0), 0.01, brt.StandardMaterial())]))
    rng = np.random.default_rng(55)
    pts = _points(rng.uniform(-6, 6, size=(2000, 3)), _unit(rng, 2000))
    A, B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])
    want = np.pi * A[None, :] + (2.0 * np.pi / 3.0) * B[None, :] * pts["normal"][:, 1:2].astype(np.float64)
    for flags in (0, WRAP):
        vol = brt.make_volume((-3.0, -2.0, -3.0), (3.0, 2.0, 3.0), (3, 3, 3), SH9, 77, flags)
        rec, st, d_rec = _bake_volume_device(plugin, vol, 1024, 8)
        assert (rec["hits"] == 0).all() and (rec["status"] == 0).all()
        got = _sample_device(plugin, vol, d_rec, pts)
        assert ((got["status"] & ~np.uint32(CLAMPED)) == 0).all() and ((got["status"] & CLAMPED) != 0).any() and (got["status"] == 0).any()
        err = np.abs(got["rgb"].astype(np.float64) - want)
        print(f"flags {flags}: largest |E - analytic| {err.max():.3e}")
        assert (err <= SKY_E_BOUND + SAME_TOLERANCE * np.maximum(1.0, np.abs(want))).all()


@pytest.mark.gpu
def test_streams_uploads_frames_and_refusals(plugin):
    import torch
    b = _cover()
    w, h = 160, 90
    lvl, cam, win = brt.cover_camera(w, h, 2, 4, brt.Raytracing.Pure, 0.5)
    before = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=brt.FLAG_COUNTERS).copy()
    stats_before = dict(plugin.node.last_stats)
    vol = _cover_volume(SH9, WRAP)
    n = vr.n_probes(vol)
    rng = np.random.default_rng(56)
    pts = _points(rng.uniform((-6, 0, -6), (6, 4, 6), size=(5000, 3)), _unit(rng, 5000))
    rec, _, d_rec = _bake_volume_device(plugin, vol, 64, 4)
    serial = _sample_device(plugin, vol, d_rec, pts).copy()
    vr.assert_samples_equal(serial, vr.sample(vol, rec, pts), "one stream")
    # a bake on one caller stream, the sample on another: the same bytes
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_rec2 = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
    d_pts, d_out = _dev(pts), torch.zeros(len(pts) * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = plugin.node.bake_volume(vol, 64, 4, d_records=d_rec2.data_ptr(), stream=s1.cuda_stream)
    assert (st["walks"], st["hits"], st["refused"], st["chunks"]) == (0, 0, 0, 1)
    plugin.node.sample_volume(vol, d_rec2.data_ptr(), (d_pts.data_ptr(), len(pts), d_out.data_ptr()), device=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert d_rec2.cpu().numpy().tobytes() == rec.tobytes()
    assert d_out.cpu().numpy().tobytes() == serial.tobytes()
    # an upload between the bake and the sample changes nothing in the samples
    moved = b.models.copy()
    moved["position"][np.flatnonzero(moved["radius"] == 1.0)] += np.array([0.0, 0.6, 0.0], F32)
    d_out.zero_()
    torch.cuda.synchronize()
    plugin.node.bake_volume(vol, 64, 4, d_records=d_rec2.data_ptr(), stream=s1.cuda_stream)
    plugin.node.write_buffers(brt.Buffers(moved, b.materials, brt.build_bvh(moved)))
    plugin.node.sample_volume(vol, d_rec2.data_ptr(), (d_pts.data_ptr(), len(pts), d_out.data_ptr()), device=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == serial.tobytes()
    assert _bake_volume_device(plugin, vol, 64, 4)[0].tobytes() != rec.tobytes()             # (the new scene bakes other records)
    plugin.node.write_buffers(b)

    # every refusal is followed by a correct call
    lib, ctx = plugin._lib, plugin._ctx
    g = np.ascontiguousarray(vol).ctypes.data
    bad = vol.copy()
    bad["count"][0, 1] = 0
    d_buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    d_a, d_b = d_buf.data_ptr(), d_buf.data_ptr() + (1 << 19)
    host_rec, host_out = np.zeros(n, brt.PROBE_RECORD_DTYPE), np.zeros(len(pts), brt.VOLUME_SAMPLE_DTYPE)
    hp = np.ascontiguousarray(pts)

    def refused(code, call, what):
        assert call() == code, what
        assert _sample_device(plugin, vol, d_rec, pts).tobytes() == serial.tobytes(), f"after {what}"

    R, P, O = d_rec.data_ptr(), d_pts.data_ptr(), d_out.data_ptr()
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, bad.ctypes.data, R, P, 10, O, None, 0), "a bad descriptor")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, None, R, P, 10, O, None, 0), "no descriptor")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, None, P, 10, O, None, 0), "null records")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, None, 10, O, None, 0), "null points")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 10, None, None, 0), "null out")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 10, P + 16, None, 0), "out over the points")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 10, R + 128, None, 0), "out over the records")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 0x7FFF0001, O, None, 0), "too many points")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P + 8, 10, O, None, 0), "points not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R + 4, P, 10, O, None, 0), "records not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 10, d_a + 12, None, 0), "out not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_sample_volume_device(ctx, g, R, P, 10, O, None, brt.FLAG_DENOISE), "unknown flag")
    refused(INVALID, lambda: lib.brt_sample_volume(ctx, bad.ctypes.data, host_rec.ctypes.data, hp.ctypes.data, 10, host_out.ctypes.data), "host, bad descriptor")
    refused(INVALID, lambda: lib.brt_sample_volume(ctx, g, host_rec.ctypes.data, hp.ctypes.data, 10, hp.ctypes.data + 16), "host, overlap")
    refused(INVALID, lambda: lib.brt_volume_probes_device(ctx, bad.ctypes.data, d_a, None, 0), "probes, bad descriptor")
    refused(INVALID, lambda: lib.brt_volume_probes_device(ctx, g, None, None, 0), "probes, null")
    refused(INVALID, lambda: lib.brt_volume_probes_device(ctx, g, d_a + 4, None, 0), "probes, not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_volume_probes_device(ctx, g, d_a, None, brt.FLAG_COUNTERS), "probes, unknown flag")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, bad.ctypes.data, 64, 4, 0.0, d_a, None, 0, None), "bake, bad descriptor")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 0, 4, 0.0, d_a, None, 0, None), "bake, n_dirs 0")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 65537, 4, 0.0, d_a, None, 0, None), "bake, n_dirs 65537")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 65536, 0.0, d_a, None, 0, None), "bake, bounces 65536")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, float("nan"), d_a, None, 0, None), "bake, origin_bound NaN")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, -1.0, d_a, None, 0, None), "bake, origin_bound < 0")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, 0.0, None, None, 0, None), "bake, null records")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, 0.0, d_a + 8, None, 0, None), "bake, records not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, 0.0, d_a, None, brt.FLAG_DENOISE, None), "bake, unknown flag")
    refused(INVALID, lambda: lib.brt_bake_volume(ctx, g, 0, 4, 0.0, host_rec.ctypes.data, None), "host bake, n_dirs 0")
    refused(INVALID, lambda: lib.brt_bake_volume(ctx, g, 64, 4, 0.0, None, None), "host bake, null records")
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        refused(UNSUPPORTED, lambda: lib.brt_bake_volume(ctx, g, 64, 4, 0.0, host_rec.ctypes.data, None), "host bake under a policy")
        refused(UNSUPPORTED, lambda: lib.brt_bake_volume_device(ctx, g, 64, 4, 0.0, d_a, None, 0, None), "bake under a policy")
    finally:
        plugin.set_policy(0)
    assert lib.brt_sample_volume_device(ctx, g, None, None, 0, None, None, 0) == 0          # no points: OK, nothing launched
    assert plugin.node.sample_volume(vol, rec, pts[:0]).shape == (0,)
    assert _bake_volume_device(plugin, vol, 64, 4)[0].tobytes() == rec.tobytes()
    with brt.RaytracePlugin([0]) as empty:
        for call in (lambda: empty.node.bake_volume(vol, 64, 4), lambda: empty.node.bake_volume(vol, 64, 4, d_records=d_b)):
            with pytest.raises(brt.BrtError) as e:
                call()
            assert e.value.code == NO_SCENE
        assert empty.node.sample_volume(vol, rec, pts).tobytes() == serial.tobytes()        # sampling needs no scene
        empty.node.write_buffers(b)
        assert empty.node.bake_volume(vol, 64, 4).tobytes() == rec.tobytes()

    # a plain frame after all of it is the frame before
    after = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for k in ("rays", "node_pops", "interior_visits", "sphere_tests", "hits", "kernel_variant", "n_workgroups", "scene_in_lds"):
        assert plugin.node.last_stats[k] == stats_before[k], k
