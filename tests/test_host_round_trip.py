"""One staging buffer for every host form (brt_frame.h host_round_trip): the host-buffer exports of all families in turn on ONE context,
each held to the device form of the same call.

The sequence makes consecutive calls come from different families, makes the staged size grow, shrink and grow past its earlier
maximum, and puts two device-form calls on callers' streams (a lightmap bake and a query, each held back by a sleep kernel) in front of
host forms, so that a host form stages -- and grows the buffer -- behind work that is still in flight.  Afterwards every host-form
result is compared, byte for byte, with the device form of the same call on that context (inputs uploaded through torch, the context's
own stream), and the stats words with it (all of them: on the own stream the device form counts too; times excepted).

The shapes are the smallest at which the plumbing can go wrong: frames of 20x12 and 40x24 (neither a multiple of 8 in both axes: the
progressive tile order pads), lists of 7, 300 and 70 entries (below, above and again below one workgroup of 256), 8 directions, a 6x4
lightmap, an envmap of size 4 with 2 levels."""
import numpy as np
import pytest

import bevyray_amd as brt
import gbuffer_cases as gc
from helpers import cover, dev

F32 = np.float32
TIMES = ("kernel_ms", "gather_ms", "total_ms", "prepass_ms")
SMALL, LARGE = (20, 12), (40, 24)
SPP, BOUNCES, N_DIRS = 2, 3, 8


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _down(t, like):
    """The bytes of a device tensor as a host array shaped like `like`"""
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _no_times(stats):
    return {k: v for k, v in stats.items() if k not in TIMES}


def _view(size):
    return brt.cover_camera(*size, SPP, BOUNCES)[1:]


def _rays(rng, n, dtype):
    """n rays from around the cover view towards the scene's middle: hits and misses"""
    rays = np.zeros(n, dtype)
    rays["origin"] = (np.array([13.0, 2.0, 3.0]) + rng.uniform(-1.0, 1.0, (n, 3))).astype(F32)
    rays["direction"] = (rng.uniform(-4.0, 4.0, (n, 3)) - rays["origin"]).astype(F32)
    rays["user"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    if "t_max" in dtype.names:
        rays["t_max"] = np.inf
    else:
        rays["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    return rays


def _lightmap_points():
    b = cover()
    i = int(np.flatnonzero(b.models["radius"] < 10.0)[0])
    r = float(b.models["radius"][i])
    return brt.lightmap_sphere_points(b.models["position"][i], r, 6, 4, seed=11, offset=1e-3 * r)


# ---- the calls: each -> (what the host form returned, what the device form returned), as {name: array} and a stats dict ----------------

def _query(n, seed):
    rays = _rays(np.random.default_rng(seed), n, brt.RAY_DTYPE)

    def host(node):
        return {"hits": node.query_rays(rays)}, node.last_query_stats

    def device(node, stream=None):
        import torch
        d_rays, d_hits = dev(rays), torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        st = node.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=stream)
        return lambda: {"hits": _down(d_hits, np.zeros(n, brt.HIT_DTYPE))}, st, (d_rays, d_hits)
    return "query", host, device


def _radiance(n, seed):
    rays = _rays(np.random.default_rng(seed), n, brt.RADIANCE_RAY_DTYPE)

    def host(node):
        return {"out": node.radiance_rays(rays, SPP, BOUNCES)}, node.last_radiance_stats

    def device(node, stream=None):
        import torch
        d_rays, d_out = dev(rays), torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        st = node.radiance_rays((d_rays.data_ptr(), n, d_out.data_ptr()), SPP, BOUNCES, device=True, stream=stream)
        return lambda: {"out": _down(d_out, np.zeros(n, brt.RADIANCE_DTYPE))}, st, (d_rays, d_out)
    return "radiance", host, device


def _pixels(n, size, seed, flags=0):
    cam, win = _view(size)
    w, h = size
    px = np.random.default_rng(seed).permutation(w * h)[:n].astype(np.uint32)

    def host(node):
        return {"pixels": node.render_pixels(cam, win, w, h, px, flags)}, _no_times(node.last_stats)

    def device(node, stream=None):
        import torch
        d_px, d_out = dev(px), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        st = node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), n, d_out.data_ptr(), stream=stream, flags=flags)
        return lambda: {"pixels": _down(d_out, np.zeros((n, 4), F32))}, _no_times(st), (d_px, d_out)
    return "pixels", host, device


def _probes(n, seed):
    rng = np.random.default_rng(seed)
    probes = np.zeros(n, brt.PROBE_DTYPE)
    probes["position"] = rng.uniform((-3.0, 0.5, -3.0), (3.0, 3.0, 3.0), (n, 3)).astype(F32)
    probes["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)

    def host(node):
        return {"records": node.bake_probes(probes, N_DIRS, BOUNCES)}, node.last_probe_stats

    def device(node, stream=None):
        import torch
        d_probes, d_out = dev(probes), torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
        st = node.bake_probes((d_probes.data_ptr(), n, d_out.data_ptr()), N_DIRS, BOUNCES, device=True, stream=stream)
        return lambda: {"records": _down(d_out, np.zeros(n, brt.PROBE_RECORD_DTYPE))}, st, (d_probes, d_out)
    return "probes", host, device


VOLUME = brt.make_volume((-1.0, 0.5, -1.0), (2.0, 1.5, 2.0), (2, 2, 2), brt.PROBE_SH9, 5, 0)


def _volume_bake():
    def host(node):
        return {"records": node.bake_volume(VOLUME, N_DIRS, BOUNCES)}, node.last_probe_stats

    def device(node, stream=None):
        import torch
        d_rec = torch.zeros(8 * 128, dtype=torch.uint8, device="cuda")
        st = node.bake_volume(VOLUME, N_DIRS, BOUNCES, d_records=d_rec.data_ptr(), stream=stream)
        return lambda: {"records": _down(d_rec, np.zeros(8, brt.PROBE_RECORD_DTYPE))}, st, (d_rec,)
    return "volume_bake", host, device


def _volume_sample(n, seed, records):
    """`records`: a one-element list the volume bake's step fills in before this step runs"""
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, brt.VOLUME_POINT_DTYPE)
    pts["position"] = rng.uniform((-1.5, 0.0, -1.5), (1.5, 2.5, 1.5), (n, 3)).astype(F32)
    nrm = rng.standard_normal((n, 3))
    pts["normal"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F32)

    def host(node):
        return {"samples": node.sample_volume(VOLUME, records[0], pts)}, {}

    def device(node, stream=None):
        import torch
        d_rec, d_pts, d_out = dev(records[0]), dev(pts), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        node.sample_volume(VOLUME, d_rec.data_ptr(), (d_pts.data_ptr(), n, d_out.data_ptr()), device=True, stream=stream)
        return lambda: {"samples": _down(d_out, np.zeros(n, brt.VOLUME_SAMPLE_DTYPE))}, {}, (d_rec, d_pts, d_out)
    return "volume_sample", host, device


def _envmap():
    pos, size, levels, taps = (0.0, 2.0, 0.0), 4, 2, 8
    n = brt.envmap_level_offsets(size, levels)[-1]

    def host(node):
        return {"chain": node.bake_envmap(pos, size, levels, 1, BOUNCES, n_taps=taps, seed=3)}, node.last_probe_stats

    def device(node, stream=None):
        import torch
        d_out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        st = node.bake_envmap(pos, size, levels, 1, BOUNCES, n_taps=taps, seed=3, d_out=d_out.data_ptr(), stream=stream)
        return lambda: {"chain": _down(d_out, np.zeros((n, 4), F32))}, st, (d_out,)
    return "envmap", host, device


def _lightmap(passes, info):
    pts = _lightmap_points()

    def host(node):
        texels, rec = node.bake_lightmap(pts, N_DIRS, BOUNCES, passes=passes, info=info)
        assert (rec is not None) == info
        return ({"texels": texels, "info": rec} if info else {"texels": texels}), node.last_probe_stats

    def device(node, stream=None):
        import torch
        d_pts, d_out = dev(pts), torch.zeros(24 * 16, dtype=torch.uint8, device="cuda")
        d_info = torch.zeros(24 * 8, dtype=torch.uint8, device="cuda") if info else None
        st = node.bake_lightmap((d_pts.data_ptr(), 6, 4, d_out.data_ptr(), d_info.data_ptr() if info else 0), N_DIRS, BOUNCES, passes=passes,
                                device=True, stream=stream)

        def read():
            out = {"texels": _down(d_out, np.zeros((4, 6, 4), F32))}
            if info:
                out["info"] = _down(d_info, np.zeros((4, 6), brt.LIGHTMAP_INFO_DTYPE))
            return out
        return read, st, (d_pts, d_out, d_info)
    return "lightmap", host, device


def _gbuffer(size, planes, full):
    """full: with a previous camera, previous models and a coverage frame, over planes the caller filled with 0x5A"""
    cam, win = _view(size)
    w, h = size
    desc = brt.gbuffer(brt.GBUFFER_DEPTH_SHADER, brt.GBUFFER_NORMAL_RGB10A2, brt.GBUFFER_MOTION_UV16F) if full else brt.gbuffer()
    prev_cam = brt.cover_camera(w, h, SPP, BOUNCES, seed=0.25)[1] if full else None
    prev_models = gc.moved_models(cover().models, (0.0, 0.5, 0.0))[0] if full else None
    cov = gc.coverage_frame(w, h, "blocks") if full else None

    def filled():
        into = {k: brt.gbuffer_plane(desc, k, w, h) for k in planes}
        for a in into.values():
            a.view(np.uint8)[...] = 0x5A
        return into

    def host(node):
        got = node.render_gbuffer(cam, win, w, h, desc, planes, prev_camera=prev_cam, prev_models=prev_models, coverage=cov, into=filled())
        return got, node.last_gbuffer_stats

    def device(node, stream=None):
        into = filled()
        d = {k: dev(a) for k, a in into.items()}
        d_prev, d_cov = (dev(prev_models), dev(cov)) if full else (None, None)
        st = node.render_gbuffer_device(cam, win, w, h, desc, **{"d_" + k: t.data_ptr() for k, t in d.items()}, prev_camera=prev_cam,
                                        d_prev_models=d_prev.data_ptr() if full else 0, d_coverage=d_cov.data_ptr() if full else 0,
                                        stream=stream)
        return lambda: {k: _down(t, into[k]) for k, t in d.items()}, st, (d, d_prev, d_cov)
    return "gbuffer", host, device


def _prog_state(size, seed):
    """A state plane half of whose pixels hold one sample already (a sum, a mean, a generator state, a ray count: the call continues
    them, so what it returns depends on the plane having gone in); the others are new"""
    w, h = size
    rng = np.random.default_rng(seed)
    st = np.zeros((h, w), brt.PROG_PIXEL_DTYPE)
    run = rng.random((h, w)) < 0.5
    st["sum"][run] = rng.random((int(run.sum()), 3), dtype=F32)
    st["m1"][run] = st["sum"][run].mean(axis=1)
    st["rng"][run] = rng.integers(1, 2 ** 32, int(run.sum()), dtype=np.uint32)
    st["n"][run] = 1
    st["rays"][run] = 3
    return st


def _prog_sample(size, seed, listed, with_frame):
    cam, win = _view(size)
    w, h = size
    px = np.random.default_rng(seed).permutation(w * h)[:listed].astype(np.uint32) if listed else None
    first = np.full((h, w, 4), 0.25, F32)

    def host(node):
        state, frame = _prog_state(size, seed), first.copy() if with_frame else None
        node.progressive_sample(cam, win, w, h, state, 3, pixels=px, frame=frame)
        return ({"state": state, "frame": frame} if with_frame else {"state": state}), _no_times(node.last_stats)

    def device(node, stream=None):
        d_state, d_frame = dev(_prog_state(size, seed)), dev(first) if with_frame else None
        d_px = dev(px) if listed else None
        st = node.progressive_sample_device(cam, win, w, h, d_state.data_ptr(), 3, d_px.data_ptr() if listed else 0, listed or None,
                                            d_frame=d_frame.data_ptr() if with_frame else 0, stream=stream)

        def read():
            out = {"state": _down(d_state, _prog_state(size, seed))}
            if with_frame:
                out["frame"] = _down(d_frame, first)
            return out
        return read, _no_times(st), (d_state, d_frame, d_px)
    return "progressive_sample", host, device


def _prog_render(size, seed):
    cam, win = _view(size)
    w, h = size

    def host(node):
        state, frame = _prog_state(size, seed), np.zeros((h, w, 4), F32)
        node.render_progressive(cam, win, w, h, state, frame)
        return {"state": state, "frame": frame}, _no_times(node.last_stats)

    def device(node, stream=None):
        import torch
        d_state, d_frame = dev(_prog_state(size, seed)), torch.zeros(w * h * 16, dtype=torch.uint8, device="cuda")
        st = node.render_progressive_device(cam, win, w, h, d_state.data_ptr(), d_frame.data_ptr(), stream=stream)
        return (lambda: {"state": _down(d_state, _prog_state(size, seed)), "frame": _down(d_frame, np.zeros((h, w, 4), F32))}), _no_times(st), \
            (d_state, d_frame)
    return "progressive_render", host, device


def _sequence():
    """-> [(family, host, device) or ("held", family, device)]: consecutive host calls from different families; the bytes staged per
    call (each plane rounded up to 256) first grow, then shrink, then pass the earlier maximum twice, each time behind a held call"""
    records = [None]
    bake = _volume_bake()

    def bake_and_keep(node):
        got, st = bake[1](node)
        records[0] = got["records"].copy()
        return got, st
    return [
        _query(7, 1),                                         # 512 bytes
        _gbuffer(SMALL, ("depth",), False),                   # 1 024
        _radiance(300, 2),                                    # 19 456: grows
        _pixels(70, SMALL, 3),                                # 1 536: shrinks
        _probes(7, 4),
        ("held", _lightmap(1, True)),
        _prog_sample(LARGE, 5, 0, True),                      # 46 080: past the maximum, behind the held bake
        ("volume_bake", bake_and_keep, bake[2]),
        _lightmap(0, False),
        _volume_sample(300, 6, records),
        _envmap(),
        ("held", _query(300, 7)),
        _gbuffer(LARGE, brt.GBUFFER_PLANES, True),            # 77 056 and the models: past it again, behind the held query
        _prog_render(SMALL, 8),
        _lightmap(1, True),
        _query(300, 7),
        _prog_sample(SMALL, 9, 70, False),
        _radiance(70, 10),
        _pixels(300, LARGE, 11, brt.FLAG_KERNEL_SIMPLE),
        _query(70, 12),
        _pixels(7, SMALL, 13),
    ]


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(_bytes(got[k]), _bytes(want[k])), f"{what}: {k} differs between the two forms"


@pytest.mark.gpu
def test_every_host_form_in_turn_on_one_staging_buffer():
    import torch
    steps = _sequence()
    families = [s[0] for s in steps if s[0] != "held"]
    assert all(a != b for a, b in zip(families, families[1:]))
    assert {"query", "radiance", "volume_sample", "probes", "lightmap", "pixels", "progressive_sample", "progressive_render",
            "gbuffer"} <= set(families)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with brt.RaytracePlugin([0]) as plugin:
        node = plugin.node
        node.write_buffers(cover())
        plugin.set_progressive(2, 4)
        torch.cuda.synchronize()
        hosts, helds = [], []
        for step in steps:
            if step[0] == "held":
                s = streams[len(helds)]
                with torch.cuda.stream(s):
                    torch.cuda._sleep(20_000_000)              # (a few ms: the call starts after the host forms behind it have been made)
                read, st, keep = step[1][2](node, stream=s.cuda_stream)
                helds.append((step[1], read, keep))
            else:
                hosts.append((step, *step[1](node)))
        torch.cuda.synchronize()
        # the held calls computed what the host form of the same call computes (their counts stay 0: a caller's stream)
        for (family, host, _), read, _keep in helds:
            _same(read(), host(node)[0], f"held {family}")
        # every host form against the device form of the same call on this context
        for i, ((family, _host, device), got, stats) in enumerate(hosts):
            read, dev_stats, _keep = device(node)
            torch.cuda.synchronize()
            _same(got, read(), f"step {i} {family}")
            assert stats == dev_stats, f"step {i} {family}: stats {stats} != {dev_stats}"
