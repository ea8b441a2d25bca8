"""Calls of one context in flight on several caller streams at once -- needs an MI355X.

include/bevyray_amd.h promises that a call of a context first makes its stream wait for the previous call's kernel, whatever
stream that ran on, and that a call uses the strip table in force when it is called.  These tests put that to work with more than
one call really in flight: a side stream runs torch.cuda._sleep, stream A waits on it (HELD), the call under test is enqueued on
A and the next calls on other streams.  Their host work is then certain to run before A's kernel starts, so a buffer that one
call rewrites under another shows every time, not sometimes.  Nothing waits on work the host has yet to do.  Every tile and frame
is held to the CPU oracle bit for bit; a synchronous call's ray count is held to the oracle's count of the same strips.
"""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
from bevyray_amd.parallel import frame_rows_of_part
from test_parity_gpu import COUNTER_KEYS, assert_frames_equal

pytestmark = pytest.mark.gpu

W, H = 200, 149                 # 19 strips: the last group of every split is partial
SPP, BOUNCES = 2, 4
SENTINEL = np.float32(-3.0)     # what a tile or frame holds where nothing may be written
HOLD_MS = 35.0


# ---- streams, holds, oracle frames ------------------------------------------------------------------------------------

class Streams:
    """Three streams of our own: `side` runs the sleeps, A and B take the calls."""

    def __init__(self):
        import torch
        self.side, self.a = torch.cuda.Stream(), torch.cuda.Stream()
        self.cycles = self._calibrate()
        self.b = self._free_stream()

    def _free_stream(self):
        # With more streams in the process than hardware queues, two streams may share a queue, and the work of one then waits behind
        # the other's: a B that shares the side stream's or A's queue would be held too, and hide every race.  Take the first stream
        # of torch's pool whose work runs while A is held.
        import torch
        x = torch.zeros(1, device="cuda")
        for _ in range(8):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                x.add_(1.0)
            torch.cuda.synchronize()
            held = self.hold(self.a)
            with torch.cuda.stream(s):
                x.add_(1.0)
            done = torch.cuda.Event()
            done.record(s)
            while not done.query() and not held.query():
                pass
            free = done.query() and not held.query()
            torch.cuda.synchronize()
            if free:
                return s
        raise AssertionError("no stream of torch's pool runs while A is held")

    def _sleep_ms(self, cycles):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.side)
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(cycles)
        e1.record(self.side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        # _sleep counts a clock nobody has measured on this GPU: grow the count until one sleep takes a few ms, then scale it to
        # HOLD_MS.  Nothing below depends on the exact length, only on a hold outlasting the host work of a few calls.
        self._sleep_ms(1000)
        cycles, ms = 1 << 16, 0.0
        while cycles < (1 << 40):
            ms = self._sleep_ms(cycles)
            if ms >= 4.0:
                break
            cycles *= 4
        assert ms >= 4.0, f"torch.cuda._sleep({cycles}) took {ms} ms"
        return max(1, int(cycles * HOLD_MS / ms))

    def hold(self, stream):
        """Make `stream` wait for a sleep on the side stream; returns the event that ends the hold."""
        import torch
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(self.cycles)
        ev = torch.cuda.Event()
        ev.record(self.side)
        stream.wait_event(ev)
        return ev


@pytest.fixture(scope="module")
def streams():
    return Streams()


@pytest.fixture(scope="module")
def scene():
    return brt.generate_scene(brt.SCENE_COVER, 1)


def _view(seed, w=W, h=H, spp=SPP, level=brt.Raytracing.Pure):
    return brt.cover_camera(w, h, spp, BOUNCES, level, seed)


@functools.lru_cache(maxsize=None)
def _oracle_frame(oracle, seed, w=W, h=H, spp=SPP):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = _view(seed, w, h, spp)
    return oracle.render(b, lvl, cam, win, w, h)


@functools.lru_cache(maxsize=None)
def _oracle_strip_rays(oracle, seed, w=W, h=H, spp=SPP):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = _view(seed, w, h, spp)
    return tuple(oracle.render(b, lvl, cam, win, w, h, rows=(y, min(y + 8, h)))[1]["rays"] for y in range(0, h, 8))


def _shuffled(n_parts, h=H, seed=0):
    strips = (h + 7) // 8
    rng = np.random.default_rng(1000 * seed + n_parts)
    t = np.zeros(strips, np.uint32)
    for g in range(0, strips, n_parts):
        n = min(n_parts, strips - g)
        t[g:g + n] = rng.permutation(n_parts)[:n]
    return t


def _tiles(n_parts, w=W, h=H):
    import torch
    return torch.full((n_parts, brt.tile_rows(h, n_parts), w, 4), float(SENTINEL), dtype=torch.float32, device="cuda")


def _frame(w=W, h=H):
    import torch
    return torch.full((h, w, 4), float(SENTINEL), dtype=torch.float32, device="cuda")


def _check_tile(tile, want, part, n_parts, table, h=H, what=""):
    """The tile holds exactly the rows frame_rows_of_part says; padding rows are never written."""
    fr = frame_rows_of_part(h, part, n_parts, table)
    t = tile.cpu().numpy()
    try:
        assert_frames_equal(t[fr >= 0], want[fr[fr >= 0]])
    except AssertionError as e:
        raise AssertionError(f"{what} part {part}/{n_parts}: {e}") from None
    assert np.all(t[fr < 0].view(np.uint32) == SENTINEL.view(np.uint32)), f"{what} part {part}/{n_parts}: padding rows written"


def _paths(part, n_parts, table, w=W, h=H, spp=SPP):
    return int((frame_rows_of_part(h, part, n_parts, table) >= 0).sum()) * w * spp


def _part_rays(oracle, seed, part, n_parts, table, h=H):
    strips = (h + 7) // 8
    owner = [s % n_parts for s in range(strips)] if table is None else [int(x) for x in table]
    rays = _oracle_strip_rays(oracle, seed, W, h)
    return sum(rays[s] for s in range(strips) if owner[s] == part)


def _render_sync(p, oracle, seed, part, n_parts, table, tile=None, h=H):
    """One part on the context's own stream: synchronous, full stats (rays against the oracle's rays of its strips)."""
    import torch
    if tile is None:
        tile = _tiles(n_parts, h=h)[part]
    torch.cuda.synchronize()                   # (the context's own stream does not wait for torch's)
    lvl, cam, win = _view(seed, W, h)
    st = p.node.render_part_device(lvl, cam, win, W, h, part, n_parts, tile.data_ptr())
    _check_tile(tile, _oracle_frame(oracle, seed, W, h)[0], part, n_parts, table, h, what=f"synchronous (seed {seed})")
    assert st["rays"] == _part_rays(oracle, seed, part, n_parts, table, h)
    assert st["paths"] == _paths(part, n_parts, table, h=h)


def _render_async(p, seed, part, n_parts, table, tile, stream, h=H):
    lvl, cam, win = _view(seed, W, h)
    st = p.node.render_part_device(lvl, cam, win, W, h, part, n_parts, tile.data_ptr(), stream=stream.cuda_stream)
    assert st["paths"] == _paths(part, n_parts, table, h=h)


def _last_error(p):
    msg = _lib.load().brt_last_error(p._ctx)
    return msg.decode() if msg else ""


# ---- 1. the parts of one context on separate streams under a table --------------------------------------------------------

def _parts_in_flight(p, streams, oracle, n_parts, table, order, seed):
    """order[0] on the held stream A, the other parts on B and the side stream in turn, no host sync in between; the assembly on
    the side stream behind every part's stream.  The context's call before was order[0] (synchronous, another seed)."""
    import torch
    _render_sync(p, oracle, seed + 0.5, order[0], n_parts, table)
    tiles, frame = _tiles(n_parts), _frame()
    torch.cuda.synchronize()
    held = streams.hold(streams.a)
    for i, part in enumerate(order):
        s = streams.a if i == 0 else (streams.b, streams.side)[(i - 1) % 2]
        _render_async(p, seed, part, n_parts, table, tiles[part], s)
    for s in (streams.a, streams.b):
        streams.side.wait_stream(s)
    p.node.deinterleave_device(tiles.data_ptr(), n_parts, W, H, frame.data_ptr(), stream=streams.side.cuda_stream)
    pending = not held.query()
    torch.cuda.synchronize()
    want = _oracle_frame(oracle, seed)[0]
    for part in order:
        _check_tile(tiles[part], want, part, n_parts, table, what=f"in flight (order {order[:3]}...)")
    assert_frames_equal(frame.cpu().numpy(), want)
    assert pending, "a call behind the held one waited on the host for it (a host sync on a caller stream)"


@pytest.mark.parametrize("n_parts", [2, 3, 8])
def test_parts_on_separate_streams_under_a_table(streams, scene, oracle, n_parts):
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_strip_table(n_parts, _shuffled(n_parts))
        forward, backward = list(range(n_parts)), list(range(n_parts))[::-1]
        _parts_in_flight(p, streams, oracle, n_parts, _shuffled(n_parts), forward, 0.11)
        _parts_in_flight(p, streams, oracle, n_parts, _shuffled(n_parts), backward, 0.13)
        lvl, cam, win = _view(0.17)
        planned = p.plan_strips(lvl, cam, win, W, H, n_parts, probe_spp=2)
        _parts_in_flight(p, streams, oracle, n_parts, planned, forward, 0.19)
        _parts_in_flight(p, streams, oracle, n_parts, planned, backward, 0.23)


# ---- 2. an assembly while a part p != 0 is in flight -----------------------------------------------------------------------

@pytest.mark.parametrize("n_parts,part", [(3, 1), (3, 2), (8, 5)])
def test_assembly_while_a_part_is_in_flight(streams, scene, oracle, n_parts, part):
    import torch
    table = _shuffled(n_parts, seed=1)
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_strip_table(n_parts, table)
        done = _tiles(n_parts)
        for q in [q for q in range(n_parts) if q != part] + [part]:       # (the context's last call: `part`)
            _render_sync(p, oracle, 0.29, q, n_parts, table, done[q])
        tile, frame = _tiles(n_parts)[part], _frame()
        torch.cuda.synchronize()
        held = streams.hold(streams.a)
        _render_async(p, 0.31, part, n_parts, table, tile, streams.a)
        p.node.deinterleave_device(done.data_ptr(), n_parts, W, H, frame.data_ptr(), stream=streams.b.cuda_stream)
        pending = not held.query()
        torch.cuda.synchronize()
        _check_tile(tile, _oracle_frame(oracle, 0.31)[0], part, n_parts, table, what="held")
        assert_frames_equal(frame.cpu().numpy(), _oracle_frame(oracle, 0.29)[0])
        assert pending, "the assembly waited on the host for the held part"


# ---- 3. a new table while calls under the old one are queued ---------------------------------------------------------------

@pytest.mark.parametrize("held", ["part", "assembly"])
@pytest.mark.parametrize("n_parts", [3, 8])
def test_a_call_uses_the_table_in_force_when_it_is_called(streams, scene, oracle, n_parts, held):
    """Held on A under T1: part 0, or the assembly of a tile set rendered under T1.  Then T2 is installed and part 1 rendered on B,
    then no table and part 2 on B.  Every call must use the table in force when it was called."""
    import torch
    t1, t2 = _shuffled(n_parts, seed=2), _shuffled(n_parts, seed=3)
    assert not np.array_equal(t1, t2)
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_strip_table(n_parts, t1)
        done = _tiles(n_parts)
        for q in list(range(n_parts))[::-1]:                             # (the context's last call: part 0)
            _render_sync(p, oracle, 0.37, q, n_parts, t1, done[q])
        tiles, frame = _tiles(n_parts), _frame()
        torch.cuda.synchronize()
        ev = streams.hold(streams.a)
        if held == "part":
            _render_async(p, 0.41, 0, n_parts, t1, tiles[0], streams.a)
        else:
            p.node.deinterleave_device(done.data_ptr(), n_parts, W, H, frame.data_ptr(), stream=streams.a.cuda_stream)
        p.set_strip_table(n_parts, t2)
        _render_async(p, 0.43, 1, n_parts, t2, tiles[1], streams.b)
        p.set_strip_table(n_parts, None)
        _render_async(p, 0.47, 2, n_parts, None, tiles[2], streams.b)
        pending = not ev.query()
        torch.cuda.synchronize()
        if held == "part":
            _check_tile(tiles[0], _oracle_frame(oracle, 0.41)[0], 0, n_parts, t1, what="held, under T1")
        else:
            assert_frames_equal(frame.cpu().numpy(), _oracle_frame(oracle, 0.37)[0])
        _check_tile(tiles[1], _oracle_frame(oracle, 0.43)[0], 1, n_parts, t2, what="under T2")
        _check_tile(tiles[2], _oracle_frame(oracle, 0.47)[0], 2, n_parts, None, what="no table")
        assert pending, "a call behind the held one waited on the host for it"


# ---- 4. table edge rules ----------------------------------------------------------------------------------------------

def test_a_refused_table_changes_nothing(streams, scene, oracle):
    import torch
    n = 3
    table = _shuffled(n, seed=4)
    dup = table.copy()
    dup[1] = dup[0]
    out_of_range = table.copy()
    out_of_range[4] = n
    refused = [(n, dup), (n, out_of_range), (65, np.arange(19, dtype=np.uint32)),          # (a permutation, but 65 parts)
               (2, np.arange(4097, dtype=np.uint32) % 2), (0, table)]
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_strip_table(n, table)
        for q in range(n):
            _render_sync(p, oracle, 0.53, q, n, table)
        for k, t in refused:
            with pytest.raises(brt.BrtError) as e:
                p.set_strip_table(k, t)
            assert e.value.code == -1 and e.value.text and _last_error(p) == e.value.text, (k, len(t), e.value.text)
        # the table in force is still `table`, for synchronous calls and for calls in flight alike
        for q in range(n):
            _render_sync(p, oracle, 0.59, q, n, table)
        tiles, frame = _tiles(n), _frame()
        torch.cuda.synchronize()
        streams.hold(streams.a)
        for q in range(n):
            _render_async(p, 0.61, q, n, table, tiles[q], (streams.a, streams.b)[q % 2])
        streams.b.wait_stream(streams.a)
        p.node.deinterleave_device(tiles.data_ptr(), n, W, H, frame.data_ptr(), stream=streams.b.cuda_stream)
        torch.cuda.synchronize()
        want = _oracle_frame(oracle, 0.61)[0]
        for q in range(n):
            _check_tile(tiles[q], want, q, n, table, what="after the refusals")
        assert_frames_equal(frame.cpu().numpy(), want)


def test_frames_the_table_does_not_fit_go_by_s_mod_n(streams, scene, oracle):
    """A table for 149 rows in 3 parts: frames of 141 rows, or of 2 parts, render and assemble by s % n_parts; frames it fits keep
    using it, in flight beside them; None brings s % n_parts back."""
    import torch
    table = _shuffled(3, seed=5)
    h2 = 141                                                                 # 18 strips
    cases = [(0.67, H, 3, table), (0.71, H, 2, None), (0.73, h2, 3, None), (0.79, H, 3, table)]
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_strip_table(3, table)
        for seed, h, n, t in cases:
            for q in range(n):
                _render_sync(p, oracle, seed, q, n, t, h=h)
        sets = [(seed, h, n, t, _tiles(n, h=h), _frame(h=h)) for seed, h, n, t in cases]
        torch.cuda.synchronize()
        held = streams.hold(streams.a)
        k = 0
        for seed, h, n, t, tiles, frame in sets:
            for q in range(n):
                _render_async(p, seed + 0.001, q, n, t, tiles[q], (streams.a, streams.b)[k % 2], h=h)
                k += 1
            streams.b.wait_stream(streams.a)
            p.node.deinterleave_device(tiles.data_ptr(), n, W, h, frame.data_ptr(), stream=streams.b.cuda_stream)
        pending = not held.query()
        torch.cuda.synchronize()
        for seed, h, n, t, tiles, frame in sets:
            want = _oracle_frame(oracle, seed + 0.001, W, h)[0]
            for q in range(n):
                _check_tile(tiles[q], want, q, n, t, h=h, what=f"{h} rows in {n} parts")
            assert_frames_equal(frame.cpu().numpy(), want)
        assert pending, "a call behind the held one waited on the host for it"
        p.set_strip_table(3, None)
        for q in range(3):
            _render_sync(p, oracle, 0.83, q, 3, None)


# ---- 5. the ev_last chain without a table ---------------------------------------------------------------------------------

def test_frames_on_alternating_streams_behind_half_sample_jobs(streams, scene, oracle):
    """A context whose order holds half-sample jobs (the shared pixel-state buffer and its serial in play): six frames on A (held
    anew each time) and B in turn, each into its own tile."""
    import torch
    w, h, spp = W, H, 4
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        p.set_tuning("BRT_SPLIT_FORCE", 40)
        for seed in (0.89, 0.97):
            lvl, cam, win = _view(seed, w, h, spp)
            tile = _tiles(1)[0]
            st = p.node.render_part_device(lvl, cam, win, w, h, 0, 1, tile.data_ptr(), flags=brt.FLAG_COUNTERS)
            want, cnt = _oracle_frame(oracle, seed, w, h, spp)
            _check_tile(tile, want, 0, 1, None, what="synchronous")
            assert {k: st[k] for k in COUNTER_KEYS} == cnt
        p.debug_profile()
        assert p.last_order_meta["split_tiles"] > 0
        tiles = torch.cat([_tiles(1) for _ in range(6)])
        torch.cuda.synchronize()
        seeds = [1.03 + 0.07 * i for i in range(6)]
        for i, seed in enumerate(seeds):
            s = streams.b if i % 2 else streams.a
            if s is streams.a:
                held = streams.hold(s)
            lvl, cam, win = _view(seed, w, h, spp)
            p.node.render_part_device(lvl, cam, win, w, h, 0, 1, tiles[i].data_ptr(), stream=s.cuda_stream)
        pending = not held.query()
        torch.cuda.synchronize()
        for i, seed in enumerate(seeds):
            _check_tile(tiles[i], _oracle_frame(oracle, seed, w, h, spp)[0], 0, 1, None, what=f"frame {i}")
        assert pending


def test_a_synchronous_frame_behind_a_held_one_grows_the_buffers(streams, scene, oracle):
    """A held frame, then a synchronous frame of another view at a larger size (the order, cost and tile buffers grow while the
    held frame still needs the old ones), then the held view again."""
    import torch
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(scene)
        _render_sync(p, oracle, 1.51, 0, 1, None)
        t1, t2 = _tiles(1)[0], _tiles(1)[0]
        torch.cuda.synchronize()
        streams.hold(streams.a)
        _render_async(p, 1.53, 0, 1, None, t1, streams.a)
        w2, h2 = 512, 301
        lvl, cam, win = brt.cover_camera(w2, h2, SPP, BOUNCES, brt.Raytracing.Pure, 1.57)
        got = p.node.run(lvl, cam, win, w2, h2, flags=brt.FLAG_COUNTERS)
        want2, cnt2 = oracle.render(scene, lvl, cam, win, w2, h2)
        assert_frames_equal(got, want2)
        assert {k: p.node.last_stats[k] for k in COUNTER_KEYS} == cnt2
        _render_async(p, 1.59, 0, 1, None, t2, streams.b)
        torch.cuda.synchronize()
        _check_tile(t1, _oracle_frame(oracle, 1.53)[0], 0, 1, None, what="held")
        _check_tile(t2, _oracle_frame(oracle, 1.59)[0], 0, 1, None, what="after the larger frame")


def test_render_device_on_alternating_streams_with_device_raster_inputs(streams, scene, oracle):
    """brt_render_device on a [0, 0, 0] context at level 2 with raster inputs on the device: frames on A (held) and B in turn."""
    import torch
    rng = np.random.default_rng(11)
    raster = rng.random((H, W, 4), dtype=np.float32)
    depth = (rng.random((H, W), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    with brt.RaytracePlugin([0, 0, 0]) as p:
        p.node.write_buffers(scene)
        d_raster, d_depth = torch.from_numpy(raster).cuda(), torch.from_numpy(depth).cuda()
        frames = [_frame() for _ in range(4)]
        seeds = [1.61 + 0.05 * i for i in range(4)]
        torch.cuda.synchronize()
        for i, seed in enumerate(seeds):
            s = streams.b if i % 2 else streams.a
            if s is streams.a:
                streams.hold(s)
            lvl, cam, win = _view(seed, level=brt.Raytracing.FallbackRaytraced)
            p.node.render_device(lvl, cam, win, W, H, frames[i].data_ptr(), d_raster.data_ptr(), d_depth.data_ptr(),
                                 stream=s.cuda_stream)
        torch.cuda.synchronize()
        for i, seed in enumerate(seeds):
            lvl, cam, win = _view(seed, level=brt.Raytracing.FallbackRaytraced)
            want, _ = oracle.render(scene, lvl, cam, win, W, H, raster_rgba=raster, raster_depth=depth)
            assert_frames_equal(frames[i].cpu().numpy(), want)
