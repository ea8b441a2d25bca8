"""The hand-written loops of brt_device.h (walk_wave_lds_asm, walk_wave_top_asm, walk_rows_asm, ball_loop_asm) by their own step counts,
and row mode and the steady-state instantiation reached on purpose.

The shipped build says nothing about which loop ran or how many steps it took, so the cases of tests/hand_loops_cases.py are rendered
twice.  Once in a -DBRT_ASM_COUNT build (made here, once per run, with the Makefile's own variables) by a child process
(tests/tools/hand_loops_child.py; the session's plugin has the shipped library loaded, and bevyray_amd/_lib.py reads BRT_LIB_PATH once):
there the loops count their executions and active lanes, and

  * the lanes of the interior steps, plus those of the compiler's repairing loop, are the oracle's interior_visits; likewise the leaf
    steps and its sphere_tests -- a hand-written step that descends into a box it should have culled, or tests a sphere twice, leaves the
    pixels alone and breaks this;
  * the lanes of the sampler loop are those of the FLAG_COUNTERS frame of the same build, i.e. of the compiler-built sampler loop (the
    oracle does not count sampler iterations, so this one identity has no CPU side);
  * rows_calls, rows_interior_exec, repairing_loop_lanes, kernel_variant and scene_in_lds prove that a case reached the loop and the
    instantiation it is meant for.

Lane counts do not depend on which rays share a wave and are asserted at every frame size; execution counts do, and are asserted only
for the one-tile frames whose schedule is fixed by construction.  Then the row-mode cases and the large views are rendered in the
shipped library, where frame and ray count must equal the oracle's; nothing is asserted there about a case the counting build did not
prove.  Every comparison is an equality.

The module's first run failed the interior identity in every LDS-resident knobs-live launch: the repairing loop's lane counter came back
with float bit patterns added.  walk_rows_asm widens EXEC, it was called under the kernel's divergent `if (active)`, and in that
instantiation the compiler kept the parked lanes' counter in a register it had also given to the loop's temporaries.  The kernel now
calls walk_run with the whole wave wherever row mode exists (brt_trace.h, kRowsHere)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hand_loops_cases as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM_LIB = os.path.join(ROOT, "ab", "libasmcount.so")
# A from-scratch build of the variant takes 25 s wall at -j16 on a CPU-only machine (2 min 38 s of CPU); the limit is ten times that.
# (The first from-scratch build on the MI355X machine, at -j16 on its 16 CPUs, took 7 s.)
BUILD_LIMIT_S = 250
# The child's first run on an MI355X took 3 s (fixture set-up 2.8 s with a no-op make); the limit is ten times that, and at least 60 s.
CHILD_LIMIT_S = 60


def _assert_frame(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"


# ---- CPU: the placement of R3 (b) - (d) is a checked claim ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(hl.CHAIN_PIXELS))
def test_chain_is_seen_by_its_pixels_only(oracle, name):
    """The 8 x 8 frame with the chain differs from the frame of the same view without it in exactly the pixels the chain was laid
    through -- lane 63, lane 0, or both, of the tile's wave -- and each of them hit it."""
    pixels = hl.CHAIN_PIXELS[name]
    b, lvl, cam, win, w, h, _ = hl.chain_pixels_case(pixels)
    with_chain, cnt = oracle.render(b, lvl, cam, win, w, h)
    b0, lvl, cam, win, w, h, _ = hl.chain_pixels_case(pixels, with_chain=False)
    without, cnt0 = oracle.render(b0, lvl, cam, win, w, h)
    differ = (with_chain.view(np.uint32) != without.view(np.uint32)).any(axis=-1)
    assert sorted((int(x), int(y)) for y, x in np.argwhere(differ)) == sorted(pixels)
    assert cnt0["rays"] == w * h * hl.CHAIN_SPP and cnt0["hits"] == 0           # without the chain: sky
    assert cnt["hits"] >= len(pixels) and cnt["rays"] > cnt0["rays"]


# ---- the counting build and its child process ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def counting_lib():
    """ab/libasmcount.so, as scripts/build_variant.sh builds it; the object directory stays, so a second run is a no-op make."""
    os.makedirs(os.path.dirname(ASM_LIB), exist_ok=True)
    proc = subprocess.run(["make", "-C", os.path.join(ROOT, "bevyray_amd", "csrc"), "-j8", "EXTRA=-DBRT_ASM_COUNT=1", "BUILD=build_asmcount",
                           f"OUT={ASM_LIB}"], capture_output=True, text=True, timeout=BUILD_LIMIT_S)
    assert proc.returncode == 0, proc.stdout[-4000:] + proc.stderr[-4000:]
    return ASM_LIB


@pytest.fixture(scope="module")
def child(counting_lib, tmp_path_factory):
    """Everything the child saw: records (dict), frames (npz), dir.  Raises if the child ends by a signal, a non-zero status or its time
    limit, so that nothing else of this module starts on the GPU."""
    out = tmp_path_factory.mktemp("hand_loops")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "hand_loops_child.py"), str(out)],
                          env={**os.environ, "BRT_LIB_PATH": counting_lib}, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    if proc.returncode != 0:
        raise RuntimeError(f"hand_loops_child.py ended with status {proc.returncode}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")
    with open(out / "records.json") as f:
        records = json.load(f)
    assert records["lib"] == counting_lib
    return {"records": records, "frames": np.load(out / "frames.npz"), "dir": out}


_WANT = {}


def _want(oracle, name, make):
    """The oracle's frame and counters of a case, computed once: (case, frame, counters)."""
    if name not in _WANT:
        case = make()
        b, lvl, cam, win, w, h, _ = case
        frame, cnt = oracle.render(b, lvl, cam, win, w, h)
        _WANT[name] = (case, np.asarray(frame, np.float32), cnt)
    return _WANT[name]


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _want_large(oracle, name):
    w, h = hl.large_size(_n_cus())
    return _want(oracle, name, lambda: hl.LARGE[name][0](w, h))


def _assert_identities(rec, frame, want, cnt, what):
    """Section 2 of the module docstring for one production launch of the counting build."""
    asm, st = rec["asm"], rec["stats"]
    _assert_frame(frame, want, what)
    assert st["rays"] == cnt["rays"], (what, st["rays"], cnt["rays"])
    fix_i, fix_l = asm["repairing_loop_lanes"]
    assert asm["interior"][1] + fix_i == cnt["interior_visits"], (what, asm, cnt)
    assert asm["leaf"][1] + fix_l == cnt["sphere_tests"], (what, asm, cnt)
    # (the counting frame is the same build's COUNTERS instantiation: its own counters are the oracle's too)
    assert rec["counting"]["rays"] == cnt["rays"], (what, rec["counting"], cnt)
    assert asm["ball"][1] == rec["profile"]["ball"][1], (what, asm, rec["profile"])


# ---- lane-step identities ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(hl.MODES))
@pytest.mark.parametrize("name", list(hl.SMALL))
def test_lane_steps_equal_the_oracles_counters(child, oracle, name, mode):
    """Frames 0 and 1 of the view, production (kernel_variant 0 .. 2) and knobs-live (bit 4): the frame, the rays, the interior and leaf
    lane steps against the oracle on the caller's tree that both walk, the sampler's lane steps against the counting frame."""
    case, want, cnt = _want(oracle, name, hl.SMALL[name])
    for frame in range(hl.SMALL_FRAMES):
        key = f"{name}/{mode}/{frame}"
        rec = child["records"][key]
        variant = rec["stats"]["kernel_variant"]
        assert (variant & 16) if mode == "knobs_live" else variant in (0, 1, 2), (key, variant)
        if "BRT_FORCE_LDS_TOP" in case[6]:
            assert rec["stats"]["scene_in_lds"] == 2, key
        _assert_identities(rec, child["frames"][key], want, cnt, key)


def test_the_half_sample_case_has_enough_samples():
    """(CPU) the kernel runs half-sample jobs only from 16 samples on (brt_trace.h `slices`): the case keeps that many."""
    for make in hl.HALF.values():
        assert int(make()[2]["sample_count"][0]) >= 16


@pytest.mark.gpu
def test_forced_half_sample_jobs_ran(child):
    """The second production frame of the forced case handed tiles out as two half-sample jobs: second-half lanes took pixels over or
    left them to their first-half lanes (the kernel's own tally); its lane steps are held to the oracle's like every case's."""
    (name, _), = hl.HALF_FORCED.items()
    order = child["records"][f"{name}/production/1"]["order"]
    assert order["second_halves_taken"] + order["second_halves_left"] > 0, order


# ---- row mode ----------------------------------------------------------------------------------------------------------------------------------

def _assert_reach(child, oracle, name):
    """The evidence of the counting build that case `name` reaches the loop it is meant for, in both modes and both frames."""
    for mode in hl.MODES:
        for frame in range(hl.SMALL_FRAMES):
            key = f"{name}/{mode}/{frame}"
            rec = child["records"][key]
            asm, st = rec["asm"], rec["stats"]
            assert st["scene_in_lds"] == 1 and st["kernel_variant"] & 3 != 2, (key, st)           # row mode exists there (LEAN 0 / 1, knobs-live)
            if name in hl.R1:         # every walk in row mode, no unsafe ray
                assert tuple(asm["repairing_loop_lanes"]) == (0, 0), (key, asm)
                assert asm["rows_calls"] > 0 and asm["rows_interior_exec"] == asm["interior"][0] > 0, (key, asm)
            elif name in hl.R2 or name in hl.R3:      # the wide loop hands its last walks over
                assert asm["rows_calls"] > 0 and 0 < asm["rows_interior_exec"] < asm["interior"][0], (key, asm)
            elif name in hl.R4:
                # walk_run, one lane walking (exit_at = 0): the camera ray is unsafe, so the compiler's repairing loop walks it to its
                # end and the wide loop returns at its first test with no step taken; a bounce is safe and alone: one row-mode call
                # that walks it to its end.  So the repairing loop's lanes are the steps of the camera rays -- the oracle's counters
                # of the same view without bounces --, the row-mode calls are the other rays, and the hand-written interior steps are
                # all row-mode steps.
                b, lvl, cam, win, w, h, _ = hl.SMALL[name]()
                cam0 = cam.copy()
                cam0["bounce_count"] = 0
                _, cam_cnt = oracle.render(b, lvl, cam0, win, w, h)
                assert cam_cnt["rays"] == hl.R4_SPP and cam_cnt["interior_visits"] > 0
                assert tuple(asm["repairing_loop_lanes"]) == (cam_cnt["interior_visits"], cam_cnt["sphere_tests"]), (key, asm, cam_cnt)
                assert asm["rows_calls"] == st["rays"] - hl.R4_SPP > 0, (key, asm, st["rays"])
                assert asm["rows_interior_exec"] == asm["interior"][0] > 0, (key, asm)
            else:
                raise AssertionError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hl.ROW_CASES))
def test_counting_build_proves_the_case_reaches_row_mode(child, oracle, name):
    _assert_reach(child, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hl.ROW_CASES))
def test_row_mode_in_the_shipped_build_matches_the_oracle(plugin, child, oracle, name):
    """The same case in the shipped library, in which walk_rows_asm leaves no trace of its own: two production frames and a knobs-live
    one, frame and rays against the oracle.  Only for what the counting build proved."""
    _assert_reach(child, oracle, name)
    (b, lvl, cam, win, w, h, knobs), want, cnt = _want(oracle, name, hl.SMALL[name])
    for mode, extra in hl.MODES.items():
        with plugin.tuning(**knobs, **extra):
            for frame in range(hl.SMALL_FRAMES):
                got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
                st = dict(plugin.node.last_stats)
                key = f"{name}/{mode}/{frame}"
                # (the launch the counting build proved: same instantiation, same residency)
                proved = child["records"][key]["stats"]
                assert (st["kernel_variant"], st["scene_in_lds"], st["lds_bytes"]) == \
                       (proved["kernel_variant"], proved["scene_in_lds"], proved["lds_bytes"]), (key, st, proved)
                assert st["rays"] == cnt["rays"], (key, st["rays"], cnt["rays"])
                _assert_frame(got, want, key)


# ---- no row scratch ------------------------------------------------------------------------------------------------------------------------------

def _assert_scratch_window(child):
    """At R5_N spheres the {1024, 1} launch keeps the scene in LDS and gives the row scratch up -- a 2 x 1 frame, which walks in rows
    wherever it can, makes no row-mode call --; 100 spheres earlier it has the scratch and walks in rows.  A layout change that moves
    the window fails here."""
    for mode in hl.MODES:
        for frame in range(hl.SMALL_FRAMES):
            without, with_ = (child["records"][f"{name}/{mode}/{frame}"] for name in ("r5_no_scratch", "r5_with_scratch"))
            for rec in (without, with_):
                assert rec["stats"]["scene_in_lds"] == 1 and rec["stats"]["threads_per_workgroup"] == 1024, rec["stats"]
                assert tuple(rec["asm"]["repairing_loop_lanes"]) == (0, 0), rec["asm"]
            assert without["asm"]["rows_calls"] == 0 and without["asm"]["rows_interior_exec"] == 0, (mode, frame, without["asm"])
            assert with_["asm"]["rows_calls"] > 0 and with_["asm"]["rows_interior_exec"] == with_["asm"]["interior"][0] > 0, (mode, frame, with_["asm"])
            # (100 spheres are 12 800 bytes, the scratch 5 120: the smaller scene's launch is larger only by what the scratch adds back)
            assert without["stats"]["lds_bytes"] - with_["stats"]["lds_bytes"] < 100 * 128, (without["stats"], with_["stats"])


@pytest.mark.gpu
def test_counting_build_proves_the_scratch_window(child):
    _assert_scratch_window(child)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hl.R5))
def test_launches_around_the_scratch_window_match_the_oracle(plugin, child, oracle, name):
    """The two scenes in the shipped library under the same knobs: frame and rays against the oracle, the launch the one that was proved."""
    _assert_scratch_window(child)
    (b, lvl, cam, win, w, h, knobs), want, cnt = _want(oracle, name, hl.SMALL[name])
    for mode, extra in hl.MODES.items():
        with plugin.tuning(**knobs, **extra):
            for frame in range(hl.SMALL_FRAMES):
                got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
                st = dict(plugin.node.last_stats)
                key = f"{name}/{mode}/{frame}"
                proved = child["records"][key]["stats"]
                assert (st["kernel_variant"], st["scene_in_lds"], st["lds_bytes"]) == \
                       (proved["kernel_variant"], proved["scene_in_lds"], proved["lds_bytes"]), (key, st, proved)
                assert st["rays"] == cnt["rays"], (key, st["rays"], cnt["rays"])
                _assert_frame(got, want, key)


# ---- the steady-state instantiation on scenes other than the cover scene ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hl.LARGE))
def test_steady_state_instantiation_on_other_scenes(plugin, child, oracle, name):
    """1 spp, 4 bounces, a frame of 2 * (bounces + 2) pixels per lane of the GPU: three frames of the view in the shipped library, each
    with its rays against the oracle, the third in LEAN 2 with the expected residency; and the third frame of the counting build: the
    lane-step identities, and no row-mode call (LEAN 2 compiles row mode out)."""
    (b, lvl, cam, win, w, h, knobs), want, cnt = _want_large(oracle, name)
    assert w * h >= 2 * (hl.LARGE_BOUNCES + 2) * _n_cus() * 1024
    residency = hl.LARGE[name][1]
    with plugin.tuning(**knobs):
        for frame in range(hl.LARGE_FRAMES):
            got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
            st = dict(plugin.node.last_stats)
            assert st["rays"] == cnt["rays"], (name, frame, st["rays"], cnt["rays"])
            assert st["scene_in_lds"] == residency, (name, frame, st["scene_in_lds"])
            _assert_frame(got, want, f"{name} frame {frame} variant {st['kernel_variant']}")
    assert st["kernel_variant"] == 2, st["kernel_variant"]
    key = f"{name}/production/{hl.LARGE_FRAMES - 1}"
    rec = child["records"][key]
    assert rec["stats"]["kernel_variant"] == 2 and rec["stats"]["scene_in_lds"] == residency, (key, rec["stats"])
    assert rec["asm"]["rows_calls"] == 0 and rec["asm"]["rows_interior_exec"] == 0, (key, rec["asm"])
    _assert_identities(rec, np.load(child["dir"] / f"{name}.npy"), want, cnt, key)
