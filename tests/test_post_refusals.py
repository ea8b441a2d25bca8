"""The refusals of the twelve device entry points on a whole frame behind the tracer -- post-passes, upsampling, adaptive sampling -- are
what they were before the entry points were folded onto one skeleton (brt_frame.h frame_call): the return code and the brt_last_error
text of every case of tests/post_refusal_cases.py, among them every pair of adjacent checks violated together (which pins the ORDER of
the checks), against tests/golden/post_refusals.json (scripts/record_post_refusals.py, on the commit before the fold).  The suites of
the families (test_denoise.py, test_temporal.py, test_blend_post.py, test_upscale*.py, test_adaptive.py) assert the codes of single
faults; this module adds the texts and the order.  Nothing is launched: the GPU test takes about a second."""
import json
import os

import pytest

import post_refusal_cases as prc
from bevyray_amd import _lib
from helpers import GOLDEN

TWELVE = ("brt_denoise_device", "brt_blend_post_device", "brt_upscale_device", "brt_upscale_blend_device", "brt_render_upscaled_device",
          "brt_render_upscaled_blend_device", "brt_upscale_refine_device", "brt_render_upscaled_refined_device",
          "brt_upscale_refine_mask_device", "brt_render_adaptive_device", "brt_adaptive_refine_device", "brt_adaptive_mask_device")


def _golden():
    with open(os.path.join(GOLDEN, "post_refusals.json")) as f:
        return prc.unpack(json.load(f))


def test_the_table_covers_the_twelve_exports_and_their_pairs():
    cases = prc.cases()
    assert set(prc.EXPORTS) == set(TWELVE) <= set(_lib.EXPORTS)
    for export in TWELVE:
        mine = [c for c in cases if c["export"] == export]
        assert sum(1 for c in mine if c["faults"] == 1) >= 10 and sum(1 for c in mine if c["faults"] == 2) >= 1, export
        n_checks = len(prc.TABLE[export]["checks"])
        assert sum(1 for c in mine if c["faults"] == 2) == n_checks - 1            # every pair of adjacent checks
        assert all(len(c["args"]) == len(_lib._PROTOTYPES[export][1]) for c in mine), export
        # every bit the export does not allow is a case of its own
        flags = [c for c in mine if c["faults"] == 1 and ":flag_bit" in c["id"]]
        assert 24 <= len(flags) <= 31 and all(bin(c["args"][[k for k, _ in prc.TABLE[export]["base"]].index("flags")]).count("1") == 1 for c in flags)
    # the arena's regions are disjoint, so that only a case that says so overlaps
    spans = sorted(prc.ARENA.values())
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= prc.ARENA_BYTES


def test_the_recorded_answers_are_refusals_of_exactly_the_table():
    golden = _golden()
    assert set(golden) == {c["id"] for c in prc.cases()}
    for cid, (rc, text) in golden.items():
        assert rc != 0 and text, cid
    # a case without a context leaves its text where a caller without a context reads it
    assert all(golden[c["id"]] == [-1, "ctx is null"] for c in prc.cases() if c["states"] == ["null"])


@pytest.mark.gpu
def test_every_refusal_is_what_it_was():
    golden, got = _golden(), prc.run_on_gpu()
    assert set(got) == set(golden)
    wrong = {cid: (got[cid], golden[cid]) for cid in golden if got[cid] != golden[cid]}
    assert not wrong, wrong
