"""The selecting kernel of progressive frames (k_prog_select, brt_progressive_select_device) on synthetic state planes
(tests/progressive_ref.py): ten frame sizes around its 16-pixel tile, each plane with selected and unselected pixels and waves of 0, 1
and 64 selected lanes (asserted on the CPU first), at five (threshold, radius) pairs -- the mask, the count and the list as a set are exact
against the restatement, which tests/test_progressive.py holds bitwise to the host twin --; the special board; and a plane the GPU
produced.  The mask-only instantiation writes the same mask and touches neither list nor count."""
import numpy as np
import pytest

import bevyray_amd as brt
import progressive_ref as pr

TARGET = 16
PAIRS = ((0.1, 1), (0.1, 0), (0.02, 1), (0.4, 1), (0.4, 0))      # (threshold, radius)


def _planes():
    return [(w, h, pr.synthetic_plane(w, h, k, TARGET)) for k, (w, h) in enumerate(pr.SIZES)]


def test_every_synthetic_plane_is_non_vacuous():
    for w, h, plane in _planes():
        for thr, radius in PAIRS:
            cls = pr.classes(plane, TARGET, thr, radius)
            assert cls.any() and not cls.all(), (w, h, thr, radius)
            if thr == 0.1:      # (the threshold the planes are crafted for: waves of 0, 1 and 64 selected lanes)
                assert pr.non_vacuous(cls), (w, h, radius, pr.wave_counts(cls))
    board = pr.special_board(TARGET)
    assert pr.classes(board, TARGET, 0.1, 1).any() and not pr.classes(board, TARGET, 0.1, 1).all()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _select(plugin, w, h, d_state, target, with_list=True, with_mask=True):
    import torch
    d_list = torch.full((w * h + 16,), 0xCDCDCDCD - (1 << 32), dtype=torch.int32, device="cuda")
    d_count = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    d_mask = torch.full((w * h + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plugin.node.progressive_select_device(w, h, d_state.data_ptr(), target, d_list.data_ptr() if with_list else 0,
                                          d_count.data_ptr() if with_list else 0, d_mask.data_ptr() if with_mask else 0)
    torch.cuda.synchronize()
    return d_list.cpu().numpy().view(np.uint32), d_count.cpu().numpy().view(np.uint32), d_mask.cpu().numpy()


def _check(plugin, w, h, plane, target, thr, radius, where):
    want = pr.classes(plane, target, thr, radius)
    d_state = _dev(plane)
    lst, cnt, msk = _select(plugin, w, h, d_state, target)
    n = int(cnt[0])
    assert n == int((want != 0).sum()) and (cnt[1:] == 77).all(), where
    assert np.array_equal(msk[:w * h].reshape(h, w), want) and (msk[w * h:] == 0xCD).all(), where
    assert np.array_equal(np.sort(lst[:n]), np.flatnonzero(want.reshape(-1))) and (lst[n:] == 0xCDCDCDCD).all(), where
    # the mask-only instantiation, and the list without a mask
    lst2, cnt2, msk2 = _select(plugin, w, h, d_state, target, with_list=False)
    assert np.array_equal(msk2, msk) and (lst2 == 0xCDCDCDCD).all() and (cnt2 == 77).all(), where
    lst3, cnt3, msk3 = _select(plugin, w, h, d_state, target, with_mask=False)
    assert int(cnt3[0]) == n and np.array_equal(np.sort(lst3[:n]), np.sort(lst[:n])) and (msk3 == 0xCD).all(), where
    assert d_state.cpu().numpy().tobytes() == plane.tobytes(), where                # the state is read only


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(pr.SIZES)), ids=["%dx%d" % s for s in pr.SIZES])
def test_select_on_synthetic_planes(plugin, k):
    w, h = pr.SIZES[k]
    plane = pr.synthetic_plane(w, h, k, TARGET)
    try:
        for thr, radius in PAIRS:
            plugin.set_progressive(8, 64, thr, radius)
            _check(plugin, w, h, plane, TARGET, thr, radius, (w, h, thr, radius))
        plugin.set_progressive(8, 64, 0.1, 1)
        for target in (1, 2, 15, 17, 65535):
            _check(plugin, w, h, plane, target, 0.1, 1, (w, h, "target", target))
    finally:
        plugin.set_progressive()


@pytest.mark.gpu
def test_select_on_the_special_board_and_tiny_frames(plugin):
    board = pr.special_board(TARGET)
    h, w = board.shape
    try:
        for thr, radius in PAIRS:
            plugin.set_progressive(8, 64, thr, radius)
            _check(plugin, w, h, board, TARGET, thr, radius, ("board", thr, radius))
            for tw, th in ((1, 1), (1, 5), (5, 1), (2, 2)):
                _check(plugin, tw, th, np.ascontiguousarray(board[3:3 + th, 4:4 + tw]), TARGET, thr, radius, ("tiny", tw, th, thr, radius))
    finally:
        plugin.set_progressive()


@pytest.mark.gpu
def test_select_on_a_plane_the_gpu_produced(plugin):
    import torch
    w, h = 64, 40
    plugin.node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    lvl, cam, win = brt.cover_camera(w, h, 1, 4)
    d_state = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plugin.node.progressive_sample_device(cam, win, w, h, d_state.data_ptr(), 8)
    half = np.random.default_rng(1).permutation(w * h)[:w * h // 2].astype(np.uint32)
    plugin.node.progressive_sample_device(cam, win, w, h, d_state.data_ptr(), 16, _dev(half).data_ptr(), half.size)
    torch.cuda.synchronize()
    plane = d_state.cpu().numpy().view(pr.REC).reshape(h, w).copy()
    assert sorted(np.unique(plane["n"])) == [8, 16]
    try:
        for thr, radius in PAIRS:
            plugin.set_progressive(8, 64, thr, radius)
            want = pr.classes(plane, 16, thr, radius)
            if thr == 0.1:
                assert want.any() and not want.all()
            _check(plugin, w, h, plane, 16, thr, radius, ("gpu plane", thr, radius))
            _check(plugin, w, h, plane, 32, thr, radius, ("gpu plane", 32, thr, radius))
    finally:
        plugin.set_progressive()
