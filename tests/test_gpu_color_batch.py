"""Colour (BGR) batches on the device: omr_batch_run_device_cn / omr_batch_deskew_device_cn.

The sweep of a BGR scan gives the winners and the f64 scores, bit for bit, that the 1-channel entry points give for
cvtColor(COLOR_RGB2GRAY) of it (quirk B8: BGR bytes through RGB weights) -- on the run-merging path and on the scan-lane
path -- without writing a gray image; the colour deskew of scan i is bit for bit omr_rotate (3 channels, CONTAIN) by
its detected angle: the oracle's rotate_mat exactly for NEAREST and within one level per channel for LINEAR.
synth.make_color_card's inks are classified the opposite way by true BGR weights, so a kernel that gets the channel
order wrong cannot pass (tests/test_color_batch_abi.py pins that property of the card)."""
import ctypes as C

import numpy as np
import pytest

import oics
from oics import projection, synth, transfer
from oics.types import RotateClipStrategy

pytestmark = pytest.mark.gpu

NEAREST, LINEAR = 0, 1
WHITE = (255, 255, 255)


def _dev():
    import torch
    return torch, torch.device("cuda:0")


def _cards(rows, cols, n, seed0, skews=None):
    out, th = [], []
    for i in range(n):
        img, t = synth.make_color_card(rows, cols, seed0 + i, skew=None if skews is None else skews[i])
        out.append(img)
        th.append(t)
    return np.stack(out), th


def _gray(oracle, cards):
    return np.stack([oracle.rgb2gray(c) for c in cards])


def _sweep_both(b, cards, gray, black_max=127):
    """(best, v_sd, h_sd) of the colour entry point on `cards` and of omr_batch_run_device on `gray`"""
    torch, dev = _dev()
    n, rows, cols = gray.shape
    A = b.A
    res = []
    for imgs, cn in ((cards, 3), (gray, 1)):
        d = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
        best = torch.full((n,), -1, dtype=torch.int32, device=dev)
        vs = torch.zeros((n, A), dtype=torch.float64, device=dev)
        hs = torch.zeros((n, A), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()  # (the batch's streams do not wait for torch's)
        if cn == 3:
            b.run_device_cn(d.data_ptr(), rows * cols * 3, cols * 3, 3, n, black_max, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        else:
            b.run_device(d.data_ptr(), rows * cols, cols, n, black_max, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        b.sync()
        res.append((best.cpu().numpy(), vs.cpu().numpy(), hs.cpu().numpy()))
        del d
    return res


def _check_sweep(oracle, res, gray, theta, max_angle, step, sample):
    (cb, cv, ch), (gb, gv, gh) = res
    assert (cb == gb).all(), np.nonzero(cb != gb)
    assert (cv.view(np.uint64) == gv.view(np.uint64)).all() and (ch.view(np.uint64) == gh.view(np.uint64)).all()
    N = len(cv[0]) // 2
    for i in range(len(cb)):
        assert abs((int(cb[i]) - N) * step - theta[i]) <= step + 1e-9, (i, cb[i], theta[i])
    for i in sample:
        _, _, evs, ehs = oracle.sweep(oracle.threshold_binary(gray[i]), max_angle, step, want_proj=False)
        assert (cv[i].view(np.uint64) == evs.view(np.uint64)).all() and (ch[i].view(np.uint64) == ehs.view(np.uint64)).all(), i
        assert cb[i] == oracle.argmax_path1(evs, ehs)[0], i


@pytest.mark.parametrize("cols", [452, 453])
def test_run_merging_sweep_colour_equals_gray(oracle, cols):
    rows, max_angle, step = 640, 10, 0.5
    skews = [-9.3, -4.0, -0.2, 0.0, 0.7, 3.1, 6.6, 9.4, 2.2, -7.5, 5.0]  # 11 scans: a last group of 3 at group = 4
    cards, theta = _cards(rows, cols, len(skews), 300, skews)
    gray = _gray(oracle, cards)
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=2)
    b.set_group(4)
    assert b.info()[0] > 0, "the run-merging kernel must sweep candidates here"
    res = _sweep_both(b, cards, gray)
    b.close()
    _check_sweep(oracle, res, gray, theta, max_angle, step, (0, 5, 10))


def test_scan_lane_sweep_colour_equals_gray(oracle):
    rows, cols, max_angle, step, n = 1000, 708, 10, 0.5, 130
    rng = np.random.default_rng(5)
    skews = [float(v) for v in rng.uniform(-9.4, 9.4, n)]
    cards, theta = _cards(rows, cols, n, 900, skews)
    gray = _gray(oracle, cards)
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=2)
    b.set_lanes(128)  # two launches: 128 scans, then 2
    res = _sweep_both(b, cards, gray)
    b.close()
    _check_sweep(oracle, res, gray, theta, max_angle, step, (0, 77, 129))


def _deskew_cn(b, imgs, cn, interp, border, black_max=127, sentinel=7):
    """(out [n, DR, DC * cn], size [n, 2], best [n]) of omr_batch_deskew_device_cn"""
    torch, dev = _dev()
    n, rows, cols = imgs.shape[:3]
    dr, dc = b.deskew_canvas()
    d = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
    out = torch.full((n, dr, dc * cn), sentinel, dtype=torch.uint8, device=dev)
    size = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the batch's streams do not wait for torch's)
    b.deskew_device_cn(d.data_ptr(), rows * cols * cn, cols * cn, cn, n, black_max, interp, border, out.data_ptr(),
                       dr * dc * cn, dc * cn, size.data_ptr(), best.data_ptr())
    b.sync()
    return out, size.cpu().numpy(), best.cpu().numpy()


def _check_canvas(oracle, got_slot, card, angle, interp, border, size, sentinel=7):
    exp = oracle.rotate_mat(card, angle, 1.0, interp, tuple(border) + (0,), 1)
    dr, dc = exp.shape[:2]
    assert tuple(size) == (dr, dc), (size, exp.shape)
    got = got_slot[:dr, :dc * 3].reshape(dr, dc, 3)
    if interp == NEAREST:
        assert (got == exp).all(), int((got != exp).sum())
    else:
        assert np.abs(got.astype(np.int16) - exp.astype(np.int16)).max() <= 1
    per_call = transfer.rotate_mat(card, angle, 1.0, interp, 0, tuple(float(v) for v in border) + (0.0,),
                                   RotateClipStrategy.CONTAIN).get_mat()
    assert per_call.shape == got.shape and (got == per_call).all()
    # nothing outside the scan's own canvas is written
    assert (got_slot[dr:, :] == sentinel).all() and (got_slot[:, dc * 3:] == sentinel).all()


@pytest.mark.parametrize("interp,cols,border", [(NEAREST, 452, WHITE), (LINEAR, 452, WHITE), (NEAREST, 453, WHITE),
                                                (LINEAR, 453, (10, 128, 250)), (LINEAR, 452, (10, 128, 250))])
def test_batch_deskew_colour_small_batch_every_scan(oracle, interp, cols, border):
    # cols = 453: the colour rows (1359 bytes) are not whole dwords, every tile takes the unstaged per-tap path
    rows, max_angle, step = 640, 10, 0.5
    skews = [-9.3, -4.0, -0.2, 0.0, 0.7, 3.1, 6.6, 9.4, 2.2, -7.5, 5.0]
    cards, theta = _cards(rows, cols, len(skews), 500, skews)
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=1)
    b.set_group(4)
    out, size, best = _deskew_cn(b, cards, 3, interp, border)
    # the winners are the gray path's
    gray = _gray(oracle, cards)
    (cb, _, _), (gb, _, _) = _sweep_both(b, cards, gray)
    N = b.N
    b.close()
    assert (best == cb).all() and (best == gb).all()
    out = out.cpu().numpy()
    for i in range(len(skews)):
        angle = (int(best[i]) - N) * step
        assert abs(angle - theta[i]) <= step + 1e-9, (i, angle, theta[i])
        _check_canvas(oracle, out[i], cards[i], angle, interp, border, size[i])


def test_batch_deskew_colour_a4_behind_scan_lanes(oracle):
    rows, cols, max_angle, step, n = 3508, 2480, 10, 0.05, 64
    uniq, theta8 = _cards(rows, cols, 8, 40)
    idx = [i % 8 for i in range(n)]  # 64 scans: 8 distinct cards, each in 8 slots
    gray8 = _gray(oracle, uniq)
    torch, dev = _dev()
    d8 = torch.from_numpy(uniq).to(dev)
    scans = d8[idx].contiguous()
    del d8
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=2)
    b.set_lanes(64)
    # winners of the gray path on the same scans
    g = torch.from_numpy(gray8).to(dev)[idx].contiguous()
    gbest = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    b.run_device(g.data_ptr(), rows * cols, cols, n, 127, gbest.data_ptr())
    b.sync()
    gbest = gbest.cpu().numpy()
    del g
    dr, dc = b.deskew_canvas()
    N = b.N
    for interp in (NEAREST, LINEAR):
        out = torch.full((n, dr, dc * 3), 7, dtype=torch.uint8, device=dev)
        size = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        best = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        b.deskew_device_cn(scans.data_ptr(), rows * cols * 3, cols * 3, 3, n, 127, interp, WHITE, out.data_ptr(),
                           dr * dc * 3, dc * 3, size.data_ptr(), best.data_ptr())
        b.sync()
        best = best.cpu().numpy()
        size = size.cpu().numpy()
        assert (best == gbest).all()
        for i in (0, 37, 63):
            angle = (int(best[i]) - N) * step
            assert abs(angle - theta8[idx[i]]) <= 2 * step, (i, angle, theta8[idx[i]])
            _check_canvas(oracle, out[i].cpu().numpy(), uniq[idx[i]], angle, interp, WHITE, size[i])
        del out
    b.close()


def test_one_channel_through_the_new_entry_points(oracle):
    torch, dev = _dev()
    rows, cols, max_angle, step = 640, 452, 10, 0.5
    skews = [-8.0, -1.5, 0.5, 4.4, 9.0, 2.0, -3.3]
    gray = np.stack([synth.make_card(rows, cols, 700 + i, skew=s)[0] for i, s in enumerate(skews)])
    n = len(skews)
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=2)
    b.set_group(4)
    A = b.A
    d = torch.from_numpy(gray).to(dev)
    outs = []
    for new in (True, False):
        best = torch.full((n,), -1, dtype=torch.int32, device=dev)
        vs = torch.zeros((n, A), dtype=torch.float64, device=dev)
        hs = torch.zeros((n, A), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        if new:
            b.run_device_cn(d.data_ptr(), rows * cols, cols, 1, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        else:
            b.run_device(d.data_ptr(), rows * cols, cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        b.sync()
        outs.append((best.cpu().numpy(), vs.cpu().numpy().view(np.uint64), hs.cpu().numpy().view(np.uint64)))
    for x, y in zip(*outs):
        assert (x == y).all()
    dr, dc = b.deskew_canvas()
    for interp in (NEAREST, LINEAR):
        res = []
        for new in (True, False):
            out = torch.full((n, dr, dc), 7, dtype=torch.uint8, device=dev)
            size = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            best = torch.full((n,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            if new:
                b.deskew_device_cn(d.data_ptr(), rows * cols, cols, 1, n, 127, interp, (200, 1, 2), out.data_ptr(), dr * dc,
                                   dc, size.data_ptr(), best.data_ptr())
            else:
                b.deskew_device(d.data_ptr(), rows * cols, cols, n, 127, interp, 200, out.data_ptr(), dr * dc, dc,
                                size.data_ptr(), best.data_ptr())
            b.sync()
            res.append((out.cpu().numpy(), size.cpu().numpy(), best.cpu().numpy()))
        for x, y in zip(*res):
            assert (x == y).all()
    b.close()


def test_argument_errors_leave_the_context_usable(oracle):
    torch, dev = _dev()
    rows, cols, max_angle, step, n = 320, 228, 5, 0.5, 3
    cards, theta = _cards(rows, cols, n, 60, [1.0, -2.0, 3.5])
    gray = _gray(oracle, cards)
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=1)
    ref = _sweep_both(b, cards, gray)
    dr, dc = b.deskew_canvas()
    d = torch.from_numpy(cards).to(dev)
    out = torch.full((n, dr, dc * 3), 7, dtype=torch.uint8, device=dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    L = oics.lib()
    border = (C.c_uint8 * 4)(255, 255, 255, 0)
    S, P = rows * cols * 3, cols * 3

    def run(channels=3, black_max=127):
        return L.omr_batch_run_device_cn(b.handle, d.data_ptr(), S, P, channels, n, black_max, best.data_ptr(), None, None)

    def deskew(interp=0, out_step=dc * 3, channels=3, black_max=127):
        return L.omr_batch_deskew_device_cn(b.handle, d.data_ptr(), S, P, channels, n, black_max, interp, border, out.data_ptr(),
                                            dr * dc * 3, out_step, None, best.data_ptr())

    cases = [(lambda: run(channels=4), -213), (lambda: run(channels=2), -213), (lambda: run(black_max=-1), -5),
             (lambda: run(black_max=256), -5), (lambda: deskew(channels=4), -213), (lambda: deskew(black_max=-1), -5),
             (lambda: deskew(black_max=256), -5), (lambda: deskew(out_step=3 * dc - 1), -5), (lambda: deskew(interp=2), -213)]
    for k, (call, code) in enumerate(cases):
        assert call() == code, k
        assert len(L.omr_last_error()) > 0
        # the context still works and gives the same answer
        best.fill_(-1)
        torch.cuda.synchronize()
        assert run() == 0
        b.sync()
        assert (best.cpu().numpy() == ref[0][0]).all(), k
    assert deskew(interp=1) == 0
    b.sync()
    assert (best.cpu().numpy() == ref[0][0]).all()
    b.close()
