"""The per-tile records of the batch warp (csrc/deskew.hip, deskew_tiles_kernel<LINEAR, CN>) on shapes small enough that
every branch of the record decides a visible share of the canvas: one tile, a canvas that ends at and just past a tile
border, a padded pitch (staged: interior tiles in 16-byte pieces, edge tiles patched) and the same scans from an odd
address (every tile unstaged) -- 1 and 3 channels, NEAREST and LINEAR.

Every scan's canvas is byte for byte the per-call rotate by the detected angle (omr_rotate_device for 1 channel,
transfer.rotate_mat for BGR: code the batch warp shares nothing with but the table arithmetic), the oracle's rotate_mat
exactly for NEAREST and within one level for LINEAR (its bilinear weights are floats rounded to 15 bits, the kernels'
are the exact integers: the same bound the other deskew tests use), out_size is the canvas, and the slot's sentinel
fill is untouched outside it.  No agreement between detected and injected angle is asked of cards this small."""
import ctypes as C
import functools

import numpy as np
import pytest

import oics
from oics import _lib, projection, synth, transfer
from oics.types import RotateClipStrategy

pytestmark = pytest.mark.gpu

NEAREST, LINEAR = 0, 1
MAX_ANGLE, STEP = 10, 0.5
SKEWS = (-9.3, -4.0, 0.5, 3.1, 9.4)  # five cards: a launch of 4 and one of 1 at set_group(4)
SENTINEL = 7
BORDER = {1: (200, 200, 200), 3: (10, 128, 250)}
# (rows, cols, bytes per pixel row and channel, offset of the first scan from an aligned address)
LAYOUTS = {
    "one_tile_37x41": (37, 41, 41, 0),
    "tile_border_64x128": (64, 128, 128, 0),
    "past_tile_border_65x132": (65, 132, 132, 0),
    "padded_pitch_300x404": (300, 404, 416, 0),
    "odd_address_300x404": (300, 404, 416, 1),
}


@functools.lru_cache(maxsize=None)
def _cards(rows, cols, cn):
    make = synth.make_card if cn == 1 else synth.make_color_card
    cards = np.stack([make(rows, cols, 1200 + i, skew=s)[0] for i, s in enumerate(SKEWS)])
    cards.setflags(write=False)
    return cards


def _rotate_device_gray(d_src_ptr, sstep, rows, cols, angle, interp, border):
    """omr_rotate_device (CONTAIN) of one scan where it lies -> numpy canvas"""
    import torch
    L = oics.lib()
    dr, dc = C.c_int32(), C.c_int32()
    assert L.omr_rotate_size(rows, cols, angle, 1, C.byref(dr), C.byref(dc)) == 0
    out = torch.zeros((dr.value, dc.value), dtype=torch.uint8, device="cuda:0")
    b = (C.c_uint8 * 4)(*border, 0)
    rc = L.omr_rotate_device(C.c_void_p(d_src_ptr), sstep, rows, cols, 1, float(angle), 1.0, interp, C.cast(b, _lib.u8p), 1,
                             C.c_void_p(out.data_ptr()), dc.value, dr.value, dc.value, None)
    assert rc == 0, L.omr_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("interp", [NEAREST, LINEAR], ids=["nearest", "linear"])
@pytest.mark.parametrize("cn", [1, 3], ids=["gray", "bgr"])
def test_every_scan_is_the_per_call_rotate(oracle, cn, interp, layout):
    import torch
    rows, cols, pitch1, offset = LAYOUTS[layout]
    cards = _cards(rows, cols, cn)
    n, pitch, border = len(cards), pitch1 * cn, BORDER[cn]
    stride = rows * pitch
    dev = torch.device("cuda:0")
    # the scans inside a buffer of 0x55 bytes: `offset` bytes in, rows `pitch` apart
    host = np.full(offset + n * stride + 16, 0x55, np.uint8)
    view = host[offset:offset + n * stride].reshape(n, rows, pitch)
    view[:, :, :cols * cn] = cards.reshape(n, rows, cols * cn)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    d_scans = buf.data_ptr() + offset

    b = projection.Batch(rows, cols, MAX_ANGLE, STEP, device=0, n_streams=1)
    b.set_group(4)
    dr, dc = b.deskew_canvas()
    out = torch.full((n, dr, dc * cn), SENTINEL, dtype=torch.uint8, device=dev)
    size = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the batch's streams do not wait for torch's)
    if cn == 1:
        b.deskew_device(d_scans, stride, pitch, n, 127, interp, border[0], out.data_ptr(), dr * dc, dc, size.data_ptr(),
                        best.data_ptr())
    else:
        b.deskew_device_cn(d_scans, stride, pitch, cn, n, 127, interp, border, out.data_ptr(), dr * dc * cn, dc * cn,
                           size.data_ptr(), best.data_ptr())
    b.sync()
    N = b.N
    b.close()
    out, size, best = out.cpu().numpy(), size.cpu().numpy(), best.cpu().numpy()
    assert ((best >= 0) & (best <= 2 * N)).all(), best
    for i in range(n):
        angle = (int(best[i]) - N) * STEP
        exp = oracle.rotate_mat(cards[i], angle, 1.0, interp, border + (0,), 1)
        er, ec = exp.shape[:2]
        assert tuple(size[i]) == (er, ec), (i, size[i], exp.shape)
        assert er <= dr and ec <= dc
        got = out[i, :er, :ec * cn].reshape(exp.shape)
        if cn == 1:
            per_call = _rotate_device_gray(d_scans + i * stride, pitch, rows, cols, angle, interp, border)
        else:
            per_call = transfer.rotate_mat(cards[i], angle, 1.0, interp, 0, tuple(float(v) for v in border) + (0.0,),
                                           RotateClipStrategy.CONTAIN).get_mat()
        assert per_call.shape == got.shape, (i, per_call.shape, got.shape)
        assert (got == per_call).all(), (i, angle, int((got != per_call).sum()))
        if interp == NEAREST:
            assert (got == exp).all(), (i, angle, int((got != exp).sum()))
        else:
            assert np.abs(got.astype(np.int16) - exp.astype(np.int16)).max() <= 1, (i, angle)
        # nothing outside the scan's own canvas is written
        assert (out[i, er:, :] == SENTINEL).all() and (out[i, :, ec * cn:] == SENTINEL).all(), i
