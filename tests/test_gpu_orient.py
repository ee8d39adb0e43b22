"""The orientation kernel (csrc/orient.hip) on the GPU: omr_orient_batch_device and omr_orient against the numpy
restatement (tests/orient_ref.py, itself checked against Pillow's exif_transpose).

Sizes: 1 x 1, single rows and columns, one pixel either side of the 3-channel tile (63 x 65, 64 x 64, 65 x 129 -- 129 also
crosses the 1-channel tile of 128), and 37 x 53, whose colour row of 159 bytes is no multiple of 4.  Both sides have padded
pitches that are no multiple of 4 and bases that are not dword-aligned, so row ends are ragged in every way."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orient_ref as O  # noqa: E402
from oics import _lib, transfer  # noqa: E402

pytestmark = pytest.mark.gpu

SLOT = (70, 131)
SIZES = [(1, 1), (1, 67), (67, 1), (63, 65), (64, 64), (65, 129), (37, 53)]
FILL = 0xA5


def _images(cn):
    """every size x every code, the codes rotating so that neighbours differ; the first image once more at the end"""
    rng = np.random.Generator(np.random.PCG64(11 + cn))
    imgs, codes = [], []
    for k, (r, c) in enumerate(SIZES):
        for code in O.CODES:
            imgs.append(rng.integers(0, 256, (r, c) if cn == 1 else (r, c, cn), dtype=np.uint8))
            codes.append((code + k - 1) % 8 + 1)
    imgs.append(imgs[3].copy()), codes.append(codes[3])
    return imgs, codes


def _run(imgs, codes, cn, sizes=True, src_pad=3, dst_pad=5, src_off=1, dst_off=3, dst_slot=(131, 131)):
    import torch
    n = len(imgs)
    sstep, dstep = SLOT[1] * cn + src_pad, dst_slot[1] * cn + dst_pad
    sstride, dstride = SLOT[0] * sstep + src_pad, dst_slot[0] * dstep + dst_pad
    host = np.full(src_off + n * sstride, 0x3C, np.uint8)
    for i, im in enumerate(imgs):
        body = host[src_off + i * sstride: src_off + i * sstride + SLOT[0] * sstep].reshape(SLOT[0], sstep)
        if im.size:
            body[:im.shape[0], :im.shape[1] * cn] = im.reshape(im.shape[0], -1)
    src = torch.from_numpy(host).to("cuda:0")
    dst = torch.full((dst_off + n * dstride + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    sz = [im.shape[:2] for im in imgs] if sizes else None
    out = transfer.orient_batch_device(src.data_ptr() + src_off, sstride, sstep, SLOT[0], SLOT[1], dst.data_ptr() + dst_off, dstride,
                                       dstep, dst_slot[0], dst_slot[1], cn, sz, codes)
    got = dst.cpu().numpy()
    assert (src.cpu().numpy() == host).all(), "the source was written"
    assert (got[:dst_off] == FILL).all() and (got[dst_off + n * dstride:] == FILL).all()
    res = []
    for i in range(n):
        slot = got[dst_off + i * dstride: dst_off + (i + 1) * dstride]
        body = slot[:dst_slot[0] * dstep].reshape(dst_slot[0], dstep)
        r, c = int(out[i, 0]), int(out[i, 1])
        mask = np.ones(body.shape, bool)
        mask[:r, :c * cn] = False
        assert (body[mask] == FILL).all() and (slot[dst_slot[0] * dstep:] == FILL).all(), "slot %d written outside its image" % i
        im = body[:r, :c * cn].copy()
        res.append(im.reshape(r, c) if cn == 1 else im.reshape(r, c, cn))
    return res, out


@pytest.mark.parametrize("cn", [1, 3])
def test_mixed_batch_equals_the_restatement(cn):
    imgs, codes = _images(cn)
    assert set(codes) == set(O.CODES)
    res, out = _run(imgs, codes, cn)
    for i, (im, code) in enumerate(zip(imgs, codes)):
        want = O.apply(im, code)
        assert tuple(out[i]) == want.shape[:2], (i, code, out[i])
        assert res[i].shape == want.shape and (res[i] == want).all(), (i, im.shape, code, int((res[i] != want).sum()))
    assert (res[-1] == res[3]).all()          # the same image at another place in the batch


@pytest.mark.parametrize("cn", [1, 3])
def test_aligned_pitches_and_null_sizes(cn):
    """pitches that are multiples of 4 and a dword-aligned base (image 0's rows move as whole dwords), every image filling
    its slot"""
    rng = np.random.Generator(np.random.PCG64(5))
    imgs = [rng.integers(0, 256, SLOT if cn == 1 else SLOT + (cn,), dtype=np.uint8) for _ in O.CODES]
    pad = (-SLOT[1] * cn) % 4
    res, out = _run(imgs, list(O.CODES), cn, sizes=False, src_pad=pad, dst_pad=(-131 * cn) % 4 + 4, src_off=0, dst_off=0)
    for i, code in enumerate(O.CODES):
        want = O.apply(imgs[i], code)
        assert res[i].shape == want.shape and (res[i] == want).all(), (code, int((res[i] != want).sum()))


def test_a_zero_entry_leaves_its_slot_untouched():
    rng = np.random.Generator(np.random.PCG64(9))
    imgs = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), np.zeros((0, 0, 3), np.uint8),
            rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)]
    res, out = _run(imgs, [6, 7, 8], 3)        # _run checks every byte outside an image: slot 1 is all sentinel
    assert [tuple(o) for o in out] == [(53, 37), (0, 0), (53, 37)] and res[1].size == 0
    assert (res[0] == O.apply(imgs[0], 6)).all() and (res[2] == O.apply(imgs[2], 8)).all()


def test_overlap_and_an_oversize_turned_image_are_refused_before_any_launch():
    import torch
    buf = torch.full((4 * 70 * 131,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with pytest.raises(_lib.OmrError) as e:    # the destination begins inside the source
        transfer.orient_batch_device(p, 70 * 131, 131, 70, 131, p + 100, 70 * 131, 131, 70, 131, 1, [[5, 5]], [1])
    assert e.value.code == -5 and "overlap" in e.value.message
    with pytest.raises(_lib.OmrError) as e:    # 70 x 131 turned by 6 is 131 x 70: no room in a 70 x 131 slot
        transfer.orient_batch_device(p, 70 * 131, 131, 70, 131, p + 2 * 70 * 131, 70 * 131, 131, 70, 131, 1, None, [6])
    assert e.value.code == -5 and "after the turn" in e.value.message
    with pytest.raises(_lib.OmrError) as e:
        transfer.orient_batch_device(p, 70 * 131, 131, 70, 131, p + 2 * 70 * 131, 70 * 131, 131, 70, 131, 1, [[5, 5]], [9])
    assert e.value.code == -5
    assert (buf.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("code", O.CODES)
def test_host_image_form(code):
    img = np.random.Generator(np.random.PCG64(code)).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    got = transfer.orient(img, code).get_mat()
    want = O.apply(img, code)
    assert got.shape == want.shape and (got == want).all()
    gray = transfer.orient(img[..., 1], code).get_mat()       # a strided view: as_image packs it
    assert (gray == O.apply(img[..., 1], code)).all()
