"""The device JPEG decoder (csrc/oics_jpeg_dec.cpp, csrc/jpeg_dec.hip) on streams libjpeg would not write itself: the
dialects of tests/jpeg_rewrap.py -- flat, deep, per-component and redefined Huffman tables under ids 0..3, several tables
in one segment, DRI anywhere before SOS, long and unknown segments, fill bytes before header markers and before RSTn, junk
behind EOI, intervals padded with 0-bits or mixed bits, restart intervals that do not divide a row, span the
whole scan or wrap the RSTn counter, gray frames that declare sampling factors.  Every rewritten stream holds the
coefficients of a stream Pillow wrote, and tests/test_jpeg_rewrap.py shows that Pillow (libjpeg-turbo, the arbiter) reads
it as the original; here every comparison is byte for byte against Pillow's decode, at 1 and 3 channels, with the
streams of a group in one call so that different dialects are neighbours, in slots with a pitch at an odd base, the
bytes around the images checked untouched."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import jpeg_rewrap as W  # noqa: E402
from oics import imread, jpeg, projection, synth  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def _codes():
    """OMR_ERR_NOTIMPL and OMR_ERR_BADARG as include/omrdeskew.h defines them"""
    text = open(os.path.join(os.path.dirname(HERE), "include", "omrdeskew.h")).read()
    return tuple(int(re.search(r"#define %s \((-?\d+)\)" % name, text).group(1)) for name in ("OMR_ERR_NOTIMPL", "OMR_ERR_BADARG"))


def _want(original, channels):
    """Pillow's decode of the stream the rewritten one came from, computed once"""
    key = (original, channels)
    if key not in _WANT:
        _WANT[key] = fz.pillow_decode(original, channels)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _on_device(decode_batch, streams, rows, cols, channels, pitch_pad=5, base_offset=1, fill=0xA5):
    """-> (images, out_size, rc) of decode_batch(streams, channels, d_out, stride, step, rows, cols); asserts that every byte
    outside an accepted image, and every byte of a refused stream's slot, still holds `fill`"""
    import torch
    n = len(streams)
    step = cols * channels + pitch_pad
    stride = rows * step + pitch_pad
    out = torch.full((base_offset + n * stride + 8,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size, rc = decode_batch(streams, channels, out.data_ptr() + base_offset, stride, step, rows, cols)
    got = out.cpu().numpy()
    assert (got[:base_offset] == fill).all() and (got[base_offset + n * stride:] == fill).all()
    imgs = []
    for i in range(n):
        slot = got[base_offset + i * stride: base_offset + (i + 1) * stride]
        body = slot[:rows * step].reshape(rows, step)
        r, c = (int(size[i, 0]), int(size[i, 1])) if rc[i] == 0 else (0, 0)
        mask = np.ones((rows, step), bool)
        mask[:r, :c * channels] = False
        if rc[i] != -215:   # the content of a slot whose entropy data failed is unspecified, inside its image
            assert (body[mask] == fill).all() and (slot[rows * step:] == fill).all(), "slot %d written outside its image" % i
        im = body[:r, :c * channels].copy()
        imgs.append(im.reshape(r, c) if channels == 1 else im.reshape(r, c, 3))
    return imgs, size, rc


def _check_group(items, rows, cols, channels, decode_batch=jpeg.decode_batch):
    """items: [(what, original, rewritten, stats)], all in one call"""
    imgs, size, rc = _on_device(decode_batch, [s for _, _, s, _ in items], rows, cols, channels)
    bad = [(what, int(rc[i])) for i, (what, _, _, _) in enumerate(items) if rc[i] != 0]
    assert not bad, bad
    for i, (what, original, _, _) in enumerate(items):
        want = _want(original, channels)
        assert imgs[i].shape == want.shape, (what, imgs[i].shape, want.shape)
        assert (imgs[i] == want).all(), (what, int((imgs[i] != want).sum()), "bytes differ from Pillow's")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("group", list(W.GROUPS))
def test_group_equals_pillow(group, channels):
    items = [item for name in W.GROUPS[group] for item in W.case_streams(name)]
    _check_group(items, 36, 50, channels)


@pytest.mark.parametrize("channels", [1, 3])
def test_scans_that_span_workgroups(channels):
    """176 x 208 colour noise at quality 95: more than 256 subsequences of 1024 bits in every stream, the deep and flat
    tables and the paddings among them, next to the original"""
    items = W.big_streams()
    for what, _, _, stats in items:
        assert stats["entropy"] * 8 > W.BIG_BITS, (what, stats)
    original = items[0][1]
    _check_group(items + [(("as Pillow wrote it", "big"), original, original, None)], 176, 208, channels)


@pytest.mark.parametrize("channels", [1, 3])
def test_gray_frames_that_declare_sampling_factors(channels):
    """a one-component frame at 2 x 2, 2 x 1 or 1 x 2: the factors mean nothing (T.81 A.2.2), one MCU is one block"""
    items = W.gray_sampling_streams()
    for _, _, s, _ in items:
        assert jpeg.info(s)[2:] == (1, 0x11)
    _check_group(items, 17, 17, channels)
    what, original, s, _ = items[-1]
    want = _want(original, channels)
    assert (jpeg.decode(s, channels) == want).all() and (imread.decode(s, channels) == want).all(), what


def test_refusals_between_good_neighbours():
    notimpl, badarg = _codes()
    good = [W.case_streams(name)[k] for k, name in enumerate(("deep_pad_zeros", "split", "flat_pad_alt", "fill_before_rst"))]
    base = W.original(33, 47, "420")
    sof = base.index(b"\xff\xc0")

    def patched(at, value):
        b = bytearray(base)
        b[at] = value
        return bytes(b)

    # three codes of one bit: the counts overflow the code space, the segment itself is well formed
    overflow = base[:sof] + W.segment(0xC4, bytes([0x00, 3] + [0] * 15 + [0, 1, 2])) + base[sof:]
    streams = [good[0][2], patched(sof + 14, 0x21), good[1][2], patched(sof + 11, 0x41), good[2][2], overflow, good[3][2],
               patched(sof + 17, 0x12)]
    for channels in (1, 3):
        imgs, size, rc = _on_device(jpeg.decode_batch, streams, 36, 50, channels)
        assert list(rc) == [0, notimpl, 0, notimpl, 0, badarg, 0, notimpl]
        for k in range(4):
            assert (imgs[2 * k] == _want(good[k][1], channels)).all(), good[k][0]
            assert list(size[2 * k + 1]) == [0, 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_through_imread(channels):
    """one stream of every case, samplings and shapes rotating, and the gray frames with factors, through
    omr_imread_batch_device"""
    items = [W.case_streams(name)[(5 * k) % 12] for k, name in enumerate(W.CASES)] + W.gray_sampling_streams()[::5]
    _check_group(items, 36, 50, channels, decode_batch=imread.decode_batch_device)


def test_projection_streams_flow_does_not_see_the_dialect():
    """omr_deskew_with_projections_batch_streams on a sheet as Pillow wrote it and on the same sheet in four other dialects:
    the same angle bits, the same best index, the same output stream"""
    sheet = fz.make_stream(synth.make_color_card(120, 90, 81, 9.0)[0], 95, subsampling=2)
    gray = fz.make_stream(synth.make_color_card(120, 90, 81, 9.0)[0], 95, gray=True)
    streams = [sheet] + [W.rewrap(sheet, **W.CASES[name])[0] for name in ("deep_pad_zeros", "split", "flat_pad_alt", "fill_before_rst")]
    streams += [gray, W.rewrap(gray, gray_sampling=0x22, **W.CASES["deep_pad_alt"])[0]]
    ang, idx, rc, out = projection.deskew_streams(streams, 10, 0.5, 0.5, interp=1, quality=95, want_idx=True)
    assert list(rc) == [0] * len(streams)
    for i, first in ((1, 0), (2, 0), (3, 0), (4, 0), (6, 5)):
        assert np.float64(ang[i]).view(np.uint64) == np.float64(ang[first]).view(np.uint64) and idx[i] == idx[first], i
        assert out[i] is not None and out[i] == out[first], (i, "the output streams differ")
    assert ang[0] != 0.0
