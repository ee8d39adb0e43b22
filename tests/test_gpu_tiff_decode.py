"""The device TIFF decoder (omr_tiff_decode_batch_device / omr_tiff_decode) and the imread layer's third kind against Pillow's
libtiff, byte for byte: every small shape x RowsPerStrip x compression x content in one call per channel count, long runs,
one A4 page, damaged strips between good ones, and a mixed imread batch.  The inputs are those of tiff_cases.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import tiff_cases  # noqa: E402
import tiff_ref  # noqa: E402
from oics import imread, synth, tiff  # noqa: E402

pytestmark = pytest.mark.gpu


def decode_on_device(streams, rows, cols, channels, pitch_pad=0, base_offset=0, fill=0xA5, fn=None, shapes=None):
    """-> (images, out_size, rc); asserts that every byte outside the images still holds `fill` -- for a damaged image (-215)
    outside the image its header names (shapes[i]), whose content is unspecified"""
    import torch
    fn = fn or tiff.decode_batch_device
    n = len(streams)
    step = cols * channels + pitch_pad
    stride = rows * step + pitch_pad
    out = torch.full((base_offset + max(n, 1) * stride + 8,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size, rc = fn(streams, channels, out.data_ptr() + base_offset, stride, step, rows, cols)
    got = out.cpu().numpy()
    assert (got[:base_offset] == fill).all() and (got[base_offset + n * stride:] == fill).all()
    imgs = []
    for i in range(n):
        slot = got[base_offset + i * stride: base_offset + (i + 1) * stride]
        body = slot[:rows * step].reshape(rows, step)
        r, c = (int(size[i, 0]), int(size[i, 1])) if rc[i] == 0 else (0, 0)
        mask = np.ones((rows, step), bool)
        if rc[i] == -215:
            mask[:shapes[i][0], :shapes[i][1] * channels] = False
        else:
            mask[:r, :c * channels] = False
        assert (body[mask] == fill).all() and (slot[rows * step:] == fill).all(), "slot %d written outside its image" % i
        im = body[:r, :c * channels].copy()
        imgs.append(im.reshape(r, c) if channels == 1 else im.reshape(r, c, 3))
    return imgs, size, rc


def _want(stream, channels):
    g = tiff_ref.pillow_read(stream)
    return g if channels == 1 else np.repeat(g[..., None], 3, axis=2)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, int((got != want).sum()), "bytes differ")


@pytest.mark.parametrize("channels", [3, 1])
def test_every_shape_compression_and_content_in_one_call(channels):
    cases = tiff_cases.small_cases()
    assert len(cases) == 3 * 8 * sum(len({1, min(8, r), r}) for r in tiff_cases.ROWS) * 9
    streams = [s for _, s in cases]
    imgs, size, rc = decode_on_device(streams, 40, 260, channels, pitch_pad=5, base_offset=1)
    assert (rc == 0).all(), [(cases[i][0], int(rc[i])) for i in np.nonzero(rc)[0][:10]]
    for i, (name, s) in enumerate(cases):
        _same(imgs[i], _want(s, channels), name)


def test_long_runs():
    cases = tiff_cases.long_run_cases()
    imgs, size, rc = decode_on_device([s for _, s in cases], 2, 5200, 1, pitch_pad=3, base_offset=3)
    assert (rc == 0).all(), rc
    for i, (name, s) in enumerate(cases):
        _same(imgs[i], _want(s, 1), name)
        _same(imgs[i], tiff_ref.decode(s), name + " (restatement)")


def test_one_a4_page_in_one_strip_and_in_default_strips():
    card = synth.make_binary_card(3508, 2480, 7, skew=1.5)[0]
    bits = (card < 128).astype(np.uint8)
    one = tiff_ref.pillow_tiff(bits, "group4", 3508)
    many = tiff_ref.pillow_tiff(bits, "group4")
    assert tiff.info(one)[5] == 1 and tiff.info(many)[:2] == (3508, 2480)
    for name, s in (("one strip", one), ("default strips", many)):
        got = tiff.decode(s, 1)
        _same(got, _want(s, 1), name)
    assert 0 < int((got == 0).sum()) < got.size  # a page with something on it


def _damaged():
    """[(name, stream, the restatement's verdict: an image or None for -215)]"""
    a = tiff_cases.content("text", 37, 257, seed=9)
    good = tiff_ref.pillow_tiff(a)
    (strip,) = tiff_ref.strips_of(good)
    h = tiff_ref.parse(good)
    out = [("cut in half", tiff_ref.assemble(37, 257, [strip[:len(strip) // 2]], 4, photometric=h["photometric"]))]
    hit = parsed = None
    rng = np.random.RandomState(24)
    for _ in range(400):  # a byte of the middle that breaks the stream, and one that does not
        at, val = int(rng.randint(len(strip) // 4, 3 * len(strip) // 4)), int(rng.randint(0, 256))
        bad = strip[:at] + bytes([val]) + strip[at + 1:]
        if bad == strip:
            continue
        try:
            tiff_ref.t6_decode(bad, 37, 257)
            parsed = parsed or bad
        except tiff_ref.Damaged:
            hit = hit or bad
        if hit and parsed:
            break
    assert hit is not None
    out.append(("a byte overwritten: no longer a T.6 stream", tiff_ref.assemble(37, 257, [hit], 4, photometric=h["photometric"])))
    if parsed is not None:
        out.append(("a byte overwritten: still a T.6 stream", tiff_ref.assemble(37, 257, [parsed], 4, photometric=h["photometric"])))
    pb = tiff_ref.strips_of(tiff_ref.pillow_tiff(a, "packbits", 8))
    pb[1] = pb[1] + b"\x7f" + bytes(128)  # not reached: the strip's rows are full before it
    long_strip = tiff_ref.assemble(37, 257, pb, 32773, rps=8)
    pb2 = list(pb)
    pb2[2] = pb2[2][:-3] + b"\x81\xff"   # the last run made 128 long: past the strip's rows
    out.append(("PackBits with bytes behind its rows", long_strip))
    out.append(("PackBits past its rows", tiff_ref.assemble(37, 257, pb2, 32773, rps=8)))
    res = []
    for name, s in out:
        try:
            res.append((name, s, tiff_ref.decode(s)))
        except tiff_ref.Damaged:
            res.append((name, s, None))
    assert sum(v is None for _, _, v in res) >= 3
    return good, res


def test_damaged_strips_between_good_ones():
    good, res = _damaged()
    streams = [good]
    for _, s, _ in res:
        streams += [s, good]
    for channels in (1, 3):
        imgs, size, rc = decode_on_device(streams, 40, 260, channels, pitch_pad=7, base_offset=5, shapes=[(37, 257)] * len(streams))
        for i in range(0, len(streams), 2):
            assert rc[i] == 0
            _same(imgs[i], _want(good, channels), "the good neighbour %d" % i)
        for k, (name, s, verdict) in enumerate(res):
            i = 2 * k + 1
            if verdict is None:
                assert rc[i] == -215 and tuple(size[i]) == (0, 0), (name, rc[i])
            else:
                assert rc[i] == 0, (name, rc[i])
                _same(imgs[i], verdict if channels == 1 else np.repeat(verdict[..., None], 3, axis=2), name)


def test_single_decode_and_stats():
    name, s = tiff_cases.small_cases()[700]
    _same(tiff.decode(s, 3), _want(s, 3), name)
    tiff.stats(True)
    tiff.decode(s, 1)
    groups, ms = tiff.stats(False)
    assert groups == 1 and len(ms) == 4 and all(v >= 0 for v in ms) and sum(ms) > 0


def test_stats_on_a_fresh_thread_report_the_last_call_alone():
    """per thread and per call: on, one group with its stage times; off again, the next decode reports no group"""
    import math
    import threading
    _, s = tiff_cases.small_cases()[700]
    seen = {}

    def work():
        tiff.stats(True)
        try:
            tiff.decode(s, 1)
            seen["on"] = tiff.stats(False)
        finally:
            tiff.stats(False)
        tiff.decode(s, 1)
        seen["off"] = tiff.stats(False)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    groups, ms = seen["on"]
    assert groups == 1 and all(math.isfinite(v) and v >= 0 for v in ms) and sum(ms) > 0, ms
    assert seen["off"][0] == 0


def test_decode_stats_are_not_the_png_encoders():
    """the two codecs have as many stages; their statistics are still two objects: with the TIFF decoder's collection on,
    a PNG encode on the same thread collects nothing and leaves the decoder's figures alone"""
    import threading
    from oics import png
    _, s = tiff_cases.small_cases()[700]
    seen = {}

    def work():
        tiff.stats_ex(True)
        try:
            img = tiff.decode(s, 1)
            seen["before"] = tiff.stats_ex(True)
            png.encode(img)
            seen["png"] = png.encode_stats(False)
            seen["after"] = tiff.stats_ex(False)
        finally:
            tiff.stats_ex(False), png.encode_stats(False)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert seen["before"][0] == 1 and sum(seen["before"][1]) > 0
    assert seen["png"] == (0, [0.0] * len(png.STAGES_ENC))
    assert seen["after"] == seen["before"]


def test_imread_mixes_the_three_kinds():
    import fuzz_jpeg_decode as fz
    import orient_ref as O
    import png_ref as P
    rgb = synth.make_color_card(64, 48, 3, 2.0)[0]
    a = tiff_cases.content("text", 64, 48, seed=3)
    g4 = tiff_ref.pillow_tiff(a)
    tiled = tiff_ref.rewrap(g4, extra=[(322, 3, [16]), (323, 3, [16])])
    streams = [fz.make_stream(rgb, 95, subsampling=2), O.tag_jpeg(fz.make_stream(np.ascontiguousarray(rgb.transpose(1, 0, 2)), 95, subsampling=2), 6),
               P.write(np.ascontiguousarray(rgb[..., ::-1]), 2, 8), g4, tiled]
    assert imread.info(g4) == (64, 48, 1, 1, imread.OMR_IMREAD_KIND_TIFF)
    imgs, size, rc = decode_on_device(streams, 66, 50, 3, pitch_pad=2, base_offset=1, fn=imread.decode_batch_device)
    assert list(rc) == [0, 0, 0, 0, -213] and tuple(size[4]) == (0, 0)
    _same(imgs[0], fz.pillow_decode(streams[0], 3), "jpeg")
    _same(imgs[1], O.apply(fz.pillow_decode(streams[1], 3), 6), "jpeg, orientation 6")
    _same(imgs[2], rgb, "png")
    _same(imgs[3], _want(g4, 3), "tiff")
    _same(imread.decode(g4, 1), _want(g4, 1), "omr_imread of a TIFF")
