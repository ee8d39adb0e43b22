"""The device JPEG decoder (csrc/jpeg_dec.hip) on the GPU: omr_jpeg_decode_batch_device, omr_jpeg_decode and the streams
form of correct_default, omr_correct_default_batch_streams.  Every
comparison is byte for byte against Pillow (libjpeg-turbo, the arbiter: what imread returns).

The Huffman kernels cut every restart interval into subsequences of 1024 bits, a lane each, 256 lanes a workgroup.  Noise
at quality 100 has blocks longer than a subsequence, so several lanes in a row start in the middle of a block; a flat
image has hundreds of blocks per subsequence; one restart interval per MCU makes every subsequence its own interval."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg as fze  # noqa: E402
import fuzz_jpeg_decode as fz  # noqa: E402
from oics import jpeg, omr, synth  # noqa: E402
from oics.transfer import TransformableMatrix  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 16), (16, 17), (37, 53), (64, 48)]
DATASET = os.path.join(HERE, "golden", "dataset")


def _content(rows, cols, kind):
    rng = np.random.Generator(np.random.PCG64(1000 * rows + cols))
    if kind == "noise":
        return rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((rows, cols, 3), (31, 140, 222), np.uint8)
    return synth.make_color_card(rows, cols, 5)[0].copy()


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, int((got != want).sum()), "bytes differ")


@pytest.mark.parametrize("channels", [1, 3])
def test_mixed_batch_equals_pillow(channels):
    """every shape x variant in one call, contents and qualities rotating, in slots larger than the images with a pitch;
    the helper checks every slack byte untouched"""
    streams = []
    k = 0
    for rows, cols in SHAPES:
        for v in fz.VARIANTS:
            img = _content(rows, cols, ("noise", "flat", "ruled")[k % 3])
            streams.append(fz.make_stream(img, (100, 90, 25)[(k // 3) % 3], **v))
            k += 1
    imgs, size, rc = fz.decode_on_device(streams, 70, 60, channels, pitch_pad=5, base_offset=1)
    assert (rc == 0).all(), rc
    for i, s in enumerate(streams):
        _same(imgs[i], fz.pillow_decode(s, channels), i)


def test_empty_batch_and_a_refused_stream_between_two_good_ones():
    imgs, size, rc = fz.decode_on_device([], 16, 16, 3)
    assert imgs == []
    a, b = _content(37, 53, "noise"), _content(16, 17, "ruled")
    good0, good1 = fz.make_stream(a, 90, subsampling=2), fz.make_stream(b, 100, subsampling=0)
    prog = fz.make_stream(a, 90, progressive=True)
    imgs, size, rc = fz.decode_on_device([good0, prog, good1, good0], 37, 53, 3, pitch_pad=3)
    assert list(rc) == [0, -213, 0, 0] and list(size[1]) == [0, 0]
    _same(imgs[0], fz.pillow_decode(good0, 3), 0)
    _same(imgs[2], fz.pillow_decode(good1, 3), 2)
    _same(imgs[3], imgs[0], 3)
    # an image larger than the slot: its own code, the others unaffected
    imgs, size, rc = fz.decode_on_device([good1, good0], 16, 17, 3)
    assert list(rc) == [0, -5]
    _same(imgs[0], fz.pillow_decode(good1, 3), 0)


@pytest.mark.parametrize("kind,quality", [("noise", 100), ("flat", 90)])
def test_long_and_short_blocks(kind, quality):
    """256 x 384 noise at quality 100: blocks longer than a subsequence; flat: hundreds of blocks per subsequence"""
    img = _content(256, 384, kind)
    streams = [fz.make_stream(img, quality, **v) for v in (dict(subsampling=2), dict(subsampling=0), dict(gray=True))]
    for channels in (1, 3):
        imgs, _, rc = fz.decode_on_device(streams, 256, 384, channels)
        assert (rc == 0).all(), rc
        for i, s in enumerate(streams):
            _same(imgs[i], fz.pillow_decode(s, channels), (kind, channels, i))


def test_one_restart_interval_per_mcu():
    img = _content(150, 270, "ruled")
    streams = [fz.make_stream(img, 75, subsampling=2, restart_marker_blocks=1),
               fz.make_stream(_content(150, 270, "noise"), 100, subsampling=1, restart_marker_blocks=1),
               fz.make_stream(img, 75, gray=True, restart_marker_blocks=1)]
    imgs, _, rc = fz.decode_on_device(streams, 150, 270, 3, pitch_pad=2)
    assert (rc == 0).all(), rc
    for i, s in enumerate(streams):
        _same(imgs[i], fz.pillow_decode(s, 3), i)


def test_dataset_sheet_as_bgr():
    s = open(os.path.join(DATASET, "image001.jpg"), "rb").read()
    rows, cols, comps, sampling = jpeg.info(s)
    assert comps == 1 and sampling == 0x11
    imgs, size, rc = fz.decode_on_device([s], rows, cols, 3)
    assert rc[0] == 0 and list(size[0]) == [rows, cols]
    _same(imgs[0], fz.pillow_decode(s, 3), "image001")


def test_a4_canvas_round_trip():
    """2480 x 3508 colour noise encoded by omr_jpeg_encode_batch_device at quality 100 and decoded again: about 2e8 bits of
    entropy data in one image (the 32-bit offsets and the scans at size), equal to Pillow's decode of the same bytes"""
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.integers(0, 256, (3508, 2480, 3), dtype=np.uint8)
    (stream,), _ = fze.encode_on_device([img], 3508, 2480, 3, 100)
    imgs, _, rc = fz.decode_on_device([stream], 3508, 2480, 3)
    assert rc[0] == 0
    _same(imgs[0], fz.pillow_decode(stream, 3), "a4")


def test_single_decode_equals_the_batch_form():
    img = _content(53, 37, "ruled")
    for v in (dict(subsampling=2), dict(gray=True)):
        s = fz.make_stream(img, 90, **v)
        for channels in (1, 3):
            one = jpeg.decode(s, channels)
            (many,), _, rc = fz.decode_on_device([s], 53, 37, channels)
            assert rc[0] == 0
            _same(one, many, (v, channels))
            _same(TransformableMatrix.from_jpeg_bytes(s, channels).get_mat(), one, "from_jpeg_bytes")
    with pytest.raises(Exception) as e:
        jpeg.decode(fz.make_stream(img, 90, progressive=True))
    assert e.value.code == -213


PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)  # correct_default's, lib.rs:192-205


def test_correct_default_from_streams_equals_the_form_fed_with_pillows_decode():
    """eight dataset sheets of two shapes, interleaved, with a refused stream among them: angle, flag, code and output
    stream of omr_correct_default_batch_streams are those of omr_correct_default_batch_jpeg given Pillow's decode (what
    imread(IMREAD_COLOR) returns) of the same files"""
    by_shape = {}
    for f in sorted(os.listdir(DATASET)):
        if f.lower().endswith(".jpg"):
            s = open(os.path.join(DATASET, f), "rb").read()
            by_shape.setdefault(jpeg.info(s)[:2], []).append(s)
    (a, b) = sorted(by_shape.values(), key=len, reverse=True)[:2]
    sheets = [a[0], b[0], a[1], a[2], b[1], a[3], a[4], a[5]]      # 100 sheets are 1150 x 1240, two 1300 x 1237
    assert len({jpeg.info(s)[:2] for s in sheets}) == 2
    prog = fz.make_stream(_content(37, 53, "noise"), 90, progressive=True)
    got = omr.correct_default_batch_streams(sheets[:3] + [prog] + sheets[3:], *PARAMS)
    assert got[3] == (0.0, False, None, -213)
    got = got[:3] + got[4:]
    want = omr.correct_default_batch_jpeg([fz.pillow_decode(s, 3) for s in sheets], *PARAMS)
    assert len(got) == len(want) == 8
    for i, (g, w) in enumerate(zip(got, want)):
        assert w[3] == 0 and w[2] is not None, i
        assert g[0] == w[0] and g[1] == w[1] and g[3] == w[3], (i, g[:2], w[:2])
        assert g[2] == w[2], (i, "the output streams differ")
    assert len({w[0] for w in want}) > 1      # the sheets are not all turned alike: the comparison says something


def test_decode_stats_count_rounds_and_stages():
    s = fz.make_stream(_content(256, 384, "noise"), 100, subsampling=2)
    jpeg.decode_stats(True)
    try:
        imgs, _, rc = fz.decode_on_device([s, s], 256, 384, 3)
        bits, groups, rounds, ms = jpeg.decode_stats(False)
    finally:
        jpeg.decode_stats(False)
    assert rc[0] == 0 and groups == 1 and rounds >= 2 and all(v > 0 for v in ms)
    _same(imgs[1], fz.pillow_decode(s, 3), "with the collection on")
    fz.decode_on_device([s], 256, 384, 3)
    assert jpeg.decode_stats(False)[1:] == (0, 0, [0.0] * 6)


def test_fill_bytes_before_a_stuffed_ff_are_refused():
    """0xFF 0xFF 0x00 inside a scan (libjpeg and libjpeg-turbo read it differently): -215, never one of the two pictures;
    the same bytes behind the scan's end refuse nothing"""
    good = fz.make_stream(_content(150, 270, "noise"), 100, subsampling=2)
    at = good.index(b"\xff\x00", good.index(b"\xff\xda") + 5000)     # in the scan's second 4096-byte segment
    filled = good[:at] + b"\xff" + good[at:]
    trailing = good + b"\xff\xff\x00" * 3
    imgs, _, rc = fz.decode_on_device([good, filled, trailing], 150, 270, 3)
    assert list(rc) == [0, -215, 0]
    _same(imgs[0], fz.pillow_decode(good, 3), 0)
    _same(imgs[2], imgs[0], "trailing")


def _three_small_streams():
    """24 x 40: a good 4:2:0 stream, a copy cut in the middle of its entropy data (its header still parses: only the device
    can refuse it), a good gray one"""
    img = _content(24, 40, "ruled")
    good = fz.make_stream(img, 90, subsampling=2)
    sos = good.index(b"\xff\xda")
    cut = good[:sos + (len(good) - sos) // 2]
    assert jpeg.info(cut)[:2] == (24, 40)
    return [good, cut, fz.make_stream(img, 90, gray=True)]


def test_out_size_is_zero_where_the_device_finds_the_damage():
    """the header's promise ("0 x 0 where rc[i] != 0") for a refusal that comes from the device, not from the parser"""
    streams = _three_small_streams()
    imgs, size, rc = fz.decode_on_device(streams, 24, 40, 3, pitch_pad=3)
    assert list(rc) == [0, -215, 0]
    assert list(size[1]) == [0, 0]
    assert list(size[0]) == [24, 40] and list(size[2]) == [24, 40]
    for i in (0, 2):
        _same(imgs[i], fz.pillow_decode(streams[i], 3), i)


def test_decode_stats_on_a_fresh_thread_report_the_last_call_alone():
    """the statistics are per thread and per call: on, one group with its rounds and stage times; off again, the next
    decode reports no group"""
    import math
    import threading
    streams = _three_small_streams()
    seen = {}

    def work():
        jpeg.decode_stats(True)
        try:
            fz.decode_on_device(streams, 24, 40, 3, pitch_pad=3)
            seen["on"] = jpeg.decode_stats(False)
        finally:
            jpeg.decode_stats(False)
        fz.decode_on_device(streams, 24, 40, 3, pitch_pad=3)
        seen["off"] = jpeg.decode_stats(False)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    _, groups, rounds, ms = seen["on"]
    assert groups == 1 and rounds >= 1
    assert all(math.isfinite(v) and v >= 0 for v in ms) and sum(ms) > 0, ms
    assert seen["off"][1] == 0


def test_zz_damaged_entropy_data_between_two_good_streams():
    """Last in the file.  A stream cut in the middle of its entropy data, and one with a byte of it changed: rc = -215, or a
    full decode equal to Pillow's where the change happens to leave a valid stream.  The neighbours stay exact."""
    img = _content(150, 270, "noise")
    good = fz.make_stream(img, 90, subsampling=2)
    hdr = good.index(b"\xff\xda")
    cut = good[:hdr + (len(good) - hdr) // 2]
    changed = bytearray(good)
    at = hdr + (len(good) - hdr) // 3
    changed[at] = (changed[at] ^ 0x5A) if (changed[at] ^ 0x5A) != 0xFF and changed[at] != 0xFF else 0x01
    changed = bytes(changed)
    imgs, _, rc = fz.decode_on_device([good, cut, good, changed, good], 150, 270, 3, pitch_pad=1)
    want = fz.pillow_decode(good, 3)
    for i in (0, 2, 4):
        assert rc[i] == 0
        _same(imgs[i], want, i)
    assert rc[1] == -215
    if rc[3] == 0:
        _same(imgs[3], fz.pillow_decode(changed, 3), "changed")
    else:
        assert rc[3] == -215
