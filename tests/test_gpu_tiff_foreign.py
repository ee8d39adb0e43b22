"""The device TIFF decoder on the streams libtiff would not write itself (t6_rewrap.py, validated on the CPU by
test_t6_rewrap.py): other T.6 mode choices, split make-up codes, five strip endings, rows of 12288 single pixels that
outrun the input window and fill a line buffer to its last entry, PackBits cut into runs in four ways, and IFDs laid out,
typed and thinned as foreign writers do.  Every comparison is with Pillow (libtiff's decoder), byte for byte, through
decode_on_device of test_gpu_tiff_decode.py: slots larger than the images, a pitch pad, a base offset, every slack byte
checked; a group per call, for 1 and 3 channels.

Left out of the Pillow comparison, each by name: the pins of t6_rewrap.pins() with their codes, and the files of
t6_rewrap.NO_ARBITER (several strips of Compression 4 or 32773 without StripByteCounts), where Pillow raises
OSError("decoder error -2") behind libtiff's 'MissingRequired: TIFF directory is missing required "StripByteCounts" field';
those are held to the picture they were made from."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import t6_rewrap as T  # noqa: E402
import tiff_ref  # noqa: E402
from test_gpu_tiff_decode import _same, decode_on_device  # noqa: E402
from oics import imread, projection, synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _want(name, stream, made_from, channels):
    g = made_from if name in T.NO_ARBITER else tiff_ref.pillow_read(stream)
    if name not in T.NO_ARBITER:
        assert g.shape == made_from.shape and (g == made_from).all(), (name, "Pillow does not read the picture")
    return g if channels == 1 else np.repeat(g[..., None], 3, axis=2)


def _group(cases, rows, cols, channels, **kw):
    imgs, size, rc = decode_on_device([s for _, s, _ in cases], rows, cols, channels, **kw)
    assert (rc == 0).all(), [(cases[i][0], int(rc[i])) for i in np.nonzero(rc)[0][:10]]
    for i, (name, s, made_from) in enumerate(cases):
        _same(imgs[i], _want(name, s, made_from, channels), name)


@pytest.mark.parametrize("channels", [3, 1])
def test_t6_mode_policies_and_endings(channels):
    _group(T.t6_dialects(), 40, 260, channels, pitch_pad=5, base_offset=1)


@pytest.mark.parametrize("channels", [3, 1])
def test_t6_split_make_up_codes(channels):
    cases = T.split_dialects()[0]
    _group([c for c in cases if c[2].shape[1] == 257], 40, 260, channels, pitch_pad=5, base_offset=3)
    _group([c for c in cases if c[2].shape[1] != 257], 2, 5200, channels, pitch_pad=3, base_offset=1)


@pytest.mark.parametrize("channels", [3, 1])
def test_widest_rows_and_one_column_more(channels):
    cases = T.widest_rows()
    assert len(cases) == 4
    wider = tiff_ref.assemble(2, T.WIDEST + 1, [b"\0\0"], 4)
    streams = [cases[0][1], cases[1][1], wider, cases[2][1], cases[3][1]]
    imgs, size, rc = decode_on_device(streams, 3, T.WIDEST + 4, channels, pitch_pad=3, base_offset=1)
    assert list(rc) == [0, 0, -213, 0, 0] and tuple(size[2]) == (0, 0)
    for i, c in zip((0, 1, 3, 4), cases):
        _same(imgs[i], _want(c[0], c[1], c[2], channels), c[0])


@pytest.mark.parametrize("channels", [3, 1])
def test_packbits_run_policies(channels):
    _group(T.packbits_dialects(), 40, 260, channels, pitch_pad=5, base_offset=1)


@pytest.mark.parametrize("channels", [3, 1])
def test_ifd_layouts_missing_tags_and_types(channels):
    cases = T.ifd_dialects()
    assert sum(n in T.NO_ARBITER for n, _, _ in cases) == 8
    _group(cases, 40, 260, channels, pitch_pad=7, base_offset=5)


def _mixed():
    """streams of every group"""
    return [T.t6_dialects()[i] for i in (5, 150, 333)] + [T.packbits_dialects()[i] for i in (7, 900)] + \
        [c for c in T.ifd_dialects() if "none-of-the-five-no-counts" in c[0]][:1]


def test_through_imread_next_to_a_jpeg_and_a_png():
    import fuzz_jpeg_decode as fz
    import png_ref as P
    rgb = synth.make_color_card(64, 48, 3, 2.0)[0]
    cases = _mixed()
    streams = [fz.make_stream(rgb, 95, subsampling=2)] + [s for _, s, _ in cases] + [P.write(np.ascontiguousarray(rgb[..., ::-1]), 2, 8)]
    imgs, size, rc = decode_on_device(streams, 66, 260, 3, pitch_pad=2, base_offset=1, fn=imread.decode_batch_device)
    assert (rc == 0).all(), rc
    _same(imgs[0], fz.pillow_decode(streams[0], 3), "jpeg")
    _same(imgs[-1], rgb, "png")
    for i, (name, s, made_from) in enumerate(cases):
        _same(imgs[1 + i], _want(name, s, made_from, 3), name)


def test_through_the_projection_streams_flow():
    """the flow fed foreign forms of two sheets returns what it returns for their libtiff forms: angles as f64 bits, output
    streams byte for byte"""
    lib, foreign = [], []
    for k, (rows, cols, seed, skew, rps) in enumerate(((120, 90, 80, 4.0, 120), (150, 199, 64, -6.0, 32))):
        bits = (synth.make_color_card(rows, cols, seed, skew)[0][..., 1] < 128).astype(np.uint8)
        base = tiff_ref.pillow_tiff(bits, "group4", rps)
        h = tiff_ref.parse(base)
        stored = bits if h["photometric"] == 0 else 1 - bits
        lib.append(base)
        strips = T.t6_strips(stored, rps, ("random", "h-only")[k], "split", T.ENDINGS[2 + k], 5 + k)
        foreign.append(tiff_ref.assemble(rows, cols, strips, 4, photometric=h["photometric"], fill_order=2, rps=rps, order=">",
                                         ifd_first=True, shuffle=k, reverse=True, gap=1, drop=(258, 277)))
        assert (tiff_ref.pillow_read(foreign[k]) == tiff_ref.pillow_read(base)).all()
    first = (tiff_ref.pillow_read(lib[0]) == 0).astype(np.uint8)  # the first sheet again: PackBits across the rows, no byte counts
    packed = tiff_ref.assemble(120, 90, [T.packbits_encode(T.pack_rows(first), "crossing")], 32773, photometric=0, drop=(279,))
    assert (tiff_ref.pillow_read(packed) == tiff_ref.pillow_read(lib[0])).all()
    sweep = (10, 0.5, 0.5)
    a0, i0, r0, o0 = projection.deskew_streams(lib + [lib[0]], *sweep, interp=1, quality=95, want_idx=True)
    a1, i1, r1, o1 = projection.deskew_streams(foreign + [packed], *sweep, interp=1, quality=95, want_idx=True)
    assert list(r0) == [0, 0, 0] and list(r1) == [0, 0, 0]
    assert (np.asarray(a0, np.float64).view(np.uint64) == np.asarray(a1, np.float64).view(np.uint64)).all() and list(i0) == list(i1)
    for k in range(3):
        assert o0[k] == o1[k], (k, "the output streams differ")


def test_pins_between_good_neighbours():
    pins = T.pins()
    good = T.t6_dialects()[400]
    streams = [good[1]]
    for _, s, _ in pins:
        streams += [s, good[1]]
    for channels in (1, 3):
        imgs, size, rc = decode_on_device(streams, 40, 260, channels, pitch_pad=7, base_offset=5,
                                          shapes=[(0, 0)] * len(streams))
        for i in range(0, len(streams), 2):
            assert rc[i] == 0
            _same(imgs[i], _want(good[0], good[1], good[2], channels), "the good neighbour %d" % i)
        for k, (name, s, code) in enumerate(pins):
            assert rc[2 * k + 1] == code and tuple(size[2 * k + 1]) == (0, 0), (name, int(rc[2 * k + 1]))
