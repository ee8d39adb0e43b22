"""The device decoder on the 8-bit TIFF files libtiff would not write itself (tiff8_rewrap.py, validated on the CPU by
test_tiff8_rewrap.py): LZW coders that match less than they could, clear at a fixed cadence or write literals alone; strips
that end with EOI, with nothing, with junk, with more rows than the file gives them, or inside their last code; contents
whose period stands around the 64 codes of a round; a constant page whose entries reach 3839 bytes; noise rows around the
finishing kernel's turn of 1024 pixels; PackBits cut into runs in four ways over 8-bit rows; and IFDs laid out, typed and
thinned as foreign writers do.  Every comparison is with Pillow (libtiff's decoder), byte for byte, through
decode_on_device of test_gpu_tiff_decode.py: slots larger than the images, a pitch pad, a base offset, every slack byte
checked; a group per call, gray files for 1 and 3 channels, RGB files for 3.  Every call ends with a file of libtiff's own
kind, so that whatever a strip writes behind its rows lands on bytes that are compared.

Left out of the Pillow comparison, each by name: the pins of tiff8_rewrap.pins() with their codes, and the files of
tiff8_rewrap.NO_ARBITER (several LZW or PackBits strips without StripByteCounts), where Pillow raises OSError("decoder
error -2") behind libtiff's 'MissingRequired: TIFF directory is missing required "StripByteCounts" field'; those are held
to the picture they were made from."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import t6_rewrap  # noqa: E402
import tiff8_ref as R  # noqa: E402
import tiff8_rewrap as T  # noqa: E402
import tiff_ref  # noqa: E402
from test_gpu_tiff_decode import _same, decode_on_device  # noqa: E402
from oics import imread, projection, synth  # noqa: E402

pytestmark = pytest.mark.gpu
_WANT = {}


def _want(case, channels):
    """libtiff's picture of a case (read once), as the library returns it"""
    name, s, made_from = case[:3]
    if name not in _WANT:
        g = made_from if name in T.NO_ARBITER else R.pillow_read(s)
        assert g.shape == made_from.shape and (g == made_from).all(), (name, "Pillow does not read the picture")
        _WANT[name] = g
    return R.as_output(_WANT[name], channels)


def _last(spp, rows, cols):
    a = R.content("text", rows, cols, spp, seed=1)
    return ("the last file, %d x %d x %d" % (rows, cols, spp), R.pillow_tiff(a, "tiff_lzw", max(1, rows // 2)), a)


def _group(cases, rows, cols, channels, **kw):
    cases = list(cases)
    cases.append(_last(1 if cases[-1][2].ndim == 2 else 3, min(rows, 8), min(cols, 64)))
    imgs, size, rc = decode_on_device([c[1] for c in cases], rows, cols, channels, **kw)
    assert (rc == 0).all(), [(cases[i][0], int(rc[i])) for i in np.nonzero(rc)[0][:10]]
    for i, case in enumerate(cases):
        _same(imgs[i], _want(case, channels), case[0])


def _by_samples(cases):
    """(spp, channels) -> the cases of that many samples"""
    gray, rgb = [c for c in cases if c[2].ndim == 2], [c for c in cases if c[2].ndim == 3]
    return {(1, 1): gray, (1, 3): gray, (3, 3): rgb}


FORMS = [(1, 1), (1, 3), (3, 3)]


@pytest.mark.parametrize("spp,channels", FORMS)
def test_lzw_policies_and_endings(spp, channels):
    _group(T.policy_dialects(spp), 35, 259, channels, pitch_pad=5, base_offset=1)


@pytest.mark.parametrize("spp,channels", FORMS)
def test_period_contents(spp, channels):
    _group(_by_samples(T.period_dialects())[spp, channels], 8, 260, channels, pitch_pad=3, base_offset=3)


@pytest.mark.parametrize("spp,channels", FORMS)
def test_strips_that_code_more_than_their_rows(spp, channels):
    cases = _by_samples(T.cut_dialects())[spp, channels]
    assert len(cases) >= 30 and sum("cut-lzw" not in c[0] for c in cases) == 6
    _group(cases, 25, 66, channels, pitch_pad=5, base_offset=1)


@pytest.mark.parametrize("spp,channels", FORMS)
def test_wide_predictor_rows(spp, channels):
    _group(_by_samples(T.wide_dialects())[spp, channels], 3, 2050, channels, pitch_pad=1, base_offset=3)


@pytest.mark.parametrize("spp,channels", FORMS)
def test_packbits_run_policies_over_8_bit_rows(spp, channels):
    _group(_by_samples(T.packbits_dialects())[spp, channels], 20, 80, channels, pitch_pad=5, base_offset=1)


@pytest.mark.parametrize("spp,channels", FORMS)
def test_ifd_layouts_missing_tags_and_types(spp, channels):
    cases = _by_samples(T.ifd_dialects())[spp, channels]
    assert sum(c[0] in T.NO_ARBITER for c in cases) == (6 if spp == 1 else 3)
    _group(cases, 40, 70, channels, pitch_pad=7, base_offset=5)


@pytest.mark.parametrize("channels", [1, 3])
def test_the_long_constant_pages(channels):
    """the cut page first: what its second strip writes behind its 1650 rows lands in the next page's first rows"""
    by = {c[0]: c for c in T.long_constant()}
    cases = [by["long-constant-rows+"], by["long-constant-libtiff"], by["long-constant-late"]]
    _group(cases, T.LONG_ROWS + T.LONG_CUT, T.LONG_COLS, channels, pitch_pad=4, base_offset=4)


def test_pins_between_good_neighbours():
    pins = T.pins()
    good = T.policy_dialects(1)[200]
    rgb = T.policy_dialects(3)[100]
    for channels in (1, 3):
        neighbour = good if channels == 1 else rgb
        streams, shapes = [neighbour[1]], [(0, 0)]
        for _, s, code in pins:
            streams += [s, neighbour[1]]
            shapes += [tuple(R.parse(s)[k] for k in ("rows", "cols")) if code == -215 else (0, 0), (0, 0)]
        imgs, size, rc = decode_on_device(streams, 35, 259, channels, pitch_pad=7, base_offset=5, shapes=shapes)
        for i in range(0, len(streams), 2):
            assert rc[i] == 0
            _same(imgs[i], _want(neighbour, channels), "the good neighbour %d" % i)
        for k, (name, s, code) in enumerate(pins):  # an RGB pin in a gray call: -213 as well
            assert rc[2 * k + 1] == code and tuple(size[2 * k + 1]) == (0, 0), (name, int(rc[2 * k + 1]))


def test_through_imread_next_to_a_jpeg_a_png_and_a_bilevel_tiff():
    import fuzz_jpeg_decode as fz
    import png_ref as P
    import tiff_cases
    rgb = synth.make_color_card(64, 48, 3, 2.0)[0]
    g4 = tiff_ref.pillow_tiff(tiff_cases.content("text", 30, 100, seed=3))
    def pick(cases, *parts):
        return next(c for c in cases if all(p in c[0] for p in parts))
    gray, colour = T.policy_dialects(1), T.policy_dialects(3)
    cases = [pick(gray, "-short-rows+-", "-33x"), pick(gray, "-cadence-300-overrun-", "-33x"), pick(gray, "-literal-254-junk-", "-33x"),
             pick(colour, "-cap-3-", "-33x6"), pick(colour, "-cadence-800-", "-33x257"), pick(T.cut_dialects(), "cut-lzw-cadence-300-rows+", "rps5"),
             T.cut_dialects()[-1], pick(T.period_dialects(), "period-64-spp1"), pick(T.packbits_dialects(), "crossing", "x3-"),
             pick(T.ifd_dialects(), "ifd-lzw2-rgb-no-counts-reverse-gaps"), pick(T.ifd_dialects(), "ifd-raw-rgb-no-278-no-279"),
             pick(T.ifd_dialects(), "ifd-lzw-gray-no-277-278-279-shuffled")]
    streams = [fz.make_stream(rgb, 95, subsampling=2)] + [c[1] for c in cases] + [P.write(np.ascontiguousarray(rgb[..., ::-1]), 2, 8), g4]
    imgs, size, rc = decode_on_device(streams, 66, 259, 3, pitch_pad=2, base_offset=1, fn=imread.decode_batch_device)
    assert (rc == 0).all(), rc
    _same(imgs[0], fz.pillow_decode(streams[0], 3), "jpeg")
    _same(imgs[-2], rgb, "png")
    _same(imgs[-1], np.repeat(tiff_ref.pillow_read(g4)[..., None], 3, axis=2), "bilevel")
    for i, case in enumerate(cases):
        _same(imgs[1 + i], _want(case, 3), case[0])


def test_through_the_projection_streams_flow():
    """the flow fed foreign forms of three gray sheets returns what it returns for their libtiff forms: angles as f64 bits,
    indices, output streams byte for byte"""
    lib, foreign, sheets = [], [], []
    for k, (rows, cols, seed, skew, rps) in enumerate(((120, 90, 80, 4.0, 40), (150, 199, 64, -6.0, 32))):
        gray = np.ascontiguousarray(synth.make_color_card(rows, cols, seed, skew)[0][..., 1])
        sheets.append(gray)
        lib.append(R.pillow_tiff(gray, "tiff_lzw", rps))
        foreign.append(T.write(gray, "short", "rows+", rps, seed=5 + k, order=">", ifd_first=True, reverse=True))
        assert foreign[k][:2] == b"MM" and (R.pillow_read(foreign[k]) == gray).all() and (R.pillow_read(lib[k]) == gray).all()
    packed = tiff_ref.assemble(120, 90, [t6_rewrap.packbits_encode(sheets[0].tobytes(), "crossing")], 32773, photometric=1, drop=(279,),
                               extra=[(258, 3, [8])])
    assert (R.pillow_read(packed) == sheets[0]).all()
    sweep = (10, 0.5, 0.5)
    a0, i0, r0, o0 = projection.deskew_streams(lib + [lib[0]], *sweep, interp=1, quality=95, want_idx=True)
    a1, i1, r1, o1 = projection.deskew_streams(foreign + [packed], *sweep, interp=1, quality=95, want_idx=True)
    assert list(r0) == [0, 0, 0] and list(r1) == [0, 0, 0]
    assert (np.asarray(a0, np.float64).view(np.uint64) == np.asarray(a1, np.float64).view(np.uint64)).all() and list(i0) == list(i1)
    for k in range(3):
        assert o0[k] == o1[k], (k, "the output streams differ")
