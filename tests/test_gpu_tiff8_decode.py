"""The device decoder on 8-bit gray and RGB TIFF (raw, PackBits, LZW; Predictor 1 and 2) against Pillow's libtiff and the
restatement (tiff8_ref.py), byte for byte, channels 1 and 3: the widths around the dword stores and the predictor's scan,
rows 1 to 70, every RowsPerStrip form, five contents, both byte orders and gray photometrics, strips that end on a byte and
one bit past it, every writer policy, a mixed imread call, damaged strips between good ones, and one A4 page."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import tiff8_ref as R  # noqa: E402
import tiff_ref  # noqa: E402
from oics import imread, tiff  # noqa: E402
from oics._lib import OmrError  # noqa: E402
from test_gpu_tiff_decode import _same, decode_on_device  # noqa: E402
from test_tiff8_ref import damaged_strips  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 63, 64, 65, 257)
ROWS = (1, 2, 7, 33, 70)
KINDS = ("noise", "constant", "period2", "text", "gradient")
FORMS = ((5, 1), (5, 2), (32773, 1), (1, 1))
_CASES = {}


def cases(spp):
    """[(name, stream, libtiff's picture)], built once: Pillow's reading of every stream is the restatement's"""
    if spp not in _CASES:
        out = []
        for wi, cols in enumerate(WIDTHS):
            for ri, rows in enumerate(ROWS):
                kind = KINDS[(wi + ri + spp) % len(KINDS)]
                a = R.content(kind, rows, cols, spp, seed=wi * 7 + ri)
                for fi, (comp, pred) in enumerate(FORMS):
                    for rps in sorted({1, min(7, rows), rows, rows // 2 + 1}):  # rows // 2 + 1: a short last strip
                        if rps == 1 and rows > 33:
                            continue
                        order = "<>"[(wi + ri + fi) & 1]
                        photometric = None if spp == 3 else (wi + fi + rps) & 1
                        s = R.write(a, comp, rps, pred, photometric=photometric, order=order, policy=R.POLICIES[(wi + ri) % 3], seed=wi + ri)
                        out.append(("%s %dx%dx%d comp %d pred %d rps %d %s ph %s" % (kind, rows, cols, spp, comp, pred, rps, order, photometric), s, a))
        # every content at one shape that spans waves and chunks, every policy; the 70 x 53 RGB noise image in one strip
        for kind in KINDS:
            a = R.content(kind, 70, 257, spp, seed=3)
            for pi, policy in enumerate(R.POLICIES):
                out.append(("%s policy %s" % (kind, policy), R.write(a, 5, 70, 1 + (pi & 1), policy=policy, seed=pi), a))
            out.append(("%s by Pillow" % kind, R.pillow_tiff(a, "tiff_lzw", 16, 2), a))
        a = R.content("noise", 70, 53, spp, seed=1)
        out += [("noise 70x53 policy %s" % p, R.write(a, 5, policy=p, seed=3), a) for p in R.POLICIES]
        wide = R.content("gradient", 2, 2500, spp, seed=1)  # more than two chunks of the finishing kernel
        out.append(("a wide row", R.write(wide, 5, 1, 2), wide))
        for name, s, a in out:
            assert (R.pillow_read(s) == a).all() and (R.decode(s) == a).all(), name
        _CASES[spp] = out
    return _CASES[spp]


@pytest.mark.parametrize("spp,channels", [(1, 1), (1, 3), (3, 3)])
def test_every_shape_form_and_content_in_one_call(spp, channels):
    cs = cases(spp)
    imgs, size, rc = decode_on_device([s for _, s, _ in cs], 70, 2500, channels, pitch_pad=5, base_offset=1)
    assert (rc == 0).all(), [(cs[i][0], int(rc[i])) for i in np.nonzero(rc)[0][:10]]
    for i, (name, s, a) in enumerate(cs):
        _same(imgs[i], R.as_output(a, channels), name)


def test_strips_that_end_on_a_byte_and_one_bit_past_it():
    found = {}
    rng = np.random.RandomState(4)
    for n in range(2, 400):
        a = rng.randint(0, 4, (1, n)).astype(np.uint8)
        bits = _bits(R.lzw_codes(a.tobytes(), "no_eoi"))
        if bits % 8 in (0, 1) and bits % 8 not in found:
            found[bits % 8] = (a, R.write(a, 5, policy="no_eoi"))
        if len(found) == 2:
            break
    assert len(found) == 2
    streams = [found[0][1], found[1][1]]
    for _, s in found.values():
        assert tiff.info_ex(s)[5] == 1
    imgs, size, rc = decode_on_device(streams, 1, 400, 1, pitch_pad=1, base_offset=3)
    assert (rc == 0).all(), rc
    for k in (0, 1):
        assert (R.pillow_read(streams[k]) == found[k][0]).all()
        _same(imgs[k], found[k][0], "ends %d bits past a byte" % k)


def _bits(codes):
    """the bits of a strip's codes, the first of them Clear"""
    i, n = 0, 9
    for c in codes[1:]:
        n += R.width(i)
        i = 0 if c == R.CLEAR else i + 1
    return n


def test_damaged_strips_between_good_ones():
    good = R.content("text", 24, 20, 1, seed=5)
    whole = R.write(good, 5, 8)
    bad = damaged_strips(good[8:16].tobytes())
    big = bad.pop("the table pushed past 4095")
    streams, shapes = [whole], [(24, 20)]
    for name, strip in bad.items():
        streams += [R.write(good, 5, 8, strip_codes={1: lambda raw, strip=strip: strip}), whole]
        shapes += [(24, 20), (24, 20)]
    streams += [tiff_ref.assemble(100, 100, [big], 5, photometric=1, extra=[(258, 3, [8])]), whole]
    shapes += [(100, 100), (24, 20)]
    for channels in (1, 3):
        imgs, size, rc = decode_on_device(streams, 100, 100, channels, pitch_pad=7, base_offset=5, shapes=shapes)
        for i in range(len(streams)):
            if i & 1:
                assert rc[i] == -215 and tuple(size[i]) == (0, 0), (i, rc[i])
            else:
                assert rc[i] == 0
                _same(imgs[i], R.as_output(good, channels), "the good neighbour %d" % i)


def test_imread_mixes_bilevel_gray_and_rgb_tiff_with_a_jpeg_and_a_png():
    import fuzz_jpeg_decode as fz
    import png_ref as P
    import tiff_cases
    from oics import synth
    rgb = synth.make_color_card(64, 48, 3, 2.0)[0]
    g4 = tiff_ref.pillow_tiff(tiff_cases.content("text", 30, 100, seed=3))
    gray = R.content("text", 41, 77, 1, seed=2)
    colour = R.content("gradient", 50, 33, 3, seed=2)
    streams = [g4, R.pillow_tiff(gray, "tiff_lzw", 8), R.write(colour, 5, 9, 2, order=">"), fz.make_stream(rgb, 95, subsampling=2),
               P.write(np.ascontiguousarray(rgb[..., ::-1]), 2, 8), R.pillow_tiff(colour, "raw"), R.pillow_tiff(gray, "packbits", 5)]
    assert imread.info(streams[2]) == (50, 33, 3, 1, imread.OMR_IMREAD_KIND_TIFF)
    imgs, size, rc = decode_on_device(streams, 66, 100, 3, pitch_pad=2, base_offset=1, fn=imread.decode_batch_device)
    assert list(rc) == [0] * 7
    g4_want = tiff_ref.pillow_read(g4)
    want = [np.repeat(g4_want[..., None], 3, axis=2), R.as_output(gray, 3), R.as_output(colour, 3), fz.pillow_decode(streams[3], 3), rgb,
            R.as_output(colour, 3), R.as_output(gray, 3)]
    for i in range(7):
        _same(imgs[i], want[i], "member %d" % i)
    # the same members asked for as gray: the RGB files are refused, the others are not touched by that
    imgs, size, rc = decode_on_device([streams[k] for k in (0, 1, 2, 5, 6)], 66, 100, 1, fn=imread.decode_batch_device)
    assert list(rc) == [0, 0, -213, -213, 0] and tuple(size[2]) == (0, 0)
    _same(imgs[0], g4_want, "bilevel, gray")
    _same(imgs[1], gray, "gray LZW, gray")
    _same(imgs[4], gray, "gray PackBits, gray")
    with pytest.raises(OmrError) as e:
        tiff.decode(streams[2], 1)
    assert e.value.code == -213
    _same(imread.decode(streams[2], 3), R.as_output(colour, 3), "omr_imread of an RGB TIFF")


def test_one_a4_gray_page_in_default_lzw_strips_and_in_one_raw_strip():
    page = R.content("text", 3508, 2480, 1, seed=7)
    lzw, raw = R.pillow_tiff(page, "tiff_lzw"), R.pillow_tiff(page, "raw", 3508)
    assert tiff.info_ex(lzw)[5] > 100 and tiff.info_ex(raw)[2:6:3] == (1, 1)
    tiff.stats_ex(True)
    _same(tiff.decode(lzw, 1), page, "LZW")
    groups, ms = tiff.stats_ex(False)
    assert groups == 1 and len(ms) == 6 and ms[3] > 0 and ms[5] > 0 and min(ms) >= 0
    _same(tiff.decode(raw, 1), page, "raw")
