"""omr_tiff_info_ex / omr_imread_info on 8-bit gray and RGB TIFF streams, no GPU: every accepted variant reports what the
restatement's parser reports, every new refusal has its code, and the refusals test_tiff_decode_abi.py pins keep theirs."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import tiff8_ref as R  # noqa: E402
import tiff_cases  # noqa: E402
import tiff_ref  # noqa: E402
from oics import imread, tiff  # noqa: E402
from oics._lib import SYMBOLS as _PROTOTYPES, OmrError  # noqa: E402

SYMBOLS = ("omr_tiff_info_ex", "omr_tiff_decode_stats_ex")


def _code(fn, *a):
    try:
        fn(*a)
        return 0
    except OmrError as e:
        return e.code


def test_symbols_in_header_ctypes_and_shim():
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header) and s in _PROTOTYPES and "pub fn %s(" % s in ffi, s
    assert "#define OMR_TIFF_DECODE_STAGES 6" in header and len(tiff.STAGES_EX) == 6
    # the old call keeps its four stages
    assert len(tiff.STAGES) == 4 and tiff.stats(False)[1] == [0.0] * 4 and tiff.stats_ex(False)[1] == [0.0] * 6


def _variants():
    for spp in (1, 3):
        a = R.content("text", 9, 21, spp, seed=spp)
        for comp, name, pred in ((5, "tiff_lzw", 1), (5, "tiff_lzw", 2), (32773, "packbits", 1), (1, "raw", 1)):
            yield a, R.pillow_tiff(a, name, 4, pred)
            for order in "<>":
                for photometric in ((0, 1) if spp == 1 else (2,)):
                    yield a, R.write(a, comp, 4, pred, photometric=photometric, order=order)


def test_accepted_variants_report_what_the_restatement_reports():
    n = 0
    for a, s in _variants():
        h = R.parse(s)
        assert tiff.info_ex(s) == (h["rows"], h["cols"], h["compression"], h["photometric"], 1, len(h["strips"]), 8, h["spp"], h["predictor"])
        assert tiff.info(s) == tiff.info_ex(s)[:6]
        assert imread.info(s) == (9, 21, 1 if a.ndim == 2 else 3, 1, imread.OMR_IMREAD_KIND_TIFF)
        n += 1
    assert n == 2 * 4 + 4 * 2 * 3
    g4 = tiff_ref.pillow_tiff(tiff_cases.content("text", 20, 100, seed=1), "group4", 8)
    assert tiff.info_ex(g4)[6:] == (1, 1, 1)


def _gray(comp=5, **kw):
    a = R.content("text", 9, 21, 1, seed=1)
    return R.write(a, comp, 4, **kw)


def _rgb(comp=5, **kw):
    return R.write(R.content("text", 9, 21, 3, seed=1), comp, 4, **kw)


def _old_style():
    a = R.content("text", 9, 21, 1, seed=1)
    return R.write(a, 5, 4, strip_codes={1: lambda raw: b"\x00\x01" + R.lzw_encode(raw)})


NEW_REFUSALS = [
    ("Deflate", lambda: _gray(extra=[(259, 3, [8])]), -213),
    ("old Deflate", lambda: _gray(extra=[(259, 3, [32946])]), -213),
    ("JPEG", lambda: _rgb(extra=[(259, 3, [7])]), -213),
    ("palette", lambda: _gray(extra=[(262, 3, [3]), (320, 3, [0] * 768)]), -213),
    ("16 bits", lambda: _gray(extra=[(258, 3, [16])]), -213),
    ("8,8,16", lambda: _rgb(extra=[(258, 3, [8, 8, 16])]), -213),
    ("alpha", lambda: _rgb(extra=[(277, 3, [4]), (258, 3, [8] * 4), (338, 3, [2])]), -213),
    ("ExtraSamples", lambda: _rgb(extra=[(338, 3, [0])]), -213),
    ("planar 2", lambda: _rgb(extra=[(284, 3, [2])]), -213),
    ("RGB with photometric 1", lambda: _rgb(extra=[(262, 3, [1])]), -213),
    ("gray with photometric 2", lambda: _gray(extra=[(262, 3, [2])]), -213),
    ("old-style LZW", _old_style, -213),
    ("LZW at 1 bit", lambda: _gray(extra=[(258, 3, [1])]), -213),
    ("T.6 at 8 bits", lambda: _gray(extra=[(259, 3, [4])]), -213),
    ("fill order 2 at 8 bits", lambda: _gray(extra=[(266, 3, [2])]), -213),
    ("predictor 3", lambda: _gray(extra=[(317, 3, [3])]), -213),
    ("orientation 3", lambda: _gray(extra=[(274, 3, [3])]), -213),
    ("tiles", lambda: _gray(extra=[(322, 3, [16]), (323, 3, [16])]), -213),
    ("a raw strip one byte short", lambda: tiff_ref.assemble(2, 5, [bytes(29)], 1, photometric=2, extra=[(258, 3, [8, 8, 8]), (277, 3, [3])]), -5),
]


@pytest.mark.parametrize("name,make,code", NEW_REFUSALS, ids=[r[0] for r in NEW_REFUSALS])
def test_new_refusals(name, make, code):
    s = make()
    assert _code(tiff.info_ex, s) == code and _code(tiff.info, s) == code and _code(imread.info, s) == code
    with pytest.raises(R.Refused) as e:
        R.parse(s)
    assert e.value.code == code


def test_a_raw_strip_of_exactly_its_rows_is_taken():
    s = tiff_ref.assemble(2, 5, [bytes(30)], 1, photometric=2, extra=[(258, 3, [8, 8, 8]), (277, 3, [3])])
    assert tiff.info_ex(s)[6:] == (8, 3, 1)


def test_the_bilevel_refusal_table_keeps_its_answers():
    import test_tiff_decode_abi as old
    base = old._base()
    h = tiff_ref.parse(base)
    for name, kw, code in old.REFUSALS:
        s = tiff_ref.assemble(20, 100, tiff_ref.strips_of(base), 4, **dict(dict(photometric=h["photometric"], rps=8), **kw))
        assert _code(tiff.info, s) == code and _code(tiff.info_ex, s) == code, name
        with pytest.raises(R.Refused) as e:
            R.parse(s)
        assert e.value.code == code, name


def test_every_prefix_and_flipped_byte_of_an_lzw_file_is_answered_as_the_restatement_answers():
    base = R.write(R.content("text", 4, 7, 3, seed=2), 5, 2, 2)
    for n in range(len(base)):
        assert _code(tiff.info_ex, base[:n]) in (0, -5, -213, -215)
    for i in range(len(base)):
        for m in (0xff, 0x01, 0x08):
            s = base[:i] + bytes([base[i] ^ m]) + base[i + 1:]
            c = _code(tiff.info_ex, s)
            try:
                R.parse(s)
                assert c == 0, (i, m)
            except R.Refused as e:
                assert c == e.code, (i, m, c, e.code)


def test_refused_files_and_an_rgb_file_asked_as_gray_need_no_device():
    rgb, gray = _rgb(), _gray()
    assert _code(tiff.decode, rgb, 1) == -213 and _code(imread.info, rgb) == 0
    size, rc = tiff.decode_batch_device([rgb, _gray(extra=[(259, 3, [8])]), gray[:30]], 1, 4096, 9 * 21, 21, 9, 21)
    assert list(rc) == [-213, -213, -5] and (size == 0).all()
    size, rc = imread.decode_batch_device([rgb, _old_style()], 1, 4096, 9 * 21, 21, 9, 21)
    assert list(rc) == [-213, -213] and (size == 0).all()
    size, rc = tiff.decode_batch_device([rgb], 3, 4096, 8 * 63, 63, 8, 21)  # too large for the slot
    assert list(rc) == [-5]
