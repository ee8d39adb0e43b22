"""omr_tiff_info / omr_imread_info on bilevel TIFF streams, no GPU: every accepted variant reports what the restatement's
parser reports, every refusal has its code, and JPEG and PNG streams keep what omr_imread_info said about them."""
import os
import re
import struct
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import tiff_cases  # noqa: E402
import tiff_ref  # noqa: E402
from oics import imread, tiff  # noqa: E402
from oics._lib import SYMBOLS as _PROTOTYPES, OmrError  # noqa: E402

SYMBOLS = ("omr_tiff_info", "omr_tiff_code_tables", "omr_tiff_decode_batch_device", "omr_tiff_decode", "omr_tiff_decode_stats")


def _code(fn, *a):
    try:
        fn(*a)
        return 0
    except OmrError as e:
        return e.code


def _base():
    a = tiff_cases.content("text", 20, 100, seed=1)
    return tiff_ref.pillow_tiff(a, "group4", 8)


def test_symbols_in_header_ctypes_and_shim():
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header) and s in _PROTOTYPES and "pub fn %s(" % s in ffi, s
    assert "#define OMR_IMREAD_KIND_TIFF 2" in header and imread.OMR_IMREAD_KIND_TIFF == 2
    assert "pub fn decode_tiff(" in open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()


def test_accepted_variants_report_what_the_restatement_reports():
    seen = set()
    for name, s in tiff_cases.small_cases()[::7] + tiff_cases.long_run_cases():
        h = tiff_ref.parse(s)
        assert tiff.info(s) == (h["rows"], h["cols"], h["compression"], h["photometric"], h["fill_order"], len(h["strips"])), name
        assert imread.info(s) == (h["rows"], h["cols"], 1, 1, 2), name
        seen.add((h["compression"], h["photometric"], h["fill_order"], s[:2]))
    assert len(seen) == 3 * 2 * 2 * 2
    base = _base()
    for kw in (dict(drop=(258,)), dict(drop=(277,)), dict(drop=(258, 277)), dict(drop=(278,), rps=20), dict(offsets_type=3, counts_type=3),
               dict(drop=(293,)), dict(drop=(266,)), dict(drop=(279,)), dict(drop=(279,), reverse=True, gap=3), dict(drop=(279,), ifd_first=True), dict(extra=[(284, 3, [2])]), dict(extra=[(274, 3, [1])])):
        h = tiff_ref.parse(base)
        strips = tiff_ref.strips_of(base) if "rps" not in kw else [b"".join(tiff_ref.strips_of(tiff_ref.pillow_tiff(
            tiff_cases.content("text", 20, 100, seed=1), "group4", 20)))]
        s = tiff_ref.assemble(20, 100, strips, 4, **dict(dict(photometric=h["photometric"], rps=8), **kw))
        assert tiff.info(s)[:2] == (20, 100), kw
        assert (tiff_ref.decode(s) == tiff_ref.pillow_read(base)).all(), kw


REFUSALS = [
    ("BigTIFF", dict(big=True), -213),
    ("tiles", dict(extra=[(322, 3, [16]), (323, 3, [16])]), -213),
    ("depth 8", dict(extra=[(258, 3, [8])]), -213),
    ("three samples", dict(extra=[(277, 3, [3]), (258, 3, [1, 1, 1])]), -213),
    ("T.4", dict(extra=[(259, 3, [3])]), -213),
    ("LZW", dict(extra=[(259, 3, [5])]), -213),
    ("RGB photometric", dict(extra=[(262, 3, [2])]), -213),
    ("no photometric", dict(drop=(262,)), -213),
    ("uncompressed mode", dict(extra=[(293, 4, [2])]), -213),
    ("orientation 6", dict(extra=[(274, 3, [6])]), -213),
    ("zero width", dict(extra=[(256, 4, [0])]), -5),
    ("zero length", dict(extra=[(257, 4, [0])]), -5),
    ("no width", dict(drop=(256,)), -5),
    ("RowsPerStrip 0", dict(extra=[(278, 4, [0])]), -5),
    ("RowsPerStrip that disagrees with the strips", dict(extra=[(278, 4, [5])]), -5),
    ("no StripOffsets", dict(drop=(273,)), -5),
    ("one byte count for three strips", dict(extra=[(279, 4, [10])]), -5),
    ("an empty strip", dict(extra=[(279, 4, [0, 10, 10])]), -5),
    ("a strip offset beyond len", dict(extra=[(273, 4, [8, 1 << 20, 30])]), -5),
    ("a strip that runs past the end", dict(extra=[(279, 4, [10, 10, 1 << 20])]), -5),
    ("a tag of type ASCII", dict(extra=[(259, 2, [4])]), -5),
    ("a tag of type BYTE", dict(extra=[(259, 1, [4])]), -5),
    ("planar 2 with three samples", dict(extra=[(284, 3, [2]), (277, 3, [3])]), -213),
    ("fill order 3", dict(extra=[(266, 3, [3])]), -5),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, kw, code):
    base = _base()
    h = tiff_ref.parse(base)
    s = tiff_ref.assemble(20, 100, tiff_ref.strips_of(base), 4, **dict(dict(photometric=h["photometric"], rps=8), **kw))
    assert _code(tiff.info, s) == code
    if not kw.get("big"):
        assert _code(imread.info, s) == code
    with pytest.raises(tiff_ref.Refused) as e:
        tiff_ref.parse(s)
    assert e.value.code == code


def test_truncated_streams_and_wild_offsets():
    base = _base()
    for n in (0, 2, 4, 7):
        assert _code(tiff.info, base[:n]) == -5, n
    ifd = struct.unpack("<I", base[4:8])[0]
    assert _code(tiff.info, base[:ifd + 1]) == -5           # the IFD's count is cut
    assert _code(tiff.info, base[:ifd + 2 + 12 * 3]) == -5  # the IFD's entries are cut
    assert _code(tiff.info, base[:4] + struct.pack("<I", len(base) + 100) + base[8:]) == -5
    assert _code(tiff.info, base[:4] + struct.pack("<I", 0xfffffff0) + base[8:]) == -5
    wide = tiff_ref.assemble(1, 12289, [b"\x00"], 4)
    assert _code(tiff.info, wide) == -213                   # a T.6 line of more columns than the kernel's line buffers
    assert _code(tiff.info, tiff_ref.assemble(1, 12289, [bytes(1537)], 1)) == 0
    assert _code(tiff.info, tiff_ref.assemble(2, 100, [bytes(25)], 1)) == -5  # two raw rows need 26 bytes
    assert _code(tiff.info, tiff_ref.assemble(1 << 20, (1 << 10) + 1, [b"\0\0"], 4)) == -215


def test_every_prefix_and_every_flipped_byte_is_answered():
    """no prefix and no single damaged byte of a small file makes the parser read outside it or fail in another way"""
    base = tiff_ref.pillow_tiff(tiff_cases.content("stair", 4, 33), "group4", 2)
    for n in range(len(base)):
        assert _code(tiff.info, base[:n]) in (0, -5, -213, -215)
    for i in range(len(base)):
        s = base[:i] + bytes([base[i] ^ 0xff]) + base[i + 1:]
        c = _code(tiff.info, s)
        assert c in (0, -5, -213, -215)
        try:
            tiff_ref.parse(s)
            assert c == 0, i
        except tiff_ref.Refused as e:
            assert c == e.code, (i, c, e.code)


def test_imread_info_keeps_its_answers_for_jpeg_and_png():
    """the streams tests/test_imread_abi.py builds (its helpers, its picture), with the answers that file pins"""
    import orient_ref as O
    import png_ref as P
    import test_imread_abi as old
    png = P.write(old._rgb(), 2, 8)
    assert imread.info(old._jpeg()) == (37, 53, 3, 1, 0)
    assert imread.info(old._jpeg(gray=True)) == (37, 53, 1, 1, 0)
    assert imread.info(O.tag_jpeg(old._jpeg(), 6)) == (53, 37, 3, 6, 0)
    assert imread.info(O.tag_jpeg(old._jpeg(), 6), imread.IGNORE_ORIENTATION) == (37, 53, 3, 6, 0)
    assert imread.info(png) == (37, 53, 3, 1, 1)
    assert imread.info(P.write(old._rgb()[..., 0].copy(), 0, 8)) == (37, 53, 1, 1, 1)
    assert _code(imread.info, O.tag_png(png, 6)) == -213 and _code(imread.info, O.tag_jpeg(old._jpeg(), 9)) == -213
    assert _code(imread.info, old._jpeg(progressive=True)) == -213
    assert _code(imread.info, b"II+\0" + bytes(20)) == -5   # BigTIFF is not this layer's TIFF: it goes by the JPEG rules, as before
    assert _code(imread.info, b"\xff\xd8" + bytes(20)) == -5


def test_batch_entry_point_argument_errors_and_refusals_without_a_device():
    s = _base()
    tiled = tiff_ref.rewrap(s, extra=[(322, 3, [16]), (323, 3, [16])])
    # every stream refused: the codes are in rc and no device is needed
    size, rc = tiff.decode_batch_device([tiled, s[:20]], 3, 4096, 100 * 300, 300, 100, 100)
    assert list(rc) == [-213, -5] and (size == 0).all()
    size, rc = imread.decode_batch_device([tiled], 3, 4096, 100 * 300, 300, 100, 100)
    assert list(rc) == [-213]
    assert _code(tiff.decode_batch_device, [s], 2, 4096, 100 * 300, 300, 100, 100) == -5
    assert _code(tiff.decode_batch_device, [s], 3, 4096, 100 * 300, 299, 100, 100) == -5
    assert _code(tiff.decode_batch_device, [s], 3, 0, 100 * 300, 300, 100, 100) == -5
    size, rc = tiff.decode_batch_device([tiled, s], 3, 4096, 10 * 30, 30, 10, 10)   # too large for the slot: its own code
    assert list(rc) == [-213, -5]
    assert _code(tiff.code_tables, 0) == 0
