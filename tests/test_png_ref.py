"""The PNG decoder's restatement (png_ref.py) against Pillow and zlib: every writer variant Pillow can read, the crafted
deflate blocks, and seeded mutations of small streams.  No GPU."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as P  # noqa: E402

SHAPES = [(1, 1), (1, 9), (7, 9), (8, 8), (15, 17), (37, 53), (64, 48), (65, 33), (130, 5)]
FILTERS = [0, 1, 2, 3, 4, ("first", 1), ("first", 2), ("first", 3), ("first", 4), "rotate"]
CONTENTS = ("noise", "flat", "ruled")


def palette_of(depth, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (1 << depth, 3), dtype=np.uint8)


def content(rows, cols, color_type, depth, kind, seed=0):
    """samples for the writer: noise, one value, or ruled lines on a flat ground"""
    rng = np.random.default_rng(seed * 7919 + rows * 131 + cols)
    top = 1 << depth
    n = P.SAMPLES[color_type]
    shape = (rows, cols) if n == 1 else (rows, cols, n)
    if kind == "noise":
        return rng.integers(0, top, shape, dtype=np.uint8 if depth == 8 else np.int64).astype(np.uint8)
    a = np.full(shape, top - 1 if kind == "ruled" else top // 2, np.uint8)
    if kind == "ruled":
        a[::4] = 0
        a[:, ::7] = top // 3
    return a


def pillow(stream, channels=3):
    im = Image.open(io.BytesIO(stream))
    im.load()
    if channels == 1:
        return np.asarray(im.convert("L"))
    return np.asarray(im.convert("RGB"))[..., ::-1]


def critical_only(stream):
    """the stream without its ancillary chunks: Pillow checks their CRC, libpng (and so imread) only warns"""
    out, p = stream[:8], 8
    while p < len(stream):
        n = int.from_bytes(stream[p:p + 4], "big")
        if not stream[p + 4] & 0x20:
            out += stream[p:p + 12 + n]
        p += 12 + n
    return out


def variants():
    """(name, stream, color_type) over shapes x taken types x filters x contents: every pair of the three appears"""
    k = 0
    for rows, cols in SHAPES:
        for ct, depth in P.TAKEN:
            for f in FILTERS:
                kind = CONTENTS[k % 3]
                pal = palette_of(depth) if ct == 3 else None
                arr = content(rows, cols, ct, depth, kind, seed=k)
                yield "%dx%d ct%d d%d f%s %s" % (rows, cols, ct, depth, f, kind), P.write(arr, ct, depth, pal, filters=f), ct
                k += 1


DEFLATE_FORMS = [dict(level=0), dict(strategy=zlib.Z_FIXED), dict(), dict(flush_every=200), dict(wbits=9), dict(level=9, wbits=12)]


def test_restatement_equals_pillow_on_every_writer_variant():
    n = 0
    for name, s, ct in variants():
        for ch in (3, 1):
            code, img = P.decode(s, ch)
            if ch == 1 and ct not in (0, 4):
                assert code == P.NOTIMPL, name
                continue
            assert code == 0, name
            assert np.array_equal(img, pillow(s, ch)), (name, ch)
            n += 1
    assert n > 1000


def test_deflate_forms_and_idat_cuts():
    arr = content(37, 53, 2, 8, "ruled")
    want = arr[..., ::-1]
    for z in DEFLATE_FORMS:
        for cuts in (None, 1, 7, [0, 1, 0, 5, 0]):
            s = P.write(arr, 2, 8, filters="rotate", cuts=cuts, **z)
            code, img = P.decode(s)
            assert code == 0 and np.array_equal(img, want), (z, cuts)
            assert np.array_equal(pillow(s), want)
    s = P.write(arr, 2, 8, before_idat=[(b"gAMA", b"\x00\x00\xb1\x8f"), (b"tEXt", b"k\x00v")], after_idat=[(b"tIME", b"\x07\xe6\x01\x01\x00\x00\x00")])
    assert np.array_equal(P.decode(s)[1], want)
    # ancillary chunks are skipped without a CRC check
    bad = P.assemble(37, 53, 2, 8, P.deflate(P.filter_rows(P.pack_rows(arr, 2, 8), 3, 0)), before_idat=[])
    i = bad.index(b"IDAT") - 4
    bad = bad[:i] + P.chunk(b"tEXt", b"k\x00v", crc=1) + bad[i:]
    assert P.decode(bad)[0] == 0


def test_inflate_equals_zlib_on_the_crafted_blocks():
    rng = np.random.default_rng(3)
    raw = bytes(rng.integers(0, 15, 300, dtype=np.uint8) * 16 + 3)
    for zs in (P.crafted_15bit(raw), P.crafted_crossing(bytes(rng.integers(0, 256, 300, dtype=np.uint8)))):
        out = zlib.decompress(zs)
        assert P.inflate(zs, len(out)) == out
    assert zlib.decompress(P.crafted_15bit(raw)) == raw
    w = P.BitWriter()
    P.fixed_block(w, [65, 66, 67, (258, 3), (3, 1), (10, 264)])
    out = zlib.decompressobj(-15).decompress(w.done())
    assert len(out) == 274 and P.inflate(P.zlib_wrap(w.done(), out), 274) == out
    w = P.BitWriter()
    P.fixed_block(w, [65, (3, 2)])
    with pytest.raises(P.Damaged):
        P.inflate(P.zlib_wrap(w.done(), b"A"), 4)
    with pytest.raises(zlib.error):
        zlib.decompress(P.zlib_wrap(w.done(), b"A"))


def test_code_set_rules_are_zlibs():
    ok = [[1], [1, 1], [0, 0, 0], [2, 2, 2, 2], [1, 2, 3, 3]]
    bad = [[1, 1, 1], [2], [2, 2, 2], [1, 2], [3]]
    for lens in ok:
        P._Huff(lens)
    for lens in bad:
        with pytest.raises(P.Damaged):
            P._Huff(lens)
    with pytest.raises(P.Damaged):
        P._Huff([1], codes=True)


def test_whenever_the_restatement_returns_an_image_pillow_returns_the_same():
    """mutations of whole files (a CRC guards the critical chunks, none the ancillary ones) and of the zlib stream inside
    intact chunks (only inflate and Adler-32 guard those)"""
    rng = np.random.default_rng(11)
    seeds = []
    for ct, depth in [(0, 8), (2, 8), (3, 4), (0, 1), (6, 8)]:
        arr = content(9, 11, ct, depth, "ruled", seed=ct)
        raw = P.filter_rows(P.pack_rows(arr, ct, depth), P.bpp_of(ct, depth), "rotate")
        for z in (dict(level=0), dict(strategy=zlib.Z_FIXED), dict()):
            seeds.append((ct, depth, palette_of(depth) if ct == 3 else None, P.deflate(raw, **z)))
    text = [(b"tEXt", b"Comment\x00" + bytes(80))]
    images = refused = 0
    for k in range(700):
        ct, depth, pal, zs = seeds[(k // 6) % len(seeds)]
        how, inside = k % 3, (k // 3) % 2
        s = bytearray(zs if inside else P.assemble(9, 11, ct, depth, zs, pal, before_idat=text, after_idat=text))
        at = int(rng.integers(2 if inside else 8, len(s) + inside))
        if how == 0:
            s[min(at, len(s) - 1)] ^= 1 << int(rng.integers(0, 8))
        elif how == 1:
            s = s[:at]
        else:
            s[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        s = P.assemble(9, 11, ct, depth, bytes(s), pal) if inside else bytes(s)
        code, img = P.decode(s)
        if code:
            refused += 1
            continue
        images += 1
        assert np.array_equal(img, pillow(critical_only(s))), k
        h = P.parse(s)[1]
        assert len(zlib.decompressobj().decompress(h.idat)) == h.rows * (1 + P.row_bytes(h))
    assert images > 20 and refused > 300, (images, refused)
