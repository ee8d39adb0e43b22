"""EXIF orientation for the tests: a numpy restatement of the eight transforms (OpenCV's ExifTransform, Pillow's
ImageOps.exif_transpose), a builder of an APP1 EXIF segment in either byte order, and a splice of it into a JPEG stream."""
import struct

import numpy as np

CODES = (1, 2, 3, 4, 5, 6, 7, 8)
TRANSPOSING = (5, 6, 7, 8)


def apply(img, code):
    """img [rows, cols] or [rows, cols, cn] turned by `code`; the bytes of a pixel keep their order"""
    t = np.swapaxes(img, 0, 1)
    out = {1: img,
           2: img[:, ::-1],              # flip left-right
           3: img[::-1, ::-1],           # turn by 180 degrees
           4: img[::-1],                 # flip top-bottom
           5: t,                         # transpose
           6: t[:, ::-1],                # transpose, then flip left-right: 90 degrees clockwise
           7: t[::-1, ::-1],             # transpose, then flip both: transverse
           8: t[::-1]}[code]             # transpose, then flip top-bottom: 90 degrees counter-clockwise
    return np.ascontiguousarray(out)


def turned_shape(rows, cols, code):
    return (cols, rows) if code in TRANSPOSING else (rows, cols)


def tiff_orientation(code, little_endian=True):
    """a TIFF block (what APP1 carries behind "Exif\\0\\0" and a PNG's eXIf chunk as a whole) with IFD0 = one entry,
    Orientation (0x0112, SHORT, count 1) = code"""
    e = "<" if little_endian else ">"
    head = (b"II*\x00" if little_endian else b"MM\x00*") + struct.pack(e + "I", 8)
    ifd = struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, code, 0) + struct.pack(e + "I", 0)
    return head + ifd


def app1(code, little_endian=True):
    """the APP1 segment, marker and length included"""
    body = b"Exif\x00\x00" + tiff_orientation(code, little_endian)
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def tag_jpeg(stream, code, little_endian=True):
    """the JPEG stream with an EXIF orientation spliced in right behind SOI (where cameras put it)"""
    assert stream[:2] == b"\xff\xd8"
    return stream[:2] + app1(code, little_endian) + stream[2:]


def tag_png(stream, code, little_endian=True):
    """the PNG stream with an eXIf chunk behind IHDR"""
    import zlib
    assert stream[:8] == b"\x89PNG\r\n\x1a\n" and stream[12:16] == b"IHDR"
    body = tiff_orientation(code, little_endian)
    chunk = struct.pack(">I", len(body)) + b"eXIf" + body + struct.pack(">I", zlib.crc32(b"eXIf" + body))
    return stream[:33] + chunk + stream[33:]
