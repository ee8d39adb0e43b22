"""A plain Python / numpy restatement of the Group 4 TIFF encoder (csrc/oics_tiff_enc.cpp, csrc/tiff_enc.hip): the
threshold, libtiff's Fax3Encode2DRow rule for one row, the strips with their EOFB, and the file's layout.  The run-length
code tables are not restated: they come from the library's own dump (omr_tiff_code_tables, host only), as in tiff_ref.py.
Nothing here shares code with the kernels: find() looks a position up in the list of the row's changes."""
import bisect
import functools
import struct

import numpy as np

_CODES = None

PASS = (0b0001, 4)
HORIZONTAL = (0b001, 3)
# a1 - b1 -> (code, bits)
VERTICAL = {0: (0b1, 1), 1: (0b011, 3), 2: (0b000011, 6), 3: (0b0000011, 7), -1: (0b010, 3), -2: (0b000010, 6), -3: (0b0000010, 7)}
EOFB = "000000000001" * 2


def codes():
    """[white, black]: {run: (code, bits)}"""
    global _CODES
    if _CODES is None:
        from oics import tiff
        _CODES = [{r: (c, b) for r, c, b in tiff.code_tables(k)} for k in (0, 1)]
    return _CODES


def gray_of(img):
    """the project's gray of a BGR image in memory order (bgr.hpp, oracle.rgb2gray): byte 0 takes the R weight"""
    a = np.asarray(img).astype(np.uint32)
    return ((a[..., 0] * 9798 + a[..., 1] * 19235 + a[..., 2] * 3735 + 16384) >> 15).astype(np.uint8)


def threshold(img, thr):
    """-> uint8 [rows, cols], 1 = black: a pixel is white iff its gray value is greater than thr"""
    a = np.asarray(img)
    g = a if a.ndim == 2 else gray_of(a)
    return (g <= thr).astype(np.uint8)


class _Row:
    """a row's pixels and the positions where it changes colour, so that find() need not walk pixel by pixel"""

    def __init__(self, px):
        self.px = [int(v) for v in px]
        self.n = len(self.px)
        self.changes = [x for x in range(1, self.n) if self.px[x] != self.px[x - 1]]

    def __getitem__(self, x):
        return self.px[x]


def _find(row, s, c, n):
    """the first position >= s whose pixel differs from c, or n"""
    if s >= n:
        return n
    if row.px[s] != c:
        return s
    i = bisect.bisect_right(row.changes, s)
    return row.changes[i] if i < len(row.changes) else n


def _span(out, k, colour):
    tab = codes()[colour]
    while k >= 2624:
        out.append(tab[2560])
        k -= 2560
    if k >= 64:
        out.append(tab[k & ~63])
        k &= 63
    out.append(tab[k])


def row_codes(bp, rp):
    """one row against its reference row -> [(code, bits)], and the steps taken"""
    bp, rp = _Row(bp), _Row(rp)
    n = bp.n
    out = []
    a0 = 0
    a1 = 0 if bp[0] else _find(bp, 0, 0, n)
    b1 = 0 if rp[0] else _find(rp, 0, 0, n)
    steps = 0
    while True:
        steps += 1
        b2 = _find(rp, b1, rp[b1], n) if b1 < n else n
        if b2 >= a1:
            d = b1 - a1
            if d < -3 or d > 3:
                a2 = _find(bp, a1, bp[a1], n) if a1 < n else n
                out.append(HORIZONTAL)
                if a0 + a1 == 0 or bp[a0] == 0:
                    _span(out, a1 - a0, 0)
                    _span(out, a2 - a1, 1)
                else:
                    _span(out, a1 - a0, 1)
                    _span(out, a2 - a1, 0)
                a0 = a2
            else:
                out.append(VERTICAL[a1 - b1])
                a0 = a1
        else:
            out.append(PASS)
            a0 = b2
        if a0 >= n:
            break
        c = bp[a0]
        a1 = _find(bp, a0, c, n)
        b1 = _find(rp, a0, 1 - c, n)
        b1 = _find(rp, b1, c, n)
    return out, steps


def _bitstring(cs):
    return "".join("{:0{}b}".format(c, b) for c, b in cs)


@functools.lru_cache(maxsize=4096)
def _row_bits(bp, rp):
    return _bitstring(row_codes(bp, rp)[0])


def row_bits(bp, rp):
    return _row_bits(bytes(bytearray(int(v) for v in bp)), bytes(bytearray(int(v) for v in rp)))


def strip(bits):
    """bits: uint8 [rows, cols], 1 = black -> the strip's bytes: every row under the one above, the first under a white
    line, EOFB, zeros to a byte"""
    s = ""
    ref = np.zeros(bits.shape[1], np.uint8)
    for r in range(bits.shape[0]):
        s += row_bits(bits[r], ref)
        ref = bits[r]
    s += EOFB
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")


def strips(bits, rps):
    rows = bits.shape[0]
    rps = rows if rps <= 0 else min(rps, rows)
    return rps, [strip(bits[r:r + rps]) for r in range(0, rows, rps)]


def assemble(rows, cols, rps, strip_bytes, dpi=0):
    """the file: "II" 42, the IFD at 8, tags ascending, the resolutions, the two strip arrays (inside their entries for one
    strip), the strips at even offsets; nothing behind the last strip"""
    ns = len(strip_bytes)
    nt = 13 if dpi > 0 else 10
    ifd_end = 8 + 2 + 12 * nt + 4
    res_at = ifd_end
    arrays_at = ifd_end + (16 if dpi > 0 else 0)
    data_at = arrays_at + (8 * ns if ns > 1 else 0)
    offs, at = [], data_at
    for s in strip_bytes:
        offs.append(at)
        at += len(s) + (len(s) & 1)
    counts = [len(s) for s in strip_bytes]
    SHORT, LONG, RATIONAL = 3, 4, 5

    def entry(tag, typ, count, value):
        return struct.pack("<HHI", tag, typ, count) + (struct.pack("<HH", value, 0) if typ == SHORT else struct.pack("<I", value))
    e = [entry(256, LONG, 1, cols), entry(257, LONG, 1, rows), entry(258, SHORT, 1, 1), entry(259, SHORT, 1, 4),
         entry(262, SHORT, 1, 0), entry(273, LONG, ns, arrays_at if ns > 1 else offs[0]), entry(277, SHORT, 1, 1),
         entry(278, LONG, 1, rps), entry(279, LONG, ns, arrays_at + 4 * ns if ns > 1 else counts[0])]
    if dpi > 0:
        e += [entry(282, RATIONAL, 1, res_at), entry(283, RATIONAL, 1, res_at + 8)]
    e.append(entry(293, LONG, 1, 0))
    if dpi > 0:
        e.append(entry(296, SHORT, 1, 2))
    assert len(e) == nt
    out = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", nt) + b"".join(e) + struct.pack("<I", 0)
    if dpi > 0:
        out += struct.pack("<IIII", dpi, 1, dpi, 1)
    if ns > 1:
        out += struct.pack("<%dI" % ns, *offs) + struct.pack("<%dI" % ns, *counts)
    assert len(out) == data_at
    for k, s in enumerate(strip_bytes):
        out += s + (b"\0" if len(s) & 1 and k + 1 < ns else b"")
    return out


def encode_bits(bits, rows_per_strip=0, dpi=0):
    """bits: uint8 [rows, cols], 1 = black -> the file"""
    bits = np.asarray(bits, np.uint8)
    rps, ss = strips(bits, rows_per_strip)
    return assemble(bits.shape[0], bits.shape[1], rps, ss, dpi)


def encode(img, thr=127, rows_per_strip=0, dpi=0):
    """img: uint8 [rows, cols] gray or [rows, cols, 3] BGR -> the file omr_tiff_encode writes"""
    return encode_bits(threshold(img, thr), rows_per_strip, dpi)


def row_bound(cols):
    """bits of one row's code at most (csrc/oics_tiff_enc.cpp has the argument)"""
    return 7 * cols + 32


def bound(rows, cols, rows_per_strip=0):
    """omr_tiff_bound, restated"""
    rps = rows if rows_per_strip <= 0 else min(rows_per_strip, rows)

    def strip_max(r):
        b = (r * row_bound(cols) + 24 + 7) // 8
        return b + (b & 1)
    full, rest = divmod(rows, rps)
    return 186 + 8 * (full + (1 if rest else 0)) + full * strip_max(rps) + (strip_max(rest) if rest else 0)
