"""The 8-bit gray and RGB TIFF encoder restated in plain Python / numpy, the whole file: the head,
the strip split, the RGB order, Predictor 2, the serial LZW with its Clear rule, EOI, the pads and the even offsets.  The
device's files equal encode() byte for byte (tests/test_gpu_tiff8_encode.py); test_tiff8_enc_ref.py proves that libtiff
(Pillow) and the decoder's restatement (tiff8_ref.py) read these files back as the picture.

The LZW rule.  Codes most significant bit first; Clear (256) first, 9 bits; then the codes of the longest matches, the
code with index i since the last Clear at width(i) bits (9 for i < 254, 10 for i < 766, 11 for i < 1790, else 12) and
adding entry 258 + i; Clear again as the code with index CLEAR_AT = 3836, and only there -- libtiff's writer's point,
when entry 4093 has been made; the strip's last match is a code like any other (a Clear follows it if it has index 3835);
then EOI at the width of the index it stands at; then zeros to a byte."""
import struct

import numpy as np

CLEAR, EOI, FIRST = 256, 257, 258
CLEAR_AT = 3836
DEFAULT_STRIP = 8192
HEAD_MAX = 8 + 2 + 12 * 14 + 4 + 16 + 8


def width(i):
    return 9 + (i >= 254) + (i >= 766) + (i >= 1790)


def lzw_codes(raw):
    """bytes -> [(code, index since the last Clear)], the leading Clear (index None) and EOI among them"""
    raw = bytes(raw)
    out = [(CLEAR, None)]
    tab, i, w = {}, 0, b""

    def send(code):
        nonlocal i, tab
        out.append((code, i))
        i += 1
        if i == CLEAR_AT:
            out.append((CLEAR, i))
            i, tab = 0, {}
            return True
        return False
    for b in raw:
        wb = w + bytes([b])
        if len(wb) == 1 or wb in tab:
            w = wb
            continue
        entry = FIRST + i
        if not send(w[0] if len(w) == 1 else tab[w]):
            tab[wb] = entry
        w = bytes([b])
    if w:
        send(w[0] if len(w) == 1 else tab[w])
    out.append((EOI, i))
    return out


def lzw_strip(raw):
    acc, nb, out = 0, 0, bytearray()
    for code, i in lzw_codes(raw):
        w = 9 if i is None else width(i)
        acc, nb = (acc << w) | code, nb + w
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 0xff)
            nb -= 8
        acc &= (1 << nb) - 1
    if nb:
        out.append((acc << (8 - nb)) & 0xff)
    return bytes(out)


def code_counts(raw):
    """the number of codes between two Clears (Clear and EOI not counted), per stretch"""
    counts, n = [], 0
    for code, i in lzw_codes(raw)[1:]:
        if code == CLEAR or code == EOI:
            counts.append(n)
            n = 0
        else:
            n += 1
    return counts


def pairless_noise(n, seed):
    """n <= 4000 noise bytes in which no pair of neighbours occurs twice: every code but the first Clear and EOI is a literal,
    so a strip of n of them has exactly n codes since its Clear (plain noise of 1790 bytes repeats some twenty pairs)"""
    rng = np.random.RandomState(seed)
    out, seen = [int(rng.randint(0, 256))], set()
    while len(out) < n:
        b = int(rng.randint(0, 256))
        if (out[-1], b) not in seen:
            seen.add((out[-1], b))
            out.append(b)
    return np.array(out, np.uint8)


def rows_of_strip(rows, cols, cn, rows_per_strip=0):
    if rows_per_strip > 0:
        return min(rows_per_strip, rows)
    return min(rows, max(1, DEFAULT_STRIP // (cols * cn)))


def raw_strips(img, predictor=1, rows_per_strip=0):
    """a gray [rows, cols] or BGR [rows, cols, 3] image -> the strips' raw bytes: samples R, G, B; Predictor 2: every sample
    minus the same sample of the pixel on its left, mod 256, a row's first pixel as it is"""
    a = np.asarray(img, np.uint8)
    cn = 1 if a.ndim == 2 else 3
    rows, cols = a.shape[:2]
    px = a.reshape(rows, cols, cn)[:, :, ::-1].astype(np.int64)
    if predictor == 2:
        px = np.concatenate([px[:, :1], px[:, 1:] - px[:, :-1]], axis=1) % 256
    flat = px.astype(np.uint8).reshape(rows, cols * cn)
    rps = rows_of_strip(rows, cols, cn, rows_per_strip)
    return [flat[r:r + rps].tobytes() for r in range(0, rows, rps)], rps


def head(rows, cols, cn, compression, predictor, rps, ns, dpi):
    """-> (the first bytes up to the strip arrays, where StripOffsets' and StripByteCounts' values stand, the first strip's
    offset)"""
    tags = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, cn, None if cn == 3 else 8), (259, 3, 1, compression),
            (262, 3, 1, 2 if cn == 3 else 1), (273, 4, ns, None), (277, 3, 1, cn), (278, 4, 1, rps), (279, 4, ns, None)]
    if dpi > 0:
        tags += [(282, 5, 1, None), (283, 5, 1, None), (296, 3, 1, 2)]
    if cn == 3:
        tags.append((284, 3, 1, 1))
    if predictor == 2:
        tags.append((317, 3, 1, 2))
    tags.sort()
    ifd_end = 8 + 2 + 12 * len(tags) + 4
    res_at = ifd_end
    bps_at = res_at + (16 if dpi > 0 else 0)
    arrays_at = bps_at + (8 if cn == 3 else 0)
    h = bytearray(arrays_at)
    h[:8] = b"II" + struct.pack("<HI", 42, 8)
    struct.pack_into("<H", h, 8, len(tags))
    off_pos = cnt_pos = None
    for k, (tag, typ, count, value) in enumerate(tags):
        at = 10 + 12 * k
        struct.pack_into("<HHI", h, at, tag, typ, count)
        if tag == 258 and cn == 3:
            value = bps_at
        elif tag == 282:
            value = res_at
        elif tag == 283:
            value = res_at + 8
        elif tag == 273:
            value, off_pos = (arrays_at, arrays_at) if ns > 1 else (0, at + 8)
        elif tag == 279:
            value, cnt_pos = (arrays_at + 4 * ns, arrays_at + 4 * ns) if ns > 1 else (0, at + 8)
        if typ == 3 and count == 1:
            struct.pack_into("<H", h, at + 8, value)
        else:
            struct.pack_into("<I", h, at + 8, value)
    if dpi > 0:
        struct.pack_into("<IIII", h, res_at, dpi, 1, dpi, 1)
    if cn == 3:
        struct.pack_into("<HHH", h, bps_at, 8, 8, 8)
    return h, off_pos, cnt_pos, arrays_at + (8 * ns if ns > 1 else 0)


def encode(img, compression=5, predictor=1, rows_per_strip=0, dpi=0):
    a = np.asarray(img, np.uint8)
    cn = 1 if a.ndim == 2 else 3
    rows, cols = a.shape[:2]
    assert compression in (1, 5) and predictor in (1, 2) and not (predictor == 2 and compression == 1)
    raws, rps = raw_strips(a, predictor, rows_per_strip)
    strips = [lzw_strip(r) if compression == 5 else r for r in raws]
    ns = len(strips)
    h, off_pos, cnt_pos, data_at = head(rows, cols, cn, compression, predictor, rps, ns, dpi)
    out = bytearray(h) + bytearray(data_at - len(h))
    for k, s in enumerate(strips):
        if len(out) & 1:
            out.append(0)
        struct.pack_into("<I", out, off_pos + 4 * k, len(out))
        struct.pack_into("<I", out, cnt_pos + 4 * k, len(s))
        out += s
    return bytes(out)


def strip_bound(n, compression):
    """bytes of a strip of n raw bytes at most: n codes at most, a Clear in front and behind every 3836 of them, EOI, 12
    bits each, the pad"""
    return (12 * (n + n // CLEAR_AT + 2) + 7) // 8 if compression == 5 else n


def bound(rows, cols, cn, compression, rows_per_strip=0):
    rps = rows_of_strip(rows, cols, cn, rows_per_strip)
    b = HEAD_MAX + 8 * ((rows + rps - 1) // rps)
    for r in range(0, rows, rps):
        b += (strip_bound(min(rps, rows - r) * cols * cn, compression) + 1) & ~1
    return b
