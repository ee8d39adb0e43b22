"""numpy restatement of libjpeg's baseline encoder as `jpeg_set_defaults` + `jpeg_set_quality(q, TRUE)` leaves it
(what OpenCV's imwrite(.., JPEG) and Pillow's save(format="JPEG") run): csrc/jpeg.hip is held to it stage by stage,
and it is held to Pillow's bytes (tests/test_jpeg_ref.py).  Stages, each a function of its own:

  quant_tables   jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
  header         SOI, JFIF APP0, DQT per table, SOF0, DHT per table, SOS
  components     rgb_ycc_convert (16-bit fixed point), edge replication, h2v2_downsample
  fdct_quant     samples - 128, jfdctint.c (CONST_BITS 13, PASS1_BITS 2), jcdctmgr.c's rounding division
  scan_blocks    the blocks in scan order with jccoefct.c's dummy blocks: (component, zig-zag coefficients)
  block_bits     jchuff.c's encode_one_block: the code bits of one block
  entropy        DC differences, the bit string, padding with 1-bits, 0xFF stuffing
"""
import numpy as np

# Annex K.1 / K.2 base tables, natural order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, np.int64)

# Annex K.3 - K.6: (bits[1..16], huffval)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order)


ZIGZAG = _zigzag()   # ZIGZAG[k] = natural index of the k-th coefficient in zig-zag order (jpeg_natural_order)


def quant_tables(quality):
    """(luma, chroma), natural order, as jpeg_set_quality(quality, TRUE) leaves them."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16) for base in (BASE_LUMA, BASE_CHROMA))


def huff_codes(table):
    """{symbol: (code, length)} of one DHT table (jchuff.c jpeg_make_c_derived_tbl)."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(rows, cols, channels, quality):
    """SOI .. SOS, as jcmarker.c writes them for a 1- or 3-component baseline image."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8)))
    if channels == 3:
        out += _seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    dims = rows.to_bytes(2, "big") + cols.to_bytes(2, "big")
    if channels == 3:
        out += _seg(0xC0, b"\x08" + dims + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
    else:
        out += _seg(0xC0, b"\x08" + dims + b"\x01\x01\x11\x00")
    tabs = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if channels == 3 else [])
    for ident, (bits, vals) in tabs:
        out += _seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    if channels == 3:
        out += _seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")
    else:
        out += _seg(0xDA, b"\x01\x01\x00\x00\x3f\x00")
    return out


def _ceil(a, b):
    return -(-a // b)


def components(img):
    """The component planes the DCT reads, each a whole number of its 8 x 8 blocks wide and of iMCU rows high.
    gray: [Y].  BGR: [Y, Cb, Cr] with Cb, Cr at half size (h2v2_downsample).  The right edge is replicated in the source
    (expand_right_edge before the down-sampler), the bottom by repeating the last row of the *down-sampled* component
    (expand_bottom_edge after it) -- for an even height that is not the average of two copies of the last source row."""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    if img.ndim == 2:
        ys = np.minimum(np.arange(_ceil(rows, 8) * 8), rows - 1)
        xs = np.minimum(np.arange(_ceil(cols, 8) * 8), cols - 1)
        return [img[np.ix_(ys, xs)].astype(np.int64)]
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mcu_rows = _ceil(rows, 16)
    ys = np.minimum(np.arange(mcu_rows * 16), rows - 1)
    xs = np.minimum(np.arange(_ceil(cols, 8) * 8), cols - 1)
    out = [y[np.ix_(ys, xs)]]
    crows, ccols = _ceil(rows, 2), _ceil(cols, 2)
    cwb = _ceil(ccols, 8)
    cy = np.minimum(np.arange(mcu_rows * 8), crows - 1)      # bottom: repeat the last down-sampled row
    y0, y1 = np.minimum(2 * cy, rows - 1), np.minimum(2 * cy + 1, rows - 1)
    cx = np.arange(cwb * 8)
    x0, x1 = np.minimum(2 * cx, cols - 1), np.minimum(2 * cx + 1, cols - 1)
    bias = 1 + (cx & 1)                                      # 1, 2, 1, 2, ... from 1 in every row
    for c in (cb, cr):
        s = c[np.ix_(y0, x0)] + c[np.ix_(y0, x1)] + c[np.ix_(y1, x0)] + c[np.ix_(y1, x1)] + bias[None, :]
        out.append(s >> 2)
    return out


_F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069,
          c2053=16819, c2562=20995, c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint.c over the last axis of d (.., 8)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _F["c0541"]
    out[..., 2] = _descale(z1 + t13 * _F["c0765"], n)
    out[..., 6] = _descale(z1 - t12 * _F["c1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F["c1175"]
    t4, t5, t6, t7 = t4 * _F["c0298"], t5 * _F["c2053"], t6 * _F["c3072"], t7 * _F["c1501"]
    z1, z2 = -z1 * _F["c0899"], -z2 * _F["c2562"]
    z3, z4 = -z3 * _F["c1961"] + z5, -z4 * _F["c0390"] + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_quant(plane, qtab):
    """(block rows, block cols, 64) quantised coefficients of a component plane, zig-zag order."""
    h, w = plane.shape
    blocks = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).astype(np.int64)
    d = _fdct_pass(blocks, True)                                  # rows
    d = _fdct_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)    # columns
    div = (qtab.astype(np.int64) * 8).reshape(8, 8)
    mag = (np.abs(d) + (div >> 1)) // div
    q = np.where(d < 0, -mag, mag)
    return q.reshape(h // 8, w // 8, 64)[..., ZIGZAG]


def scan_blocks(img, quality):
    """[(component index, 64 zig-zag coefficients)] in scan order.  Interleaved 4:2:0: per MCU Y00 Y01 Y10 Y11 Cb Cr, where
    a Y block past the component's real size in blocks is a dummy: AC all zero, DC = that of the block before it in its
    row of the MCU (right edge) or of the last block of the MCU's row above (bottom edge: both blocks of the row)."""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    ql, qc = quant_tables(quality)
    planes = components(img)
    if img.ndim == 2:
        c = fdct_quant(planes[0], ql)
        return [(0, c[by, bx]) for by in range(_ceil(rows, 8)) for bx in range(_ceil(cols, 8))]
    yq, cbq, crq = fdct_quant(planes[0], ql), fdct_quant(planes[1], qc), fdct_quant(planes[2], qc)
    bw, bh = _ceil(cols, 8), _ceil(rows, 8)
    out = []
    for my in range(_ceil(rows, 16)):
        for mx in range(_ceil(cols, 16)):
            mcu = []
            for yi in range(2):
                for xi in range(2):
                    by, bx = 2 * my + yi, 2 * mx + xi
                    if by < bh and bx < bw:
                        blk = yq[by, bx]
                    else:
                        blk = np.zeros(64, np.int64)
                        blk[0] = mcu[-1][0] if by < bh else mcu[1][0]
                    mcu.append(blk)
            out += [(0, b) for b in mcu] + [(1, cbq[my, mx]), (2, crq[my, mx])]
    return out


def _nbits(v):
    return int(v).bit_length()


def block_bits(blk, dc_diff, dc_codes, ac_codes):
    """The code bits of one block as a '0'/'1' string."""
    out = []

    def emit(code, n):
        if n:
            out.append(format(code & ((1 << n) - 1), "0%db" % n))

    def value(v):
        n = _nbits(abs(v))
        emit(v if v >= 0 else v - 1, n)

    n = _nbits(abs(dc_diff))
    emit(*dc_codes[n])
    value(dc_diff)
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            emit(*ac_codes[0xF0])
            run -= 16
        emit(*ac_codes[(run << 4) | _nbits(abs(v))])
        value(v)
        run = 0
    if run:
        emit(*ac_codes[0x00])
    return "".join(out)


def entropy(blocks, channels):
    """The entropy-coded segment: the bit string of every block, padded with 1-bits, 0xFF followed by 0x00."""
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    last = [0, 0, 0]
    parts = []
    for comp, blk in blocks:
        t = 0 if comp == 0 else 1
        parts.append(block_bits(blk, int(blk[0]) - last[comp], dc[t], ac[t]))
        last[comp] = int(blk[0])
    bits = "".join(parts)
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def encode(img, quality):
    """The whole file, SOI to EOI.  img: (rows, cols) gray or (rows, cols, 3) BGR, uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] == 3)
    channels = 1 if img.ndim == 2 else 3
    return header(img.shape[0], img.shape[1], channels, quality) + entropy(scan_blocks(img, quality), channels) + b"\xff\xd9"
