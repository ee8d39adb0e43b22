"""A PNG writer with every knob the decoder's tests need, a tiny deflate block writer for code sets no compressor emits,
and a restatement of the decoder's rules (omrdeskew.h, the PNG section): chunk walk, bit-serial inflate by zlib's rules for
code sets, Adler-32, the five filters and imread's conversion.  Pure Python, numpy and the standard library's zlib."""
import struct
import zlib

import numpy as np

OK, BADARG, NOTIMPL, ASSERT = 0, -5, -213, -215
SIGNATURE = b"\x89PNG\r\n\x1a\n"
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
MAX_SIDE, MAX_PIXELS = 1 << 20, 1 << 30  # imread's own limits: a larger image is refused (ASSERT)
# every colour type / depth the decoder takes
TAKEN = [(0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (4, 8), (6, 8)]


# ---------------------------------------------------------------------------------------------------------- writer
def chunk(kind, data=b"", crc=None):
    c = zlib.crc32(kind + data) & 0xffffffff if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", c)


def ihdr(rows, cols, color_type, depth, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, depth, color_type, compression, filt, interlace))


def pack_rows(arr, color_type, depth):
    """samples [rows, cols(, samples)] -> the packed rows, uint8 [rows, row_bytes]"""
    a = np.asarray(arr)
    rows, cols = a.shape[:2]
    a = a.reshape(rows, cols * SAMPLES[color_type]).astype(np.uint8)
    if depth == 8:
        return a
    per = 8 // depth
    pad = (-a.shape[1]) % per
    a = np.concatenate([a, np.zeros((rows, pad), np.uint8)], axis=1).reshape(rows, -1, per)
    out = np.zeros(a.shape[:2], np.uint8)
    for j in range(per):
        out |= (a[:, :, j] & ((1 << depth) - 1)) << (8 - depth * (j + 1))
    return out


def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(packed, bpp, filters):
    """filters: one type for all rows, a list per row, "rotate" (row r gets r % 5) or ("first", t) (t on row 0, else 0)"""
    rows, rb = packed.shape
    if filters == "rotate":
        types = [r % 5 for r in range(rows)]
    elif isinstance(filters, tuple):
        types = [filters[1]] + [0] * (rows - 1)
    elif isinstance(filters, int):
        types = [filters] * rows
    else:
        types = list(filters)
    out = bytearray()
    prev = np.zeros(rb, np.int32)
    for r in range(rows):
        cur = packed[r].astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        t = types[r]
        if t == 0 or t > 4:
            pred = np.zeros(rb, np.int32)
        elif t == 1:
            pred = left
        elif t == 2:
            pred = prev
        elif t == 3:
            pred = (left + prev) >> 1
        else:
            pa, pb, pc = abs(prev - ul), abs(left - ul), abs(left + prev - 2 * ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def deflate(raw, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=0):
    """flush_every: a Z_FULL_FLUSH (an empty stored block) behind every that many bytes"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if not flush_every:
        return co.compress(raw) + co.flush()
    out = b""
    for i in range(0, len(raw), flush_every):
        out += co.compress(raw[i:i + flush_every]) + co.flush(zlib.Z_FULL_FLUSH)
    return out + co.flush()


def cut(zs, cuts):
    """the zlib stream as IDAT payloads: None (one chunk), an int (chunks of that size), or a list of sizes (0 allowed; the
    rest goes into a last chunk)"""
    if cuts is None:
        return [zs]
    if isinstance(cuts, int):
        return [zs[i:i + cuts] for i in range(0, len(zs), cuts)] or [b""]
    out, at = [], 0
    for c in cuts:
        out.append(zs[at:at + c])
        at += c
    return out + [zs[at:]]


def assemble(rows, cols, color_type, depth, zs, palette=None, cuts=None, before_idat=(), after_idat=(), interlace=0, iend=True):
    s = SIGNATURE + ihdr(rows, cols, color_type, depth, interlace)
    if palette is not None:
        s += chunk(b"PLTE", palette if isinstance(palette, bytes) else np.asarray(palette, np.uint8).tobytes())
    for kind, data in before_idat:
        s += chunk(kind, data)
    for piece in cut(zs, cuts):
        s += chunk(b"IDAT", piece)
    for kind, data in after_idat:
        s += chunk(kind, data)
    return s + (chunk(b"IEND") if iend else b"")


def bpp_of(color_type, depth):
    return max(1, SAMPLES[color_type] * depth // 8)


def write(arr, color_type, depth=8, palette=None, filters=0, cuts=None, before_idat=(), after_idat=(), **z):
    """arr: samples [rows, cols] (colour types 0 and 3: values below 2^depth) or [rows, cols, 2 / 3 / 4]; z: deflate()'s"""
    rows, cols = np.asarray(arr).shape[:2]
    raw = filter_rows(pack_rows(arr, color_type, depth), bpp_of(color_type, depth), filters)
    return assemble(rows, cols, color_type, depth, deflate(raw, **z), palette, cuts, before_idat, after_idat)


# ------------------------------------------------------------------------------------- the crafted deflate blocks
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):  # a value, lowest bit first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code, first bit first
        for k in range(n - 1, -1, -1):
            self.bits(c >> k & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of a list of code lengths"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code that has all 19 symbols
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _runs(seq):
    """the lengths of both sets as ONE sequence -> code-length symbols; a run goes on across the border of the sets"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11, 7))
                n -= k
            if n >= 3:
                out.append((17, n - 3, 3))
                n = 0
        else:
            out.append((v, 0, 0))
            n -= 1
            while n >= 3:
                k = min(n, 6)
                out.append((16, k - 3, 2))
                n -= k
        out += [(v, 0, 0)] * n
        i = j
    return out


def dynamic_literal_block(w, data, lit_lens, dist_lens, final=True):
    """one dynamic block of literals alone into BitWriter w: lit_lens [257 .. 286] (data's bytes and 256 must have codes),
    dist_lens [1 .. 30]"""
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for sym, extra, nbits in _runs(list(lit_lens) + list(dist_lens)):
        w.code(*cl[sym])
        w.bits(extra, nbits)
    codes = canonical(lit_lens)
    for b in data:
        w.code(*codes[b])
    w.code(*codes[256])


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def fixed_block(w, symbols, final=True):
    """symbols: ints (literals) and (length, distance) pairs"""
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    codes = canonical(FIXED_LIT)
    for s in symbols:
        if isinstance(s, int):
            w.code(*codes[s])
            continue
        n, d = s
        k = max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28 or n < 258))
        w.code(*codes[257 + k])
        w.bits(n - LEN_BASE[k], LEN_EXTRA[k])
        k = max(i for i in range(30) if DIST_BASE[i] <= d)
        w.code(k, 5)
        w.bits(d - DIST_BASE[k], DIST_EXTRA[k])
    w.code(*codes[256])


def zlib_wrap(deflated, raw, adler=None):
    a = zlib.adler32(raw) & 0xffffffff if adler is None else adler
    return b"\x78\x9c" + deflated + struct.pack(">I", a)


def lens_15bit(symbols):
    """code lengths 1, 2, .., 14, 15, 15 over the 16 given symbols (256 among them): a complete set with 15-bit codes"""
    assert len(symbols) == 16 and 256 in symbols
    lens = [0] * 257
    for k, s in enumerate(symbols):
        lens[s] = min(k + 1, 15)
    return lens


def crafted_15bit(raw):
    """raw (bytes over at most 15 distinct values) as one dynamic block with 15-bit codes and a one-code distance set"""
    vals = sorted(set(raw))
    assert len(vals) <= 15
    vals += [v for v in range(256) if v not in vals][:15 - len(vals)]
    w = BitWriter()
    dynamic_literal_block(w, raw, lens_15bit(vals[:7] + [256] + vals[7:]), [1])
    return zlib_wrap(w.done(), raw)


def crafted_crossing(raw):
    """raw as one dynamic block whose literal lengths end in zeros that a repeat code carries on into the distance lengths:
    286 literal / length lengths (257 .. 285 are 0), 30 distance lengths of which only the last is set"""
    lens = [8] * 256 + [0] * 30  # 256 codes of 8 bits would fill the space: 254 of them, two of 9 and the end code on 8
    lens[254] = lens[255] = 9
    lens[256] = 8
    dist = [0] * 29 + [1]
    w = BitWriter()
    dynamic_literal_block(w, raw, lens, dist)
    assert _runs(lens + dist) != _runs(lens) + _runs(dist), "the zero run must cross the border"
    return zlib_wrap(w.done(), raw)


# ------------------------------------------------------------------------------------------------ the restatement
class Header:
    rows = cols = color_type = depth = npal = 0
    palette = None
    idat = b""
    critical_ok = True


def _exif_orientation(t):
    if len(t) < 8:
        return 1
    if t[:4] == b"II*\x00":
        e = "<"
    elif t[:4] == b"MM\x00*":
        e = ">"
    else:
        return 1
    ifd = struct.unpack(e + "I", t[4:8])[0]
    if ifd + 2 > len(t):
        return 1
    cnt = struct.unpack(e + "H", t[ifd:ifd + 2])[0]
    for k in range(cnt):
        o = ifd + 2 + 12 * k
        if o + 12 > len(t):
            break
        if struct.unpack(e + "H", t[o:o + 2])[0] == 0x0112:
            return struct.unpack(e + "H", t[o + 8:o + 10])[0]
    return 1


def row_bytes(h):
    return (h.cols * SAMPLES[h.color_type] * h.depth + 7) // 8


def parse(s):
    """-> (code, Header or None): the header is there whenever IHDR was readable"""
    s = bytes(s)
    if len(s) < 8 or s[:8] != SIGNATURE:
        return BADARG, None
    h = None
    have_plte = have_iend = apng = idat_open = False
    pieces = []
    interlace, orient, p = 0, 1, 8
    crc_ok = True
    while p < len(s):
        if p + 12 > len(s):
            return BADARG, h
        n = struct.unpack(">I", s[p:p + 4])[0]
        kind, body = s[p + 4:p + 8], s[p + 8:p + 8 + n]
        if p + 12 + n > len(s):
            return BADARG, h
        if h is None and kind != b"IHDR":
            return BADARG, None
        if not kind[0] & 0x20 and zlib.crc32(kind + body) & 0xffffffff != struct.unpack(">I", s[p + 8 + n:p + 12 + n])[0]:
            crc_ok = False
        if kind != b"IDAT" and pieces:
            idat_open = False
        if kind == b"IHDR":
            if h is not None or n != 13:
                return BADARG, h
            cols, rows, d, ct, comp, filt, il = struct.unpack(">IIBBBBB", body)
            if cols == 0 or rows == 0 or cols > 0x7fffffff or rows > 0x7fffffff:
                return BADARG, None
            if not ((ct == 0 and d in (1, 2, 4, 8, 16)) or (ct == 3 and d in (1, 2, 4, 8)) or (ct in (2, 4, 6) and d in (8, 16))):
                return BADARG, None
            if comp or filt or il > 1:
                return BADARG, None
            h = Header()
            h.rows, h.cols, h.color_type, h.depth, interlace = rows, cols, ct, d, il
        elif kind == b"PLTE":
            if n == 0 or n % 3 or n > 768 or have_plte or pieces:
                return BADARG, h
            have_plte, h.npal, h.palette = True, n // 3, np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            if pieces and not idat_open:
                return BADARG, h
            idat_open = True
            pieces.append(body)
        elif kind == b"IEND":
            have_iend = True
            break
        elif not kind[0] & 0x20:
            return BADARG, h
        elif kind == b"acTL":
            apng = apng or not pieces
        elif kind == b"eXIf":
            o = _exif_orientation(body)
            orient = o if o != 1 else orient
        p += 12 + n
    if h is None or not pieces:
        return BADARG, h
    if h.color_type == 3 and not have_plte:
        return BADARG, h
    h.idat = b"".join(pieces)
    z = h.idat[:2]
    if len(z) < 2 or z[0] & 15 != 8 or z[0] >> 4 > 7 or z[1] & 0x20 or (z[0] << 8 | z[1]) % 31:
        return BADARG, h
    if interlace or h.depth == 16 or apng or orient != 1:
        return NOTIMPL, h
    if not have_iend or h.cols > MAX_SIDE or h.rows > MAX_SIDE or h.rows * h.cols > MAX_PIXELS:
        return ASSERT, h
    if h.rows * (1 + row_bytes(h)) >= 1 << 32 or len(h.idat) >= 1 << 28:
        return ASSERT, h
    h.critical_ok = crc_ok
    return OK, h


class Damaged(Exception):
    pass


class _Huff:
    def __init__(self, lens, codes=False):
        self.count = [0] * 16
        for n in lens:
            self.count[n] += 1
        self.count[0] = 0
        left, longest = 1, 0
        for n in range(1, 16):
            left = left * 2 - self.count[n]
            if left < 0:
                raise Damaged("over-subscribed")
            if self.count[n]:
                longest = n
        if left > 0 and longest != 0 and (codes or longest != 1):
            raise Damaged("incomplete")
        offs = [0] * 16
        for n in range(1, 15):
            offs[n + 1] = offs[n] + self.count[n]
        self.symbol = [0] * sum(self.count)
        for s, n in enumerate(lens):
            if n:
                self.symbol[offs[n]] = s
                offs[n] += 1


class _Reader:
    def __init__(self, data, limit):
        self.d, self.pos, self.limit = data, 0, limit * 8

    def bit(self):
        if self.pos >= self.limit:
            raise Damaged("input running out")
        v = self.d[self.pos >> 3] >> (self.pos & 7) & 1
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for k in range(n):
            v |= self.bit() << k
        return v

    def symbol(self, h):
        code = first = index = 0
        for n in range(1, 16):
            code |= self.bit()
            c = h.count[n]
            if code - c < first:
                return h.symbol[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise Damaged("invalid code")


def inflate(zs, want):
    """the zlib stream zs (header already checked) -> exactly `want` bytes, or Damaged"""
    if len(zs) < 6:
        raise Damaged("input running out")
    r = _Reader(zs, len(zs) - 4)
    r.pos = 16
    out = bytearray()
    last = 0
    while not last:
        last, kind = r.bit(), r.bits(2)
        if kind == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            if n != (~nn & 0xffff):
                raise Damaged("stored length")
            at = r.pos >> 3
            if at + n > len(zs) - 4:
                raise Damaged("input running out")
            if len(out) + n > want:
                raise Damaged("too long")
            out += zs[at:at + n]
            r.pos += 8 * n
            continue
        if kind == 3:
            raise Damaged("block type")
        if kind == 1:
            hl, hd = _Huff(FIXED_LIT), _Huff([5] * 32)
        else:
            nlen, ndist, ncode = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
            if nlen > 286 or ndist > 30:
                raise Damaged("too many symbols")
            cl = [0] * 19
            for i in range(ncode):
                cl[CL_ORDER[i]] = r.bits(3)
            hc = _Huff(cl, codes=True)
            lens = []
            while len(lens) < nlen + ndist:
                s = r.symbol(hc)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Damaged("repeat without a length")
                    rep, v = 3 + r.bits(2), lens[-1]
                elif s == 17:
                    rep, v = 3 + r.bits(3), 0
                else:
                    rep, v = 11 + r.bits(7), 0
                if len(lens) + rep > nlen + ndist:
                    raise Damaged("repeat past the end")
                lens += [v] * rep
            if lens[256] == 0:
                raise Damaged("no end-of-block code")
            hl, hd = _Huff(lens[:nlen]), _Huff(lens[nlen:])
        while True:
            s = r.symbol(hl)
            if s < 256:
                if len(out) >= want:
                    raise Damaged("too long")
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise Damaged("invalid length code")
                n = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
                d = r.symbol(hd)
                if d > 29:
                    raise Damaged("invalid distance code")
                d = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
                if d > len(out):
                    raise Damaged("distance too far back")
                if len(out) + n > want:
                    raise Damaged("too long")
                for _ in range(n):
                    out.append(out[-d])
    if len(out) != want:
        raise Damaged("too short")
    at = (r.pos + 7) >> 3
    if at + 4 > len(zs):
        raise Damaged("input running out")
    if struct.unpack(">I", zs[at:at + 4])[0] != zlib.adler32(bytes(out)) & 0xffffffff:
        raise Damaged("Adler-32")
    return bytes(out)


def unfilter(raw, rows, rb, bpp):
    out = np.zeros((rows, rb), np.uint8)
    prev = [0] * rb
    for r in range(rows):
        line = raw[r * (rb + 1):(r + 1) * (rb + 1)]
        t, cur = line[0], list(line[1:])
        if t > 4:
            raise Damaged("filter byte")
        for x in range(rb):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]
            cur[x] = (cur[x] + pred) & 255
        out[r] = cur
        prev = cur
    return out


def convert(h, rows_u8, channels):
    """imread's conversion of the unfiltered rows"""
    ct, d = h.color_type, h.depth
    if ct in (0, 3):
        if d < 8:
            per = 8 // d
            s = np.stack([(rows_u8 >> (8 - d * (j + 1))) & ((1 << d) - 1) for j in range(per)], axis=2)
            s = s.reshape(h.rows, -1)[:, :h.cols]
        else:
            s = rows_u8
        if ct == 3:
            if int(s.max()) >= h.npal:
                raise Damaged("palette index")
            return h.palette[s][..., ::-1].copy()
        g = (s * {1: 255, 2: 85, 4: 17, 8: 1}[d]).astype(np.uint8)
    elif ct == 4:
        g = rows_u8.reshape(h.rows, h.cols, 2)[..., 0]
    else:
        return rows_u8.reshape(h.rows, h.cols, SAMPLES[ct])[..., 2::-1].copy()
    return g.copy() if channels == 1 else np.repeat(g[..., None], 3, axis=2)


def decode(s, channels=3):
    """-> (code, image or None)"""
    code, h = parse(s)
    if code:
        return code, None
    if channels == 1 and h.color_type not in (0, 4):
        return NOTIMPL, None
    try:
        if not h.critical_ok:
            raise Damaged("CRC")
        rb = row_bytes(h)
        raw = inflate(h.idat, h.rows * (1 + rb))
        return OK, convert(h, unfilter(raw, h.rows, rb, bpp_of(h.color_type, h.depth)), channels)
    except Damaged:
        return ASSERT, None
