"""A plain Python / numpy restatement of the bilevel TIFF decoder (csrc/oics_tiff_dec.cpp, csrc/tiff_dec.hip): the walk
over the first IFD with its refusals, T.6, PackBits and the unpack to 0 / 255 -- and a small TIFF assembler that wraps
strips with any tags and byte order, for the files Pillow cannot write.  The run-length code tables are not restated: they
come from the library's own dump (omr_tiff_code_tables, host only), so that the restatement, the kernel's lookup table and
the proof against Pillow in test_tiff_ref.py speak about one set of numbers."""
import io
import struct

import numpy as np

OK, BADARG, NOTIMPL, ASSERT = 0, -5, -213, -215
T6_MAX_COLS = 12288


class Refused(Exception):
    def __init__(self, code, why):
        Exception.__init__(self, "%d: %s" % (code, why))
        self.code = code


class Damaged(Exception):
    pass


_TABLES = None


def tables():
    """[white, black]: {(code, bits): run}"""
    global _TABLES
    if _TABLES is None:
        from oics import tiff
        _TABLES = [{(c, b): r for r, c, b in tiff.code_tables(k)} for k in (0, 1)]
    return _TABLES


# ---- the parser ------------------------------------------------------------------------------------------------------
def parse(s):
    """-> dict(rows, cols, compression, photometric, fill_order, rps, strips=[(off, len)]) or raises Refused"""
    s = bytes(s)
    n = len(s)
    if n < 4 or s[:2] not in (b"II", b"MM"):
        raise Refused(BADARG, "no byte-order mark")
    e = "<" if s[:2] == b"II" else ">"
    magic = struct.unpack(e + "H", s[2:4])[0]
    if magic == 43:
        raise Refused(NOTIMPL, "BigTIFF")
    if magic != 42:
        raise Refused(BADARG, "version")
    if n < 8:
        raise Refused(BADARG, "short header")
    ifd = struct.unpack(e + "I", s[4:8])[0]
    if ifd < 8 or ifd + 2 > n:
        raise Refused(BADARG, "IFD outside")
    cnt = struct.unpack(e + "H", s[ifd:ifd + 2])[0]
    if cnt == 0 or ifd + 2 + 12 * cnt > n:
        raise Refused(BADARG, "IFD entries outside")
    known = (256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 293)
    v = {259: 1, 262: -1, 266: 1, 274: 1, 278: 0xffffffff, 284: 1, 293: 0}
    bps, spp, tiles, arr = 1, 1, False, {}
    for k in range(cnt):
        at0 = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack(e + "HHI", s[at0:at0 + 8])
        if 322 <= tag <= 325:
            tiles = True
            continue
        if tag not in known:
            continue
        size = {3: 2, 4: 4, 1: 1}.get(typ, 0)
        if size == 0 or (size == 1 and tag != 258):
            raise Refused(BADARG, "tag type")
        if count < 1:
            raise Refused(BADARG, "tag without value")
        at = at0 + 8
        if count * size > 4:
            at = struct.unpack(e + "I", s[at0 + 8:at0 + 12])[0]
            if at < 8 or at > n or count * size > n - at:
                raise Refused(BADARG, "tag values outside")
        val = struct.unpack(e + {1: "B", 2: "H", 4: "I"}[size], s[at:at + size])[0]
        if tag in (273, 279):
            arr[tag] = (at, count, size)
        elif tag == 258:
            bps = val if count == 1 else -1
        elif tag == 277:
            spp = val
        else:
            if count != 1:
                raise Refused(BADARG, "tag with several values")
            v[tag] = val
    if tiles:
        raise Refused(NOTIMPL, "tiles")
    if bps != 1:
        raise Refused(NOTIMPL, "depth")
    if spp != 1:
        raise Refused(NOTIMPL, "samples")
    if v[259] not in (1, 4, 32773):
        raise Refused(NOTIMPL, "compression")
    if v[262] not in (0, 1):
        raise Refused(NOTIMPL, "photometric")
    if v[266] not in (1, 2):
        raise Refused(BADARG, "fill order")
    if v[259] == 4 and v[293] & 2:
        raise Refused(NOTIMPL, "uncompressed mode")
    if v[259] == 4 and v[293]:
        raise Refused(BADARG, "T6Options")
    if v[274] != 1:
        raise Refused(NOTIMPL, "orientation")
    rows, cols = v.get(257, 0), v.get(256, 0)
    if rows < 1 or cols < 1:
        raise Refused(BADARG, "size")
    if rows > 1 << 20 or cols > 1 << 20 or rows * cols > 1 << 30:
        raise Refused(ASSERT, "size limits")
    if v[259] == 4 and cols > T6_MAX_COLS:
        raise Refused(NOTIMPL, "T.6 width")
    if v[278] < 1:
        raise Refused(BADARG, "RowsPerStrip 0")
    rps = min(v[278], rows)
    ns = (rows + rps - 1) // rps
    if 273 not in arr:
        raise Refused(BADARG, "no strips")
    if arr[273][1] != ns or (279 in arr and arr[279][1] != ns):
        raise Refused(BADARG, "strip count")

    def value(t, k):
        return struct.unpack(e + {2: "H", 4: "I"}[arr[t][2]], s[arr[t][0] + arr[t][2] * k:arr[t][0] + arr[t][2] * (k + 1)])[0]
    offs = [value(273, k) for k in range(ns)]
    strips = []
    rb = (cols + 7) // 8
    for k in range(ns):
        off = offs[k]
        if 279 in arr:
            ln = value(279, k)
        else:  # no StripByteCounts: up to the next strip offset above this one, or to the stream's end
            ln = min([o for o in offs if o > off] or [n]) - off
        if ln < 1 or off < 8 or off > n or ln > n - off:
            raise Refused(BADARG, "strip outside")
        if ln >= 1 << 28:
            raise Refused(ASSERT, "strip length")
        if v[259] == 1 and ln < min(rps, rows - k * rps) * rb:
            raise Refused(BADARG, "short strip")
        strips.append((off, ln))
    return dict(rows=rows, cols=cols, compression=v[259], photometric=v[262], fill_order=v[266], rps=rps, strips=strips)


# ---- the decoders ----------------------------------------------------------------------------------------------------
_REV = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


class _Bits:
    def __init__(self, data, lsb):
        data = bytes(data)
        self.data = data.translate(_REV) if lsb else data
        self.n = 8 * len(data)
        self.pos = 0

    def peek(self, k=13):
        i = self.pos >> 3
        w = int.from_bytes(self.data[i:i + 3].ljust(3, b"\0"), "big")
        return (w >> (24 - k - (self.pos & 7))) & ((1 << k) - 1)

    def skip(self, k):
        """a code that begins inside the data may end behind it: its missing bits were read as zeros, as libtiff does"""
        if self.pos >= self.n:
            raise Damaged("input ends")
        self.pos += k


def _run(rd, colour, limit):
    tab = tables()[colour]
    total = 0
    while True:
        b = rd.peek()
        for bits in range(2, 14):
            r = tab.get((b >> (13 - bits), bits))
            if r is not None:
                break
        else:
            raise Damaged("no code")
        rd.skip(bits)
        total += r
        if total > limit:
            raise Damaged("run past the end")
        if r < 64:
            return total


def t6_decode(data, rows, cols, lsb=False, modes=None):
    """One strip -> uint8 [rows, cols], 1 inside a black run.  modes (a list): receives the mode of every code."""
    rd = _Bits(data, lsb)
    out = np.zeros((rows, cols), np.uint8)
    ref = []
    for y in range(rows):
        R = ref + [cols] * 8
        nr = len(ref)
        C = []
        a0, colour, ri = -1, 0, 0
        while a0 < cols:
            while ri < nr and R[ri] <= a0:
                ri += 2
            b1, b2 = R[ri], R[ri + 1]
            b = rd.peek()
            if b & 0x1000:
                rd.skip(1)
                v = 0
            elif b >> 10 == 3:
                rd.skip(3)
                v = 1
            elif b >> 10 == 2:
                rd.skip(3)
                v = -1
            elif b >> 10 == 1:
                rd.skip(3)
                s = max(a0, 0)
                a1 = s + _run(rd, colour, cols - s)
                a2 = a1 + _run(rd, colour ^ 1, cols - a1)
                if a1 <= a0 or (a2 <= a1 and a1 < cols):
                    raise Damaged("a run of 0")
                C += [p for p in (a1, a2) if p < cols]
                a0 = a2
                if modes is not None:
                    modes.append("H")
                continue
            elif b >> 9 == 1:
                rd.skip(4)
                a0 = b2
                ri += 2
                if modes is not None:
                    modes.append("P")
                continue
            elif b >> 7 == 3:
                rd.skip(6)
                v = 2
            elif b >> 7 == 2:
                rd.skip(6)
                v = -2
            elif b >> 6 == 3:
                rd.skip(7)
                v = 3
            elif b >> 6 == 2:
                rd.skip(7)
                v = -3
            else:
                raise Damaged("input ends" if rd.pos + 7 > rd.n else "invalid code")
            if modes is not None:
                modes.append("V%+d" % v if v else "V0")
            a1 = b1 + v
            if a1 <= a0 or a1 > cols:
                raise Damaged("a1 outside")
            if a1 < cols:
                C.append(a1)
            a0, colour = a1, colour ^ 1
            ri = ri - 1 if ri > 0 else ri + 1
        edges = C + ([cols] if len(C) & 1 else [])
        for k in range(0, len(edges), 2):
            out[y, edges[k]:edges[k + 1]] = 1
        ref = C
    return out


def packbits_decode(data, total, lsb=False):
    data = bytes(data).translate(_REV) if lsb else bytes(data)
    out = bytearray()
    p = 0
    while len(out) < total:
        if p >= len(data):
            raise Damaged("input ends")
        b = data[p]
        p += 1
        if b == 128:
            continue
        if b < 128:
            cnt = b + 1
            if cnt > len(data) - p:
                raise Damaged("input ends")
            if cnt > total - len(out):
                raise Damaged("past the rows")
            out += data[p:p + cnt]
            p += cnt
        else:
            cnt = 257 - b
            if p >= len(data):
                raise Damaged("input ends")
            if cnt > total - len(out):
                raise Damaged("past the rows")
            out += bytes([data[p]]) * cnt
            p += 1
    return bytes(out)


def decode(stream):
    """-> uint8 [rows, cols] of 0 / 255; raises Refused or Damaged"""
    h = parse(stream)
    rows, cols, rps = h["rows"], h["cols"], h["rps"]
    rb = (cols + 7) // 8
    lsb = h["fill_order"] == 2
    bits = np.zeros((rows, cols), np.uint8)
    for k, (off, ln) in enumerate(h["strips"]):
        r0 = k * rps
        nr = min(rps, rows - r0)
        data = bytes(stream[off:off + ln])
        if h["compression"] == 4:
            bits[r0:r0 + nr] = t6_decode(data, nr, cols, lsb)
            continue
        if h["compression"] == 32773:
            raw = packbits_decode(data, nr * rb, lsb)
        else:
            raw = data[:nr * rb].translate(_REV) if lsb else data[:nr * rb]
        a = np.unpackbits(np.frombuffer(raw, np.uint8).reshape(nr, rb), axis=1)[:, :cols]
        bits[r0:r0 + nr] = a
    return np.where(bits ^ (1 if h["photometric"] == 0 else 0), 255, 0).astype(np.uint8)


# ---- the assembler ---------------------------------------------------------------------------------------------------
def _layout(strips, reverse, gap, share, odd):
    """-> (each strip's offset in the blob, the blob): file order, gaps of 0xa5 bytes, equal strips stored once"""
    n = len(strips)
    rel, blob, seen = [0] * n, b"", {}
    for k in (range(n - 1, -1, -1) if reverse else range(n)):
        if share and strips[k] in seen:
            rel[k] = seen[strips[k]]
            continue
        if odd and len(blob) & 1:  # the blob stands at an odd offset: even offsets in it are odd in the file
            blob += b"\xa5"
        rel[k] = seen[strips[k]] = len(blob)
        blob += strips[k] + b"\xa5" * gap
    return rel, blob


def _ifd(e, at, tags, next_ifd, shuffle):
    """the IFD that stands at `at`: count, entries, the next IFD's offset, then the values that do not fit an entry"""
    ext_at = at + 2 + 12 * len(tags) + 4
    ext = b""
    ent = b""
    order = sorted(tags)
    if shuffle is not None:
        np.random.RandomState(shuffle).shuffle(order)
    for tag in order:
        typ, vals = tags[tag]
        if typ in (5, 10):  # RATIONAL: two LONGs a value
            data, count = struct.pack(e + "I" * len(vals), *vals), len(vals) // 2
        elif typ in (1, 2, 3, 4, 7):  # 2: ASCII, 7: UNDEFINED, a byte a value
            data, count = struct.pack(e + {1: "B", 2: "B", 3: "H", 4: "I", 7: "B"}[typ] * len(vals), *vals), len(vals)
        else:  # a type number no one knows: its value field is four bytes of something
            data, count = struct.pack(e + "I", vals[0]), 1
        if len(data) <= 4:
            field = data.ljust(4, b"\0")
        else:
            field = struct.pack(e + "I", ext_at + len(ext))
            ext += data + (b"\0" if len(data) & 1 else b"")
        ent += struct.pack(e + "HHI", tag, typ, count) + field
    return struct.pack(e + "H", len(tags)) + ent + struct.pack(e + "I", next_ifd) + ext


def _page(base, next_ifd, rows, cols, strips, compression, photometric=0, fill_order=1, rps=None, order="<", offsets_type=4,
          counts_type=4, extra=(), drop=(), ifd_first=False, odd=False, shuffle=None, reverse=False, gap=0, share=False, over=0):
    """one picture's strips and IFD as they stand from file offset `base` (even) on -> (the IFD's offset, the bytes)"""
    e = order
    strips = [bytes(s) for s in strips]
    if fill_order == 2:
        strips = [s.translate(_REV) for s in strips]
    rel, body = _layout(strips, reverse, gap, share, odd)
    body += bytes(over)

    def tags_for(data_at):
        tags = {256: (4, [cols]), 257: (4, [rows]), 258: (3, [1]), 259: (3, [compression]), 262: (3, [photometric]),
                266: (3, [fill_order]), 273: (offsets_type, [data_at + r for r in rel]), 277: (3, [1]),
                278: (4, [rps if rps is not None else rows]), 279: (counts_type, [len(s) + over for s in strips])}
        if compression == 4:
            tags[293] = (4, [0])
        for tag, typ, vals in extra:
            tags[tag] = (typ, list(vals))
        for tag in drop:
            tags.pop(tag, None)
        return tags

    start = base + (1 if odd else 0)
    if ifd_first:
        data_at = start + len(_ifd(e, start, tags_for(0), 0, shuffle))
        data_at += 1 if odd and not data_at & 1 else 0
        ifd = _ifd(e, start, tags_for(data_at), next_ifd, shuffle)
        return start, bytes(start - base) + ifd + bytes(data_at - start - len(ifd)) + body
    data = body + (b"\0" if (start + len(body)) & 1 != (1 if odd else 0) else b"")
    return start + len(data), bytes(start - base) + data + _ifd(e, start + len(data), tags_for(start), next_ifd, shuffle)


def assemble(rows, cols, strips, compression, big=False, chain=None, **kw):
    """Strips (bytes each) -> a TIFF stream.  Keywords: photometric, fill_order (2 stores the strips bit-reversed; they are
    given in FillOrder 1), rps, order, offsets_type, counts_type; extra: [(tag, type, [values])] added or replacing; drop:
    tags left out.  The forms a foreign writer may choose: ifd_first: the IFD in front of the strip data; odd: the IFD
    and every strip at an odd offset; shuffle (a seed): the entries in a shuffled order; reverse: the strips in reverse
    file order; gap: bytes between them; share: strips with equal bytes stored once; over: every byte count that much
    larger than its strip; chain: the arguments (a dict) of a second picture, whose IFD the first one's points to."""
    e = kw.get("order", "<")
    ifd_at, first = _page(8, 0, rows, cols, strips, compression, **kw)
    tail = b""
    if chain is not None:  # the first page's length does not depend on the pointer it holds
        first += bytes(len(first) & 1)
        ifd2, tail = _page(8 + len(first), 0, **dict(chain, order=e))
        ifd_at, first = _page(8, ifd2, rows, cols, strips, compression, **kw)
        first += bytes(len(first) & 1)
    head = (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", 43 if big else 42, ifd_at)
    return head + first + tail


def strips_of(stream):
    """the strips of a stream the parser accepts, as stored, given in FillOrder 1"""
    h = parse(stream)
    out = [bytes(stream[o:o + n]) for o, n in h["strips"]]
    return [s.translate(_REV) for s in out] if h["fill_order"] == 2 else out


def pillow_tiff(bits, compression="group4", rps=None):
    """bits: [rows, cols], nonzero = black -> the file Pillow (libtiff) writes: Photometric 0, FillOrder 1"""
    from PIL import Image
    img = Image.fromarray(np.where(np.asarray(bits) != 0, 0, 255).astype(np.uint8)).convert("1")
    bio = io.BytesIO()
    kw = {"tiffinfo": {278: int(rps)}} if rps else {}
    img.save(bio, format="TIFF", compression=compression, **kw)
    return bio.getvalue()


def pillow_read(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(stream))).convert("L"))


def rewrap(stream, **kw):
    """a stream Pillow wrote, with other tags, byte order, fill order or strip array types"""
    h = parse(stream)
    args = dict(photometric=h["photometric"], rps=h["rps"])
    args.update(kw)
    return assemble(h["rows"], h["cols"], strips_of(stream), h["compression"], **args)
