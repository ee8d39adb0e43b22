"""A plain Python / numpy restatement of the 8-bit gray and RGB TIFF decoder (csrc/oics_tiff_dec.cpp, csrc/tiff_lzw.hpp,
csrc/tiff_dec8.hip): the first IFD's walk with the tags the 8-bit files add, TIFF 6.0 LZW read a code at a time, an LZW
writer with policies (where it puts its Clear codes, whether it ends with EOI, bytes behind it), Predictor 2, PackBits and
raw strips, and an assembler for either byte order and any RowsPerStrip (tiff_ref.assemble with the 8-bit tags).  The
bilevel restatement, tiff_ref.py, stays what it is; its Refused / Damaged and its assembler are used here."""
import io
import struct

import numpy as np

import tiff_ref
from tiff_ref import ASSERT, BADARG, NOTIMPL, Damaged, Refused

CLEAR, EOI, FIRST, ENTRIES = 256, 257, 258, 4096
POLICIES = ("libtiff", "late", "random", "no_eoi", "trailing")


def width(i):
    """of the code with index i since the last Clear: the early change"""
    return 9 + (i >= 254) + (i >= 766) + (i >= 1790)


# ---- the parser ------------------------------------------------------------------------------------------------------
def parse(s):
    """-> tiff_ref.parse's dict and bps, spp, predictor; raises Refused.  The rules of tdec_parse, in its order."""
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
    known = (256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 293, 317)
    v = {259: 1, 262: -1, 266: 1, 274: 1, 278: 0xffffffff, 284: 1, 293: 0, 317: 1}
    bps, bps_count, spp, tiles, extra, arr = 1, 1, 1, False, False, {}
    for k in range(cnt):
        at0 = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack(e + "HHI", s[at0:at0 + 8])
        if 322 <= tag <= 325:
            tiles = True
            continue
        if tag == 338:
            extra = True
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
        fmt = e + {1: "B", 2: "H", 4: "I"}[size]
        val = struct.unpack(fmt, s[at:at + size])[0]
        if tag in (273, 279):
            arr[tag] = (at, count, size)
        elif tag == 258:
            bps, bps_count = val, count
            if count == 3:
                if any(struct.unpack(fmt, s[at + size * j:at + size * (j + 1)])[0] != val for j in (1, 2)):
                    bps = -1
            elif count != 1:
                bps = -1
        elif tag == 277:
            spp = val
        else:
            if count != 1:
                raise Refused(BADARG, "tag with several values")
            v[tag] = val
    comp = v[259]
    if tiles:
        raise Refused(NOTIMPL, "tiles")
    if extra:
        raise Refused(NOTIMPL, "ExtraSamples")
    if bps not in (1, 8):
        raise Refused(NOTIMPL, "depth")
    if v[284] != 1 and spp > 1:
        raise Refused(NOTIMPL, "planar")
    if spp not in (1, 3):
        raise Refused(NOTIMPL, "samples")
    if spp == 3 and (bps != 8 or bps_count != 3):
        raise Refused(NOTIMPL, "three samples below 8,8,8")
    if spp == 1 and bps_count != 1:
        raise Refused(NOTIMPL, "depth values")
    if comp not in (1, 4, 5, 32773):
        raise Refused(NOTIMPL, "compression")
    if comp == 4 and bps != 1:
        raise Refused(NOTIMPL, "T.6 above 1 bit")
    if comp == 5 and bps != 8:
        raise Refused(NOTIMPL, "LZW at 1 bit")
    if (v[262] != 2) if spp == 3 else (v[262] not in (0, 1)):
        raise Refused(NOTIMPL, "photometric")
    if v[266] not in (1, 2):
        raise Refused(BADARG, "fill order")
    if v[266] == 2 and bps == 8:
        raise Refused(NOTIMPL, "fill order 2 at 8 bits")
    if comp == 5 and v[317] not in (1, 2):
        raise Refused(NOTIMPL, "predictor")
    if comp == 4 and v[293] & 2:
        raise Refused(NOTIMPL, "uncompressed mode")
    if comp == 4 and v[293]:
        raise Refused(BADARG, "T6Options")
    if v[274] != 1:
        raise Refused(NOTIMPL, "orientation")
    rows, cols = v.get(257, 0), v.get(256, 0)
    if rows < 1 or cols < 1:
        raise Refused(BADARG, "size")
    if rows > 1 << 20 or cols > 1 << 20 or rows * cols > 1 << 30:
        raise Refused(ASSERT, "size limits")
    if comp == 4 and cols > tiff_ref.T6_MAX_COLS:
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
    rb = cols * spp if bps == 8 else (cols + 7) // 8
    for k in range(ns):
        off = offs[k]
        ln = value(279, k) if 279 in arr else min([o for o in offs if o > off] or [n]) - off
        if ln < 1 or off < 8 or off > n or ln > n - off:
            raise Refused(BADARG, "strip outside")
        if ln >= 1 << 28:
            raise Refused(ASSERT, "strip length")
        nr = min(rps, rows - k * rps)
        if comp == 5:
            if ln >= 2 and s[off] == 0 and s[off + 1] & 1:
                raise Refused(NOTIMPL, "old-style LZW")
            if nr * rb >= 1 << 31:
                raise Refused(ASSERT, "LZW strip rows")
        if comp == 1 and ln < nr * rb:
            raise Refused(BADARG, "short strip")
        strips.append((off, ln))
    return dict(rows=rows, cols=cols, compression=comp, photometric=v[262], fill_order=v[266], rps=rps, strips=strips, bps=bps,
                spp=spp, predictor=v[317] if comp == 5 else 1)


# ---- LZW -------------------------------------------------------------------------------------------------------------
def lzw_decode(data, total):
    """one strip -> `total` bytes; raises Damaged.  A code at a time, the table as byte strings."""
    data = bytes(data)
    nbits = 8 * len(data)

    def code(pos, w):
        if pos + w > nbits:
            return None
        k = pos >> 3
        x = int.from_bytes(data[k:k + 3].ljust(3, b"\0"), "big")
        return (x >> (24 - (pos & 7) - w)) & ((1 << w) - 1)
    c = code(0, 9)
    if c != CLEAR:
        raise Damaged("no leading Clear" if c is not None else "input ends")
    pos, i, out, tab, prev = 9, 0, bytearray(), {}, b""
    while len(out) < total:
        w = width(i)
        c = code(pos, w)
        if c is None or c == EOI:
            raise Damaged("input ends")
        pos += w
        if c == CLEAR:
            i, tab = 0, {}
            continue
        if c > 257 + i:
            raise Damaged("a code above the next free entry")
        if i >= 1 and 257 + i >= ENTRIES:
            raise Damaged("the table is full")
        if c < 256:
            cur = bytes([c])
        elif c == 257 + i:
            cur = prev + prev[:1]
        else:
            cur = tab[c]
        if i >= 1:
            tab[257 + i] = prev + cur[:1]
        out += cur
        prev = cur
        i += 1
    return bytes(out[:total])


def pack_codes(codes):
    """codes (Clear and EOI among them) -> bytes, every code at the width of its index since the last Clear"""
    acc, nb, i, out = 0, 0, 0, bytearray()
    first = True
    for c in codes:
        w = 9 if first else width(i)
        acc, nb = (acc << w) | c, nb + w
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 0xff)
            nb -= 8
        acc &= (1 << nb) - 1
        if first:
            first = False  # the leading Clear
            if c != CLEAR:
                i = 1
        elif c == CLEAR:
            i = 0
        else:
            i += 1
    if nb:
        out.append((acc << (8 - nb)) & 0xff)
    return bytes(out)


def lzw_codes(data, policy="libtiff", seed=0):
    """bytes -> the writer's codes.  libtiff: Clear when entry 4093 is made; late: when entry 4095 is, the last index that
    a decoder takes; random: also at random places (two in a row among them); no_eoi / trailing: libtiff's Clears."""
    assert policy in POLICIES
    rng = np.random.RandomState(seed)
    limit = 3839 if policy == "late" else 3836
    codes, tab, i, w = [CLEAR], {}, 0, b""
    data = bytes(data)

    def emit(c):
        nonlocal i, tab
        codes.append(c)
        i += 1
        if i == limit or (policy == "random" and rng.randint(0, 40) == 0):
            codes.append(CLEAR)
            if policy == "random" and rng.randint(0, 4) == 0:
                codes.append(CLEAR)
            i, tab = 0, {}
            return True
        return False
    for b in data:
        wb = w + bytes([b])
        if len(wb) == 1 or wb in tab:
            w = wb
            continue
        c = w[0] if len(w) == 1 else tab[w]
        nxt = 258 + i  # the entry this emission makes
        if not emit(c):
            tab[wb] = nxt
        w = bytes([b])
    if w:
        codes.append(w[0] if len(w) == 1 else tab[w])
    if policy != "no_eoi":
        codes.append(EOI)
    return codes


def lzw_encode(data, policy="libtiff", seed=0):
    out = pack_codes(lzw_codes(data, policy, seed))
    return out + b"\x5a\xa5\xff\x00\x01" if policy == "trailing" else out


# ---- Predictor 2, PackBits ---------------------------------------------------------------------------------------------
def difference(rows, spp):
    """[nr, cols * spp] uint8 -> the same with every sample replaced by its difference to the pixel on the left"""
    a = np.asarray(rows, np.uint8).copy()
    a[:, spp:] = a[:, spp:] - a[:, :-spp]
    return a


def accumulate(rows, spp):
    a = np.asarray(rows, np.uint8).reshape(rows.shape[0], -1, spp)
    return np.cumsum(a, axis=1, dtype=np.uint64).astype(np.uint8).reshape(rows.shape)


def packbits_encode(row):
    """one row -> PackBits, runs of three or more as replicate runs"""
    row = bytes(row)
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j < n and row[j] == row[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            out += bytes([257 - (j - i), row[i]])
            i = j
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and row[j] == row[j + 1] == row[j + 2]):
            j += 1
        out += bytes([j - i - 1]) + row[i:j]
        i = j
    return bytes(out)


# ---- files -----------------------------------------------------------------------------------------------------------
def raw_rows(img, photometric=None):
    """[rows, cols] gray or [rows, cols, 3] RGB -> ([rows, cols * spp] as the file stores them, spp, photometric)"""
    a = np.asarray(img, np.uint8)
    spp = 1 if a.ndim == 2 else 3
    if photometric is None:
        photometric = 1 if spp == 1 else 2
    rows = a.reshape(a.shape[0], -1)
    return (255 - rows if photometric == 0 else rows), spp, photometric


def write(img, compression=5, rps=None, predictor=1, photometric=None, policy="libtiff", seed=0, order="<", strip_codes=None, **kw):
    """An image -> a TIFF stream of this module's making.  strip_codes: {strip index: a function(raw bytes) -> the strip's
    bytes} for hand-made strips."""
    rows, spp, photometric = raw_rows(img, photometric)
    nr, rb = rows.shape
    rps = rps or nr
    strips = []
    for k, r0 in enumerate(range(0, nr, rps)):
        part = rows[r0:r0 + rps]
        if predictor == 2 and compression == 5:
            part = difference(part, spp)
        raw = part.tobytes()
        if strip_codes and k in strip_codes:
            strips.append(strip_codes[k](raw))
        elif compression == 5:
            strips.append(lzw_encode(raw, policy, seed + k))
        elif compression == 32773:
            strips.append(b"".join(packbits_encode(r) for r in part))
        else:
            strips.append(raw)
    extra = [(258, 3, [8] * spp), (277, 3, [spp])] + ([(317, 3, [predictor])] if predictor != 1 else []) + list(kw.pop("extra", []))
    return tiff_ref.assemble(nr, rb // spp, strips, compression, photometric=photometric, rps=rps, order=order, extra=extra, **kw)


def decode(stream):
    """-> uint8 [rows, cols] (gray) or [rows, cols, 3] (RGB), what libtiff gives; raises Refused or Damaged"""
    h = parse(stream)
    assert h["bps"] == 8
    rows, cols, rps, spp = h["rows"], h["cols"], h["rps"], h["spp"]
    rb = cols * spp
    out = np.zeros((rows, rb), np.uint8)
    for k, (off, ln) in enumerate(h["strips"]):
        r0 = k * rps
        nr = min(rps, rows - r0)
        data = bytes(stream[off:off + ln])
        if h["compression"] == 5:
            raw = lzw_decode(data, nr * rb)
        elif h["compression"] == 32773:
            raw = tiff_ref.packbits_decode(data, nr * rb)
        else:
            raw = data[:nr * rb]
        part = np.frombuffer(raw, np.uint8).reshape(nr, rb)
        out[r0:r0 + nr] = accumulate(part, spp) if h["predictor"] == 2 else part
    if h["photometric"] == 0:
        out = 255 - out
    return out if spp == 1 else out.reshape(rows, cols, 3)


def pillow_tiff(img, compression="tiff_lzw", rps=None, predictor=1):
    """the file Pillow (libtiff) writes for a gray or RGB array"""
    from PIL import Image
    bio = io.BytesIO()
    info = {}
    if rps:
        info[278] = int(rps)
    if predictor != 1:
        info[317] = int(predictor)
    Image.fromarray(np.asarray(img, np.uint8)).save(bio, format="TIFF", compression=compression, **({"tiffinfo": info} if info else {}))
    return bio.getvalue()


def pillow_read(stream):
    """-> gray [rows, cols] or RGB [rows, cols, 3]; raises whatever Pillow raises for a damaged file"""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(stream)))
    im.load()
    assert im.mode in ("L", "RGB"), im.mode
    return np.asarray(im)


def as_output(img, channels):
    """what the library returns for libtiff's picture: gray, B = G = R, or BGR"""
    a = np.asarray(img)
    if a.ndim == 3:
        assert channels == 3
        return np.ascontiguousarray(a[..., ::-1])
    return a if channels == 1 else np.repeat(a[..., None], 3, axis=2)


# ---- contents --------------------------------------------------------------------------------------------------------
def content(kind, rows, cols, spp=1, seed=0):
    rng = np.random.RandomState(seed)
    shape = (rows, cols) if spp == 1 else (rows, cols, 3)
    if kind == "noise":
        a = rng.randint(0, 256, shape)
    elif kind == "constant":
        a = np.full(shape, 200)
    elif kind == "period2":
        a = np.zeros(shape, np.int64)
        a.reshape(-1)[1::2] = 255
    elif kind == "text":  # a light page with noise of a few levels and dark strokes
        a = 240 + rng.randint(0, 4, shape)
        for _ in range(max(1, rows * cols // 40)):
            y, x = rng.randint(0, rows), rng.randint(0, cols)
            a[y:y + 1, x:x + rng.randint(1, 6)] = rng.randint(0, 40)
    elif kind == "gradient":
        a = (np.arange(cols)[None, :] * 3 + np.arange(rows)[:, None] * 5)
        a = a if spp == 1 else np.stack([a, a * 2 + 7, 255 - a], axis=2)
    else:
        raise ValueError(kind)
    return (a % 256).astype(np.uint8)
