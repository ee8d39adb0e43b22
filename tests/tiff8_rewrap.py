"""8-bit gray and RGB TIFF as writers other than libtiff make it, plain Python and numpy: the same picture in the LZW code
streams a coder may choose, in strips that end in five ways, in PackBits cut into runs in four ways (t6_rewrap's writer over
rows of cols * spp bytes), and under every form of tiff_ref.assemble's IFD.  TIFF 6.0 LZW leaves the coder free in what
it matches (any entry of the table, not the longest), where it puts a Clear, and what stands behind the last code; a
decoder has to read all of it as the same picture.

lzw_recode's policies, each a list of codes for tiff8_ref.pack_codes:
  literal-N   literals alone and a Clear behind every N of them.  N <= 254: the literals have the indices 0 .. N - 1 and stay
              9 bits wide.  The Clear behind 254 literals has index 254 and is the one code of 10 bits (the early change).
  cap-L       the longest match, cut at L bytes
  short       at every step a random length between 1 and the longest match
  cadence-N   the longest match, and a Clear behind every N codes: N = 300, 800, 1800 put one width change in front of it
All of them also clear where libtiff does (3836 codes since the last Clear).  The coder follows the decoder's table rule:
the code with index i >= 1 adds entry 257 + i, the output of the code in front and its own first byte; of two entries
with equal bytes it names the first.

ENDINGS: "eoi" EOI behind the last code; "none" nothing; "junk" no EOI, random bits and bytes behind the last code;
"rows+" the strip codes more rows than the file gives it (noise); "overrun" the last code alone reaches past the strip's
last byte.  Where no entry of the table reaches past the end (a strip of literals), "overrun" cannot be written, and the
case is made and named "none".

Held to the picture they were made from and to the restatement alone, by name (NO_ARBITER): the files of several LZW or
PackBits strips without StripByteCounts, ifd-lzw2-rgb-no-counts*, ifd-lzw-gray-no-counts* and ifd-packbits-gray-no-counts*
(not the one-strip forms, and not the raw picture, whose counts libtiff estimates).  Pillow raises OSError("decoder error
-2") for them, behind libtiff's 'MissingRequired: TIFF directory is missing required "StripByteCounts" field'."""
import functools

import numpy as np

import t6_rewrap
import tiff8_ref as R
import tiff_ref
from tiff8_ref import CLEAR, EOI

LITERAL_N = (1, 2, 63, 64, 65, 127, 253, 254)
CAP_L = (2, 3, 8)
CADENCE_N = (300, 800, 1800)
POLICIES = tuple("literal-%d" % n for n in LITERAL_N) + tuple("cap-%d" % n for n in CAP_L) + ("short",) + \
    tuple("cadence-%d" % n for n in CADENCE_N)
ENDINGS = ("eoi", "none", "junk", "rows+", "overrun")
LIMIT = 3836  # libtiff's Clear: behind that many codes
PERIODS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127)
WIDE = (1023, 1024, 1025, 2048, 2049)
WIDTHS, ROWS = (1, 3, 64, 65, 257), (1, 7, 33)
KINDS = ("noise", "constant", "period2", "text", "gradient")
NO_ARBITER = set()


# ---- the coder ---------------------------------------------------------------------------------------------------------
def _recode(data, policy, seed=0):
    """-> (the codes from the leading Clear to the last data code, [(start, length)] of the data codes, the table behind the
    last code as {bytes: code})"""
    kind, _, arg = policy.partition("-")
    arg = int(arg) if arg else 0
    assert policy in POLICIES or (kind, arg) == ("cadence", 0), policy  # cadence-0: the plain greedy coder
    every = arg if kind in ("literal", "cadence") else 0
    rng = np.random.RandomState(seed)
    data = bytes(data)
    codes, spans, tab, i, prev, p, n = [CLEAR], [], {}, 0, b"", 0, len(data)
    while p < n:
        if i >= 1:
            tab.setdefault(prev + data[p:p + 1], 257 + i)
        m = 1
        if kind != "literal":
            while p + m < n and data[p:p + m + 1] in tab:
                m += 1
            if kind == "cap":
                m = min(m, arg)
            elif kind == "short":
                m = int(rng.randint(1, m + 1))
        cur = data[p:p + m]
        codes.append(cur[0] if m == 1 else tab[cur])
        spans.append((p, m))
        p, prev, i = p + m, cur, i + 1
        if p < n and (i == LIMIT or i == every):
            codes.append(CLEAR)
            tab, i, prev = {}, 0, b""
    return codes, spans, tab


def lzw_recode(raw, policy, seed=0, eoi=True):
    """bytes -> the codes of one strip under `policy`, with or without EOI"""
    return _recode(raw, policy, seed)[0] + ([EOI] if eoi else [])


def walk(codes):
    """A code list read as a decoder reads it -> [(place in the list, index since the last Clear, code, output position,
    length, how many codes earlier the entry it names was made or None for a literal)]; raises on a code no decoder takes"""
    out, lens, i, pos, prev = [], {}, 0, 0, 0
    assert codes[0] == CLEAR
    for k, c in enumerate(codes):
        if c == CLEAR:
            lens, i = {}, 0
            continue
        if c == EOI:
            break
        assert c <= 257 + i and c != 257 and (i == 0 or 257 + i < R.ENTRIES) and (i > 0 or c < 256), (k, c, i)
        ln = 1 if c < 256 else prev + 1 if c == 257 + i else lens[c]
        if i >= 1:
            lens[257 + i] = prev + 1
        out.append((k, i, c, pos, ln, None if c < 256 else i - (c - 257)))
        pos, prev, i = pos + ln, ln, i + 1
    return out


def read_codes(strip, total):
    """a strip's bytes -> its codes up to the one that fills `total` bytes, every code at the width of its index"""
    strip = bytes(strip)
    val = int.from_bytes(strip, "big")
    nbits = 8 * len(strip)
    codes, pos, i, got, lens, prev = [], 0, 0, 0, {}, 0
    while got < total or not codes:
        w = 9 if not codes else R.width(i)
        assert pos + w <= nbits, "the strip ends"
        c = (val >> (nbits - pos - w)) & ((1 << w) - 1)
        pos += w
        first = not codes
        codes.append(c)
        if first:
            assert c == CLEAR
        elif c == CLEAR:
            i, lens = 0, {}
        else:
            assert c != EOI
            ln = 1 if c < 256 else prev + 1 if c == 257 + i else lens[c]
            if i >= 1:
                lens[257 + i] = prev + 1
            got, prev, i = got + ln, ln, i + 1
    return codes


def straddler(codes, total):
    """the place of the code whose output begins in front of byte `total` and ends behind it, or None"""
    for k, _, _, pos, ln, _ in walk(codes):
        if pos < total < pos + ln:
            return k
    return None


def _noise(rng, n):
    return bytes(rng.randint(0, 256, n).astype(np.uint8))


def surplus(raw, policy, seed, n):
    """n bytes of noise to code behind a strip's rows.  Where the table holds an entry that begins with the last code's
    bytes and goes on, the noise begins with that entry's further bytes, so that a coder that takes the longest match
    writes one code across the rows' end."""
    rng = np.random.RandomState(seed + 7919)
    more = _noise(rng, n)
    _, spans, tab = _recode(raw, policy, seed)
    tail = bytes(raw)[spans[-1][0]:]
    longer = sorted(k for k in tab if len(k) > len(tail) and k.startswith(tail))
    if longer:
        ext = longer[int(rng.randint(0, len(longer)))][len(tail):]
        more = (ext + more)[:max(n, len(ext))]
    return more


def lzw_strip(raw, policy, ending, seed=0, more=None):
    """one strip's rows -> (its bytes, the ending it got).  more: the surplus bytes of "rows+" / "overrun" (default: a row's
    worth of surplus(), at least 8 bytes)"""
    assert ending in ENDINGS
    raw = bytes(raw)
    rng = np.random.RandomState(seed + 104729)
    if ending in ("rows+", "overrun"):
        if more is None:
            more = surplus(raw, policy, seed, 8)
        codes = _recode(raw + more, policy, seed)[0]
        if ending == "rows+":
            return R.pack_codes(codes + [EOI]), ending
        k = straddler(codes, len(raw))
        if k is not None:
            return R.pack_codes(codes[:k + 1]), ending
        ending = "none"
    codes = _recode(raw, policy, seed)[0]
    if ending == "eoi":
        return R.pack_codes(codes + [EOI]), ending
    out = bytearray(R.pack_codes(codes))
    if ending == "junk":
        pad = -sum_bits(codes) % 8
        out[-1] |= int(rng.randint(0, 1 << pad)) if pad else 0
        out += _noise(rng, int(rng.randint(1, 5)))
    return bytes(out), ending


def cuts_a_code(s):
    """whether in every strip of an LZW file the code that fills the rows goes on behind them"""
    h = R.parse(s)
    for k, (off, ln) in enumerate(h["strips"]):
        total = min(h["rps"], h["rows"] - k * h["rps"]) * h["cols"] * h["spp"]
        if straddler(read_codes(s[off:off + ln], total), total) is None:
            return False
    return True


def sum_bits(codes):
    """the bits of a code list, the first of them the leading Clear"""
    i, n = 0, 9
    for c in codes[1:]:
        n += R.width(i)
        i = 0 if c == CLEAR else i + 1
    return n


def write(img, policy, ending, rps=None, predictor=1, photometric=None, seed=0, more_rows=1, got=None, **kw):
    """a picture -> an LZW file with every strip coded by lzw_strip; "rows+" and "overrun" strips code more_rows rows of
    surplus.  got (a list): receives the ending every strip got"""
    rb = R.raw_rows(img, photometric)[0].shape[1]

    def strip(k):
        def make(raw):
            more = surplus(raw, policy, seed + k, more_rows * rb) if ending in ("rows+", "overrun") else None
            data, e = lzw_strip(raw, policy, ending, seed + k, more)
            if got is not None:
                got.append(e)
            return data
        return make
    nstrips = -(-np.asarray(img).shape[0] // (rps or np.asarray(img).shape[0]))
    return R.write(img, 5, rps, predictor, photometric, strip_codes={k: strip(k) for k in range(nstrips)}, **kw)


# ---- contents ----------------------------------------------------------------------------------------------------------
def period_content(p, rows, cols, spp=1, seed=0):
    """p different pixels, repeated along the raster"""
    rng = np.random.RandomState(seed)
    if spp == 1:
        unit = rng.permutation(256)[:p].astype(np.uint8)
        return np.resize(unit, rows * cols).reshape(rows, cols)
    unit = rng.permutation(1 << 24)[:p]
    px = np.stack([unit & 255, unit >> 8 & 255, unit >> 16], axis=1).astype(np.uint8)
    return np.resize(px, (rows * cols, 3)).reshape(rows, cols, 3)


def constant_codes(value, total, limit=LIMIT, exact=True):
    """`total` bytes of one value as the longest-match coder writes them, in closed form: behind a Clear the literal, then
    258, 259, ... -- every code the entry it is about to add, one byte longer than the code in front -- and a Clear behind
    `limit` codes.  exact: the last code is the entry that ends on byte `total`; else it is the next in the row and reaches
    past it.  -> (codes with EOI, the longest output of a code)"""
    codes, left, longest = [CLEAR], total, 0
    while left > 0:
        for i in range(limit):
            ln = i + 1
            if ln >= left and exact:
                ln = left
            codes.append(value if ln == 1 else 256 + ln)
            longest = max(longest, ln)
            left -= ln
            if left <= 0:
                break
        if left > 0:
            codes.append(CLEAR)
    return codes + [EOI], longest


# ---- the streams: (name, stream, the picture) ----------------------------------------------------------------------------
def _variant(k):
    """the gray Photometric, the byte order and the Predictor from the bits of a counter"""
    return k & 1, "<>"[k >> 1 & 1], 1 + (k >> 2 & 1)


@functools.lru_cache(maxsize=None)
def policy_dialects(spp):
    """every small shape x RowsPerStrip, every policy, the endings and the contents in turn"""
    out, k = [], 0
    for cols in WIDTHS:
        for rows in ROWS:
            for rps in sorted({1, min(7, rows), rows}):
                for pi, policy in enumerate(POLICIES):
                    kind = KINDS[(k // 75 + k // 15 + pi) % 5]  # k // 15: the shape; the endings go by shape + policy
                    a = R.content(kind, rows, cols, spp, seed=rows * 1000 + cols)
                    photo, order, pred = _variant(k)
                    got, asked = [], ENDINGS[(k + k // len(POLICIES)) % 5]
                    s = write(a, policy, asked, rps, pred, photo if spp == 1 else None, seed=3 * k, got=got, order=order)
                    ending = asked if asked != "overrun" or "overrun" in got else "none"
                    out.append(("lzw-%s-%s-%s-%dx%dx%d-rps%d-pred%d-p%d-%s" % (policy, ending, kind, rows, cols, spp, rps, pred, photo, order), s, a))
                    k += 1
    return out


@functools.lru_cache(maxsize=None)
def period_dialects():
    """the period contents under the longest-match coder: gray, and RGB with the period in pixels"""
    out = []
    for p in PERIODS:
        for spp in (1, 3):
            a = period_content(p, 7, 257, spp, seed=p)
            s = R.write(a, 5, 4, policy=("libtiff", "no_eoi")[p & 1], order="<>"[p >> 1 & 1])
            out.append(("period-%d-spp%d" % (p, spp), s, a))
    return out


@functools.lru_cache(maxsize=None)
def cut_dialects():
    """the "rows+" and "overrun" files of the three compressions.  LZW: every strip codes surplus rows, so that a good
    strip stands behind every cut one but the last.  PackBits and raw: the last strip (or the only one, with RowsPerStrip
    above ImageLength) carries all RowsPerStrip rows."""
    out = []
    for spp in (1, 3):
        for kind in ("text", "constant", "period2", "gradient"):
            a = R.content(kind, 23, 65, spp, seed=11)
            for policy in ("cadence-300", "cap-8", "short", "cadence-1800"):
                for ending in ("rows+", "overrun"):
                    for rps, rows_tag in ((5, None), (23, 30)):
                        kw = dict(extra=[(278, 4, [rows_tag])]) if rows_tag else {}
                        got = []
                        s = write(a, policy, ending, rps, 1 + (policy == "cap-8"), seed=len(out), more_rows=2, got=got, **kw)
                        if set(got) == {ending} and cuts_a_code(s):
                            out.append(("cut-lzw-%s-%s-%s-spp%d-rps%s" % (policy, ending, kind, spp, rows_tag or rps), s, a))
    rng = np.random.RandomState(5)
    for spp in (1, 3):
        a = R.content("text", 23, 53, spp, seed=12)
        rows, spp, photo = R.raw_rows(a)
        rb = rows.shape[1]
        for comp in (32773, 1):
            for rps, rows_tag in ((5, 5), (8, 8), (23, 30)):
                strips = []
                for r0 in range(0, 23, rps):
                    part = rows[r0:r0 + rps].tobytes()
                    if r0 + rps >= 23:  # the last strip: all of RowsPerStrip's rows
                        part += _noise(rng, (r0 + rows_tag - 23) * rb)
                    strips.append(part if comp == 1 else t6_rewrap.packbits_encode(part, "max", 0, rb))
                s = tiff_ref.assemble(23, 53, strips, comp, photometric=photo, rps=rows_tag, extra=[(258, 3, [8] * spp), (277, 3, [spp])])
                out.append(("cut-%d-rows+-spp%d-rps%d" % (comp, spp, rows_tag), s, a))
    return out


@functools.lru_cache(maxsize=None)
def wide_dialects():
    """three rows of noise around the finishing kernel's turn of 1024 pixels, LZW with Predictor 2"""
    out = []
    for k, cols in enumerate(WIDE):
        for spp in (1, 3):
            a = R.content("noise", 3, cols, spp, seed=cols)
            photo = 0 if (spp == 1 and cols == 1025) else None
            out.append(("wide-%d-spp%d" % (cols, spp), R.write(a, 5, 2, 2, photometric=photo, order="<>"[k & 1]), a))
    return out


@functools.lru_cache(maxsize=None)
def packbits_dialects():
    out, k = [], 0
    for spp in (1, 3):
        for cols in (77, 53):
            for rps in (1, 8, 19):
                for policy in t6_rewrap.PACKBITS:
                    kind = KINDS[k % 5]
                    a = R.content(kind, 19, cols, spp, seed=cols + k)
                    rows, _, photo = R.raw_rows(a, (k >> 1 & 1) if spp == 1 else None)
                    strips = [t6_rewrap.packbits_encode(rows[r:r + rps].tobytes(), policy, 13 * k + r, cols * spp) for r in range(0, 19, rps)]
                    s = tiff_ref.assemble(19, cols, strips, 32773, photometric=photo, rps=rps, order="<>"[k & 1],
                                          extra=[(258, 3, [8] * spp), (277, 3, [spp])])
                    out.append(("packbits8-%s-%s-19x%dx%d-rps%d-p%d" % (policy, kind, cols, spp, rps, photo), s, a))
                    k += 1
    return out


def ifd_picture(spp):
    """37 x 67: eight rows again and again, so that the strips of RowsPerStrip 8 hold equal bytes but the last"""
    return np.tile(R.content("text", 8, 67, spp, seed=77), (5, 1) if spp == 1 else (5, 1, 1))[:37]


@functools.lru_cache(maxsize=None)
def ifd_dialects():
    """the forms of the assembler over an LZW + Predictor 2 RGB, an LZW gray, a PackBits gray and a raw RGB picture"""
    other = dict(rows=5, cols=40, strips=[t6_rewrap.pack_rows(np.eye(5, 40))], compression=1, photometric=1)
    many = [
        ("ifd-first", dict(ifd_first=True)), ("odd", dict(odd=True)), ("odd-ifd-first", dict(odd=True, ifd_first=True)),
        ("shuffled", dict(shuffle=5)), ("reverse-gaps", dict(reverse=True, gap=3)), ("gaps", dict(gap=5)), ("shared", dict(share=True)),
        ("shared-reverse-odd", dict(share=True, reverse=True, odd=True)), ("counts-over", dict(over=9)), ("big-endian", dict(order=">")),
        ("big-endian-odd-shuffled", dict(order=">", odd=True, shuffle=3)), ("short-arrays", dict(offsets_type=3, counts_type=3)),
        ("short-arrays-big-endian-ifd-first", dict(offsets_type=3, counts_type=3, order=">", ifd_first=True)),
        ("bits-long", dict(bits_long=True)), ("bits-long-big-endian-odd", dict(bits_long=True, order=">", odd=True)),
        ("no-277", dict(drop=(277,))), ("chained", dict(chain=other)), ("chained-ifd-first-odd", dict(chain=other, ifd_first=True, odd=True)),
        ("no-counts", dict(drop=(279,))), ("no-counts-reverse-gaps", dict(drop=(279,), reverse=True, gap=3)),
        ("no-counts-ifd-first-big-endian", dict(drop=(279,), ifd_first=True, order=">")),
    ]
    one = [("no-278", dict(drop=(278,))), ("no-278-no-279", dict(drop=(278, 279))), ("one-strip-no-counts-ifd-first-odd", dict(drop=(279,), ifd_first=True, odd=True)),
           ("no-277-278-279-shuffled", dict(drop=(277, 278, 279), shuffle=1))]
    out = []
    for pname, spp, comp, pred in (("lzw2-rgb", 3, 5, 2), ("lzw-gray", 1, 5, 1), ("packbits-gray", 1, 32773, 1), ("raw-rgb", 3, 1, 1)):
        a = ifd_picture(spp)
        for rps, forms in ((8, many), (37, one)):
            for name, kw in forms:
                kw = dict(kw)
                if 277 in kw.get("drop", ()) and spp == 3:
                    continue  # SamplesPerPixel defaults to 1
                extra = [(258, 4, [8] * spp)] if kw.pop("bits_long", False) else []
                s = R.write(a, comp, rps, pred, policy="no_eoi" if "over" in kw else "libtiff", extra=extra, **kw)
                if name == "shared":
                    assert len({bytes(s[o:o + n]) for o, n in R.parse(s)["strips"][:4]}) == 1 and len({o for o, _ in R.parse(s)["strips"]}) == 2
                out.append(("ifd-%s-%s" % (pname, name), s, a))
                if 279 in kw.get("drop", ()) and rps == 8 and comp != 1:
                    NO_ARBITER.add(out[-1][0])
    return out


LONG_COLS, LONG_ROWS, LONG_CUT = 2800, 2700, 1650


@functools.lru_cache(maxsize=None)
def long_constant():
    """-> [(name, stream, picture, the longest output of a code)]: a constant gray page of 7.56 MB in one strip, under
    libtiff's Clear and under "late" (entry 4095 made and used); and 4350 rows of the same in strips of 2700, the second
    of them coding all 2700 rows, so that its 1650 rows end inside the output of a code of some 3000 bytes"""
    out = []
    a = np.full((LONG_ROWS, LONG_COLS), 200, np.uint8)
    for name, limit in (("libtiff", LIMIT), ("late", 3839)):
        codes, longest = constant_codes(200, a.size, limit)
        s = tiff_ref.assemble(LONG_ROWS, LONG_COLS, [R.pack_codes(codes)], 5, photometric=1, extra=[(258, 3, [8])])
        out.append(("long-constant-" + name, s, a, longest))
    b = np.full((LONG_ROWS + LONG_CUT, LONG_COLS), 200, np.uint8)
    strip = R.pack_codes(codes)
    s = tiff_ref.assemble(LONG_ROWS + LONG_CUT, LONG_COLS, [strip, strip], 5, photometric=1, rps=LONG_ROWS, extra=[(258, 3, [8])])
    out.append(("long-constant-rows+", s, b, longest))
    return out


def _lzw_file(rows, cols, strips, **kw):
    return tiff_ref.assemble(rows, cols, strips, 5, photometric=1, extra=[(258, 3, [8])] + kw.pop("extra", []), **kw)


def pack_nine(codes):
    """every code at 9 bits, whatever its index"""
    bits = "".join("{:09b}".format(c) for c in codes)
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def pins():
    """[(name, stream, code)]: the streams the device refuses, each with the code of tdec_parse / tiff8_ref.parse, or -215
    where the strip itself is damaged"""
    g = R.content("text", 6, 40, 1, seed=4)
    c = R.content("gradient", 6, 40, 3, seed=4)
    old = b"\x00\x01" + R.lzw_encode(g.tobytes())
    hi = np.random.RandomState(3).randint(128, 256, (3, 200)).astype(np.uint8)
    nine = [CLEAR]
    for k, b in enumerate(hi.tobytes()):  # a Clear behind every 255 literals: the literal with index 254 is read at 10 bits
        nine += [b] + ([CLEAR] if k % 255 == 254 else [])
    raw = g.tobytes()
    full = _recode(raw + surplus(raw, "cadence-300", 0, 40), "cadence-300", 0)[0]
    k = [w for w in walk(full) if w[3] + w[4] >= len(raw)][0][0]  # the code that fills the rows
    return [
        ("no PhotometricInterpretation at 8 bits", R.write(g, 5, drop=(262,)), -213),
        ("ExtraSamples with three samples", R.write(c, 5, extra=[(338, 3, [2])]), -213),
        ("PlanarConfiguration 2 with three samples", R.write(c, 1, extra=[(284, 3, [2])]), -213),
        ("old-style LZW", _lzw_file(6, 40, [old]), -213),
        ("FillOrder 2 at 8 bits", R.write(g, 1, extra=[(266, 3, [2])]), -213),
        ("BitsPerSample 8,8,4", R.write(c, 5, extra=[(258, 3, [8, 8, 4])]), -213),
        ("literals at 9 bits past index 253", _lzw_file(3, 200, [pack_nine(nine + [EOI])]), -215),
        ("rows+ cut one code short of its rows", _lzw_file(6, 40, [R.pack_codes(full[:k])], rps=9), -215),
    ]
