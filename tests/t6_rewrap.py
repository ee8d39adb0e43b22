"""A T.6 (CCITT Group 4) encoder with policies and a PackBits writer, plain Python and numpy: the same picture in the code
streams a writer other than libtiff may choose.  T.6 leaves the coder free in three ways -- which of the legal modes codes
a step, how a run of 64 or more is cut into make-up codes, and what stands behind the last row -- and PackBits in how the
bytes are cut into runs.  A decoder has to read all of them as the same picture.

The code tables come from tiff_ref.tables(), the library's own dump, turned round to {run: (code, bits)}.

t6_encode's policy "libtiff" with runs "fewest" and ending "eofb" is the procedure of T.6 itself and equals libtiff's
encoder byte for byte (test_t6_rewrap.py); the others differ from it in the one named respect."""
import bisect
import functools

import numpy as np

import tiff_cases
import tiff_ref

POLICIES = ("libtiff", "h-only", "random")
RUNS = ("fewest", "split")
ENDINGS = ("eofb", "none", "cut", "junk", "rows+")
PACKBITS = ("literal1", "max", "crossing", "noop")

_VCODE = {0: "1", 1: "011", -1: "010", 2: "000011", -2: "000010", 3: "0000011", -3: "0000010"}
_PASS, _HORIZ, _EOFB = "0001", "001", "000000000001" * 2

_BY_RUN = None


def by_run():
    """[white, black]: {run: the code as a string of bits}"""
    global _BY_RUN
    if _BY_RUN is None:
        _BY_RUN = [{r: "{:0{}b}".format(c, b) for (c, b), r in t.items()} for t in tiff_ref.tables()]
    return _BY_RUN


def changes(row):
    """the positions where a row changes colour, the first from white: strictly increasing, below len(row)"""
    row = np.asarray(row, np.uint8)
    prev = np.concatenate(([0], row[:-1]))
    return [int(p) for p in np.nonzero(row != prev)[0]]


def _compose(rng, m, kmin):
    """m units of 64 as at least kmin make-up codes (as far as m allows) of at most 40 units, in a random order"""
    while True:
        k = min(m, max(kmin, -(-m // 40)) + int(rng.randint(0, 3)))
        cuts = sorted(rng.choice(np.arange(1, m), k - 1, replace=False).tolist()) if k > 1 else []
        parts = np.diff([0] + cuts + [m]).tolist()
        if max(parts) <= 40:
            return parts


def run_codes(n, colour, runs="fewest", rng=None, stats=None):
    """one run as make-up codes and a terminating code -> a string of bits.  stats (a dict) counts what "split" wrote:
    "three": runs with three or more make-up codes, "mixed": runs above 2560 with an extended and an ordinary one"""
    tab = by_run()[colour]
    if runs == "fewest" or n < 64:
        out = ""
        while n >= 2624:
            out += tab[2560]
            n -= 2560
        if n >= 64:
            out += tab[n & ~63]
        return out + tab[n & 63]
    m = n >> 6
    if m > 40:  # one extended code (1792 .. 2560), the rest with an ordinary one (64 .. 1728) among them
        while True:
            x = int(rng.randint(28, 41))
            parts = [x] + _compose(rng, m - x, min(2, m - x))
            if min(parts) <= 27:
                break
        parts = [parts[i] for i in rng.permutation(len(parts))]
    else:
        parts = _compose(rng, m, min(3, m))
    if stats is not None:
        stats["three"] = stats.get("three", 0) + (len(parts) >= 3)
        stats["mixed"] = stats.get("mixed", 0) + (n > 2560 and max(parts) >= 28 and min(parts) <= 27)
    assert 64 * sum(parts) + (n & 63) == n and (n < 192 or len(parts) >= 3)
    return "".join(tab[64 * p] for p in parts) + tab[n & 63]


def _row(cur, ref, cols, policy, runs, rng, stats):
    """one row's codes; cur and ref: the change positions of the row and of the one above"""
    out = []
    a0, colour = -1, 0
    while a0 < cols:
        j = bisect.bisect_right(cur, a0)
        a1 = cur[j] if j < len(cur) else cols
        a2 = cur[j + 1] if j + 1 < len(cur) else cols
        i = bisect.bisect_right(ref, a0)  # b1: right of a0 and a change to the other colour than a0's
        i += (i & 1) != colour
        b1 = ref[i] if i < len(ref) else cols
        b2 = ref[i + 1] if i + 1 < len(ref) else cols
        legal = ["H"]
        if b2 < a1:
            legal.append("P")
        if abs(a1 - b1) <= 3:
            legal.append("V")
        if policy == "libtiff":
            mode = "P" if "P" in legal else "V" if "V" in legal else "H"
        elif policy == "h-only":
            mode = "H"
        else:
            mode = legal[int(rng.randint(0, len(legal)))]
        if mode == "P":
            out.append(_PASS)
            a0 = b2
        elif mode == "V":
            out.append(_VCODE[a1 - b1])
            a0, colour = a1, colour ^ 1
        else:  # a0a1 in the current colour (from 0 at a row's start, a run of 0 where it begins black), a1a2 in the other
            out.append(_HORIZ + run_codes(a1 - max(a0, 0), colour, runs, rng, stats) + run_codes(a2 - a1, colour ^ 1, runs, rng, stats))
            a0 = a2
    return "".join(out)


def t6_encode(bits, policy="libtiff", runs="fewest", ending="eofb", seed=0, stats=None):
    """bits [rows, cols] (1 = black) -> one strip in FillOrder 1"""
    assert policy in POLICIES and runs in RUNS and ending in ENDINGS
    bits = np.asarray(bits, np.uint8)
    rows, cols = bits.shape
    rng = np.random.RandomState(seed)
    if ending == "rows+":  # one more coded row than the strip's rows
        bits = np.concatenate([bits, (rng.rand(1, cols) < 0.5).astype(np.uint8) & bits[-1:] | bits[:1]])
    out, ref = [], []
    for r in range(bits.shape[0]):
        cur = changes(bits[r])
        out.append(_row(cur, ref, cols, policy, runs, rng, stats))
        ref = cur
    s = "".join(out)
    if ending in ("eofb", "junk"):
        s += _EOFB
    s += "0" * (-len(s) % 8)
    data = bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))
    if ending == "cut":
        data = data.rstrip(b"\0") or b"\0"
    if ending == "junk":
        data += bytes(rng.randint(0, 256, int(rng.randint(1, 4))).astype(np.uint8))
    return data


def _greedy(raw):
    """the runs of a piece as a max-length coder takes them: replicate runs of 2 .. 128, literals of 1 .. 128"""
    out, p, n = [], 0, len(raw)
    while p < n:
        r = 1
        while p + r < n and r < 128 and raw[p + r] == raw[p]:
            r += 1
        if r >= 2:
            out.append(bytes([257 - r, raw[p]]))
            p += r
            continue
        q = p + 1
        while q < n and q - p < 128 and not (q + 1 < n and raw[q] == raw[q + 1]):
            q += 1
        out.append(bytes([q - p - 1]) + raw[p:q])
        p = q
    return out


def packbits_encode(raw, policy, seed=0, row_bytes=None):
    """raw (the packed rows of a strip) -> one PackBits strip.  row_bytes: "max" and "noop" keep their runs inside rows of
    that many bytes, as libtiff does; "crossing" never does"""
    assert policy in PACKBITS
    raw = bytes(raw)
    rng = np.random.RandomState(seed)
    if policy == "literal1":
        return b"".join(b"\0" + raw[i:i + 1] for i in range(len(raw)))
    if policy == "crossing" or not row_bytes:
        runs = _greedy(raw)
    else:
        runs = [r for i in range(0, len(raw), row_bytes) for r in _greedy(raw[i:i + row_bytes])]
    if policy == "noop":
        runs = [r + b"\x80" * int(rng.randint(0, 3)) for r in runs] + [b"\x80"]
    return b"".join(runs)


def pack_rows(bits):
    """bits [rows, cols] (1 = a set bit) -> the packed rows, first pixel in a byte's top bit"""
    return np.packbits(np.asarray(bits, np.uint8), axis=1).tobytes()


# ---- the streams of test_t6_rewrap.py (CPU) and test_gpu_tiff_foreign.py: (name, stream, the picture as uint8 0 / 255) -----
def want_of(a, photo):
    """what a reader returns for strips whose set bits are `a` under Photometric `photo`"""
    return np.where(np.asarray(a, np.uint8) ^ (1 if photo == 0 else 0), 255, 0).astype(np.uint8)


def _variant(k):
    """Photometric, FillOrder and byte order from the bits of a counter, as tiff_cases.small_cases cycles them"""
    return k & 1, 1 + (k >> 1 & 1), "<>"[k >> 2 & 1]


def t6_strips(a, rps, policy, runs, ending, seed, stats=None):
    return [t6_encode(a[r:r + rps], policy, runs, ending, seed + r, stats) for r in range(0, a.shape[0], rps)]


@functools.lru_cache(maxsize=None)
def t6_dialects():
    """every small shape and content, RowsPerStrip 8 and rows, h-only and random modes, the five endings in turn"""
    out, k = [], 0
    for kind in tiff_cases.CONTENTS:
        for rows in tiff_cases.ROWS:
            for cols in tiff_cases.WIDTHS:
                a = tiff_cases.content(kind, rows, cols, seed=rows * 1000 + cols)
                for rps in sorted({min(8, rows), rows}):
                    for policy in ("h-only", "random"):
                        ending = ENDINGS[k % 5]
                        photo, fill, order = _variant(k)
                        s = tiff_ref.assemble(rows, cols, t6_strips(a, rps, policy, "fewest", ending, 7 * k), 4, photometric=photo,
                                              fill_order=fill, rps=rps, order=order)
                        out.append(("t6-%s-%s-%s-%dx%d-rps%d-p%d-f%d-%s" % (policy, ending, kind, rows, cols, rps, photo, fill, order), s,
                                    want_of(a, photo)))
                        k += 1
    return out


def long_pictures():
    a = np.zeros((2, 5200), np.uint8)
    a[0, 5000:] = 1
    return [("long-white", a), ("long-black", 1 - a), ("wide-white", np.zeros((1, 2561), np.uint8))]


@functools.lru_cache(maxsize=None)
def split_dialects():
    """-> (cases, stats): "split" runs on the contents with long runs, the counts of what the encoder wrote"""
    out, k, stats = [], 0, {}
    pics = [("%s-%d" % (kind, rows), tiff_cases.content(kind, rows, 257, seed=rows * 1000 + 257))
            for kind in ("white", "black", "endblack") for rows in tiff_cases.ROWS] + long_pictures()
    for name, a in pics:
        rows, cols = a.shape
        for rps in sorted({min(8, rows), rows}):
            for policy in ("h-only", "random"):
                ending = ENDINGS[k % 5]
                photo, fill, order = _variant(k)
                s = tiff_ref.assemble(rows, cols, t6_strips(a, rps, policy, "split", ending, 11 * k, stats), 4, photometric=photo,
                                      fill_order=fill, rps=rps, order=order)
                out.append(("split-%s-%s-%s-rps%d-p%d-f%d-%s" % (policy, ending, name, rps, photo, fill, order), s, want_of(a, photo)))
                k += 1
    return out, stats


WIDEST = 12288


@functools.lru_cache(maxsize=None)
def widest_rows():
    """2 x 12288 of single pixels: a row that begins black has a change at every column, and in horizontal mode costs 12 bits
    for two pixels -- 9216 bytes, more than the kernel's input window"""
    x = np.arange(WIDEST) & 1
    black_first = np.stack([1 - x, 1 - x]).astype(np.uint8)
    white_first = np.stack([x, 1 - x]).astype(np.uint8)
    out = []
    for pname, a in (("black-first-equal", black_first), ("white-first-inverse", white_first)):
        for policy in ("h-only", "libtiff"):
            s = tiff_ref.assemble(2, WIDEST, [t6_encode(a, policy, "fewest", "eofb")], 4)
            out.append(("widest-%s-%s" % (pname, policy), s, want_of(a, 0)))
    return out


@functools.lru_cache(maxsize=None)
def packbits_dialects():
    out, k = [], 0
    for kind in tiff_cases.CONTENTS:
        for rows in tiff_cases.ROWS:
            for cols in tiff_cases.WIDTHS:
                a = tiff_cases.content(kind, rows, cols, seed=rows * 1000 + cols)
                rb = (cols + 7) // 8
                for rps in sorted({1, min(8, rows), rows}):
                    for policy in PACKBITS:
                        photo, fill, order = _variant(k)
                        strips = [packbits_encode(pack_rows(a[r:r + rps]), policy, 13 * k + r, rb) for r in range(0, rows, rps)]
                        s = tiff_ref.assemble(rows, cols, strips, 32773, photometric=photo, fill_order=fill, rps=rps, order=order)
                        out.append(("packbits-%s-%s-%dx%d-rps%d-p%d-f%d-%s" % (policy, kind, rows, cols, rps, photo, fill, order), s,
                                    want_of(a, photo)))
                        k += 1
    return out


# libtiff estimates a missing StripByteCounts for a picture in one strip only; with several strips of Compression 4 or 32773
# Pillow raises OSError("decoder error -2") behind libtiff's 'MissingRequired: TIFF directory is missing required
# "StripByteCounts" field'.  These names are held to the picture they were made from and to the restatement alone.
NO_ARBITER = set()


def ifd_picture():
    """37 x 257: eight rows of random runs again and again, so that the strips of RowsPerStrip 8 hold equal bytes but the last"""
    return np.tile(tiff_cases.content("text", 8, 257, seed=77), (5, 1))[:37]


def strips_for(a, comp, rps):
    if comp == 4:
        return t6_strips(a, rps, "libtiff", "fewest", "eofb", 0)
    raw = [pack_rows(a[r:r + rps]) for r in range(0, a.shape[0], rps)]
    return raw if comp == 1 else [packbits_encode(x, "max", 0, (a.shape[1] + 7) // 8) for x in raw]


@functools.lru_cache(maxsize=None)
def ifd_dialects():
    """the forms of the assembler, missing tags, tag types and strip arrays over a G4, a PackBits and a raw picture"""
    a = ifd_picture()
    rows, cols = a.shape
    other = dict(rows=5, cols=40, strips=[pack_rows(tiff_cases.content("checker", 5, 40))], compression=1, photometric=1)
    many = [  # forms for a picture in five strips of 8 rows
        ("ifd-first", dict(ifd_first=True)), ("odd", dict(odd=True)), ("odd-ifd-first", dict(odd=True, ifd_first=True)),
        ("shuffled", dict(shuffle=5)), ("reverse-gaps", dict(reverse=True, gap=3)), ("gaps", dict(gap=5)), ("shared", dict(share=True)),
        ("shared-reverse", dict(share=True, reverse=True)), ("counts-over", dict(over=9)), ("chained", dict(chain=other)),
        ("chained-ifd-first", dict(chain=other, ifd_first=True)),
        ("extra-rational", dict(extra=[(282, 5, [300, 1]), (283, 5, [300, 1])])), ("extra-undefined", dict(extra=[(34377, 7, [1, 2, 3, 4, 5, 6])])),
        ("extra-unknown-type", dict(extra=[(65001, 99, [0x01020304])])),
        ("extra-ascii-long-short", dict(extra=[(305, 2, list(b"a scanner\0")), (65002, 4, [1, 2, 3]), (296, 3, [2]), (65003, 3, [7, 8, 9])])),
        ("no-counts", dict(drop=(279,))), ("no-counts-reverse-gaps", dict(drop=(279,), reverse=True, gap=3)),
        ("no-counts-ifd-first", dict(drop=(279,), ifd_first=True)), ("no-counts-shuffled-odd", dict(drop=(279,), shuffle=2, odd=True)),
        ("no-258", dict(drop=(258,))), ("no-277", dict(drop=(277,))), ("no-266", dict(drop=(266,))), ("no-293", dict(drop=(293,))),
        ("short-sizes", dict(extra=[(256, 3, [cols]), (257, 3, [rows]), (278, 3, [8])])),
        ("long-enums", dict(long_enums=True)), ("short-arrays-5", dict(offsets_type=3, counts_type=3)),
    ]
    one = [  # forms for a picture in one strip
        ("no-counts-one-strip", dict(drop=(279,))), ("no-counts-one-strip-ifd-first", dict(drop=(279,), ifd_first=True, gap=4)),
        ("no-278", dict(drop=(278,))), ("none-of-the-five", dict(drop=(258, 277, 266, 293, 278))),
        ("none-of-the-five-no-counts", dict(drop=(258, 277, 266, 293, 278, 279))),
        ("rps-ffffffff", dict(rps=0xffffffff)), ("rps-rows+5", dict(rps=rows + 5)),
    ]
    two = [("short-arrays-2", dict(offsets_type=3, counts_type=3))]
    out, k = [], 0
    for comp in (4, 32773, 1):
        for rps, forms in ((8, many), (rows, one), (19, two)):
            for name, kw in forms:
                kw = dict(kw)
                photo, fill, order = _variant(k)
                if 266 in kw.get("drop", ()):
                    fill = 1
                if kw.pop("long_enums", False):
                    kw["extra"] = [(259, 4, [comp]), (262, 4, [photo]), (266, 4, [fill])]
                if comp == 4 and name == "shared":
                    assert len(set(strips_for(a, comp, rps)[:4])) == 1
                s = tiff_ref.assemble(rows, cols, strips_for(a, comp, rps), comp, **dict(dict(photometric=photo, fill_order=fill, rps=rps, order=order), **kw))
                out.append(("ifd-%d-%s-p%d-f%d-%s" % (comp, name, photo, fill, order), s, want_of(a, photo)))
                if 279 in kw.get("drop", ()) and rps == 8 and comp != 1:
                    NO_ARBITER.add(out[-1][0])
                k += 1
    return out


def pins():
    """[(name, stream, code)]: the streams the device refuses, each with its code; Pillow reads some of them"""
    a = tiff_cases.content("text", 2, 200, seed=4)
    tab = by_run()
    # H W128 B0, H W2 B5, ... : a run of 0 inside a row
    row = np.zeros((1, 200), np.uint8)
    row[0, 130:135] = 1
    inner = _HORIZ + tab[0][128] + tab[0][0] + tab[1][0] + _HORIZ + tab[0][2] + tab[1][5] + _HORIZ + run_codes(65, 0) + tab[1][0] + _EOFB
    ext = "0000001111" + _HORIZ + tab[0][200 & ~63] + tab[0][200 & 63] + tab[1][0] + _EOFB  # the extension code where a mode code stands
    early = _row(changes(a[0]), [], 200, "libtiff", "fewest", None, None) + _EOFB  # EOFB where the second row begins

    def pack(s):
        s += "0" * (-len(s) % 8)
        return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))
    g4 = t6_encode(a)
    over = bytes([257 - 128, 0])  # 128 bytes of 0 for two white rows of 25 bytes
    return [
        ("an inner run of 0", tiff_ref.assemble(1, 200, [pack(inner)], 4), -215),
        ("a PackBits run past the strip's rows", tiff_ref.assemble(2, 200, [over], 32773), -215),
        ("orientation 3", tiff_ref.assemble(2, 200, [g4], 4, extra=[(274, 3, [3])]), -213),
        ("T6Options bit 1", tiff_ref.assemble(2, 200, [g4], 4, extra=[(293, 4, [2])]), -213),
        ("a byte count of 0", tiff_ref.assemble(2, 200, [g4], 4, extra=[(279, 4, [0])]), -5),
        ("an extension code", tiff_ref.assemble(1, 200, [pack(ext)], 4), -215),
        ("EOFB before the last row", tiff_ref.assemble(2, 200, [pack(early)], 4), -215),
    ]
