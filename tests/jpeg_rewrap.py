"""A coefficient-level rewriter of baseline JPEG streams, in the role tiff_ref.rewrap / assemble play for TIFF: it reads a
stream libjpeg wrote (jpeg_dec_ref.parse / unstuff / huff_decode give its quantised coefficients) and writes the same
coefficients, quantisation values and geometry again (jpeg_ref.huff_codes / block_bits emit them) in a dialect the caller
chooses -- so any conforming decoder returns the same picture, and Pillow's decode of the original is the expectation for
the rewritten stream.  Written from ITU T.81; pure Python and numpy.

What the caller chooses (rewrap's keywords):
  tables        the Huffman table shape, one for all or per component, each a kind or (DC kind, AC kind):
                  annexk   Annex K.3 - K.6, luma's for component 0 and chroma's for the others
                  lean     only the symbols the stream uses, all at one length
                  unused   lean, and five symbols the stream never uses listed behind them at a longer length
                  flat     every symbol at a length that the 9-bit first level resolves: DC 0..11 at 4 bits; all 256 AC
                           symbols, the 128 most frequent at 8 bits and the others at 9 (a length's count is one byte)
                  deep     the most frequent symbols get the longest codes: 16, 15, .. 11 bits for the six most frequent,
                           10 for every other used one; symbols the stream never uses fill lengths 2 .. 9 in front, so the
                           long codes sit high in the code space.  No all-ones code.
  ids           per component (Tq, Td, Ta); components that share an id share the table of the first
  dht / dqt     "each": a segment per table; "one": all tables in one segment
  decoy         every id is defined twice: a decoy before SOF, the real table behind SOF (the last definition wins)
  ri, dri       the restart interval in MCUs (0: none) and where DRI stands: "first", "after_sof" or "before_sos"
  pad           the bits that fill the last byte of every interval: "ones" (what encoders write), "zeros", "alt"
  extras        segments (marker, body) put between the tables: even ones behind the first DQT, odd ones behind the first DHT
  fill          0xFF fill bytes in front of every header marker behind SOI
  rst_fill      0xFF fill bytes in front of every RSTn
  eoi, tail     whether EOI is written, and bytes behind it
  gray_sampling the H << 4 | V a one-component frame declares
-> (stream, stats): stats counts what the emitted scan uses -- symbols, long (codes of more than 9 bits), sixteen (codes
of 16 bits), entropy (bytes between SOS and EOI)."""
import functools

import numpy as np

import jpeg_dec_ref as R
import jpeg_ref as E

_SOURCES = {}


def segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


class Source:
    """a stream taken apart: h (jpeg_dec_ref's header), coef [blocks][64] (zig-zag, DC values), comp (component of every
    block of an MCU), frame [(id, H << 4 | V, Tq)], app0 (the JFIF segment's body, or None)"""


def read(stream):
    stream = bytes(stream)
    if stream in _SOURCES:
        return _SOURCES[stream]
    code, h = R.parse(stream)
    assert code == 0, "the source stream must be one the restatement decodes (%d)" % code
    data, ivals, rst_ok = R.unstuff(stream, h.data)
    coef, code = R.huff_decode(h, data, ivals)
    assert code == 0 and rst_ok
    src = Source()
    src.h, src.coef = h, coef
    ny = h.hs * h.vs if h.ncomp == 3 else 1
    src.comp = [0] * ny + ([1, 2] if h.ncomp == 3 else [])
    src.app0, p = None, 2
    while True:     # the frame's own fields, which the restatement's header does not keep
        m, n = stream[p + 1], (stream[p + 2] << 8) | stream[p + 3]
        body = stream[p + 4:p + 2 + n]
        if m == 0xE0:
            src.app0 = body
        if m == 0xC0:
            src.frame = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(h.ncomp)]
            break
        p += 2 + n
    _SOURCES[stream] = src
    return src


def _block_symbols(blk, diff):
    """(the DC symbol, [AC symbols]) of one block, as jpeg_ref.block_bits emits them"""
    ac, run = [], 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            ac.append(0xF0)
            run -= 16
        ac.append((run << 4) | abs(v).bit_length())
        run = 0
    if run:
        ac.append(0x00)
    return abs(int(diff)).bit_length(), ac


def _from_lengths(pairs):
    """[(symbol, length)] -> (bits[16], vals) with the symbols of one length in the order given"""
    pairs = sorted(pairs, key=lambda sl: sl[1])     # stable
    bits = [0] * 16
    for _, ln in pairs:
        bits[ln - 1] += 1
    assert sum(b / (1 << (i + 1)) for i, b in enumerate(bits)) < 1, "Kraft's inequality, strictly: no all-ones code"
    return bits, [s for s, _ in pairs]


def make_table(kind, freq, dc, comp):
    """freq: {symbol: count} of what the table must code"""
    used = sorted(freq, key=lambda s: (-freq[s], s))
    universe = range(16) if dc else range(256)
    unused = [s for s in universe if s not in freq]
    if kind == "annexk":
        return (E.DC_LUMA, E.AC_LUMA)[not dc] if comp == 0 else (E.DC_CHROMA, E.AC_CHROMA)[not dc]
    if kind == "flat":
        if dc:
            return _from_lengths([(s, 4) for s in range(12)])
        order = used + unused       # a length holds at most 255 codes (its count is a byte): 128 at 8 bits, 128 at 9
        return _from_lengths([(s, 8) for s in sorted(order[:128])] + [(s, 9) for s in sorted(order[128:])])
    if kind in ("lean", "unused"):
        ln = max(1, len(used).bit_length())      # 2^ln >= used + 1
        pairs = [(s, ln) for s in sorted(used)]
        if kind == "unused":
            pairs += [(s, ln + 3) for s in unused[-5:]]
        return _from_lengths(pairs)
    if kind == "deep":
        pairs = [(s, 2 + i) for i, s in enumerate(unused[:8])]
        pairs += [(s, max(16 - i, 10)) for i, s in enumerate(used)]
        return _from_lengths(pairs)
    raise ValueError(kind)


def _decoy_for(table, dc):
    """another table than `table` for the same id: Annex K's luma table, or the flat one where that is the real one"""
    annex = E.DC_LUMA if dc else E.AC_LUMA
    same = (list(table[0]), list(table[1])) == (list(annex[0]), list(annex[1]))
    return make_table("flat", {}, dc, 0) if same else annex


_PAD = {"ones": "1111111", "zeros": "0000000", "alt": "0101010"}


def rewrap(stream, tables="annexk", ids=None, dht="each", dqt="each", decoy=False, ri=0, dri="first", pad="ones", extras=(),
           fill=0, rst_fill=0, eoi=True, tail=b"", gray_sampling=None):
    src = read(stream)
    h = src.h
    nc = h.ncomp
    if ids is None:
        ids = [(0, 0, 0)] + [(1, 1, 1)] * (nc - 1)
    ids = list(ids)[:nc]
    kinds = [tables] * nc if isinstance(tables, str) else list(tables)[:nc]
    kinds = [(k, k) if isinstance(k, str) else tuple(k) for k in kinds]
    mw, mh, bpm, nm, _ = R.geometry(h)
    per = ri if ri else nm                      # MCUs per interval
    # the symbols of every block, DC differences starting again in every interval
    syms = []
    last = [0] * nc
    for b in range(nm * bpm):
        if b % (per * bpm) == 0:
            last = [0] * nc
        c = src.comp[b % bpm]
        dc = int(src.coef[b, 0])
        syms.append((c, dc - last[c]) + _block_symbols(src.coef[b], dc - last[c]))
        last[c] = dc
    # one table per id, built for the symbols of every component that names it
    built = {}
    for c in range(nc):
        for tc in (0, 1):
            key = (tc, ids[c][1 + tc])
            if key in built:
                continue
            freq = {}
            for cb, _, dsym, acs in syms:
                if ids[cb][1 + tc] == key[1]:
                    for s in ([dsym] if tc == 0 else acs):
                        freq[s] = freq.get(s, 0) + 1
            built[key] = make_table(kinds[c][tc], freq, tc == 0, c)
    codes = {key: E.huff_codes(t) for key, t in built.items()}
    stats = dict(symbols=0, long=0, sixteen=0)
    for c, _, dsym, acs in syms:
        for key, ss in (((0, ids[c][1]), [dsym]), ((1, ids[c][2]), acs)):
            for s in ss:
                ln = codes[key][s][1]
                stats["symbols"] += 1
                stats["long"] += ln > 9
                stats["sixteen"] += ln == 16
    # the scan
    scan = bytearray()
    nint = -(-nm // per)
    for k in range(nint):
        parts = []
        for b in range(k * per * bpm, min((k + 1) * per, nm) * bpm):
            c, diff = syms[b][0], syms[b][1]
            parts.append(E.block_bits(src.coef[b], diff, codes[(0, ids[c][1])], codes[(1, ids[c][2])]))
        bits = "".join(parts)
        bits += _PAD[pad][:-len(bits) % 8]
        raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
        scan += raw.replace(b"\xff", b"\xff\x00")
        if k + 1 < nint:
            scan += b"\xff" * rst_fill + bytes([0xFF, 0xD0 + (k & 7)])
    stats["entropy"] = len(scan)
    # the header
    quant = {}
    for c in range(nc):
        quant.setdefault(ids[c][0], bytes(h.quant[c].astype(np.uint8)))

    def table_segments(marker, bodies, layout):
        return [segment(marker, b"".join(bodies))] if layout == "one" else [segment(marker, b) for b in bodies]

    dqt_bodies = [bytes([tq]) + q for tq, q in quant.items()]
    dht_bodies = [bytes([tc << 4 | th]) + bytes(t[0]) + bytes(t[1]) for (tc, th), t in built.items()]
    real_dqt, real_dht = table_segments(0xDB, dqt_bodies, dqt), table_segments(0xC4, dht_bodies, dht)
    sampling = [src.frame[c][1] for c in range(nc)]
    if gray_sampling is not None:
        assert nc == 1
        sampling[0] = gray_sampling
    sof = b"\x08" + h.rows.to_bytes(2, "big") + h.cols.to_bytes(2, "big") + bytes([nc])
    sof += b"".join(bytes([src.frame[c][0], sampling[c], ids[c][0]]) for c in range(nc))
    sos = bytes([nc]) + b"".join(bytes([src.frame[c][0], ids[c][1] << 4 | ids[c][2]]) for c in range(nc)) + b"\x00\x3f\x00"
    dri_seg = [segment(0xDD, ri.to_bytes(2, "big"))] if ri else []
    extras = [segment(m, b) for m, b in extras]
    segs = [segment(0xE0, src.app0)] if src.app0 is not None else []
    if dri == "first":
        segs += dri_seg
    if decoy:     # the tables SOS must not use: other quantisation values, and a table shape the real one does not have
        segs += table_segments(0xDB, [bytes([tq]) + bytes([7] * 64) for tq in quant], dqt)
        wrong = [_decoy_for(t, tc == 0) for (tc, th), t in built.items()]
        segs += table_segments(0xC4, [bytes([tc << 4 | th]) + bytes(w[0]) + bytes(w[1])
                                      for (tc, th), w in zip(built, wrong)], dht)
        segs += [segment(0xC0, sof)]
        if dri == "after_sof":
            segs += dri_seg
        segs += real_dqt[:1] + extras[0::2] + real_dqt[1:] + real_dht[:1] + extras[1::2] + real_dht[1:]
    else:
        segs += real_dqt[:1] + extras[0::2] + real_dqt[1:] + [segment(0xC0, sof)]
        if dri == "after_sof":
            segs += dri_seg
        segs += real_dht[:1] + extras[1::2] + real_dht[1:]
    if dri == "before_sos":
        segs += dri_seg
    segs += [segment(0xDA, sos)]
    out = b"\xff\xd8" + b"".join(b"\xff" * fill + s for s in segs) + bytes(scan)
    return out + (b"\xff\xd9" if eoi else b"") + bytes(tail), stats


# ---- the cases tests/test_jpeg_rewrap.py (CPU, against Pillow) and tests/test_gpu_jpeg_foreign.py (the kernels) both run

SPLIT = dict(tables=[("annexk", "annexk"), ("lean", "deep"), ("flat", "unused")], ids=[(0, 3, 3), (1, 1, 1), (2, 2, 2)])
_JUNK = np.random.Generator(np.random.PCG64(300)).integers(0, 256, 300, dtype=np.uint8).tobytes()

CASES = {
    # tables
    "flat": dict(tables="flat"),
    "deep": dict(tables="deep"),
    "split": SPLIT,
    "one_segment": dict(dht="one", dqt="one"),
    "one_segment_split": dict(dht="one", dqt="one", **SPLIT),
    "decoy": dict(decoy=True),
    "decoy_deep_one_segment": dict(decoy=True, tables="deep", dht="one", dqt="one"),
    "unused": dict(tables="unused"),
    "lean": dict(tables="lean"),
    # layout
    "dri_after_sof": dict(ri=2, dri="after_sof"),
    "dri_before_sos": dict(ri=2, dri="before_sos"),
    "com_and_app9": dict(extras=[(0xFE, b"c" * 65533), (0xE9, b"an unknown segment \xff\xd8\xff\xda" * 9)]),
    "fill_1": dict(fill=1),
    "fill_2": dict(fill=2, tables="lean"),
    "fill_7": dict(fill=7, ri=2, dri="before_sos"),
    "junk_after_eoi": dict(tail=_JUNK),
    # no "eoi_missing" (eoi=False): libjpeg supplies the marker, but Pillow feeds it through a suspending source and raises
    # "image file is truncated" when the data ends before EOI, so there is no arbiter for that stream
    # padding: the last byte of every restart interval and of the scan
    "pad_zeros": dict(pad="zeros", ri=3),
    "pad_alt": dict(pad="alt", ri=3),
    "pad_zeros_no_restart": dict(pad="zeros"),
    "pad_alt_no_restart": dict(pad="alt"),
    "deep_pad_ones": dict(tables="deep", pad="ones", ri=3),
    "deep_pad_zeros": dict(tables="deep", pad="zeros", ri=3),
    "deep_pad_alt": dict(tables="deep", pad="alt", ri=3),
    "flat_pad_ones": dict(tables="flat", pad="ones", ri=3),
    "flat_pad_zeros": dict(tables="flat", pad="zeros", ri=3),
    "flat_pad_alt": dict(tables="flat", pad="alt", ri=3),
    # restart
    "ri_partial": dict(ri=4),                 # 33 x 47: 6 or 3 MCUs a row, 30, 15 or 9 in all
    "ri_larger_than_the_scan": dict(ri=65535),
    "ri_every_mcu": dict(ri=1),               # 33 x 47: 9 intervals or more, RST7 is followed by RST0
    "fill_before_rst": dict(ri=2, rst_fill=3),
}
GROUPS = {
    "tables": ["flat", "deep", "split", "one_segment", "one_segment_split", "decoy", "decoy_deep_one_segment", "unused", "lean"],
    "layout": ["dri_after_sof", "dri_before_sos", "com_and_app9", "fill_1", "fill_2", "fill_7", "junk_after_eoi"],
    "padding": ["pad_zeros", "pad_alt", "pad_zeros_no_restart", "pad_alt_no_restart", "deep_pad_ones", "deep_pad_zeros",
                "deep_pad_alt", "flat_pad_ones", "flat_pad_zeros", "flat_pad_alt"],
    "restart": ["ri_partial", "ri_larger_than_the_scan", "ri_every_mcu", "fill_before_rst"],
}
assert sorted(sum(GROUPS.values(), [])) == sorted(CASES)
# the cases run on the large picture too: the scan spans more than one workgroup of the synchronisation kernel
BIG_CASES = ["flat", "deep", "split", "deep_pad_zeros", "flat_pad_alt", "pad_zeros_no_restart", "ri_partial", "fill_before_rst"]
BIG_BITS = 256 * 1024

SAMPLINGS = {"gray": dict(gray=True), "444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2)}
SHAPES = [(1, 1), (8, 8), (17, 9), (33, 47)]     # rows x cols; the last two have partial MCUs both ways at every sampling
GRAY_SAMPLINGS = [0x22, 0x21, 0x12]
GRAY_SHAPES = [(8, 8), (9, 17), (17, 9), (17, 17), (8, 9)]
_ORIGINALS = {}


def picture(rows, cols):
    """noise for the odd shapes, a card for the others"""
    from oics import synth
    if (rows + cols) % 2 == 0 or rows * cols > 4096:
        return np.random.Generator(np.random.PCG64(1000 * rows + cols)).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    return synth.make_color_card(rows, cols, 5)[0].copy()


def original(rows, cols, sampling, quality=None):
    """Pillow's stream of the picture of that shape (cached)"""
    import fuzz_jpeg_decode as fz
    key = (rows, cols, sampling, quality)
    if key not in _ORIGINALS:
        q = quality or (95, 90, 75)[(rows + cols) % 3]
        _ORIGINALS[key] = fz.make_stream(picture(rows, cols), q, **SAMPLINGS[sampling])
    return _ORIGINALS[key]


@functools.lru_cache(maxsize=None)
def case_streams(name):
    """[(what, original, rewritten, stats)] of one case: every sampling at a small shape and at both large ones"""
    out = []
    for si, sampling in enumerate(SAMPLINGS):
        for rows, cols in (SHAPES[(si + len(name)) % 2], SHAPES[2], SHAPES[3]):
            o = original(rows, cols, sampling)
            s, stats = rewrap(o, **CASES[name])
            out.append(((name, sampling, rows, cols), o, s, stats))
    return out


@functools.lru_cache(maxsize=None)
def big_streams():
    """[(what, original, rewritten, stats)]: 176 x 208 colour noise at quality 95, 4:2:0"""
    o = original(176, 208, "420", 95)
    return [((name, "big"), o) + rewrap(o, **CASES[name]) for name in BIG_CASES]


@functools.lru_cache(maxsize=None)
def gray_sampling_streams():
    """gray frames that declare 2 x 2, 2 x 1 or 1 x 2, in three dialects"""
    out = []
    for k, (rows, cols) in enumerate(GRAY_SHAPES):
        o = original(rows, cols, "gray")
        for hv in GRAY_SAMPLINGS:
            for name in ("lean", "deep_pad_zeros", "ri_every_mcu")[k % 3:][:2]:
                out.append(((name, "gray declared %02x" % hv, rows, cols), o) + rewrap(o, gray_sampling=hv, **CASES[name]))
    return out
