"""Crafted canvases that drive libjpeg's baseline entropy coder to the Huffman symbols ordinary content never writes, and a
histogram of what a canvas reaches.  numpy only; every figure comes from tests/jpeg_ref.py (scan_blocks and the run/size
walk of block_bits), which tests/test_jpeg_cases.py holds to Pillow on every canvas here.

  symbols(img, quality)        what the scan of img writes: AC symbols and DC categories per table, ZRLs, the longest block
  basis_canvas(q, saturated)   gray: a block per zig-zag position 1..63 x size 1..10 x sign, a single DCT basis function
  chroma_canvas(q)             BGR: the same in Cb and in Cr, in 16 x 16 cells of 2 x 2 replicated samples
  dc_staircase(q, colour)      flat blocks (cells) whose successive DC differences land in every category that q allows
  zrl_canvas(q)                gray: blocks whose only AC coefficients sit at zig-zag 17, 33, 49 and 63
  binary_canvas(colour)        every pixel 0 or 255: the longest blocks
  cases()                      every (name, canvas, quality) the tests run, built once
  crops()                      windows of them with heights and widths of 8 k + 1 and 16 k + 1
  explain(img, q, got, want)   the first differing byte of two streams, and the block and symbol it falls in
"""
import collections
import functools
import itertools

import numpy as np

import jpeg_ref

BLOCKS_PER_ROW = 32     # gray canvases: 256 pixels wide
CELLS_PER_ROW = 20      # colour canvases: 320 pixels wide
STAIR_BLOCKS_PER_ROW = 20

Symbols = collections.namedtuple("Symbols", "ac dc dc_signed max_zrl max_block_bits zrl_counts")

_CODES = {"dc": [jpeg_ref.huff_codes(jpeg_ref.DC_LUMA), jpeg_ref.huff_codes(jpeg_ref.DC_CHROMA)],
          "ac": [jpeg_ref.huff_codes(jpeg_ref.AC_LUMA), jpeg_ref.huff_codes(jpeg_ref.AC_CHROMA)]}


def _nbits(v):
    return int(abs(int(v))).bit_length()


def block_walk(blk, dc_diff, table):
    """[(kind, symbol, zig-zag position, bits)] of one block in the order block_bits writes them; kind "dc", "zrl", "ac" or
    "eob"; bits = the code's length plus the value bits behind it"""
    out = [("dc", _nbits(dc_diff), 0, _CODES["dc"][table][_nbits(dc_diff)][1] + _nbits(dc_diff))]
    ac = _CODES["ac"][table]
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(("zrl", 0xF0, k, ac[0xF0][1]))
            run -= 16
        sym = (run << 4) | _nbits(v)
        out.append(("ac", sym, k, ac[sym][1] + _nbits(v)))
        run = 0
    if run:
        out.append(("eob", 0x00, 63, ac[0x00][1]))
    return out


def scan_walk(blocks):
    """[(component, table, DC difference, block_walk)] of scan_blocks' list"""
    last = [0, 0, 0]
    out = []
    for comp, blk in blocks:
        t = 0 if comp == 0 else 1
        diff = int(blk[0]) - last[comp]
        last[comp] = int(blk[0])
        out.append((comp, t, diff, block_walk(blk, diff, t)))
    return out


def symbols_of(blocks):
    ac, dc, dcs = [set(), set()], [set(), set()], [set(), set()]
    max_bits = 0
    zrls = set()
    for _, t, diff, walk in scan_walk(blocks):
        dc[t].add(_nbits(diff))
        dcs[t].add(_nbits(diff) if diff >= 0 else -_nbits(diff))
        zrl = 0
        for kind, sym, _, _ in walk[1:]:
            ac[t].add(sym)
            if kind == "ac":
                zrls.add(zrl)
            zrl = zrl + 1 if kind == "zrl" else 0
        max_bits = max(max_bits, sum(w[3] for w in walk))
    return Symbols(ac, dc, dcs, max(zrls, default=0), max_bits, zrls)


def symbols(img, quality):
    """Symbols(ac, dc, dc_signed, max_zrl, max_block_bits, zrl_counts): ac[t], dc[t] the sets of AC symbols (ZRL 0xF0 and
    EOB 0x00 among them) and DC categories written with table t (0 luma, 1 chroma); dc_signed[t] the categories with the
    sign of the difference; the largest number of ZRLs in front of one coefficient; the largest bit length of one block;
    the set of ZRL counts seen in front of a coefficient"""
    return symbols_of(jpeg_ref.scan_blocks(img, quality))


ALL_AC = frozenset([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])
assert len(ALL_AC) == 162 and ALL_AC == set(jpeg_ref.AC_LUMA[1]) == set(jpeg_ref.AC_CHROMA[1])


def basis(n):
    """the orthonormal 8 x 8 DCT basis function of natural index n (row = vertical frequency n // 8)"""
    r, c = divmod(int(n), 8)
    x = (2 * np.arange(8) + 1) * np.pi / 16
    scale = [np.sqrt(0.125) if f == 0 else 0.5 for f in (r, c)]
    return np.outer(scale[0] * np.cos(x * r), scale[1] * np.cos(x * c))


def middle(s):
    """the middle of size category s: 1, 2.5, 5.5, 11.5, .."""
    return ((1 << (s - 1)) + (1 << s) - 1) / 2


def _px(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _tile(blocks, per_row, side, fill):
    """blocks of side x side (x 3) pixels, per_row to a canvas row, the last row completed with `fill`"""
    blocks = list(blocks)
    while len(blocks) % per_row:
        blocks.append(np.broadcast_to(np.asarray(fill, np.uint8), blocks[0].shape))
    rows = [np.concatenate(blocks[i:i + per_row], axis=1) for i in range(0, len(blocks), per_row)]
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def basis_canvas(quality, saturated):
    """gray, 32 blocks per row: for zig-zag position k = 1..63, size s = 1..10 and both signs the block
    128 + c * B, c = +/- middle(s) x the luma quantiser of ZIGZAG[k].  Where that leaves 0..255 the unsaturated form drops
    the block; the saturated form takes 128 +/- 127.5 * sign(B) (once per position and sign)."""
    ql = jpeg_ref.quant_tables(quality)[0]
    blocks = []
    for k in range(1, 64):
        n = jpeg_ref.ZIGZAG[k]
        b = basis(n)
        done = set()
        for s in range(1, 11):
            for sign in (1, -1):
                a = 128 + sign * middle(s) * float(ql[n]) * b
                if a.min() < 0 or a.max() > 255:
                    if not saturated or sign in done:
                        continue
                    done.add(sign)
                    a = 128 + sign * 127.5 * np.sign(b)
                blocks.append(_px(a))
    return _tile(blocks, BLOCKS_PER_ROW, 8, 128)


# JFIF's YCbCr -> RGB, as offsets of (R, G, B) from Y for cb, cr measured from 128
def _rgb_offsets(cb, cr):
    return np.stack([1.402 * cr, -0.344136 * cb - 0.714136 * cr, 1.772 * cb], -1)


BLACK, WHITE, GRAY = (0, 0, 0), (255, 255, 255), (128, 128, 128)
BLUE, YELLOW, RED, CYAN = (255, 0, 0), (0, 255, 255), (0, 0, 255), (255, 255, 0)      # BGR
_EXTREMES = ((BLUE, YELLOW), (RED, CYAN))      # Cb = 255 / 0 at Cr near 128, Cr = 255 / 0 at Cb near 128


def _cell(samples_bgr):
    """8 x 8 chroma samples (BGR each) -> a 16 x 16 cell, each sample 2 x 2: h2v2_downsample returns the samples"""
    return np.repeat(np.repeat(samples_bgr, 2, 0), 2, 1)


def _flat_cell(bgr):
    return np.broadcast_to(np.asarray(bgr, np.uint8), (16, 16, 3)).copy()


def chroma_cell(d, axis):
    """the cell whose Cb (axis 0) or Cr (axis 1) block is 128 + d (d: 8 x 8) with the other at 128 and Y as near 128 as
    the RGB cube allows; None where some sample has no Y at all inside the cube"""
    zero = np.zeros_like(d)
    off = _rgb_offsets(d, zero) if axis == 0 else _rgb_offsets(zero, d)
    lo, hi = (-off).max(-1), (255 - off).min(-1)
    if (lo > hi).any():
        return None
    y = np.clip(128.0, lo, hi)
    rgb = _px(y[..., None] + off)
    return _cell(rgb[..., ::-1])


def chroma_canvas(quality):
    """BGR, 20 cells of 16 x 16 per row.  For zig-zag position k = 1..63 and size s = 1..10 one cell whose Cb block
    (k + s even) or Cr block (odd) is 128 + c * B, c = +/- middle(s) x the chroma quantiser, the sign alternating; outside
    the RGB cube the cell takes the two extreme colours of its axis by sign(B) (once per position and axis).  Then a row of
    flat cells alternating black / white, blue / yellow, red / cyan: DC differences of -1024 .. +1016 at quality 100 in Y,
    Cb and Cr."""
    qc = jpeg_ref.quant_tables(quality)[1]
    cells = []
    for k in range(1, 64):
        n = jpeg_ref.ZIGZAG[k]
        b = basis(n)
        done = set()
        for s in range(1, 11):
            axis = (k + s) & 1
            sign = 1 if ((k + s) >> 1) & 1 == 0 else -1
            cell = chroma_cell(sign * middle(s) * float(qc[n]) * b, axis)
            if cell is None:
                if (axis, sign) in done:
                    continue
                done.add((axis, sign))
                hi, lo = _EXTREMES[axis]
                cell = _cell(np.where((sign * b > 0)[..., None], np.asarray(hi, np.uint8), np.asarray(lo, np.uint8)))
            cells.append(cell)
    while len(cells) % CELLS_PER_ROW:
        cells.append(_flat_cell(GRAY))
    flat = [BLACK, WHITE, BLACK, WHITE, GRAY, BLUE, YELLOW, BLUE, YELLOW, GRAY, RED, CYAN, RED, CYAN, GRAY, WHITE, BLUE, RED,
            YELLOW, CYAN]
    assert len(flat) == CELLS_PER_ROW
    cells += [_flat_cell(c) for c in flat]
    return _tile(cells, CELLS_PER_ROW, 16, GRAY)


def _targets():
    """(category, sign) of the DC differences a staircase asks for: the longest codes first"""
    return [(n, sg) for n in range(11, 0, -1) for sg in (1, -1)] + [(0, 1)]


def _in_category(diff, n, sg):
    return _nbits(diff) == n and (diff == 0 or (diff > 0) == (sg > 0))


@functools.lru_cache(maxsize=None)
def _flat_dc(quality, colour):
    """the quantised DC of flat blocks: gray -> ([values], [[dc]]); colour -> a pool of flat colours along black - white,
    blue - yellow and red - cyan with their (Y, Cb, Cr) DCs, through the restatement itself"""
    if not colour:
        pool = [(v,) for v in range(256)]
        img = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(8, 32), 8, 0), 8, 1)
        dcs = [(int(b[0]),) for _, b in jpeg_ref.scan_blocks(img, quality)]
        return pool, dcs
    pool = []
    for t in range(0, 256, 3):
        pool += [(t, t, t), (t, 255 - t, 255 - t), (255 - t, 255 - t, t)]
    while len(pool) % 16:
        pool.append(GRAY)
    img = _tile([_flat_cell(c) for c in pool], 16, 16, GRAY)
    blocks = jpeg_ref.scan_blocks(img, quality)
    dcs = [tuple(int(blocks[6 * i + j][1][0]) for j in (0, 4, 5)) for i in range(len(pool))]
    return pool, dcs


def staircase_sequence(quality, colour):
    """indices into _flat_dc's pool: successive flat blocks whose DC difference (in Y for gray; in Y, then Cb, then Cr for
    colour) lands in each category 11 .. 0 with both signs, where the quantiser of `quality` allows it at all.  A target
    the current value cannot reach directly is reached from an extreme value put in between."""
    pool, dcs = _flat_dc(quality, colour)
    ncomp = 3 if colour else 1
    start = pool.index(GRAY if colour else (128,))
    seq = [start]
    for comp in range(ncomp):
        ends = (min(range(len(pool)), key=lambda i: dcs[i][comp]), max(range(len(pool)), key=lambda i: dcs[i][comp]))
        for n, sg in _targets():
            for via in (None, ends[0] if sg > 0 else ends[1]):
                cur = seq[-1] if via is None else via
                hit = [i for i in range(len(pool)) if _in_category(dcs[i][comp] - dcs[cur][comp], n, sg)]
                if hit:
                    if via is not None:
                        seq.append(via)
                    # the candidate nearest the middle of the pool's range, so that the walk keeps room on both sides
                    mid = (dcs[ends[0]][comp] + dcs[ends[1]][comp]) / 2
                    seq.append(min(hit, key=lambda i: (abs(dcs[i][comp] - mid), i)))
                    break
    return seq


def ff_tail_block():
    """a gray block whose last coefficient (zig-zag 63) quantises to 255 at quality 100: size 8 with value bits 11111111,
    and no EOB behind it, so a stream that ends with this block ends with 0xFF once padded"""
    b = basis(63)
    for c in np.arange(253.0, 257.0, 0.125):
        blk = _px(128 + c * b)
        if int(jpeg_ref.scan_blocks(blk, 100)[0][1][63]) == 255:
            return blk
    raise AssertionError("no amplitude quantises to 255")


def dc_staircase(quality, colour=False, blocks=320):
    """flat blocks (gray, 20 per row) or flat 16 x 16 cells (BGR, 20 per row): staircase_sequence repeated to `blocks`
    blocks, so that the prediction runs across row ends and across the 256-block segments of the device's scans.  The
    cycle starts where its largest difference (in Y for gray, in Cb for colour) falls on the first block of the second
    segment: block 256 of a gray scan, the Cb block of MCU 42 (block 256 = 6 * 42 + 4) of a BGR one.  The gray form ends
    with ff_tail_block()."""
    pool, dcs = _flat_dc(quality, colour)
    seq = staircase_sequence(quality, colour)
    comp, at = (1, 42) if colour else (0, 256)
    step = [abs(dcs[seq[j]][comp] - dcs[seq[j - 1]][comp]) for j in range(len(seq))]
    first = (step.index(max(step)) - at) % len(seq)
    idx = list(itertools.islice(itertools.cycle(seq[first:] + seq[:first]), blocks))
    if colour:
        return _tile([_flat_cell(pool[i]) for i in idx], CELLS_PER_ROW, 16, GRAY)
    out = [np.full((8, 8), pool[i][0], np.uint8) for i in idx]
    out[-1] = ff_tail_block()
    return _tile(out, STAIR_BLOCKS_PER_ROW, 8, 128)


ZRL_POSITIONS = (17, 33, 49, 63)


def zrl_canvas(quality):
    """gray, 32 blocks per row: for every non-empty subset of zig-zag positions 17, 33, 49, 63, sizes 1..3 and both signs
    the block 128 + sum of c_k * B_k: one, two or three ZRLs in front of a coefficient, EOB behind it or (63) none.
    A block that would leave 0..255 is dropped."""
    ql = jpeg_ref.quant_tables(quality)[0]
    blocks = []
    for m in range(1, 16):
        ks = [k for i, k in enumerate(ZRL_POSITIONS) if m >> i & 1]
        for s in (1, 2, 3):
            for sign in (1, -1):
                a = np.full((8, 8), 128.0)
                for j, k in enumerate(ks):
                    n = jpeg_ref.ZIGZAG[k]
                    a += (sign if j % 2 == 0 else -sign) * middle(s) * float(ql[n]) * basis(n)
                if a.min() >= 0 and a.max() <= 255:
                    blocks.append(_px(a))
    return _tile(blocks, BLOCKS_PER_ROW, 8, 128)


def binary_canvas(colour=False):
    """64 x 256 pixels, each 0 or 255 (black or white in the BGR form): the whole sample range in every coefficient, so at
    quality 100 nearly every AC coefficient is of size 7 or 8 -- the longest blocks 8-bit content gives"""
    rng = np.random.Generator(np.random.PCG64(11))
    img = (rng.integers(0, 2, (64, 256), dtype=np.uint8) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(img[..., None], 3, 2)) if colour else img


BASIS_QUALITIES = (100, 98, 95, 90, 75, 50, 25)
CHROMA_QUALITIES = (100, 98, 95, 90, 75)
STAIR_QUALITIES = (100, 95, 75)
ZRL_QUALITIES = (75, 50)

# (case, first row, first column, rows, cols): windows whose height and width are 16 k + 1 or 8 k + 1 with k odd.  In the
# BGR ones the last MCU column or row then holds dummy blocks beside flat cells of the extreme colours: cells 6, 7 and
# 24 .. 26 of the colour staircase at quality 100 swing between black and white; the last 16 rows of a chroma canvas are
# its flat cells, black and white first.  tests/test_jpeg_cases.py counts the MCUs this gives.
CROPS = (("stair-colour-q100", 0, 48, 17, 49), ("stair-colour-q100", 0, 64, 33, 41), ("stair-colour-q100", 0, 80, 41, 33),
         ("chroma-q100", -32, 0, 17, 49), ("chroma-q100", -32, 0, 25, 57),
         ("stair-q100", 0, 0, 33, 41), ("basis-sat-q100", 8, 0, 41, 33), ("binary-q100", 0, 0, 17, 49))


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, canvas, quality)]: every crafted canvas with the qualities it is run at"""
    out = []
    for q in BASIS_QUALITIES:
        out.append(("basis-q%d" % q, basis_canvas(q, False), q))
        out.append(("basis-sat-q%d" % q, basis_canvas(q, True), q))
    for q in CHROMA_QUALITIES:
        out.append(("chroma-q%d" % q, chroma_canvas(q), q))
    for q in STAIR_QUALITIES:
        out.append(("stair-q%d" % q, dc_staircase(q), q))
        out.append(("stair-colour-q%d" % q, dc_staircase(q, True), q))
    for q in ZRL_QUALITIES:
        out.append(("zrl-q%d" % q, zrl_canvas(q), q))
    out.append(("binary-q100", binary_canvas(), 100))
    out.append(("binary-colour-q100", binary_canvas(True), 100))
    for _, img, _ in out:
        img.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def crops():
    """[(name, canvas, quality)] of CROPS"""
    out = []
    for name, y0, x0, rows, cols in CROPS:
        _, img, q = case(name)
        y0 %= img.shape[0]
        c = np.ascontiguousarray(img[y0:y0 + rows, x0:x0 + cols])
        assert c.shape[:2] == (rows, cols)
        c.setflags(write=False)
        out.append(("%s-crop-%dx%d" % (name, rows, cols), c, q))
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


def names(colour=None):
    return [n for n, img, _ in cases() if colour is None or (img.ndim == 3) == colour]


@functools.lru_cache(maxsize=None)
def case_blocks(name):
    """scan_blocks of a case, computed once"""
    _, img, q = case(name)
    return jpeg_ref.scan_blocks(img, q)


def noise(cn):
    """the suite's 150 x 270 noise (tests/test_gpu_jpeg.py's _image)"""
    rng = np.random.Generator(np.random.PCG64(1000 * 150 + 270 + 7 * cn))
    return rng.integers(0, 256, (150, 270) if cn == 1 else (150, 270, 3), dtype=np.uint8)


def scan_of(stream):
    """(offset of the entropy-coded bytes, those bytes with the stuffing removed) of a stream without restart markers"""
    sos = stream.index(b"\xff\xda")
    start = sos + 2 + ((stream[sos + 2] << 8) | stream[sos + 3])
    assert stream[-2:] == b"\xff\xd9"
    return start, stream[start:-2].replace(b"\xff\x00", b"\xff")


def explain(img, quality, got, want):
    """where two streams of img first differ: the byte offset and, from the restatement's walk, the block (scan index,
    component) and the symbol that byte of `want` belongs to"""
    n = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    msg = "first difference at byte %d of %d (got %d bytes)" % (n, len(want), len(got))
    start, _ = scan_of(want)
    if n < start:
        return msg + ": in the header"
    bit = 8 * (n - start - want[start:n].count(b"\xff\x00"))
    at = 0
    for i, (comp, t, diff, walk) in enumerate(scan_walk(jpeg_ref.scan_blocks(img, quality))):
        for kind, sym, k, bits in walk:
            if at + bits > bit:
                return msg + ": scan bit %d, block %d (component %d), %s symbol 0x%02X at zig-zag %d (bits %d..%d), table %s" % (
                    bit, i, comp, kind, sym, k, at, at + bits - 1, "luma" if t == 0 else "chroma")
            at += bits
    return msg + ": in the padding or EOI"
