"""A restatement of the PNG encoder's rules (omrdeskew.h, the PNG encoding section) in numpy and
plain Python: the filter choice, the three candidate distances with their tie-break, the greedy parse in pieces, the
blocks' code construction (padding to two codes, weights scaled below a Fibonacci number, the merge order), the
run-length coding of the code lengths, the choice between stored, fixed and dynamic, and the placement with an empty
stored block behind every block but the last.  encode() writes the stream the device must write, byte for byte."""
import heapq
import struct
import zlib

import numpy as np

import png_ref
from png_ref import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_LIT, LEN_BASE, LEN_EXTRA, BitWriter, canonical

PIECE = 512
BLOCK_PIECES = 32
BLOCK = PIECE * BLOCK_PIECES
MAX_DISTANCE = 32768
BEFORE, AFTER = 8 + 25 + 8 + 2, 4 + 4 + 12
LIMIT15, LIMIT7 = 2584, 55  # Fibonacci(18), Fibonacci(10)
COLOR_TYPE = {1: 0, 3: 2, 4: 6}


def raw_bytes(rows, cols, cn):
    return rows * (1 + cols * cn)


def bound(rows, cols, cn):
    raw = raw_bytes(rows, cols, cn)
    return BEFORE + raw + 5 * ((raw + BLOCK - 1) // BLOCK) + AFTER


# ------------------------------------------------------------------------------------------------------ the filter
def samples(img):
    """gray / BGR / BGRA in memory -> the file's samples [rows, cols x cn]"""
    a = np.asarray(img)
    if a.ndim == 2:
        return a.astype(np.uint8)
    if a.shape[2] == 3:
        return a[..., ::-1].reshape(a.shape[0], -1).astype(np.uint8)
    return a[..., [2, 1, 0, 3]].reshape(a.shape[0], -1).astype(np.uint8)


def filtered(img):
    """every row with the filter of the smallest sum of |signed byte| (ties: the lowest type) -> the raw bytes"""
    s = samples(img).astype(np.int32)
    rows, rb = s.shape
    bpp = 1 if np.asarray(img).ndim == 2 else np.asarray(img).shape[2]
    out = np.zeros((rows, rb + 1), np.uint8)
    prev = np.zeros(rb, np.int32)
    for r in range(rows):
        cur = s[r]
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[:rb]
        ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[:rb]
        pa, pb, pc = abs(prev - ul), abs(left - ul), abs(left + prev - 2 * ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        cands = [cur & 255, (cur - left) & 255, (cur - prev) & 255, (cur - ((left + prev) >> 1)) & 255, (cur - paeth) & 255]
        sums = [int(np.where(c < 128, c, 256 - c).sum()) for c in cands]
        t = sums.index(min(sums))
        out[r, 0] = t
        out[r, 1:] = cands[t]
        prev = cur
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------------ matches
def distances(cn, row_bytes):
    """candidate number -> distance, None where the candidate is not tried"""
    d = [1, cn if cn > 1 else None, row_bytes + 1]
    if d[2] > MAX_DISTANCE:
        d[2] = None
    return d


def match_table(raw, dists):
    """per position (length, candidate) of the longest run, capped at 258; on equal length the earlier candidate"""
    n = len(raw)
    best_len = np.zeros(n, np.int64)
    best_c = np.zeros(n, np.int64)
    pos = np.arange(n)
    for c, d in enumerate(dists):
        if d is None:
            continue
        eq = np.zeros(n + 1, bool)
        eq[d:n] = raw[d:] == raw[:n - d]
        zeros = np.flatnonzero(~eq)
        run = np.minimum(zeros[np.searchsorted(zeros, pos)] - pos, 258)
        better = run > best_len
        best_len[better], best_c[better] = run[better], c
    return best_len, best_c


def parse(raw, best_len, best_c):
    """-> per piece its tokens: ints (literals) and (length, candidate) pairs; a match is cut at the piece's end"""
    pieces = []
    for start in range(0, len(raw), PIECE):
        end = min(start + PIECE, len(raw))
        pos, toks = start, []
        while pos < end:
            n = min(int(best_len[pos]), end - pos)
            if n >= 3:
                toks.append((n, int(best_c[pos])))
                pos += n
            else:
                toks.append(int(raw[pos]))
                pos += 1
        pieces.append(toks)
    return pieces


# ------------------------------------------------------------------------------------------------------ code sets
def length_symbol(n):
    k = 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)
    return k, LEN_EXTRA[k], n - LEN_BASE[k]


def distance_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def code_lengths(freq, limit):
    """Huffman code lengths: pad to two symbols with the lowest unused ones, scale the weights to max(1, f >> s) for the
    smallest s whose sum is below `limit`, merge the two smallest (weight, index); merge number m has index n + m"""
    n = len(freq)
    w = list(freq)
    i = 0
    while sum(1 for v in w if v) < 2:
        if w[i] == 0:
            w[i] = 1
        i += 1
    s = 0
    while sum(max(1, v >> s) for v in w if v) >= limit:
        s += 1
    heap = [(max(1, v >> s), i) for i, v in enumerate(w) if v]
    heapq.heapify(heap)
    parent = {}
    nxt = n
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1]] = parent[b[1]] = nxt
        heapq.heappush(heap, (a[0] + b[0], nxt))
        nxt += 1
    root = heap[0][1]
    lens = [0] * n
    for i, v in enumerate(w):
        if v:
            j = i
            while j != root:
                j = parent[j]
                lens[i] += 1
    return lens


def runs(seq):
    """the code lengths of both sets as one sequence -> [(code-length symbol, extra value, extra bits)]"""
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


def block_bytes(tokens, raw_block, dists, last, stored_only=False):
    """one block (its tokens, its raw bytes) -> (type, its bytes in the stream)"""
    stored = bytes([1 if last else 0]) + struct.pack("<HH", len(raw_block), ~len(raw_block) & 0xffff) + bytes(raw_block)
    if stored_only:
        return 0, stored
    fl, fd = [0] * 286, [0] * 30
    dsym = [distance_symbol(d) if d else None for d in dists]
    for t in tokens:
        if isinstance(t, int):
            fl[t] += 1
        else:
            fl[257 + length_symbol(t[0])[0]] += 1
            fd[dsym[t[1]][0]] += 1
    fl[256] += 1
    len_l, len_d = code_lengths(fl, LIMIT15), code_lengths(fd, LIMIT15)
    hlit = max(257, max(i for i in range(286) if len_l[i]) + 1)
    hdist = max(1, max(i for i in range(30) if len_d[i]) + 1)
    rl = runs(len_l[:hlit] + len_d[:hdist])
    fc = [0] * 19
    for sym, _, _ in rl:
        fc[sym] += 1
    len_c = code_lengths(fc, LIMIT7)
    hclen = max(4, max(i for i in range(19) if len_c[CL_ORDER[i]]) + 1)

    def write(kind, lit_lens, dist_lens):
        w = BitWriter()
        w.bits(1 if last else 0, 1)
        w.bits(kind, 2)
        if kind == 2:
            w.bits(hlit - 257, 5), w.bits(hdist - 1, 5), w.bits(hclen - 4, 4)
            for i in range(hclen):
                w.bits(len_c[CL_ORDER[i]], 3)
            cc = canonical(len_c)
            for sym, extra, nbits in rl:
                w.code(*cc[sym])
                w.bits(extra, nbits)
        cl, cd = canonical(lit_lens), canonical(dist_lens)
        for t in tokens:
            if isinstance(t, int):
                w.code(*cl[t])
                continue
            k, eb, ev = length_symbol(t[0])
            w.code(*cl[257 + k])
            w.bits(ev, eb)
            k, eb, ev = dsym[t[1]]
            w.code(*cd[k])
            w.bits(ev, eb)
        w.code(*cl[256])
        if not last:
            w.bits(0, 3)
            w.done()
            w.out += b"\x00\x00\xff\xff"
        return w.done()

    best = (0, stored)
    fixed = write(1, FIXED_LIT, [5] * 30)
    if len(fixed) < len(best[1]):
        best = (1, fixed)
    dynamic = write(2, len_l, len_d)
    if len(dynamic) < len(best[1]):
        best = (2, dynamic)
    return best


def deflate_blocks(raw, cn, row_bytes, compression=1):
    """-> [(type, bytes)] per block of the raw data"""
    raw = np.asarray(raw, np.uint8)
    stored_only = min(max(int(compression), 0), 9) == 0
    dists = distances(cn, row_bytes)
    pieces = None if stored_only else parse(raw, *match_table(raw, dists))
    out = []
    nblk = (len(raw) + BLOCK - 1) // BLOCK
    for b in range(nblk):
        toks = [] if stored_only else [t for p in pieces[b * BLOCK_PIECES:(b + 1) * BLOCK_PIECES] for t in p]
        out.append(block_bytes(toks, raw[b * BLOCK:(b + 1) * BLOCK].tobytes(), dists, b == nblk - 1, stored_only))
    return out


def encode(img, compression=1):
    """gray [rows, cols], BGR [rows, cols, 3] or BGRA [rows, cols, 4] -> the stream"""
    a = np.asarray(img)
    rows, cols = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    raw = filtered(a)
    body = b"".join(d for _, d in deflate_blocks(raw, cn, cols * cn, compression))
    zs = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xffffffff)
    return png_ref.assemble(rows, cols, COLOR_TYPE[cn], 8, zs)


def block_types(stream):
    """walks the block headers of a stream's deflate data with png_ref's inflate rules -> the BTYPEs met, in order
    (the empty stored blocks between the blocks included)"""
    code, h = png_ref.parse(stream)
    assert code == 0
    zs = h.idat
    r = png_ref._Reader(zs, len(zs) - 4)
    r.pos = 16
    kinds = []
    last = 0
    while not last:
        last, kind = r.bit(), r.bits(2)
        kinds.append(kind)
        if kind != 0:
            return kinds + ["compressed"]
        r.pos = (r.pos + 7) & ~7
        n, nn = r.bits(16), r.bits(16)
        assert n == (~nn & 0xffff)
        r.pos += 8 * n
    return kinds
