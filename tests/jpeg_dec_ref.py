"""numpy restatement of the baseline JPEG decoder of csrc/jpeg_dec.hip: what libjpeg gives with its
defaults (JDCT_ISLOW, fancy up-sampling, no scaling), which is what imread and Pillow return.  Written from the JPEG
standard (ITU T.81) and libjpeg's published algorithm; held to Pillow in tests/test_jpeg_dec_ref.py, and the kernels are
held to the same arbiter.  Stages, each a function of its own:

  parse          the marker parser: tables, frame, scan, what is refused (NOTIMPL) and what is malformed (BADARG)
  unstuff        0xFF 0x00 -> 0xFF, RSTn positions, the scan's end: one byte string and the intervals' byte offsets
  huff_decode    a plain sequential Huffman decoder: coefficients [blocks][64] in zig-zag order, DC differences summed
  selfsync       the self-synchronising scheme as the kernels run it, the subsequence length a parameter
  idct           de-quantisation and jidctint.c (CONST_BITS 13, PASS1_BITS 2), + 128, clamped
  upsample       h2v1 / h2v2 fancy up-sampling with libjpeg's edge rules
  ycc_to_bgr     ycc_rgb_convert's 16-bit fixed-point tables
  decode         the whole file -> (rows, cols) or (rows, cols, 3) BGR
"""
import numpy as np

OK, NOTIMPL, BADARG, ASSERT = 0, -213, -5, -215


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order)


ZIGZAG = _zigzag()   # ZIGZAG[k] = natural index of the k-th coefficient in zig-zag order


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


class Header:
    """what the scan needs: rows, cols, ncomp, hs, vs (Y's sampling; chroma is 1 x 1), ri (restart interval, 0: none),
    quant[c] (64, zig-zag order), dc[c] / ac[c] ((bits, vals) per component), data (offset of the entropy data)"""


def _orientation(body):
    """the EXIF orientation of an APP1 body, or 1"""
    if len(body) < 14 or body[:6] != b"Exif\x00\x00":
        return 1
    t = body[6:]
    if t[:4] == b"II*\x00":
        order = "little"
    elif t[:4] == b"MM\x00*":
        order = "big"
    else:
        return 1
    ifd = int.from_bytes(t[4:8], order)
    if ifd + 2 > len(t):
        return 1
    n = int.from_bytes(t[ifd:ifd + 2], order)
    for e in range(n):
        o = ifd + 2 + 12 * e
        if o + 12 > len(t):
            break
        if int.from_bytes(t[o:o + 2], order) == 0x0112:
            return int.from_bytes(t[o + 8:o + 10], order)
    return 1


def parse(stream):
    """-> (code, Header or None).  The header is returned with its size whenever SOF was readable."""
    s = bytes(stream)
    h = Header()
    h.rows = h.cols = h.ncomp = h.hs = h.vs = 0
    try:
        _parse(s, h)
        return OK, h
    except Refused as e:
        return e.code, (h if h.rows or h.cols else None)


def _parse(s, h):
    if len(s) < 4 or s[0] != 0xFF or s[1] != 0xD8:
        raise Refused(BADARG, "no SOI")
    qt, dht = {}, {}
    jfif = adobe = False
    orient = 1
    frame = None
    h.ri = 0
    p = 2
    while True:
        if p + 4 > len(s):
            raise Refused(BADARG, "the stream ends before SOS")
        if s[p] != 0xFF:
            raise Refused(BADARG, "no marker where one must be")
        m = s[p + 1]
        if m == 0xFF:       # fill byte
            p += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:   # stand-alone markers
            p += 2
            continue
        if m == 0xD9:
            raise Refused(BADARG, "EOI before SOS")
        n = (s[p + 2] << 8) | s[p + 3]
        if n < 2 or p + 2 + n > len(s):
            raise Refused(BADARG, "a segment runs past the end")
        body = s[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq:
                    raise Refused(NOTIMPL, "16-bit quantisation table")
                if tq > 3 or q + 65 > len(body):
                    raise Refused(BADARG, "bad DQT")
                qt[tq] = np.frombuffer(body[q + 1:q + 65], np.uint8).astype(np.int64)
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                if q + 17 > len(body):
                    raise Refused(BADARG, "bad DHT")
                tc, th = body[q] >> 4, body[q] & 15
                bits = list(body[q + 1:q + 17])
                nv = sum(bits)
                if tc > 1 or th > 3 or nv > 256 or q + 17 + nv > len(body):
                    raise Refused(BADARG, "bad DHT")
                code = 0
                for ln in range(16):    # the code space must not overflow
                    code = (code + bits[ln]) << 1
                    if code > (2 << (ln + 1)):
                        raise Refused(BADARG, "bad DHT")
                dht[(tc, th)] = (bits, list(body[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xC0 or (0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            if frame is not None:
                raise Refused(BADARG, "two frames")
            if len(body) < 6:
                raise Refused(BADARG, "bad SOF")
            prec, h.rows, h.cols, nf = body[0], (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if m != 0xC0:
                raise Refused(NOTIMPL, "frame type SOF%d" % (m - 0xC0))
            if prec != 8:
                raise Refused(NOTIMPL, "%d-bit samples" % prec)
            if len(body) != 6 + 3 * nf:
                raise Refused(BADARG, "bad SOF")
            if h.cols == 0:
                raise Refused(BADARG, "a size of 0")
            frame = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
        elif m == 0xCC:
            raise Refused(NOTIMPL, "arithmetic coding")
        elif m == 0xDC:
            raise Refused(NOTIMPL, "DNL")
        elif m == 0xDD:
            if len(body) != 2:
                raise Refused(BADARG, "bad DRI")
            h.ri = (body[0] << 8) | body[1]
        elif m == 0xE0:
            if len(body) >= 14 and body[:5] == b"JFIF\x00":
                jfif = True
        elif m == 0xE1:
            o = _orientation(body)
            if o != 1:
                orient = o
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                adobe = True
        elif m == 0xDA:
            break
    if frame is None:
        raise Refused(BADARG, "SOS before SOF")
    if h.rows == 0:
        raise Refused(BADARG, "a size of 0")
    nf = len(frame)
    if nf not in (1, 3):
        raise Refused(NOTIMPL, "%d components" % nf)
    ns = body[0] if body else 0
    if len(body) != 4 + 2 * ns or ns < 1 or ns > 4:
        raise Refused(BADARG, "bad SOS")
    if ns != nf:
        raise Refused(NOTIMPL, "more than one scan")
    if adobe:
        raise Refused(NOTIMPL, "Adobe APP14")
    if nf == 3 and not jfif and [f[0] for f in frame] == [82, 71, 66]:
        raise Refused(NOTIMPL, "component ids R G B")
    if orient != 1:
        raise Refused(NOTIMPL, "EXIF orientation %d" % orient)
    if nf == 1:
        hs = vs = 1   # a single-component scan is not interleaved: its MCU is one block whatever SOF says (T.81 A.2.2)
        if not (1 <= frame[0][1] <= 4 and 1 <= frame[0][2] <= 4):
            raise Refused(NOTIMPL, "sampling factors")
    else:
        hs, vs = frame[0][1], frame[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or frame[1][1:3] != (1, 1) or frame[2][1:3] != (1, 1):
            raise Refused(NOTIMPL, "sampling factors")
    if (body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns]) != (0, 63, 0):
        raise Refused(NOTIMPL, "a spectral selection that is not a baseline scan's")
    h.ncomp, h.hs, h.vs = nf, hs, vs
    h.quant, h.dc, h.ac = [], [], []
    for i in range(ns):
        cs, t = body[1 + 2 * i], body[2 + 2 * i]
        if cs != frame[i][0]:
            raise Refused(NOTIMPL, "scan components out of frame order")
        if frame[i][3] not in qt or (0, t >> 4) not in dht or (1, t & 15) not in dht:
            raise Refused(BADARG, "a table that SOS names but nobody defined")
        h.quant.append(qt[frame[i][3]])
        h.dc.append(dht[(0, t >> 4)])
        h.ac.append(dht[(1, t & 15)])
    h.data = p
    if (len(s) - p) * 8 >= 1 << 32:
        raise Refused(ASSERT, "entropy data of 2^32 bits or more")


def geometry(h):
    """(mw, mh, blocks per MCU, MCUs, intervals)"""
    mw, mh = -(-h.cols // (8 * h.hs)), -(-h.rows // (8 * h.vs))
    bpm = h.hs * h.vs + (2 if h.ncomp == 3 else 0)
    nm = mw * mh
    return mw, mh, bpm, nm, (-(-nm // h.ri) if h.ri else 1)


def unstuff(s, start):
    """-> (bytes without stuffing and markers, [byte offset of every interval's start] + [length], rst_ok).
    A 0x00 behind 0xFF is dropped; 0xFF before anything but 0x00 is dropped; 0xFF RSTn starts an interval; 0xFF before any
    other byte (0xFF: a fill byte) ends the scan.  Fill bytes before 0xFF 0x00 (libjpeg and libjpeg-turbo read them
    differently) clear rst_ok: the stream is refused."""
    a = np.frombuffer(bytes(s[start:]) + b"\x00", np.uint8)
    n = len(a) - 1
    ff = a[:n] == 0xFF
    nxt = a[1:]
    prev_ff = np.concatenate([[False], ff[:-1]])
    end_at = np.nonzero(ff & (nxt != 0) & (nxt != 0xFF) & ~((nxt >= 0xD0) & (nxt <= 0xD7)))[0]
    end = int(end_at[0]) if len(end_at) else n
    if not len(end_at) and n and ff[n - 1]:
        end = n - 1     # a lone 0xFF at the end of the buffer is no data
    keep = ~(ff & (nxt != 0)) & ~prev_ff
    keep[end:] = False
    rst = ff & (nxt >= 0xD0) & (nxt <= 0xD7)
    rst[end:] = False
    pos = np.cumsum(keep) - keep           # exclusive
    r = np.nonzero(rst)[0]
    ok = all(int(a[i + 1]) == 0xD0 + (k & 7) for k, i in enumerate(r))
    ok = ok and not (ff & prev_ff & (nxt == 0))[:end].any()
    out = a[:n][keep].tobytes()
    return out, [0] + [int(pos[i]) for i in r] + [len(out)], ok


class _Lut:
    """every 16-bit window -> (symbol, length) of the code it starts with"""

    def __init__(self, table):
        bits, vals = table
        self.sym = np.zeros(1 << 16, np.int64)
        self.len = np.zeros(1 << 16, np.int64)   # 0: no code
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                lo = code << (16 - ln)
                self.sym[lo:lo + (1 << (16 - ln))] = vals[k]
                self.len[lo:lo + (1 << (16 - ln))] = ln
                code += 1
                k += 1
            code <<= 1
        self.sym, self.len = self.sym.tolist(), self.len.tolist()

    def decode(self, bitstr, p):
        """(symbol, length, valid) of the code at bit p, bits behind the string read as 0; an invalid code is symbol 0 of
        16 bits (the kernels' rule)"""
        w = int(bitstr[p:p + 16].ljust(16, "0"), 2)
        ln = self.len[w]
        return (self.sym[w], ln, True) if ln else (0, 16, False)


def _extend(v, n):
    return v if n == 0 or v >= (1 << (n - 1)) else v - (1 << n) + 1


def _bits_of(data):
    return "".join(format(b, "08b") for b in data)


def _step(bits, luts, comp_of_slot, bpm, p, slot, zz):
    """One code at bit p in state (slot, zz): -> (new p, slot', zz', block_done, (kind, index, value), valid).
    kind 0: a DC difference; 1: an AC coefficient at zig-zag `index`; 2: nothing to store."""
    c = comp_of_slot[slot]
    if zz == 0:
        sym, ln, ok = luts[0][c].decode(bits, p)
        n = sym & 15
        v = int(bits[p + ln:p + ln + n].ljust(n, "0"), 2) if n else 0
        return p + ln + n, slot, 1, False, (0, 0, _extend(v, n)), ok
    sym, ln, ok = luts[1][c].decode(bits, p)
    r, n = sym >> 4, sym & 15
    if n == 0:
        if r == 15:
            zz2 = zz + 16
            done = zz2 > 63
            return p + ln, ((slot + 1) % bpm if done else slot), (0 if done else zz2), done, (2, 0, 0), ok
        return p + ln, (slot + 1) % bpm, 0, True, (2, 0, 0), ok
    k = zz + r
    v = int(bits[p + ln:p + ln + n].ljust(n, "0"), 2)
    done = k >= 63
    store = (1, k, _extend(v, n)) if k <= 63 else (2, 0, 0)
    return p + ln + n, ((slot + 1) % bpm if done else slot), (0 if done else k + 1), done, store, ok and k <= 63


def _tables(h):
    luts = ([_Lut(t) for t in h.dc], [_Lut(t) for t in h.ac])
    ny = h.hs * h.vs if h.ncomp == 3 else 1
    bpm = ny + (2 if h.ncomp == 3 else 0)
    comp = [0] * ny + ([1, 2] if h.ncomp == 3 else [])
    return luts, comp, bpm


def huff_decode(h, data, ivals):
    """The plain sequential decoder.  -> (coef int64 [blocks][64] zig-zag with DC values in [:, 0], code)"""
    luts, comp, bpm = _tables(h)
    _, _, _, nm, nint = geometry(h)
    coef = np.zeros((nm * bpm, 64), np.int64)
    if len(ivals) - 1 != nint:
        return coef, ASSERT
    code = OK
    for k in range(nint):
        bits = _bits_of(data[ivals[k]:ivals[k + 1]])
        b0 = k * h.ri * bpm
        nb = (min(h.ri, nm - k * h.ri) if h.ri else nm) * bpm
        pred = [0, 0, 0]
        p, slot, zz, b = 0, 0, 0, 0
        while b < nb:
            if p >= len(bits):
                code = ASSERT
                break
            p, slot, zz, done, (kind, idx, v), ok = _step(bits, luts, comp, bpm, p, slot, zz)
            if not ok or p > len(bits):
                code = ASSERT
                break
            if kind == 0:
                c = comp[slot]
                pred[c] += v
                coef[b0 + b, 0] = pred[c]
            elif kind == 1:
                coef[b0 + b, idx] = v
            b += done
        if code == OK and (len(bits) - p >= 8):
            code = ASSERT      # blocks left over
    return coef, code


def selfsync(h, data, ivals, sub_bits):
    """The scheme of the kernels.  Every interval is cut into subsequences of sub_bits bits.  state[i] = (p, slot, zz) is
    where the lane of subsequence i stands when it crosses its end: round 0 starts every lane at its own first bit in state
    (0, 0), except an interval's first, which is right from the start; each later round restarts lane i from state[i - 1]
    where that changed in the round before, until a round changes nothing.  Then the blocks finished and the DC differences
    summed per subsequence are scanned, and a last decode from the known states writes the coefficients; it reads no code
    behind the interval's last block (the padding, whatever its bits), and a byte or more left there is an error.
    -> (coef, code, rounds)"""
    luts, comp, bpm = _tables(h)
    _, _, _, nm, nint = geometry(h)
    coef = np.zeros((nm * bpm, 64), np.int64)
    if len(ivals) - 1 != nint:
        return coef, ASSERT, 0
    code = OK
    rounds_max = 0
    for k in range(nint):
        bits = _bits_of(data[ivals[k]:ivals[k + 1]])
        end = len(bits)
        nsub = max(1, -(-end // sub_bits))
        b0 = k * h.ri * bpm
        nb = (min(h.ri, nm - k * h.ri) if h.ri else nm) * bpm

        def run(i, p, slot, zz, write=None):
            """lane i from (p, slot, zz) to the end of its subsequence"""
            lim = min((i + 1) * sub_bits, end)
            nblk, dsum, bad = 0, [0, 0, 0], False
            while p < lim:
                if write is not None and write[0] + nblk >= nb:
                    break       # the interval's blocks are done: the padding behind them is not read as codes
                p2, slot2, zz2, done, (kind, idx, v), ok = _step(bits, luts, comp, bpm, p, slot, zz)
                if p2 > end:        # the code runs past the interval (the padding, or a cut stream): the lane stops
                    p = end     # there, and the count of blocks and the state at the end tell which it was
                    break
                bad |= not ok
                if kind == 0:
                    dsum[comp[slot]] += v
                if write is not None:
                    b, dcb = write
                    if b + nblk < nb:
                        if kind == 0:
                            coef[b0 + b + nblk, 0] = dcb[comp[slot]] + dsum[comp[slot]]
                        elif kind == 1:
                            coef[b0 + b + nblk, idx] = v
                p, slot, zz = p2, slot2, zz2
                nblk += done
            return (p, slot, zz), nblk, dsum, bad

        state = [None] * nsub
        info = [None] * nsub
        for i in range(nsub):
            state[i], nblk, dsum, _ = run(i, i * sub_bits, 0, 0)
            info[i] = (nblk, dsum)
        changed = [True] * nsub
        rounds = 1
        while True:
            now = [False] * nsub
            for i in range(1, nsub):
                if changed[i - 1]:
                    st, nblk, dsum, _ = run(i, *state[i - 1])
                    now[i] = st != state[i]
                    state[i], info[i] = st, (nblk, dsum)
            rounds += 1
            changed = now
            if not any(now):
                break
        rounds_max = max(rounds_max, rounds)
        b, dcb = 0, [0, 0, 0]
        for i in range(nsub):
            entry = (0, 0, 0) if i == 0 else state[i - 1]
            st, nblk, dsum, bad = run(i, *entry, write=(b, list(dcb)))
            assert i == nsub - 1 or b + info[i][0] >= nb or (st == state[i] and (nblk, dsum) == info[i])
            if bad:
                code = ASSERT
            b += info[i][0] if i < nsub - 1 else nblk     # the scan of the counts the rounds left
            dcb = [x + y for x, y in zip(dcb, info[i][1])]
        if b != nb or st[1:] != (0, 0) or end - st[0] >= 8:
            code = ASSERT
    return coef, code, rounds_max


_C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069,
          c2053=16819, c2562=20995, c3072=25172)


def _idct_pass(d, shift):
    """One pass of jidctint.c over the last axis of d (.., 8)."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * _C["c0541"]
    t2 = z1 - z3 * _C["c1847"]
    t3 = z1 + z2 * _C["c0765"]
    t0, t1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C["c1175"]
    t0, t1, t2, t3 = t0 * _C["c0298"], t1 * _C["c2053"], t2 * _C["c3072"], t3 * _C["c1501"]
    z1, z2 = -z1 * _C["c0899"], -z2 * _C["c2562"]
    z3, z4 = -z3 * _C["c1961"] + z5, -z4 * _C["c0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct(coef, quant):
    """coef [n][64] zig-zag, quant [64] zig-zag -> samples uint8 [n][8][8]"""
    nat = np.zeros(coef.shape, np.int64)
    nat[:, ZIGZAG] = coef * quant[None, :]
    d = nat.reshape(-1, 8, 8)
    d = _idct_pass(d.swapaxes(-1, -2), 13 - 2).swapaxes(-1, -2)   # columns
    d = _idct_pass(d, 13 + 2 + 3)                                 # rows
    return np.clip(d + 128, 0, 255).astype(np.uint8)


def planes(h, coef):
    """The component planes, each a whole number of MCUs large."""
    mw, mh, bpm, nm, _ = geometry(h)
    ny = h.hs * h.vs if h.ncomp == 3 else 1
    c = coef.reshape(nm, bpm, 64)
    out = []
    y = idct(c[:, :ny].reshape(-1, 64), h.quant[0]).reshape(mh, mw, h.vs if h.ncomp == 3 else 1, h.hs if h.ncomp == 3 else 1, 8, 8)
    out.append(y.transpose(0, 2, 4, 1, 3, 5).reshape(mh * y.shape[2] * 8, mw * y.shape[3] * 8))
    for k in range(1, h.ncomp):
        s = idct(c[:, ny + k - 1], h.quant[k]).reshape(mh, mw, 8, 8)
        out.append(s.transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8))
    return out


def _h2v1(row_block, w):
    """h2v1_fancy_upsample of rows [r][w] -> [r][2 w]; plain doubling when w <= 2 (jinit_upsampler's rule)"""
    a = row_block[:, :w].astype(np.int64)
    if w <= 2:
        return np.repeat(a, 2, 1)
    left = np.concatenate([a[:, :1], a[:, :-1]], 1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    out = np.empty((a.shape[0], 2 * w), np.int64)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0], out[:, -1] = a[:, 0], a[:, -1]
    return out


def _h2v2(plane, w, hgt):
    """h2v2_fancy_upsample of the real [hgt][w] samples -> [2 hgt][2 w]; plain doubling when w <= 2"""
    a = plane[:hgt, :w].astype(np.int64)
    if w <= 2:
        return np.repeat(np.repeat(a, 2, 0), 2, 1)
    up = np.concatenate([a[:1], a[:-1]], 0)
    down = np.concatenate([a[1:], a[-1:]], 0)
    out = np.empty((2 * hgt, 2 * w), np.int64)
    for v, far in ((0, up), (1, down)):
        s = 3 * a + far
        last = np.concatenate([s[:, :1], s[:, :-1]], 1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even = (3 * s + last + 8) >> 4
        odd = (3 * s + nxt + 7) >> 4
        even[:, 0] = (4 * s[:, 0] + 8) >> 4
        odd[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def upsample(h, plane):
    cw = -(-h.cols // h.hs)
    ch = -(-h.rows // h.vs)
    if h.hs == 1:
        return plane[:h.rows, :h.cols].astype(np.int64)
    if h.vs == 1:
        return _h2v1(plane[:h.rows], cw)[:, :h.cols]
    return _h2v2(plane, cw, ch)[:h.rows, :h.cols]


def ycc_to_bgr(y, cb, cr):
    y, cb, cr = (np.asarray(v, np.int64) for v in (y, cb, cr))
    r = y + ((91881 * (cr - 128) + 32768) >> 16)
    g = y + ((-22554 * (cb - 128) + 32768 - 46802 * (cr - 128)) >> 16)
    b = y + ((116130 * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def render(h, coef, channels):
    p = planes(h, coef)
    y = p[0][:h.rows, :h.cols]
    if channels == 1:
        return y.copy()
    if h.ncomp == 1:
        return np.repeat(y[..., None], 3, 2)
    return ycc_to_bgr(y, upsample(h, p[1]), upsample(h, p[2]))


def decode(stream, channels, sub_bits=None):
    """-> (code, image or None).  sub_bits: decode with the self-synchronising scheme at that subsequence length."""
    code, h = parse(stream)
    if code:
        return code, None
    data, ivals, rst_ok = unstuff(stream, h.data)
    if sub_bits:
        coef, code, _ = selfsync(h, data, ivals, sub_bits)
    else:
        coef, code = huff_decode(h, data, ivals)
    if code or not rst_ok:
        return ASSERT, None
    return OK, render(h, coef, channels)
