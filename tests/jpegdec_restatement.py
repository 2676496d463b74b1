"""A plain baseline JPEG decoder in Python / NumPy for the tests of maggie_amd/utils/jpegdec.py: the marker walk, the Huffman decoding, the DC
prediction and the restart handling. The inverse transform's passes, the upsampling and the colour rules are imported from
tests/photometric_restatement.py, which holds them against Pillow. Nothing here imports the package.

`decode(data)` is the sequential decoder; `sync_rounds(data, sub_bytes)` states the device's subsequence algorithm on the host, one Python
"lane" per subsequence. Both walk the stream with the same `run_sub`; what makes them two statements is where a lane
starts and what it knows when it does. tests/test_jpegdec_cpu.py holds `decode` against Pillow itself."""
import io

import numpy as np

import photometric_restatement as P

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SUB_BYTES = (8, 29, 64)                       # the minimum (which the measured default equals), one value that divides nothing evenly, a longer one
ST_INDEX, ST_CODE, ST_PAST_END, ST_COUNT, ST_RESTART = 1, 2, 4, 8, 16


# ---- the marker walk -----------------------------------------------------------------------------------------------------------------------------
def parse(data):
    """dict(h, w, comps [(id, hs, vs, tq)], quant {id: (64,) natural}, dc / ac {id: (counts, values)}, scan [(id, td, ta)], ri, offset, length)."""
    d = bytes(data)
    assert d[:2] == b'\xff\xd8'
    out = dict(quant={}, dc={}, ac={}, ri=0)
    p = 2
    while True:
        assert d[p] == 0xFF
        m, size = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        seg = d[p + 4:p + 2 + size]
        if m == 0xC0:
            assert seg[0] == 8
            out.update(h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                       comps=[(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])])
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = np.frombuffer(seg[q + 1:q + 17], np.uint8)
                n = int(counts.sum())
                out['ac' if seg[q] >> 4 else 'dc'][seg[q] & 15] = (counts, np.frombuffer(seg[q + 17:q + 17 + n], np.uint8))
                q += 17 + n
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                out['quant'][seg[q] & 15] = t
                q += 65
        elif m == 0xDD:
            out['ri'] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            out['scan'] = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(seg[0])]
            p += 2 + size
            break
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
        p += 2 + size
    q = p
    while True:
        q = d.index(b'\xff', q)
        if d[q + 1] == 0 or 0xD0 <= d[q + 1] <= 0xD7:
            q += 2
            continue
        break
    assert d[q + 1] == 0xD9 and [c[0] for c in out['comps']] == [s[0] for s in out['scan']]
    out.update(offset=p, length=q - p)
    return out


def layout_of(hdr):
    """(blocks per MCU, luma blocks per MCU side, the slots' (component, dc id, ac id))."""
    s = hdr['scan']
    if len(s) == 1:
        return 1, 1, [(0, s[0][1], s[0][2])]
    hs = hdr['comps'][0][1]
    assert hs in (1, 2) and hdr['comps'][0][2] == hs and all(c[1] == c[2] == 1 for c in hdr['comps'][1:])
    slots = [(0, s[0][1], s[0][2])] * (hs * hs) + [(1, s[1][1], s[1][2]), (2, s[2][1], s[2][2])]
    return len(slots), hs, slots


def geometry(hdr):
    bpm, hs, _ = layout_of(hdr)
    side = 8 * hs
    return bpm, hs, (hdr['w'] + side - 1) // side, (hdr['h'] + side - 1) // side


# ---- the bit stream ------------------------------------------------------------------------------------------------------------------------------
def lookup16(counts, values):
    """A 65536-entry list: the 16 leading bits -> len << 8 | symbol, 0 for an unassigned code (T.81 Annex C: canonical codes by length)."""
    t = np.zeros(65536, np.int64)
    code = k = 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            t[code << (16 - l):(code + 1) << (16 - l)] = (l << 8) | int(values[k])
            code += 1
            k += 1
        code <<= 1
    return t.tolist()


class Stream:
    """An entropy-coded segment: byte i is stuffing iff it is 0x00 and byte i - 1 is 0xFF; 0xFF 0xD0..0xD7 is a restart marker. Positions are RAW
    bit positions. `clean` holds the data bytes, `di[i]` the number of data bytes in front of raw byte i, `raw[k]` the raw index of data
    byte k, `end[k]` the data index at which the run of data byte k stops (a marker or the segment's end)."""

    def __init__(self, seg):
        self.seg, self.len = seg, len(seg)
        clean, raw, di, self.marker = bytearray(), [], [0] * (len(seg) + 1), set()
        runs, i, n = [], 0, len(seg)
        start = 0
        while i < n:
            di[i] = len(clean)
            b = seg[i]
            if b == 0xFF:
                nx = seg[i + 1] if i + 1 < n else 0xD9
                if nx == 0:
                    clean.append(b); raw.append(i); di[i + 1] = len(clean); i += 2
                    continue
                runs.append((start, len(clean)))
                start = len(clean)
                if 0xD0 <= nx <= 0xD7:
                    self.marker.add(i); di[i + 1] = len(clean); i += 2
                    continue
                self.len = i                                               # anything else ends the data
                break
            clean.append(b); raw.append(i); i += 1
        runs.append((start, len(clean)))
        di[min(i, n)] = len(clean)
        self.clean, self.raw, self.di = bytes(clean), raw, di
        self.end = [0] * len(clean)
        for a, b in runs:
            self.end[a:b] = [b] * (b - a)

    def start_of(self, q):
        """The first raw position at or after byte q from which a lane may start: not a stuffed byte, not inside a restart marker."""
        if q >= self.len:
            return 8 * self.len
        b, p = self.seg[q], self.seg[q - 1] if q > 0 else 0
        if p == 0xFF and (b == 0 or 0xD0 <= b <= 0xD7):
            return 8 * (q + 1)
        if q in self.marker:
            return min(8 * (q + 2), 8 * self.len)
        return 8 * q


def run_sub(S, tabs, slots, state, endbit, coef=None, blk0=0, ri_blocks=0):
    """Decode from `state` = (pos, slot, zz) to the first symbol that starts at or after `endbit`: the exit state, the blocks completed, the
    status bits. With `coef` (blocks, 64) the coefficients are written in natural order, the DC term as its difference."""
    pos, slot, zz = state
    nblk = status = 0
    bpm, total, nbf = len(slots), 8 * S.len, 0 if coef is None else len(coef)
    while pos < endbit:
        i, o = pos >> 3, pos & 7
        at_marker = i in S.marker
        k = S.di[i]
        stop = S.end[k] if (i < S.len and not at_marker and k < len(S.clean)) else k
        have = min(stop - k, 5)
        bits = (int.from_bytes(S.clean[k:k + have], 'big') << (8 * (5 - have))) | ((1 << (8 * (5 - have))) - 1)       # ones behind the data
        bits = (bits >> (8 - o)) & 0xFFFFFFFF
        e = tabs[slots[slot][1] if zz == 0 else 2 + slots[slot][2]][bits >> 16]
        ln, sym, bad = e >> 8, e & 255, e == 0
        if bad:
            ln = 16
        s, run = (sym, 0) if zz == 0 else (sym & 15, sym >> 4)
        if s > 11:
            s, bad = 11, True
        n = ln + s
        if o + n > 8 * have:                                                # the symbol does not fit in front of where the data stops
            stop_raw = i if at_marker or have == 0 else S.raw[stop - 1] + (2 if S.clean[stop - 1] == 0xFF else 1)
            if stop_raw in S.marker:
                done = blk0 + nblk
                if coef is not None and (slot or zz or ri_blocks <= 0 or done % max(ri_blocks, 1) or
                                         ((done // max(ri_blocks, 1) - 1) & 7) != S.seg[stop_raw + 1] & 7):
                    status |= ST_RESTART
                pos, slot, zz = min(8 * (stop_raw + 2), total), 0, 0
                continue
            if coef is not None and blk0 + nblk < nbf:
                status |= ST_PAST_END
            pos = total
            break
        if bad:
            status |= ST_CODE
        v = (bits >> (32 - ln - s)) & ((1 << s) - 1) if s else 0
        if s and v < (1 << (s - 1)):
            v = v - (1 << s) + 1
        blk = blk0 + nblk
        if zz == 0:
            if coef is not None:
                if blk < nbf:
                    coef[blk, 0] = v
                else:
                    status |= ST_COUNT
            zz = 1
        elif s == 0:
            zz = zz + 16 if run == 15 else 64
            if zz > 64:
                status |= ST_INDEX
        else:
            zz += run
            if zz > 63:
                status |= ST_INDEX
            elif coef is not None:
                if blk < nbf:
                    coef[blk, ZIGZAG[zz]] = v
                else:
                    status |= ST_COUNT
            zz += 1
        if zz >= 64:
            zz, nblk, slot = 0, nblk + 1, (slot + 1) % bpm
        kk = (o + n) >> 3                                                   # whole data bytes consumed, with the stuffed bytes behind them
        if kk:
            last = S.raw[k + kk - 1]
            nxt = S.raw[k + kk] if k + kk < stop else last + (2 if S.clean[k + kk - 1] == 0xFF else 1)
            pos = 8 * nxt + ((o + n) & 7)
        else:
            pos += n
    return (pos, slot, zz), nblk, status


def _setup(data):
    hdr = parse(data)
    bpm, hs, mx, my = geometry(hdr)
    _, _, slots = layout_of(hdr)
    tabs = [lookup16(*hdr['dc'][k]) if k in hdr['dc'] else [0] * 65536 for k in (0, 1)] + \
           [lookup16(*hdr['ac'][k]) if k in hdr['ac'] else [0] * 65536 for k in (0, 1)]
    S = Stream(bytes(data)[hdr['offset']:hdr['offset'] + hdr['length']])
    return hdr, S, tabs, slots, bpm, mx * my


def dc_sum(coef, slots, mcus, ri):
    """Differences -> DC terms: the inclusive sum per component within each restart interval."""
    bpm = len(slots)
    c = coef.reshape(mcus, bpm, 64)
    for comp in sorted({s[0] for s in slots}):
        sl = [k for k, s in enumerate(slots) if s[0] == comp]
        step = ri if ri > 0 else mcus
        for a in range(0, mcus, step):
            part = c[a:a + step, sl, 0]
            c[a:a + step, sl, 0] = np.cumsum(part.reshape(-1)).reshape(part.shape)
    return coef


def coefficients(data):
    """The sequential decoder: (blocks, 64) int64 quantised coefficients in scan order, natural order inside a block; raises on a status bit."""
    hdr, S, tabs, slots, bpm, mcus = _setup(data)
    coef = np.zeros((mcus * bpm, 64), np.int64)
    _, nblk, status = run_sub(S, tabs, slots, (0, 0, 0), 8 * S.len, coef, 0, hdr['ri'] * bpm)
    if nblk != mcus * bpm:
        status |= ST_COUNT
    if status:
        raise ValueError('corrupt stream: status %d' % status)
    return dc_sum(coef, slots, mcus, hdr['ri'])


def sync_rounds(data, sub_bytes):
    """The subsequence algorithm on the host. Lane j owns the symbols that start in raw bytes [j * sub_bytes, (j + 1) * sub_bytes). First pass:
    every lane decodes from the first bit of its subsequence assuming slot 0, index 0 (lane 0 IS right). A round: every lane whose entry -- the
    exit state of the lane before it -- is new to it decodes again from that entry. The rounds end when one changes no exit state; each makes
    at least one more subsequence right, so there are at most as many as subsequences. Then the exclusive sum of the block counts, the
    writing pass and the DC sum. Returns (coefficients, rounds)."""
    hdr, S, tabs, slots, bpm, mcus = _setup(data)
    nsub = max(1, -(-S.len // sub_bytes))
    ends = [8 * min((j + 1) * sub_bytes, S.len) for j in range(nsub)]
    E, cnt, seen = [None] * nsub, [0] * nsub, [None] * nsub
    for j in range(nsub):
        st = (0, 0, 0) if j == 0 else (S.start_of(j * sub_bytes), 0, 0)
        E[j], cnt[j], _ = run_sub(S, tabs, slots, st, ends[j])
    rounds = 0
    while True:
        prev, changed = list(E), False
        for j in range(1, nsub):
            if prev[j - 1] != seen[j]:
                seen[j] = prev[j - 1]
                now, cnt[j], _ = run_sub(S, tabs, slots, seen[j], ends[j])
                changed |= now != E[j]
                E[j] = now
        if not changed:
            break
        rounds += 1
        assert rounds <= nsub
    coef = np.zeros((mcus * bpm, 64), np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])
    status = 0
    for j in range(nsub):
        _, n, st = run_sub(S, tabs, slots, (0, 0, 0) if j == 0 else E[j - 1], ends[j], coef, int(first[j]), hdr['ri'] * bpm)
        assert n == cnt[j]
        status |= st
    if first[-1] != mcus * bpm:
        status |= ST_COUNT
    if status:
        raise ValueError('corrupt stream: status %d' % status)
    return dc_sum(coef, slots, mcus, hdr['ri']), rounds


# ---- from coefficients to pixels -----------------------------------------------------------------------------------------------------------------
def range_limit(v):
    """libjpeg's table behind the inverse transform, indexed with the descaled value masked to 10 bits (the + 128 is part of the table): equal
    to clip(v + 128, 0, 255) for -512 <= v < 512, periodic beyond."""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def idct(coefs):
    """jpeg_idct_islow of dequantised int64 (..., 8, 8) blocks: P's passes, columns (descale 11) then rows (descale 18), then the range limit."""
    cols = np.swapaxes(P.idct_1d(np.swapaxes(coefs, -1, -2), P.CONST_BITS - P.PASS1_BITS), -1, -2)
    return range_limit(P.idct_1d(cols, P.CONST_BITS + P.PASS1_BITS + 3))


def planes_of(data, coef):
    """The decoded component planes as the coder holds them (whole MCUs): a list of int64 (H, W) arrays, one per component."""
    hdr = parse(data)
    bpm, hs, mx, my = geometry(hdr)
    _, _, slots = layout_of(hdr)
    c = np.asarray(coef, np.int64).reshape(my, mx, bpm, 8, 8)
    out = []
    for comp in range(len(hdr['comps'])):
        sl = [k for k, s in enumerate(slots) if s[0] == comp]
        px = idct(c[:, :, sl] * hdr['quant'][hdr['comps'][comp][3]].reshape(8, 8))
        n = hs if comp == 0 else 1
        out.append(px.reshape(my, mx, n, n, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * n * 8, mx * n * 8))
    return out


def pixels(data, coef):
    """Image.open(...).convert('RGB') from the coefficients: (h, w, 3) uint8."""
    hdr = parse(data)
    h, w = hdr['h'], hdr['w']
    pl = planes_of(data, coef)
    if len(pl) == 1:
        return np.repeat(pl[0][:h, :w, None], 3, 2).astype(np.uint8)
    if pl[1].shape != pl[0].shape:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        return P.ycc_to_rgb(pl[0][:h, :w], P.upsample(pl[1][:ch, :cw], h, w), P.upsample(pl[2][:ch, :cw], h, w))
    return P.ycc_to_rgb(pl[0][:h, :w], pl[1][:h, :w], pl[2][:h, :w])


def decode(data):
    return pixels(data, coefficients(data))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (9, 4), (16, 16), (17, 23), (33, 65), (37, 53), (64, 48)]
QUALITIES = (1, 50, 90, 100)
KINDS = ('uniform', 'smooth', 'flat', 'binary')
MODES = (2, 0, 'L')                            # Pillow's subsampling 2 (4:2:0), 0 (4:4:4), and mode L


def image(h, w, kind, seed, mode):
    r = np.random.RandomState(seed)
    if kind == 'uniform':
        x = r.randint(0, 256, (h, w, 3))
    elif kind == 'binary':
        x = r.randint(0, 2, (h, w, 3)) * 255
    elif kind == 'flat':
        x = np.full((h, w, 3), 128)
    elif kind == 'periodic':                  # one 8 x 8 block repeated: a periodic code stream
        x = np.tile(r.randint(0, 256, (8, 8, 3)), (h // 8, w // 8, 1))
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        x = np.clip(np.stack([40 + 3 * xx + yy, 200 - 2 * yy - xx, 90 + 2 * ((xx + yy) % 40)], -1) + r.randint(-6, 7, (h, w, 3)), 0, 255)
    x = x.astype(np.uint8)
    return x[..., 0] if mode == 'L' else x


def _cases():
    c = {}

    def add(h, w, kind, mode, **save):
        name = '%dx%d_%s_%s_%s' % (h, w, kind, mode, '_'.join('%s%s' % (k[:3], 'T' if v is True else (v if np.isscalar(v) else v[0][0]))
                                                                for k, v in sorted(save.items())))
        c[name] = (h, w, kind, mode, save)
    for i, (h, w) in enumerate(SIZES):
        for j, q in enumerate(QUALITIES):
            for mode in MODES:
                add(h, w, KINDS[(i + j) % 4], mode, quality=q)
    add(64, 256, 'periodic', 2, quality=100)      # one 8 x 8 block repeated: the lanes never synchronise by themselves
    for mode in MODES:
        add(37, 53, 'uniform', mode, quality=90, optimize=True)
        add(64, 48, 'smooth', mode, quality=50, optimize=True)
        add(16, 16, 'flat', mode, quality=90, optimize=True)
        add(37, 53, 'uniform', mode, quality=90, restart_marker_blocks=1)
        add(64, 48, 'uniform', mode, quality=100, restart_marker_blocks=3)
        add(16, 16, 'flat', mode, quality=50, restart_marker_blocks=3, optimize=True)
        add(64, 48, 'smooth', mode, quality=50, restart_marker_rows=1)
        add(33, 65, 'binary', mode, qtables=[[255] * 64] * 2)
        add(33, 65, 'binary', mode, qtables=[[1] * 64] * 2)
    add(64, 48, 'uniform', 0, quality=100)
    return c


CASES = _cases()
LARGE = (256, 256, 'uniform', 0, dict(quality=100))       # about 270 KB: the default sub_bytes spans several workgroups too


def stream(h, w, kind, mode, save):
    """The bytes Pillow writes for a case."""
    from PIL import Image
    x = image(h, w, kind, 100 * h + w, mode)
    buf = io.BytesIO()
    kw = dict(save)
    if mode != 'L':
        kw['subsampling'] = mode
    Image.fromarray(x).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
