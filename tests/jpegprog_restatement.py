"""A plain progressive (SOF2) JPEG decoder in Python / NumPy for the tests of maggie_amd/utils/jpegprog.py: the marker walk over several scans
and the four scan kinds (DC first, DC refinement, AC first, AC refinement with end-of-band runs), block after block, coefficient after
coefficient. It fills the coefficient buffer of the device -- (blocks, 64), natural order, interleaved MCU order with the padding blocks, DC
terms final -- and hands it to the arithmetic of tests/jpegdec_restatement.py (`planes_of`, `pixels`), imported and not edited. Nothing here
imports the package. tests/test_jpegprog_cpu.py holds `decode` against Pillow itself."""
import io

import numpy as np

import jpegdec_restatement as R

P = R.P
ZIGZAG = R.ZIGZAG
_ZZ = ZIGZAG.tolist()
_TABLES = {}


def _table(t):
    key = (bytes(t[0]), bytes(t[1]))
    if key not in _TABLES:
        _TABLES[key] = R.lookup16(*t)
    return _TABLES[key]


# ---- the marker walk -----------------------------------------------------------------------------------------------------------------------------
def parse(data):
    """dict(h, w, comps [(id, hs, vs, tq)], quant {id: (64,) natural}, scans [dict(comps [(component index, dc table, ac table)], Ss, Se, Ah, Al,
    ri, offset, length)]), tables as (counts, values) in force at the scan's SOS."""
    d = bytes(data)
    assert d[:2] == b'\xff\xd8'
    out = dict(quant={}, scans=[])
    dc, ac, ri, p = {}, {}, 0, 2
    while True:
        assert d[p] == 0xFF
        m = d[p + 1]
        if m == 0xD9:
            break
        size = (d[p + 2] << 8) | d[p + 3]
        seg = d[p + 4:p + 2 + size]
        if m == 0xC2:
            assert seg[0] == 8
            out.update(h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                       comps=[(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])])
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = np.frombuffer(seg[q + 1:q + 17], np.uint8)
                n = int(counts.sum())
                (ac if seg[q] >> 4 else dc)[seg[q] & 15] = (counts, np.frombuffer(seg[q + 17:q + 17 + n], np.uint8))
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
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in out['comps']]
            p += 2 + size
            q = p
            while True:
                q = d.index(b'\xff', q)
                if d[q + 1] == 0 or 0xD0 <= d[q + 1] <= 0xD7:
                    q += 2
                    continue
                break
            out['scans'].append(dict(comps=[(ids.index(seg[1 + 2 * k]), dc.get(seg[2 + 2 * k] >> 4), ac.get(seg[2 + 2 * k] & 15)) for k in range(ns)],
                                     Ss=seg[1 + 2 * ns], Se=seg[2 + 2 * ns], Ah=seg[3 + 2 * ns] >> 4, Al=seg[3 + 2 * ns] & 15, ri=ri, offset=p,
                                     length=q - p))
            p = q
            continue
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
        p += 2 + size
    return out


def script(data):
    """[(component indices, Ss, Se, Ah, Al)] in file order."""
    return [(tuple(c[0] for c in s['comps']), s['Ss'], s['Se'], s['Ah'], s['Al']) for s in parse(data)['scans']]


def header_twin(data):
    """The headers of a progressive file as a baseline file without data (SOI, DQT, SOF0, SOS, EOI): what `jpegdec_restatement.parse` reads the
    size, the sampling and the quantisation tables from when its `planes_of` / `pixels` finish our coefficients."""
    d = bytes(data)
    out, p = bytearray(b'\xff\xd8'), 2
    while d[p + 1] != 0xDA:
        size = (d[p + 2] << 8) | d[p + 3]
        if d[p + 1] == 0xDB:
            out += d[p:p + 2 + size]
        elif d[p + 1] == 0xC2:
            out += b'\xff\xc0' + d[p + 2:p + 2 + size]
            ids = [d[p + 10 + 3 * k] for k in range(d[p + 9])]
        p += 2 + size
    out += b'\xff\xda' + (6 + 2 * len(ids)).to_bytes(2, 'big') + bytes([len(ids)]) + b''.join(bytes([i, 0]) for i in ids) + b'\x00\x3f\x00'
    return bytes(out + b'\xff\xd9')


# ---- the bit stream ------------------------------------------------------------------------------------------------------------------------------
class Reader:
    """A scan's segment, cut at its restart markers; inside a part the stuffed 0x00 behind a data 0xFF is dropped. Reading past a part's last bit,
    a restart that is not where the bits end or carries the wrong number, and whole bytes left at the end raise ValueError."""

    def __init__(self, seg):
        self.parts, cur, i, n = [], bytearray(), 0, len(seg)
        while i < n:
            b = seg[i]
            if b == 0xFF:
                nx = seg[i + 1] if i + 1 < n else 0xD9
                if nx == 0:
                    cur.append(b)
                    i += 2
                    continue
                if 0xD0 <= nx <= 0xD7:
                    self.parts.append((bytes(cur), nx & 7))
                    cur = bytearray()
                    i += 2
                    continue
                break
            cur.append(b)
            i += 1
        self.parts.append((bytes(cur), None))
        self.part = -1
        self._next()

    def _next(self):
        self.part += 1
        self.clean = self.parts[self.part][0] + bytes(8)
        self.nbits, self.pos = 8 * len(self.parts[self.part][0]), 0

    def take(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.nbits:
            raise ValueError('corrupt stream: the segment ends inside a scan')
        i, o = self.pos >> 3, self.pos & 7
        self.pos += n
        return (int.from_bytes(self.clean[i:i + 5], 'big') >> (40 - o - n)) & ((1 << n) - 1)

    def symbol(self, table):
        i, o = self.pos >> 3, self.pos & 7
        e = table[(int.from_bytes(self.clean[i:i + 3], 'big') >> (8 - o)) & 0xFFFF]
        if e == 0 or self.pos + (e >> 8) > self.nbits:
            raise ValueError('corrupt stream: an unassigned Huffman code, or the segment ends inside one')
        self.pos += e >> 8
        return e & 255

    def restart(self, number):
        if self.nbits - self.pos >= 8 or self.parts[self.part][1] != number:
            raise ValueError('corrupt stream: a restart marker out of place')
        self._next()

    def finish(self):
        if self.nbits - self.pos >= 8 or self.part != len(self.parts) - 1:
            raise ValueError('corrupt stream: bytes left behind the last block of a scan')


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
def geometry(hdr):
    """(blocks per MCU, luma blocks per MCU side, MCU columns, MCU rows, first slot of each component in the MCU)."""
    comps = hdr['comps']
    if len(comps) == 1:
        hs = 1
    else:
        hs = comps[0][1]
        assert hs in (1, 2) and comps[0][2] == hs and all(c[1] == c[2] == 1 for c in comps[1:])
    side = 8 * hs
    first = [0] if len(comps) == 1 else [0, hs * hs, hs * hs + 1]
    return (1 if len(comps) == 1 else hs * hs + 2), hs, (hdr['w'] + side - 1) // side, (hdr['h'] + side - 1) // side, first


def block_order(hdr, scan):
    """The buffer indices of the blocks a scan visits, in its order, as a list of units (a unit is what the restart interval counts): an
    interleaved scan walks the MCUs, padding blocks included; a scan of one component walks the component's real blocks in raster order."""
    bpm, hs, mx, my, first = geometry(hdr)
    comps = [c[0] for c in scan['comps']]
    if len(comps) > 1:
        per = [(k, first[c] + j) for k, c in enumerate(comps) for j in range(hs * hs if c == 0 else 1)]
        return [[(k, m * bpm + sl) for k, sl in per] for m in range(mx * my)]
    c = comps[0]
    n = hs if c == 0 else 1                                    # the component's blocks per MCU side
    div = 8 * hs // n                                          # image pixels per block side of this component
    bw, bh = -(-hdr['w'] // div), -(-hdr['h'] // div)
    return [[(0, ((by // n) * mx + bx // n) * bpm + first[c] + (by % n) * n + bx % n)] for by in range(bh) for bx in range(bw)]


# ---- the four scan kinds -------------------------------------------------------------------------------------------------------------------------
def decode_scan(coef, hdr, scan, seg, stats=None):
    """One scan into `coef` (blocks, 64) int64, natural order."""
    rd = Reader(seg)
    Ss, Se, Ah, Al, ri = scan['Ss'], scan['Se'], scan['Ah'], scan['Al'], scan['ri']
    units = block_order(hdr, scan)
    preds, eobrun = [0] * len(scan['comps']), 0
    p1, m1 = 1 << Al, -(1 << Al)
    if Ss == 0:
        assert Se == 0
        tabs = [_table(c[1]) if Ah == 0 else None for c in scan['comps']]
    else:
        assert len(scan['comps']) == 1 and 1 <= Ss <= Se <= 63
        tab = _table(scan['comps'][0][2])
        band = [_ZZ[k] for k in range(Ss, Se + 1)]
        busy = (coef[:, band] != 0).any(1) if Ah else None      # blocks that hold a non-zero coefficient of the band: only those take bits in a run
    for u, unit in enumerate(units):
        if ri and u and u % ri == 0:
            rd.restart((u // ri - 1) & 7)
            preds, eobrun = [0] * len(preds), 0
        if Ss == 0:
            for k, blk in unit:
                if Ah == 0:
                    s = rd.symbol(tabs[k])
                    if s > 11:
                        raise ValueError('corrupt stream: a DC category above 11')
                    preds[k] += extend(rd.take(s), s)
                    coef[blk, 0] = preds[k] << Al
                elif rd.take(1):
                    coef[blk, 0] |= p1
            continue
        blk = unit[0][1]
        if Ah == 0:                                            # AC first
            if eobrun > 0:
                eobrun -= 1
                continue
            k = Ss
            while k <= Se:
                rs = rd.symbol(tab)
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    if k > Se:
                        raise ValueError('corrupt stream: a zig-zag index past the band')
                    coef[blk, _ZZ[k]] = extend(rd.take(s), s) << Al
                elif r == 15:
                    k += 15
                else:
                    eobrun = (1 << r) + (rd.take(r) if r else 0) - 1
                    if stats is not None:
                        stats.setdefault('eob_classes', set()).add(r)
                    break
                k += 1
            continue
        # AC refinement
        if eobrun > 0 and not busy[blk]:                       # a block of a run without history reads no bit
            eobrun -= 1
            if stats is not None:
                stats['silent'] = stats.get('silent', 0) + 1
            continue
        row = [int(coef[blk, z]) for z in _ZZ]                 # zig-zag order
        k = Ss
        if eobrun == 0:
            while k <= Se:
                rs = rd.symbol(tab)
                r, s = rs >> 4, rs & 15
                value = 0
                if s:
                    if s != 1:
                        raise ValueError('corrupt stream: a refinement symbol of size %d' % s)
                    value = p1 if rd.take(1) else m1
                elif r < 15:
                    eobrun = (1 << r) + (rd.take(r) if r else 0)
                    break
                while k <= Se:
                    if row[k] != 0:
                        if rd.take(1) and (row[k] & p1) == 0:
                            row[k] += p1 if row[k] >= 0 else m1
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if value:
                    if k > Se:
                        raise ValueError('corrupt stream: a new value past the end of the band')
                    row[k] = value
                k += 1
        if eobrun > 0:
            while k <= Se:
                if row[k] != 0 and rd.take(1) and (row[k] & p1) == 0:
                    row[k] += p1 if row[k] >= 0 else m1
                k += 1
            eobrun -= 1
        coef[blk, ZIGZAG] = row
    rd.finish()


def coefficients(data, stats=None):
    """The sequential decoder: (blocks, 64) int64 quantised coefficients in the device's layout; raises ValueError on a corrupt stream."""
    hdr = parse(data)
    bpm, _, mx, my, _ = geometry(hdr)
    coef = np.zeros((mx * my * bpm, 64), np.int64)
    d = bytes(data)
    for scan in hdr['scans']:
        decode_scan(coef, hdr, scan, d[scan['offset']:scan['offset'] + scan['length']], stats)
    return coef


def touched(data):
    """A mask over the buffer's blocks: True where a pixel of the image lies in the block (the others are padding)."""
    hdr = parse(data)
    bpm, hs, mx, my, first = geometry(hdr)
    m = np.zeros((my, mx, bpm), bool)
    for c in range(len(hdr['comps'])):
        n = hs if c == 0 else 1
        div = 8 * hs // n
        bw, bh = -(-hdr['w'] // div), -(-hdr['h'] // div)
        for j in range(n * n):
            by, bx = np.mgrid[0:my, 0:mx]
            m[:, :, first[c] + j] = (by * n + j // n < bh) & (bx * n + j % n < bw)
    return m.reshape(-1)


def planes_of(data, coef):
    return R.planes_of(header_twin(data), coef)


def pixels(data, coef):
    return R.pixels(header_twin(data), coef)


def decode(data):
    return pixels(data, coefficients(data))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
QUALITIES = (1, 50, 90, 100)


def _cases():
    c = {}
    for h, w in R.SIZES:
        for kind in R.KINDS:
            for mode in R.MODES:
                for q in QUALITIES:
                    c['%dx%d_%s_%s_q%d' % (h, w, kind, mode, q)] = (h, w, kind, mode, dict(quality=q, progressive=True))
    return c


def _restart_cases():
    c = {}
    for mode in R.MODES:
        c['37x53_uniform_%s_q90_blocks1' % mode] = (37, 53, 'uniform', mode, dict(quality=90, progressive=True, restart_marker_blocks=1))
        c['64x48_smooth_%s_q50_rows1' % mode] = (64, 48, 'smooth', mode, dict(quality=50, progressive=True, restart_marker_rows=1))
        c['33x65_binary_%s_q100_blocks1' % mode] = (33, 65, 'binary', mode, dict(quality=100, progressive=True, restart_marker_blocks=1))
    return c


CASES = _cases()
RESTART = _restart_cases()
LARGE = R.LARGE[:4] + (dict(R.LARGE[4], progressive=True),)    # 256 x 256, uniform, quality 100: the byte window refills many times
RUNS_SIDE = 1472                                               # 184 x 184 blocks per component: runs past libjpeg's flush at 32 767


def stream(h, w, kind, mode, save):
    """The bytes Pillow writes for a case. A progressive file leaves the encoder in one piece, so Pillow's output block has to hold all of it."""
    from PIL import ImageFile
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 4 * h * w + 65536)
    try:
        return R.stream(h, w, kind, mode, save)
    finally:
        ImageFile.MAXBLOCK = keep


def twin(h, w, kind, mode, save):
    """The baseline twin: the same array, quality and subsampling saved without `progressive`."""
    return R.stream(h, w, kind, mode, {k: v for k, v in save.items() if k != 'progressive'})


def runs_stream():
    """1472 x 1472, 4:4:4, value 77 everywhere but an 8 x 8 noise patch at the top left: 33 856 blocks per component, all but the first without
    AC terms. The encoder flushes an end-of-band run at 32 767, so the AC-first scans hold the largest run class (14) and the refinement scans
    long runs that read no bit."""
    from PIL import Image
    x = np.full((RUNS_SIDE, RUNS_SIDE, 3), 77, np.uint8)
    x[:8, :8] = np.random.RandomState(7).randint(0, 256, (8, 8, 3))
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=90, subsampling=0, progressive=True)
    return buf.getvalue()


def named(name):
    """The stream of a case of CASES or RESTART, of 'large' or of 'runs'."""
    if name == 'runs':
        return runs_stream()
    return stream(*(LARGE if name == 'large' else CASES[name] if name in CASES else RESTART[name]))


pillow = R.pillow
