"""The other chroma samplings -- 4:2:2, 4:4:0, 4:1:1: luma sampling (hs, vs) = (2, 1), (1, 2), (4, 1) over (1, 1) Cb and Cr -- in Python / NumPy
for the tests of maggie_amd/utils/jpegsamp.py. The Huffman decoding, the scan kinds, the inverse transform and the colour rule are those of
tests/jpegdec_restatement.py and tests/jpegprog_restatement.py, imported and not edited; what is stated here is the geometry of an MCU of
8 hs x 8 vs pixels, the three upsampling rules, and two small WRITERS, because Pillow writes 4:4:4, 4:2:2 and 4:2:0 only. Nothing here imports
the package. tests/test_jpegsamp_cpu.py holds `decode` against Pillow itself on every case."""
import types

import numpy as np

import jpegdec_restatement as R
import jpegprog_restatement as PR

P = R.P
ZIGZAG = R.ZIGZAG
SAMPLINGS = {'422': (2, 1), '440': (1, 2), '411': (4, 1)}


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
def progressive(data):
    """Whether the frame header is SOF2."""
    d, p = bytes(data), 2
    while d[p + 1] not in (0xC0, 0xC2):
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
    return d[p + 1] == 0xC2


def header(data):
    return PR.parse(data) if progressive(data) else R.parse(data)


def geometry(hdr):
    """(blocks per MCU, hs, vs, MCU columns, MCU rows): an MCU holds the hs * vs luma blocks row by row, then Cb, then Cr."""
    (_, hs, vs, _), cb, cr = hdr['comps']
    assert (hs, vs) in SAMPLINGS.values() and cb[1:3] == cr[1:3] == (1, 1)
    return hs * vs + 2, hs, vs, -(-hdr['w'] // (8 * hs)), -(-hdr['h'] // (8 * vs))


def block_order(hdr, scan):
    """`jpegprog_restatement.block_order` for (hs, vs): an interleaved scan walks the MCUs, padding blocks included; a luma scan walks the
    ceil(h / 8) x ceil(w / 8) real luma blocks in raster order -- block (by, bx) lives in MCU (by // vs, bx // hs), slot (by % vs) * hs + bx % hs;
    a chroma scan walks its mcuy x mcux blocks."""
    bpm, hs, vs, mx, my = geometry(hdr)
    comps = [c[0] for c in scan['comps']]
    first = [0, hs * vs, hs * vs + 1]
    if len(comps) > 1:
        per = [(k, first[c] + j) for k, c in enumerate(comps) for j in range(hs * vs if c == 0 else 1)]
        return [[(k, m * bpm + sl) for k, sl in per] for m in range(mx * my)]
    if comps[0]:
        return [[(0, m * bpm + first[comps[0]])] for m in range(mx * my)]
    bw, bh = -(-hdr['w'] // 8), -(-hdr['h'] // 8)
    return [[(0, ((by // vs) * mx + bx // hs) * bpm + (by % vs) * hs + bx % hs)] for by in range(bh) for bx in range(bw)]


# jpegprog_restatement.decode_scan, its code unchanged, walking the blocks in the order above
_decode_scan = types.FunctionType(PR.decode_scan.__code__, dict(vars(PR), block_order=block_order), 'decode_scan', PR.decode_scan.__defaults__)


# ---- coefficients --------------------------------------------------------------------------------------------------------------------------------
def coefficients(data):
    """(blocks, 64) int64 quantised coefficients in the device's layout (MCU order, natural order inside a block, DC terms final); raises
    ValueError on a corrupt stream."""
    hdr = header(data)
    bpm, hs, vs, mx, my = geometry(hdr)
    coef = np.zeros((mx * my * bpm, 64), np.int64)
    d = bytes(data)
    if 'scans' in hdr:
        for scan in hdr['scans']:
            _decode_scan(coef, hdr, scan, d[scan['offset']:scan['offset'] + scan['length']])
        return coef
    s = hdr['scan']
    slots = [(0, s[0][1], s[0][2])] * (hs * vs) + [(1, s[1][1], s[1][2]), (2, s[2][1], s[2][2])]
    tabs = [R.lookup16(*hdr[kind][k]) if k in hdr[kind] else [0] * 65536 for kind in ('dc', 'ac') for k in (0, 1)]
    S = R.Stream(d[hdr['offset']:hdr['offset'] + hdr['length']])
    _, nblk, status = R.run_sub(S, tabs, slots, (0, 0, 0), 8 * S.len, coef, 0, hdr['ri'] * bpm)
    if nblk != len(coef):
        status |= R.ST_COUNT
    if status:
        raise ValueError('corrupt stream: status %d' % status)
    return R.dc_sum(coef, slots, mx * my, hdr['ri'])


# ---- from coefficients to pixels -----------------------------------------------------------------------------------------------------------------
def planes_of(data, coef):
    """The decoded planes over whole MCUs: Y (mcuy * 8 vs, mcux * 8 hs), Cb and Cr (mcuy * 8, mcux * 8), int64."""
    hdr = header(data)
    bpm, hs, vs, mx, my = geometry(hdr)
    c = np.asarray(coef, np.int64).reshape(my, mx, bpm, 8, 8)
    q = [hdr['quant'][comp[3]].reshape(8, 8) for comp in hdr['comps']]
    y = R.idct(c[:, :, :hs * vs] * q[0]).reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
    return [y] + [R.idct(c[:, :, hs * vs + k] * q[1 + k]).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8) for k in range(2)]


def device_planes(flat, T, h, w, hs, vs):
    """The device's plane buffer (include/maggie_hip.h: Y of all frames, then Cb, then Cr; the luma row pitch a multiple of 16 bytes, the 4:4:0
    chroma pitch too) -> [Y (T, H, W), Cb, Cr (T, H / vs, W / hs)] over whole MCUs, the bytes between a row's blocks and its pitch dropped."""
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    yp, cp = -(-mx * 8 * hs // 16) * 16, -(-mx * 8 // 16) * 16 if vs == 2 else mx * 8
    flat = np.asarray(flat).reshape(-1)
    assert flat.size == T * my * 8 * (vs * yp + 2 * cp)
    ny, nc = T * my * 8 * vs * yp, T * my * 8 * cp
    return [flat[:ny].reshape(T, my * 8 * vs, yp)[:, :, :mx * 8 * hs]] + \
        [flat[ny + k * nc:ny + (k + 1) * nc].reshape(T, my * 8, cp)[:, :, :mx * 8] for k in range(2)]


def triangle(c):
    """libjpeg's fancy 2x along the last axis over the REAL samples: out[2j] = (3 c[j] + c[j-1] + 1) >> 2, out[2j+1] = (3 c[j] + c[j+1] + 2) >> 2,
    the neighbour clamped to the samples (which makes the first and the last output a copy)."""
    left, right = np.concatenate([c[..., :1], c[..., :-1]], -1), np.concatenate([c[..., 1:], c[..., -1:]], -1)
    out = np.empty(c.shape[:-1] + (2 * c.shape[-1],), np.int64)
    out[..., 0::2] = (3 * c + left + 1) >> 2
    out[..., 1::2] = (3 * c + right + 2) >> 2
    return out


def upsample(c, h, w, hs, vs):
    """The real chroma samples (ceil(h / vs), ceil(w / hs)) -> (h, w). 4:2:2: the triangle along the row, replication when there are at most two
    columns; 4:4:0: the triangle along the column at every size; 4:1:1: replication."""
    if (hs, vs) == (2, 1):
        return (triangle(c) if c.shape[1] > 2 else np.repeat(c, 2, 1))[:, :w]
    if (hs, vs) == (1, 2):
        return triangle(c.T).T[:h]
    return np.repeat(c, 4, 1)[:, :w]


def pixels(data, coef):
    """Image.open(...).convert('RGB') from the coefficients: (h, w, 3) uint8."""
    hdr = header(data)
    _, hs, vs, _, _ = geometry(hdr)
    h, w = hdr['h'], hdr['w']
    ch, cw = -(-h // vs), -(-w // hs)
    y, cb, cr = planes_of(data, coef)
    return P.ycc_to_rgb(y[:h, :w], upsample(cb[:ch, :cw], h, w, hs, vs), upsample(cr[:ch, :cw], h, w, hs, vs))


def decode(data):
    return pixels(data, coefficients(data))


# ---- the writers ---------------------------------------------------------------------------------------------------------------------------------
def _codes(counts, values):
    """symbol -> (code, length), T.81 Annex C."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            out[int(values[k])] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc, self.n = (self.acc << n) | (v & ((1 << n) - 1)), self.n + n
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out += b'\xff\x00' if b == 255 else bytes([b])     # byte stuffing
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)           # one-bit padding

    def value(self, tab, sym, v, s):
        self.put(*tab[sym])
        if s:
            self.put(v if v >= 0 else v + (1 << s) - 1, s)


def _dc(b, tab, diff):
    s = int(abs(diff)).bit_length()
    b.value(tab, s, diff, s)


def _ac(b, tab, block):
    """Coefficients 1..63 of a block (natural order in, zig-zag out): (run, size) symbols, ZRL, EOB."""
    run = 0
    for z in ZIGZAG[1:]:
        v = int(block[z])
        if v == 0:
            run += 1
            continue
        while run > 15:
            b.put(*tab[0xF0])
            run -= 16
        s = abs(v).bit_length()
        b.value(tab, (run << 4) | s, v, s)
        run = 0
    if run:
        b.put(*tab[0x00])


def _blocks(x, hs, vs, save):
    """The coefficients of a picture at luma sampling (hs, vs) in the device's layout, from two Pillow 4:4:4 files of the same settings: the Y
    blocks of the picture (zero blocks up to whole MCUs), the Cb / Cr blocks of the picture taken at every vs-th row and hs-th column. Returns
    (coefficients (mcuy, mcux, bpm, 64), the first file, its header dict)."""
    from PIL import Image
    import io

    def save444(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'JPEG', subsampling=0, **save)
        return buf.getvalue()
    h, w = x.shape[:2]
    full, small = save444(x), save444(np.ascontiguousarray(x[::vs, ::hs]))
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    cy = R.coefficients(full).reshape(-(-h // 8), -(-w // 8), 3, 64)[:, :, 0]
    cc = R.coefficients(small).reshape(my, mx, 3, 64)
    y = np.zeros((my * vs, mx * hs, 64), np.int64)
    y[:cy.shape[0], :cy.shape[1]] = cy
    coef = np.zeros((my, mx, hs * vs + 2, 64), np.int64)
    coef[:, :, :hs * vs] = y.reshape(my, vs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, hs * vs, 64)
    coef[:, :, hs * vs:] = cc[:, :, 1:]
    return coef, full, R.parse(full)


def _head(full, hdr, hs, vs, sof, ri):
    """Pillow's header up to its SOS, the frame marker `sof`, the luma sampling byte replaced, a DRI segment added."""
    d = bytearray(full[:hdr['offset']])
    p = 2
    while d[p + 1] != 0xC0:
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
    d[p + 1] = sof
    assert d[p + 11] == 0x11
    d[p + 11] = (hs << 4) | vs
    sos = bytes(d).rindex(b'\xff\xda')
    return bytes(d[:sos]) + (b'\xff\xdd\x00\x04' + ri.to_bytes(2, 'big') if ri else b''), bytes(d[sos:])


def write_baseline(x, hs, vs, ri=0, **save):
    """A baseline file of luma sampling (hs, vs): the blocks of `_blocks` recoded with the file's own Huffman tables in interleaved MCU order, a
    restart marker every `ri` MCUs."""
    coef, full, hdr = _blocks(x, hs, vs, save)
    dc, ac = {k: _codes(*v) for k, v in hdr['dc'].items()}, {k: _codes(*v) for k, v in hdr['ac'].items()}
    sel = [(0, s[1], s[2]) for s in hdr['scan'][:1]] * (hs * vs) + [(k, s[1], s[2]) for k, s in enumerate(hdr['scan']) if k]
    head, sos = _head(full, hdr, hs, vs, 0xC0, ri)
    b, pred = _Bits(), [0, 0, 0]
    for m, mcu in enumerate(coef.reshape(-1, hs * vs + 2, 64)):
        if ri and m and m % ri == 0:
            b.flush()
            b.out += bytes([0xFF, 0xD0 + ((m // ri - 1) & 7)])
            pred = [0, 0, 0]
        for (c, td, ta), block in zip(sel, mcu):
            _dc(b, dc[td], int(block[0]) - pred[c])
            pred[c] = int(block[0])
            _ac(b, ac[ta], block)
    b.flush()
    return head + sos + bytes(b.out) + b'\xff\xd9'


def write_progressive(x, hs, vs, **save):
    """The same coefficients as a progressive file, spectral selection only: one interleaved DC scan, then per component one scan of
    coefficients 1..63 over its real blocks. No successive approximation, no end-of-band runs."""
    coef, full, hdr = _blocks(x, hs, vs, save)
    dc, ac = {k: _codes(*v) for k, v in hdr['dc'].items()}, {k: _codes(*v) for k, v in hdr['ac'].items()}
    head, _ = _head(full, hdr, hs, vs, 0xC2, 0)
    my, mx = coef.shape[:2]
    h, w = x.shape[:2]
    ids, scan = [c[0] for c in hdr['comps']], hdr['scan']
    out = bytearray(head) + b'\xff\xda\x00\x0c\x03' + b''.join(bytes([i, (s[1] << 4) | s[2]]) for i, s in zip(ids, scan)) + b'\x00\x00\x00'
    b, pred = _Bits(), [0, 0, 0]
    for mcu in coef.reshape(-1, hs * vs + 2, 64):
        for k, block in enumerate(mcu):
            c = max(0, k - hs * vs + 1)
            _dc(b, dc[scan[c][1]], int(block[0]) - pred[c])
            pred[c] = int(block[0])
    b.flush()
    out += b.out
    for c in range(3):
        out += b'\xff\xda\x00\x08\x01' + bytes([ids[c], scan[c][2], 1, 63, 0])
        b = _Bits()
        if c == 0:
            blocks = [coef[by // vs, bx // hs, (by % vs) * hs + bx % hs] for by in range(-(-h // 8)) for bx in range(-(-w // 8))]
        else:
            blocks = coef[:, :, hs * vs + c - 1].reshape(-1, 64)
        for block in blocks:
            _ac(b, ac[scan[c][2]], block)
        b.flush()
        out += b.out
    return bytes(out + b'\xff\xd9')


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 4), (2, 5), (4, 4), (8, 8), (9, 4), (4, 9), (8, 15), (8, 16), (8, 17), (15, 8), (17, 8), (5, 31),
         (5, 33), (8, 65), (17, 23), (23, 17), (33, 65), (37, 53), (64, 48)]
PROG_SIZES = [(1, 1), (9, 4), (17, 23), (37, 53)]              # the writer's progressive script
QUALITIES = (1, 50, 90, 100)
TAGS = {'restart_marker_blocks': 'rsb', 'restart_marker_rows': 'rsr'}


def _cases():
    """name -> (sampling, h, w, kind, source, settings). source 'pillow': Pillow's own file (4:2:2 only), settings its save arguments; 'base' /
    'prog': the writers, settings theirs."""
    c = {}

    def add(samp, h, w, kind, source, **kw):
        tag = '_'.join('%s%s' % (TAGS.get(k, k[:3]), 'T' if v is True else (v if np.isscalar(v) else v[0][0])) for k, v in sorted(kw.items()))
        name = '%s_%dx%d_%s_%s_%s' % (samp, h, w, kind, source, tag)
        assert name not in c, name
        c[name] = (samp, h, w, kind, source, kw)
    for samp in SAMPLINGS:
        own = 'pillow' if samp == '422' else 'base'
        for i, (h, w) in enumerate(SIZES):
            add(samp, h, w, R.KINDS[(i + i // 4) % 4], own, quality=QUALITIES[i % 4])
        for h, w, kind, q in ((37, 53, 'uniform', 90), (64, 48, 'smooth', 50)):
            mx = -(-w // (8 * SAMPLINGS[samp][0]))
            if samp == '422':
                add(samp, h, w, kind, 'pillow', quality=q, optimize=True)
                add(samp, h, w, kind, 'pillow', quality=q, restart_marker_blocks=1)
                add(samp, h, w, kind, 'pillow', quality=q, restart_marker_blocks=3, optimize=True)
                add(samp, h, w, kind, 'pillow', quality=q, restart_marker_rows=1)
            for ri in sorted({1, 3, mx}):                        # every MCU, every third, every MCU row
                add(samp, h, w, kind, 'base', quality=q, ri=ri)
            for t in (1, 255):
                add(samp, h, w, 'binary', own, qtables=[[t] * 64] * 2)
    for h, w in ((1, 3), (17, 23), (37, 53)):                  # the writer against Pillow's own sampling
        add('422', h, w, 'uniform', 'base', quality=90)
    for i, (h, w) in enumerate(SIZES):                         # Pillow's full script: ten scans with successive approximation
        for q in (50, 90):
            add('422', h, w, R.KINDS[(i + q // 40) % 4], 'pillow', quality=q, progressive=True)
    add('422', 37, 53, 'uniform', 'pillow', quality=90, progressive=True, restart_marker_blocks=1)
    for samp in ('440', '411'):
        for i, (h, w) in enumerate(PROG_SIZES):
            add(samp, h, w, R.KINDS[i % 4], 'prog', quality=QUALITIES[(i + 1) % 4])
    return c


CASES = _cases()
_STREAMS = {}


def stream(name):
    """The bytes of a case (made once per process)."""
    if name not in _STREAMS:
        samp, h, w, kind, source, kw = CASES[name]
        if source == 'pillow':
            _STREAMS[name] = PR.stream(h, w, kind, 1, kw)
        else:
            x = R.image(h, w, kind, 100 * h + w, 0)
            _STREAMS[name] = (write_baseline if source == 'base' else write_progressive)(x, *SAMPLINGS[samp], **kw)
    return _STREAMS[name]


def parts(n):
    """The case names in n parts of about the same work."""
    names = sorted(CASES, key=lambda k: (CASES[k][1] * CASES[k][2], k))
    return [names[i::n] for i in range(n)]


pillow = R.pillow
