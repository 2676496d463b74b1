"""A plain baseline JPEG encoder in Python / NumPy for the tests of maggie_amd/utils/jpegenc.py: the file `PIL.Image.fromarray(x).save(buf,
'JPEG', quality=q)` writes for an (h, w, 3) uint8 RGB frame -- 4:2:0, the Annex K tables, no optimisation, no restart markers -- byte for
byte. The lossy half (colour conversion, edge replication, 2 x 2 down-sampling, the forward transform) is imported from
tests/photometric_restatement.py, which holds it against Pillow; what is stated here is what DESIGN.md section 28 adds. Nothing here imports
the package. tests/test_jpegenc_cpu.py holds `file_bytes` against Pillow itself.

  * `coefficients(x, quality)`  the quantised coefficients in scan order (MCUs row by row, y0 y1 y2 y3 cb cr in an MCU), natural order in a
                                block, DC terms not differenced: the layout of `jpegdec_restatement.coefficients`. A luma block that lies wholly
                                beyond ceil(w / 8) block columns or ceil(h / 8) block rows is a DUMMY block: all AC terms zero, its DC the DC of
                                the block before it in the MCU (y1 <- y0, y2 <- y1, y3 <- y2). Chroma has none in 4:2:0.
  * `block_bits(coef)`          the bits each block takes in the scan.
  * `scan(coef)`                (unstuffed, stuffed): the entropy-coded segment before and after the 0x00 behind every 0xFF byte; the last byte
                                is filled with 1-bits.
  * `header(h, w, tables)`      the 623 bytes in front of the scan.
  * `file_bytes(x, quality)`    header + stuffed scan + EOI."""
import io

import numpy as np

import photometric_restatement as P

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ISO/IEC 10918-1 Annex K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
TABLES = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)              # the order of the DHT segments: DC0, AC0, DC1, AC1

MAX_BLOCK_BITS = 20 + 63 * 26                                  # DC: 9 code + 11 value bits; an AC term: 16 code + 10 value bits


def codes_of(counts, values):
    """{symbol: (code, length)}: the canonical codes of T.81 Annex C."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[values[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = [codes_of(*t) for t in TABLES]                         # DC0, AC0, DC1, AC1


def tables_of(quality):
    """(2, 64) int64 in natural order: a quality 1..100, or a table taken as it is."""
    return np.asarray(quality, np.int64).reshape(2, 64) if np.ndim(quality) else P.quant_tables(quality)


def geometry(h, w):
    """(MCU columns, MCU rows, real luma block columns, real luma block rows)."""
    return (w + 15) // 16, (h + 15) // 16, (w + 7) // 8, (h + 7) // 8


def quantise(c, t):
    """k = sign(c) * ((|c| + qv // 2) // qv), qv = 8 t (the transform carries a factor 8)."""
    qv = 8 * t
    return np.sign(c) * ((np.abs(c) + qv // 2) // qv)


def plane_coefficients(p, t):
    """int64 (H, W) samples with sides that are multiples of 8 -> (H / 8, W / 8, 64) quantised coefficients, natural order."""
    H, W = p.shape
    b = (p - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    return quantise(P.fdct(b), t.reshape(8, 8)).reshape(H // 8, W // 8, 64)


def coefficients(x, quality):
    """(blocks, 64) int64: see the module docstring."""
    h, w = x.shape[:2]
    mx, my, bw, bh = geometry(h, w)
    t = tables_of(quality)
    Y, Cb, Cr = (P.pad_rows(P.pad_cols(p, 16 * mx), h + (h & 1)) for p in P.rgb_to_ycc(x))
    cy = plane_coefficients(P.pad_rows(Y, 16 * my), t[0])
    cc = [plane_coefficients(P.pad_rows(P.downsample(p), 8 * my), t[1]) for p in (Cb, Cr)]
    out = np.zeros((my, mx, 6, 64), np.int64)
    for r in range(my):
        for c in range(mx):
            for k in range(4):
                br, bc = 2 * r + (k >> 1), 2 * c + (k & 1)
                if br < bh and bc < bw:
                    out[r, c, k] = cy[br, bc]
                else:                                            # a dummy block; k = 0 is always real
                    out[r, c, k, 0] = out[r, c, k - 1, 0]
            out[r, c, 4], out[r, c, 5] = cc[0][r, c], cc[1][r, c]
    return out.reshape(-1, 64)


def symbols(coef):
    """The scan as a list over the blocks of lists of (table index in CODES, symbol, value bits, number of value bits)."""
    c = np.asarray(coef, np.int64).reshape(-1, 6, 64)
    pred = [0, 0, 0]
    out = []
    for m in range(c.shape[0]):
        for k in range(6):
            comp = 0 if k < 4 else k - 3
            dc_tab, ac_tab = (0, 1) if comp == 0 else (2, 3)
            blk = c[m, k]
            d = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            n = abs(d).bit_length()
            s = [(dc_tab, n, (d if d >= 0 else d - 1) & ((1 << n) - 1), n)]
            run = 0
            for z in range(1, 64):
                v = int(blk[ZIGZAG[z]])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    s.append((ac_tab, 0xF0, 0, 0))
                    run -= 16
                n = abs(v).bit_length()
                s.append((ac_tab, (run << 4) | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
                run = 0
            if run:
                s.append((ac_tab, 0x00, 0, 0))
            out.append(s)
    return out


def block_bits(coef):
    """(blocks,) int64: the bits of each block in the scan."""
    return np.array([sum(CODES[t][sym][1] + n for t, sym, _, n in s) for s in symbols(coef)], np.int64)


def scan(coef):
    """(unstuffed, stuffed) bytes of the entropy-coded segment."""
    acc = nbits = 0
    for s in symbols(coef):
        for t, sym, v, n in s:
            code, l = CODES[t][sym]
            acc = (acc << (l + n)) | (code << n) | v
            nbits += l + n
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, 'big')
    return raw, raw.replace(b'\xff', b'\xff\x00')


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)


def header(h, w, quality):
    """SOI, APP0 (JFIF 1.01, no units, 1 : 1), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS."""
    t = tables_of(quality)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for k in range(2):
        out.append(_segment(0xDB, bytes([k]) + bytes(int(v) for v in t[k][ZIGZAG])))
    out.append(_segment(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for ident, (counts, values) in zip((0x00, 0x10, 0x01, 0x11), TABLES):
        out.append(_segment(0xC4, bytes([ident]) + bytes(counts) + bytes(values)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])))
    return b''.join(out)


def file_bytes(x, quality):
    h, w = x.shape[:2]
    return header(h, w, quality) + scan(coefficients(x, quality))[1] + b'\xff\xd9'


def pillow(x, quality):
    """The bytes Pillow writes: a quality, or a (2, 64) table (Pillow's `qtables` lists are in natural order, as the table is here)."""
    from PIL import Image
    buf = io.BytesIO()
    if np.ndim(quality):
        t = np.asarray(quality).reshape(2, 64)
        Image.fromarray(x).save(buf, 'JPEG', qtables=[[int(v) for v in t[0]], [int(v) for v in t[1]]], subsampling=2)
    else:
        Image.fromarray(x).save(buf, 'JPEG', quality=int(quality))
    return buf.getvalue()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
QUALITIES = (1, 21, 50, 75, 80, 100)
CRAFTED = ('blocks', 'checker', 'columns')


def crafted(kind, seed=0):
    """48 x 48 inputs the random kinds do not make reliably: whole 8 x 8 blocks of 0 or 255, a one-pixel checkerboard, one-pixel columns."""
    yy, xx = np.mgrid[0:48, 0:48]
    if kind == 'blocks':
        g = np.random.RandomState(7 + seed).randint(0, 2, (6, 6, 3)) * 255
        x = np.repeat(np.repeat(g, 8, 0), 8, 1)
    elif kind == 'checker':
        x = np.repeat((((yy + xx) & 1) * 255)[..., None], 3, 2)
    else:
        x = np.repeat(((xx & 1) * 255)[..., None], 3, 2) + 0 * yy[..., None]
    return x.astype(np.uint8)


def _cases():
    c = {}
    for h, w in P.SHAPES:
        for q in QUALITIES:
            for kind in P.KINDS:
                c['%dx%d_%s_q%d' % (h, w, kind, q)] = (h, w, kind, q, P.seed_of(h, w, q, kind))
    for kind in CRAFTED:
        for q in QUALITIES:
            c['48x48_%s_q%d' % (kind, q)] = (48, 48, kind, q, 0)
    return c


CASES = _cases()                                               # name -> (h, w, kind, quality, seed)


def image(h, w, kind, seed):
    return crafted(kind, seed) if kind in CRAFTED else P.inputs(h, w, kind, seed)


def events(coef):
    """What the coverage condition of tests/test_jpegenc_cpu.py counts in one file's scan."""
    ev = dict(zrl=0, no_eob=0, ac10=0, dc11=0)
    for s in symbols(coef):
        ev['dc11'] += s[0][1] == 11
        ev['zrl'] += sum(1 for _, sym, _, _ in s[1:] if sym == 0xF0)
        ev['ac10'] += sum(1 for _, sym, _, _ in s[1:] if sym & 15 == 10)
        ev['no_eob'] += len(s) > 1 and s[-1][1] != 0x00
    return ev
