"""PNG frames and planes restated sequentially in Python from the PNG specification (RFC 2083: sample packing, Adam7, scanline filters) and
Pillow's `convert("RGB")` / `convert("L")`: what maggie_amd/utils/pngcolor.py and csrc/pngcolor.hip are tested against, next to live Pillow.

  * the writer: `pack` (samples of any depth -> scanline bytes, MSB first), `sub_images` (the 7-pass split), `make` (a file from samples, with a
    chosen or drawn filter type per row; the prior row restarts at each pass). Pillow writes no Adam7 and no 16-bit RGB(A).
  * the decoder: `decode_samples` (zlib, then per pass the sequential `unfilter` of tests/pngdec_restatement.py, unpacking, scattering).
  * the conversions of DESIGN.md section 34: `to_rgb`, `to_l`.
  * the case list: `small_cases` (every shape at which the kernels can go wrong) and `clip_cases` (the 270 x 480 clip)."""
import io
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pngdec_restatement as P                              # noqa: E402

CHANNELS = P.CHANNELS
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
INDEX = P.INDEX


def bpp_of(ct, depth):
    return max(1, CHANNELS[ct] * depth // 8)


def pass_table(w, h, ct, depth, interlace):
    """[(pw, ph, rb, offset)] by the formula of the specification, and the total of the inflated bytes."""
    table, off = [], 0
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        pw = len(range(x0, w, dx))
        ph = len(range(y0, h, dy))
        rb = (pw * CHANNELS[ct] * depth + 7) // 8
        table.append((pw, ph, rb, off))
        if pw and ph:
            off += ph * (1 + rb)
    return table, off


# ---- the writer -------------------------------------------------------------------------------------------------------------------------------
def pack(samples, depth):
    """Samples int (h, w, ch) -> scanline bytes uint8 (h, rb): 16-bit samples big-endian, sub-byte samples MSB first, padding bits zero."""
    h, w, ch = samples.shape
    if depth == 16:
        out = np.zeros((h, w * ch, 2), np.uint8)
        flat = samples.reshape(h, w * ch)
        out[..., 0], out[..., 1] = flat >> 8, flat & 255
        return out.reshape(h, w * ch * 2)
    if depth == 8:
        return samples.reshape(h, w * ch).astype(np.uint8)
    ppb = 8 // depth
    rb = (w + ppb - 1) // ppb
    out = np.zeros((h, rb), np.uint8)
    for x in range(w):
        out[:, x // ppb] |= (samples[:, x, 0] << (8 - depth * (x % ppb + 1))).astype(np.uint8)
    return out


def sub_images(samples, interlace):
    return [samples[y0::dy, x0::dx] for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),))]


def make(samples, ct, depth, *, interlace=0, types=None, seed=0, plte=None, trns=None, extra=b''):
    """A PNG file of `samples` int (h, w, channels). `types`: one filter type for every row, or None = one drawn per row."""
    h, w, _ = samples.shape
    rng = np.random.RandomState(seed)
    raw = b''
    for sub in sub_images(samples, interlace):
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        rows = pack(sub, depth)
        tt = [int(t) for t in rng.randint(0, 5, sub.shape[0])] if types is None else [types] * sub.shape[0]
        raw += P.filter_rows(rows, tt, bpp_of(ct, depth))
    return P.png(w, h, depth, ct, raw, plte=plte, trns=trns, interlace=interlace, extra=extra)


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------
def unpack(rows, pw, ch, depth):
    h = rows.shape[0]
    if depth == 16:
        r = rows.astype(np.int64).reshape(h, pw * ch, 2)
        return (r[..., 0] << 8 | r[..., 1]).reshape(h, pw, ch)
    if depth == 8:
        return rows.astype(np.int64).reshape(h, pw, ch)
    ppb = 8 // depth
    s = np.zeros((h, rows.shape[1] * ppb), np.int64)
    for i in range(ppb):
        s[:, i::ppb] = (rows >> (8 - depth * (i + 1))) & ((1 << depth) - 1)
    return s[:, :pw, None]


def decode_samples(data):
    """A file -> (the defiltered bytes: every scanline behind its filter type byte, pass after pass; the samples int (h, w, channels); IHDR;
    PLTE bytes or None)."""
    ihdr, plte, z, _ = P.walk(data)
    w, h, depth, ct, _, _, lace = ihdr
    raw = zlib.decompress(z)
    table, total = pass_table(w, h, ct, depth, lace)
    assert len(raw) == total, (len(raw), total)
    ch = CHANNELS[ct]
    samples = np.zeros((h, w, ch), np.int64)
    out = bytearray()
    for (pw, ph, rb, off), (x0, y0, dx, dy) in zip(table, ADAM7 if lace else ((0, 0, 1, 1),)):
        if not pw or not ph:
            continue
        part = raw[off:off + ph * (1 + rb)]
        rows = P.unfilter(part, ph, rb, bpp_of(ct, depth))         # the prior row is zero at the first row of the pass
        for y in range(ph):
            out.append(part[y * (1 + rb)])
            out += rows[y].tobytes()
        samples[y0::dy, x0::dx] = unpack(rows, pw, ch, depth)
    return bytes(out), samples, ihdr, plte


def luma(rgb):
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def to_rgb(samples, ct, depth, plte=None):
    """Pillow's convert("RGB") of the samples: uint8 (h, w, 3)."""
    s = samples
    if ct == 3:
        pal = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        if s.max() >= len(pal):
            raise P.Corrupt(INDEX, 'a palette index past the last entry')
        return pal[s[..., 0]]
    if ct in (0, 4):
        g = s[..., 0]
        if depth == 16:
            g = np.minimum(g, 255) if ct == 0 else g >> 8          # grey 16 saturates (Pillow's I;16); grey + alpha 16 takes the high byte
        elif depth < 8:
            g = g * (255 // ((1 << depth) - 1))
        return np.repeat(g[..., None], 3, -1).astype(np.uint8)
    v = s[..., :3]
    return (v >> 8 if depth == 16 else v).astype(np.uint8)


def to_l(samples, ct, depth, plte=None):
    rgb = to_rgb(samples, ct, depth, plte)
    return rgb[..., 0].copy() if ct in (0, 4) else luma(rgb)


def decode(data):
    """A file -> (defiltered bytes, RGB uint8 (h, w, 3), L uint8 (h, w))."""
    raw, s, ihdr, plte = decode_samples(data)
    return raw, to_rgb(s, ihdr[3], ihdr[2], plte), to_l(s, ihdr[3], ihdr[2], plte)


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), np.asarray(Image.open(io.BytesIO(data)).convert('L'))


# ---- the case list ----------------------------------------------------------------------------------------------------------------------------
def draw(w, h, ct, depth, seed, entries=None):
    """Samples int (h, w, channels): noise below 2^depth (below `entries` for a palette), smoothed a little so that every filter type pays."""
    rng = np.random.RandomState(seed)
    top = entries if ct == 3 else 1 << depth
    a = rng.randint(0, top, (h, w, CHANNELS[ct])).astype(np.int64)
    if h > 2 and w > 2 and ct != 3:
        a[1:, 1:] = (a[1:, 1:] + 3 * a[:-1, :-1]) // 4
    return a


def palette(n, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8).tobytes()


def _file(w, h, ct, depth, lace, seed, types=None, entries=None, trns=None, extra=b''):
    plte = None
    if ct == 3:
        entries = entries or (1 << depth)
        plte = palette(entries, seed + 1000)
    return make(draw(w, h, ct, depth, seed, entries), ct, depth, interlace=lace, types=types, seed=seed, plte=plte, trns=trns, extra=extra)


def small_cases():
    """{name: file}. Sizes are width x height."""
    c = {}
    seed = [0]

    def add(name, *a, **kw):
        seed[0] += 1
        c[name] = _file(*a, seed=seed[0], **kw)
    # all 15 (type, depth) pairs x interlace, one size: any three of them are a clip of mixed type, depth and interlace
    for ct, depth in PAIRS:
        for lace in (0, 1):
            add('pair_c%d_d%d_i%d_17x13' % (ct, depth, lace), 17, 13, ct, depth, lace)
    # every filter type on every row -- the first pixel and the first row of each pass with Avg and Paeth among them -- at bpp 1, 2, 3, 4, 6, 8
    for ct, depth in ((0, 8), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16)):
        for ft in range(5):
            add('ft%d_bpp%d_i1_9x9' % (ft, bpp_of(ct, depth)), 9, 9, ct, depth, 1, types=ft)
            add('ft%d_bpp%d_i0_5x5' % (ft, bpp_of(ct, depth)), 5, 5, ct, depth, 0, types=ft)
    # sizes with empty passes and the smallest ones
    for w, h in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (4, 4), (5, 5), (8, 8), (9, 9)):
        for ct, depth in ((2, 8), (0, 1), (3, 2), (4, 16)):
            for lace in (0, 1):
                add('size_c%d_d%d_i%d_%dx%d' % (ct, depth, lace, w, h), w, h, ct, depth, lace)
    for ct in (0, 3):                                          # the padding bits of pass rows
        for lace in (0, 1):
            add('bits_c%d_d1_i%d_11x6' % (ct, lace), 11, 6, ct, 1, lace)
    for w in (15, 16, 17, 33):                                 # the 16-pixel lanes of the convert kernel
        for ct, depth in ((2, 8), (3, 4), (0, 16)):
            for lace in (0, 1):
                add('lane_c%d_d%d_i%d_%dx3' % (ct, depth, lace, w), w, 3, ct, depth, lace)
    for ct, depth, w in ((0, 8, 63), (0, 8, 64), (0, 8, 65), (2, 8, 21), (6, 16, 8), (0, 1, 513), (2, 16, 11)):      # row bytes 63, 64, 65 (66): the tile step
        add('rowbytes%d_c%d_d%d_i0_%dx3' % (P.rowbytes(ct, depth, w), ct, depth, w), w, 3, ct, depth, 0)
    for h in (64, 65, 129):                                    # the band carry
        add('band_c2_d8_i0_5x%d' % h, 5, h, 2, 8, 0)
        add('band_c0_d16_i0_3x%d' % h, 3, h, 0, 16, 0)
    add('band_c2_d8_i1_9x131', 9, 131, 2, 8, 1)                # pass 7 has 65 rows: more than one band
    add('band_c6_d16_i1_9x131', 9, 131, 6, 16, 1)
    # grey 16 holding 0, 255, 256 and 65535
    edge = np.array([0, 255, 256, 65535, 1, 254, 257, 32768], np.int64).reshape(2, 4, 1)
    c['grey16_edges_i0_4x2'] = make(edge, 0, 16, types=0)
    c['grey16_edges_i1_4x2'] = make(edge, 0, 16, interlace=1, types=4)
    # palettes shorter than 2^depth, tRNS on palette, grey and RGB files, ancillary chunks in front of PLTE
    for depth, entries in ((1, 1), (2, 3), (4, 11), (8, 200)):
        add('short_palette_d%d_i%d_13x7' % (depth, depth & 1), 13, 7, 3, depth, depth & 1, entries=entries)
    add('trns_palette_i1_13x7', 13, 7, 3, 4, 1, entries=9, trns=bytes([0, 128, 255, 7]))
    add('trns_grey_i0_13x7', 13, 7, 0, 8, 0, trns=struct.pack('>H', 200))
    add('trns_rgb_i1_13x7', 13, 7, 2, 8, 1, trns=struct.pack('>HHH', 1, 2, 3))
    add('trns_rgb16_i0_13x7', 13, 7, 2, 16, 0, trns=struct.pack('>HHH', 256, 2, 3), extra=P.chunk(b'gAMA', struct.pack('>I', 45455)))
    return c


def clip_cases():
    """The 270 x 480 RGB-8 clip of 4 as Pillow writes it: {name: file}."""
    from PIL import Image
    c = {}
    for k in range(4):
        a = P.content(270, 480, 'smooth', 40 + k, 3).astype(np.int32) + np.random.RandomState(k).randint(0, 16, (270, 480, 3))
        c['clip%d_c2_d8_i0_480x270' % k] = P._save(Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)))
    return c


def golden_names(cases):
    """The subset the pinned fixture holds: each (colour type, depth) pair once, interlaced or not in turn, the grey-16 edge values, a short
    palette and a palette with tRNS."""
    pairs = ['pair_c%d_d%d_i%d_17x13' % (ct, depth, k & 1) for k, (ct, depth) in enumerate(PAIRS)]
    return sorted(pairs + [n for n in cases if n.startswith(('grey16_', 'short_palette_d4', 'trns_palette'))])
