"""The photometric steps of the loaders' training stream in integer NumPy, for the tests of maggie_amd/utils/photometric.py. Nothing here
imports the package.

  lut -> additive noise -> JPEG round trip   (him.py:46-48, vim.py:51-54, transforms.py:812-924)

The JPEG round trip restates what libjpeg-turbo computes at Pillow's defaults -- baseline, 4:2:0, JDCT_ISLOW, no smoothing, fancy upsampling --
without the entropy coding, which is lossless: colour conversion, edge replication, h2v2 downsampling, the Loeffler-Ligtenberg-Moschytz forward
DCT, quantisation, dequantisation, the inverse DCT, triangle upsampling and the conversion back. All arithmetic is integer (int64 here; every
intermediate fits an int32) and `>>` is arithmetic. tests/test_photometric_cpu.py holds it against Pillow itself."""
import numpy as np

# ISO/IEC 10918-1 Annex K, tables K.1 and K.2, natural (row-major) order
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)

CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172


def quality_from_compression(c):
    return int(np.clip(np.round(1 + 99 * (1 - c / 100.)), 1, 100))


def quant_tables(quality):
    """(2, 64) int64, natural order: luma, chroma (jpeg_set_quality with force_baseline)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality must be in 1..100')
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)])


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first):
    """One pass of jpeg_fdct_islow along the last axis of int64 (..., 8)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        o0, o4 = (tmp10 + tmp11) * (1 << PASS1_BITS), (tmp10 - tmp11) * (1 << PASS1_BITS)
    else:
        o0, o4 = descale(tmp10 + tmp11, PASS1_BITS), descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * F_0_541196100
    o2 = descale(z1 + tmp13 * F_0_765366865, n)
    o6 = descale(z1 + tmp12 * (-F_1_847759065), n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F_1_175875602
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F_0_298631336, tmp5 * F_2_053119869, tmp6 * F_3_072711026, tmp7 * F_1_501321110
    z1, z2, z3, z4 = z1 * (-F_0_899976223), z2 * (-F_2_562915447), z3 * (-F_1_961570560), z4 * (-F_0_390180644)
    z3, z4 = z3 + z5, z4 + z5
    o7, o5, o3, o1 = descale(tmp4 + z1 + z3, n), descale(tmp5 + z2 + z4, n), descale(tmp6 + z2 + z3, n), descale(tmp7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct(blocks):
    """jpeg_fdct_islow of int64 (..., 8, 8) blocks of samples minus 128: rows, then columns. The result carries a factor 8."""
    rows = fdct_1d(blocks, True)
    return np.swapaxes(fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def idct_1d(d, n):
    """One pass of jpeg_idct_islow along the last axis, descaled by n bits."""
    in0, in1, in2, in3, in4, in5, in6, in7 = (d[..., k] for k in range(8))
    z1 = (in2 + in6) * F_0_541196100
    tmp2 = z1 + in6 * (-F_1_847759065)
    tmp3 = z1 + in2 * F_0_765366865
    tmp0, tmp1 = (in0 + in4) << CONST_BITS, (in0 - in4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = in7, in5, in3, in1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175875602
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298631336, tmp1 * F_2_053119869, tmp2 * F_3_072711026, tmp3 * F_1_501321110
    z1, z2, z3, z4 = z1 * (-F_0_899976223), z2 * (-F_2_562915447), z3 * (-F_1_961570560), z4 * (-F_0_390180644)
    z3, z4 = z3 + z5, z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([descale(tmp10 + tmp3, n), descale(tmp11 + tmp2, n), descale(tmp12 + tmp1, n), descale(tmp13 + tmp0, n),
                     descale(tmp13 - tmp0, n), descale(tmp12 - tmp1, n), descale(tmp11 - tmp2, n), descale(tmp10 - tmp3, n)], -1)


def idct(coefs):
    """jpeg_idct_islow of dequantised int64 (..., 8, 8) blocks: columns, then rows, + 128, clamp."""
    cols = np.swapaxes(idct_1d(np.swapaxes(coefs, -1, -2), CONST_BITS - PASS1_BITS), -1, -2)
    return np.clip(idct_1d(cols, CONST_BITS + PASS1_BITS + 3) + 128, 0, 255)


def quantise(c, t):
    """k = sign(c) * ((|c| + qv // 2) // qv), qv = 8 t; returns the dequantised k * t."""
    qv = 8 * t
    return np.sign(c) * ((np.abs(c) + qv // 2) // qv) * t


def code_plane(p, t):
    """The lossy part of one component plane whose sides are multiples of 8: int64 (H, W) samples -> decoded samples."""
    H, W = p.shape
    b = (p - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    out = idct(quantise(fdct(b), t.reshape(8, 8)))
    return out.transpose(0, 2, 1, 3).reshape(H, W)


def rgb_to_ycc(x):
    R, G, B = (x[..., k].astype(np.int64) for k in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def ycc_to_rgb(Y, Cb, Cr):
    R = Y + ((91881 * (Cr - 128) + 32768) >> 16)
    B = Y + ((116130 * (Cb - 128) + 32768) >> 16)
    G = Y + ((-22554 * (Cb - 128) - 46802 * (Cr - 128) + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


def downsample(p):
    """h2v2_downsample of an int64 plane with even sides: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... along the output columns."""
    bias = 1 + (np.arange(p.shape[1] // 2) & 1)
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2


def pad_rows(p, H):
    return np.concatenate([p, np.repeat(p[-1:], H - p.shape[0], 0)], 0) if H > p.shape[0] else p


def pad_cols(p, W):
    return np.concatenate([p, np.repeat(p[:, -1:], W - p.shape[1], 1)], 1) if W > p.shape[1] else p


def upsample(p, h, w):
    """The decoder's chroma upsampling of the real (ceil(h / 2), ceil(w / 2)) int64 plane to (h, w): the triangle filter, or plain 2 x 2
    replication when the plane is at most 2 samples wide."""
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, 0), 2, 1)[:h, :w]
    up, dn = p[np.maximum(np.arange(ch) - 1, 0)], p[np.minimum(np.arange(ch) + 1, ch - 1)]
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * p + up, 3 * p + dn
    left, right = s[:, np.maximum(np.arange(cw) - 1, 0)], s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:h, :w]


def jpeg_planes(x, quality):
    """The decoded component planes of one (h, w, 3) uint8 image, padded as the coder holds them: Y (h16, w16), Cb and Cr (h16 / 2, w16 / 2),
    int64 in 0..255."""
    h, w = x.shape[:2]
    h16, w16 = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    t = np.asarray(quality, np.int64).reshape(2, 64) if np.ndim(quality) else quant_tables(quality)
    Y, Cb, Cr = (pad_rows(pad_cols(p, w16), h + (h & 1)) for p in rgb_to_ycc(x))
    planes = [code_plane(pad_rows(Y, h16), t[0])]
    for p in (Cb, Cr):
        planes.append(code_plane(pad_rows(downsample(p), h16 // 2), t[1]))
    return planes


def jpeg_roundtrip(x, quality):
    """PIL.Image.fromarray(x).save(quality=quality) -> PIL.Image.open of one (h, w, 3) uint8 image. `quality`: 1..100, or a (2, 64) table."""
    h, w = x.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    Y, Cb, Cr = jpeg_planes(x, quality)
    return ycc_to_rgb(Y[:h, :w], upsample(Cb[:ch, :cw], h, w), upsample(Cr[:ch, :cw], h, w))


def apply_lut(frames, lut):
    return np.stack([lut[c][frames[..., c]] for c in range(3)], -1).astype(np.uint8)


def add_noise(frames, noise):
    """clip(int(v) + noise, 0, 255): frames (..., h, w, 3) uint8, noise int16 (h, w, 1) or (h, w, 3)."""
    return np.clip(frames.astype(np.int64) + noise.astype(np.int64), 0, 255).astype(np.uint8)


def photometric(frames, lut=None, noise=None, quality=None):
    """lut -> noise -> JPEG round trip on (T, h, w, 3) uint8 frames; each step only when its argument is given."""
    x = np.asarray(frames)
    if lut is not None:
        x = apply_lut(x, np.asarray(lut))
    if noise is not None:
        x = add_noise(x, np.asarray(noise))
    if quality is not None:
        x = np.stack([jpeg_roundtrip(f, quality) for f in x])
    return x


def normalize(frames, mean, std):
    """ToTensor + Normalize.norm in fp32: (T, h, w, 3) uint8 -> (T, 3, h, w)."""
    f = np.moveaxis(frames.astype(np.float32), -1, 1) / np.float32(255)
    m, s = (np.asarray(v, np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    return ((f - m) / s).astype(np.float32)


def inputs(h, w, kind, seed):
    """The three test inputs: 'random' uniform, 'smooth' (a gradient plus small noise), 'binary' (random 0 / 255: drives both clamps)."""
    r = np.random.RandomState(seed)
    if kind == 'random':
        return r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 'binary':
        return (r.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([40 + 3 * xx + yy, 200 - 2 * yy - xx, 90 + 2 * ((xx + yy) % 40)], -1)
    return np.clip(base + r.randint(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


# The cases both test files run: tests/test_photometric_cpu.py holds the restatement against Pillow on every one of them, and
# tests/test_gpu_photometric.py the device against the restatement. The shapes end just below, at and above the kernel's 32 x 64 tile.
SHAPES = [(1, 1), (1, 7), (2, 2), (3, 2), (8, 8), (9, 4), (20, 4), (34, 2), (21, 5), (16, 16), (17, 23), (30, 18), (37, 53), (64, 48),
          (31, 63), (32, 64), (33, 65)]
QUALITIES = (1, 21, 50, 80, 100)
KINDS = ('random', 'smooth', 'binary')


def seed_of(h, w, q, kind):
    return 1000 * h + 10 * w + q + KINDS.index(kind)
