"""A sequential NumPy / Python statement of the device PNG encoder (maggie_amd/csrc/pngenc.hip): the byte-for-byte oracle of
the kernels, of the sanitized host build and of `maggie_amd.utils.pngenc`. Written from RFC 1950 / 1951 and the PNG specification; the block size is
a parameter. `encode_stream` returns the zlib stream AND the per-block records the device leaves, `unlimited_lengths` is the same Huffman
construction without the length limit (so that a test can prove that a case really exceeds 15 / 7 bits), `fixed_bits` / `zlib_rle` give the two
sizes the tests compare with, and `cases` is the shared case list."""
import struct
import zlib

import numpy as np

BLOCK = 16384                                                   # MG_PNGENC_BLOCK_BYTES
REC_WORDS = 88                                                  # MG_PNGENC_REC_WORDS
ADLER = 65521
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
SIGNATURE = b'\x89PNG\r\n\x1a\n'


# ---- pixels -> filtered bytes --------------------------------------------------------------------------------------------------------------------
def to_bytes(plane, mode):
    """The three input forms. 'u8': as is. 'unit': (uint8)(x * 255.0f) in float32, NaN and x < 0 -> 0, x > 1 -> 255. 'threshold': x > 0.5 -> 255."""
    a = np.asarray(plane)
    if mode == 'u8':
        assert a.dtype == np.uint8
        return a
    a = a.astype(np.float32)
    if mode == 'threshold':
        return np.where(a > np.float32(0.5), 255, 0).astype(np.uint8)
    assert mode == 'unit'
    with np.errstate(invalid='ignore'):
        y = a * np.float32(255.0)
        out = np.zeros(a.shape, np.uint8)
        ok = y >= 0                                             # false for NaN
        out[ok & (y >= 255)] = 255
        mid = ok & (y < 255)
        out[mid] = y[mid].astype(np.int32).astype(np.uint8)
    return out


def filtered(plane):
    """uint8 (h, w) -> the Sub-filtered scanlines, uint8 (h * (1 + w),): row r is 01, p[0], p[1] - p[0], ..."""
    p = np.asarray(plane, np.uint8)
    h, w = p.shape
    f = np.empty((h, 1 + w), np.uint8)
    f[:, 0] = 1
    f[:, 1] = p[:, 0]
    f[:, 2:] = p[:, 1:] - p[:, :-1]
    return f.reshape(-1)


def plane_from_filtered(f, h, w):
    """The plane whose Sub-filtered scanlines are `f` ((h, 1 + w), column 0 all ones)."""
    f = np.asarray(f, np.uint8).reshape(h, 1 + w)
    assert (f[:, 0] == 1).all()
    return np.cumsum(f[:, 1:].astype(np.int64), axis=1).astype(np.uint8)


# ---- tokens ----------------------------------------------------------------------------------------------------------------------------------------
def token_at(o, L):
    """What the byte at offset `o` of a run of length `L` starts: 0 nothing, 1 a literal, else a match of that length at distance 1."""
    if L < 4 or o == 0:
        return 1
    m = (L - 1) // 258
    q, ro = divmod(o - 1, 258)
    if q < m:
        return 258 if ro == 0 else 0
    rem = (L - 1) - 258 * m
    if rem >= 3:
        return rem if ro == 0 else 0
    return 1


def tokens(block):
    """One block's bytes -> (positions, kinds): kinds[i] = 1 for a literal of block[positions[i]], else the length of a match at distance 1."""
    b = np.asarray(block, np.uint8)
    n = b.size
    start = np.ones(n, bool)
    start[1:] = b[1:] != b[:-1]
    s = np.flatnonzero(start)
    lens = np.diff(np.append(s, n))
    pos, kind = [], []
    for s0, L in zip(s.tolist(), lens.tolist()):
        if L < 4:
            for o in range(L):
                pos.append(s0 + o)
                kind.append(1)
            continue
        for o in sorted({0, L - 2, L - 1} | set(range(1, L, 258))):        # the only offsets that can start a token
            k = token_at(o, L)
            if k:
                pos.append(s0 + o)
                kind.append(k)
    return np.asarray(pos, np.int64), np.asarray(kind, np.int64)


def tokens_slow(block):
    """The same by asking every position (the definition; `tokens` only skips positions that cannot start one)."""
    b = list(bytes(block))
    n = len(b)
    pos, kind, i = [], [], 0
    while i < n:
        e = i
        while e < n and b[e] == b[i]:
            e += 1
        for o in range(e - i):
            k = token_at(o, e - i)
            if k:
                pos.append(i + o)
                kind.append(k)
        i = e
    return np.asarray(pos, np.int64), np.asarray(kind, np.int64)


def length_symbol(length):
    """A match length 3..258 -> (literal/length symbol, extra bits, extra value)."""
    if length == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


# ---- code lengths ------------------------------------------------------------------------------------------------------------------------------------
def _depths(counts):
    """Two-queue Huffman over the used symbols sorted by (count, symbol); a tie between a leaf and an internal node takes the leaf.
    Returns (used symbols in sorted order, the depth of each)."""
    used = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    m = len(used)
    if m == 0:
        return [], []
    if m == 1:
        return used, [1]
    lw = [int(counts[s]) for s in used]
    iw, lp, ip = [], [0] * m, [0] * (m - 1)
    li = ii = 0
    for k in range(m - 1):
        w = 0
        for _ in range(2):
            if li < m and (ii >= len(iw) or lw[li] <= iw[ii]):
                w += lw[li]
                lp[li] = k
                li += 1
            else:
                w += iw[ii]
                ip[ii] = k
                ii += 1
        iw.append(w)
    idepth = [0] * (m - 1)
    for j in range(m - 3, -1, -1):
        idepth[j] = idepth[ip[j]] + 1
    return used, [idepth[lp[i]] + 1 for i in range(m)]


def unlimited_lengths(counts):
    out = [0] * len(counts)
    used, d = _depths(counts)
    for s, x in zip(used, d):
        out[s] = x
    return out


def code_lengths(counts, maxbits):
    """The lengths, limited to `maxbits`: depths above the limit are folded into it, the Kraft sum is repaired by moving one code from the
    deepest level below the limit down a level for every unit of excess, and the lengths are handed out longest first in (count, symbol) order."""
    out = [0] * len(counts)
    used, d = _depths(counts)
    if not used:
        return out
    blc = [0] * (maxbits + 1)
    for x in d:
        blc[min(x, maxbits)] += 1
    total = sum(blc[l] << (maxbits - l) for l in range(1, maxbits + 1))
    while total > (1 << maxbits):
        blc[maxbits] -= 1
        for l in range(maxbits - 1, 0, -1):
            if blc[l]:
                blc[l] -= 1
                blc[l + 1] += 2
                break
        total -= 1
    i = 0
    for l in range(maxbits, 0, -1):
        for _ in range(blc[l]):
            out[used[i]] = l
            i += 1
    return out


def canonical_codes(lens):
    """RFC 1951 3.2.2: the code of each symbol, most significant bit first."""
    maxl = max(lens) if len(lens) else 0
    blc = [0] * (maxl + 2)
    for l in lens:
        if l:
            blc[l] += 1
    nxt, c = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        c = (c + blc[l - 1]) << 1 if l > 1 else 0
        nxt[l] = c
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1)
        c >>= 1
    return r


def rle_lengths(lst):
    """The 16 / 17 / 18 coding of a length list -> [(symbol, extra bits, extra value)]: a zero run takes 18s of up to 138 while >= 11 remain, then
    17s of up to 10 while >= 3 remain, then plain zeros; another value is sent once, then 16s of up to 6 while >= 3 remain, then plain."""
    out, i, n = [], 0, len(lst)
    while i < n:
        v, r = lst[i], 1
        while i + r < n and lst[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, 7, k - 11))
                r -= k
            while r >= 3:
                k = min(r, 10)
                out.append((17, 3, k - 3))
                r -= k
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
        out.extend([(v, 0, 0)] * r)
    return out


# ---- one block -----------------------------------------------------------------------------------------------------------------------------------------
class Block:
    """type 1 fixed / 2 dynamic, bits (header and end-of-block included), nbytes, ntokens (without the end-of-block), s1 / s2 (the Adler partials:
    sum b and sum (n - i) b_i, mod 65521), hlit / hclen (codes sent), lens (286 literal/length lengths of the dynamic construction, whatever the
    type), cl_lens (19), fixed_bits, dynamic_bits, hist, cl_hist, and `code` = [(value, nbits)] in stream order."""


def encode_block(block, final):
    b = np.asarray(block, np.uint8)
    n = b.size
    pos, kind = tokens(b)
    lit = kind == 1
    hist = np.zeros(286, np.int64)
    hist[:256] += np.bincount(b[pos[lit]], minlength=256)
    msym = [length_symbol(int(k)) for k in kind[~lit]]
    for s, _, _ in msym:
        hist[s] += 1
    hist[256] = 1
    nmatch = int((~lit).sum())
    lens = code_lengths(hist.tolist(), 15)
    hlit = max(s for s in range(286) if lens[s]) + 1
    rle = rle_lengths(lens[:hlit] + [1])                                  # one distance code: code 0, length 1
    cl_hist = [0] * 19
    for s, _, _ in rle:
        cl_hist[s] += 1
    cl_lens = code_lengths(cl_hist, 7)
    hclen = max(max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1, 4)
    extra = sum(int(hist[257 + i]) * LEN_EXTRA[i] for i in range(29))
    fixed = 3 + sum(int(hist[s]) * FIXED_LENS[s] for s in range(286)) + extra + 5 * nmatch
    dyn = 3 + 14 + 3 * hclen + sum(cl_lens[s] + e for s, e, _ in rle) + sum(int(hist[s]) * lens[s] for s in range(286)) + extra + nmatch
    r = Block()
    r.type = 2 if dyn < fixed else 1
    r.bits, r.nbytes, r.ntokens, r.fixed_bits, r.dynamic_bits = min(dyn, fixed), n, int(pos.size), fixed, dyn
    w = np.arange(n, 0, -1, dtype=np.int64)
    r.s1, r.s2 = int(b.astype(np.int64).sum() % ADLER), int((w * b).sum() % ADLER)
    r.hlit, r.hclen, r.lens, r.cl_lens, r.hist, r.cl_hist = hlit, hclen, lens, cl_lens, hist, cl_hist
    code = [(1 if final else 0, 1), (r.type, 2)]
    if r.type == 2:
        code += [(hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(cl_lens[CL_ORDER[i]], 3) for i in range(hclen)]
        cc = canonical_codes(cl_lens)
        for s, e, v in rle:
            code.append((_rev(cc[s], cl_lens[s]), cl_lens[s]))
            if e:
                code.append((v, e))
        use, dbits = lens, 1
    else:
        use, dbits = FIXED_LENS, 5
    cc = canonical_codes(use)
    rc = [_rev(cc[s], use[s]) for s in range(286)]
    mi = 0
    for p, k in zip(pos.tolist(), kind.tolist()):
        if k == 1:
            s = int(b[p])
            code.append((rc[s], use[s]))
        else:
            s, e, v = msym[mi]
            mi += 1
            code.append((rc[s] | (v << use[s]) , use[s] + e + dbits))          # length code, its extra bits, the distance code 0
    code.append((rc[256], use[256]))
    assert sum(nb for _, nb in code) == r.bits, (sum(nb for _, nb in code), r.bits, r.type)
    r.code = code
    return r


def record(r):
    """The int32 record of a block (MG_PNGENC_REC_WORDS words, include/maggie_hip.h)."""
    rec = np.zeros(REC_WORDS, np.int32)
    rec[:8] = [r.type, r.bits, r.nbytes, r.ntokens, r.s1, r.s2, r.hlit, r.hclen]
    lb = np.zeros(288, np.uint8)
    lb[:286] = r.lens
    rec[8:80] = lb.view(np.int32)
    cb = np.zeros(20, np.uint8)
    cb[:19] = r.cl_lens
    rec[80:85] = cb.view(np.int32)
    return rec


def _pack(code):
    v = np.asarray([c for c, _ in code], np.int64)
    nb = np.asarray([n for _, n in code], np.int64)
    start = np.cumsum(nb) - nb
    idx = np.repeat(np.arange(v.size), nb)
    within = np.arange(int(nb.sum())) - np.repeat(start, nb)
    return ((v[idx] >> within) & 1).astype(np.uint8)


def encode_stream(f, B=BLOCK):
    """The filtered bytes of one plane -> (zlib stream, [Block])."""
    f = np.asarray(f, np.uint8).reshape(-1)
    nb = -(-f.size // B)
    blocks = [encode_block(f[k * B:(k + 1) * B], k == nb - 1) for k in range(nb)]
    bits = np.concatenate([_pack(r.code) for r in blocks])
    body = np.packbits(bits, bitorder='little').tobytes()
    A, Bs = 1, 0
    for r in blocks:                                                    # the partials combined in block order
        Bs = (Bs + r.nbytes * A + r.s2) % ADLER
        A = (A + r.s1) % ADLER
    assert ((Bs << 16) | A) == zlib.adler32(f.tobytes())
    return b'\x78\x01' + body + struct.pack('>I', (Bs << 16) | A), blocks


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def png_file(h, w, stream):
    return SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0)) + chunk(b'IDAT', stream) + chunk(b'IEND', b'')


def encode(plane, B=BLOCK, mode='u8'):
    """A plane -> (the PNG file, [Block])."""
    p = to_bytes(plane, mode)
    stream, blocks = encode_stream(filtered(p), B)
    return png_file(p.shape[0], p.shape[1], stream), blocks


def idat(data):
    """The concatenated IDAT payloads of a PNG file."""
    p, out = 8, []
    while p < len(data):
        size, kind = struct.unpack('>I4s', data[p:p + 8])
        if kind == b'IDAT':
            out.append(data[p + 8:p + 8 + size])
        p += 12 + size
    return b''.join(out)


def all_fixed_bytes(blocks):
    """The size of the zlib stream had every block taken the fixed form of its own tokens."""
    return 2 + (sum(r.fixed_bits for r in blocks) + 7) // 8 + 4


def zlib_rle(f):
    """The reference writer's configuration restated: zlib level 1, Z_RLE, on the same filtered bytes."""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(bytes(f)) + c.flush()


# ---- the case list -----------------------------------------------------------------------------------------------------------------------------------
def soft_ellipse(h, w, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx, ry, rx = h * (0.45 + 0.1 * rng.rand()), w * (0.45 + 0.1 * rng.rand()), h * 0.3, w * 0.33
    d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
    return np.clip((1.15 - d) / 0.3, 0, 1).astype(np.float32)


def _mixed(h, w, seed):
    """Flat stretches, ramps and noise side by side, so that every token kind appears at a small size."""
    rng = np.random.RandomState(seed)
    p = np.zeros((h, w), np.uint8)
    for r in range(h):
        x = 0
        while x < w:
            n = int(rng.choice([1, 2, 3, 4, 5, 9, 40, 300, 700]))
            k = rng.randint(3)
            seg = np.full(n, rng.randint(256)) if k == 0 else (rng.randint(256) + rng.randint(1, 4) * np.arange(n) if k == 1 else rng.randint(0, 256, n))
            p[r, x:x + n] = seg[:w - x].astype(np.uint8)
            x += n
    return p


def _no_repeat(n, seed):
    """n bytes in 2..250 without two equal neighbours."""
    v = np.random.RandomState(seed).randint(2, 250, n).astype(np.int64)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = 2 + (v[i] - 1) % 248
    return v.astype(np.uint8)


def _exact(n):
    """(h, w) with h * (1 + w) = n and w <= 16383."""
    for h in range(1, n + 1):
        if n % h == 0 and 1 <= n // h - 1 <= 16383:
            return h, n // h - 1
    raise ValueError(n)


def run_plane(lengths, B, seed):
    """A plane whose filtered stream holds, for every L of `lengths`, a run of L ending at a block boundary, one starting at it (both at one
    boundary) and one lying across the next boundary, in a background without repeats."""
    nbound = 2 * len(lengths)
    spots = []
    for i, L in enumerate(lengths):
        k = (2 * i + 1) * B
        spots += [(k - L, L, 251), (k, L, 252), (k + B - L // 2, L, 253)]
    for w in range(12000, 16383):                                         # the first width that keeps every filter byte out of the runs
        if all((a - 1) // (1 + w) == (a + L) // (1 + w) and (a - 1) % (1 + w) for a, L, _ in spots):
            break
    h = -(-((nbound + 1) * B) // (1 + w))
    f = _no_repeat(h * (1 + w), seed).reshape(h, 1 + w)
    f[:, 0] = 1
    f = f.reshape(-1)
    rows = set(range(0, f.size, 1 + w))

    def put(a, L, v):
        assert not rows & set(range(a - 1, a + L + 1)), 'a run over a filter byte'
        f[a:a + L] = v
        for e in (a - 1, a + L):
            if f[e] == v:
                f[e] = v + 1
    for a, L, v in spots:
        put(a, L, v)
    return plane_from_filtered(f, h, w)


def interleave(symbols, counts, first_not):
    """A sequence with counts[i] of symbols[i], no two equal neighbours, not starting with `first_not`."""
    order = sorted(range(len(symbols)), key=lambda i: -counts[i])
    flat = np.concatenate([np.full(counts[i], symbols[i], np.int64) for i in order])
    n = flat.size
    assert max(counts) <= (n + 1) // 2
    out = np.empty(n, np.int64)
    ne = (n + 1) // 2
    out[0::2] = flat[:ne]
    out[1::2] = flat[ne:]
    assert (out[1:] != out[:-1]).all() and out[0] != first_not
    return out.astype(np.uint8)


def fib_plane():
    """One row whose symbol counts are the Fibonacci numbers: the filter byte and the end-of-block are F1 and F2 (one each), the bytes 10, 12, .. 42
    take F3..F19 as literals (10 943 bytes, inside one block). The unlimited tree is 18 deep."""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    body = interleave([10 + 2 * i for i in range(17)], fib[2:], 1)
    return plane_from_filtered(np.concatenate([[1], body]), 1, body.size)


# {code length: how many literal/length symbols take it}: a dyadic histogram (count 2^(10 - length)), the symbols two apart so that the length
# list alternates with zeros. The code-length alphabet then sees these counts plus the zeros over 11 symbols: its unlimited tree is 8 deep.
CL_SKEW_MULT = {2: 1, 3: 1, 4: 1, 5: 13, 7: 8, 8: 1, 9: 21, 10: 50}


def cl_skew_plane(mult):
    """`mult`: {length: symbols of that length}, Kraft-complete together with the filter byte (01) and the end-of-block, both of the greatest
    length. One row."""
    L = max(mult)
    syms, counts, s = [], [], 4
    for l in sorted(mult):
        k = mult[l] - (2 if l == L else 0)
        for _ in range(k):
            syms.append(s)
            counts.append(1 << (L - l))
            s += 2
    assert s <= 256
    body = interleave(syms, counts, 1)
    return plane_from_filtered(np.concatenate([[1], body]), 1, body.size)


def cases(B=BLOCK):
    """name -> uint8 plane: the smallest shapes at which each mechanism can first go wrong."""
    rng = np.random.RandomState(7)
    c = {}
    for i, (h, w) in enumerate([(1, 1), (1, 70), (65, 3), (64, 64), (130, 67), (3, 16383)]):
        c['mixed_%dx%d' % (h, w)] = _mixed(h, w, 100 + i)
    for tag, n in [('Bm1', B - 1), ('B', B), ('Bp1', B + 1), ('2Bp1', 2 * B + 1)]:
        h, w = _exact(n)
        c['stream_' + tag] = _mixed(h, w, 200 + len(tag))
    c['runs_1_5'] = run_plane([1, 2, 3, 4, 5], B, 1)
    c['runs_258_263'] = run_plane([258, 259, 260, 261, 262, 263], B, 2)
    c['runs_516_521'] = run_plane([516, 517, 518, 519, 520, 521], B, 3)
    c['zeros_512'] = np.zeros((512, 512), np.uint8)
    c['ones_512'] = np.full((512, 512), 255, np.uint8)
    c['noise_64'] = rng.randint(0, 256, (64, 64)).astype(np.uint8)
    e = soft_ellipse(96, 160)
    c['ellipse'] = to_bytes(e, 'unit')
    c['ellipse_bin'] = to_bytes(e, 'threshold')
    c['fib_literals'] = fib_plane()
    c['fib_code_lengths'] = cl_skew_plane(CL_SKEW_MULT)
    c['one_pixel'] = np.array([[200]], np.uint8)
    return c



# ---- the planes of the size table ---------------------------------------------------------------------------------------------
SIZE_TABLE = ('soft ellipse 512x512', 'soft ellipse 1080x1920', 'binary 512x512', 'all-zero 512x512', 'noise 256x256', 'noisy matte 512x512')


def size_table_plane(name):
    rng = np.random.RandomState(0)
    e = soft_ellipse(1080, 1920) if '1080' in name else soft_ellipse(512, 512)
    if name.startswith('soft'):
        return to_bytes(e, 'unit')
    if name.startswith('binary'):
        return to_bytes(e, 'threshold')
    if name.startswith('all-zero'):
        return np.zeros((512, 512), np.uint8)
    if name.startswith('noise'):
        return rng.randint(0, 256, (256, 256)).astype(np.uint8)
    return np.clip(to_bytes(e, 'unit').astype(int) + rng.randint(-3, 4, (512, 512)), 0, 255).astype(np.uint8)
