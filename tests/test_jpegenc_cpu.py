"""JPEG encoding without a GPU: the restatement (tests/jpegenc_restatement.py) against live Pillow, the whole file on every case; its
coefficients against the decoder's restatement reading Pillow's file; the host half of `maggie_amd.utils.jpegenc` (the header, the argument
checks); the C entries' argument errors; the pinned fixture; the capacity bound; the coverage the case list claims; and the kernel source
itself, compiled for the host with the address and undefined-behaviour sanitizers (tests/csrc/jpegenc_host.cpp), equal to the restatement
stage by stage. Every comparison is exact equality."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
sys.path.insert(0, ROOT)

import jpegdec_restatement as D                              # noqa: E402
import jpegenc_restatement as R                              # noqa: E402
import make_jpegenc_golden as G                              # noqa: E402
from helpers import load_golden                              # noqa: E402
from maggie_amd.utils import jpegdec, jpegenc, photometric   # noqa: E402

NAMES = list(R.CASES)
HEADER_QUALITIES = (1, 20, 21, 49, 50, 51, 75, 80, 81, 100)


@pytest.fixture(scope='module')
def restated():
    """name -> (frame, quality, coefficients, (unstuffed, stuffed), file): computed once, shared, never changed."""
    out = {}
    for name, (h, w, kind, q, seed) in R.CASES.items():
        x = R.image(h, w, kind, seed)
        coef = R.coefficients(x, q)
        sc = R.scan(coef)
        out[name] = (x, q, coef, sc, R.header(h, w, q) + sc[1] + b'\xff\xd9')
    return out


def test_the_case_list_is_the_issue_s():
    assert len(NAMES) == len(R.P.SHAPES) * len(R.QUALITIES) * len(R.P.KINDS) + 3 * len(R.QUALITIES)
    assert R.QUALITIES == (1, 21, 50, 75, 80, 100) and R.CRAFTED == ('blocks', 'checker', 'columns')
    b, c, k = (R.crafted(n) for n in R.CRAFTED)
    assert b.shape == c.shape == k.shape == (48, 48, 3)
    blocks = b.reshape(6, 8, 6, 8, 3)
    assert set(np.unique(b)) == {0, 255} and (blocks == blocks[:, :1, :, :1]).all()
    assert (c[1:] != c[:-1]).all() and (c[:, 1:] != c[:, :-1]).all()
    assert (k[1:] == k[:-1]).all() and (k[:, 1:] != k[:, :-1]).all()


def test_restatement_equals_pillow_on_every_case(restated):
    for name, (x, q, _, _, mine) in restated.items():
        assert mine == R.pillow(x, q), name
        assert mine == R.file_bytes(x, q), name


def test_coefficients_equal_the_decoder_s_reading_of_pillow_s_file(restated):
    for name in NAMES[::3] + NAMES[-18:]:
        x, q, coef, _, _ = restated[name]
        assert np.array_equal(coef, D.coefficients(R.pillow(x, q))), name


def test_dummy_blocks_are_what_makes_the_odd_sizes_equal():
    """Transforming replicated pixels instead of writing dummy blocks changes exactly the sizes with an odd ceil(w / 8) or ceil(h / 8)."""
    for (h, w), differs in (((2, 2), True), ((8, 8), True), ((9, 4), True), ((17, 23), True), ((33, 65), True), ((37, 53), True),
                            ((1, 1), False), ((16, 16), False), ((31, 63), False), ((64, 48), False)):
        x = R.image(h, w, 'random', R.P.seed_of(h, w, 50, 'random'))
        mx, my, bw, bh = R.geometry(h, w)
        assert not differs or (bw & 1) or (bh & 1)              # 1 x 1 has dummies too, but a flat MCU's replicated blocks equal them
        t = R.tables_of(50)
        Y = R.P.pad_rows(R.P.pad_cols(R.P.rgb_to_ycc(x)[0], 16 * mx), 16 * my)
        padded = R.plane_coefficients(Y, t[0]).reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, 4, 64)
        luma = R.coefficients(x, 50).reshape(my * mx, 6, 64)[:, :4]
        assert np.array_equal(padded, luma) != differs, (h, w)


def test_tables_in_natural_order_and_the_extreme_tables():
    x = R.image(17, 23, 'random', 5)
    t = np.stack([np.arange(1, 65), np.arange(64, 0, -1)]).astype(np.int32)
    for table in (t, np.full((2, 64), 1, np.int32), np.full((2, 64), 255, np.int32)):
        data = R.pillow(x, table)
        assert R.file_bytes(x, table) == data
        assert np.array_equal(jpegdec.parse(data).qtables[:2], table)
        assert jpegenc.header(17, 23, table) == data[:623]


@pytest.mark.parametrize('q', HEADER_QUALITIES)
def test_header_equals_pillow_s(q):
    for h, w in ((1, 1), (37, 53), (300, 517)):
        data = R.pillow(np.zeros((h, w, 3), np.uint8), q)
        head = jpegenc.header(h, w, photometric.quant_tables(q))
        assert len(head) == 623 and data[:623] == head and R.header(h, w, q) == head, (q, h, w)
        plan = jpegdec.parse(data)
        assert plan.offset == 623 and (plan.height, plan.width, plan.layout) == (h, w, jpegdec.L420)


def test_block_bits_and_both_streams_agree(restated):
    for name, (x, q, coef, (raw, stuffed), data) in restated.items():
        bits = R.block_bits(coef)
        assert len(bits) == jpegenc.blocks_of(*x.shape[:2]) and len(raw) == (int(bits.sum()) + 7) // 8, name
        assert len(stuffed) == len(raw) + raw.count(b'\xff') and stuffed.replace(b'\xff\x00', b'\xff') == raw, name
        pad = -int(bits.sum()) % 8
        assert raw[-1] & ((1 << pad) - 1) == (1 << pad) - 1, name
        assert data[623:-2] == stuffed and data[-2:] == b'\xff\xd9', name


def test_capacity_bound(restated):
    """A block is at most 20 + 63 x 26 = 1658 bits, derived from the tables: a symbol with run r takes r + 1 of the 63 AC positions (a ZRL 16), so
    the most bits per position decide. With run 0 that is max over the category n of len(0x0n) + n: 26 for luma (K.5's 0x0A is a 16-bit
    code), 22 for chroma (K.6's is 12 bits). With a run it is at most (16 + 10) / 2 = 13, and a ZRL gives 11 / 16: both less, so 63 run-0 terms
    of the costliest category are the worst block. The DC term adds at most 9 + 11 (luma) or 11 + 11 (chroma). Stuffing at most doubles the
    bytes; the shortest block is 4 bits (chroma: DC category 0, then EOB)."""
    dc = [max(l + s for s, (_, l) in R.CODES[t].items()) for t in (0, 2)]
    assert dc == [20, 22]
    worst = []
    for k, t in enumerate((1, 3)):
        run0 = max(R.CODES[t][n][1] + n for n in range(1, 11))
        longer = max((l + (s & 15)) / ((s >> 4) + 1) for s, (_, l) in R.CODES[t].items() if s >> 4 and s & 15)
        assert longer <= 13 < run0 and R.CODES[t][0xF0][1] / 16 < 1
        worst.append(dc[k] + 63 * run0)
    assert worst == [20 + 63 * 26, 22 + 63 * 22]
    assert max(worst) == R.MAX_BLOCK_BITS == jpegenc.MAX_BLOCK_BITS == 1658
    shortest = min(R.CODES[t][0][1] for t in (0, 2)) + min(R.CODES[t][0][1] for t in (1, 3))
    assert shortest == 4
    for name, (x, q, coef, (raw, stuffed), _) in restated.items():
        assert R.block_bits(coef).max() <= R.MAX_BLOCK_BITS and R.block_bits(coef).min() >= shortest, name
        assert len(stuffed) <= 2 * len(raw) and len(raw) + 4 <= jpegenc.raw_stride(*x.shape[:2]), name


def test_the_list_covers_every_event(restated):
    total = dict(zrl=0, no_eob=0, ac10=0, dc11=0, stuffed=0, aligned=0)
    for name, (x, q, coef, (raw, stuffed), _) in restated.items():
        for k, v in R.events(coef).items():
            total[k] += int(v)
        total['stuffed'] += len(stuffed) - len(raw)
        total['aligned'] += int(R.block_bits(coef).sum()) % 8 == 0
    print(total)
    assert all(v >= 1 for v in total.values()), total
    # the inputs the issue names
    x, q, coef, (raw, stuffed), _ = restated['37x53_random_q50']
    assert R.events(coef)['zrl'] >= 1
    for name in ('48x48_checker_q100', '48x48_columns_q100'):
        assert R.events(restated[name][2])['ac10'] >= 1, name
    assert R.events(restated['48x48_blocks_q100'][2])['dc11'] >= 1
    assert R.events(restated['48x48_checker_q100'][2])['no_eob'] >= 1
    for name in ('48x48_blocks_q100', '48x48_checker_q100'):
        assert len(restated[name][3][1]) - len(restated[name][3][0]) >= 1, name


def test_constants_are_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    for name, v in (('THREADS', jpegenc.THREADS), ('PACK_BLOCKS', jpegenc.PACK_BLOCKS), ('CHUNK_BYTES', jpegenc.CHUNK_BYTES),
                    ('MAX_BLOCK_BITS', jpegenc.MAX_BLOCK_BITS), ('MAX_FRAMES', jpegenc.MAX_FRAMES)):
        assert '#define MG_JPEGENC_%s %d' % (name, v) in text, name
    assert jpegenc.MAX_SIDE == photometric.MAX_SIDE == 32767 and np.array_equal(jpegenc.ZIGZAG, R.ZIGZAG)
    assert jpegenc.blocks_of(1, 1) == 6 and jpegenc.blocks_of(17, 33) == 2 * 3 * 6 and jpegenc.raw_stride(1, 1) % 16 == 0


@pytest.mark.parametrize('name', list(G.pinned_cases()))
def test_fixture_key_by_key(name):
    d = load_golden('jpegenc_pinned.npz')
    x, q = G.pinned_cases()[name]
    assert np.array_equal(d[name + '.frame'], x) and np.array_equal(d[name + '.quality'], np.asarray(q, np.int32))
    q = int(d[name + '.quality']) if d[name + '.quality'].ndim == 0 else d[name + '.quality']
    data = d[name + '.file'].tobytes()
    assert R.file_bytes(d[name + '.frame'], q) == data
    if str(d['versions']) == G.versions():
        assert R.pillow(d[name + '.frame'], q) == data
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), D.decode(data))


def test_fixture_records_the_versions():
    v = str(load_golden('jpegenc_pinned.npz')['versions'])
    assert v.startswith('Pillow ') and 'libjpeg_turbo' in v and 'jpg' in v


def test_argument_errors_come_before_any_launch():
    ok = np.zeros((2, 8, 8, 3), np.uint8)
    for bad, exc in ((np.zeros((2, 8, 8, 3), np.float32), TypeError), (np.zeros((2, 8, 8, 3), np.int16), TypeError), ([[0]], TypeError),
                     (np.zeros((8, 8, 3), np.uint8), ValueError), (np.zeros((2, 2, 8, 8, 3), np.uint8), ValueError),
                     (np.zeros((2, 8, 8, 4), np.uint8), ValueError), (np.zeros((0, 8, 8, 3), np.uint8), ValueError),
                     (np.zeros((1, 0, 8, 3), np.uint8), ValueError), (np.zeros((1, 1, 32768, 3), np.uint8), ValueError)):
        with pytest.raises(exc):
            jpegenc.encode_clip(bad)
    for q, exc in ((0, ValueError), (101, ValueError), (75.0, TypeError), (True, TypeError), (np.zeros((2, 64), np.int64), ValueError),
                   (np.zeros((3, 64), np.int32), ValueError), (torch.zeros((2, 64), dtype=torch.float32), ValueError)):
        with pytest.raises(exc):
            jpegenc.encode_clip(ok, q)
        with pytest.raises(exc):
            jpegenc.encode(ok[0], q)
    with pytest.raises(ValueError):
        jpegenc.encode(ok)
    with pytest.raises(ValueError):
        jpegenc.encode(ok[0], lut=np.zeros((3, 255), np.uint8))
    with pytest.raises(ValueError):
        jpegenc.encode(ok[0], noise=np.zeros((8, 9, 1), np.int16))
    with pytest.raises(ValueError):
        jpegenc.encode(ok[0], noise=np.zeros((8, 8, 1), np.int32))
    with pytest.raises(ValueError):
        jpegenc.header(0, 8, photometric.quant_tables(75))
    with pytest.raises(ValueError):
        jpegenc.header(8, 8, np.zeros((2, 64), np.int32))


def test_no_cpu_fallback():
    from maggie_amd.hip import MaggieHipError
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(MaggieHipError):
        jpegenc.encode(np.zeros((8, 8, 3), np.uint8))


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_jpegenc_limits, lib.mg_jpegenc_coef, lib.mg_jpegenc_bits, lib.mg_jpegenc_pack, lib.mg_jpegenc_stuff):
        fn.restype = ctypes.c_int
    v = [ctypes.c_int() for _ in range(6)]
    assert lib.mg_jpegenc_limits(*[ctypes.byref(x) for x in v]) == 0 and lib.mg_jpegenc_limits(None, None, None, None, None, None) == -2
    assert [x.value for x in v] == [jpegenc.THREADS, jpegenc.PACK_BLOCKS, jpegenc.CHUNK_BYTES, jpegenc.MAX_BLOCK_BITS, jpegenc.MAX_SIDE,
                                    jpegenc.MAX_FRAMES]
    buf = (ctypes.c_uint8 * 4096)()
    base = ctypes.addressof(buf)
    a = ctypes.c_void_p((base + 63) // 64 * 64)                        # 64-byte aligned
    odd, off8 = ctypes.c_void_p(a.value + 1), ctypes.c_void_p(a.value + 8)
    stride = jpegenc.raw_stride(16, 16)

    def coef(n=1, h=16, w=16, elems=6 * 64, src=a, q=a, out=a, noise=None, nc=1):
        return lib.mg_jpegenc_coef(src, None, noise, I(nc), q, out, L(elems), L(n), I(h), I(w), None)

    def bits(n=1, h=16, w=16, elems=6 * 64, c=a, b=a, o=a, s=a):
        return lib.mg_jpegenc_bits(c, L(elems), b, o, s, L(n), I(h), I(w), None)

    def pack(n=1, h=16, w=16, elems=6 * 64, c=a, b=a, o=a, s=a, raw=a, st=stride, ff=a, ch=a):
        return lib.mg_jpegenc_pack(c, L(elems), b, o, s, raw, L(st), ff, ch, L(n), I(h), I(w), None)

    def stuff(n=1, h=16, w=16, raw=a, st=stride, ch=a, s=a, out=a, ob=64, gc=1):
        return lib.mg_jpegenc_stuff(raw, L(st), ch, s, out, L(ob), L(n), I(h), I(w), L(gc), None)
    for bad in (dict(n=0), dict(n=-1), dict(n=jpegenc.MAX_FRAMES + 1), dict(h=0), dict(w=0), dict(h=32768), dict(w=32768)):
        assert coef(**bad) == bits(**bad) == pack(**bad) == stuff(**bad) == -2, bad
    for bad in (dict(elems=6 * 64 - 1), dict(elems=6 * 64 + 64), dict(elems=0)):
        assert coef(**bad) == bits(**bad) == pack(**bad) == -2, bad
    assert coef(src=None) == coef(q=None) == coef(out=None) == coef(out=off8) == coef(q=odd) == coef(noise=a, nc=2) == -2
    assert bits(c=None) == bits(b=None) == bits(o=None) == bits(s=None) == bits(c=odd) == bits(b=odd) == bits(o=odd) == bits(s=odd) == -2
    assert pack(c=None) == pack(raw=None) == pack(ff=None) == pack(ch=None) == pack(raw=off8) == pack(ff=odd) == pack(ch=odd) == -2
    assert pack(st=stride - 16) == pack(st=stride + 8) == pack(st=0) == -2
    assert stuff(raw=None) == stuff(ch=None) == stuff(s=None) == stuff(out=None) == stuff(raw=off8) == stuff(ch=odd) == stuff(s=odd) == -2
    assert stuff(st=stride - 16) == stuff(ob=0) == stuff(gc=0) == stuff(gc=2) == -2
    # more workgroups than a launch takes: the largest frame at the largest frame count, refused before any launch
    n, side = jpegenc.MAX_FRAMES, jpegenc.MAX_SIDE
    big, elems = jpegenc.raw_stride(side, side), n * jpegenc.blocks_of(side, side) * 64
    assert coef(n=n, h=side, w=side, elems=elems) == pack(n=n, h=side, w=side, elems=elems, st=big) == -3
    assert stuff(n=n, h=side, w=side, st=big, gc=-(-big // jpegenc.CHUNK_BYTES)) == -3


# ---- the kernel source on the host, under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
    assert cxx is not None, 'no host C++ compiler (g++, c++, clang++): the sanitizer run of the kernel source is the only bounds evidence without a GPU, so it does not skip'
    exe = str(tmp_path_factory.mktemp('jpegenc_host') / 'jpegenc_host')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'jpegenc_host.cpp')])
    return exe


def run_host(exe, tmp_path, tag, calls):
    """calls: [(frames (T, h, w, 3), table (2, 64), lut or None, noise or None)] -> [(rcs, sizes (4, T), coef, bits, offs, raw (T, stride), out bytes)]"""
    body = []
    for frames, table, lut, noise in calls:
        T, h, w, _ = frames.shape
        body.append(struct.pack('<5i', h, w, T, 0 if noise is None else noise.shape[-1], int(lut is not None)) +
                    np.ascontiguousarray(table, np.int32).tobytes() + np.ascontiguousarray(frames).tobytes() +
                    (b'' if lut is None else np.ascontiguousarray(lut, np.uint8).tobytes()) +
                    (b'' if noise is None else np.ascontiguousarray(noise, np.int16).tobytes()))
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(calls)) + b''.join(body))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'jpegenc_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, buf, p = [], open(dst, 'rb').read(), 0
    for frames, _, _, _ in calls:
        T = frames.shape[0]
        rcs = struct.unpack_from('<4i', buf, p)
        nb, stride, total = struct.unpack_from('<3q', buf, p + 16)
        p += 40
        parts = []
        for dtype, n in ((np.int64, 4 * T), (np.int16, T * nb * 64), (np.int32, T * nb), (np.int64, T * nb), (np.uint8, T * stride)):
            parts.append(np.frombuffer(buf, dtype, n, p))
            p += parts[-1].nbytes
        out.append((rcs, parts[0].reshape(4, T), parts[1].reshape(T, nb, 64), parts[2].reshape(T, nb), parts[3].reshape(T, nb),
                    parts[4].reshape(T, stride), buf[p:p + total]))
        p += total
    assert p == len(buf)
    return out


def check_host(got, frames, q, tag):
    rcs, sizes, coef, bits, offs, raw, blob = got
    assert rcs == (0, 0, 0, 0), tag
    assert raw.shape[1] == jpegenc.raw_stride(*frames.shape[1:3]), tag
    at = 0
    for t, x in enumerate(frames):
        want = R.coefficients(x, q)
        unstuffed, stuffed = R.scan(want)
        wb = R.block_bits(want)
        assert np.array_equal(coef[t], want), (tag, t, 'coefficients')
        assert np.array_equal(bits[t], wb) and np.array_equal(offs[t], np.cumsum(wb) - wb), (tag, t, 'bits')
        assert sizes[:, t].tolist() == [len(stuffed) + 2, len(unstuffed), int(wb.sum()), at], (tag, t, 'sizes')
        assert raw[t, :len(unstuffed)].tobytes() == unstuffed and not raw[t, len(unstuffed):].any(), (tag, t, 'unstuffed stream')
        assert blob[at:at + len(stuffed) + 2] == stuffed + b'\xff\xd9', (tag, t, 'scan')
        at += len(stuffed) + 2
    assert at == len(blob), tag


HOST_CASES = ['1x1_random_q75', '2x2_binary_q100', '8x8_random_q50', '9x4_smooth_q21', '17x23_random_q100', '16x16_binary_q1', '37x53_random_q50',
              '33x65_binary_q80', '48x48_checker_q100', '48x48_blocks_q100']


def test_kernel_source_on_the_host_equals_the_restatement(host_exe, tmp_path, restated):
    calls = [(restated[n][0][None], R.tables_of(restated[n][1]), None, None) for n in HOST_CASES]
    for n, c, g in zip(HOST_CASES, calls, run_host(host_exe, tmp_path, 'list', calls)):
        check_host(g, c[0], restated[n][1], n)


def test_kernel_source_on_the_host_clips_operands_and_boundaries(host_exe, tmp_path):
    """A clip of three frames; the tone curve and the noise; both extreme tables; and a stream of three packing workgroups and four stuffing
    chunks (64 x 128 uniform at quality 100), alone and behind another frame."""
    rs = np.random.RandomState(3)
    clip = np.stack([R.P.inputs(17, 23, k, 9) for k in R.P.KINDS])
    x = R.P.inputs(37, 53, 'smooth', 3)
    lut = np.stack([np.clip((np.arange(256) / 255.0) ** g * 255 + 0.5, 0, 255) for g in (0.7, 1.0, 1.4)]).astype(np.uint8)
    noise = {nc: rs.randint(-40, 41, (37, 53, nc)).astype(np.int16) for nc in (1, 3)}
    big = R.P.inputs(64, 128, 'random', 6528)
    two = np.stack([big[::-1], big])
    ones, most = np.full((2, 64), 1, np.int64), np.full((2, 64), 255, np.int64)
    calls = [(clip, R.tables_of(50), None, None), (x[None], R.tables_of(75), lut, noise[1]), (x[None], R.tables_of(75), None, noise[3]),
             (x[None], R.tables_of(75), lut, None), (clip, ones, None, None), (clip, most, None, None), (big[None], R.tables_of(100), None, None),
             (two, R.tables_of(100), None, None)]
    got = run_host(host_exe, tmp_path, 'more', calls)
    check_host(got[0], clip, 50, 'clip')
    check_host(got[1], R.P.add_noise(R.P.apply_lut(x, lut), noise[1])[None], 75, 'lut and noise')
    check_host(got[2], R.P.add_noise(x, noise[3])[None], 75, 'noise of three channels')
    check_host(got[3], R.P.apply_lut(x, lut)[None], 75, 'lut')
    check_host(got[4], clip, ones, 'table of ones')
    check_host(got[5], clip, most, 'table of 255')
    check_host(got[6], big[None], 100, 'three packing workgroups')
    check_host(got[7], two, 100, 'clip of two large frames')
    offs, raw_bytes = got[6][4][0], int(got[6][1][1, 0])
    assert len(offs) > 2 * jpegenc.PACK_BLOCKS and raw_bytes > 2 * jpegenc.CHUNK_BYTES
    assert (offs[jpegenc.PACK_BLOCKS::jpegenc.PACK_BLOCKS] % 32 != 0).any()                    # a word shared by two packing workgroups
