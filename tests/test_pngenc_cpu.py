"""PNG encoding without a GPU: the restatement (tests/pngenc_restatement.py) read back by Pillow, zlib, `pngdec.parse` and the decoder's own
restatement; its size against zlib's level-1 Z_RLE configuration; the float conversions against NumPy; the host half of
`maggie_amd.utils.pngenc` (framing, the path rule of `save_visualization` against the pinned fixture); and the kernel source itself, compiled
for the host with the address and undefined-behaviour sanitizers (tests/csrc/pngenc_host.cpp), byte-equal to the restatement on the case list."""
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pngdec_restatement as D                              # noqa: E402
import pngenc_restatement as R                              # noqa: E402
from maggie_amd.utils import pngdec, pngenc                 # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pngenc_pinned.npz')
B = R.BLOCK


@pytest.fixture(scope='module')
def cases():
    return R.cases(B)


@pytest.fixture(scope='module')
def restated(cases):
    """name -> (file, [Block]): computed once, shared, never changed."""
    return {name: R.encode(p, B) for name, p in cases.items()}


def test_constants_are_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    for name, v in (('BLOCK_BYTES', R.BLOCK), ('REC_WORDS', R.REC_WORDS), ('THREADS', pngenc.THREADS), ('MAX_SIDE', pngenc.MAX_SIDE),
                    ('MAX_WIDTH', pngenc.MAX_WIDTH), ('MAX_PLANES', pngenc.MAX_PLANES)):
        assert '#define MG_PNGENC_%s %d' % (name, v) in text, name
    assert (pngenc.BLOCK_BYTES, pngenc.REC_WORDS) == (R.BLOCK, R.REC_WORDS)
    assert pngenc.MAX_SIDE == pngdec.MAX_SIDE and pngenc.MAX_WIDTH == pngdec.MAX_ROWBYTES      # the device decoder reads back what this writes


def test_the_list_holds_what_it_claims(cases, restated):
    assert [cases[n].shape for n in list(cases)[:6]] == [(1, 1), (1, 70), (65, 3), (64, 64), (130, 67), (3, 16383)]
    for tag, n in (('Bm1', B - 1), ('B', B), ('Bp1', B + 1), ('2Bp1', 2 * B + 1)):
        assert R.filtered(cases['stream_' + tag]).size == n
    for name, lengths in (('runs_1_5', range(1, 6)), ('runs_258_263', range(258, 264)), ('runs_516_521', range(516, 522))):
        f = R.filtered(cases[name])
        for i, L in enumerate(lengths):
            k = (2 * i + 1) * B
            for a, v in ((k - L, 251), (k, 252), (k + B - L // 2, 253)):                      # at a block's end, its start, across a boundary
                assert (f[a:a + L] == v).all() and f[a - 1] != v and f[a + L] != v, (name, L)
    assert cases['zeros_512'].shape == (512, 512) and not cases['zeros_512'].any() and (cases['ones_512'] == 255).all()
    assert set(np.unique(cases['ellipse_bin'])) == {0, 255} and len(np.unique(cases['ellipse'])) > 50
    # the two skewed cases really exceed the limits, and the limited lengths are what was emitted
    lit = restated['fib_literals'][1][0]
    assert max(R.unlimited_lengths(lit.hist.tolist())) > 15 and max(lit.lens) == 15 and lit.type == 2
    assert sum(1 for c in lit.hist[:256] if c) >= 17
    cl = restated['fib_code_lengths'][1][0]
    assert max(R.unlimited_lengths(cl.cl_hist)) > 7 and max(cl.cl_lens) == 7 and cl.type == 2 and sum(1 for c in cl.cl_hist if c) >= 9
    one = restated['one_pixel'][1]
    assert len(one) == 1 and one[0].type == 1                                                   # the fixed form must win
    types = {b.type for _, bl in restated.values() for b in bl}
    assert types == {1, 2}
    kinds = set()
    for name in ('runs_258_263', 'runs_516_521', 'mixed_130x67'):
        f = R.filtered(cases[name])
        for k in range(0, f.size, B):
            kinds |= set(R.tokens(f[k:k + B])[1].tolist())
    assert {1, 3, 4, 257, 258} <= kinds


def test_tokens_by_position_equal_the_definition(cases):
    for name in ('mixed_130x67', 'runs_1_5', 'runs_258_263', 'runs_516_521', 'ellipse_bin', 'zeros_512'):
        f = R.filtered(cases[name])
        for k in range(0, min(f.size, 6 * B), B):
            a, b = R.tokens(f[k:k + B]), R.tokens_slow(f[k:k + B])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, k)
            n = np.where(a[1] == 1, 1, a[1])                                                 # the tokens tile the block
            assert np.array_equal(a[0], np.cumsum(n) - n) and n.sum() == f[k:k + B].size, (name, k)


def test_every_reader_returns_the_plane(cases, restated):
    for name, p in cases.items():
        f, blocks = restated[name]
        im = Image.open(io.BytesIO(f))
        assert im.mode == 'L' and np.array_equal(np.asarray(im), p), name
        assert zlib.decompress(R.idat(f)) == R.filtered(p).tobytes(), name
        plan = pngdec.parse(f)
        assert (plan.height, plan.width, plan.color_type, plan.depth, plan.idat_chunks) == (p.shape[0], p.shape[1], 0, 8, 1), name
        assert np.array_equal(D.decode(f), p), name


def test_fixed_form_is_never_smaller_and_sizes_against_zlib(cases, restated):
    for name, p in cases.items():
        f, blocks = restated[name]
        stream = R.idat(f)
        for b in blocks:
            assert b.bits == min(b.fixed_bits, b.dynamic_bits) and (b.type == 2) == (b.dynamic_bits < b.fixed_bits), name
            assert b.bits <= 9 * b.nbytes + 10, name                                            # the capacity bound
        assert len(stream) == 2 + (sum(b.bits for b in blocks) + 7) // 8 + 4, name
        assert len(stream) <= R.all_fixed_bytes(blocks), name
        z = len(R.zlib_rle(R.filtered(p)))
        print('%-18s %7d bytes, zlib Z_RLE level 1 %7d, ratio %.3f, %d blocks' % (name, len(stream), z, len(stream) / z, len(blocks)))
        assert len(stream) <= 1.02 * z + 32 * len(blocks), (name, len(stream), z, len(blocks))


@pytest.mark.parametrize('name', list(R.SIZE_TABLE))
def test_size_table_of_the_design_document(name):
    """The planes of DESIGN.md section 27's size table at both block sizes: the bar, and the figures the table quotes (printed)."""
    p = R.size_table_plane(name)
    f = R.filtered(p)
    z = len(R.zlib_rle(f))
    for blk in (16384, 32768):
        stream, blocks = R.encode_stream(f, blk)
        print('%-24s B = %5d: %7d bytes, zlib Z_RLE level 1 %7d, ratio %.3f, %d blocks' % (name, blk, len(stream), z, len(stream) / z, len(blocks)))
        assert zlib.decompress(stream) == f.tobytes()
        assert len(stream) <= 1.02 * z + 32 * len(blocks), (name, blk, len(stream), z, len(blocks))
        assert len(stream) <= R.all_fixed_bytes(blocks), (name, blk)


def test_float_modes_at_the_byte_edges():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))]).astype(np.float32)
    x = x[(x >= 0) & (x <= 1)]
    assert np.array_equal(R.to_bytes(x, 'unit'), (x * 255).astype('uint8'))
    h = np.float32(0.5)
    y = np.concatenate([x, [np.nextafter(h, np.float32(0)), h, np.nextafter(h, np.float32(1))]]).astype(np.float32)
    assert np.array_equal(R.to_bytes(y, 'threshold'), (y > 0.5).astype('uint8') * 255)
    odd = np.array([np.nan, -1.0, -0.0, 1.5, np.inf, -np.inf, 1.0], np.float32)
    assert R.to_bytes(odd, 'unit').tolist() == [0, 0, 0, 255, 255, 0, 255]
    assert R.to_bytes(odd, 'threshold').tolist() == [0, 0, 0, 255, 255, 0, 255]


def test_host_framing_and_argument_checks(cases, restated):
    for name in ('mixed_130x67', 'one_pixel'):
        f = restated[name][0]
        assert pngenc.frame(cases[name].shape[0], cases[name].shape[1], R.idat(f)) == f
    with pytest.raises(TypeError):
        pngenc.encode_planes(np.zeros((2, 4, 4), np.float64), mode='unit')
    with pytest.raises(TypeError):
        pngenc.encode_planes(np.zeros((2, 4, 4), np.float32), mode='u8')
    with pytest.raises(TypeError):
        pngenc.encode_planes(np.zeros((2, 4, 4), np.uint8), mode='threshold')
    with pytest.raises(ValueError):
        pngenc.encode_planes(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        pngenc.encode_planes(np.zeros((1, 2, 16385), np.uint8))
    with pytest.raises(ValueError):
        pngenc.encode_planes(np.zeros((0, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        pngenc.encode_planes(np.zeros((1, 2, 2), np.uint8), mode='rgb')


def test_paths_are_the_reference_s():
    z = np.load(GOLDEN)
    for tag in ('named', 'numbered', 'single'):
        want = sorted(str(s) for s in z[tag + '.paths'])
        names = [[str(s)] for s in z[tag + '.image_names']]
        alpha_names = [[str(s)] for s in z[tag + '.alpha_names']] if (tag + '.alpha_names') in z.files else None
        n_i = z[tag + '.alphas'].shape[2]
        has_diff, has_inc = (tag + '.diff_pred') in z.files, (tag + '.inc_bin_maps') in z.files
        plan = pngenc.plan_paths(names, alpha_names, n_i, has_diff, has_inc)
        got = sorted(p for _, _, p in plan)
        assert got == sorted(set(want)), tag


# ---- the kernel source on the host, under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
    assert cxx is not None, 'no host C++ compiler (g++, c++, clang++): the sanitizer run of the kernel source is the only bounds evidence, so it does not skip'
    exe = str(tmp_path_factory.mktemp('pngenc_host') / 'pngenc_host')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'pngenc_host.cpp')])
    return exe


MODES = {'u8': 0, 'unit': 1, 'threshold': 2}


def run_host(exe, tmp_path, tag, calls):
    """calls: [(planes array (P, h, w), mode)] -> [(rc_size, rc_emit, sizes, recs (P, blocks, REC_WORDS), blob)]"""
    body = []
    for planes, mode in calls:
        P, h, w = planes.shape
        body.append(struct.pack('<4i', h, w, P, MODES[mode]) + np.ascontiguousarray(planes).tobytes())
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(calls)) + b''.join(body))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'pngenc_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, buf, p = [], open(dst, 'rb').read(), 0
    for planes, _ in calls:
        P = planes.shape[0]
        rc1, rc2, nb, total = struct.unpack_from('<4i', buf, p)
        p += 16
        sizes = np.frombuffer(buf, np.int64, P, p)
        p += 8 * P
        recs = np.frombuffer(buf, np.int32, P * nb * R.REC_WORDS, p).reshape(P, nb, R.REC_WORDS)
        p += recs.nbytes
        out.append((rc1, rc2, sizes, recs, buf[p:p + total]))
        p += total
    assert p == len(buf)
    return out


def check_call(got, planes, mode, want):
    """`want`: [(file, [Block])] per plane"""
    rc1, rc2, sizes, recs, blob = got
    assert rc1 == 0 and rc2 == 0
    at = 0
    for k, (f, blocks) in enumerate(want):
        stream = R.idat(f)
        assert np.array_equal(recs[k], np.stack([R.record(b) for b in blocks])), (k, 'block records')
        assert sizes[k] == len(stream), (k, 'stream size')
        assert blob[at:at + len(stream)] == stream, (k, 'stream bytes')
        assert blob[at + len(stream) - 4:at + len(stream)] == struct.pack('>I', zlib.adler32(R.filtered(R.to_bytes(planes[k], mode)).tobytes())), k
        at += len(stream)
    assert at == len(blob)


def test_kernel_source_on_the_host_equals_the_restatement(host_exe, tmp_path, cases, restated):
    names = list(cases)
    got = run_host(host_exe, tmp_path, 'list', [(cases[n][None], 'u8') for n in names])
    for n, g in zip(names, got):
        check_call(g, cases[n][None], 'u8', [restated[n]])


def test_kernel_source_on_the_host_planes_and_modes(host_exe, tmp_path, cases, restated):
    e = R.soft_ellipse(96, 160)
    x = np.stack([e, np.roll(e, 7, 1) * np.float32(1.2) - np.float32(0.1), np.full_like(e, np.nan)])
    three = np.stack([cases['mixed_130x67'], np.roll(cases['mixed_130x67'], 5, 1), cases['mixed_130x67'][::-1]])
    calls = [(x, 'unit'), (x, 'threshold'), (three, 'u8'), (np.stack([cases['stream_Bp1']] * 2 + [cases['stream_Bp1'][:, ::-1]]), 'u8')]
    got = run_host(host_exe, tmp_path, 'planes', calls)
    for (planes, mode), g in zip(calls, got):
        check_call(g, planes, mode, [R.encode(p, B, mode) for p in planes])
