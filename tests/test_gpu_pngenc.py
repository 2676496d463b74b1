"""The device PNG encoder (maggie_amd.utils.pngenc, csrc/pngenc.hip) against the sequential restatement of tests/pngenc_restatement.py, which
tests/test_pngenc_cpu.py holds readable by Pillow, zlib and the decoder: block records first, then the stream bytes, so that a wrong byte
points at the right kernel; then the loop closed on the device through `pngdec.decode_planes`. Every comparison is exact."""
import ctypes
import io
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pngenc_restatement as R                                        # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import pngdec, pngenc                           # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pngenc_pinned.npz')
_CASES, _REF = {}, {}


def cases():
    if not _CASES:
        _CASES.update(R.cases(pngenc.BLOCK_BYTES))
    return _CASES


def variant(name, k):
    """Plane k of a call on case `name`: the case itself, then column rolls of it (the same size, other streams)."""
    p = cases()[name]
    return p if k == 0 else np.ascontiguousarray(np.roll(p, 3 * k, axis=1))


def ref(name, k=0):
    """(plane, file, [Block]) of variant k of a case: computed once, never modified."""
    if (name, k) not in _REF:
        p = variant(name, k)
        _REF[(name, k)] = (p,) + R.encode(p, pngenc.BLOCK_BYTES)
    return _REF[(name, k)]


def check(r, want):
    """An `Encoded` of encode_stats(guard=...) against [(plane, file, [Block])]: records, sizes, bytes, guards."""
    assert len(r.files) == len(want) and r.readbacks == 2
    for k, (_, f, blocks) in enumerate(want):
        assert np.array_equal(r.recs[k], np.stack([R.record(b) for b in blocks])), (k, 'block records')
        assert r.sizes[k] == len(R.idat(f)), (k, 'stream size')
        assert r.streams[k] == R.idat(f), (k, 'stream bytes')
        assert r.files[k] == f, (k, 'file')
    assert len(r.guards) == 6 and all(bool((g == 0xA5).all()) for g in r.guards)
    assert r.blob.numel() == int(r.sizes.sum()) and not bool(r.slack.any())


def test_limits_are_the_module_s():
    v = [ctypes.c_int() for _ in range(6)]
    assert hip.lib().mg_pngenc_limits(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [pngenc.THREADS, pngenc.BLOCK_BYTES, pngenc.REC_WORDS, pngenc.MAX_SIDE, pngenc.MAX_WIDTH, pngenc.MAX_PLANES]
    assert hip.lib().mg_pngenc_limits(None, *[ctypes.byref(x) for x in v[1:]]) == -2


@pytest.mark.parametrize('part', range(4))
def test_one_plane_equals_the_restatement(part):
    for name in list(cases())[part::4]:
        p, f, _ = ref(name)
        check(pngenc.encode_stats(p[None], guard=64), [ref(name)])
        assert pngenc.encode(torch.from_numpy(p).cuda()) == f, name


@pytest.mark.parametrize('part', range(3))
def test_three_and_twenty_four_planes_a_call(part):
    for name in list(cases())[part::3]:
        for P in (3, 24):
            ks = [i % 3 for i in range(P)]                                           # three distinct streams, each eight times at P = 24
            x = np.stack([variant(name, k) for k in ks])
            check(pngenc.encode_stats(x, guard=64), [ref(name, k) for k in ks])


def test_decoder_reads_back_what_the_encoder_writes():
    for name in cases():
        x = torch.from_numpy(np.stack([variant(name, k) for k in range(3)])).cuda()
        back = pngdec.decode_planes(pngenc.encode_planes(x))
        assert back.dtype == torch.uint8 and back.is_cuda and torch.equal(back, x), name


def test_three_input_modes():
    e = R.soft_ellipse(96, 160)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           [np.nan, -1.0, -0.0, 1.5, np.inf, -np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(1))]]).astype(np.float32)
    edges = np.resize(edge, (96, 160)).astype(np.float32)
    x = np.stack([e, np.roll(e, 7, 1) * np.float32(1.2) - np.float32(0.1), edges])
    inside = (edge >= 0) & (edge <= 1)
    assert np.array_equal(R.to_bytes(edge[inside], 'unit'), (edge[inside] * 255).astype('uint8'))      # the reference's own expression
    for mode in ('unit', 'threshold'):
        want = [(None,) + R.encode(p, pngenc.BLOCK_BYTES, mode) for p in x]
        check(pngenc.encode_stats(torch.from_numpy(x).cuda(), mode=mode, guard=64), want)
        back = pngdec.decode_planes(pngenc.encode_planes(x, mode=mode))
        assert np.array_equal(back.cpu().numpy(), np.stack([R.to_bytes(p, mode) for p in x])), mode
    f = pngenc.encode(torch.from_numpy(e).cuda(), mode='unit')
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), (e * 255).astype('uint8'))


def test_two_calls_give_identical_bytes():
    x = torch.from_numpy(np.stack([variant('runs_258_263', k) for k in range(3)])).cuda()
    a, b = pngenc.encode_planes(x), pngenc.encode_planes(x)
    assert a == b and all(isinstance(f, bytes) for f in a)


def test_argument_errors_return_minus_two_before_any_launch():
    L = hip.lib()
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device='cuda')
    xf = torch.zeros((2 * 8 * 8 + 1,), dtype=torch.float32, device='cuda')
    recs = torch.zeros((2 * pngenc.REC_WORDS + 4,), dtype=torch.int32, device='cuda')
    sizes = torch.zeros((4,), dtype=torch.int64, device='cuda')
    out = torch.zeros((256,), dtype=torch.uint8, device='cuda')
    P, I, Lg, V = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    torch.cuda.synchronize()

    def size(planes=x.data_ptr(), mode=0, n=2, h=8, w=8, r=recs.data_ptr(), s=sizes.data_ptr()):
        return L.mg_pngenc_size(P(planes), I(mode), Lg(n), I(h), I(w), P(r), P(s), V(None))

    def emit(planes=x.data_ptr(), mode=0, n=2, h=8, w=8, r=recs.data_ptr(), s=sizes.data_ptr(), o=out.data_ptr(), nbytes=256):
        return L.mg_pngenc_emit(P(planes), I(mode), Lg(n), I(h), I(w), P(r), P(s), P(o), Lg(nbytes), V(None))

    assert size(planes=None) == -2 and size(r=None) == -2 and size(s=None) == -2
    assert size(mode=3) == -2 and size(mode=-1) == -2 and size(n=0) == -2 and size(n=pngenc.MAX_PLANES + 1) == -2
    assert size(h=0) == -2 and size(w=0) == -2 and size(h=pngenc.MAX_SIDE + 1) == -2 and size(w=pngenc.MAX_WIDTH + 1) == -2
    assert size(planes=xf.data_ptr() + 1, mode=1) == -2 and size(r=recs.data_ptr() + 2) == -2 and size(s=sizes.data_ptr() + 4) == -2
    assert emit(planes=None) == -2 and emit(r=None) == -2 and emit(s=None) == -2 and emit(o=None) == -2
    assert emit(o=out.data_ptr() + 4) == -2 and emit(nbytes=254) == -2 and emit(nbytes=0) == -2 and emit(mode=7) == -2
    assert size(n=pngenc.MAX_PLANES, h=pngenc.MAX_SIDE, w=pngenc.MAX_WIDTH) == -3                      # 65536 x 32769 blocks
    torch.cuda.synchronize()
    assert not bool(recs.any()) and not bool(sizes.any()) and not bool(out.any())                      # nothing ran
    with pytest.raises(TypeError):
        pngenc.encode_planes(x.float(), mode='u8')
    with pytest.raises(ValueError):
        pngenc.encode_planes(x[0])


def test_save_visualization_writes_the_reference_s_tree(tmp_path):
    z = np.load(GOLDEN)
    for tag in ('named', 'numbered', 'single'):
        names = [[str(s)] for s in z[tag + '.image_names']]
        anames = [[str(s)] for s in z[tag + '.alpha_names']] if (tag + '.alpha_names') in z.files else None
        H, W = z[tag + '.alphas'].shape[-2:]
        pad = z[tag + '.pad']
        info = [{'name': 'resize', 'ori_size': (H, W)}, {'name': 'padding', 'pad_size': (int(pad[0]), int(pad[1]))}]
        output = {}
        if (tag + '.diff_pred') in z.files:
            output = {'diff_pred': torch.from_numpy(z[tag + '.diff_pred']).cuda(), 'inc_bin_maps': [torch.from_numpy(z[tag + '.inc_bin_maps']).cuda()]}
        d = tmp_path / tag
        cb = partial(pngenc.save_visualization, save_dir=str(d))
        cb(names, anames, torch.from_numpy(z[tag + '.alphas']).cuda(), info, output)
        paths = [str(s) for s in z[tag + '.paths']]
        found = sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
        assert found == sorted(set(paths)), tag
        first = {}
        for i, p in enumerate(paths):
            if p not in first or not p.startswith(('diff_pred', 'inc_pred')):        # an alpha is rewritten, the other two are kept
                first[p] = i
        for p, i in first.items():
            im = Image.open(str(d / p))
            assert im.mode == 'L' and np.array_equal(np.asarray(im), z['%s.plane_%d' % (tag, i)]), (tag, p)
        if output:                                               # a second call leaves diff_pred / inc_pred as they are and rewrites the alphas
            stamp = {p: os.stat(str(d / p)).st_mtime_ns for p in first if p.startswith(('diff_pred', 'inc_pred'))}
            marker = str(d / sorted(stamp)[0])
            with open(marker, 'wb') as f:
                f.write(b'kept')
            cb(names, anames, z[tag + '.alphas'], info, output)                      # NumPy alphas are uploaded
            assert open(marker, 'rb').read() == b'kept'
            assert sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs) == found
