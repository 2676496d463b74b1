"""The device JPEG encoder (maggie_amd.utils.jpegenc, csrc/jpegenc.hip) against the sequential restatement of tests/jpegenc_restatement.py, which
tests/test_jpegenc_cpu.py holds against Pillow itself: the coefficients first, then the per-block bits, then the unstuffed stream, then the
file, so that a wrong byte points at its kernel. Every comparison is exact equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import compose_restatement as C                                       # noqa: E402
import jpegenc_restatement as R                                       # noqa: E402
import make_jpegenc_golden as G                                       # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import compose, jpegdec, jpegenc, photometric, pngdec      # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(R.CASES)
GUARD = 64
_REF = {}


def restate(x, q):
    """(coefficients, bits, unstuffed, file) of one frame."""
    coef = R.coefficients(x, q)
    raw, stuffed = R.scan(coef)
    return coef, R.block_bits(coef), raw, R.header(x.shape[0], x.shape[1], q) + stuffed + b'\xff\xd9'


def ref(name):
    """(frame, quality) + restate(...) of a case: computed once, never modified."""
    if name not in _REF:
        h, w, kind, q, seed = R.CASES[name]
        x = R.image(h, w, kind, seed)
        _REF[name] = (x, q) + restate(x, q)
    return _REF[name]


def check(r, wants, tag):
    """An `Encoded` of stats against [restate(...)] per frame, stage by stage; the guards and the slack."""
    assert r.readbacks == 2, tag
    for t, (coef, bits, raw, data) in enumerate(wants):
        assert np.array_equal(r.coef[t].cpu().numpy(), coef), (tag, t, 'coefficients')
        assert np.array_equal(r.bits[t].cpu().numpy(), bits), (tag, t, 'bits')
        assert np.array_equal(r.offs[t].cpu().numpy(), np.cumsum(bits) - bits), (tag, t, 'bit offsets')
        assert r.sizes[2][t] == bits.sum() and r.sizes[1][t] == len(raw) and r.sizes[0][t] == len(data) - 623, (tag, t, 'sizes')
        assert r.unstuffed[t] == raw, (tag, t, 'unstuffed stream')
        assert not r.raw[t, len(raw):].any(), (tag, t, 'bytes behind the unstuffed stream')
        assert r.files[t] == data, (tag, t, 'file')
    assert np.array_equal(r.sizes[3], np.cumsum(r.sizes[0]) - r.sizes[0]), tag
    assert len(r.guards) == 16 and all(bool((g == 0xA5).all()) for g in r.guards), (tag, 'guards')
    assert not r.slack.any(), (tag, 'slack')


@pytest.mark.parametrize('part', range(8))
def test_stage_by_stage_on_the_list(part):
    for name in NAMES[part::8]:
        x, q = ref(name)[:2]
        r = jpegenc.encode_stats(x[None], q, guard=GUARD)
        check(r, [ref(name)[2:]], name)


@pytest.mark.parametrize('names', [['37x53_random_q50', '37x53_smooth_q50', '37x53_binary_q50'], ['8x8_random_q100', '8x8_binary_q100', '8x8_smooth_q100'],
                                   ['48x48_blocks_q75', '48x48_checker_q75', '48x48_columns_q75']])
def test_a_clip_of_three_equals_three_single_files(names):
    frames = np.stack([ref(n)[0] for n in names])
    q = ref(names[0])[1]
    r = jpegenc.encode_stats(frames, q, guard=GUARD)
    check(r, [ref(n)[2:] for n in names], names)
    assert jpegenc.encode_clip(frames, q) == [ref(n)[5] for n in names]
    assert [jpegenc.encode(ref(n)[0], q) for n in names] == [ref(n)[5] for n in names]
    assert jpegenc.encode_clip(torch.from_numpy(frames).cuda(), q) == r.files


@pytest.mark.parametrize('offset', [0, 1])
def test_input_base_at_byte_offset(offset):
    names = ['33x65_random_q80', '33x65_smooth_q80', '33x65_binary_q80']
    frames = np.stack([ref(n)[0] for n in names])
    buf = torch.zeros((frames.size + 16,), dtype=torch.uint8, device='cuda')
    x = buf[offset:offset + frames.size].view(frames.shape)
    x.copy_(torch.from_numpy(frames))
    assert x.data_ptr() % 16 == offset
    check(jpegenc.encode_stats(x, 80, guard=GUARD), [ref(n)[2:] for n in names], offset)


def limits():
    v = [ctypes.c_int() for _ in range(6)]
    fn = hip.lib().mg_jpegenc_limits
    fn.restype = ctypes.c_int
    assert fn(*[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]


def test_workgroup_boundaries():
    """The smallest uniform-random frame at quality 100 whose stream spans three packing workgroups and three stuffing chunks, with a word that
    two packing workgroups share."""
    _, pack_blocks, chunk_bytes, _, _, _ = limits()
    assert (pack_blocks, chunk_bytes) == (jpegenc.PACK_BLOCKS, jpegenc.CHUNK_BYTES)
    chosen = None
    for h, w in ((16, 64), (32, 64), (32, 128), (64, 128), (64, 256)):
        x = R.P.inputs(h, w, 'random', 100 * h + w)
        want = restate(x, 100)
        if jpegenc.blocks_of(h, w) > 2 * pack_blocks and len(want[2]) > 2 * chunk_bytes:
            chosen = (x, want)
            break
    assert chosen is not None
    x, want = chosen
    r = jpegenc.encode_stats(x[None], 100, guard=GUARD)
    check(r, [want], x.shape)
    starts = r.offs[0].cpu().numpy()[pack_blocks::pack_blocks]
    assert len(starts) >= 2 and (starts % 32 != 0).any()                    # a first / last word written by two workgroups
    assert want[2].count(b'\xff') > 0
    # a clip of it: the second frame's workgroups start at their own slice
    two = np.stack([x, x[::-1].copy()])
    check(jpegenc.encode_stats(two, 100, guard=GUARD), [want, restate(two[1], 100)], 'clip')


@pytest.mark.parametrize('name', ['1x1_random_q1', '9x4_binary_q100', '17x23_random_q50', '37x53_smooth_q75', '33x65_random_q21', '48x48_checker_q100'])
def test_closed_loop_on_the_device(name):
    x, q = ref(name)[:2]
    out = jpegdec.decode(jpegenc.encode(x, q))
    assert torch.equal(out, photometric.jpeg_roundtrip(x, q))
    st = jpegdec.decode_stats([ref(name)[5]])
    assert torch.equal(st.coef, jpegenc.encode_stats(x[None], q).coef)      # the layout mg_jpegdec_dcsum leaves


@pytest.mark.parametrize('nc', [1, 3])
def test_curve_noise_and_file_are_one_chain(nc):
    h, w = 37, 53
    x = R.P.inputs(h, w, 'smooth', 3)
    rs = np.random.RandomState(11 + nc)
    lut = np.stack([np.clip((np.arange(256) / 255.0) ** g * 255 + 0.5, 0, 255) for g in (0.7, 1.0, 1.4)]).astype(np.uint8)
    noise = rs.randint(-40, 41, (h, w, nc)).astype(np.int16)
    for q in (50, 75):
        data = jpegenc.encode(x, q, lut=lut, noise=noise)
        y = R.P.add_noise(R.P.apply_lut(x, lut), noise)
        assert data == R.file_bytes(y, q)
        draws = photometric.PhotoDraws(lut=lut, noise=noise, quality=q)
        assert torch.equal(jpegdec.decode(data), photometric.apply(x, draws))
    assert jpegenc.encode(x, 75, lut=lut) == R.file_bytes(R.P.apply_lut(x, lut), 75)
    assert jpegenc.encode(x, 75, noise=noise) == R.file_bytes(R.P.add_noise(x, noise), 75)


@pytest.mark.parametrize('value', [1, 255])
def test_table_form(value):
    t = np.full((2, 64), value, np.int32)
    for h, w, kind in ((33, 65, 'binary'), (17, 23, 'random')):
        x = R.image(h, w, kind, 100 * h + w)
        want = restate(x, t)
        check(jpegenc.encode_stats(x[None], t, guard=GUARD), [want], (value, h, w))
        assert jpegenc.encode(x, torch.from_numpy(t).cuda()) == want[3]


@pytest.mark.parametrize('name', list(G.pinned_cases()))
def test_fixture_key_by_key(name):
    d = load_golden('jpegenc_pinned.npz')
    q = int(d[name + '.quality']) if d[name + '.quality'].ndim == 0 else d[name + '.quality']
    assert jpegenc.encode(d[name + '.frame'], q) == d[name + '.file'].tobytes()


def test_save_sample_writes_the_tool_s_tree(tmp_path):
    g = load_golden('compose_pinned.npz')
    seed = int(g['image/0/seed'])
    fgs, alphas, bg = C.image_inputs(str(g['image/0/name']))
    sample = compose.synthesize_image(seed, fgs, alphas, bg)
    loader = compose.synthesize_image(seed, fgs, alphas, bg, jpeg=True)
    n = int(sample['fgs'].shape[0])
    assert n >= 2
    dirs = [str(tmp_path / d) for d in ('images', 'bg', 'alphas', 'fg')]
    paths = jpegenc.save_sample(sample, seed, *dirs)
    want = [os.path.join(dirs[0], '%d.jpg' % seed), os.path.join(dirs[1], '%d.jpg' % seed)]
    for k in range(n):
        want += [os.path.join(dirs[2], str(seed), '%d.png' % k), os.path.join(dirs[3], str(seed), '%d.jpg' % k)]
    assert paths == want
    found = sorted(os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert found == sorted(want)
    read = lambda p: open(p, 'rb').read()
    frames = [sample['image'], sample['bg']] + list(sample['fgs'])
    decoded = [loader['image'], loader['bg']] + list(loader['fgs'])
    jpgs = want[:2] + want[3::2]
    for p, x, y in zip(jpgs, frames, decoded):
        data = read(p)
        assert data == R.file_bytes(x.cpu().numpy(), 75), p
        assert torch.equal(jpegdec.decode(data), y), p
    for k, p in enumerate(want[2::2]):
        assert torch.equal(pngdec.decode(read(p)), sample['alphas'][k]), p
    # the video tool's line: one frame to one path
    p = str(tmp_path / 'fgr' / 'clip' / '00000.jpg')
    jpegenc.save_frame(sample['image'], p)
    assert read(p) == read(want[0])
    assert jpegenc.save_sample(None, 0, *dirs) == []
