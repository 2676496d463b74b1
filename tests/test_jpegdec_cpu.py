"""Host side of the device JPEG decoder (maggie_amd.utils.jpegdec): the sequential restatement against live Pillow and the fixture Pillow wrote;
the subsequence algorithm stated on the host against the sequential decoder, with its round bound; `parse` against what Pillow reports and on
files outside the supported set; the C entries' argument errors; and the kernel source itself compiled for the host (one thread per GPU thread,
a barrier for __syncthreads) under the address and undefined-behaviour sanitizers, on the case list and on hostile streams. No GPU needed."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import jpegdec_restatement as R                                       # noqa: E402
import make_jpegdec_golden as G                                       # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import jpegdec                                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(R.CASES)
_STREAMS = {}


def stream(name):
    if name not in _STREAMS:
        _STREAMS[name] = R.stream(*(R.LARGE if name == 'large' else R.CASES[name]))
    return _STREAMS[name]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_one_the_issue_names():
    sizes = {c[:2] for c in R.CASES.values()}
    assert set(R.SIZES) <= sizes and (64, 256) in sizes
    assert {c[4].get('quality') for c in R.CASES.values()} >= {1, 50, 90, 100}
    assert {c[2] for c in R.CASES.values()} == {'uniform', 'smooth', 'flat', 'binary', 'periodic'} and {c[3] for c in R.CASES.values()} == {2, 0, 'L'}
    saves = [c[4] for c in R.CASES.values()]
    assert any(s.get('optimize') for s in saves) and {s.get('restart_marker_blocks') for s in saves} >= {1, 3}
    assert any(s.get('restart_marker_rows') == 1 for s in saves) and {s['qtables'][0][0] for s in saves if 'qtables' in s} == {1, 255}
    assert R.SUB_BYTES == (jpegdec.MIN_SUB, 29, 64) and jpegdec.DEFAULT_SUB in R.SUB_BYTES and all(len(stream(n)) % 29 for n in NAMES[:8])
    assert len(stream('large')) > 2 * 128 * jpegdec.DEFAULT_SUB and len(stream('64x48_uniform_0_qua100')) > 1000 * jpegdec.MIN_SUB


@pytest.mark.parametrize('part', range(8))
def test_restatement_equals_live_pillow(part):
    pytest.importorskip('PIL')
    for name in NAMES[part::8] + (['large'] if part == 0 else []):
        assert np.array_equal(R.decode(stream(name)), R.pillow(stream(name))), name


def test_the_range_limit_cases_leave_the_sample_range():
    """The all-1 and all-255 tables on the 0 / 255 input drive the inverse transform outside 0..255 before the range limit: the rule is used."""
    hit = 0
    for name in NAMES:
        if 'qta' in name:
            d = stream(name)
            hdr = R.parse(d)
            c = R.coefficients(d).reshape(-1, 8, 8) * hdr['quant'][0].reshape(8, 8)
            cols = np.swapaxes(R.P.idct_1d(np.swapaxes(c, -1, -2), 11), -1, -2)
            v = R.P.idct_1d(cols, 18)
            hit += int((v < -128).any() and (v > 127).any())
            assert v.min() >= -512 and v.max() < 512                       # where the table and a clamp agree: what an 8-bit encoder reaches
            assert np.array_equal(R.range_limit(v), np.clip(v + 128, 0, 255))
    assert hit >= 4
    v = np.arange(-2048, 2048)
    assert np.array_equal(R.range_limit(v)[(v >= -512) & (v < 512)], np.clip(v + 128, 0, 255)[(v >= -512) & (v < 512)])
    assert R.range_limit(np.array([512, 640, 1023, -513, -1024]))[:5].tolist() == [0, 0, 127, 255, 128]      # periodic beyond, unlike a clamp


@pytest.mark.parametrize('name', G.PINNED)
def test_fixture_equals_the_restatement(name):
    d = load_golden('jpegdec_pinned.npz')
    data = d[name + '.stream'].tobytes()
    assert np.array_equal(R.decode(data), d[name + '.pixels'])
    assert 'Pillow' in str(d['versions']) and 'jpg' in str(d['versions'])
    try:
        live = stream(name)
    except ImportError:
        return
    assert live == data, 'Pillow writes another stream than the fixture holds'


def test_fixture_is_small():
    path = os.path.join(ROOT, 'tests', 'golden', 'jpegdec_pinned.npz')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'photometric_pinned.npz'))
    assert 10 <= len(G.PINNED) <= 14


# ---- the subsequence algorithm on the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', range(8))
def test_sync_rounds_gives_the_sequential_coefficients_within_the_bound(part):
    for name in NAMES[part::8]:
        data = stream(name)
        want = R.coefficients(data)
        length = R.parse(data)['length']
        for s in R.SUB_BYTES:
            got, rounds = R.sync_rounds(data, s)
            assert np.array_equal(got, want), (name, s)
            assert rounds <= max(1, -(-length // s)), (name, s, rounds)


def test_sync_rounds_on_the_large_stream_and_the_periodic_one_is_slow():
    data = stream('large')
    got, rounds = R.sync_rounds(data, 64)
    assert np.array_equal(got, R.coefficients(data)) and rounds <= -(-R.parse(data)['length'] // 64)
    per = stream('64x256_periodic_2_qua100')
    n = -(-R.parse(per)['length'] // jpegdec.MIN_SUB)
    assert n // 2 < R.sync_rounds(per, jpegdec.MIN_SUB)[1] <= n                # the lanes never agree by themselves: the true start walks the stream


# ---- parse ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES[::7] + [n for n in NAMES if 'res' in n or 'opt' in n or 'qta' in n])
def test_parse_returns_what_pillow_reports(name):
    Image = pytest.importorskip('PIL.Image')
    data = stream(name)
    h, w, kind, mode, save = R.CASES[name]
    plan, im, hdr = jpegdec.parse(data), Image.open(io.BytesIO(data)), R.parse(data)
    assert (plan.width, plan.height) == im.size == (w, h)
    assert plan.layout == {2: jpegdec.L420, 0: jpegdec.L444, 'L': jpegdec.GREY}[mode]
    assert plan.sampling == (((2, 2), (1, 1), (1, 1)) if mode == 2 else ((1, 1),) * (1 if mode == 'L' else 3))
    assert sorted(plan.quantization) == sorted(im.quantization)
    for k, t in im.quantization.items():
        assert plan.quantization[k].dtype == np.int32 and np.array_equal(plan.quantization[k], np.asarray(t))
    assert plan.qtables.shape == (3, 64) and plan.qtables.dtype == np.int32
    if 'qtables' in save:
        assert (plan.qtables == save['qtables'][0][0]).all()
    mcux = -(-w // (16 if mode == 2 else 8))
    want_ri = save.get('restart_marker_blocks', 0) or save.get('restart_marker_rows', 0) * mcux
    assert plan.restart_interval == want_ri == hdr['ri']
    assert (plan.offset, plan.length) == (hdr['offset'], hdr['length']) and data[plan.offset + plan.length:plan.offset + plan.length + 2] == b'\xff\xd9'
    assert sorted(plan.dc) == sorted(hdr['dc']) and sorted(plan.ac) == sorted(hdr['ac'])
    for k in plan.ac:
        assert np.array_equal(plan.ac[k][0], hdr['ac'][k][0]) and np.array_equal(plan.ac[k][1], hdr['ac'][k][1])
    if save.get('optimize'):
        std = jpegdec.parse(stream(NAMES[0]))
        assert not np.array_equal(plan.ac[0][0], std.ac[0][0])              # not the Annex K table


def _save(x, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def test_parse_rejects_what_the_device_does_not_decode():
    pytest.importorskip('PIL')
    x = R.image(17, 23, 'smooth', 1, 2)
    with pytest.raises(jpegdec.Unsupported, match='progressive'):
        jpegdec.parse(_save(x, quality=80, progressive=True))
    with pytest.raises(jpegdec.Unsupported, match='sampling'):
        jpegdec.parse(_save(x, quality=80, subsampling=1))
    good = bytearray(_save(x, quality=80))
    assert jpegdec.parse(bytes(good)).layout == jpegdec.L420
    sof = good.index(b'\xff\xc0')
    bad = bytearray(good); bad[sof + 4] = 12                                # 12-bit precision
    with pytest.raises(jpegdec.Unsupported, match='12-bit'):
        jpegdec.parse(bytes(bad))
    bad = bytearray(good)                                                   # 4 components: one more entry in SOF0
    bad[sof + 2:sof + 4] = struct.pack('>H', 8 + 3 * 4)
    bad[sof + 9] = 4
    bad[sof + 19:sof + 19] = bytes([4, 0x11, 0])
    with pytest.raises(jpegdec.Unsupported, match='4 components'):
        jpegdec.parse(bytes(bad))
    dqt = good.index(b'\xff\xdb')
    bad = bytearray(good); bad[dqt + 4] |= 0x10                             # a 16-bit table
    with pytest.raises(jpegdec.Unsupported, match='16-bit'):
        jpegdec.parse(bytes(bad))
    adobe = bytes(good[:2]) + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + bytes(good[2:])
    with pytest.raises(jpegdec.Unsupported, match='Adobe'):
        jpegdec.parse(adobe)
    assert jpegdec.parse(adobe[:17] + b'\x01' + adobe[18:]).layout == jpegdec.L420        # transform 1 = YCbCr
    dnl = bytes(good[:-2]) + b'\xff\xdc\x00\x04\x00\x11\xff\xd9'
    with pytest.raises(jpegdec.Unsupported, match='DNL'):
        jpegdec.parse(dnl)
    two = bytes(good[:-2]) + bytes(good[good.index(b'\xff\xda'):])
    with pytest.raises(jpegdec.Unsupported, match='several scans'):
        jpegdec.parse(two)
    com = bytes(good[:2]) + b'\xff\xfe\x00\x05abc' + b'\xff\xe1\x00\x08Exif\x00\x00' + bytes(good[2:])
    assert jpegdec.parse(com).geometry == jpegdec.parse(bytes(good)).geometry        # COM and APPn are skipped
    for junk in (b'', b'\x89PNG\r\n\x1a\n' + bytes(40), bytes(good[:40])):
        with pytest.raises(jpegdec.Unsupported):
            jpegdec.parse(junk)
    assert issubclass(jpegdec.Unsupported, ValueError)


def test_argument_errors_come_before_any_launch():
    data = stream(NAMES[5])
    for bad in (None, 'file.jpg', 5, np.zeros(4, np.uint8)):
        with pytest.raises(TypeError):
            jpegdec.decode(bad)
    with pytest.raises(TypeError):
        jpegdec.decode_clip(data)
    with pytest.raises(TypeError):
        jpegdec.decode_clip([data, None])
    with pytest.raises(ValueError):
        jpegdec.decode_clip([])
    with pytest.raises(ValueError, match='one size'):
        jpegdec.decode_clip([stream(NAMES[5]), stream(NAMES[20])])
    with pytest.raises(ValueError, match='one size'):
        jpegdec.decode_clip([stream('17x23_binary_2_qua100'), stream('17x23_binary_0_qua100')])      # same size, another layout
    for s in (jpegdec.MIN_SUB - 1, jpegdec.MAX_SUB + 1):
        with pytest.raises(ValueError):
            jpegdec.decode(data, sub_bytes=s)
    with pytest.raises(TypeError):
        jpegdec.decode(data, sub_bytes=8.0)
    for f in (jpegdec.decode, jpegdec.decode_clip):
        assert 'graph' in f.__doc__ and 'read-back' in f.__doc__
    assert 'NOT graph-capturable' in jpegdec.__doc__ and 'Read-backs per call' in jpegdec.__doc__


def test_no_gpu_raises_maggie_hip_error():
    import torch
    from maggie_amd.hip import MaggieHipError
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(MaggieHipError):
        jpegdec.decode(stream(NAMES[5]))


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_jpegdec_sync, lib.mg_jpegdec_coef, lib.mg_jpegdec_dcsum, lib.mg_jpegdec_idct, lib.mg_jpegdec_rgb, lib.mg_jpegdec_limits):
        fn.restype = ctypes.c_int
    v = [ctypes.c_int() for _ in range(5)]
    assert lib.mg_jpegdec_limits(*[ctypes.byref(x) for x in v]) == 0 and lib.mg_jpegdec_limits(None, None, None, None, None) == -2
    assert [x.value for x in v] == [jpegdec.THREADS, jpegdec.MIN_SUB, jpegdec.MAX_SUB, jpegdec.DEFAULT_SUB, jpegdec.TAB_WORDS]
    header = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    for name, val in (('420', jpegdec.L420), ('444', jpegdec.L444), ('GREY', jpegdec.GREY), ('422', jpegdec.L422), ('440', jpegdec.L440),
                      ('411', jpegdec.L411), ('MAX_BYTES', '(1L << 28)')):
        assert '#define MG_JPEGDEC_%s %s\n' % (name, val) in header
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    a, b, c, odd = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4))
    odd = ctypes.c_void_p(4100)

    def sync(n=1, nsub=4, s=8, layout=0, launch=0, words=8, data=a, nbytes=64):
        return lib.mg_jpegdec_sync(data, L(nbytes), b, c, c, c, c, c, I(words), L(n), I(nsub), I(s), I(layout), I(launch), None)

    def coef(n=1, nsub=4, s=8, h=16, w=16, layout=0, elems=6 * 64, data=a):
        return lib.mg_jpegdec_coef(data, L(64), b, c, c, c, c, L(elems), c, L(n), I(nsub), I(s), I(h), I(w), I(layout), None)

    def dcsum(n=1, h=16, w=16, layout=0, elems=6 * 64, p=a):
        return lib.mg_jpegdec_dcsum(p, L(elems), b, L(n), I(h), I(w), I(layout), None)

    def idct(n=1, h=16, w=16, layout=0, elems=6 * 64, pb=384, planes=c, p=a):
        return lib.mg_jpegdec_idct(p, L(elems), b, planes, L(pb), L(n), I(h), I(w), I(layout), None)

    def rgb(n=1, h=16, w=16, layout=1, pb=768, e=0, mean=three, planes=a, out=b):
        return lib.mg_jpegdec_rgb(planes, L(pb), out, L(n), I(h), I(w), I(layout), I(e), mean, mean, None)
    assert sync(n=0) == coef(n=0, elems=0) == dcsum(n=0, elems=0) == idct(n=0, elems=0, pb=0) == rgb(n=0, pb=0) == 0
    assert sync(data=None) == coef(data=None) == dcsum(p=None) == idct(p=None) == rgb(planes=None) == -2
    for bad in (dict(n=-1), dict(layout=6), dict(layout=-1)):
        assert sync(**bad) == coef(**bad) == dcsum(**bad) == idct(**bad) == rgb(**bad) == -2, bad
    for bad in (dict(nsub=0), dict(s=jpegdec.MIN_SUB - 1), dict(s=jpegdec.MAX_SUB + 1), dict(nsub=1 << 20, s=4096)):
        assert sync(**bad) == coef(**bad) == -2, bad
    assert sync(launch=-1) == sync(launch=3, words=8) == sync(words=3) == sync(nbytes=-1) == -2
    for bad in (dict(h=0), dict(w=0), dict(h=32768), dict(w=32768), dict(elems=6 * 64 - 1), dict(elems=6 * 64 + 64)):
        assert coef(**bad) == dcsum(**bad) == idct(**bad) == -2, bad
    assert idct(pb=383) == idct(planes=odd) == idct(layout=1, elems=12 * 64, pb=384) == -2
    assert rgb(layout=0, pb=384) == rgb(pb=767) == rgb(e=2) == rgb(e=-1) == rgb(mean=None) == rgb(out=a) == -2


# ---- the kernel source on the host, under the sanitizers ---------------------------------------------------------------------------------------
def _case_bytes(datas, sub_bytes, recs=None):
    plans = [jpegdec.parse(d) for d in datas]
    offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
    if recs is None:
        recs = np.stack([jpegdec.record(p, int(o)) for p, o in zip(plans, offs)])
    h, w, layout = plans[0].geometry
    blob = b''.join(datas)
    return struct.pack('<6i', h, w, layout, sub_bytes, len(datas), len(blob)) + recs.astype('<i4').tobytes() + blob


def _run_host(exe, tmp_path, cases, tag):
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'jpegdec_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, raw, p = [], open(dst, 'rb').read(), 0
    for _ in cases:
        rc, status, rounds, launches, nc, npl, nrgb = struct.unpack_from('<7i', raw, p)
        p += 28
        coef = np.frombuffer(raw, '<i2', nc, p); p += 2 * nc
        planes = np.frombuffer(raw, np.uint8, npl, p); p += npl
        rgb = np.frombuffer(raw, np.uint8, nrgb, p); p += nrgb
        out.append(dict(rc=rc, status=status, rounds=rounds, launches=launches, coef=coef, planes=planes, rgb=rgb))
    assert p == len(raw)
    return out


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('jpegdec_host') / 'jpegdec_host')
    # -fwrapv: a hostile stream can make the 32-bit inverse passes wrap, as libjpeg's do; every result goes through the 10-bit range limit
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fwrapv',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'jpegdec_host.cpp')])
    return exe


def _planes_flat(datas):
    per = [R.planes_of(d, R.coefficients(d)) for d in datas]
    return np.concatenate([np.stack([p[c] for p in per]).reshape(-1) for c in range(len(per[0]))]).astype(np.uint8)


def test_host_build_of_the_kernels_reproduces_the_restatement(host_exe, tmp_path):
    # every case at one sub_bytes in turn; the ones with restarts, optimised tables or extreme tables at all three (the periodic stream, whose
    # rounds are barriers here, not at the minimum)
    special = [n for n in NAMES if any(k in n for k in ('res', 'opt', 'qta'))] + ['64x48_uniform_0_qua100']
    jobs = [([stream(n)], s) for i, n in enumerate(NAMES) for s in (R.SUB_BYTES if n in special else R.SUB_BYTES[i % 3:i % 3 + 1])]
    jobs += [([stream('64x256_periodic_2_qua100')], s) for s in R.SUB_BYTES[1:]]
    jobs.append(([stream('large')], 64))                                    # several workgroups at every sub_bytes; 64 keeps the barriers few
    clip = ['37x53_uniform_2_qua90_res1', '37x53_uniform_2_optT_qua90', '37x53_flat_2_qua1']
    jobs += [([stream(n) for n in clip], s) for s in R.SUB_BYTES]
    res = _run_host(host_exe, tmp_path, [_case_bytes(d, s) for d, s in jobs], 'list')
    for (datas, s), r in zip(jobs, res):
        assert r['rc'] == 0 and r['status'] == 0, (len(datas[0]), s, r['rc'], r['status'])
        want = np.concatenate([R.coefficients(d).reshape(-1) for d in datas])
        assert np.array_equal(r['coef'], want), (len(datas[0]), s)
        assert np.array_equal(r['planes'], _planes_flat(datas)), (len(datas[0]), s)
        if len(r['rgb']):
            assert np.array_equal(r['rgb'], np.stack([R.decode(d) for d in datas]).reshape(-1)), (len(datas[0]), s)
        nsub = max(1, -(-max(R.parse(d)['length'] for d in datas) // s))
        assert r['rounds'] <= nsub and r['launches'] <= -(-nsub // jpegdec.THREADS) + 2


def test_host_build_stays_clean_on_hostile_streams(host_exe, tmp_path):
    """Exactly sized buffers under ASan / UBSan: the segment cut at 1/4, 1/2 and 3/4, every single-byte flip of a short stream, a DRI that lies.
    Every run either sets a status bit or decodes to the right shape; nothing is read or written out of bounds."""
    cases, kinds = [], []
    for name in ('64x48_smooth_2_qua50_res1', '37x53_uniform_0_optT_qua90', '33x65_uniform_L_qua100'):
        data = stream(name)
        plan = jpegdec.parse(data)
        for frac in (1, 2, 3):
            cut = data[:plan.offset + plan.length * frac // 4] + b'\xff\xd9'
            for s in R.SUB_BYTES:
                cases.append(_case_bytes([cut], s)); kinds.append('cut')
    short = stream('8x8_uniform_L_qua100')
    for i in range(len(short)):
        flipped = short[:i] + bytes([short[i] ^ 0xFF]) + short[i + 1:]
        try:
            plan = jpegdec.parse(flipped)
        except jpegdec.Unsupported:
            continue
        if plan.width * plan.height > 1 << 16:
            continue
        cases.append(_case_bytes([flipped], jpegdec.MIN_SUB)); kinds.append('flip')
    for name, ri in (('64x48_smooth_2_qua50_res1', 2), ('64x48_smooth_2_qua50_res1', 4), ('37x53_uniform_0_optT_qua90', 5),
                     ('37x53_uniform_2_qua90_res1', 0)):
        data = stream(name)
        rec = jpegdec.record(jpegdec.parse(data), 0)
        assert rec[920] != ri
        rec[920] = ri
        cases.append(_case_bytes([data], 29, rec[None])); kinds.append('dri%d' % ri)
    assert kinds.count('flip') > 100
    res = _run_host(host_exe, tmp_path, cases, 'hostile')
    for kind, r in zip(kinds, res):
        assert r['rc'] == 0 and r['launches'] >= 1
        if kind == 'cut':
            assert r['status'] & (R.ST_PAST_END | R.ST_COUNT), kind
        if kind in ('dri2', 'dri4', 'dri0'):
            assert r['status'] & R.ST_RESTART, kind
    assert sum(1 for k, r in zip(kinds, res) if k == 'flip' and r['status']) > 10
