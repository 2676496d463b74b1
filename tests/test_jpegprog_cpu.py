"""Host side of the device progressive JPEG decoder (maggie_amd.utils.jpegprog): the sequential restatement of tests/jpegprog_restatement.py
against live Pillow and against the coefficients of the baseline twins; `parse` on Pillow's scan scripts and on files outside the supported
set; argument errors and the dispatch of `load`; the C entries' argument errors; and the kernel source itself compiled for the host (one thread
per lane, a barrier for __syncthreads, the ballot through a shared array) under the address and undefined-behaviour sanitizers. No GPU needed."""
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

import jpegprog_restatement as J                                      # noqa: E402
import make_jpegprog_golden as G                                      # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import jpegdec, jpegprog                        # noqa: E402

pytest.importorskip('PIL')
R = J.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(J.CASES)
PARTS = 16
YCC_SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
              ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
GREY_SCRIPT = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
_STREAMS = {}


def stream(name):
    if name not in _STREAMS:
        _STREAMS[name] = J.named(name)
    return _STREAMS[name]


def case_of(name):
    return J.LARGE if name == 'large' else J.CASES[name] if name in J.CASES else J.RESTART[name]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_one_the_issue_names():
    assert len(J.CASES) == len(R.SIZES) * len(R.KINDS) * len(R.MODES) * 4 and J.QUALITIES == (1, 50, 90, 100)
    assert all(c[4]['progressive'] is True for c in list(J.CASES.values()) + list(J.RESTART.values()) + [J.LARGE])
    saves = [c[4] for c in J.RESTART.values()]
    assert {c[3] for c in J.RESTART.values()} == set(R.MODES)
    assert any(s.get('restart_marker_blocks') == 1 for s in saves) and any(s.get('restart_marker_rows') == 1 for s in saves)
    assert J.LARGE[:4] == (256, 256, 'uniform', 0) and J.LARGE[4]['quality'] == 100


def check(name):
    """Pixels against Pillow; coefficients against the baseline twin on every block a pixel of the image touches. The padding blocks are NOT
    compared with the twin: a baseline scan codes their AC terms (the encoder's edge replication), a progressive file's one-component scans
    never visit them; here they must hold no AC term at all."""
    data = stream(name)
    coef = J.coefficients(data)
    assert np.array_equal(J.pixels(data, coef), J.pillow(data)), (name, 'pixels')
    twin = R.coefficients(J.twin(*case_of(name)))
    real = J.touched(data)
    assert coef.shape == twin.shape and np.array_equal(coef[real], twin[real]), (name, 'coefficients')
    assert not coef[~real][:, 1:].any(), (name, 'padding blocks')
    return coef, real


@pytest.mark.parametrize('part', range(PARTS))
def test_restatement_equals_live_pillow_and_the_baseline_twin(part):
    for name in NAMES[part::PARTS]:
        check(name)


def test_restatement_on_the_restart_cases_and_the_large_stream():
    for name in list(J.RESTART) + ['large']:
        data = stream(name)
        check(name)
        if name != 'large':
            hdr = J.parse(data)
            assert all(s['ri'] > 0 for s in hdr['scans']) and data.count(b'\xff\xdd') >= 1, name
    coef, real = check('17x23_uniform_2_q90')
    assert (~real).sum() == 2 * 2 * 4 - 3 * 3 and real.sum() == 3 * 3 + 2 * 2 * 2      # 4:2:0 with an odd block count: padding exists


def test_restatement_on_the_longest_end_of_band_runs():
    data = J.runs_stream()
    stats = {}
    coef = J.coefficients(data, stats)
    assert len(data) < 32 * 1024 and coef.shape == (3 * 184 * 184, 64)
    assert 14 in stats['eob_classes'] and stats['silent'] > 4 * 33672       # the largest run class; refinement runs that read no bit
    assert np.array_equal(J.pixels(data, coef), J.pillow(data))
    assert (coef.reshape(184 * 184, 3, 64)[1:, :, 1:] == 0).all() and coef[:3, 1:].any()


@pytest.mark.parametrize('name', G.PINNED)
def test_fixture_equals_the_restatement_and_live_pillow(name):
    d = load_golden('jpegprog_pinned.npz')
    data = d[name + '.stream'].tobytes()
    assert np.array_equal(J.decode(data), d[name + '.pixels']) and np.array_equal(J.pillow(data), d[name + '.pixels'])
    assert 'Pillow' in str(d['versions']) and 10 <= len(G.PINNED) <= 14
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpegprog_pinned.npz')) < 58 * 1024


# ---- parse ---------------------------------------------------------------------------------------------------------------------------------------
def _save(x, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', **kw)
    return buf.getvalue()


@pytest.mark.parametrize('name', NAMES[::29] + list(J.RESTART))
def test_parse_returns_pillows_script_tables_and_segments(name):
    data = stream(name)
    h, w, _, mode, save = case_of(name)
    plan, hdr = jpegprog.parse(data), J.parse(data)
    assert plan.geometry == (h, w, {2: jpegdec.L420, 0: jpegdec.L444, 'L': jpegdec.GREY}[mode])
    assert plan.geometry == jpegdec.parse(J.twin(*case_of(name))).geometry            # the tuple jpegdec has
    assert plan.script == (GREY_SCRIPT if mode == 'L' else YCC_SCRIPT) == J.script(data)
    want = [('dc', None, [0, 4])] + [('ac', 0, [1, 2, 3, 5])] if mode == 'L' else \
        [('dc', None, [0, 6]), ('ac', 0, [1, 4, 5, 9]), ('ac', 1, [3, 8]), ('ac', 2, [2, 7])]
    assert plan.chains == want
    mcux = -(-w // (16 if mode == 2 else 8))
    ri = save.get('restart_marker_blocks', 0) or save.get('restart_marker_rows', 0) * mcux
    for s, t in zip(plan.scans, hdr['scans']):
        assert (s.offset, s.length) == (t['offset'], t['length']) and data[s.offset + s.length] == 0xFF
        assert s.restart_interval == t['ri'] and (ri == 0) == (t['ri'] == 0)
        for k, (_, tdc, tac) in enumerate(t['comps']):
            for mine, theirs in ((s.dc[k], tdc), (s.ac[k], tac)):
                if mine is not None:
                    assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
        assert all(x is None for x in s.ac) == (s.Ss == 0) and all(x is None for x in s.dc) == (s.Ss > 0 or s.Ah > 0)
    tw = jpegdec.parse(J.twin(*case_of(name)))
    assert np.array_equal(plan.qtables, tw.qtables) and plan.qtables.dtype == np.int32
    scans, chains = jpegprog.records(plan, 5, 2, 7)
    assert scans.shape == (len(plan.scans), jpegprog.SCAN_WORDS) and chains.shape == (len(plan.chains), jpegprog.CHAIN_WORDS)
    assert (chains[:, 0] == 2).all() and chains[0, 1] == 7 and chains[:, 2].sum() == len(plan.scans)
    assert sorted(scans[:, 456]) == sorted(5 + s.offset for s in plan.scans)


def _sos(data, number):
    """The offset of the SOS marker of scan `number`."""
    s = J.parse(data)['scans'][number]
    at = data.rfind(b'\xff\xda', 0, s['offset'])
    assert at + 2 + ((data[at + 2] << 8) | data[at + 3]) == s['offset']
    return at


def test_parse_refuses_by_name():
    x = R.image(17, 23, 'smooth', 1, 2)
    good = _save(x, quality=80, progressive=True)
    assert jpegprog.parse(good).script == YCC_SCRIPT and jpegprog.Unsupported is jpegdec.Unsupported
    with pytest.raises(jpegdec.Unsupported, match='use jpegdec'):
        jpegprog.parse(_save(x, quality=80))
    with pytest.raises(jpegdec.Unsupported, match='sampling'):
        jpegprog.parse(_save(x, quality=80, progressive=True, subsampling=1))
    scans = J.parse(good)['scans']
    for k in range(1, 10):                                                  # cut after each of the first nine scans, closed with EOI
        cut = good[:scans[k - 1]['offset'] + scans[k - 1]['length']] + b'\xff\xd9'
        assert len(J.parse(cut)['scans']) == k
        with pytest.raises(jpegdec.Unsupported, match='incomplete progression'):
            jpegprog.parse(cut)
    for number, byte, match in ((5, 0x20, 'does not continue'), (5, 0x11, 'does not continue'), (1, 0x12, 'no first scan'),
                                (9, 0x21, 'does not continue')):
        at = _sos(good, number)
        bad = bytearray(good)
        assert bad[at + 9] in (0x21, 0x02, 0x10)                            # Ah / Al of a one-component scan
        bad[at + 9] = byte
        with pytest.raises(jpegdec.Unsupported, match=match):
            jpegprog.parse(bytes(bad))
    at = _sos(good, 1)                                                      # an AC scan header with two components
    two = good[:at + 2] + struct.pack('>HB', 10, 2) + bytes([1, 0x00, 2, 0x00]) + good[at + 7:]
    with pytest.raises(jpegdec.Unsupported, match='AC scan of 2 components'):
        jpegprog.parse(two)
    at = _sos(good, 1)
    dqt = good.index(b'\xff\xdb')
    size = (good[dqt + 2] << 8) | good[dqt + 3]
    with pytest.raises(jpegdec.Unsupported, match='DQT segment behind the first scan'):
        jpegprog.parse(good[:at] + good[dqt:dqt + 2 + size] + good[at:])
    sof = good.index(b'\xff\xc2')
    bad = bytearray(good); bad[sof + 4] = 12
    with pytest.raises(jpegdec.Unsupported, match='12-bit'):
        jpegprog.parse(bytes(bad))
    bad = bytearray(good); bad[dqt + 4] |= 0x10
    with pytest.raises(jpegdec.Unsupported, match='16-bit'):
        jpegprog.parse(bytes(bad))
    bad = bytearray(good); bad[sof + 1] = 0xCA
    with pytest.raises(jpegdec.Unsupported, match='arithmetic'):
        jpegprog.parse(bytes(bad))
    adobe = good[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + good[2:]
    with pytest.raises(jpegdec.Unsupported, match='Adobe'):
        jpegprog.parse(adobe)
    assert jpegprog.parse(adobe[:17] + b'\x01' + adobe[18:]).script == YCC_SCRIPT
    with pytest.raises(jpegdec.Unsupported, match='DNL'):
        jpegprog.parse(good[:-2] + b'\xff\xdc\x00\x04\x00\x11\xff\xd9')
    com = good[:2] + b'\xff\xfe\x00\x05abc' + b'\xff\xe1\x00\x08Exif\x00\x00' + good[2:]
    assert jpegprog.parse(com).geometry == jpegprog.parse(good).geometry
    for junk in (b'', b'\x89PNG\r\n\x1a\n' + bytes(40), good[:40], good[:len(good) // 2]):
        with pytest.raises(jpegdec.Unsupported):
            jpegprog.parse(junk)
    with pytest.raises(TypeError):
        jpegprog.parse('file.jpg')


def test_argument_errors_come_before_any_launch(monkeypatch):
    from maggie_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a, **k: pytest.fail('a launch'))
    data = stream('16x16_uniform_2_q50')
    for f in (jpegprog.decode, jpegprog.load):
        for bad in (None, 'file.jpg', 5, np.zeros(4, np.uint8)):
            with pytest.raises(TypeError):
                f(bad)
    for f in (jpegprog.decode_clip, jpegprog.load_clip, jpegprog.decode_stats):
        with pytest.raises(TypeError):
            f(data)
        with pytest.raises(TypeError):
            f([data, None])
        with pytest.raises(ValueError, match='at least one'):
            f([])
    other_size, other_layout = stream('64x48_uniform_2_q90'), stream('16x16_uniform_0_q50')
    assert jpegprog.parse(data).geometry[:2] == jpegprog.parse(other_layout).geometry[:2]
    for f in (jpegprog.decode_clip, jpegprog.load_clip):
        with pytest.raises(ValueError, match='one size'):
            f([data, other_size])
        with pytest.raises(ValueError, match='one size'):
            f([data, other_layout])
    with pytest.raises(jpegdec.Unsupported, match='use jpegdec'):
        jpegprog.decode(J.twin(*J.CASES['16x16_uniform_2_q50']))
    with pytest.raises(jpegdec.Unsupported, match='SOF1'):                  # neither decoder: what jpegdec.parse said
        bad = bytearray(data); bad[data.index(b'\xff\xc2') + 1] = 0xC1
        jpegprog.load(bytes(bad))
    for f in (jpegprog.decode, jpegprog.decode_clip):
        assert 'read-back' in f.__doc__
    assert 'no CPU fallback' in jpegprog.__doc__


def test_no_gpu_raises_maggie_hip_error():
    import torch
    from maggie_amd.hip import MaggieHipError
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(MaggieHipError):
        jpegprog.decode(stream('16x16_uniform_2_q50'))


def test_load_dispatches_by_parsing_only(monkeypatch):
    import torch
    case = (37, 53, 'uniform', 2)
    base = [R.stream(*case, dict(quality=q)) for q in (50, 90)]
    prog = [J.stream(*case, dict(quality=q, progressive=True)) for q in (50, 90)]
    seen = []

    def fake_baseline(datas, plans, normalize, mean, std, device, out):
        seen.append(('baseline', list(datas), [type(p).__name__ for p in plans]))
        out.fill_(1)

    def fake_clip(datas, normalize, mean, std, device, out=None, plans=None):
        seen.append(('progressive', list(datas), [type(p).__name__ for p in plans]))
        out.fill_(2)
    monkeypatch.setattr(jpegprog, '_baseline', fake_baseline)
    monkeypatch.setattr(jpegprog, '_clip', fake_clip)
    monkeypatch.setattr(jpegprog, 'resolve_device', lambda device=None: torch.device('cpu'))
    out = jpegprog.load_clip([prog[0], base[0], prog[1], base[1]])
    assert out.shape == (4, 37, 53, 3) and out.dtype == torch.uint8 and out[:, 0, 0, 0].tolist() == [2, 1, 2, 1]
    assert seen == [('baseline', base, ['JpegPlan'] * 2), ('progressive', prog, ['ProgPlan'] * 2)]      # each group once
    del seen[:]
    assert jpegprog.load(base[0], normalize=True).shape == (3, 37, 53) and seen[0][0] == 'baseline' and len(seen) == 1
    del seen[:]
    assert jpegprog.load(prog[0]).shape == (37, 53, 3) and seen[0][0] == 'progressive' and len(seen) == 1


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    lib.mg_jpegprog_limits.restype = lib.mg_jpegprog_chains.restype = ctypes.c_int
    v = [ctypes.c_int() for _ in range(3)]
    assert lib.mg_jpegprog_limits(*[ctypes.byref(x) for x in v]) == 0 and lib.mg_jpegprog_limits(None, None, None) == -2
    assert [x.value for x in v] == [jpegprog.THREADS, jpegprog.SCAN_WORDS, jpegprog.CHAIN_WORDS]
    a, b, c, d, e = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4, 5))

    def chains(n=1, h=16, w=16, layout=0, elems=6 * 64, nbytes=64, nscans=1, nchains=1, data=a, coef=d):
        return lib.mg_jpegprog_chains(data, L(nbytes), b, L(nscans), c, L(nchains), coef, L(elems), e, L(n), I(h), I(w), I(layout), None)
    assert chains(n=0, elems=0) == 0 and chains(nchains=0) == 0
    for bad in (dict(n=-1), dict(layout=6), dict(layout=-1), dict(h=0), dict(w=0), dict(h=32768), dict(elems=6 * 64 - 1), dict(elems=12 * 64),
                dict(nbytes=-1), dict(nscans=-1), dict(nchains=-1), dict(data=None), dict(coef=None), dict(layout=1, elems=6 * 64)):
        assert chains(**bad) == -2, bad


# ---- the kernel source on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('jpegprog_host') / 'jpegprog_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'jpegprog_host.cpp')])
    return exe


def _case_bytes(datas, front=0, edit=None):
    plans = [jpegprog.parse(d) for d in datas]
    blob, scans, chains, _ = jpegprog.pack(plans, datas)
    scans[:, 456] += front
    if edit is not None:
        edit(scans, chains)
    h, w, layout = plans[0].geometry
    return struct.pack('<7i', h, w, layout, len(datas), len(scans), len(chains), front + len(blob)) + scans.astype('<i4').tobytes() + \
        chains.astype('<i4').tobytes() + b'\xff' * front + blob


def _run_host(exe, tmp_path, cases, frames, tag):
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'jpegprog_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, raw, p = [], open(dst, 'rb').read(), 0
    for n in frames:
        rc, nc = struct.unpack_from('<2i', raw, p)
        p += 8
        info = np.frombuffer(raw, '<i4', n, p); p += 4 * n
        coef = np.frombuffer(raw, '<i2', nc, p); p += 2 * nc
        out.append(dict(rc=rc, info=info, coef=coef))
    assert p == len(raw)
    return out


def test_host_build_of_the_kernel_reproduces_the_restatement(host_exe, tmp_path):
    jobs = [([stream(n)], i % 4) for i, n in enumerate(NAMES[::5] + list(J.RESTART))] + [([stream('large')], 3)]
    jobs.append(([stream(n) for n in ('37x53_uniform_2_q1', '37x53_uniform_2_q90_blocks1', '37x53_uniform_2_q100')], 1))
    res = _run_host(host_exe, tmp_path, [_case_bytes(d, f) for d, f in jobs], [len(d) for d, _ in jobs], 'list')
    for (datas, front), r in zip(jobs, res):
        assert r['rc'] == 0 and not r['info'].any(), (len(datas[0]), front, r['rc'], r['info'])
        assert np.array_equal(r['coef'], np.concatenate([J.coefficients(d).reshape(-1) for d in datas])), (len(datas[0]), front)


def test_host_build_stays_clean_on_hostile_streams(host_exe, tmp_path):
    """Exactly sized buffers under ASan / UBSan: a scan's segment cut at 1/4, 1/2 and 3/4, every single-byte flip behind the frame header of a
    short file, a DRI that lies, records that point outside the buffers. Every run either sets a status bit or fills the buffer; nothing is read
    or written out of bounds, and no loop spins (the program ends)."""
    cases, kinds = [], []
    for name in ('64x48_smooth_2_q50_rows1', '37x53_uniform_0_q90', '33x65_uniform_L_q100'):
        data = stream(name)
        for s in J.parse(data)['scans'][1::3]:
            for frac in (1, 2, 3):
                cut = data[:s['offset'] + s['length'] * frac // 4] + data[s['offset'] + s['length']:]
                cases.append(_case_bytes([cut])); kinds.append('cut')
    short = stream('8x8_uniform_L_q100')
    for i in range(short.index(b'\xff\xc2') + 12, len(short)):
        flipped = short[:i] + bytes([short[i] ^ 0xFF]) + short[i + 1:]
        try:
            plan = jpegprog.parse(flipped)
        except jpegdec.Unsupported:
            continue
        cases.append(_case_bytes([flipped])); kinds.append('flip')
    data = stream('64x48_smooth_2_q50_rows1')

    def lie(word, value, row=slice(None)):
        def edit(scans, chains):
            scans[row, word] = value
        return edit
    for ri in (0, 2, 4):
        cases.append(_case_bytes([data], edit=lie(458, ri))); kinds.append('dri')
    for word, value in ((456, 1 << 30), (457, 1 << 30), (456, -5), (460, 64), (459, -1), (462, 14), (463, 7), (464, 3), (466, 0x7F)):
        cases.append(_case_bytes([data], edit=lie(word, value))); kinds.append('record')

    def chain_outside(scans, chains):
        chains[0, 1:3] = (len(scans) - 1, 5)
    cases.append(_case_bytes([data], edit=chain_outside)); kinds.append('record')
    assert kinds.count('flip') > 50
    res = _run_host(host_exe, tmp_path, cases, [1] * len(cases), 'hostile')
    for kind, r in zip(kinds, res):
        assert r['rc'] == 0, kind
        if kind in ('cut', 'dri', 'record'):
            assert r['info'][0] != 0, kind
    assert sum(1 for k, r in zip(kinds, res) if k == 'flip' and r['info'][0]) > 10
