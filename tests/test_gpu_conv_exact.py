"""Exact-integer tests of the convolution family, one case per kernel form and edge (tests/conv_exact.py: the cases, the fp64 reference and the
conditions under which fp32 accumulation is exact in any order). Every case calls the public entry through maggie_amd.kernels, asserts that the
kernel forms mg_conv_last_forms reports are the ones the case is filed under, and compares the stored bits with torch.equal."""
import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu

_DEVICE_ERROR = []
CASES = [(fam, c, dt) for fam, c in X.all_cases() for dt in c.dtypes]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


class _Forced:
    """mg_set_halo3 / mg_set_halo3_cfg for the duration of a case; the defaults come back whatever happens."""

    def __init__(self, c):
        from maggie_amd import hip
        self.c, self.lib = c, hip.lib()

    def __enter__(self):
        self.lib.mg_set_halo3(int(self.c.halo3))
        self.lib.mg_set_halo3_cfg(*(self.c.cfg or (0, 0, 0)))

    def __exit__(self, *exc):
        self.lib.mg_set_halo3(1)
        self.lib.mg_set_halo3_cfg(0, 0, 0)


def _geo(c, o, K):
    mode = {'CONV': K.MODE_CONV, 'TCONV': K.MODE_TCONV, 'GATHER': K.MODE_GATHER}[c.mode]
    if c.mode == 'GATHER':
        return dict(mode=mode, R=c.k, S=c.k)
    return dict(mode=mode, N=c.N, Hin=c.H, Win=c.W, Hout=o['Ho'], Wout=o['Wo'], R=c.k, S=c.k, stride=c.stride, pad=c.pad, dil=c.dil)


def _xf(c, o, dev):
    if o['xf'] is None:
        return None
    sc, sh, act = o['xf']
    return sc.float().to(dev), sh.float().to(dev), act, X.SLOPE


def _same(c, got, want):
    rep = X.mismatch_report(c, got, want)
    assert rep is None, rep


def _run_fprop(c, dtype, dev):
    from maggie_amd import kernels as K
    o = X.build(c)
    M, Cout = o['M'], c.Cout
    t16 = lambda v: None if v is None else v.to(dtype).to(dev)
    f32 = lambda v: None if v is None else v.float().to(dev)
    x = t16(o['x']).reshape(-1, c.Cin)
    w = t16(o['w'])
    nbr = None if o['nbr'] is None else o['nbr'].to(dev)
    res = None if o['res'] is None else t16(o['res']).reshape(-1, Cout)
    res2 = t16(o['res2'])
    e = X.EPILOGUES[c.epi]
    width = (Cout + 7) // 8 * 8 + 16
    big = torch.zeros((M, width), dtype=dtype, device=dev)
    stats = None
    if c.stats:
        stats = torch.zeros((K.conv_stat_rows(M, *((c.N, o['Ho'], o['Wo']) if c.mode != 'GATHER' else (1, 1, 1))), 2 * Cout), device=dev)
    with _Forced(c):
        K.conv_fprop(x, w, nbr=nbr, scale=f32(o['scale']), shift=f32(o['shift']), res=res, res_mode=o['res_mode'] or 1, res2=res2, act=e.act,
                     pre_act=e.pre_act, slope=X.SLOPE, stats=stats, out=big, yoff=X.YOFF, xf=_xf(c, o, dev), **_geo(c, o, K))
        forms = K.conv_last_forms()
    assert forms == list(c.forms), 'the call ran %s, the case is filed under %s' % (forms, list(c.forms))
    want = X.stored(o['ref'], dtype)
    _same(c, big[:, X.YOFF:X.YOFF + Cout].cpu().contiguous(), want)
    assert not bool(big[:, :X.YOFF].any()) and not bool(big[:, X.YOFF + Cout:].any()), 'columns outside the channel slice were written'
    if c.stats:
        s = stats.double().sum(0).cpu()                                       # deterministic mode: every output tile owns a row
        wd = want.double()
        assert torch.equal(s[:Cout], wd.sum(0)), 'sum y: %d channels differ' % int((s[:Cout] != wd.sum(0)).sum())
        assert torch.equal(s[Cout:], (wd * wd).sum(0)), 'sum y^2: %d channels differ' % int((s[Cout:] != (wd * wd).sum(0)).sum())


def _run_wgrad(c, dtype, dev):
    from maggie_amd import kernels as K
    o = X.build(c)
    x = o['x'].to(dtype).to(dev).reshape(-1, c.Cin)
    dy = o['dy'].to(dtype).to(dev)
    nbr = None if o['nbr'] is None else o['nbr'].to(dev)
    od = dtype if c.dw16 else torch.float32
    kw = dict(cout=c.Cout, nbr=nbr, out_dtype=od, xf=_xf(c, o, dev), **_geo(c, o, K))
    want = X.stored(o['ref'], od)
    with _Forced(c):
        dw = K.conv_wgrad(x, dy, **kw)
        forms = K.conv_last_forms()
    assert forms == list(c.forms), 'the call ran %s, the case is filed under %s' % (forms, list(c.forms))
    assert dw.dtype == od
    _same(c, dw.cpu(), want)
    if c.park:                                                                # parked slabs + one batched reduction: the same bits
        park = []
        with _Forced(c):
            dw2 = K.conv_wgrad(x, dy, park=park, **kw)
            forms = K.conv_last_forms()
            assert forms == list(c.forms[:1]) and len(park) == 1, (forms, len(park))
            K.wgrad_reduce_batched(park)
            assert K.conv_last_forms() == ['reduce_batched']
        _same(c, dw2.cpu(), want)


@pytest.mark.parametrize('fam,c,dt', CASES, ids=['%s-%s-%s' % (fam, X.case_id(c), dt) for fam, c, dt in CASES])
def test_conv_exact(fam, c, dt):
    dev = _dev()
    if _DEVICE_ERROR:
        pytest.fail('not run: an earlier case ended with a device error (%s)' % _DEVICE_ERROR[0])
    dtype = X.DTYPES[dt]
    X.check_conditions(c, dtype)
    try:
        (_run_wgrad if c.kind == 'wgrad' else _run_fprop)(c, dtype, dev)
    except AssertionError:
        raise
    except Exception as e:                                                  # a launch or device error: nothing more goes to the device from this file
        _DEVICE_ERROR.append('%s: %r' % (X.case_id(c), e))
        raise


def test_deterministic_mode_is_on():
    """The statistics comparison above sums one row per output tile: that layout exists in deterministic mode only."""
    from maggie_amd import hip
    _dev()
    assert hip.DETERMINISTIC


def test_large_lds_forms_on_a_second_device():
    """ARMS ITSELF with >= 2 GPUs (skipped on one). The dynamic-LDS opt-in and the CU count are kept per (kernel, device): in a fresh process
    (tests/second_device_worker.py) the smallest exact-integer case of four forms runs on cuda:0 and then on cuda:1 -- every call returns 0 and
    holds its expectation on both devices -- and a 66 KiB token-linear launch gives the same bits on both. What each leg exercises there:
    `h3<8,64,3>` and `async<128,128,2,3>` ask for more than 64 KiB and opt in on the second device, as does the token launch; `h3_slab` asks for
    less and checks the per-device CU count that sizes its grid; `wgrad_gather9<1>` asks for 60 KiB (the <2> form for exactly 64 KiB), so it
    opts in nowhere and checks only that the launcher runs on a second device without the 80 KiB requests it used to make."""
    import json
    import os
    import subprocess
    import sys
    _dev()
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs: the per-device LDS opt-in stays unexecuted on a second device on this box')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'second_device_worker.py')
    forms = ('h3<8,64,3>/CONV', 'h3_slab/CONV', 'async<128,128,2,3>/CONV', 'wgrad_gather9<1>')
    p = subprocess.run([sys.executable, worker, '0,1'] + list(forms), capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
    assert line, (p.returncode, p.stderr[-3000:])
    r = json.loads(line[-1][7:])
    assert p.returncode == 0 and 'error' not in r, (r, p.stderr[-3000:])
    for form in forms:
        for d in (0, 1):
            assert r.get('%s@%d' % (form, d)) == 'ok', r
    assert r['token_equal'] is True, r
