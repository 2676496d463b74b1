"""Exact-integer convolution tests: operands, fp64 reference, bit comparison, and the table of cases keyed by kernel form.

Method. Operands are small integers, so every product and every partial sum of a convolution is an integer far below 2^24:
fp32 accumulation is exact in ANY order (MFMA blocks, ring stages, split-K slabs, parked and ordered reductions), the stored 16-bit value is
exactly representable, and the comparison with an fp64 reference is torch.equal on the stored bits -- one dropped, duplicated, misplaced or stale
term is an integer difference. The two conditions this rests on are ASSERTED on the reference of every case (check_conditions), never assumed.

This is a plain module (no fixtures, no pytest settings): tests/test_conv_exact_cpu.py checks the helper, the conditions and the form ledger
without a GPU, tests/test_gpu_conv_exact.py runs the cases on the device.
"""
import re
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE = 0.25
YOFF = 8                    # outputs land in columns [8, 8 + Cout) of a zeroed buffer of round_up(Cout, 8) + 16 columns

_FIELDS = dict(
    kind='fprop',           # 'fprop' (mg_conv_fprop[_ws]) | 'wgrad' (mg_conv_wgrad_ws / _park)
    mode='CONV',            # CONV | TCONV | GATHER
    N=1, Cin=32, Cout=32, H=8, W=16,        # x is (N, H, W, Cin); TCONV: the transposed convolution's INPUT map
    k=3, stride=1, pad=1, dil=1,
    out=None,               # TCONV: (Hout, Wout) when it is not the default (H - 1) * stride - 2 * pad + dil * (k - 1) + 1
    rows=0,                 # GATHER: rows of x (the output has N rows: the neighbour table is [N, k * k])
    epi='plain',            # epilogue variant (EPILOGUES)
    stats=False,            # BatchNorm statistics of the stored values, one row per output tile
    xf=None,                # operand transform variant (XFORMS) applied to x in flight
    cfg=None,               # mg_set_halo3_cfg(th, bn, ns) for the call
    halo3=True,             # mg_set_halo3(on) for the call
    dtypes=('bf16',),
    dens=768,               # weights (wgrad: dy) are +-1 with density min(1, dens / K), else 0
    dw16=False,             # wgrad: dW in the activations' 16-bit type (the converting reduce)
    park=False,             # wgrad: also through mg_conv_wgrad_park + mg_wgrad_reduce_batched, which must give the same bits
    forms=(),               # the kernel forms the call must launch, in launch order
    seed=0,
)
Case = namedtuple('Case', list(_FIELDS))
Case.__new__.__defaults__ = tuple(_FIELDS.values())


def case_id(c):
    geo = '%s%dx%d_%s_n%d_c%d-%d_%dx%d' % (c.kind[0], c.k, c.k, c.mode, c.N, c.Cin, c.Cout, c.H, c.W)
    if c.stride != 1 or c.dil != 1:
        geo += '_s%dd%d' % (c.stride, c.dil)
    tags = [c.epi if c.epi != 'plain' else '', 'st' if c.stats else '', 'xf-' + c.xf if c.xf else '', 'cfg%d.%d.%d' % c.cfg if c.cfg else '',
            '' if c.halo3 else 'h3off', 'dw16' if c.dw16 else '', 'park' if c.park else '']
    return '-'.join([c.forms[0] if c.forms else '?', geo] + [t for t in tags if t])


# ---- epilogue and operand-transform variants: every parameter keeps the arithmetic exact (halves, quarters and integers) ------------------------
# scales: per-channel draws from the set; shift: integers in [-8, 8]; res / res2: integers in [-4, 4]; res 'half' = res_mode 2 (half resolution,
# nearest: the output map of such a case must be even), 'full' = res_mode 1.
Epi = namedtuple('Epi', 'scales shift res res2 act pre_act')
EPILOGUES = {
    'plain': Epi(None, False, None, False, ACT_NONE, False),
    'relu': Epi((0.5, -0.5, 1.0, -1.0), True, None, False, ACT_RELU, False),
    'res': Epi(None, False, 'full', False, ACT_NONE, False),
    'lrelu_res': Epi((1.0, -1.0), True, 'half', True, ACT_LRELU, False),
    'lrelu_full': Epi((1.0, -1.0), True, 'full', True, ACT_LRELU, False),     # the same with a full-resolution residual (odd output maps)
    'pre2': Epi((2.0, -1.0, 1.0), True, 'full', False, ACT_RELU, True),       # |scale| > 1: the case halves its weight density
}
XFORMS = {                   # (scales, act): x' = act(x * scale[c] + shift[c]), integer shift in [-2, 2]
    'relu': ((1.0, -1.0, 2.0, -2.0), ACT_RELU),
    'lrelu': ((1.0, -1.0, 2.0), ACT_LRELU),
}


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * SLOPE)
    return v


def out_hw(c):
    if c.mode == 'GATHER':
        return 1, 1
    if c.mode == 'CONV':
        f = lambda h: (h + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
        return f(c.H), f(c.W)
    if c.out is not None:
        return c.out
    f = lambda h: (h - 1) * c.stride - 2 * c.pad + c.dil * (c.k - 1) + 1
    return f(c.H), f(c.W)


def reduction_length(c):
    if c.kind == 'wgrad':
        Ho, Wo = out_hw(c)
        return c.N * Ho * Wo
    return c.k * c.k * c.Cin


def linear(c, x, wk, nbr=None):
    """The convolution itself in the dtype of its arguments (float64 here). x: (N, H, W, Cin) rows (GATHER: (rows, Cin)); wk: the kernels' weight
    layout (Cout, k * k, Cin) -- TCONV: wk[co, tap, ci] = w_transposed[ci, co, ky, kx]. Returns (M, Cout) rows."""
    if c.mode == 'GATHER':
        xp = torch.cat([x, x.new_zeros((1, c.Cin))], 0)                        # nbr == -1 reads the zero row
        y = x.new_zeros((c.N, c.Cout))
        for t in range(c.k * c.k):
            y = y + xp[nbr[:, t].long()] @ wk[:, t, :].t()
        return y
    xn = x.permute(0, 3, 1, 2)
    w4 = wk.reshape(c.Cout, c.k, c.k, c.Cin)
    if c.mode == 'CONV':
        y = F.conv2d(xn, w4.permute(0, 3, 1, 2), None, c.stride, c.pad, c.dil)
    else:
        Ho, Wo = out_hw(c)
        dflt = (c.H - 1) * c.stride - 2 * c.pad + c.dil * (c.k - 1) + 1, (c.W - 1) * c.stride - 2 * c.pad + c.dil * (c.k - 1) + 1
        y = F.conv_transpose2d(xn, w4.permute(3, 0, 1, 2), None, c.stride, c.pad, (Ho - dflt[0], Wo - dflt[1]), 1, c.dil)
    return y.permute(0, 2, 3, 1).reshape(-1, c.Cout)


def _ints(rs, lo, hi, shape):
    return torch.from_numpy(rs.randint(lo, hi + 1, size=shape).astype(np.float64))


def _sparse_pm1(rs, dens, K, shape):
    q = min(1.0, dens / float(K))
    return torch.from_numpy(((rs.uniform(size=shape) < q) * (rs.randint(0, 2, size=shape) * 2 - 1)).astype(np.float64))


_BUILT = {}
_HEAVY = []                 # one slot: the references of the 49 152-row cases are 100 MB each


def build(c):
    """Operands and float64 reference of a case, computed once and shared (callers must not modify them). Keys: x, w (fprop) or dy (wgrad), nbr,
    scale, shift, res, res_mode, res2, xf (scale, shift, act), ref -- the float64 value every stored output must equal: (M, Cout) rows for fprop,
    (Cout, k * k, Cin) for wgrad."""
    if c in _BUILT:
        return _BUILT[c]
    if _HEAVY and _HEAVY[0][0] == c:
        return _HEAVY[0][1]
    rs = np.random.RandomState((zlib.crc32(repr((c.N, c.Cin, c.Cout, c.H, c.W, c.k, c.stride, c.dil, c.mode, c.kind)).encode()) + c.seed) % (2 ** 31))
    Ho, Wo = out_hw(c)
    M = c.N if c.mode == 'GATHER' else c.N * Ho * Wo
    o = {'M': M, 'Ho': Ho, 'Wo': Wo, 'nbr': None, 'xf': None, 'scale': None, 'shift': None, 'res': None, 'res2': None, 'res_mode': 0}
    if c.mode == 'GATHER':
        o['x'] = _ints(rs, -2, 2, (c.rows, c.Cin))
        nbr = rs.randint(0, c.rows, size=(M, c.k * c.k))
        nbr[rs.uniform(size=nbr.shape) < 0.3] = -1
        o['nbr'] = torch.from_numpy(nbr.astype(np.int32))
    else:
        o['x'] = _ints(rs, -2, 2, (c.N, c.H, c.W, c.Cin))
    xe = o['x']
    if c.xf:
        scales, act = XFORMS[c.xf]
        xs = torch.from_numpy(rs.choice(scales, size=c.Cin).astype(np.float64))
        xt = _ints(rs, -2, 2, (c.Cin,))
        o['xf'] = (xs, xt, act)
        xe = _act(xe * xs + xt, act)                                          # padding stays zero: the transform applies to in-image pixels only
    K = reduction_length(c)
    if c.kind == 'wgrad':
        o['dy'] = _sparse_pm1(rs, c.dens, K, (M, c.Cout))
        wk = torch.zeros((c.Cout, c.k * c.k, c.Cin), dtype=torch.float64, requires_grad=True)
        (linear(c, xe, wk, o['nbr']) * o['dy']).sum().backward()
        o['ref'] = wk.grad.detach()
        return _keep(c, o)
    o['w'] = _sparse_pm1(rs, c.dens, K, (c.Cout, c.k * c.k, c.Cin))
    e = EPILOGUES[c.epi]
    if e.scales:
        o['scale'] = torch.from_numpy(rs.choice(e.scales, size=c.Cout).astype(np.float64))
    if e.shift:
        o['shift'] = _ints(rs, -8, 8, (c.Cout,))
    if e.res:
        if e.res == 'half':
            # no fall-back: a case that names a half-resolution residual runs res_mode 2, so its output map must be even
            assert c.mode != 'GATHER' and Ho % 2 == 0 and Wo % 2 == 0, 'half-resolution residual on an odd map: %s' % case_id(c)
            o['res'], o['res_mode'] = _ints(rs, -4, 4, (c.N, Ho // 2, Wo // 2, c.Cout)), 2
        else:
            o['res'], o['res_mode'] = _ints(rs, -4, 4, (M, c.Cout)), 1
    if e.res2:
        o['res2'] = _ints(rs, -4, 4, (M, c.Cout))
    o['xe'] = xe
    o['acc'] = linear(c, xe, o['w'], o['nbr'])
    o['ref'] = epilogue(c, o, o['acc'])
    return _keep(c, o)


def _keep(c, o):
    if o['M'] * c.Cout > (1 << 21):
        _HEAVY[:] = [(c, o)]
    else:
        _BUILT[c] = o
    return o


def epilogue(c, o, acc):
    """The kernels' documented epilogue order in float64: pre-activation, * scale + shift, + res, activation, + res2."""
    e = EPILOGUES[c.epi]
    v = acc
    if e.pre_act:
        v = _act(v, e.act)
    if o['scale'] is not None:
        v = v * o['scale']
    if o['shift'] is not None:
        v = v + o['shift']
    if o['res'] is not None:
        up = o['res'].repeat_interleave(2, 1).repeat_interleave(2, 2) if o['res_mode'] == 2 else o['res']
        v = v + up.reshape(o['M'], c.Cout)
    if not e.pre_act:
        v = _act(v, e.act)
    if o['res2'] is not None:
        v = v + o['res2']
    return v


def stored(ref, dtype):
    """The reference as the kernel stores it: float64 -> float32 -> dtype (both steps exact under check_conditions)."""
    return ref.float().to(dtype)


def _lsb(v):
    """Largest power of two (<= 1) that divides every value."""
    s = 1.0
    while s > 2.0 ** -8 and not bool((v / s == (v / s).round()).all()):
        s /= 2
    return s


def check_conditions(c, dtype):
    """The exactness conditions, asserted on the reference alone. A case that violates one is changed, the condition never relaxed."""
    o = build(c)
    ref = o['ref']
    if c.kind == 'wgrad' and not c.dw16:
        dtype = torch.float32                                                # dW is stored in fp32 unless the case asks for the converting reduce
    assert bool((stored(ref, dtype).double() == ref).all()), 'a reference value is not representable in %s (max |ref| %g)' % (dtype, ref.abs().max())
    if c.kind == 'wgrad':
        # a dW entry is one fp32 accumulator (and sums of its row-split partials): bounded by the sum of |terms|
        assert float(ref.abs().max()) < 2 ** 24
        K = reduction_length(c)
        assert 6.5 * 4 * K < 2 ** 24                                          # sum of |x'| * |dy| over the reduction in quarter steps, |x'| <= 6.5 behind a transform
        return
    acc = o['acc']
    lsb = _lsb(acc)
    assert float(acc.abs().max()) / lsb < 2 ** 24 and 6.5 * reduction_length(c) / lsb < 2 ** 24          # any partial sum of the walk
    if c.stats:
        # one statistics row's partial sums of y and y * y are fp32 accumulators too: bounded by the whole column's sums of |y| and y * y
        l = _lsb(ref)
        assert float((ref.abs() / l).sum(0).max()) < 2 ** 24, 'sum |y| of a channel is not exact in fp32'
        assert float(((ref / l) ** 2).sum(0).max()) < 2 ** 24, 'sum y^2 of a channel is not exact in fp32'


def form_tile(form):
    """(rows-or-tile-height, pixels-per-tile-row or 0, channels) of a form name, for the residues a mismatch report prints."""
    m = re.match(r'(\w+)<([\d,]+)>', form)
    if not m:
        return None
    a = [int(v) for v in m.group(2).split(',')]
    if m.group(1) in ('h3', 'h3_persist', 'halo'):
        return a[0], 16, a[1]
    if m.group(1) == 'c8':
        return a[0], 16, 32
    if m.group(1) in ('fprop', 'async'):
        return a[0], 0, a[1]
    if m.group(1) == 'split':
        return 128, 0, a[0]
    if m.group(1) == 'wgrad':
        return a[0], 0, a[1]
    return None


def mismatch_report(c, got, want, limit=8):
    """None when `got` and `want` (same dtype) hold the same bits; else a description: how many elements differ, the first differing positions as
    (image, y, x, channel) -- (cout, tap, cin) for dW, (row, channel) in gather mode -- and their residues modulo the tile shape of the form."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if torch.equal(got, want):
        return None
    bad = (got != want) | (got.isnan() != want.isnan())
    idx = bad.reshape(-1).nonzero().reshape(-1)
    tile = form_tile(c.forms[0]) if c.forms else None
    Ho, Wo = out_hw(c)
    lines = ['%d of %d elements differ (%s, form %s)' % (idx.numel(), bad.numel(), case_id(c), ','.join(c.forms))]
    for i in idx[:limit].tolist():
        g, w = float(got.reshape(-1)[i]), float(want.reshape(-1)[i])
        if c.kind == 'wgrad':
            co, rem = divmod(i, c.k * c.k * c.Cin)
            tap, ci = divmod(rem, c.Cin)
            pos = '(cout %d, tap %d, cin %d)' % (co, tap, ci)
            if tile:
                pos += ' cout %% %d = %d, cin %% %d = %d' % (tile[0], co % tile[0], tile[2], ci % tile[2])
        else:
            row, ch = divmod(i, c.Cout)
            if c.mode == 'GATHER':
                pos = '(row %d, channel %d)' % (row, ch)
            else:
                n, rem = divmod(row, Ho * Wo)
                y, x = divmod(rem, Wo)
                pos = '(image %d, y %d, x %d, channel %d)' % (n, y, x, ch)
                if tile and tile[1]:
                    pos += ' y %% %d = %d, x %% %d = %d' % (tile[0], y % tile[0], tile[1], x % tile[1])
            if tile:
                if not tile[1]:
                    pos += ' row %% %d = %d' % (tile[0], row % tile[0])
                pos += ', channel %% %d = %d' % (tile[2], ch % tile[2])
        lines.append('  %s: got %r, reference %r' % (pos, g, w))
    return '\n'.join(lines)


# ---- the cases, by kernel form -----------------------------------------------------------------------------------------------------------------
# Every shape below is derived from the dispatch code (conv_halo3.hip: dispatch_h3, h3_eligible; conv_igemm.hip: dispatch_fprop, dispatch_fprop_halo,
# dispatch_fprop_async, dispatch_fprop_ks, plan_splitk; conv_wgrad.hip: dispatch_wgrad and the plan_* functions); the GPU test asserts the forms
# mg_conv_last_forms reports, so a threshold that moves fails the case instead of silently testing another kernel.
def _h3_cases():
    cs = []
    # (form, slab counts to walk as Cin / 32: below, at, one above, more than twice the ring depth), Cout ragged / whole
    forms = [((8, 64, 3), (64, 96, 128, 288), (48, 96, 64, 128)), ((8, 64, 1), (32, 64, 96, 160), (48, 96, 64, 128)),
             ((8, 32, 4), (96, 128, 160, 288), (24, 48, 32, 64)), ((8, 32, 1), (32, 64, 96, 160), (24, 48, 32, 64)),
             ((4, 32, 4), (96, 128, 160, 288), (24, 48, 32, 64))]
    for (th, bn, ns), cins, couts in forms:
        name = 'h3<%d,%d,%d>' % (th, bn, ns)
        hs = (5, 6) if th == 4 else (9, 5)
        he = 6 if th == 4 else 10          # even and still ragged against the tile: the half-resolution residual (res_mode 2) needs an even map
        kw = dict(N=2, cfg=(th, bn, ns))
        cs += [
            Case(Cin=cins[0], Cout=couts[0], H=hs[0], W=17, forms=(name + '/CONV',), dtypes=('bf16', 'f16'), **kw),
            Case(Cin=cins[1], Cout=couts[2], H=hs[1], W=33, forms=(name + '/CONV',), epi='relu', **kw),
            Case(Cin=cins[2], Cout=couts[1], H=he, W=34, forms=(name + '/CONV/res',), epi='lrelu_res', stats=True, **kw),
            Case(Cin=cins[3], Cout=couts[3], H=hs[1], W=17, forms=(name + '/CONV/res',), epi='pre2', dens=384, stats=True, seed=int((th, bn, ns) == (8, 64, 1)), **kw),
            Case(mode='TCONV', Cin=cins[2], Cout=couts[0], H=hs[1], W=33, forms=(name + '/TCONV',), **kw),
            Case(mode='TCONV', Cin=cins[3], Cout=couts[2], H=hs[0], W=17, forms=(name + '/TCONV',), epi='relu', stats=True, **kw),
            Case(mode='TCONV', Cin=cins[0], Cout=couts[1], H=hs[0], W=17, forms=(name + '/TCONV/res',), epi='res', dtypes=('bf16', 'f16'), **kw),
            Case(mode='TCONV', Cin=cins[1], Cout=couts[3], H=he, W=18, forms=(name + '/TCONV/res',), epi='lrelu_res', stats=True, **kw),
            Case(Cin=cins[1], Cout=couts[0], H=hs[0], W=17, forms=(name + '/CONV/xf',), xf='relu', dens=192, **kw),
            Case(Cin=cins[2], Cout=couts[3], H=hs[1], W=33, forms=(name + '/CONV/res/xf',), xf='lrelu', epi='res', dens=32, stats=True, **kw),
        ]
        if ns > 1:          # several tiles per workgroup column
            cs.append(Case(Cin=96, Cout=128, H=24, W=40, forms=(name + '/CONV',), **kw))
    # the one-slab persistent form (Cin 32, Cout <= 32), forced with ns 201
    kw = dict(N=2, Cin=32, cfg=(8, 32, 201))
    cs += [
        Case(Cout=24, H=9, W=17, forms=('h3_slab/CONV',), dtypes=('bf16', 'f16'), **kw),
        Case(Cout=8, H=5, W=33, forms=('h3_slab/CONV',), epi='relu', **kw),
        Case(Cout=32, H=24, W=40, forms=('h3_slab/CONV/res',), epi='lrelu_res', stats=True, **kw),
        Case(mode='TCONV', Cout=32, H=9, W=33, forms=('h3_slab/TCONV',), stats=True, **kw),
        Case(mode='TCONV', Cout=16, H=5, W=17, forms=('h3_slab/TCONV/res',), epi='res', **kw),
        Case(Cout=24, H=9, W=33, forms=('h3_slab/CONV/xf',), xf='relu', dens=192, **kw),
        Case(Cout=32, H=5, W=17, forms=('h3_slab/CONV/res/xf',), xf='lrelu', epi='res', dens=32, stats=True, **kw),
    ]
    # persistent ring forms (forced only): even slab counts; an odd count must fall back to the round-2 two-slab halo form
    for (th, bn, ns), couts in (((8, 64, 103), (48, 128)), ((8, 32, 104), (24, 64))):
        name = 'h3_persist<%d,%d,%d>' % (th, bn, ns - 100)
        kw = dict(N=2, cfg=(th, bn, ns))
        cs += [
            Case(Cin=64, Cout=couts[0], H=9, W=17, forms=(name + '/CONV',), dtypes=('bf16', 'f16'), **kw),
            Case(Cin=128, Cout=couts[1], H=5, W=33, forms=(name + '/CONV',), epi='relu', stats=True, **kw),
            Case(Cin=96 * 2, Cout=128, H=24, W=40, forms=(name + '/CONV',), **kw),
            Case(Cin=288 * 2, Cout=couts[0], H=10, W=34, forms=(name + '/CONV/res',), epi='lrelu_res', stats=True, **kw),
            Case(mode='TCONV', Cin=128, Cout=couts[0], H=5, W=17, forms=(name + '/TCONV',), **kw),
            Case(mode='TCONV', Cin=64, Cout=couts[1], H=10, W=18, forms=(name + '/TCONV/res',), epi='lrelu_res', stats=True, **kw),
            Case(Cin=96, Cout=64, H=9, W=17, forms=('halo<8,32,2>/CONV',), **kw),
        ]
    # the default dispatch at the smallest grids that select each form: the thresholds themselves
    cs += [
        Case(N=4, Cin=96, Cout=64, H=64, W=128, forms=('h3<8,64,3>/CONV',)),                 # t64 = 256: 200 <= t64 < 320
        Case(N=4, Cin=96, Cout=64, H=32, W=128, forms=('h3<8,32,4>/CONV',)),                 # t64 = 128 < 200 <= t32 = 256
        Case(N=5, Cin=96, Cout=64, H=64, W=128, forms=('h3<8,64,1>/CONV',)),                 # t64 = 320
        Case(N=2, Cin=64, Cout=24, H=9, W=17, forms=('h3<8,32,1>/CONV',)),                   # two slabs, Cout <= 32
        Case(N=2, Cin=64, Cout=48, H=9, W=17, forms=('h3<8,64,1>/CONV',)),                   # two slabs, Cout > 32
        Case(N=2, Cin=96, Cout=64, H=9, W=17, forms=('h3<4,32,4>/CONV',)),                   # t32 < 200
        Case(N=2, Cin=96, Cout=64, H=5, W=17, mode='TCONV', forms=('h3<4,32,4>/TCONV',)),    # H < 8
    ]
    return cs


def _halo_cases():
    cs = []
    kw = dict(N=2, halo3=False)
    for th, hs in ((8, (9, 8)), (4, (5, 6))):
        for bn, couts in ((16, (8, 16)), (32, (24, 32)), (64, (48, 64))):
            name = 'halo<%d,%d,1>' % (th, bn)
            cs += [
                Case(Cin=32, Cout=couts[0], H=hs[0], W=17, forms=(name + '/CONV',), dtypes=('bf16', 'f16'), **kw),
                Case(Cin=64, Cout=couts[1], H=10 if th == 8 else 6, W=34, forms=(name + '/CONV',), epi='lrelu_res', stats=True, **kw),
                Case(mode='TCONV', Cin=64, Cout=couts[0], H=hs[0], W=33, forms=(name + '/TCONV',), epi='relu', **kw),
                Case(mode='TCONV', Cin=32, Cout=couts[1], H=hs[1], W=17, forms=(name + '/TCONV',), epi='res', stats=True, **kw),
            ]
            if bn >= 32:
                cs.append(Case(Cin=64, Cout=couts[0], H=hs[0], W=17, forms=(name + '/CONV/xf',), xf='lrelu', dens=32, stats=True, **kw))
    cs += [
        Case(Cin=96, Cout=64, H=9, W=17, forms=('halo<8,32,2>/CONV',), dtypes=('bf16', 'f16'), **kw),
        Case(Cin=160, Cout=96, H=10, W=34, forms=('halo<8,32,2>/CONV',), epi='lrelu_res', stats=True, **kw),
        Case(mode='TCONV', Cin=128, Cout=72, H=9, W=33, forms=('halo<8,32,2>/TCONV',), epi='relu', **kw),
        Case(Cin=96, Cout=72, H=9, W=33, forms=('halo<8,32,2>/CONV/xf',), xf='relu', dens=192, **kw),
        Case(Cin=96, Cout=64, H=5, W=17, forms=('halo<4,64,3>/CONV',), dtypes=('bf16', 'f16'), **kw),
        Case(Cin=288, Cout=96, H=6, W=33, forms=('halo<4,64,3>/CONV',), epi='pre2', dens=384, stats=True, **kw),
        Case(mode='TCONV', Cin=128, Cout=72, H=6, W=34, forms=('halo<4,64,3>/TCONV',), epi='lrelu_res', **kw),
        Case(N=2, Cin=64, Cout=8, H=9, W=33, forms=('halo<8,16,1>/CONV',)),                  # reached with halo3 on: Cout 8 is not a halo3 layer unless Cin is 32
    ]
    return cs


def _c8_cases():
    kw = dict(N=2, Cin=8, forms=('c8<8>',))
    return [Case(Cout=8, H=9, W=17, dtypes=('bf16', 'f16'), **kw), Case(Cout=16, H=5, W=33, epi='relu', stats=True, **kw),
            Case(Cout=32, H=20, W=24, epi='lrelu_res', stats=True, **kw)]


def _async_cases():
    big = dict(N=3, H=128, W=128, Cin=32, k=1, pad=0)                       # M = 49 152: 384 x 2 blocks = MG_FPROP_BLOCKS
    sm = dict(k=1, pad=0)
    return [
        Case(N=2, Cin=64, Cout=72, H=9, W=17, forms=('async<64,64,2,4>/CONV',), dtypes=('bf16', 'f16'), **sm),
        Case(N=2, Cin=96, Cout=128, H=10, W=34, forms=('async<64,64,2,4>/CONV',), epi='lrelu_res', stats=True, **sm),
        Case(Cout=128, forms=('async<128,64,2,4>/CONV',), dtypes=('bf16', 'f16'), **big),
        Case(Cout=256, forms=('async<128,128,2,3>/CONV',), dtypes=('bf16', 'f16'), **big),
        Case(N=2, Cin=64, Cout=72, H=9, W=17, mode='TCONV', forms=('async<64,64,2,4>/TCONV',), epi='relu', stats=True, **sm),
        Case(N=2, Cin=128, Cout=48, H=5, W=9, mode='TCONV', stride=2, forms=('async<64,64,2,4>/TCONV',), **sm),    # odd outputs (9 x 17): not phased
        Case(Cout=128, mode='TCONV', forms=('async<128,64,2,4>/TCONV',), **big),
        Case(Cout=256, mode='TCONV', forms=('async<128,128,2,3>/TCONV',), **big),
        Case(mode='GATHER', N=300, rows=257, Cin=64, Cout=72, forms=('async<64,64,2,4>/GATHER',), epi='relu', stats=True, dtypes=('bf16', 'f16')),
        Case(mode='GATHER', N=49152, rows=4099, Cin=32, Cout=128, k=1, pad=0, forms=('async<128,64,2,4>/GATHER',)),
        Case(mode='GATHER', N=49152, rows=4099, Cin=32, Cout=256, k=1, pad=0, forms=('async<128,128,2,3>/GATHER',)),
    ]


def _fprop_cases():
    """The register-staged kernel: 16-bit 3x3 shapes the halo kernels refuse (dilation 2, stride 2, W < 16), gather tables with Cin % 32 != 0 or
    Cout <= 32, the stride-2 transposed walks (phased where the output is even), and fp32."""
    cs = []
    # stage width by the slab count (3x3, 32 elements per slab): Cin 16 -> 5 slabs (KS 1), 32 -> 9 (KS 2), 96 -> 27 (KS 4)
    ks_cin = ((1, 16), (2, 32), (4, 96))
    # tile by Cout and the grid: (128,16) Cout <= 16; (128,32) <= 32; (64,32) few blocks; (64,64) >= 300 blocks of 64 x 64; the 128-row tiles >= 768 blocks
    small = dict(N=2, H=10, W=18)                                           # even (the half-resolution residual), M = 360 not a multiple of 128
    mid = dict(N=2, H=64, W=80)                                             # M = 10 240: 160 x 2 = 320 blocks of 64 x 64 at Cout 72
    big = dict(N=3, H=128, W=128)                                           # M = 49 152
    tiles = (((128, 16), small, (1, 12, 16)), ((128, 32), small, (24, 32, 20 + 4)), ((64, 32), small, (40, 72, 136)), ((64, 64), mid, (72, 72, 72)),
             ((128, 64), big, (128, 128, 128)), ((128, 128), big, (256, 256, 256)))
    for (bm, bn), geo, couts in tiles:
        for i, (ks, cin) in enumerate(ks_cin):
            name = 'fprop<%d,%d,%d>' % (bm, bn, ks)
            heavy = geo is big
            cout = couts[i]
            cs.append(Case(Cin=cin, Cout=cout, dil=2, pad=2, forms=(name + '/CONV',), epi='plain' if heavy else ('relu', 'lrelu_res', 'pre2')[i],
                           dens=384 if (not heavy and i == 2) else 768, stats=geo is small and cout % 8 == 0,
                           dtypes=('bf16', 'f16'), **geo))
            # transposed, stride 1 / dilation 2: never phased
            cs.append(Case(mode='TCONV', Cin=cin, Cout=cout if cout % 8 == 0 else 16, dil=2, pad=2, forms=(name + '/TCONV',),
                           epi='plain' if heavy else 'res', **geo))
            # gather: Cin % 32 != 0 keeps the wide outputs off the direct-to-LDS ring -- 9 taps x 24 -> 7 slabs, x 40 -> 12, x 72 -> 21
            gcin = (24, 40, 72)[i]
            gM = geo['N'] * geo['H'] * geo['W']
            cs.append(Case(mode='GATHER', N=gM + (0 if heavy else 5), rows=gM // 3 + 7, Cin=gcin, Cout=cout if cout % 8 == 0 else 8,
                           forms=(name + '/GATHER',), epi='plain' if heavy else 'relu', stats=geo is small))
            # phased: stride-2 transposed walk with even outputs, 4 taps x Cin / 32 slabs in the longest phase: Cin 32 -> 4, 64 -> 8, 160 -> 20
            pcin = (32, 64, 160)[i]
            pg = dict(N=geo['N'], H=geo['H'] // 2 if heavy or geo is mid else 5, W=geo['W'] // 2 if heavy or geo is mid else 9)
            po = (pg['H'] * 2, pg['W'] * 2)
            cs.append(Case(mode='TCONV', Cin=pcin, Cout=cout if cout % 8 == 0 else 16, stride=2, out=po, forms=(name + '/TCONV/phased',),
                           epi='plain' if heavy else 'lrelu_res', stats=geo is small, **pg))
    cs += [
        # Cout = 1 and Cout % 8 != 0: the scalar store path
        Case(N=2, Cin=32, Cout=1, H=9, W=17, stride=2, forms=('fprop<128,16,2>/CONV',)),
        Case(N=2, Cin=32, Cout=12, H=9, W=12, forms=('fprop<128,16,2>/CONV',), epi='relu'),                     # W < 16
        # stride-2 data gradients: 3x3 (1 / 2 / 2 / 4 taps) and 1x1 (three empty phases) with ragged phase tiles; the k4 s2 transposed convolution
        Case(mode='TCONV', N=2, Cin=64, Cout=32, H=12, W=20, stride=2, out=(24, 40), forms=('fprop<128,32,2>/TCONV/phased',), dtypes=('bf16', 'f16')),
        Case(mode='TCONV', N=2, Cin=128, Cout=64, H=8, W=12, k=1, pad=0, stride=2, out=(16, 24), forms=('fprop<64,32,1>/TCONV/phased',), epi='relu', stats=True),
        Case(mode='TCONV', N=2, Cin=64, Cout=48, H=7, W=9, k=4, stride=2, forms=('fprop<64,32,2>/TCONV/phased',), epi='lrelu_res', stats=True),
        # odd output sizes take the unphased walk
        Case(mode='TCONV', N=2, Cin=64, Cout=32, H=12, W=20, stride=2, forms=('fprop<128,32,2>/TCONV',)),       # 23 x 39
        # fp32: 16 elements per slab -- Cin 16 -> 9 slabs (KS 2)
        Case(N=2, Cin=16, Cout=40, H=10, W=18, forms=('fprop<64,32,2>/CONV',), dtypes=('f32',), epi='lrelu_res', stats=True),
        Case(N=2, Cin=4, Cout=6, H=9, W=17, forms=('fprop<128,16,1>/CONV',), dtypes=('f32',)),
        Case(mode='TCONV', N=2, Cin=32, Cout=24, H=12, W=20, stride=2, out=(24, 40), forms=('fprop<128,32,2>/TCONV/phased',), dtypes=('f32',), epi='relu'),
        Case(mode='GATHER', N=300, rows=257, Cin=64, Cout=72, forms=('fprop<64,32,4>/GATHER',), dtypes=('f32',)),
    ]
    return cs


def _split_cases():
    """Split-K + finish (mg_conv_fprop_ws): M <= 8192, Cout >= 64, >= 18 stages of 4 slabs, < 300 blocks of 64 x 64. Dilation 2 keeps the 16-bit
    cases off the halo kernels. The plan gives min(ceil(512 / tiles), stages / 3, 8) splits: 6 at K 2304, 8 at K 4608 (2 is not reachable)."""
    kw = dict(dil=2, pad=2)
    f64, f128 = ('split<64>/CONV', 'split_finish'), ('split<128>/CONV', 'split_finish')
    return [
        Case(N=2, Cin=256, Cout=72, H=9, W=17, forms=f64, dtypes=('bf16', 'f16'), **kw),                        # Cout % 32 != 0: the finish kernel's chunk guard
        Case(N=2, Cin=256, Cout=64, H=10, W=18, forms=f64, epi='relu', stats=True, **kw),
        Case(N=2, Cin=256, Cout=72, H=10, W=18, forms=f64, epi='lrelu_res', stats=True, **kw),
        Case(N=2, Cin=256, Cout=64, H=9, W=17, forms=f64, epi='pre2', dens=384, stats=True, **kw),
        Case(N=1, Cin=512, Cout=128, H=10, W=18, forms=f128, epi='lrelu_res', stats=True, **kw),                 # 8 splits
        Case(N=2, Cin=256, Cout=136, H=9, W=17, forms=f128, epi='res', stats=True, **kw),
        Case(mode='TCONV', N=2, Cin=256, Cout=72, H=9, W=17, forms=('split<64>/TCONV', 'split_finish'), epi='relu', **kw),
        Case(mode='TCONV', N=1, Cin=512, Cout=128, H=9, W=17, forms=('split<128>/TCONV', 'split_finish'), stats=True, **kw),
        Case(N=2, Cin=128, Cout=72, H=10, W=18, forms=f64, dtypes=('f32',), epi='lrelu_res', stats=True, **kw),  # fp32: 16 elements per slab
    ]


def _wgrad_cases():
    W_ = dict(kind='wgrad')
    cs = [
        # 8-channel input
        Case(N=2, Cin=8, Cout=32, H=9, W=17, forms=('wgrad_c8', 'reduce_tile'), dtypes=('bf16', 'f16'), park=True, **W_),
        Case(N=2, Cin=8, Cout=64, H=20, W=24, forms=('wgrad_c8', 'reduce_tile'), dw16=True, **W_),
        # halo form: one split (dW written by the GEMM; 16-bit dW through the converting reduce), a few splits, many; tpb not dividing the tile count
        Case(N=1, Cin=32, Cout=32, H=8, W=16, forms=('wgrad_halo',), **W_),
        Case(N=1, Cin=32, Cout=32, H=8, W=16, forms=('wgrad_halo', 'reduce'), dw16=True, park=True, **W_),
        Case(N=2, Cin=96, Cout=64, H=9, W=33, forms=('wgrad_halo', 'reduce_tile'), dtypes=('bf16', 'f16'), park=True, **W_),    # 12 tiles, 12 splits
        Case(N=2, Cin=256, Cout=256, H=17, W=33, forms=('wgrad_halo', 'reduce'), dw16=True, **W_),                              # 18 tiles, 4 splits of 5
        Case(N=2, Cin=64, Cout=32, H=9, W=33, forms=('wgrad_halo/xf', 'reduce_tile'), xf='lrelu', **W_),
        # all-taps gather form
        Case(mode='GATHER', N=256, rows=200, Cin=64, Cout=32, forms=('wgrad_gather9<1>', 'reduce'), dtypes=('bf16', 'f16'), **W_),
        Case(mode='GATHER', N=1100, rows=700, Cin=64, Cout=96, forms=('wgrad_gather9<1>', 'reduce_tile'), park=True, **W_),
        Case(mode='GATHER', N=256, rows=300, Cin=128, Cout=64, forms=('wgrad_gather9<2>', 'reduce'), dw16=True, **W_),
        Case(mode='GATHER', N=1100, rows=700, Cin=64, Cout=64, forms=('wgrad_gather9<2>', 'reduce_tile'), dtypes=('bf16', 'f16'), **W_),
        # the wave reduction: more than 32 splits of a small dW
        Case(N=1, Cin=32, Cout=32, H=128, W=128, k=1, pad=0, forms=('wgrad<32,32>/CONV', 'reduce_wave'), park=True, **W_),
    ]
    # per-tap forms: stride 2 keeps CONV off the halo form; M not a multiple of the 128-row step; channels not multiples of the tile
    for (tco, tci), (cout, cin) in (((32, 32), (24, 32)), ((32, 64), (32, 40)), ((64, 32), (40, 32)), ((64, 64), (72, 40))):
        name = 'wgrad<%d,%d>' % (tco, tci)
        cs += [
            Case(N=2, Cin=cin, Cout=cout, H=19, W=35, stride=2, forms=(name + '/CONV', 'reduce'), dtypes=('bf16', 'f16'), park=tco == tci, **W_),
            Case(mode='TCONV', N=2, Cin=cin, Cout=cout, H=5, W=9, stride=2, out=(10, 18), forms=(name + '/TCONV', 'reduce'), dw16=cin % 8 == 0 and tco == 64, **W_),
            Case(mode='GATHER', N=300, rows=257, Cin=cin, Cout=cout, forms=(name + '/GATHER', 'reduce'), **W_),
        ]
    cs += [
        Case(N=2, Cin=40, Cout=72, H=19, W=35, stride=2, forms=('wgrad<64,64>/CONV', 'reduce'), dtypes=('f32',), **W_),
        Case(mode='GATHER', N=333, rows=257, Cin=32, Cout=24, forms=('wgrad<32,32>/GATHER', 'reduce'), dtypes=('f32',), **W_),
    ]
    return cs


FAMILIES = {
    'halo3': _h3_cases, 'halo_round2': _halo_cases, 'c8': _c8_cases, 'async': _async_cases, 'fprop': _fprop_cases, 'split': _split_cases,
    'wgrad': _wgrad_cases,
}
_ALL = []


def all_cases():
    if not _ALL:
        for fam, fn in FAMILIES.items():
            _ALL.extend((fam, c) for c in fn())
    return list(_ALL)


def cases_by_form():
    """form name -> the cases filed under it (a case is filed under every form its call launches)."""
    table = {}
    for _, c in all_cases():
        for f in c.forms:
            table.setdefault(f, []).append(c)
    if any(c.park for _, c in all_cases()):
        table.setdefault('reduce_batched', []).extend(c for _, c in all_cases() if c.park)
    return table


# Forms without a case, by pattern (fnmatch) -> the reason. Only forms the tests cannot select from inside a process, and the two families the issue
# leaves to later work.
EXCLUDED = {
    'c8<16>': 'selected by MG_FPROP_C8_TH, an environment variable read once per process',
    'halo<8,64,3>/*': 'the wide round-2 form runs only under MG_HALO_NARROW=0, read once per process',
    'async<128,64,2,3>/*': 'three-stage ring: only under MG_ASYNC_NS < 4, read once per process',
    'async<64,64,2,3>/*': 'three-stage ring: only under MG_ASYNC_NS < 4, read once per process',
    '*/bnb': 'BatchNorm-backward link variant (bnb_x): off by default, covered by its own tests',
    '*/bnb/phased': 'BatchNorm-backward link variant (bnb_x): off by default, covered by its own tests',
    'async_mdev<*': 'device-row-count (m_dev) persistent variant: left to a later pull request',
    'fprop_mdev<*': 'device-row-count (m_dev) persistent variant: left to a later pull request',
    'wgrad_gather9<1>/xf': 'the operand transform of the gather forms exists only with a device row count (m_dev): later pull request',
    'wgrad<32,32>/CONV/xf': 'the operand transform of the per-tap forms exists only with a device row count (m_dev): later pull request',
    'wgrad<32,32>/GATHER/xf': 'the operand transform of the per-tap forms exists only with a device row count (m_dev): later pull request',
}
