"""The video-side kernels of maggie_amd/csrc/temporal.hip and temporal2.hip against float64, at their edge shapes.

ConvGRU gate math (four kernels, three storage types), the eval-time alpha aggregation, the bidirectional fusion forward and backward, loss_dtSSD
and the mean BCE with logits in both summation modes, and the eval-time bounding-box crop. The references, the sensitivities S, the cases and the
operation counts k live in tests/temporal_reference.py; tests/test_temporal_reference_cpu.py proves on the host that the references are the
operations, that honest fp32 arithmetic passes every k, and that the comparison |got - ref| <= u_out |ref| + floor + u32 k S rejects every planted
defect by 16 x k. Outputs whose arithmetic is exact (the aggregation, the crop, the copied halves, the logit stacks, exact-integer sums) are
compared with equality.

Shapes: every capped grid wraps once (4096 blocks of the element-wise kernels, 1024 of the two loss reductions, 128 per plane of the box
search), chunks per row that are no power of two, one-element tensors, T = 16 (the register-array limit) and the rejected T = 1 / 17, saturated
logits (+-88, +-100, +-20000), planes narrower than, equal to and one bit wider than a 64-bit word. The grid wrap of crop_apply_kernel needs a
clip of more than 67 M pixels and is left out; it uses the same grid-stride idiom as the other wraps.

Measured err / (u32 S) on the MI355X (largest over all cases of this file; a 16-bit output is absorbed by u_out and reads 0) and the k in use:

    kernel / output                      measured   k
    gru xrh / dh1 (sigmoid times h, g)      1.41 / 1.40    K_SIGMUL 8
    gru hn                                  1.90    15
    gru dr                                  0.74    K_SIGMUL_BWD 12
    gru dz / dc / dh2                       0.77 / 1.71 / 0.62    16 / 15 / 9
    gru dx, x half of xrh                   equal   (copies)
    bifuse fused / dpreds                   0.24 / 0.37    K_BIFUSE 11 (one frame step; the frames add up in S)
    bifuse fsig / bsig                      0.96 / 0.99    K_SIGMUL 8
    bifuse ddiffs                           0.31    sum(NI) + K_BIFUSE + 3                     (23 .. 24)
    dtssd sums[0]        det / atomic       0.43 / 2.25    sum(n) + K_DTSSD_TERM 12            (20 .. 40), atomic + blocks - 1
    dtssd sums[1]        det / atomic       2.03 / 42.1    sum(n) + 1                          (9 .. 30), atomic + blocks - 1
    dtssd loss           det / atomic       0.36 / 4.49    sum(n) + 14                         (22 .. 42), atomic + blocks - 1
    dtssd gradient       det / atomic       2.13 / 12.5    sum(n) + 1 + K_DTSSD_GRAD 19        (28 .. 48), atomic + blocks - 1
    bce sum              det / atomic       0.64 / 2.86    sum(n) + K_BCE_TERM 11              (20 .. 40), atomic + blocks - 1
    bce loss             det / atomic       0.77 / 4.53    sum(n) + 13                         (22 .. 42), atomic + blocks - 1
    bce gradient                            1.51    K_BCE_GRAD 11
    temporal_fuse, crop boxes / alpha / bits, logit stacks, exact-integer sums[0]: compared with equality

Every k is an operation count written down before the first device run, with one exception. That run measured 41.6 on the ATOMIC sums[1] of
loss_dtSSD at 1024 workgroups (no mask: 1024 equal partials) against sum(n) + 1 = 29, while the deterministic form of the same sum measured 2.0.
sum(n) counts a tree; atomicAdd adds the per-workgroup partials one after another in arrival order, and equal partials round the same way at every
step. These blocks - 1 <= 1023 additions are on the path of every atomic-mode sum and were missing from the count: temporal_reference.atomic_k adds
them to the k of all six atomic-mode sums above (not only to the one that exceeded). The atomic figures vary from run to run. That a wrap neither
drops nor repeats an element is shown in both modes by the exact-integer sums[0], which have no k.

The suspected defect was real: mg_dtssd_bwd launches nothing for T = 1 and DtSSD.backward handed out the torch.empty buffer as the gradient; the
wrapper now allocates zeros for a one-frame slice (test_dtssd_loss_of_one_frame_is_nan_with_a_zero_gradient).

Run time on the MI355X: the 74 cases take 19 s together; the slowest are the two ConvGRU wraps (16 400 x 512 bf16 3.8 s, 8 200 x 512 fp32 2.1 s,
most of it the float64 reference on the host), every other case stays below 1 s.
"""
import contextlib
import ctypes

import pytest
import torch

import rows_reference as R
import temporal_reference as T

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@contextlib.contextmanager
def _mode(det):
    from maggie_amd import hip
    was = hip.DETERMINISTIC
    hip.set_deterministic(det)
    try:
        yield
    finally:
        hip.set_deterministic(was)


def _same_bits(a, b):
    return torch.equal(R.bits_of(a), R.bits_of(b))


def _name(dtype):
    return str(dtype).replace('torch.', '')


# ------------------------------------------------------------------------------------------------------------------
# A. ConvGRU gates
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', T.GRU_GEOMS, ids=lambda g: '%dx%d-%s' % (g[0], g[1], _name(g[2])))
def test_gru_gate_kernels(geom):
    from maggie_amd import functional as MF
    dev = _dev()
    M, C, dtype = geom
    case = T.gru_case(M, C, dtype)
    ref = T.gru(**case)
    d = {n: v.to(dev) for n, v in case.items()}
    rz, x, h = (d[n].clone().requires_grad_(True) for n in ('rz', 'x', 'h'))
    xrh = MF.GruGate.apply(rz, x, h)
    xrh.backward(d['dxrh'])
    rz2, cp, h2 = (d[n].clone().requires_grad_(True) for n in ('rz', 'cpre', 'h'))
    hn = MF.GruOut.apply(rz2, cp, h2)
    hn.backward(d['dhn'])
    got = {'xrh': xrh.detach(), 'hn': hn.detach(), 'dx': x.grad, 'dr': rz.grad[:, :C], 'dh1': h.grad, 'dz': rz2.grad[:, C:], 'dc': cp.grad,
           'dh2': h2.grad}
    for name, k in T.K_GRU.items():
        assert got[name].dtype == dtype
        R.check(got[name], ref[name][0], ref[name][1], k, dtype, 'gru ' + name)
    # the copied halves keep their bits, the half of drz a kernel does not own is exactly zero
    assert _same_bits(xrh.detach()[:, :C], case['x']) and _same_bits(x.grad, case['dxrh'][:, :C])
    assert float(rz.grad[:, C:].float().abs().max()) == 0 and float(rz2.grad[:, :C].float().abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------------
# B. eval-time alpha aggregation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', T.FUSE_PLANES)
@pytest.mark.parametrize('n_frames', T.FUSE_FRAMES)
def test_temporal_fuse(n_frames, n):
    from maggie_amd import kernels as K
    dev = _dev()
    for with_prev in (True, False):
        a, prev, df, db = T.fuse_case(n_frames, n, with_prev=with_prev)
        ref = T.fuse(a, prev, df, db)['alphas'][0]
        out = K.temporal_fuse_(a.clone().to(dev), None if prev is None else prev.to(dev), df.to(dev), db.to(dev)).cpu()
        R.exact(out, ref, 'temporal_fuse')
        keep = [0] + list(range(3, n_frames))
        assert _same_bits(out[keep], a[keep])                   # frames other than 1 and 2 keep their bits


def test_temporal_fuse_rejects_two_frames():
    from maggie_amd import hip, kernels as K
    dev = _dev()
    a = torch.rand((2, 64), device=dev)
    with pytest.raises(hip.MaggieHipError):
        K.temporal_fuse_(a, None, a.clone(), a.clone())


# ------------------------------------------------------------------------------------------------------------------
# C. bidirectional fusion
# ------------------------------------------------------------------------------------------------------------------
BIFUSE_CASES = [(Tn,) + s for Tn in T.BIFUSE_T for s in T.BIFUSE_SHAPES] + [(2,) + T.BIFUSE_WRAP]


@pytest.mark.parametrize('case', BIFUSE_CASES, ids=lambda c: 'T%d-%dx%dx%dx%d' % c)
def test_bidirectional_fusion(case):
    from maggie_amd import functional as MF
    dev = _dev()
    Tn, B, NI, H, W = case
    preds, diffs, dfused = T.bifuse_case(B, Tn, NI, H, W)
    ref = T.bifuse(preds, diffs, dfused)
    p, d = preds.to(dev).requires_grad_(True), diffs.to(dev).requires_grad_(True)
    fused, aux = MF.BiFuse.apply(p, d)
    fused.backward(dfused.to(dev))
    aux = aux.detach().cpu()
    R.check(fused.detach(), *ref['fused'], T.K_BIFUSE, F32, 'bifuse fused')
    R.check(aux[2], *ref['fsig'], T.K_BIFUSE_SIG, F32, 'bifuse fsig')
    R.check(aux[3], *ref['bsig'], T.K_BIFUSE_SIG, F32, 'bifuse bsig')
    R.check(p.grad, *ref['dpreds'], T.K_BIFUSE, F32, 'bifuse dpreds')
    R.check(d.grad, *ref['ddiffs'], T.k_bifuse_dd(NI), F32, 'bifuse ddiffs')
    # the logit stacks are the inputs bit for bit with exact zeros at frame 0 resp. T - 1, where the sigmoid stacks are exactly 0.5
    assert _same_bits(aux[0], ref['fdiff'][0].float()) and _same_bits(aux[1], ref['bdiff'][0].float())
    assert _same_bits(aux[0][:, 0], torch.zeros((B, 1, H, W))) and _same_bits(aux[1][:, Tn - 1], torch.zeros((B, 1, H, W)))
    assert bool((aux[2][:, 0] == 0.5).all()) and bool((aux[3][:, Tn - 1] == 0.5).all())
    # the first and the last fused frame are the predictions themselves
    assert _same_bits(fused.detach()[:, 0], preds[:, 0]) and _same_bits(fused.detach()[:, Tn - 1], preds[:, Tn - 1])
    if Tn == 2:
        assert float(d.grad.abs().max()) == 0


@pytest.mark.parametrize('Tn', [1, T.MAXT + 1])
def test_bidirectional_fusion_rejects_frame_counts(Tn):
    from maggie_amd import functional as MF, hip
    dev = _dev()
    preds = torch.rand((1, Tn, 1, 2, 2), device=dev)
    diffs = torch.zeros((max(2 * (Tn - 1), 1), 1, 1, 2, 2), device=dev)
    with pytest.raises(hip.MaggieHipError):
        MF.BiFuse.apply(preds, diffs)


# ------------------------------------------------------------------------------------------------------------------
# D. loss_dtSSD, E. mean BCE with logits
# ------------------------------------------------------------------------------------------------------------------
def _c(v):
    return ctypes.c_long(v)


def _dtssd_sums(p, g, m, sig_on):
    """mg_dtssd_fwd on buffers of the test's own -> sums (2,) on the device."""
    from maggie_amd import functional as MF, hip
    pp, pbs, Tn, E = MF._frames(p)
    gg, gbs, _, _ = MF._frames(g)
    mm, mbs = (None, 0) if m is None else MF._frames(m)[:2]
    sums = torch.full((2,), float('nan'), device=pp.device)
    hip.call('mg_dtssd_fwd', hip.ptr(pp), _c(pbs), hip.ptr(gg), _c(gbs), hip.ptr(mm), _c(mbs), ctypes.c_int(pp.shape[0]), ctypes.c_int(Tn), _c(E),
             ctypes.c_int(int(sig_on)), hip.ptr(sums), hip.stream())
    return sums


def _bce_sum(x, y):
    from maggie_amd import functional as MF, hip
    xx, xbs, Tn, E = MF._frames(x)
    yy, ybs, _, _ = MF._frames(y)
    s = torch.full((1,), float('nan'), device=xx.device)
    hip.call('mg_bce_logits_fwd', hip.ptr(xx), _c(xbs), hip.ptr(yy), _c(ybs), ctypes.c_int(xx.shape[0]), _c(Tn * E), hip.ptr(s), hip.stream())
    return s


def _on(case, dev):
    """The tensors of a loss case on the device (the clip requires a gradient) -> clip, (slice, gt, mask)."""
    clip = case['parent'].to(dev).requires_grad_(True)
    mask = None if case['mask'] is None else case['mask'].to(dev)
    return clip, T.loss_views(clip, case['how'], case['gt'].to(dev), mask, case['copy'])


@pytest.mark.parametrize('geom', T.LOSS_GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_dtssd_loss(geom):
    from maggie_amd import functional as MF
    dev = _dev()
    B, Tn, E = geom
    ks = T.k_dtssd(B * (Tn - 1) * E)
    gout = torch.tensor(T.GOUT, device=dev)
    for ci, combo in enumerate(T.LOSS_COMBOS):
        case = T.loss_case(B, Tn, E, combo, seed=ci)
        ref = T.dtssd(*T.loss_views(**case), combo[0])
        for det in (True, False):
            with _mode(det):
                clip, (p, g, m) = _on(case, dev)
                if combo[3]:
                    assert not g[0, 0].is_contiguous() or g.stride(1) != E       # the copy path of _frames
                loss = MF.dtssd_loss(p, g, m, sig=bool(combo[0]))
                loss.backward(gout)
                sums = _dtssd_sums(p.detach(), g, m, combo[0])
                if det:
                    assert _same_bits(_dtssd_sums(p.detach(), g, m, combo[0]), sums)
            what, ka = 'dtssd %s ' % ('det' if det else 'atomic'), 0 if det else T.atomic_k(B * E)
            R.check(sums[0], *ref['sum0'], ks['sum0'] + ka, F32, what + 'sum0')
            R.check(sums[1], *ref['sum1'], ks['sum1'] + ka, F32, what + 'sum1')
            R.check(loss.detach(), *ref['loss'], ks['loss'] + ka, F32, what + 'loss')
            R.check(T._sliced(clip.grad, case['how']), *ref['grad'], ks['grad'] + ka, F32, what + 'grad')
            if combo[1] == 'zero':
                assert float(loss.detach()) == 0 and float(clip.grad.abs().max()) == 0
    # exact integers: no element is dropped or counted twice, in either mode
    for combo in ((0, '01', 'full', 0), (0, '01', 'tail', 1)):
        case = T.loss_case(B, Tn, E, combo, integer=True)
        ref = T.dtssd(*T.loss_views(**case), 0)
        for det in (True, False):
            with _mode(det):
                _, (p, g, m) = _on(case, dev)
                sums = _dtssd_sums(p.detach(), g, m, 0)
            R.exact(sums[0], ref['sum0'][0], 'dtssd integer sum0')


def test_dtssd_loss_of_one_frame_is_nan_with_a_zero_gradient():
    """loss_dtSSD on a one-frame slice (loss_temporal_sparsity on a two-frame clip: diff_forward[:, 1:]): 0 / 0 and an all-zero gradient."""
    from maggie_amd import functional as MF
    dev = _dev()
    for sig_on in (False, True):
        for shape in ((2, 2, 1, 5000), (1, 2, 1, 7)):
            junk = torch.full(shape, float('nan'), device=dev)         # what a reused block of the allocator may hold
            del junk
            clip = torch.randn(shape, device=dev).requires_grad_(True)
            gt = torch.rand(shape, device=dev)
            loss = MF.dtssd_loss(clip[:, 1:], gt[:, 1:], None, sig=sig_on)
            loss.backward()
            assert bool(torch.isnan(loss))
            assert clip.grad.shape == clip.shape and float(clip.grad.abs().max()) == 0
            junk = torch.full((shape[0], 1) + shape[2:], float('nan'), device=dev)
            del junk
            one = torch.randn((shape[0], 1) + shape[2:], device=dev).requires_grad_(True)
            loss = MF.dtssd_loss(one, gt[:, :1], None, sig=sig_on)
            loss.backward()
            assert bool(torch.isnan(loss)) and float(one.grad.abs().max()) == 0


@pytest.mark.parametrize('geom', T.LOSS_GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_bce_logits_mean(geom):
    from maggie_amd import functional as MF
    dev = _dev()
    B, Tn, E = geom
    ks = T.k_bce(B * Tn * E)
    gout = torch.tensor(T.GOUT, device=dev)
    for ci, combo in enumerate(T.BCE_COMBOS):
        case = T.loss_case(B, Tn, E, combo, seed=ci, bce=True)
        x, y, _ = T.loss_views(**case)
        ref = T.bce(x, y)
        for det in (True, False):
            with _mode(det):
                clip, (xd, yd, _) = _on(case, dev)
                loss = MF.bce_logits_mean(xd, yd)
                loss.backward(gout)
                s = _bce_sum(xd.detach(), yd)
                if det:
                    assert _same_bits(_bce_sum(xd.detach(), yd), s)
            what, ka = 'bce %s ' % ('det' if det else 'atomic'), 0 if det else T.atomic_k(B * Tn * E)
            R.check(s[0], *ref['sum'], ks['sum'] + ka, F32, what + 'sum')
            R.check(loss.detach(), *ref['loss'], ks['loss'] + ka, F32, what + 'loss')
            R.check(T._sliced(clip.grad, case['how']), *ref['grad'], ks['grad'], F32, what + 'grad')


# ------------------------------------------------------------------------------------------------------------------
# F. bounding-box crop
# ------------------------------------------------------------------------------------------------------------------
def _crop_boxes(alpha, bits, pad, box):
    """mg_temporal_crop on buffers of the test's own (in place on alpha / bits) -> the int32 boxes the kernels left in `box`."""
    from maggie_amd import hip
    P, H, W = alpha.shape
    scratch = torch.empty_like(alpha)
    hip.call('mg_temporal_crop', hip.ptr(alpha), hip.ptr(bits), ctypes.c_int(P), ctypes.c_int(H), ctypes.c_int(W), ctypes.c_float(float(T.CROP_SIGMA)),
             ctypes.c_float(T.CROP_THR), ctypes.c_int(pad), hip.ptr(scratch), hip.ptr(box), hip.stream())
    return box.cpu()


@pytest.mark.parametrize('geom', T.CROP_GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_temporal_crop(geom):
    from maggie_amd import functional as MF
    dev = _dev()
    P, H, W = geom
    a, bits, _ = T.crop_case(P, H, W)
    smooth = T.crop_smooth(a)
    assert T.crop_undecided(*smooth) == 0
    words = T.bits_words(bits)
    box = torch.full((P, 4), 12345, dtype=torch.int32, device=dev)
    for pad in T.crop_pads(W):
        for with_bits in (True, False):
            ref = T.crop(a, bits if with_bits else None, pad, smooth=smooth)
            ad, bd = a.to(dev), words.to(dev) if with_bits else None
            MF.temporal_crop_(ad, bd, pad=pad)
            assert torch.equal(ad.cpu(), ref['alpha'][0]), (pad, with_bits)
            ad, bd = a.to(dev), words.to(dev) if with_bits else None
            assert torch.equal(_crop_boxes(ad, bd, pad, box), ref['box'][0]), (pad, with_bits)
            assert torch.equal(ad.cpu(), ref['alpha'][0])
            if with_bits:
                assert torch.equal(T.words_bits(bd, W)[:, :, :W], ref['bits'][0]), pad
    # other planes through the same box buffer: it is initialised again by every call
    a2, bits2, _ = T.crop_case(P, H, W, **T.CROP_SECOND)
    ref2 = T.crop(a2, bits2, 30)
    assert not torch.equal(ref2['box'][0], ref['box'][0]) or P == 1
    ad, bd = a2.to(dev), T.bits_words(bits2).to(dev)
    assert torch.equal(_crop_boxes(ad, bd, 30, box), ref2['box'][0])
    assert torch.equal(ad.cpu(), ref2['alpha'][0]) and torch.equal(T.words_bits(bd, W)[:, :, :W], ref2['bits'][0])


def test_temporal_crop_rejects_seven_rows():
    from maggie_amd import functional as MF, hip
    dev = _dev()
    with pytest.raises(hip.MaggieHipError):
        MF.temporal_crop_(torch.zeros((1, 1, 7, 8), device=dev), None)
