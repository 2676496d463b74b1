"""Host-side proof for tests/test_gpu_temporal.py. The float64 references of tests/temporal_reference.py equal autograd through the module's own
statements (the ConvGRU formulas, oracle/refmodel.py's bidirectional_fusion blend, gaussian_smoothing, loss_dtssd, F.binary_cross_entropy_with_logits)
and the restatements of tests/test_gpu_kernels.py; a plain fp32 evaluation of every device case passes the comparison in every storage type (no k
is tighter than honest fp32 arithmetic); every planted defect is rejected, the element-wise ones by at least 16 x k; and the cases satisfy their
preconditions (no undecided crop pixel, exact-integer bounds, both sides of the fuse kernel's disagreement test populated). No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_reference as R
import temporal_reference as T

F64, F32, BF16, F16 = T.F64, T.F32, T.BF16, T.F16
TIGHT = 1e-12
MARGIN = 16


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _worst(got, ref, ks, dtype=F32, cast=False):
    """Largest err / (u32 S k) over the outputs named in ks (k = 0: equality, reported as inf when it fails)."""
    w = 0.0
    for name, k in ks.items():
        g, (r, S) = got[name][0], ref[name]
        if cast:
            g = g.to(dtype)
        ratio = R.error_ratio(g, r, S, dtype)
        w = max(w, (ratio / k) if k else (float('inf') if ratio > 0 else 0.0))
    return w


# ------------------------------------------------------------------------------------------------------------------
# ConvGRU gates
# ------------------------------------------------------------------------------------------------------------------
def test_gru_reference_equals_autograd():
    g = torch.Generator().manual_seed(0)
    M, C = 11, 8
    rz, x, h, cp = (torch.randn((M, w), generator=g, dtype=F64).requires_grad_(True) for w in (2 * C, C, C, C))
    g1, g2 = torch.randn((M, 2 * C), generator=g, dtype=F64), torch.randn((M, C), generator=g, dtype=F64)
    r, z = torch.sigmoid(rz).split(C, -1)                       # conv_gru.py:22-27
    xrh = torch.cat([x, r * h], -1)
    hn = (1 - z) * h + z * torch.tanh(cp)
    ref = T.gru(rz.detach(), x.detach(), h.detach(), cp.detach(), g1, g2)
    assert _rel(ref['xrh'][0], xrh.detach()) < TIGHT and _rel(ref['hn'][0], hn.detach()) < TIGHT
    (xrh * g1).sum().backward(retain_graph=True)
    assert _rel(ref['dx'][0], x.grad) < TIGHT and _rel(ref['dr'][0], rz.grad[:, :C]) < TIGHT and _rel(ref['dh1'][0], h.grad) < TIGHT
    assert float(rz.grad[:, C:].abs().max()) == 0
    for t in (rz, x, h):
        t.grad = None
    (hn * g2).sum().backward()
    assert _rel(ref['dz'][0], rz.grad[:, C:]) < TIGHT and _rel(ref['dc'][0], cp.grad) < TIGHT and _rel(ref['dh2'][0], h.grad) < TIGHT
    assert float(rz.grad[:, :C].abs().max()) == 0


@pytest.mark.parametrize('geom', T.GRU_GEOMS, ids=lambda g: '%dx%d-%s' % (g[0], g[1], str(g[2]).replace('torch.', '')))
def test_gru_fp32_evaluation_is_accepted(geom):
    M, C, dtype = geom
    case = T.gru_case(M, C, dtype)
    ref = T.gru(**case)
    got = T.gru(**case, dt=F32)
    for name, k in T.K_GRU.items():
        assert R.close(got[name][0].to(dtype), ref[name][0], ref[name][1], k, dtype), name
    if dtype == F16:
        assert all(bool(torch.isfinite(v).all()) for v in case.values())


@pytest.mark.parametrize('dtype', [BF16, F16, F32])
@pytest.mark.parametrize('fault', ['swap_rz', 'z_for_1mz', 'one_minus_tc', 'drop_last_row'])
def test_gru_defects_are_rejected(fault, dtype):
    case = T.gru_case(60, 16, dtype)
    ref = T.gru(**case)
    bad = T.gru(**case, fault=fault)
    assert _worst(bad, ref, T.K_GRU, dtype, cast=True) >= MARGIN, fault
    if fault == 'z_for_1mz':                                    # the defect a max-norm tolerance of 2e-2 lets through on small elements
        assert R.error_ratio(bad['hn'][0].to(dtype), *ref['hn'], dtype) >= MARGIN * T.K_GRU['hn']
    if fault == 'one_minus_tc':
        assert R.error_ratio(bad['dc'][0].to(dtype), *ref['dc'], dtype) >= MARGIN * T.K_GRU['dc']


@pytest.mark.parametrize('geom', T.GRU_GEOMS[-2:], ids=['f32', 'bf16'])
def test_gru_unwritten_tail_past_the_grid_is_rejected(geom):
    M, C, dtype = geom
    ce = 4 if dtype == F32 else 8
    assert M * (C // ce) > T.GRID                               # the geometry wraps the grid
    row0 = T.GRID // (C // ce) - 32
    case = {n: v[row0:] for n, v in T.gru_case(M, C, dtype).items()}          # 32 rows before the wrap and the rows behind it
    ref = T.gru(**case)
    bad = T.gru(**case, fault='past_grid', ce=ce, row0=row0)
    for name in T.K_GRU:
        assert torch.equal(bad[name][0][:32], ref[name][0][:32]) and float(bad[name][0][32:].abs().max()) == 0
    assert _worst(bad, ref, T.K_GRU, dtype, cast=True) >= MARGIN


# ------------------------------------------------------------------------------------------------------------------
# eval-time alpha aggregation
# ------------------------------------------------------------------------------------------------------------------
def _fuse_restatement(a, prev, df, db):
    """tests/test_gpu_kernels.py:test_temporal_fuse_kernel."""
    last = a.shape[0] - 1
    pv = a[0] if prev is None else prev
    f, bk = (df > 0.5).float(), (db > 0.5).float()
    p01 = pv * (1 - f[1]) + a[1] * f[1]
    p21 = a[last] * (1 - bk[1]) + a[1] * bk[1]
    p01 = torch.where((p01 - p21).abs() > 0, a[1], p01)
    p12 = p01 * (1 - f[2]) + a[last] * f[2]
    out = a.clone()
    out[1], out[2] = p01, p12
    return out


@pytest.mark.parametrize('with_prev', [True, False])
@pytest.mark.parametrize('n_frames', T.FUSE_FRAMES)
def test_fuse_reference_cases_and_defects(n_frames, with_prev):
    for n in T.FUSE_PLANES[:4]:
        a, prev, df, db = T.fuse_case(n_frames, n, with_prev=with_prev)
        ref = T.fuse(a, prev, df, db)
        out = ref['alphas'][0]
        assert torch.equal(out, _fuse_restatement(a, prev, df, db).double())            # fp32 restatement: every operation is exact
        assert torch.equal(out.float().double(), out)
        half, above = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1))
        if n >= 255:
            frac = float(ref['disagree'][0].float().mean())
            assert 0.1 <= frac <= 0.9, frac                                              # both sides of the disagreement test
            for t in (df, db):
                assert bool((t[1:3] == float(half)).any()) and bool((t[1:3] == float(above)).any())
        else:
            assert float(df[1, 0]) == 0.5 and float(db[1, 0]) == float(above)
        assert not torch.equal(T.fuse(a, prev, df, db, fault='ge')['alphas'][0], out), n
        if n_frames > 3 and n >= 255:
            assert not torch.equal(T.fuse(a, prev, df, db, fault='last_is_2')['alphas'][0], out)


# ------------------------------------------------------------------------------------------------------------------
# bidirectional fusion
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tn', T.BIFUSE_T)
def test_bifuse_reference_equals_autograd_through_the_oracle(Tn, monkeypatch):
    from oracle import refmodel as rm
    B, NI, H, W = 2, 3, 4, 5
    preds, diffs, dfused = (t.double() for t in T.bifuse_case(B, Tn, NI, H, W, seed=Tn))
    diffs = diffs.clamp(-30, 30)                                # sigmoid'(+-100) underflows in float64 autograd as it does in the reference
    preds.requires_grad_(True)
    diffs.requires_grad_(True)
    order = iter([diffs[i] for i in range(2 * (Tn - 1))])       # forward pairs 1 .. T - 1, then backward pairs T - 1 .. 1
    monkeypatch.setattr(rm, 'diff_module', lambda sd, p, x, training: next(order))
    monkeypatch.setattr(rm.F, 'interpolate', lambda d, **kw: d)
    feat = torch.zeros((B, Tn, 1, H, W), dtype=F64)
    fd, bd, fused = rm.bidirectional_fusion(None, 'f', feat, preds, False)
    monkeypatch.undo()
    ref = T.bifuse(preds.detach(), diffs.detach(), dfused)
    assert _rel(ref['fused'][0], fused.detach()) < TIGHT
    assert torch.equal(ref['fdiff'][0], fd.detach()) and torch.equal(ref['bdiff'][0], bd.detach())
    assert _rel(ref['fsig'][0], fd.detach().sigmoid()) < TIGHT and _rel(ref['bsig'][0], bd.detach().sigmoid()) < TIGHT
    fused.backward(dfused)
    assert _rel(ref['dpreds'][0], preds.grad) < TIGHT
    if Tn == 2:
        assert float(ref['ddiffs'][0].abs().max()) == 0 and float(ref['ddiffs'][1].abs().max()) == 0
        assert diffs.grad is None or float(diffs.grad.abs().max()) == 0
    else:
        assert _rel(ref['ddiffs'][0], diffs.grad) < 1e-11


def _bifuse_ks(NI):
    return {'fused': T.K_BIFUSE, 'fsig': T.K_BIFUSE_SIG, 'bsig': T.K_BIFUSE_SIG, 'dpreds': T.K_BIFUSE, 'ddiffs': T.k_bifuse_dd(NI)}


def _bifuse_cases():
    return [(Tn,) + s for Tn in T.BIFUSE_T for s in T.BIFUSE_SHAPES] + [(2,) + T.BIFUSE_WRAP]


@pytest.mark.parametrize('case', _bifuse_cases(), ids=lambda c: 'T%d-%dx%dx%dx%d' % c)
def test_bifuse_fp32_evaluation_is_accepted(case):
    Tn, B, NI, H, W = case
    ops = T.bifuse_case(B, Tn, NI, H, W)
    ref, got = T.bifuse(*ops), T.bifuse(*ops, dt=F32)
    for name, k in _bifuse_ks(NI).items():
        assert R.close(got[name][0], ref[name][0], ref[name][1], k, F32), name
    assert torch.equal(got['fdiff'][0].double(), ref['fdiff'][0]) and torch.equal(got['bdiff'][0].double(), ref['bdiff'][0])


@pytest.mark.parametrize('fault', ['slot_off', 'no_half', 'avg_frame0', 'no_carry'])
def test_bifuse_defects_are_rejected(fault):
    for Tn in (5, 16):
        ops = T.bifuse_case(2, Tn, 3, 8, 24)
        ref, bad = T.bifuse(*ops), T.bifuse(*ops, fault=fault)
        assert _worst(bad, ref, _bifuse_ks(3)) >= MARGIN, (fault, Tn)


# ------------------------------------------------------------------------------------------------------------------
# loss_dtSSD and mean BCE with logits
# ------------------------------------------------------------------------------------------------------------------
def test_dtssd_and_bce_references_equal_autograd():
    from oracle import refmodel as rm
    for combo in T.LOSS_COMBOS:
        case = T.loss_case(2, 4, 37, combo)
        parent, how = case['parent'], case['how']
        _, gt, m = T.loss_views(**case)
        x = parent.double().requires_grad_(True)
        sl = T._sliced(x, how)
        pr = sl.sigmoid() if combo[0] else sl
        mm = torch.ones_like(gt.double()) if m is None else m.double()
        loss = rm.loss_dtssd(pr, gt.double(), mm)                       # maggie/network/loss.py:7-16
        (loss * T.GOUT).backward()
        ref = T.dtssd(T._sliced(parent, how), gt, m, combo[0])
        assert abs(float(ref['loss'][0]) - float(loss)) <= TIGHT * max(1.0, abs(float(loss)))
        assert float((T._sliced(x.grad, how) - ref['grad'][0]).abs().max()) <= TIGHT * max(1.0, float(x.grad.abs().max()))
        x2 = parent.double().requires_grad_(True)
        lb = F.binary_cross_entropy_with_logits(T._sliced(x2, how), gt.double(), reduction='mean')
        (lb * T.GOUT).backward()
        rb = T.bce(T._sliced(parent, how), gt)
        assert abs(float(rb['loss'][0]) - float(lb)) <= TIGHT and _rel(rb['grad'][0], T._sliced(x2.grad, how)) < TIGHT
    # one frame: NaN loss, zero gradient
    x = torch.randn((2, 1, 1, 5), dtype=F64).requires_grad_(True)
    loss = rm.loss_dtssd(x, torch.rand((2, 1, 1, 5), dtype=F64), torch.ones((2, 1, 1, 5), dtype=F64))
    loss.backward()
    ref = T.dtssd(x.detach(), torch.rand((2, 1, 1, 5)), None, 0)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(ref['loss'][0]))
    assert float(x.grad.abs().max()) == 0 and float(ref['grad'][0].abs().max()) == 0


@pytest.mark.parametrize('geom', T.LOSS_GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_loss_fp32_evaluations_are_accepted_and_integer_cases_are_exact(geom):
    B, Tn, E = geom
    n = B * (Tn - 1) * E
    for ci, combo in enumerate(T.LOSS_COMBOS):
        p, gt, m = T.loss_views(**T.loss_case(B, Tn, E, combo, seed=ci))
        ref, got = T.dtssd(p, gt, m, combo[0]), T.dtssd(p, gt, m, combo[0], dt=F32)
        for name, k in T.k_dtssd(n).items():
            assert R.close(got[name][0], ref[name][0], ref[name][1], k, F32), (combo, name)
        if combo[1] == 'zero':
            assert float(ref['loss'][0]) == 0 and float(ref['grad'][0].abs().max()) == 0
    for ci, combo in enumerate(T.BCE_COMBOS):
        x, gt, _ = T.loss_views(**T.loss_case(B, Tn, E, combo, seed=ci, bce=True))
        ref, got = T.bce(x, gt), T.bce(x, gt, dt=F32)
        for name, k in T.k_bce(B * Tn * E).items():
            assert R.close(got[name][0], ref[name][0], ref[name][1], k, F32), (combo, name)
        assert bool(((gt == 0) | (gt == 1)).all()) == (combo[0] == 0)
    for combo in ((0, '01', 'full', 0), (0, '01', 'tail', 1)):
        p, gt, m = T.loss_views(**T.loss_case(B, Tn, E, combo, integer=True))
        ref = T.dtssd(p, gt, m, 0)
        R.assert_exact_conditions(p, gt, m, partial_bound=float(ref['sum0'][0]))           # the terms are >= 0: no partial sum exceeds the total
        assert float(ref['sum0'][0]) == float(T.dtssd(p, gt, m, 0, dt=F32)['sum0'][0])


@pytest.mark.parametrize('fault', ['mask_frame0', 'stride_TE', 'gp_sign'])
def test_dtssd_defects_are_rejected(fault):
    for combo in ((0, '01', 'tail', 0), (1, 'frac', 'tail', 1)):
        p, gt, m = T.loss_views(**T.loss_case(2, 3, 257, combo))
        ref, bad = T.dtssd(p, gt, m, combo[0]), T.dtssd(p, gt, m, combo[0], fault=fault)
        assert _worst(bad, ref, T.k_dtssd(2 * 2 * 257)) >= MARGIN, (fault, combo)


@pytest.mark.parametrize('fault', ['no_xy', 'wrong_count'])
def test_bce_defects_are_rejected(fault):
    for combo in ((0, None, 'tail', 0), (1, None, 'full', 0)):
        x, gt, _ = T.loss_views(**T.loss_case(2, 3, 257, combo, bce=True))
        ref, bad = T.bce(x, gt), T.bce(x, gt, fault=fault)
        assert _worst(bad, ref, T.k_bce(2 * 3 * 257)) >= MARGIN, (fault, combo)


# ------------------------------------------------------------------------------------------------------------------
# bounding-box crop
# ------------------------------------------------------------------------------------------------------------------
def _oracle_crop(a, unk, pad):
    """tests/test_gpu_kernels.py:test_temporal_crop_matches_oracle_restatement: the oracle's fp32 smoothing and the box loop."""
    from oracle import refmodel as rm
    P, H, W = a.shape
    sm = rm.gaussian_smoothing(a[None], T.CROP_SIGMA)[0]
    ref_a, ref_u = a.clone(), unk.clone()
    boxes = []
    for j in range(P):
        ys, xs = torch.nonzero(sm[j] > T.CROP_THR, as_tuple=True)
        if len(ys) == 0:
            boxes.append(T.BOX_EMPTY)
            continue
        boxes.append([int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())])
        y0, y1 = max(0, int(ys.min()) - pad), min(int(ys.max()) + pad, H)
        x0, x1 = max(0, int(xs.min()) - pad), min(int(xs.max()) + pad, W)
        tm = torch.zeros(H, W, dtype=torch.bool)
        tm[y0:y1, x0:x1] = True
        ref_a[j] = ref_a[j] * tm
        ref_u[j] = ref_u[j] & tm
    return torch.tensor(boxes, dtype=torch.int32), ref_a, ref_u


@pytest.mark.parametrize('geom', T.CROP_GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_crop_reference_cases_and_oracle(geom):
    from oracle import refmodel as rm
    P, H, W = geom
    for kw in ({}, T.CROP_SECOND):                              # the second set: the other planes of the re-initialisation test
        a, bits, kinds = T.crop_case(P, H, W, **kw)
        val, S = T.crop_smooth(a)
        assert T.crop_undecided(val, S) == 0                    # a condition on the inputs: no pixel sits on the threshold
        sm = rm.gaussian_smoothing(a.double()[None], T.CROP_SIGMA)[0]
        assert float((sm - val).abs().max()) <= 1e-6            # the oracle forms its weights in fp32
        v32, _ = T.crop_smooth(a, dt=F32)
        assert torch.equal(v32 > T.CROP_THR, val > T.CROP_THR)  # a plain fp32 evaluation decides every pixel the same way
        for pad in T.crop_pads(W):
            ref = T.crop(a, bits, pad, smooth=(val, S))
            box, ref_a, ref_u = _oracle_crop(a, bits, pad)
            assert torch.equal(ref['box'][0], box) and torch.equal(ref['alpha'][0], ref_a) and torch.equal(ref['bits'][0], ref_u)
        box = T.crop(a, None, 0, smooth=(val, S))['box'][0]
        for p, kind in enumerate(kinds):
            empty = box[p].tolist() == T.BOX_EMPTY
            if H >= 33 or kind in ('nothing', 'full'):          # in an 8-row plane a small blob stays below the threshold
                assert empty == (kind in ('nothing', 'pixel', 'faint')), (p, kind, box[p])
        w = T.bits_words(bits)
        assert w.shape == (P, H, (W + 63) // 64) and torch.equal(T.words_bits(w, W)[:, :, :W], bits)
    if H >= 200:
        p = kinds.index('bottom')
        assert int(box[p, 0]) >= 190                            # a dropped tail of the box search moves this box


@pytest.mark.parametrize('fault', ['g_not_sq', 'gauss2d', 'ymax_inclusive', 'pad_after_clamp', 'empty_zeroed'])
def test_crop_defects_are_rejected(fault):
    differing = 0
    for (P, H, W) in T.CROP_GEOMS[1:5]:
        a, bits, _ = T.crop_case(P, H, W)
        for pad in T.crop_pads(W):
            ref, bad = T.crop(a, bits, pad), T.crop(a, bits, pad, fault=fault)
            differing += sum(int((ref[n][0] != bad[n][0]).sum()) for n in ('box', 'alpha', 'bits'))
    assert differing >= 1, fault
