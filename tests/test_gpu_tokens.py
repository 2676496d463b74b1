"""The instance-token kernels against float64, element by element: the token <-> feature cross attention (csrc/attention.hip), the token-side
linear layers, the token self-attention and the mask pre-processing mg_imd_prep (csrc/token_side.hip), at the shapes where their code takes another
path -- one feature row, a row count at / next to a workgroup boundary (16 rows forward, 64 backward and in tok_ctx_kernel), the widest id table
(64), one batch element, the LDS and the global form of the self-attention, every K / N class of the linear layers, both kernel forms of the mask
pre-processing. The references, the sensitivities S, the k constants and the case builders live in tests/tokens_reference.py;
tests/test_tokens_reference_cpu.py proves on the host that the comparison |got - ref| <= u32 k S accepts plain float32 torch at k / 2 and rejects
eleven planted faults by 16 x k. Every backward runs in both summation modes (ordered slots and atomics). Exact-integer inputs are compared bit for
bit (the linear layers without LayerNorm, dx_pair, the einsum additions, the mask pre-processing).

Measured err / (u32 S) on the MI355X (largest over all cases of this file and both summation modes) and the k in use (tokens_reference.k_* / K_*,
written down before the run; sum(n) = ceil(log2 n) + 8; L = feature rows, D = dot-product width, T = tokens, R = token rows):

    output                         measured   k
    attn_tok p                       0.27     K_SCORE 16 + K_SOFTMAX 8 + sum(L)                     (33 .. 42)
    attn_tok ctx                     0.10     k(p) + 1 + sum(L)                                     (43 .. 61)
    attn_tok dfeat                   0.45     K_G 14 + 1 + sum(L) + 3 [dS] + 1 + sum(2 T)           (41 .. 50)
    attn_tok dqk                     0.26     k(dS) + 1 + sum(L)                                    (37 .. 55)
    attn_tok dbtab                   0.29     k(dS) + sum(L)                                        (36 .. 54)
    attn_feat p                      0.33     K_FEAT_P 36 = K_SCORE + K_SOFTMAX + sum(T)
    attn_feat out                    0.81     K_FEAT_OUT 49 = K_FEAT_P + 1 + sum(T + 1)
    attn_feat dfeat                  0.26     K_FEAT_DFEAT 41 = K_FEAT_DS 28 + 1 + sum(T)
    attn_feat dkq                    0.25     K_FEAT_DS 28 + 1 + sum(L)                             (38 .. 47)
    attn_feat dvp                    0.94     1 + sum(L)                                            (10 .. 19)
    attn_feat db2                    0.25     K_FEAT_DS 28 + sum(L)                                 (37 .. 46)
    attn_feat dob                    0.58     sum(B L)                                              (9 .. 19)
    token_sa p                       0.47     sum(D) + 1 + K_SOFTMAX 8 + sum(T)                     (28 .. 37)
    token_sa out                     0.29     k(p) + 1 + sum(T)                                     (38 .. 50)
    token_sa dq / dk                 0.43 / 0.28     sum(D) + 1 + sum(T) + 3 [dS] + 1 + sum(T)      (33 .. 45)
    token_sa dv                      2.08     1 + sum(T)                                            (10 .. 13)
    token_linear y, z (no LN: y)     1.96, 1.77      sum(K) + 3                                     (13 .. 19)
    token_linear y with LayerNorm    below the above  sum(K) + 3 + K_LN_Y 44
    token_linear mean / rstd         0.22 / 0.35     sum(K) + 3 + K_LN_MEAN 16 / K_LN_RSTD 40
    token_linear dx                  2.01     [K_LN_DZ 32 +] 1 + sum(N)                             (10 .. 49)
    token_linear dW                  1.83     [K_LN_DZ 32 +] 2 + sum(R)                             (11 .. 50)
    token_linear db                  0.63     [K_LN_DZ 32 +] sum(R)                                 (9 .. 48)
    token_linear dres                1.16     K_LN_DZ 32 (without LayerNorm: dy itself, k = 1)
    token_linear dgamma / dbeta      1.11 / 0.90     sum(R) + K_XHAT 3 / sum(R)                     (12 .. 19 / 9 .. 16)
    token_linear wt y / dx / dW      1.71 / 1.62 / 1.60     as above
    dx_pair dx                       0.96     1 + sum(N1) + 1 + sum(N2) = 29
    dx_pair dW / db                  1.58 / 0.59     2 + sum(R) = 14 / sum(R) = 12

No k was raised after the run: every measured ratio is below 2.1, every k is the operation count written down beforehand (6 x to 600 x above the
measurement; the large factors belong to the chains through the softmax and the LayerNorm, whose S already carries the condition of the chain).
The exact-integer comparisons (token_linear y / dx / dW / db without LayerNorm, dx_pair, the einsum additions) and mg_imd_prep have no k.

With the library built from the parent commit, test_dx_pair_matches_float64_and_repeats[96-*] fails (err / (u32 S) = 3.4e6: elements of dx carry the
second layer's term twice); K = 64, 128 and 132 pass there, and all four pass with the injective thread map of token_linear_bwd_rows.

Run time on the MI355X: the 146 cases take 20 s together. The three child processes of the compiled-forms test take 6.2 s, every other case stays
below 0.7 s (most: 0.1 s, float64 reference included).
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rows_reference as R
import tokens_reference as TR
import token_forms_worker

pytestmark = pytest.mark.gpu
F32 = torch.float32
MODES = [pytest.param(True, id='slots'), pytest.param(False, id='atomics')]


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


_CACHE = {}


def _memo(key, build):
    """A case and its mode-independent references are built once and shared by the summation modes."""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _check(got, ref, k, what):
    R.check(got, ref[0], ref[1], k, F32, what)


def _bits(t):
    return R.bits_of(t)


# ------------------------------------------------------------------------------------------------------------------
# cross attention
# ------------------------------------------------------------------------------------------------------------------
def _ids_mode(ci):
    return {2: 'skip', 6: 'one'}.get(ci, 'random')       # (2, 16, 11): id 5 has no row; (5, 129, 2): every row on id 1


def _attn_refs(ci):
    B, L, NID = TR.ATTN_CASES[ci]
    c = TR.attn_case(B, L, NID, ids_mode=_ids_mode(ci))
    assert int(c['ids'].min()) >= 0 and int(c['ids'].max()) < NID            # an id outside the table would be an out-of-bounds read
    refs = {'tok': TR.attn_tok_fwd(c['qk'], c['btab'], c['feat'], c['ids'], c['scale'])}
    for tn in (False, True):
        b2 = c['b2'].transpose(1, 2).contiguous() if tn else c['b2']
        refs[tn] = TR.attn_feat_fwd(c['feat'], c['kq'], b2, c['vp'], c['obias'] if _want_bias(ci, tn) else None, c['pads'][(ci + tn) % 3], c['ids'],
                                    c['scale'], tn)
    return c, refs


def _want_bias(ci, tn):
    return bool((ci // 2 + tn) % 2)


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('ci', range(len(TR.ATTN_CASES)), ids=['%dx%dx%d' % c for c in TR.ATTN_CASES])
def test_cross_attention_matches_float64(ci, det):
    """mg_attn_tok_fwd / _bwd and mg_attn_feat_fwd_ex / _bwd_ex (T = 10, D = 128): every output against float64. dp is present in the even cases;
    the padding mask cycles through none / one valid token / a different count per batch element, the table layout (tn) runs both ways in every case
    and the output bias alternates. An id that no row uses leaves exactly 0 in both bias-table gradients."""
    from maggie_amd import kernels as K
    dev = _dev()
    B, L, NID = TR.ATTN_CASES[ci]
    c, refs = _memo(('attn', ci), lambda: _attn_refs(ci))
    d = {n: (v.to(dev) if torch.is_tensor(v) else v) for n, v in c.items()}
    unused = [i for i in range(NID) if not bool((c['ids'] == i).any())]
    assert (_ids_mode(ci) == 'random') or unused
    with _mode(det):
        p, ctx = K.attn_tok_fwd(d['qk'], d['btab'], d['feat'], d['ids'], c['scale'])
        _check(p, refs['tok']['p'], TR.k_tok_p(L), 'attn_tok p')
        _check(ctx, refs['tok']['ctx'], TR.k_tok_ctx(L), 'attn_tok ctx')
        dp = c['dp'] if ci % 2 == 0 else None
        dqk, dbtab, dfeat = K.attn_tok_bwd(p, d['feat'], d['qk'], d['ids'], d['dctx'], None if dp is None else dp.to(dev), c['scale'], NID)
        b = TR.attn_tok_bwd(p, c['feat'], c['qk'], c['ids'], c['dctx'], dp, c['scale'], NID)
        _check(dfeat, b['dfeat'], TR.k_tok_dfeat(L), 'attn_tok dfeat')
        _check(dqk, b['dqk'], TR.k_tok_dqk(L), 'attn_tok dqk')
        _check(dbtab, b['dbtab'], TR.k_tok_dbtab(L), 'attn_tok dbtab')
        for i in unused:
            assert not _bits(dbtab[:, :, i]).any(), 'dbtab of the unused id %d' % i
        for tn in (False, True):
            pad = c['pads'][(ci + tn) % 3]
            bias = _want_bias(ci, tn)
            b2 = d['b2'].transpose(1, 2).contiguous() if tn else d['b2']
            out, p2 = K.attn_feat_fwd(d['feat'], d['kq'], b2, d['vp'], d['obias'] if bias else None, None if pad is None else pad.to(dev), d['ids'],
                                      c['scale'], tn)
            _check(out, refs[tn]['out'], TR.K_FEAT_OUT, 'attn_feat out')
            _check(p2, refs[tn]['p'], TR.K_FEAT_P, 'attn_feat p')
            if pad is not None:
                assert not _bits(p2)[pad.bool()[:, None, :].expand(B, L, TR.T_TOK)].any(), 'probability of a padded token'
            got = dict(zip(('dfeat', 'dkq', 'dvp', 'db2', 'dob'), K.attn_feat_bwd(d['dout'], p2, d['feat'], d['kq'], d['vp'], d['ids'], c['scale'], NID, bias, tn)))
            b = TR.attn_feat_bwd(c['dout'], p2, c['feat'], c['kq'], c['vp'], c['ids'], c['scale'], NID, bias, tn)
            ks = {'dfeat': TR.K_FEAT_DFEAT, 'dkq': TR.k_feat_dkq(L), 'dvp': TR.k_feat_dvp(L), 'db2': TR.k_feat_db2(L), 'dob': TR.k_feat_dob(B * L)}
            assert (got['dob'] is not None) == bias
            for name, ref in b.items():
                _check(got[name], ref, ks[name], 'attn_feat ' + name)
            for i in unused:
                assert not _bits(got['db2'][:, :, i] if tn else got['db2'][:, i]).any(), 'db2 of the unused id %d' % i


@pytest.mark.parametrize('T,D,NID', [(9, 128, 3), (10, 64, 3), (10, 128, 65)])
def test_cross_attention_refuses_what_it_is_not_built_for(T, D, NID):
    """T != 10, D != 128 and NID > 64 (the dynamic LDS is sized for 64 ids) are refused by the host check, without a launch."""
    from maggie_amd import kernels as K
    from maggie_amd.hip import MaggieHipError
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)                   # noqa: E731
    ids = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    with pytest.raises(MaggieHipError):
        K.attn_tok_fwd(z(1, T, D), z(1, T, NID), z(1, 4, D), ids, 0.1)
    with pytest.raises(MaggieHipError):
        K.attn_tok_bwd(z(1, T, 4), z(1, 4, D), z(1, T, D), ids, z(1, T, D), None, 0.1, NID)
    with pytest.raises(MaggieHipError):
        K.attn_feat_fwd(z(1, 4, D), z(1, T, D), z(1, NID, T), z(1, T, D), None, None, ids, 0.1)
    with pytest.raises(MaggieHipError):
        K.attn_feat_bwd(z(1, 4, D), z(1, 4, T), z(1, 4, D), z(1, T, D), z(1, T, D), ids, 0.1, NID, False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# token self-attention
# ------------------------------------------------------------------------------------------------------------------
def _sa_refs(si):
    c = TR.sa_case(*TR.SA_CASES[si])
    return c, [TR.token_sa_fwd(c['q'], c['k'], c['v'], pad) for pad in c['pads']]


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('si', range(len(TR.SA_CASES)), ids=['%dx%dx%d' % c for c in TR.SA_CASES])
def test_token_self_attention_matches_float64(si, det):
    """mg_token_sa_fwd / _bwd: the LDS form (D <= 128 and T D <= 2048) and the global-memory form (D = 256, D = 132), without a mask, with one valid
    token and with a different count per batch element."""
    from maggie_amd import functional as MF
    dev = _dev()
    B, T, D = TR.SA_CASES[si]
    c, refs = _memo(('sa', si), lambda: _sa_refs(si))
    with _mode(det):
        for pad, ref in zip(c['pads'], refs):
            q, k, v = (c[n].to(dev).requires_grad_(True) for n in 'qkv')
            out = MF.token_self_attention(q, k, v, None if pad is None else pad.to(dev))
            prob = out.grad_fn.saved_tensors[3]
            _check(out, ref['out'], TR.k_sa_out(T, D), 'token_sa out')
            _check(prob, ref['p'], TR.k_sa_p(T, D), 'token_sa p')
            if pad is not None:
                assert not _bits(prob)[pad[:, None, :].expand(B, T, T)].any(), 'probability of a padded token'
            b = TR.token_sa_bwd(c['dout'], c['q'], c['k'], c['v'], prob)
            out.backward(c['dout'].to(dev))
            _check(q.grad, b['dq'], TR.k_sa_dqk(T, D), 'token_sa dq')
            _check(k.grad, b['dk'], TR.k_sa_dqk(T, D), 'token_sa dk')
            _check(v.grad, b['dv'], TR.k_sa_dv(T), 'token_sa dv')


# ------------------------------------------------------------------------------------------------------------------
# token linear
# ------------------------------------------------------------------------------------------------------------------
class _LN:
    def __init__(self, gamma, beta, eps, dev):
        self.weight, self.bias, self.eps = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True), eps


def _run_linear(c, relu, wt, dev, integer, what):
    """One layer through MF.token_linear, forward and backward, against the reference (integer: bit for bit where there is no LayerNorm)."""
    from maggie_amd import functional as MF
    ln = c['gamma'] is not None
    R_, K = c['x'].shape
    N = c['dy'].shape[1]
    t = {n: (None if c[n] is None else c[n].to(dev).requires_grad_(True)) for n in ('x', 'W', 'b', 'xadd', 'res')}
    norm = _LN(c['gamma'], c['beta'], c['eps'], dev) if ln else None
    y = MF.token_linear(t['x'], t['W'], t['b'], xadd=t['xadd'], res=t['res'], relu=relu, ln=norm, wt=wt)
    saved = y.grad_fn.saved_tensors                               # (x, xadd, W, yout, gamma, z, rstat)
    f = TR.token_linear_fwd(c['x'], c['W'], c['b'], c['xadd'], c['res'], relu, c['gamma'], c['beta'], c['eps'], wt)
    st = {}
    if ln:
        z, rstat = saved[5], saved[6]
        st = dict(z=z, mean=rstat[:, 0], rstd=rstat[:, 1])
        _check(z, f['z'], TR.k_tl_lin(K), what + ' z')
        _check(st['mean'], f['mean'], TR.k_tl_stat(K, 'mean'), what + ' mean')
        _check(st['rstd'], f['rstd'], TR.k_tl_stat(K, 'rstd'), what + ' rstd')
    exact = integer and not ln
    if exact:
        R.assert_exact_conditions(c['x'], c['W'], c['dy'], *[c[n] for n in ('b', 'xadd', 'res') if c[n] is not None], partial_bound=8 * 4 * max(K, N, R_) + 8)
        R.exact(y, f['y'][0], what + ' y (integers)')
    else:
        _check(y, f['y'], TR.k_tl_y(K, ln), what + ' y')
    y.backward(c['dy'].to(dev))
    b = TR.token_linear_bwd(c['dy'], c['x'], c['W'], c['xadd'], c['b'] is not None, c['res'] is not None, y if relu else None, c['gamma'], wt=wt, **st)
    got = {'dx': t['x'].grad, 'dW': t['W'].grad, 'db': None if t['b'] is None else t['b'].grad, 'dres': None if t['res'] is None else t['res'].grad,
           'dgamma': norm.weight.grad if ln else None, 'dbeta': norm.bias.grad if ln else None}
    ks = {'dx': TR.k_tl_dx(N, ln), 'dW': TR.k_tl_dw(R_, ln), 'db': TR.k_tl_db(R_, ln), 'dres': max(TR.k_tl_dz(ln), 1), 'dgamma': TR.k_tl_dgamma(R_),
          'dbeta': TR.k_tl_dbeta(R_)}
    assert {n for n, g in got.items() if g is not None} == set(b)
    for name, ref in b.items():
        if exact:
            R.exact(got[name], ref[0], '%s %s (integers)' % (what, name))
        else:
            _check(got[name], ref, ks[name], '%s %s' % (what, name))
    if t['xadd'] is not None:
        assert torch.equal(_bits(t['xadd'].grad), _bits(t['x'].grad))


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('xadd,bias,res,relu,ln', TR.TL_OPTIONS, ids=['proj-res-ln', 'relu', 'plain', 'bias', 'bias-ln', 'xadd'])
@pytest.mark.parametrize('case', TR.TL_CASES, ids=['%dx%dx%d' % c for c in TR.TL_CASES])
def test_token_linear_matches_float64(case, xadd, bias, res, relu, ln, det):
    """mg_token_linear_fwd_ex / _bwd_ex: y = LN(res + act((x + xadd) W^T + b)) and every gradient, with normal and with small-integer operands (the
    latter bit for bit where no LayerNorm follows). K below / between / above the 64 and 128 thread-map classes, N up to 256, 33 rows for the
    32-row chunks of the column pass, 130 rows for many row blocks."""
    dev = _dev()
    R_, K, N = case
    with _mode(det):
        for integer in (False, True):
            c = _memo(('tl', case, xadd, bias, res, ln, integer), lambda: TR.tl_case(R_, K, N, xadd, bias, res, ln, integer=integer))
            _run_linear(c, relu, False, dev, integer, 'token_linear')


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('xadd', [False, True])
@pytest.mark.parametrize('case', [(5, 96, 100), (9, 256, 64)], ids=['5x96x100', '9x256x64'])
def test_token_linear_untransposed_weight_matches_float64(case, xadd, det):
    """wt = True: W given as (K, N), dW comes back as (K, N)."""
    dev = _dev()
    R_, K, N = case
    with _mode(det):
        for integer in (False, True):
            c = TR.tl_case(R_, K, N, xadd, False, False, False, integer=integer, wt=True)
            _run_linear(c, False, True, dev, integer, 'token_linear wt')


def test_token_linear_refuses_a_layer_beyond_its_lds():
    """K = N = 256 needs 4 (K + N) + K (N + 1) floats = 265 KB of LDS forward: refused (the limit is 150 KB), forward and backward."""
    from maggie_amd import functional as MF, kernels as K
    from maggie_amd.hip import MaggieHipError
    dev = _dev()
    x, W = torch.zeros(2, 256, device=dev, requires_grad=True), torch.zeros(256, 256, device=dev, requires_grad=True)
    with pytest.raises(MaggieHipError):
        MF.token_linear(x, W)
    dz, dx, dW = torch.zeros(2, 256, device=dev), torch.empty(2, 256, device=dev), torch.empty(256, 256, device=dev)
    with pytest.raises(MaggieHipError):
        K.hip.call('mg_token_linear_bwd_ex', K.hip.ptr(dz), K.hip.ptr(x), None, K.hip.ptr(W), None, K.c_int(0), None, None, None, K.hip.ptr(dx), K.hip.ptr(dW),
                   None, None, None, None, K.hip.ptr(dz), K.c_int(2), K.c_int(256), K.c_int(256), K.c_int(0), K.hip.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('K', TR.PAIR_K)
def test_dx_pair_matches_float64_and_repeats(K, det):
    """mg_token_linear_multi_bwd with dx_pair: two plain layers of unequal N read the same x, the kernel forms ONE input gradient dy1 W1 + dy2 W2.
    Against float64, bit for bit on integers, and the same bits from 8 calls on the same inputs. K = 96 is where the thread map of
    token_linear_bwd_rows left surplus threads (64 < K < 128) that owned elements of the accumulating pass twice."""
    from maggie_amd import functional as MF
    dev = _dev()
    R_, N1, N2 = 9, 40, 24
    with _mode(det):
        for integer in (False, True):
            a = TR.tl_case(R_, K, N1, False, True, False, False, integer=integer)
            b = TR.tl_case(R_, K, N2, False, False, False, False, seed=1, integer=integer)
            x = a['x'].to(dev).requires_grad_(True)
            W1, b1, W2 = (t.to(dev).requires_grad_(True) for t in (a['W'], a['b'], b['W']))
            y1, y2 = MF.token_linear_multi([dict(x=x, W=W1, b=b1), dict(x=x, W=W2)])
            assert y1.grad_fn is y2.grad_fn and y1.grad_fn.pairs == {0: 1}                      # one launch, and the pair is armed
            loss = (y1 * a['dy'].to(dev)).sum() + (y2 * b['dy'].to(dev)).sum()
            runs = [torch.autograd.grad(loss, [x, W1, b1, W2], retain_graph=True) for _ in range(8)]
            dx, dW1, db1, dW2 = runs[0]
            ref, S = TR.pair_dx(a['dy'], a['W'], b['dy'], b['W'])
            r1 = TR.token_linear_bwd(a['dy'], a['x'], a['W'], has_b=True)
            r2 = TR.token_linear_bwd(b['dy'], a['x'], b['W'])
            if integer:
                R.assert_exact_conditions(a['x'], a['W'], b['W'], a['dy'], b['dy'], partial_bound=16 * (N1 + N2 + K + R_))
                R.exact(dx, ref, 'dx_pair dx (integers)')
                R.exact(dW1, r1['dW'][0], 'dx_pair dW1 (integers)')
                R.exact(db1, r1['db'][0], 'dx_pair db1 (integers)')
                R.exact(dW2, r2['dW'][0], 'dx_pair dW2 (integers)')
            else:
                R.check(dx, ref, S, TR.k_tl_dx(N1, False, N2), F32, 'dx_pair dx')
                _check(dW1, r1['dW'], TR.k_tl_dw(R_, False), 'dx_pair dW')
                _check(db1, r1['db'], TR.k_tl_db(R_, False), 'dx_pair db')
                _check(dW2, r2['dW'], TR.k_tl_dw(R_, False), 'dx_pair dW')
            for i, run in enumerate(runs[1:]):
                for name, g0, g in zip(('dx', 'dW1', 'db1', 'dW2'), runs[0], run):
                    assert torch.equal(_bits(g0), _bits(g)), 'K = %d: %s of call %d differs from call 0' % (K, name, i + 1)


# ------------------------------------------------------------------------------------------------------------------
# mask pre-processing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ii', range(len(TR.IMD_CASES)), ids=['-'.join(str(v) for v in c) for c in TR.IMD_CASES])
def test_imd_prep_matches_the_restatement(ii):
    """mg_imd_prep through kernels.imd_prep (the binding the decoder uses): instance-id position, token validity and ground-truth guidance, bit for
    bit against the numpy restatement, for the planes form (gs = 8, s = 1 | 2) and the generic form."""
    from maggie_amd import kernels as K
    dev = _dev()
    case = TR.IMD_CASES[ii]
    B, NF, n_in, n_gt, n_i, h, w, s, gs = case
    mask, gt = TR.imd_case(*case, seed=ii)
    want_ids, want_guid, want_valid = TR.imd_prep(mask.numpy(), None if gt is None else gt.numpy(), h, w, n_i)
    ids, guid, valid = K.imd_prep(mask.to(dev), None if gt is None else gt.to(dev), h, w, n_i)
    assert ids.dtype == torch.int32 and valid.dtype == torch.uint8 and tuple(valid.shape) == (B, n_i)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    assert (guid is None) == (gt is None)
    if gt is not None:
        assert np.array_equal(guid.cpu().numpy().view(np.uint32), want_guid.view(np.uint32))
        assert 0 < want_guid.mean() < 1
    if n_in:
        assert 0 < want_valid.sum() < want_valid.size and len(np.unique(want_ids)) > 1          # the case is not degenerate


# ------------------------------------------------------------------------------------------------------------------
# token einsum: one row, one row past a workgroup, junk in the gradient's padding columns
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('L', [1, 257])
def test_token_einsum_edges_and_gradient_padding(L, det):
    """mg_token_einsum_fwd / _bwd in fp32 on small integers, bit for bit: L = 1 and L = 257 (one row past a 256-row workgroup), and finite non-zero
    junk in the columns Q .. 15 of the incoming gradient, which must reach neither dfeat nor dtok."""
    from maggie_amd import functional as MF
    dev = _dev()
    B, Q, C = 2, 10, 32
    g = torch.Generator().manual_seed(L)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()                 # noqa: E731
    feat, tok, dlog = ri(B, L, C), ri(B, Q, C), ri(B, L, 16)
    dlog[..., Q:] = torch.where(dlog[..., Q:] == 0, torch.full_like(dlog[..., Q:], 3.0), dlog[..., Q:]) * 1024        # junk: finite, never zero
    R.assert_exact_conditions(feat, tok, dlog, partial_bound=4 * 4096 * max(C, L))          # |junk| 4096 x |feat| 4 over L rows: the discarded sums are exact too
    with _mode(det):
        fd, td = feat.to(dev).requires_grad_(True), tok.to(dev).requires_grad_(True)
        out = MF.token_einsum(fd, td)
        R.exact(out[..., :Q], torch.einsum('bqc,blc->blq', tok.double(), feat.double()), 'token_einsum out')
        assert not _bits(out[..., Q:]).any()
        out.backward(dlog.to(dev))
        d = dlog[..., :Q].double()
        R.exact(fd.grad, torch.einsum('blq,bqc->blc', d, tok.double()), 'token_einsum dfeat')
        R.exact(td.grad, torch.einsum('blq,blc->bqc', d, feat.double()), 'token_einsum dtok')


# ------------------------------------------------------------------------------------------------------------------
# the other compiled forms
# ------------------------------------------------------------------------------------------------------------------
def test_other_compiled_forms_give_the_bits_of_the_default_forms(tmp_path):
    """MG_ATTN_FWD_RG = 2 | 4 (rows per 16-lane group of the forward row passes), MG_TOKEN_SA_LDS = 0 (the global-memory self-attention) and
    MG_IMD_PREP_PLANES = 0 (the generic mask pre-processing) are read once per process: three fresh child processes, one after the other, run the
    forward cases of token_forms_worker.py and must return the bits this process gets from the default forms."""
    _dev()
    for name in ('MG_ATTN_FWD_RG', 'MG_TOKEN_SA_LDS', 'MG_IMD_PREP_PLANES'):
        assert name not in os.environ, '%s is set: this process does not run the default forms' % name
    with _mode(True):
        mine = token_forms_worker.outputs()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'token_forms_worker.py')
    for i, env in enumerate([{'MG_ATTN_FWD_RG': '2'}, {'MG_ATTN_FWD_RG': '4'}, {'MG_TOKEN_SA_LDS': '0', 'MG_IMD_PREP_PLANES': '0'}]):
        path = str(tmp_path / ('forms%d.npz' % i))
        pr = subprocess.run([sys.executable, worker, path], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
        assert pr.returncode == 0 and 'DONE' in pr.stdout, (env, pr.returncode, pr.stderr[-3000:])
        theirs = np.load(path)
        assert set(theirs.files) == set(mine)
        for name in sorted(mine):
            a, b = mine[name], theirs[name]
            assert a.shape == b.shape and a.dtype == b.dtype, (env, name)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s: %s differs from the default form' % (env, name)
