"""CPU checks of the exact-integer convolution tests (tests/conv_exact.py): the comparison helper notices the smallest errors a kernel can
make, every case meets the exactness conditions on its reference alone, and every kernel form the library compiles has a case or a stated reason
for having none (the ledger)."""
import fnmatch
import os
import sys

import pytest
import torch

import conv_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(form, **match):
    for c in X.cases_by_form()[form]:
        if all(getattr(c, k) == v for k, v in match.items()):
            return c
    raise KeyError((form, match))


# three operand sets: a shallow walk, the deepest K of the table (18 slabs, K = 5184) and a split-K layer, the last two behind an epilogue
SELF_TEST = [lambda: _case('h3<8,64,3>/CONV', Cin=64, epi='plain'), lambda: _case('h3_persist<8,64,3>/CONV/res', Cin=576),
             lambda: _case('split<128>/CONV', Cin=512)]


@pytest.mark.parametrize('pick', range(len(SELF_TEST)))
def test_helper_reports_one_wrong_term_and_one_stale_vector(pick):
    c = SELF_TEST[pick]()
    assert pick != 1 or X.reduction_length(c) == max(X.reduction_length(k) for _, k in X.all_cases() if k.kind == 'fprop')
    o = X.build(c)
    for dtype in (torch.bfloat16, torch.float16):
        want = X.stored(o['ref'], dtype)
        assert X.mismatch_report(c, want.clone(), want) is None
        # one single term of one output dropped: the first output with a non-zero term at (tap 4, some channel)
        w, x = o['w'], o['x']
        co, ci = [int(v[0]) for v in (w[:, 4, :] != 0).nonzero(as_tuple=True)]
        n, y, xx = [int(v[0]) for v in (x[:, 1:-1, 1:-1, ci] != 0).nonzero(as_tuple=True)]
        y, xx = y + 1, xx + 1                                                  # an interior pixel: the centre tap of output (y, xx) reads x[y, xx]
        assert c.mode == 'CONV' and c.stride == 1 and c.pad == c.dil
        m = (n * c.H + y) * c.W + xx
        acc = o['acc'].clone()
        acc[m, co] -= x[n, y, xx, ci] * w[co, 4, ci]
        got = X.stored(X.epilogue(c, o, acc), dtype)
        rep = X.mismatch_report(c, got, want)
        assert rep is not None and rep.startswith('1 of ') and '(image %d, y %d, x %d, channel %d)' % (n, y, xx, co) in rep, rep
        # one 8-channel vector (one ds_read_b128 lane) taken from the neighbouring pixel
        x2 = x.clone()
        g = next(g for g in range(c.Cin // 8) if not torch.equal(x[0, 2, 3, 8 * g:8 * g + 8], x[0, 2, 4, 8 * g:8 * g + 8]))
        x2[0, 2, 3, 8 * g:8 * g + 8] = x[0, 2, 4, 8 * g:8 * g + 8]
        got = X.stored(X.epilogue(c, o, X.linear(c, x2, w)), dtype)
        rep = X.mismatch_report(c, got, want)
        assert rep is not None and 'elements differ' in rep and '(image 0, y ' in rep, rep


def test_helper_reports_dw_positions():
    c = _case('wgrad<64,64>/CONV', dtypes=('bf16', 'f16'))
    want = X.build(c)['ref'].float()
    got = want.clone()
    got[41, 7, 33] += 1
    rep = X.mismatch_report(c, got, want)
    assert rep.startswith('1 of ') and '(cout 41, tap 7, cin 33) cout % 64 = 41, cin % 64 = 33' in rep, rep


def _light(c):
    Ho, Wo = X.out_hw(c)
    return (c.N if c.mode == 'GATHER' else c.N * Ho * Wo) <= 20000


def test_every_light_case_meets_the_exactness_conditions():
    """The conditions hold on the reference alone (the GPU test asserts them again for every case it runs, the heavy ones included)."""
    for _, c in X.all_cases():
        if _light(c):
            for dt in c.dtypes:
                X.check_conditions(c, X.DTYPES[dt])


def test_case_ids_are_unique_and_every_case_names_its_forms():
    ids = [X.case_id(c) for _, c in X.all_cases()]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    assert all(c.forms for _, c in X.all_cases())


def _form_names():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    if not os.path.isfile(os.path.join(ROOT, 'maggie_amd', 'libmaggie_hip.so')):
        import __graft_entry__
        __graft_entry__.build()
    from maggie_amd import kernels as K
    return K.conv_form_names()


def test_form_names_are_unique_and_stable_in_shape():
    names = _form_names()
    assert len(names) == len(set(names)) and len(names) > 200
    for must in ('h3<8,64,3>/CONV/res/xf', 'h3_slab/TCONV', 'h3_persist<8,32,4>/CONV', 'halo<4,64,3>/TCONV', 'c8<8>', 'async<128,128,2,3>/GATHER',
                 'fprop<128,64,2>/TCONV/phased', 'split<128>/CONV', 'split_finish', 'wgrad_c8', 'wgrad_gather9<2>', 'wgrad_halo/xf', 'wgrad<32,64>/GATHER',
                 'reduce', 'reduce_wave', 'reduce_tile', 'reduce_batched'):
        assert must in names, must


def test_every_kernel_form_has_a_case_or_a_reason():
    """The ledger: a kernel form added to the library without an exact-integer case fails here, before any GPU run."""
    names = _form_names()
    table = X.cases_by_form()
    missing = [n for n in names if not table.get(n) and not any(fnmatch.fnmatchcase(n, pat) for pat in X.EXCLUDED)]
    assert not missing, 'kernel forms without a case in tests/conv_exact.py and without an EXCLUDED reason: %s' % missing
    unknown = [f for f in table if f not in names]
    assert not unknown, 'cases filed under names the library does not know: %s' % unknown
    for pat, why in X.EXCLUDED.items():
        assert why and any(fnmatch.fnmatchcase(n, pat) for n in names), 'EXCLUDED entry %r matches no form' % pat
        assert not any(fnmatch.fnmatchcase(f, pat) for f in table), 'EXCLUDED entry %r hides a form that has cases' % pat
