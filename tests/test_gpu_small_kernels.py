"""Direct GPU tests of the small single-launch kernels that the agents' tests reach only at
one shape each: the row-dot head backward (xa_head_bwd, gemm.hip), the TRPO helpers
(trpo.hip), the byte movers / elementwise helpers of offpolicy.hip and its TD heads, greedy
action and action noise (the arithmetic of td_terms.hpp).

Every kernel is called through the C ABI with raw pointers and compared with a numpy
float64 (or exact byte) reference of the same operation. Tolerances are bit equality, a
forward-error bound computed from the inputs (u = 2^-24, the f32 unit roundoff), or a bar the
suite already uses for the same quantity. The library is compiled with -ffp-contract=off, so
`a * x + b * y` on the device is the two-rounding f32 expression numpy evaluates: the axpby,
polyak and tanh-gradient cases are bit-exact against numpy f32 and need no ulp allowance
(largest distance observed: 0 ulp)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # f32 unit roundoff
F32 = np.float32
CANARY = F32(-7777.25)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _assert_bits_equal(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements differ, first at '
                           f'{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, '
                           f'want {want[bad][0]!r}')


def _assert_within(got, ref, bound, what=''):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{what}: max error / bound = {worst:.3g}')
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements outside the bound, '
                           f'worst error / bound = {worst:.3g}')


def _lib():
    from xagents_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------
# 1. xa_head_bwd
# ---------------------------------------------------------------------------------------------
_HB_SHAPES = [
    (1, 1, 1),        # smallest
    (15, 64, 6),      # M < HB_U
    (16, 64, 6),      # M == HB_U
    (17, 33, 8),      # one tail row after a full block of 16; A at its bound
    (250, 512, 6),    # the DQN head; M % 16 = 10
    (256, 31, 8),     # (K + 1) A = 256 exactly fills one weight block
    (33, 32, 8),      # (K + 1) A = 264 crosses a block
    (3, 4096, 2),     # K at its bound
]


def _hb_inputs(M, K, A):
    rng = np.random.default_rng(1000 * M + 10 * K + A)
    d = dict(x=rng.normal(size=(M, K)), dz=rng.normal(size=(M, A)), W=rng.normal(size=(K, A)),
             gate=rng.normal(size=(M, K)), dx0=rng.normal(size=(M, K)),
             gw0=rng.normal(size=(K, A)), gb0=rng.normal(size=A))
    d = {k: v.astype(F32) for k, v in d.items()}
    flat = d['gate'].reshape(-1)
    flat[0::7] = 0.0           # exact zeros of either sign gate off
    flat[3::7] = -0.0
    return d


def _with_canary(a, rows=2):
    """`a` followed by canary rows in one allocation."""
    a2 = a.reshape(a.shape[0], -1)
    return np.concatenate([a2, np.full((rows, a2.shape[1]), CANARY, F32)], 0)


@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('M,K,A', _HB_SHAPES)
def test_head_bwd_vs_f64_and_few_k_gemm(device, M, K, A, gated):
    """xa_head_bwd's dX is bit-identical to the few-k GEMM launch it replaced (the header's
    contract) and within (A + 1) u (sum_a |dz W| + |dx0|) of float64; its [W; b] gradient is
    within the M-term f32 chain bound (M + 1) u (sum_m |x dz| + |g0|) of float64; beta and
    accumulate start from non-zero buffers; gw = gb = NULL still writes dX and nothing else;
    the rows after every buffer stay untouched."""
    L = _lib()
    from xagents_amd.layers import gemm
    d = _hb_inputs(M, K, A)
    x, dz, W, gate = (_dev(d[k], device) for k in ('x', 'dz', 'W', 'gate'))
    gp = gate.data_ptr() if gated else None
    x64, dz64, W64 = (d[k].astype(np.float64) for k in ('x', 'dz', 'W'))
    prod = dz64[:, None, :] * W64[None, :, :]                       # [M, K, A]
    on = (d['gate'] > 0) if gated else np.ones((M, K), bool)
    dx_new = np.where(on, prod.sum(-1), 0.0)
    dx_abs = np.abs(prod).sum(-1)
    gw_new, gw_abs = x64.T @ dz64, np.abs(x64).T @ np.abs(dz64)
    gb_new, gb_abs = dz64.sum(0), np.abs(dz64).sum(0)
    ws = torch.empty(1, device=device)
    for beta in (0, 1):
        for acc in (0, 1):
            tag = f'M{M} K{K} A{A} gate{int(gated)} beta{beta} acc{acc}'
            dx = _dev(_with_canary(d['dx0']), device)
            gw = _dev(_with_canary(d['gw0']), device)
            gb = _dev(_with_canary(d['gb0'].reshape(1, A)), device)
            L.call('xa_head_bwd', x.data_ptr(), dz.data_ptr(), W.data_ptr(), gp, M, K, A,
                   dx.data_ptr(), beta, gw.data_ptr(), gb.data_ptr(), acc, L.stream())
            # the launch LayerExecutor.backward makes when XA_HEAD_BWD=0
            dx2 = _dev(d['dx0'], device)
            gemm(M, K, A, dz.data_ptr(), W.data_ptr(), dx2.data_ptr(), a_m=(1, A, 0), b_ks=1,
                 b_ns=A, ldc=K, gate=gp, ld_gate=K if gated else 0, beta=bool(beta),
                 workspace=ws)
            dxh, gwh, gbh, dx2h = _host(dx), _host(gw), _host(gb), _host(dx2)
            _assert_bits_equal(dxh[:M], dx2h, f'{tag}: dX vs the few-k GEMM')
            _assert_within(dxh[:M], beta * d['dx0'].astype(np.float64) + dx_new,
                           (A + 1) * U * (dx_abs + beta * np.abs(d['dx0'])), f'{tag}: dX')
            _assert_within(gwh[:K], acc * d['gw0'].astype(np.float64) + gw_new,
                           (M + 1) * U * (gw_abs + acc * np.abs(d['gw0'])), f'{tag}: gW')
            _assert_within(gbh[0], acc * d['gb0'].astype(np.float64) + gb_new,
                           (M + 1) * U * (gb_abs + acc * np.abs(d['gb0'])), f'{tag}: gb')
            for name, buf, n in (('dX', dxh, M), ('gW', gwh, K), ('gb', gbh, 1)):
                assert (buf[n:] == CANARY).all(), f'{tag}: wrote past the end of {name}'
            if acc == 0:
                # no parameter gradient wanted: the same dX, nothing else written
                dx3 = _dev(_with_canary(d['dx0']), device)
                L.call('xa_head_bwd', x.data_ptr(), dz.data_ptr(), W.data_ptr(), gp, M, K, A,
                       dx3.data_ptr(), beta, None, None, acc, L.stream())
                _assert_bits_equal(_host(dx3), dxh, f'{tag}: dX with gw = gb = NULL')


def test_head_bwd_refuses_bad_sizes(device):
    L = _lib()
    t = torch.zeros(64, device=device)
    p = t.data_ptr()
    for M, K, A in ((4, 4, 9), (1, 4097, 2), (0, 4, 2)):
        with pytest.raises(L.HipLibraryError, match='xa_head_bwd'):
            L.call('xa_head_bwd', p, p, p, None, M, K, A, p, 0, p, p, 0, L.stream())


_MODELS = {}


def _model(cfg, units, shape, device):
    key = (cfg, tuple(units), tuple(shape))
    if key not in _MODELS:
        from xagents_amd.nets import Adam, ModelReader
        _MODELS[key] = ModelReader(str(ROOT / 'xagents_amd' / cfg), units, shape, Adam(),
                                   seed=5, device=device).build_model()
    return _MODELS[key]


@pytest.mark.parametrize('cfg,units,shape,B', [
    ('ppo/models/cnn-actor-critic.cfg', [4, 1], (84, 84, 1), 3),    # two heads on one ReLU
    ('ppo/models/cnn-actor-critic.cfg', [4, 1], (84, 84, 1), 37),   # source: the 2nd accumulates
    ('td3/models/ann-actor.cfg', [4], (24,), 9),                    # a tanh head on a ReLU source
    ('td3/models/ann-actor.cfg', [4], (24,), 250),
    ('ppo/models/ann-actor-critic.cfg', [3, 1], (11,), 37),         # two heads on a tanh source
])
def test_head_bwd_executor_matches_gemm_path(device, monkeypatch, cfg, units, shape, B):
    """LayerExecutor.backward with XA_HEAD_BWD=1 (xa_head_bwd) against XA_HEAD_BWD=0 (the dW
    GEMM + few-k dX launches), once overwriting and once more accumulating into the same
    gradient. The input gradient into the heads' shared source is bit-identical, so every
    parameter slice below the heads is too. Each head's own [W; b] slice is held, on both
    paths, to the chain bound (B + 1) u sum_m |x dz| against float64. That reference is
    nets_f64.backward's dense-layer formula (x^T dz, 1^T dz) evaluated on the operands the
    launches read -- the device's f32 source activations and head dz -- so the bound has only
    the B-term summation to cover, not the forward pass's rounding. After the accumulating
    pass g2 = fl(g1 + chain): the first pass's error plus (B + 1) u (sum |x dz| + |g1|)."""
    from xagents_amd.layers import LayerExecutor
    model = _model(cfg, units, shape, device)
    rng = np.random.default_rng(11)
    if len(shape) == 3:
        xin = rng.integers(0, 256, size=(B, *shape), dtype=np.uint8)
    else:
        xin = rng.normal(size=(B, *shape)).astype(F32)
    xin = _dev(xin, device)
    runs = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('XA_HEAD_BWD', flag)
        ex = LayerExecutor(model, B)
        outs = ex.forward(xin)
        if flag == '0':
            douts = [_dev(rng.normal(size=tuple(o.shape)).astype(F32), device) for o in outs]
        grad = torch.full((model.n_params,), 3.0, device=device)
        ex.backward(douts, grad)
        assert ex._hb == (flag == '1')
        g1 = _host(grad).copy()
        ex.backward(douts, grad, accumulate=True)
        g2 = _host(grad).copy()
        heads = {}
        for i, dout in zip(model.outputs, douts):
            l, j = model.layers[i], ex._src_layer(i)
            assert l.kind == 'dense' and l.units <= 8 and j != -1, 'not a row-dot head'
            dz = ex.douts[i] if ex._act(i) != 0 else dout
            heads[i] = (_host(ex.outs[j]).reshape(B, -1).copy(), _host(dz).reshape(B, -1).copy(),
                        _host(ex.douts[j]).copy())
        runs[flag] = (g1, g2, heads, ex.offsets)
    (a1, a2, ha, offsets), (b1, b2, hb, _) = runs['0'], runs['1']
    head_mask = np.zeros(model.n_params, bool)
    for i, (xs, dz, dsrc) in hb.items():
        xs0, dz0, dsrc0 = ha[i]
        _assert_bits_equal(xs, xs0, f'layer {i}: source activations')
        _assert_bits_equal(dz, dz0, f'layer {i}: head dz')
        _assert_bits_equal(dsrc, dsrc0, f'layer {i}: the gradient into the shared source')
        w0, b0 = offsets[i]
        K, A = xs.shape[1], dz.shape[1]
        assert b0 == w0 + K * A
        head_mask[w0:b0 + A] = True
        x64, dz64 = xs.astype(np.float64), dz.astype(np.float64)
        ref = np.concatenate([(x64.T @ dz64).ravel(), dz64.sum(0)])
        terms = np.concatenate([(np.abs(x64).T @ np.abs(dz64)).ravel(), np.abs(dz64).sum(0)])
        for name, (p1, p2) in (('XA_HEAD_BWD=0', (a1, a2)), ('XA_HEAD_BWD=1', (b1, b2))):
            s1, s2 = p1[w0:b0 + A], p2[w0:b0 + A]
            _assert_within(s1, ref, (B + 1) * U * terms, f'{name} layer {i} [W; b]')
            _assert_within(s2, 2 * ref, (B + 1) * U * (2 * terms + np.abs(s1)),
                           f'{name} layer {i} [W; b], accumulated')
    assert head_mask.any() and not head_mask.all()
    _assert_bits_equal(b1[~head_mask], a1[~head_mask], 'parameters below the heads')
    _assert_bits_equal(b2[~head_mask], a2[~head_mask], 'parameters below the heads, accumulated')


# ---------------------------------------------------------------------------------------------
# 2. TRPO helpers
# ---------------------------------------------------------------------------------------------
def _log_softmax64(z):
    z = z.astype(np.float64)
    z = z - z.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


def _padded(a, pad, fill):
    """[n, A] values in an [n, A + pad] array whose padding columns hold `fill`."""
    out = np.full((a.shape[0], a.shape[1] + pad), fill, F32)
    out[:, :a.shape[1]] = a
    return out


def _trpo_case(n, A):
    rng = np.random.default_rng(100 * n + A)
    sd = np.sqrt(2.0)                                   # logits ~ N(0, 2): variance 2
    zn = rng.normal(scale=sd, size=(n, A)).astype(F32)
    zo = rng.normal(scale=sd, size=(n, A)).astype(F32)
    act = rng.integers(0, A, size=n).astype(np.int32)
    adv = rng.normal(size=n).astype(F32)
    return zn, zo, act, adv


def _trpo_ref(zn, zo, act, adv, c, inv_n):
    n, A = zn.shape
    lpn, lpo = _log_softmax64(zn), _log_softmax64(zo)
    pn, po = np.exp(lpn), np.exp(lpo)
    rows = np.arange(n)
    ratio = np.exp(lpn[rows, act] - lpo[rows, act])
    H = -(pn * lpn).sum(1)
    KL = (po * (lpo - lpn)).sum(1)
    ga = ratio * adv.astype(np.float64)
    onehot = np.zeros((n, A))
    onehot[rows, act] = 1.0
    # d/dz_a of [ratio adv + c H] / n:  ratio adv (1[a = act] - p_a) - c p_a (log p_a + H)
    dl = (ga[:, None] * (onehot - pn) - c * pn * (lpn + H[:, None])) * inv_n
    out = np.array([ga.mean() + c * H.mean(), KL.mean(), H.mean()])
    return out, dl, np.array([ga.sum(), KL.sum(), H.sum()])


_TRPO_N = [1, 255, 256, 257, 1000]
_TRPO_A = [2, 3, 18, 32]


@pytest.mark.parametrize('A', _TRPO_A)
@pytest.mark.parametrize('n', _TRPO_N)
def test_trpo_head_vs_f64(device, n, A):
    """xa_trpo_head with logits_new != logits_old: surrogate / mean KL / mean entropy within
    1e-5 max(1, |ref|) (test_fvp_and_surrogate_gradient_vs_f64's bar for head_out[0]), dlogits
    within 1e-5 of max |ref|; exactly xa_trpo_head_blocks(n) rows of f64 partials whose
    in-order sum times 1 / n reproduces out; NaN row padding is never read and the dlogits
    padding never written; dlogits = NULL and out = NULL variants."""
    L = _lib()
    zn, zo, act, adv = _trpo_case(n, A)
    c, inv_n = F32(0.01), F32(1.0 / n)
    ref_out, ref_dl, ref_sums = _trpo_ref(zn, zo, act, adv, float(c), float(inv_n))
    nb = L.load().xa_trpo_head_blocks(n)
    assert nb == (n + 255) // 256
    tact, tadv = _dev(act, device), _dev(adv, device)
    for pad in (0, 3):
        tzn = _dev(_padded(zn, pad, np.nan), device)
        tzo = _dev(_padded(zo, pad, np.nan), device)
        for want_dl, want_out in ((True, True), (False, True), (True, False)):
            tag = f'n{n} A{A} pad{pad} dlogits{int(want_dl)} out{int(want_out)}'
            dl = torch.full((n + 1, A + 1), float(CANARY), device=device)
            part = torch.full((nb + 1, 3), float(CANARY), device=device, dtype=torch.float64)
            out = torch.full((4,), float(CANARY), device=device)
            h = L.XaTrpoHeadArgs()
            h.n, h.n_actions = n, A
            h.logits_new, h.logits_old, h.ld_logits = tzn.data_ptr(), tzo.data_ptr(), A + pad
            h.actions, h.advantages = tact.data_ptr(), tadv.data_ptr()
            h.entropy_coef, h.inv_n = float(c), float(inv_n)
            h.dlogits, h.ld_dlogits = (dl.data_ptr() if want_dl else None), A + 1
            h.partials = part.data_ptr()
            L.call('xa_trpo_head', ctypes.byref(h), out.data_ptr() if want_out else None,
                   L.stream())
            dlh, parth, outh = _host(dl), _host(part), _host(out)
            assert (parth[nb] == float(CANARY)).all(), f'{tag}: more partial rows than blocks'
            assert np.isfinite(parth[:nb]).all()
            g = k = e = 0.0
            for b in range(nb):                      # the finalize kernel's order
                g, k, e = g + parth[b, 0], k + parth[b, 1], e + parth[b, 2]
            for q, (s, r) in enumerate(zip((g, k, e), ref_sums)):
                assert abs(s / n - r / n) <= 1e-5 * max(1.0, abs(r / n)), \
                    f'{tag}: partials column {q}: {s / n!r} vs {r / n!r}'
            if want_out:
                assert outh[3] == CANARY
                for q in range(3):
                    print(f'{tag}: out[{q}] = {outh[q]!r}, f64 {ref_out[q]!r}')
                    assert abs(outh[q] - ref_out[q]) <= 1e-5 * max(1.0, abs(ref_out[q])), \
                        f'{tag}: out[{q}] = {outh[q]!r}, f64 {ref_out[q]!r}'
                ent = F32(e * (1.0 / n))
                mine = [F32(F32(g * (1.0 / n)) + c * ent), F32(k * (1.0 / n)), ent]
                _assert_bits_equal(outh[:3], np.array(mine, F32), f'{tag}: out vs sum(partials) / n')
            else:
                assert (outh == CANARY).all(), f'{tag}: out = NULL was written'
            if want_dl:
                err = np.abs(dlh[:n, :A] - ref_dl).max()
                print(f'{tag}: dlogits max error {err:.3g}, max |ref| {np.abs(ref_dl).max():.3g}')
                assert err <= 1e-5 * np.abs(ref_dl).max(), tag
                assert (dlh[:n, A] == CANARY).all() and (dlh[n] == CANARY).all(), \
                    f'{tag}: dlogits padding written'
            else:
                assert (dlh == CANARY).all(), f'{tag}: dlogits = NULL was written'


@pytest.mark.parametrize('A', [1, 33])
def test_trpo_head_refuses_bad_action_counts(device, A):
    L = _lib()
    t = torch.zeros(256, device=device)
    h = L.XaTrpoHeadArgs()
    h.n, h.n_actions = 4, A
    h.logits_new = h.logits_old = h.actions = h.advantages = h.partials = t.data_ptr()
    h.ld_logits = h.ld_dlogits = A
    h.entropy_coef, h.inv_n = 0.01, 0.25
    with pytest.raises(L.HipLibraryError, match='xa_trpo_head'):
        L.call('xa_trpo_head', ctypes.byref(h), t.data_ptr(), L.stream())


@pytest.mark.parametrize('A', _TRPO_A)
@pytest.mark.parametrize('n', _TRPO_N)
def test_categorical_fisher_vs_f64(device, n, A):
    """scale (diag(p) - p p^T) t with strided logits / tangent / out, within 1e-5 of max |ref|;
    every output row sums to 0 (the metric's null direction) within A u sum |terms|, the terms
    being the 2 A products scale p_a t_a and scale p_a (p . t) the row sum is made of."""
    L = _lib()
    rng = np.random.default_rng(7 * n + A)
    z = rng.normal(scale=np.sqrt(2.0), size=(n, A)).astype(F32)
    t = rng.normal(size=(n, A)).astype(F32)
    scale = F32(1.0 / n)
    tz, tt = _dev(_padded(z, 3, np.nan), device), _dev(_padded(t, 2, np.nan), device)
    out = torch.full((n + 1, A + 1), float(CANARY), device=device)
    L.call('xa_categorical_fisher', tz.data_ptr(), A + 3, tt.data_ptr(), A + 2, n, A,
           float(scale), out.data_ptr(), A + 1, L.stream())
    oh = _host(out)
    p = np.exp(_log_softmax64(z))
    t64 = t.astype(np.float64)
    pt = (p * t64).sum(1, keepdims=True)
    ref = float(scale) * (p * (t64 - pt))
    err = np.abs(oh[:n, :A] - ref).max()
    print(f'n{n} A{A}: max error {err:.3g}, max |ref| {np.abs(ref).max():.3g}')
    assert err <= 1e-5 * np.abs(ref).max()
    assert (oh[:n, A] == CANARY).all() and (oh[n] == CANARY).all(), 'padding written'
    terms = float(scale) * (p * (np.abs(t64) + np.abs(pt))).sum(1)
    _assert_within(oh[:n, :A].astype(np.float64).sum(1), 0.0, A * U * terms,
                   f'n{n} A{A}: row sums')


def _vec_dot(L, x, y, device):
    tx, ty = _dev(x, device), _dev(y, device)
    out = torch.full((2,), float(CANARY), device=device, dtype=torch.float64)
    L.call('xa_vec_dot', tx.data_ptr(), ty.data_ptr(), x.size, out.data_ptr(), L.stream())
    o = _host(out)
    assert o[1] == float(CANARY)
    return o[0]


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 70001])
def test_vec_dot_vs_f64(device, n):
    """The f64-accumulated dot product: each f32 x f32 product is exact in f64, so the error
    is that of an n-term f64 sum, at most n 2^-53 sum |x y|; two launches agree bit for bit."""
    L = _lib()
    rng = np.random.default_rng(n)
    x, y = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    got = _vec_dot(L, x, y, device)
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    ref = np.dot(xl, yl)
    bound = n * 2.0 ** -53 * float(np.abs(xl * yl).sum())
    print(f'n{n}: error {abs(float(got - ref)):.3g}, bound {bound:.3g}')
    assert abs(float(got - ref)) <= bound
    again = _vec_dot(L, x, y, device)
    assert np.float64(got).tobytes() == np.float64(again).tobytes(), 'not deterministic'


def test_vec_dot_cancellation_is_exact(device):
    """x = [1e8, 1, -1e8, ...] against ones: a thread's stride of 1024 = 1 (mod 3) walks all
    three values, so an f32 accumulator (ulp 8 at 1e8) would lose every 1; f64 keeps them."""
    L = _lib()
    n = 3 * 1367
    x = np.tile(np.array([1e8, 1.0, -1e8], F32), n // 3)
    y = np.ones(n, F32)
    assert _vec_dot(L, x, y, device) == float(n // 3)


@pytest.mark.parametrize('n', [1, 257, 4096 * 256 + 5])
def test_axpby_bit_exact_and_aliased(device, n):
    """out = a x + b y, bit-identical to numpy's two-rounding f32 expression (the library is
    built without fma contraction, so no ulp allowance is needed or made), including one past
    the 4096-block grid cap; `out is x` and `out is y` (the CG's calls) give the same values."""
    L = _lib()
    rng = np.random.default_rng(n)
    x, y = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    a0, b0 = (F32(v) for v in rng.normal(size=2))
    for a, b in ((a0, b0), (F32(0), b0), (a0, F32(0))):
        ref = a * x + b * y
        assert ref.dtype == F32
        for alias in (None, 'x', 'y'):
            tx, ty = _dev(_with_canary(x.reshape(n, 1)), device), _dev(y, device)
            out = {None: torch.full((n + 2,), float(CANARY), device=device), 'x': tx,
                   'y': ty}[alias]
            L.call('xa_axpby', float(a), tx.data_ptr(), float(b), ty.data_ptr(),
                   out.data_ptr(), n, L.stream())
            oh = _host(out).reshape(-1)
            _assert_bits_equal(oh[:n], ref, f'n{n} a{a} b{b} out is {alias}')
            if alias != 'y':
                assert (oh[n:] == CANARY).all()


@pytest.mark.parametrize('eps', [0.0, 1e-8])
@pytest.mark.parametrize('n', [2, 1023, 1025, 5000])
def test_normalized_advantages_vs_f64(device, n, eps):
    """((ret - val) - mean) / (std + eps), population std, on differences with a mean of 100
    (E[d^2] - mean^2 loses digits), at test_fvp_and_surrogate_gradient_vs_f64's rtol / atol."""
    L = _lib()
    rng = np.random.default_rng(n)
    ret = (100.0 + rng.normal(size=n)).astype(F32)
    val = (0.5 * rng.normal(size=n)).astype(F32)
    adv = torch.full((n + 1,), float(CANARY), device=device)
    tret, tval = _dev(ret, device), _dev(val, device)
    L.call('xa_normalized_advantages', tret.data_ptr(), tval.data_ptr(), n, float(eps),
           adv.data_ptr(), L.stream())
    ah = _host(adv)
    d = ret.astype(np.float64) - val
    ref = (d - d.mean()) / (d.std() + eps)
    np.testing.assert_allclose(ah[:n], ref, rtol=1e-4, atol=1e-5)
    assert ah[n] == CANARY


def test_normalized_advantages_constant_input(device):
    """Variance exactly 0 with eps = 1e-8: finite zeros, not NaN."""
    L = _lib()
    n = 1025
    ret, val = np.full(n, 100.3, F32), np.full(n, 0.2, F32)
    adv = torch.full((n,), float(CANARY), device=device)
    tret, tval = _dev(ret, device), _dev(val, device)
    L.call('xa_normalized_advantages', tret.data_ptr(), tval.data_ptr(), n, 1e-8,
           adv.data_ptr(), L.stream())
    ah = _host(adv)
    assert np.isfinite(ah).all() and (ah == 0).all()


# ---------------------------------------------------------------------------------------------
# 3. byte movers and elementwise helpers
# ---------------------------------------------------------------------------------------------
_ITEM_BYTES = [1, 4, 15, 16, 17, 48, 7056, 4096 * 16 + 16, 64 * 256 * 16 + 32]
_SLOTS, _ITEMS, _TAIL = 7, 5, 64


def _byte_buffer(data, off, device, tail=_TAIL):
    """`data` (uint8) at byte offset `off` inside a larger device tensor, `tail` canary bytes
    after it. Returns (whole tensor, pointer to the data)."""
    whole = np.full(off + data.size + tail, 0xA5, np.uint8)
    whole[off:off + data.size] = data.reshape(-1)
    t = _dev(whole, device)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _check_bytes(t, off, want, what):
    h = _host(t)
    np.testing.assert_array_equal(h[off:off + want.size], want.reshape(-1), err_msg=what)
    assert (h[:off] == 0xA5).all() and (h[off + want.size:] == 0xA5).all(), \
        f'{what}: bytes outside the buffer written'


# (ring offset, batch offset): 16-byte aligned; both misaligned by 4, where item sizes that
# are multiples of 16 must take the byte path; only the batch side misaligned
_OFFSETS = [(0, 0), (4, 4), (0, 4)]


@pytest.mark.parametrize('ring_off,batch_off', _OFFSETS)
@pytest.mark.parametrize('ib', _ITEM_BYTES)
def test_ring_gather_scatter_exact(device, ib, ring_off, batch_off):
    L = _lib()
    rng = np.random.default_rng(ib)
    ring = rng.integers(0, 256, size=(_SLOTS, ib), dtype=np.uint8)
    # gather with a repeated slot
    slots = np.array([3, 0, 3, 6, 1], np.int64)
    tring, pring = _byte_buffer(ring, ring_off, device)
    tdst, pdst = _byte_buffer(np.full((_ITEMS, ib), 0xA5, np.uint8), batch_off, device)
    ts = _dev(slots, device)
    L.call('xa_ring_gather', pring, pdst, ts.data_ptr(), _ITEMS, ib, L.stream())
    _check_bytes(tdst, batch_off, ring[slots], f'gather ib={ib}')
    _check_bytes(tring, ring_off, ring, f'gather ib={ib}: the ring')
    # scatter through a permutation; the other slots keep their bytes
    slots = np.array([5, 2, 0, 6, 3], np.int64)
    src = rng.integers(0, 256, size=(_ITEMS, ib), dtype=np.uint8)
    tsrc, psrc = _byte_buffer(src, batch_off, device)
    ts = _dev(slots, device)
    L.call('xa_ring_scatter', psrc, pring, ts.data_ptr(), _ITEMS, ib, L.stream())
    want = ring.copy()
    want[slots] = src
    _check_bytes(tring, ring_off, want, f'scatter ib={ib}')
    _check_bytes(tsrc, batch_off, src, f'scatter ib={ib}: the source')


@pytest.mark.parametrize('sizes', [
    (7056, 4, 4, 4, 7056),                     # a C3 batch: frames, action, reward, done, frames
    (48, 17, 4, 1, 64 * 256 * 16 + 32),        # the grid is sized by the last field; the blocks
])                                             # past the 1-byte field's end must write nothing
def test_ring_gather_fields_exact(device, sizes):
    L = _lib()
    rng = np.random.default_rng(sum(sizes))
    slots = np.array([3, 0, 3, 6, 1], np.int64)
    ts = _dev(slots, device)
    g = L.XaGatherArgs()
    g.n_fields, g.n_items, g.slots = len(sizes), _ITEMS, ts.data_ptr()
    rings, bufs = [], []
    for f, ib in enumerate(sizes):
        ring = rng.integers(0, 256, size=(_SLOTS, ib), dtype=np.uint8)
        tring, pring = _byte_buffer(ring, 0, device)
        tdst, pdst = _byte_buffer(np.full((_ITEMS, ib), 0xA5, np.uint8), 0, device)
        g.field[f].ring, g.field[f].dst, g.field[f].item_bytes = pring, pdst, ib
        rings.append(ring)
        bufs.append((tring, tdst))
    L.call('xa_ring_gather_fields', ctypes.byref(g), L.stream())
    for f, (ring, (tring, tdst)) in enumerate(zip(rings, bufs)):
        _check_bytes(tdst, 0, ring[slots], f'field {f} ({sizes[f]} B)')
        _check_bytes(tring, 0, ring, f'field {f}: the ring')
    for bad in (0, 9):
        g.n_fields = bad
        with pytest.raises(L.HipLibraryError, match='xa_ring_gather_fields'):
            L.call('xa_ring_gather_fields', ctypes.byref(g), L.stream())


@pytest.mark.parametrize('rows,cols,ld_src,ld_dst', [
    (1, 1, 1, 1), (7, 5, 9, 5), (300, 28, 28, 32),
    (8192 * 256 // 64 + 3, 64, 70, 64),        # past the 8192-block grid cap
])
def test_copy_block_exact(device, rows, cols, ld_src, ld_dst):
    L = _lib()
    rng = np.random.default_rng(rows + cols)
    src = rng.normal(size=(rows, ld_src)).astype(F32)
    dst = torch.full((rows + 2, ld_dst), float(CANARY), device=device)
    tsrc = _dev(src, device)
    L.call('xa_copy_block', tsrc.data_ptr(), ld_src, dst.data_ptr(), ld_dst, rows, cols,
           L.stream())
    want = np.full((rows + 2, ld_dst), CANARY, F32)
    want[:rows, :cols] = src[:, :cols]
    _assert_bits_equal(_host(dst), want, 'copy_block')
    _assert_bits_equal(_host(tsrc), src, 'copy_block: the source')


_BIG = 8192 * 256 + 9      # past the 8192-block grid cap: the grid-stride loop's second pass


@pytest.mark.parametrize('n', [1, 255, _BIG])
def test_polyak_exact(device, n):
    """dst = (1 - tau) dst + tau src, bit-identical to numpy f32 (no fma contraction in the
    build, so no ulp allowance); tau = 1 is a copy, tau = 0 leaves dst as it is."""
    L = _lib()
    rng = np.random.default_rng(n)
    x, y = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    tx = _dev(x, device)
    for tau in (F32(1.0), F32(0.005), F32(0.0)):
        ty = _dev(_with_canary(y.reshape(n, 1)), device)
        L.call('xa_polyak', tx.data_ptr(), ty.data_ptr(), n, float(tau), L.stream())
        want = x if tau == 1 else (F32(1.0) - tau) * y + tau * x
        yh = _host(ty).reshape(-1)
        _assert_bits_equal(yh[:n], want, f'polyak n{n} tau{tau}')
        assert (yh[n:] == CANARY).all()
    _assert_bits_equal(_host(tx), x, 'polyak: the source')


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('act', ['relu', 'tanh', 'none'])
@pytest.mark.parametrize('n', [1, 257, _BIG])
def test_activation_grad_exact(device, n, act, in_place):
    """dz = dy act'(y), out of place and in place (dz is dy, as LayerExecutor.jvp / backward
    call it). ReLU: y = +0, -0 gate off, a positive denormal passes. tanh: bit-identical to
    numpy f32 dy (1 - y y) (no fma contraction in the build, so no ulp allowance)."""
    L = _lib()
    code = {'none': L.XA_ACT_NONE, 'relu': L.XA_ACT_RELU, 'tanh': L.XA_ACT_TANH}[act]
    rng = np.random.default_rng(n)
    y, dy = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    if act == 'tanh':
        y = np.tanh(y).astype(F32)
    if act == 'relu':
        y[0::5] = 0.0
        y[1::5] = -0.0
        y[2::5] = 1e-40                        # a positive f32 denormal
        assert n < 3 or 0 < y[2] < np.finfo(F32).tiny
    want = {'none': dy, 'relu': np.where(y > 0, dy, F32(0.0)),
            'tanh': dy * (F32(1.0) - y * y)}[act]
    ty = _dev(y, device)
    tdy = _dev(_with_canary(dy.reshape(n, 1)), device)
    tdz = tdy if in_place else torch.full((n + 2,), float(CANARY), device=device)
    L.call('xa_activation_grad', ty.data_ptr(), tdy.data_ptr(), n, code, tdz.data_ptr(),
           L.stream())
    zh = _host(tdz).reshape(-1)
    _assert_bits_equal(zh[:n], want.astype(F32), f'{act} n{n} in_place{int(in_place)}')
    assert (zh[n:] == CANARY).all()
    _assert_bits_equal(_host(ty), y, 'y')
    if not in_place:
        _assert_bits_equal(_host(tdy).reshape(-1)[:n], dy, 'dy')


# ---------------------------------------------------------------------------------------------
# 4. the off-policy TD heads, the greedy action and the action noise (csrc/td_terms.hpp)
# ---------------------------------------------------------------------------------------------
_TD_B = 70                 # one full 64-thread block and a ragged one
_DELTA = F32(0.5)


def _np_td_term(e, delta):
    """td_terms.hpp td_term in f32 numpy, one rounding per operation in its order."""
    if delta > 0:
        d = np.minimum(np.maximum(e, -delta), delta)
        ae = np.abs(e)
        return d, np.where(ae <= delta, F32(0.5) * (e * e), delta * (ae - F32(0.5) * delta))
    return F32(2.0) * e, e * e


def _exact_error_rows(B):
    """(values, targets' rewards) for the first rows of a batch whose samples are done, so
    y = r exactly: errors v - r of 0, +-0.25, +-0.5 (= delta exactly) and +-0.75."""
    e = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75], F32)
    r = np.array([1.0, -2.0, 0.25, 3.5, -0.75, 2.0, 0.5], F32)
    assert e.size <= B
    return r + e, r


@pytest.mark.parametrize('huber', [F32(0.0), _DELTA])
@pytest.mark.parametrize('twin', [False, True])
def test_critic_td_grad_exact(device, twin, huber):
    """xa_critic_td_grad, single (DDPG) and twin (TD3), MSE and Huber(0.5): dv1, dv2 and the
    per-sample loss bit-identical to the f32 numpy restatement of td_terms.hpp (nothing is
    contracted in the build). Dones of 0 and 1, errors on both sides of +-delta and exactly
    on it; the rows after every output stay untouched."""
    L = _lib()
    B = _TD_B
    rng = np.random.default_rng(17 + 2 * int(twin))
    v1, v2, tv1, tv2, rew = (rng.normal(size=B).astype(F32) for _ in range(5))
    done = (rng.random(B) < 0.3).astype(F32)
    gamma = F32(0.99)
    ve, re_ = _exact_error_rows(B)
    k = ve.size
    v1[:k], rew[:k], done[:k] = ve, re_, 1.0
    v2[:k] = (re_ - (ve - re_))                       # the mirrored errors for the twin
    assert (done == 0).any() and (done == 1).any()
    tv = np.minimum(tv1, tv2) if twin else tv1
    y = rew + ((F32(1.0) - done) * gamma) * tv
    assert y.dtype == F32 and ((np.abs(v1 - y) == _DELTA).any())
    assert (np.abs(v1 - y) < _DELTA).any() and (np.abs(v1 - y) > _DELTA).any()
    d1, loss = _np_td_term(v1 - y, huber)
    if twin:
        d2, l2 = _np_td_term(v2 - y, huber)
        loss = loss + l2
    t = {n: _dev(a, device) for n, a in dict(v1=v1, v2=v2, tv1=tv1, tv2=tv2, rew=rew,
                                             done=done).items()}
    out = {n: torch.full((B + 2,), float(CANARY), device=device) for n in ('dv1', 'dv2', 'loss')}
    L.call('xa_critic_td_grad', t['v1'].data_ptr(), t['v2'].data_ptr() if twin else None,
           t['tv1'].data_ptr(), t['tv2'].data_ptr() if twin else None, t['rew'].data_ptr(),
           t['done'].data_ptr(), B, float(gamma), float(huber), out['dv1'].data_ptr(),
           out['dv2'].data_ptr() if twin else None, out['loss'].data_ptr(), L.stream())
    tag = f'twin{int(twin)} huber{huber}'
    h = {n: _host(b) for n, b in out.items()}
    _assert_bits_equal(h['dv1'][:B], d1.astype(F32), f'{tag}: dv1')
    _assert_bits_equal(h['loss'][:B], loss.astype(F32), f'{tag}: loss')
    if twin:
        _assert_bits_equal(h['dv2'][:B], d2.astype(F32), f'{tag}: dv2')
    else:
        assert (h['dv2'] == CANARY).all()
    for n, b in h.items():
        assert (b[B:] == CANARY).all(), f'{tag}: wrote past the end of {n}'


def _dqn_rows(B, A, seed):
    """Q rows with tied maxima (pairs and whole rows) among random ones."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(B, A)).astype(F32)
    q[0::5, 2] = q[0::5, 1] = q[0::5].max(1) + F32(0.5)     # the maximum at 1 and 2
    q[3::10] = F32(0.25)                                    # every entry tied
    return q


@pytest.mark.parametrize('huber', [F32(0.0), _DELTA])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('A', [3, 6])
def test_dqn_td_grad_exact(device, A, double, huber):
    """xa_dqn_td_grad, plain and double, MSE and Huber(0.5): dq (zero off the action) and the
    per-sample loss bit-identical to the f32 numpy restatement of td_terms.hpp. Tied maxima in
    the online next-state rows (the first index selects the target value), done rows, errors
    on both sides of +-delta and exactly on it. The optimizer step counter goes up by exactly
    1 when passed and nothing is bumped when it is NULL."""
    L = _lib()
    B = _TD_B
    rng = np.random.default_rng(100 * A + 2 * int(double))
    q = rng.normal(size=(B, A)).astype(F32)
    qt = rng.normal(size=(B, A)).astype(F32)
    qo = _dqn_rows(B, A, A)
    act = rng.integers(0, A, size=B).astype(np.int32)
    rew = rng.normal(size=B).astype(F32)
    done = (rng.random(B) < 0.3).astype(F32)
    gamma = F32(0.99)
    ve, re_ = _exact_error_rows(B)
    k = ve.size
    rew[:k], done[:k] = re_, 1.0
    q[np.arange(k), act[:k]] = ve
    rows = np.arange(B)
    if double:
        best = np.argmax(qo, 1)                        # numpy: the first maximum
        assert (best[0::5] == 1).all() and (best[3::10] == 0).all()
        assert (qt[0::5, 1] != qt[0::5, 2]).all()      # the second index would show
        v = qt[rows, best]
    else:
        v = qt.max(1)
    v = np.where(done != 0, F32(0.0), v)
    y = v * gamma + rew
    diff = y - q[rows, act]
    assert diff.dtype == F32 and (np.abs(diff) == _DELTA).any()
    assert (np.abs(diff) < _DELTA).any() and (np.abs(diff) > _DELTA).any()
    d, l = _np_td_term(diff, huber)
    want_dq = np.zeros((B, A), F32)
    want_dq[rows, act] = -d / F32(A)
    want_l = (l / F32(A)).astype(F32)
    t = {n: _dev(a, device) for n, a in dict(q=q, qt=qt, qo=qo, act=act, rew=rew,
                                             done=done).items()}
    step = torch.full((2,), 7, dtype=torch.int32, device=device)
    tag = f'A{A} double{int(double)} huber{huber}'
    for with_step in (True, False):
        dq = _dev(_with_canary(np.full((B, A), CANARY, F32)), device)
        loss = torch.full((B + 2,), float(CANARY), device=device)
        L.call('xa_dqn_td_grad', t['q'].data_ptr(), t['qt'].data_ptr(),
               t['qo'].data_ptr() if double else None, t['act'].data_ptr(),
               t['rew'].data_ptr(), t['done'].data_ptr(), B, A, float(gamma), float(huber),
               dq.data_ptr(), loss.data_ptr(), step.data_ptr() if with_step else None,
               L.stream())
        dqh, lh = _host(dq), _host(loss)
        _assert_bits_equal(dqh[:B], want_dq, f'{tag}: dq')
        _assert_bits_equal(lh[:B], want_l, f'{tag}: loss')
        assert (dqh[B:] == CANARY).all() and (lh[B:] == CANARY).all()
        assert _host(step).tolist() == [8, 7], f'{tag}: adam_step (passed: {with_step})'


@pytest.mark.parametrize('A', [3, 6])
def test_dqn_act_first_argmax_and_random(device, A):
    """xa_dqn_act: the first index of each row's maximum (tied pairs, rows tied throughout),
    and with use_random the given actions (q is not needed then)."""
    L = _lib()
    n = _TD_B
    q = _dqn_rows(n, A, 7 * A)
    want = np.argmax(q, 1).astype(np.int32)
    assert (want[0::5] == 1).all() and (want[3::10] == 0).all()
    tq = _dev(q, device)
    given = np.random.default_rng(A).integers(0, A, size=n).astype(np.int32)
    tg = _dev(given, device)
    for use_random, ref in ((0, want), (1, given)):
        out = torch.full((n + 2,), -5, dtype=torch.int32, device=device)
        L.call('xa_dqn_act', None if use_random else tq.data_ptr(), n, A, tg.data_ptr(),
               use_random, out.data_ptr(), L.stream())
        oh = _host(out)
        np.testing.assert_array_equal(oh[:n], ref)
        assert (oh[n:] == -5).all()
    np.testing.assert_array_equal(_host(tg), given)


_NA_ROWS, _NA_COLS, _NA_LDX, _NA_LDO = 5, 3, 5, 4
_NA_CTR, _NA_SEED = (3 << 32) | 5, (0x9E3779B9 << 32) | 0x7F4A7C15


def _np_philox_normal(rows, cols, ctr, seed):
    """td_terms.hpp philox_normal at (row, col, ctr, seed) in float64: u1, u2 formed exactly
    from the oracle's Philox words, the angle rounded to f32 as the kernel's product is."""
    import oracle
    out = np.zeros((rows, cols))
    for b in range(rows):
        for a in range(cols):
            r = oracle.philox([b, a, ctr & 0xffffffff, ctr >> 32],
                              [seed & 0xffffffff, seed >> 32])
            u1 = (float(int(r[0]) >> 8) + 1.0) * 2.0 ** -24
            u2 = float(int(r[1]) >> 8) * 2.0 ** -24
            angle = float(F32(6.283185307179586) * F32(u2))
            out[b, a] = np.sqrt(-2.0 * np.log(u1)) * np.cos(angle)
    return out


def _noisy(L, device, x, sigma, clip, lo, hi, ctr):
    tx = _dev(x, device)
    out = torch.full((_NA_ROWS + 1, _NA_LDO), float(CANARY), device=device)
    noise = torch.full((_NA_ROWS + 1, _NA_COLS), float(CANARY), device=device)
    L.call('xa_noisy_actions', tx.data_ptr(), _NA_LDX, _NA_ROWS, _NA_COLS, float(sigma),
           float(clip), float(lo), float(hi), ctr.data_ptr() if ctr is not None else None,
           _NA_SEED, out.data_ptr(), _NA_LDO, noise.data_ptr(), L.stream())
    oh, nh = _host(out), _host(noise)
    assert (oh[_NA_ROWS:] == CANARY).all() and (oh[:, _NA_COLS:] == CANARY).all()
    assert (nh[_NA_ROWS:] == CANARY).all()
    _assert_bits_equal(_host(tx), x, 'noisy_actions: the input')
    return oh[:_NA_ROWS, :_NA_COLS], nh[:_NA_ROWS]


def test_noisy_actions_vs_philox_f64(device):
    """xa_noisy_actions on 5 x 3 with leading dimensions wider than the columns: the stored
    noise against sigma N(0, 1) from the oracle's Philox at the same (row, col, counter, seed)
    in float64, at test_fused_step_actions_vs_f64's atol for this path; out is exactly
    clip(x + stored noise, lo, hi) in f32. With a finite noise_clip no stored element exceeds
    it and some sit exactly on it. sigma = 0 stores exact zeros whatever the counter holds
    (or without one)."""
    L = _lib()
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, size=(_NA_ROWS, _NA_LDX)).astype(F32)
    sigma, lo, hi = F32(0.2), F32(-1.0), F32(1.0)
    ctr = _dev(np.array([_NA_CTR], np.int64), device)
    normal = _np_philox_normal(_NA_ROWS, _NA_COLS, _NA_CTR, _NA_SEED)
    assert normal.std() > 0.5
    xs = x[:, :_NA_COLS]
    for clip in (F32(np.inf), F32(0.1)):
        out, nz = _noisy(L, device, x, sigma, clip, lo, hi, ctr)
        raw = normal * float(sigma)
        np.testing.assert_allclose(nz, np.clip(raw, -float(clip), float(clip)), rtol=0,
                                   atol=1e-5)
        _assert_bits_equal(out, np.minimum(np.maximum(xs + nz, lo), hi), f'clip {clip}: out')
        if np.isfinite(clip):
            over = np.abs(raw) > float(clip) + 1e-4
            assert over.any() and (~over).any()
            assert (np.abs(nz) <= clip).all() and (np.abs(nz[over]) == clip).all()
    assert int(_host(ctr)[0]) == _NA_CTR                 # the kernel only reads the counter
    other = _dev(np.array([_NA_CTR + 1], np.int64), device)
    for c in (ctr, other, None):
        out, nz = _noisy(L, device, x, F32(0.0), F32(0.1), lo, hi, c)
        _assert_bits_equal(nz, np.zeros((_NA_ROWS, _NA_COLS), F32), 'sigma 0: noise')
        _assert_bits_equal(out, np.minimum(np.maximum(xs, lo), hi), 'sigma 0: out')
