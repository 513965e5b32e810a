"""GPU: the LayerNorm kernels of ``hf_ln.hip`` through the C ABI against the float64 references of ``ln_refs.py``, each
within the bound counted from the kernel file's arithmetic chains (derived, not measured); guarded outputs, operands in
NaN-filled buffers, every launch twice with the same bits.  Tangent, adjoint and the column sums receive ``xhat``,
``rstd``, ``y`` (``s``, ``g_a``) as given -- the references' values rounded to fp32 -- so the mask is the same on both sides
and no entry is left out of a comparison.  Per-column vectors sit 4 bytes off the 16-byte grid."""

import pytest
import torch

import guarded as gd
import ln_refs
from layer_refs import ratio
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
EPS = float(torch.tensor(1e-5))  # (exact in fp32: the kernel and the reference see the same number)
SCALE = 0.375                    # (exact in fp32)
ERR_ALIGN = -2                   # HF_ERR_ALIGN of include/hf_pcg.h
# (rows, c, splits): a constant row | element loads, a partial group of four rows | one quad, slab sum | more than one quad
# per lane, a ragged last quad position | top of the wave form | bottom of the LDS form | the LDS limit | the row limit
SHAPES = [(1, 1, 1), (5, 6, 1), (3, 4, 3), (7, 260, 2), (2, 1024, 1), (2, 1028, 2), (1, 16384, 1), (256, 8, 1)]


@pytest.mark.parametrize("act", [0, 1, 2], ids=["identity", "relu", "tanh"])
@pytest.mark.parametrize("shape", SHAPES, ids=gd._ids)
def test_kernels_against_float64(shape, act):
    rows, c, splits = shape
    lib, L = _lib.load(), ln_refs.chain(c)
    gen = torch.Generator().manual_seed(7 * c + rows + splits + act)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    a, ta, gy = rnd(splits, rows, c), rnd(splits, rows, c), rnd(splits, rows, c)
    gamma, beta = rnd(c), rnd(c)
    b = None if shape == (5, 6, 1) else rnd(c)                           # the Linear bias absent once
    vb, vg, vbe = (None,) * 3 if shape == (3, 4, 3) else (rnd(c), rnd(c), rnd(c))  # frozen parameters once
    if b is None and act == 1:  # the last row is constant (exactly: one slab, no bias)
        a[0, -1] = 3.25
    stride = -(-rows * c // 4) * 4 + gd.SLAB_GAP
    a_d, ta_d, gy_d = (gd.slabs_dev(t.reshape(splits, -1), stride) for t in (a, ta, gy))
    vec = lambda t: gd.ip(None if t is None else t.numpy(), 1)  # noqa: E731
    gamma_i, beta_i, b_i, vb_i, vg_i, vbe_i = (vec(t) for t in (gamma, beta, b, vb, vg, vbe))
    dims = (rows, c, gd.F32, gd.st())

    def fwd():
        out = gd.RowOut(rows, c), gd.RowOut(rows, c), gd.FlatOut(rows)
        assert lib.hf_ln_act_forward(out[0].ptr, out[1].ptr, out[2].ptr, gd.p(a_d), splits, stride, gd.pp(b_i), gamma_i.ptr,
                                     beta_i.ptr, EPS, act, *dims) == 0
        return out

    y, xh, rstd = gd.twice(fwd)
    fw, R = ln_refs.forward(a, b, gamma, beta, EPS, act), ln_refs.r_forward(splits, b is not None, L)
    assert ratio(rstd.val, fw.rstd, fw.Mrstd, R.rstd) <= 1
    assert ratio(xh.val, fw.xh, fw.Mxh, R.xh) <= 1
    assert ratio(y.val, fw.y, fw.My, R.y) <= 1
    if c == 1 or (b is None and act == 1):  # a constant row: xhat = 0, rstd = 1/sqrt(eps), exactly
        assert float(rstd.val[-1]) == float((1.0 / torch.tensor(EPS, dtype=torch.float64).sqrt()).float())
        assert not bool(xh.val[-1].any())

    # ---- tangent and adjoint: xhat, rstd and y as given (the reference's values, rounded to fp32) ------------------------
    xh32, rstd32, y32 = fw.xh.float(), fw.rstd.float(), fw.y.float()
    xh_i, rstd_i, y_i = (gd.In(t.numpy(), 0) for t in (xh32, rstd32, y32))

    def tan():
        out = gd.RowOut(rows, c)
        assert lib.hf_ln_act_tangent(out.ptr, gd.p(ta_d), splits, stride, gd.pp(vb_i), xh_i.ptr, rstd_i.ptr, gamma_i.ptr,
                                     gd.pp(vg_i), gd.pp(vbe_i), y_i.ptr, act, *dims) == 0
        return out

    want, M = ln_refs.tangent(ta, vb, xh32, rstd32, gamma, vg, vbe, y32, act)
    assert ratio(gd.twice(tan).val, want, M, ln_refs.r_tangent(splits, vb is not None, L, act)) <= 1

    def adj():
        out = gd.RowOut(rows, c), gd.RowOut(rows, c)
        assert lib.hf_ln_act_adjoint(out[0].ptr, out[1].ptr, gd.p(gy_d), splits, stride, xh_i.ptr, rstd_i.ptr, gamma_i.ptr,
                                     y_i.ptr, act, *dims) == 0
        return out

    ga, s = gd.twice(adj)
    ad, R = ln_refs.adjoint(gy, xh32, rstd32, gamma, y32, act), ln_refs.r_adjoint(splits, L, act)
    assert ratio(s.val, ad.s, ad.Ms, R.s) <= 1
    assert ratio(ga.val, ad.ga, ad.Mga, R.ga) <= 1

    # ---- the column launch, both modes: s and g_a as given; one output absent once -----------------------------------------
    s32, ga32 = ad.s.float(), ad.ga.float()
    s_i, ga_i = gd.In(s32.numpy(), 0), gd.In(ga32.numpy(), 0)
    for squared in (0, 1):
        def sums():
            out = gd.FlatOut(c, off=1), (None if shape == (7, 260, 2) else gd.FlatOut(c, off=2)), gd.FlatOut(c, off=3)
            assert lib.hf_ln_param_sums(*(gd.optr(o) for o in out), s_i.ptr, xh_i.ptr, ga_i.ptr, squared, SCALE,
                                        *dims) == 0
            return out

        for got, (wanted, Mw) in zip(gd.twice(sums), ln_refs.param_sums(s32, xh32, ga32, SCALE, squared)):
            assert got is None or ratio(got.val, wanted, Mw, 4 + squared) <= 1


def _codes(lib, rows, c, splits=1, dtype=gd.F32, off=0, null=False):
    """The four entry points' return codes; row maps ``off`` floats behind a 16-byte boundary, ``null``: a required one absent."""
    z, w = torch.zeros(1 << 15, device=gd.DEV), torch.ones(1 << 15, device=gd.DEV)
    o = torch.empty(5, 1 << 15, device=gd.DEV)
    m, v = gd.P(z.data_ptr() + 4 * off), gd.p(w)
    src = None if null else m
    g_a, s, t_y, y, xh = (gd.P(o[i].data_ptr() + 4 * off) for i in range(5))
    stride, tail = -(-rows * c // 4) * 4, (rows, c, dtype, gd.st())
    codes = [lib.hf_ln_act_forward(y, xh, gd.p(o[4, -64:]), src, splits, stride, v, v, v, EPS, 1, *tail),
             lib.hf_ln_act_tangent(t_y, src, splits, stride, v, m, v, v, v, v, m, 1, *tail),
             lib.hf_ln_act_adjoint(g_a, s, src, splits, stride, m, v, v, m, 1, *tail),
             lib.hf_ln_param_sums(v, gd.p(w[20000:]), gd.p(w[25000:]), src, m, m, 0, 1.0, *tail)]
    torch.cuda.synchronize()
    return codes


def test_refusals():
    lib = _lib.load()
    assert _codes(lib, 1, 16385) == [gd.ERR_ARG] * 4
    assert _codes(lib, 257, 4) == [gd.ERR_ARG] * 4
    assert _codes(lib, 2, 4, dtype=_lib.HF_F64) == [gd.ERR_ARG] * 4
    assert _codes(lib, 2, 4, null=True) == [gd.ERR_ARG] * 4
    assert _codes(lib, 2, 4, splits=33)[:3] == [gd.ERR_ARG] * 3  # (the column launch reads no slabs)
    assert _codes(lib, 2, 4, off=1) == [ERR_ALIGN] * 4           # the 16-byte form: row maps on the 16-byte grid
    assert _codes(lib, 2, 6, off=1) == [0] * 4                   # element loads: any 4-byte boundary
