"""GPU: every LAYER kernel of the curvature engine (``hf_bn.hip``, ``hf_head.hip``, the merged convolution launches)
through the C ABI against the high-precision references of ``layer_refs`` -- no engine, no ``modelprep``.

Inputs come from ``layer_refs`` (seeded on the CPU: ``test_layer_refs_cpu.py`` shows on the same numbers that an fp32
evaluation of the header's formula is inside the bound and that wrong variants are outside).  Bound of every
comparison: ``R * u * M`` (``layer_refs``: R roundings on the longest path, M the magnitude sum); ``tol.within`` sees
``value / bound`` against 1.  Masked-out elements, guard words, untouched halves of wider buffers, repeated launches
and ATen index / value comparisons are exact."""

import ctypes

import pytest
import torch
from tol import within

from conv_refs import GEOMS
from guarded import DEV, ERR_ARG, GUARD, NAN, P, RowOut, _ids, dv, optr, p, st, twice, wide
import layer_refs as L
from layer_refs import U32, U64
from pytorchhessianfree_amd import _lib
from pytorchhessianfree_amd.engine.common import _Launcher
from pytorchhessianfree_amd.engine.problems import Geometry, conv_problem

pytestmark = pytest.mark.gpu


def _ld(v, c):
    return v.ld[0] * c + v.ld[1] if v.ld[0] else 0


CASES = L.eval_cases()


# ---------------------------------------------------------------------------------------------------------------
# eval-mode BatchNorm, NHWC slab forms
# ---------------------------------------------------------------------------------------------------------------
def _affine_case(shape, slabs, i):
    (rows, c), (s1, s2) = shape, slabs
    o = L.eval_inputs(rows, c, s1, s2)
    v = L.AFFINE_VARIANTS[i % len(L.AFFINE_VARIANTS)]
    drop = tuple(d for d in v.drop if not (d == "a" and s1 > 1))
    ops = L.pick(o, ("a", "x", "mean", "rstd", "w", "q", "r", "add", "mask"), drop)
    a, x, mean, rstd, w, q, r, add, mask = ops
    want, M = L.chan_affine(*ops, v.relu_self)
    R = L.r_chan_affine(s1, a is not None, q is not None, r is not None, add is not None)
    ld = _ld(v, c)
    add_ld = ld if add is not None else 0
    dev = [dv(a), dv(x), dv(mean), dv(rstd), dv(w), dv(q), dv(r), wide(add, add_ld), dv(mask)]
    return NS_(o=o, v=v, ops=ops, dev=dev, want=want, M=M, R=R, ld=ld, add_ld=add_ld, rows=rows, c=c, s1=s1,
               mask=None if v.relu_self else mask)


class NS_(dict):
    __getattr__ = dict.__getitem__


def _check_affine(k, out):
    within(L.ratio(out.val, k.want, k.M, k.R), 1.0, strict=False, note=(k.rows, k.c, k.s1, k.R))
    if k.mask is not None:
        assert bool((out.val[~(k.mask > 0).to(DEV)] == 0).all()), "a masked-out element is not exactly zero"


@pytest.mark.parametrize("shape,slabs,i", CASES, ids=_ids)
def test_chan_affine_ex_against_float64(shape, slabs, i):
    """``hf_chan_affine_ex`` (eval tangent / forward form, split-K slabs): R = slab additions + 2 | 3, + joins."""
    k = _affine_case(shape, slabs, i)
    lib = _lib.load()
    n, hw = (k.rows, 1) if i % 2 else (1, k.rows)

    def launch():
        out = RowOut(k.rows, k.c, k.ld)
        _lib.check(lib.hf_chan_affine_ex(out.ptr, *(p(t) for t in k.dev), k.v.relu_self, n, k.c, hw, 1, k.ld, k.add_ld,
                                         k.s1, k.rows * k.c, _lib.HF_F32, st()), "hf_chan_affine_ex")
        return (out,)

    (out,) = twice(launch)
    _check_affine(k, out)


PAIRS = [(((200, 96), (3, 1), 0), ((37, 12), (9, 2), 5)), (((5, 4), (1, None), 1), ((130, 260), (17, 17), 7)),
         (((1568, 64), (8, 1), 2), ((3, 20), (2, 17), 6)), (((64, 1024), (1, 9), 3), ((32, 512), (9, 2), 0))]


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_chan_affine_pair_against_float64(pair):
    """``hf_chan_affine_pair``: two problems of different (rows, c, splits) in one launch, EACH against float64."""
    ks = [_affine_case(*c) for c in pair]
    lib = _lib.load()

    def launch():
        arr, outs = (_lib.AffineProblem * 2)(), []
        for q, k in zip(arr, ks):
            out = RowOut(k.rows, k.c, k.ld)
            outs.append(out)
            q.out = out.buf.data_ptr()
            for name, t in zip(("a", "x", "mean", "rstd", "w", "q", "r", "add", "mask_src"), k.dev):
                setattr(q, name, t.data_ptr() if t is not None else None)
            q.relu_self, q.n, q.c, q.hw, q.out_ld, q.add_ld = k.v.relu_self, k.rows, k.c, 1, k.ld, k.add_ld
            q.a_splits, q.a_slab = k.s1, k.rows * k.c
        _lib.check(lib.hf_chan_affine_pair(ctypes.cast(arr, P), _lib.HF_F32, st()), "hf_chan_affine_pair")
        return outs

    for k, out in zip(ks, twice(launch)):
        _check_affine(k, out)


def _bwd_case(shape, slabs, i, rb):
    (rows, c), (s1, s2) = shape, slabs
    o = L.eval_inputs(rows, c, s1, s2)
    bv = L.BWD_VARIANTS[i % len(L.BWD_VARIANTS)]
    x, mean, rstd, w, mask = L.pick(o, ("x", "mean", "rstd", "w", "mask"), bv.drop)
    ref = L.chan_affine_bwd(o.a, o.b, x, mean, rstd, w, mask)
    return NS_(o=o, drop=bv.drop, ref=ref, rows=rows, c=c, s1=s1, s2=s2, rb=rb, mask=mask,
               dev=[dv(o.a), dv(o.b), dv(x), dv(mean), dv(rstd), dv(w), dv(mask)])


def _bwd_outs(k):
    return [None if "gx" in k.drop else RowOut(k.rows, k.c), None if "gw" in k.drop else RowOut(k.rb, k.c, extra=2),
            None if "gb" in k.drop else RowOut(k.rb, k.c, extra=2), None if "gres" in k.drop else RowOut(k.rows, k.c)]


def _check_bwd(k, outs):
    gx, gw, gb, gres = outs
    ref, s1, s2 = k.ref, k.s1, k.s2
    note = (k.rows, k.c, s1, s2, k.rb)
    if gres is not None:
        within(L.ratio(gres.val, ref.g, ref.Mg, L.r_bwd_g(s1, s2)), 1.0, strict=False, note=note)
    if gx is not None:
        within(L.ratio(gx.val, ref.gx, ref.Mgx, L.r_bwd_gx(s1, s2)), 1.0, strict=False, note=note)
    if k.mask is not None:
        off = ~(k.mask > 0).to(DEV)
        for o in (gx, gres):
            assert o is None or bool((o.val[off] == 0).all()), "a masked-out element is not exactly zero"
    shares = L.row_shares(k.rows, k.rb)
    for out, f, Mf, R in ((gw, "gwe", "Mgwe", L.r_bwd_gw(s1, s2)), (gb, "g", "Mg", L.r_bwd_gb(s1, s2))):
        if out is None:
            continue
        e, Me = getattr(ref, f), getattr(ref, Mf)
        want = torch.stack([ref.col(e, lo, hi) for lo, hi in shares])
        M = torch.stack([ref.col(Me, lo, hi) for lo, hi in shares])
        # each single partial row against the float64 sum of ITS row share, then the total
        within(L.ratio(out.val, want, M, R), 1.0, strict=False, note=note)
        within(L.ratio(out.val.double().sum(0), want.sum(0), M.sum(0), R), 1.0, strict=False, note=note)


def _bwd_cases():
    out = []
    for sh, sl, i in CASES:
        ch = L.row_block_choices(*sh)
        out.append((sh, sl, i, ch[i % len(ch)]))
    for j, sh in enumerate(L.EVAL_SHAPES):
        for m, rb in enumerate(L.row_block_choices(*sh)):
            out.append((sh, L.SLAB_COUNTS_ONE_PASS[(3 * j + m) % len(L.SLAB_COUNTS_ONE_PASS)], j + m, rb))
    # more than one 16-deep pass without row shares: the channel-per-wave kernel with one element per lane (rows <= 64)
    # and with several (200 rows) for odd i (hw = 1), the column-per-block kernel for even i
    for sh in ((32, 512), (37, 12), (200, 96)):
        for sl in L.SLAB_COUNTS_MORE_PASSES:
            out += [(sh, sl, 5, 1), (sh, sl, 0, 1)]
    return out


@pytest.mark.parametrize("shape,slabs,i,rb", _bwd_cases(), ids=_ids)
def test_chan_affine_bwd_ex_against_float64(shape, slabs, i, rb):
    """``hf_chan_affine_bwd_ex``, full form: gx, gres elementwise (R = slab additions + 1 [+ 2]); gw / gb per partial
    row AND in total (fp64 accumulation, R = fp32 roundings inside one term + the store).  Row shares that would leave
    a workgroup without rows are refused."""
    k = _bwd_case(shape, slabs, i, rb)
    lib = _lib.load()
    n, hw = (k.rows, 1) if i % 2 else (1, k.rows)

    def call(outs):
        a, b, x, mean, rstd, w, mask = k.dev
        return lib.hf_chan_affine_bwd_ex(*(optr(o) for o in outs), p(a), k.s1, k.rows * k.c, p(b), k.s2 or 1,
                                         k.rows * k.c, p(x), p(mean), p(rstd), p(w), p(mask), n, k.c, hw, 1, rb,
                                         _lib.HF_F32, st())

    if rb > 1 and not L.share_ok(k.rows, rb):
        assert call(_bwd_outs(k)) == ERR_ARG  # (refused by the host-side check: nothing is launched)
        return

    def launch():
        outs = _bwd_outs(k)
        _lib.check(call(outs), "hf_chan_affine_bwd_ex")
        return outs

    _check_bwd(k, twice(launch))


BWD_PAIRS = [(((200, 96), (3, 1), 0, 7), ((37, 12), (9, 2), 4, 37)), (((130, 260), (2, 17), 1, 44), ((5, 4), (8, 1), 0, 2)),
             (((1568, 64), (17, 17), 5, 63), ((64, 1024), (1, 9), 2, 3)), (((3, 20), (1, None), 6, 3), ((32, 512), (1, 1), 0, 2))]


@pytest.mark.parametrize("pair", BWD_PAIRS, ids=_ids)
def test_chan_affine_bwd_pair_against_float64(pair):
    """``hf_chan_affine_bwd_pair``: two problems of different (rows, c, splits, row_blocks), each against float64."""
    ks = [_bwd_case(*c) for c in pair]
    lib = _lib.load()

    def fill(arr, ks_, outs_all):
        for q, k, outs in zip(arr, ks_, outs_all):
            a, b, x, mean, rstd, w, mask = k.dev
            q.gx, q.gw, q.gb, q.gres = (o.buf.data_ptr() if o is not None else None for o in outs)
            q.gy, q.gy_splits, q.gy_slab = a.data_ptr(), k.s1, k.rows * k.c
            q.gy2, q.gy2_splits, q.gy2_slab = (b.data_ptr() if b is not None else None), k.s2 or 1, k.rows * k.c
            for name, t in zip(("x", "mean", "rstd", "w", "mask_src"), (x, mean, rstd, w, mask)):
                setattr(q, name, t.data_ptr() if t is not None else None)
            q.n, q.c, q.hw, q.row_blocks = k.rows, k.c, 1, k.rb

    def launch():
        arr, outs_all = (_lib.BnAdjointProblem * 2)(), [_bwd_outs(k) for k in ks]
        fill(arr, ks, outs_all)
        _lib.check(lib.hf_chan_affine_bwd_pair(ctypes.cast(arr, P), _lib.HF_F32, st()), "hf_chan_affine_bwd_pair")
        return [o for outs in outs_all for o in outs]

    outs = twice(launch)
    for j, k in enumerate(ks):
        _check_bwd(k, outs[4 * j:4 * j + 4])
    # an empty row share in either problem: refused like the single launch
    bad = _bwd_case((37, 12), (1, None), 0, 63)
    arr, outs_all = (_lib.BnAdjointProblem * 2)(), [_bwd_outs(ks[0]), _bwd_outs(bad)]
    fill(arr, [ks[0], bad], outs_all)
    assert lib.hf_chan_affine_bwd_pair(ctypes.cast(arr, P), _lib.HF_F32, st()) == ERR_ARG


@pytest.mark.parametrize("c", [1028, 6])
def test_row_shares_refuse_channel_counts_outside_the_row_kernel(c):
    """row_blocks > 1 needs c % 4 == 0 and c <= 1024: HF_ERR_ARG before any launch."""
    lib = _lib.load()
    rows = 8
    g = torch.zeros(rows * c + 64, device=DEV)
    v = torch.zeros(2 * c, device=DEV)
    rc = lib.hf_chan_affine_bwd_ex(p(g), p(v), p(v), None, p(g), 1, 0, None, 1, 0, p(g), p(v), p(v), p(v), None, rows, c,
                                   1, 1, 2, _lib.HF_F32, st())
    assert rc == ERR_ARG


@pytest.mark.parametrize("shape,slabs,i", CASES, ids=_ids)
def test_bn_adjoint_pre_against_float64(shape, slabs, i):
    """``hf_bn_adjoint_pre``: g (R = slab additions + 1) and ga = g*(w*rstd) (R + 2)."""
    (rows, c), (s1, s2) = shape, slabs
    o = L.eval_inputs(rows, c, s1, s2)
    mask, w = (None if i % 4 == 1 else o.mask), (None if i % 4 == 2 else o.w)
    ref = L.bn_adjoint_pre(o.a, o.b, mask, w, o.rstd)
    a, b, m_, w_, rstd = dv(o.a), dv(o.b), dv(mask), dv(w), dv(o.rstd)
    lib = _lib.load()
    mode = i % 3  # both outputs / g_out only / ga_out only

    def launch():
        g, ga = (RowOut(rows, c) if mode != 2 else None), (RowOut(rows, c) if mode != 1 else None)
        _lib.check(lib.hf_bn_adjoint_pre(optr(g), optr(ga), p(a), s1, rows * c, p(b), s2 or 1, rows * c, p(m_), p(w_),
                                         p(rstd), rows, c, _lib.HF_F32, st()), "hf_bn_adjoint_pre")
        return g, ga

    g, ga = twice(launch)
    if g is not None:
        within(L.ratio(g.val, ref.g, ref.Mg, L.r_bwd_g(s1, s2)), 1.0, strict=False, note=(rows, c, s1, s2))
    if ga is not None:
        within(L.ratio(ga.val, ref.ga, ref.Mga, L.r_bwd_gx(s1, s2)), 1.0, strict=False, note=(rows, c, s1, s2))
    if mask is not None:
        for out in (g, ga):
            assert out is None or bool((out.val[~(mask > 0).to(DEV)] == 0).all())


@pytest.mark.parametrize("shape,slabs,i", CASES, ids=_ids)
def test_bn_forward_against_float64(shape, slabs, i):
    """``hf_bn_forward``: a_out = slab sum (R = slab additions), y = act(((s-mean)*rstd)*w + b + res) (R + 3 + 2)."""
    (rows, c), (s1, _) = shape, slabs
    o = L.eval_inputs(rows, c, s1, None, tag="fwd")
    bn, has_b, has_res, relu = i % 5 != 1, i % 3 != 1, i % 4 != 2, i % 2
    res_ld = (0, 2 * c, 2 * c + 4)[i % 3] if has_res else 0
    y2_ld = (2 * c, 2 * c + 4)[i % 2]
    mode = i % 3  # y and y2 / y only / y2 only
    mean, rstd, w = (o.mean, o.rstd, o.w) if bn else (None, None, None)
    b, res = (o.r if has_b else None), (o.add if has_res else None)
    ref = L.bn_forward(o.a, mean, rstd, w, b, res, relu)
    R = L.r_bn_forward(s1, bn, has_b, has_res)
    dev = [dv(o.a), dv(mean), dv(rstd), dv(w), dv(b), wide(res, res_ld)]
    lib = _lib.load()

    def launch():
        y, y2 = (RowOut(rows, c) if mode != 2 else None), (RowOut(rows, c, y2_ld) if mode != 1 else None)
        a_out = RowOut(rows, c) if i % 2 else None
        a, mu, rs, w_, b_, r_ = dev
        _lib.check(lib.hf_bn_forward(optr(y), optr(y2), y2_ld if y2 is not None else 0, optr(a_out), p(a), s1, rows * c,
                                     p(mu), p(rs), p(w_), p(b_), p(r_), res_ld, relu, rows, c, _lib.HF_F32, st()),
                   "hf_bn_forward")
        return y, y2, a_out

    y, y2, a_out = twice(launch)
    for out in (y, y2):
        if out is not None:
            within(L.ratio(out.val, ref.y, ref.My, R), 1.0, strict=False, note=(rows, c, s1, R))
    if y is not None and y2 is not None:
        assert torch.equal(y.val, y2.val)
    if a_out is not None:
        within(L.ratio(a_out.val, ref.s, ref.Ms, max(s1 - 1, 1)), 1.0, strict=False)


# ---------------------------------------------------------------------------------------------------------------
# hf_chan_affine / hf_chan_affine_bwd: layout x dtype (the autograd path)
# ---------------------------------------------------------------------------------------------------------------
def _to_layout(t, cl):
    """[n, h, w, c] (channel last, as the references take it) -> the memory order of the layout, flattened."""
    return (t if cl else t.permute(0, 3, 1, 2)).contiguous().reshape(-1)


def _from_layout(flat, n, c, h, w, cl):
    return flat.view(n, h, w, c) if cl else flat.view(n, c, h, w).permute(0, 2, 3, 1)


def _offset(t, off):
    """the same values ``off`` elements into a fresh allocation (4 bytes: no 16-byte alignment)"""
    if t is None or not off:
        return dv(t)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:]


LAYOUT_CASES = [(s, cl, dt_, 0) for s in L.LAYOUT_SHAPES for cl in (0, 1) for dt_ in (torch.float32, torch.float64)] + \
               [((3, 8, 5, 4), 1, torch.float32, 1), ((2, 32, 17, 17), 1, torch.float32, 1)]


@pytest.mark.parametrize("shape,cl,dtype,off", LAYOUT_CASES, ids=_ids)
def test_chan_affine_layouts_against_float64(shape, cl, dtype, off):
    """``hf_chan_affine`` and ``hf_chan_affine_bwd``: NCHW / NHWC, fp32 (float64 reference) / fp64 (longdouble
    reference), out_ld / add_ld in both layouts, and fp32 NHWC operands 4 bytes off the 16-byte grid (the scalar
    kernels where the vector ones would run).  R as for the slab forms with one slab."""
    f64 = dtype == torch.float64
    if f64 and not L.LD_OK:
        pytest.skip("numpy.longdouble is no wider than float64 on this machine")
    n, c, h, w = shape
    u = U64 if f64 else U32
    gen = L.gen_of("layout", *shape, cl, str(dtype), off)
    r4 = lambda: L.randn(gen, n, h, w, c, dtype=dtype)  # noqa: E731
    a, x, add, gy, gy2 = r4(), r4() * 2 + 0.5, r4(), r4(), r4()
    mask = L.mask_like(gen, n, h, w, c, dtype=dtype)
    mean, wt, q, r = (L.randn(gen, c, dtype=dtype) for _ in range(4))
    rstd = L.rstd_like(gen, c, dtype)
    lib, code = _lib.load(), _lib.dtype_code(dtype)
    hw, total = h * w, n * c * h * w
    use_ld = (sum(shape) + cl) % 2 == 1 and not off
    # the wider buffer: NHWC rows of 2c + 4 channels; NCHW samples of 2c + 1 channel planes
    ldc = (2 * c + 4) if cl else (2 * c + 1)
    ld = (ldc if cl else ldc * hw) if use_ld else 0

    def widen(t):  # [n, h, w, c] -> flat memory of the [n, h, w, ldc] / [n, ldc, h, w] buffer, other channels NaN
        if not use_ld:
            return _to_layout(t, cl)
        buf = torch.full((n, h, w, ldc), NAN, dtype=dtype)
        buf[..., :c] = t
        return _to_layout(buf, cl)

    def narrow(flat):
        full = _from_layout(flat, n, ldc if use_ld else c, h, w, cl)
        return full[..., :c], full[..., c:]

    want, M = L.chan_affine(a[None], x, mean, rstd, wt, q, r, add, mask, ld=f64)
    dev = [_offset(_to_layout(t, cl), off) for t in (a, x)] + [_offset(t, off) for t in (mean, rstd, wt, q, r)] + \
          [_offset(widen(add), off), _offset(_to_layout(mask, cl), off)]
    numel_out = n * (ldc if use_ld else c) * hw

    def launch_fwd():
        buf = torch.full((numel_out + GUARD + off,), NAN, dtype=dtype, device=DEV)
        _lib.check(lib.hf_chan_affine(P(buf[off:].data_ptr()), *(p(t) for t in dev), 0, n, c, hw, cl, ld, ld, code,
                                      st()), "hf_chan_affine")
        return buf

    b1, b2 = launch_fwd(), launch_fwd()
    iv = torch.int64 if f64 else torch.int32
    assert torch.equal(b1.view(iv), b2.view(iv))
    assert bool(torch.isnan(b1[off + numel_out:]).all()) and bool(torch.isnan(b1[:off]).all())
    got, rest = narrow(b1[off:off + numel_out].cpu())
    assert bool(torch.isnan(rest).all())
    within(L.ratio(got, want, M, L.r_chan_affine(1, True, True, True, True), u), 1.0, strict=False, note=shape)
    assert bool((got[~(mask > 0)] == 0).all())

    ref = L.chan_affine_bwd(gy[None], gy2[None], x, mean, rstd, wt, mask, ld=f64)
    dev = [_offset(_to_layout(t, cl), off) for t in (gy, gy2, x)] + [_offset(t, off) for t in (mean, rstd, wt)] + \
          [_offset(_to_layout(mask, cl), off)]

    def launch_bwd():
        gx, gres = (torch.full((total + GUARD + off,), NAN, dtype=dtype, device=DEV) for _ in range(2))
        gw, gb = (torch.full((c + GUARD,), NAN, dtype=dtype, device=DEV) for _ in range(2))
        _lib.check(lib.hf_chan_affine_bwd(P(gx[off:].data_ptr()), p(gw), p(gb), P(gres[off:].data_ptr()),
                                          *(p(t) for t in dev), n, c, hw, cl, code, st()), "hf_chan_affine_bwd")
        return gx, gw, gb, gres

    o1, o2 = launch_bwd(), launch_bwd()
    for t1, t2 in zip(o1, o2):
        assert torch.equal(t1.view(iv), t2.view(iv))
    gx, gw, gb, gres = o1
    for t, m_ in ((gx, total + off), (gres, total + off), (gw, c), (gb, c)):
        assert bool(torch.isnan(t[m_:]).all())
    gxv = _from_layout(gx[off:off + total].cpu(), n, c, h, w, cl).reshape(-1, c)
    grv = _from_layout(gres[off:off + total].cpu(), n, c, h, w, cl).reshape(-1, c)
    within(L.ratio(gxv, ref.gx, ref.Mgx, L.r_bwd_gx(1, 1), u), 1.0, strict=False, note=shape)
    within(L.ratio(grv, ref.g, ref.Mg, L.r_bwd_g(1, 1), u), 1.0, strict=False, note=shape)
    off_mask = ~(mask > 0).reshape(-1, c)
    assert bool((gxv[off_mask] == 0).all()) and bool((grv[off_mask] == 0).all())
    # column sums: fp32 -> fp64 accumulation + one store; fp64 -> every product and addition rounds (n*hw terms)
    rows = n * hw
    within(L.ratio(gw[:c].cpu(), ref.col(ref.gwe), ref.col(ref.Mgwe), (L.r_bwd_gw(1, 1) + (rows if f64 else 0)), u),
           1.0, strict=False, note=shape)
    within(L.ratio(gb[:c].cpu(), ref.col(ref.g), ref.col(ref.Mg), (L.r_bwd_gb(1, 1) + (rows if f64 else 0)), u), 1.0,
           strict=False, note=shape)


@pytest.mark.parametrize("i", range(4))
def test_bn_adjoint_pre_fp64_against_longdouble_float64(i):
    if not L.LD_OK:
        pytest.skip("numpy.longdouble is no wider than float64 on this machine")
    (rows, c), (s1, s2) = [(37, 12), (5, 4), (3, 20), (32, 64)][i], [(9, 2), (1, None), (2, 17), (3, 1)][i]
    o = L.eval_inputs(rows, c, s1, s2, dtype=torch.float64)
    ref = L.bn_adjoint_pre(o.a, o.b, o.mask, o.w, o.rstd, ld=True)
    a, b, m_, w_, rstd = dv(o.a), dv(o.b), dv(o.mask), dv(o.w), dv(o.rstd)

    def launch():
        g, ga = RowOut(rows, c, dtype=torch.float64), RowOut(rows, c, dtype=torch.float64)
        _lib.check(_lib.load().hf_bn_adjoint_pre(g.ptr, ga.ptr, p(a), s1, rows * c, p(b), s2 or 1, rows * c, p(m_),
                                                 p(w_), p(rstd), rows, c, _lib.HF_F64, st()), "hf_bn_adjoint_pre")
        return g, ga

    g, ga = twice(launch)
    within(L.ratio(g.val.cpu(), ref.g, ref.Mg, L.r_bwd_g(s1, s2), U64), 1.0, strict=False)
    within(L.ratio(ga.val.cpu(), ref.ga, ref.Mga, L.r_bwd_gx(s1, s2), U64), 1.0, strict=False)


# ---------------------------------------------------------------------------------------------------------------
# train-mode BatchNorm
# ---------------------------------------------------------------------------------------------------------------
def _train_case(rows, c, splits, nparts, i):
    o = L.train_inputs(rows, c, splits, nparts)
    vq, vr = (None, None) if i % 4 == 1 else (o.q, o.r)       # (the adjoint's use)
    add = None if i % 3 == 1 else o.add
    mask = None if i % 5 == 2 else o.mask
    want, M = L.chan_affine_train(o.a, o.x, o.mean, o.rstd, o.w, o.px, o.p1, vq, vr, float(rows), add, mask)
    ld = (0, 2 * c, 2 * c + 4)[i % 3]
    return NS_(rows=rows, c=c, splits=splits, nparts=nparts, want=want, M=M, mask=mask, ld=ld, has_add=add is not None,
               dev=[dv(o.a), dv(o.x), dv(o.mean), dv(o.rstd), dv(o.w), dv(o.px), dv(o.p1)], vq=dv(vq), vr=dv(vr),
               add=wide(add, ld), dmask=dv(mask))


def _check_train(k, out):
    R = L.r_chan_affine_train(k.splits, k.has_add)
    within(L.ratio(out.val, k.want, k.M, R), 1.0, strict=False, note=(k.rows, k.c, k.splits, k.nparts, R))
    if k.mask is not None:
        assert bool((out.val[~(k.mask > 0).to(DEV)] == 0).all())


@pytest.mark.parametrize("i,case", list(enumerate(L.TRAIN_CASES)), ids=_ids)
def test_chan_affine_train_against_float64(i, case):
    """``hf_chan_affine_train``: partial rows added up in the prologue, q / r formed (6 roundings), then the affine
    map; vq / vr / add / mask_src NULL in turn."""
    k = _train_case(*case, i)
    lib = _lib.load()

    def launch():
        out = RowOut(k.rows, k.c, k.ld)
        a, x, mean, rstd, w, px, p1 = k.dev
        _lib.check(lib.hf_chan_affine_train(out.ptr, p(a), p(x), p(mean), p(rstd), p(w), p(px), p(p1), k.nparts, p(k.vq),
                                            p(k.vr), float(k.rows), p(k.add), p(k.dmask), k.rows, k.c, 1, k.ld,
                                            k.ld if k.has_add else 0, k.splits, k.rows * k.c, _lib.HF_F32, st()),
                   "hf_chan_affine_train")
        return (out,)

    (out,) = twice(launch)
    _check_train(k, out)


@pytest.mark.parametrize("ia,ib", [(0, 9), (5, 15), (10, 3), (13, 6)])
def test_chan_affine_train_pair_against_float64(ia, ib):
    """``hf_chan_affine_train_pair``: two different problems (no residual operand), each against float64."""
    # (variants without a residual operand: 4 / 7 = with vq, vr and with / without mask; 1 = the adjoint's use)
    ks = [_train_case(*L.TRAIN_CASES[ia], 7 if ia % 2 else 4), _train_case(*L.TRAIN_CASES[ib], 1)]
    assert not any(k.has_add for k in ks)
    lib = _lib.load()

    def launch():
        arr, outs = (_lib.AffineTrainProblem * 2)(), []
        for q, k in zip(arr, ks):
            out = RowOut(k.rows, k.c, k.ld)
            outs.append(out)
            q.out = out.buf.data_ptr()
            for name, t in zip(("a", "x", "mean", "rstd", "w", "part_x", "part_1"), k.dev):
                setattr(q, name, t.data_ptr())
            q.nparts, q.count = k.nparts, float(k.rows)
            q.vq, q.vr = (k.vq.data_ptr(), k.vr.data_ptr()) if k.vq is not None else (None, None)
            q.add, q.mask_src = None, (k.dmask.data_ptr() if k.dmask is not None else None)
            q.n, q.c, q.hw, q.out_ld, q.a_splits, q.a_slab = k.rows, k.c, 1, k.ld, k.splits, k.rows * k.c
        _lib.check(lib.hf_chan_affine_train_pair(ctypes.cast(arr, P), _lib.HF_F32, st()), "hf_chan_affine_train_pair")
        return outs

    for k, out in zip(ks, twice(launch)):
        _check_train(k, out)


HESS = [((37, 8), (1, 1), 1), ((37, 8), (33, 5), 3), ((37, 8), (257, 64), 9), ((128, 256), (1, 1), 3),
        ((128, 256), (33, 5), 9), ((128, 256), (257, 64), 1), ((1568, 64), (1, 1), 9), ((1568, 64), (33, 5), 1),
        ((1568, 64), (257, 64), 3), ((32, 12), (1, 1), 3), ((32, 12), (33, 5), 1), ((32, 12), (257, 64), 9)]


@pytest.mark.parametrize("shape,parts,sp", HESS, ids=_ids)
def test_train_hessian_kernels_against_float64(shape, parts, sp):
    """``hf_bn_train_hessian_coeffs``: the six coefficient vectors and gw_corr against the float64 closed form on the
    partial rows as given (computed in fp64 by the kernel, one rounding at the store: R = 1).
    ``hf_bn_train_hessian_apply``: against the float64 formula with the kernel's own coefficients (R = slab additions
    + 3, at least 5), and against float64 DOUBLE BACKWARD of relu(gamma*xhat + beta): six more roundings -- up to
    three fp32-rounded factors inside a coefficient (first-order gradient, partial rows, rstd), the coefficient's
    store, and the fp32 mean and rstd (or the fp32 cotangent) it multiplies."""
    (rows, c), (nparts, nparts_t) = shape, parts
    pr = L.train_hessian_problem(rows, c, sp)
    rows_in = [L.partial_rows(e, nparts) for e in (pr.dg_z * pr.xh, pr.dg_z, pr.r * pr.g_z * pr.da)] + \
              [L.partial_rows(e, nparts_t) for e in (pr.da * pr.xh, pr.da)]
    gg1, gb1 = pr.gg.float(), pr.gb.float()
    cf = L.train_hessian_coeffs(*rows_in, gg1, gb1, pr.gam, pr.dgam, pr.rstd, float(rows))
    lib = _lib.load()
    dev = [dv(t) for t in rows_in]
    vecs = [dv(t) for t in (gg1, gb1, pr.gam, pr.dgam, pr.rstd)]

    def launch_c():
        coef, corr = RowOut(6, c), RowOut(1, c)
        _lib.check(lib.hf_bn_train_hessian_coeffs(coef.ptr, corr.ptr, p(dev[0]), p(dev[1]), p(dev[2]), nparts, p(dev[3]),
                                                  p(dev[4]), nparts_t, *(p(t) for t in vecs), float(rows), c,
                                                  _lib.HF_F32, st()), "hf_bn_train_hessian_coeffs")
        return coef, corr

    coef, corr = twice(launch_c)
    within(L.ratio(coef.val, cf.coef, cf.Mcoef, 1), 1.0, strict=False, note=(shape, parts))
    within(L.ratio(corr.val[0], cf.corr, cf.Mcorr, 1), 1.0, strict=False, note=(shape, parts))

    ga1, gz1, gz2 = pr.ga.float(), pr.g_z.float(), pr.dg_z.float()
    ops = [dv(t) for t in (ga1, gz1, gz2, pr.t, pr.a, pr.mean, pr.rstd)]
    kcoef = coef.val.contiguous()

    def launch_a():
        out = RowOut(rows, c)
        _lib.check(lib.hf_bn_train_hessian_apply(out.ptr, p(ops[0]), p(ops[1]), p(ops[2]), p(ops[3]), sp, rows * c,
                                                 p(ops[4]), p(ops[5]), p(ops[6]), p(kcoef), rows, c, _lib.HF_F32,
                                                 st()), "hf_bn_train_hessian_apply")
        return (out,)

    (out,) = twice(launch_a)
    R = L.r_train_hessian_apply(sp)
    want, M = L.train_hessian_apply(ga1, gz1, gz2, pr.t, pr.a, pr.mean, pr.rstd, kcoef.cpu())
    within(L.ratio(out.val, want, M, R), 1.0, strict=False, note=(shape, parts, sp))
    _, Mdb = L.train_hessian_apply(ga1, gz1, gz2, pr.t, pr.a, pr.mean, pr.rstd, cf.coef, cf.Mcoef)
    within(L.ratio(out.val, pr.want_a, Mdb, R + 6), 1.0, strict=False, note=(shape, parts, sp))


# ---------------------------------------------------------------------------------------------------------------
# heads and pooling
# ---------------------------------------------------------------------------------------------------------------
def _same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0),
                                                                        torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("i,geom", list(enumerate(L.POOL_GEOMS)), ids=_ids)
def test_maxpool_forward_equals_aten_reference(i, geom):
    """``hf_maxpool_forward_nhwc``: values AND positions equal to ATen's ``max_pool2d_with_indices`` exactly (ties,
    -inf, NaN, windows partly in the padding); then the tangent and adjoint kernels on that index map (exact: a
    gather / a sum of one or two terms in the reference's order)."""
    n, c, h, w, kh, kw, sh, sw, ph, pw = geom
    x = L.maxpool_input(geom)
    want, widx = torch.nn.functional.max_pool2d(x, (kh, kw), (sh, sw), (ph, pw), return_indices=True)
    rv, ri = L.maxpool_forward(x, kh, kw, sh, sw, ph, pw)
    assert torch.equal(ri, widx) and _same_with_nan(rv, want)
    oh, ow = want.shape[2], want.shape[3]
    xd = dv(x.permute(0, 2, 3, 1))
    lib = _lib.load()
    mode = i % 3  # out and out2 / out only / out2 (pixel stride 2c) only
    orow = n * oh * ow

    def launch():
        out, out2 = (RowOut(orow, c) if mode != 2 else None), (RowOut(orow, c, 2 * c) if mode != 1 else None)
        idx = torch.full((orow * c + GUARD,), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.hf_maxpool_forward_nhwc(optr(out), optr(out2), 2 * c if out2 is not None else 0, p(idx), p(xd), n,
                                               h, w, oh, ow, c, kh, kw, sh, sw, ph, pw, _lib.HF_F32, st()),
                   "hf_maxpool_forward_nhwc")
        return out, out2, idx

    o1, o2 = launch(), launch()
    torch.cuda.synchronize()
    idx = o1[2]
    assert torch.equal(idx, o2[2]) and bool((idx[orow * c:] == -7).all())
    want_rows = want.permute(0, 2, 3, 1).reshape(orow, c)
    for a, b in zip(o1[:2], o2[:2]):
        if a is not None:
            assert a.same(b) and a.untouched() and _same_with_nan(a.val.cpu(), want_rows)
    got_idx = idx[:orow * c].view(n, oh, ow, c).permute(0, 3, 1, 2).cpu().long()
    assert torch.equal(got_idx, widx)

    # the three kernels agree on the index convention
    gen = L.gen_of("pool-t", *geom)
    t = L.randn(gen, n, h, w, c)
    tout, td = RowOut(orow, c, 2 * c), dv(t)
    _lib.check(lib.hf_maxpool_tangent_nhwc(tout.ptr, p(td), p(idx), n, h, w, oh, ow, c, 2 * c, _lib.HF_F32, st()),
               "hf_maxpool_tangent_nhwc")
    want_t = t.permute(0, 3, 1, 2).flatten(2).gather(2, widx.flatten(2)).view(n, c, oh, ow).permute(0, 2, 3, 1)
    assert torch.equal(tout.val.cpu(), want_t.reshape(orow, c)) and tout.untouched()
    ga, gb_ = L.randn(gen, 2, orow, c), L.randn(gen, 1, orow, c)
    g, gad, gbd = RowOut(n * h * w, c), dv(ga), dv(gb_)
    _lib.check(lib.hf_maxpool_adjoint_nhwc(g.ptr, p(gad), 2, orow * c, p(gbd), 1, 0, p(idx), n, h, w, oh, ow, c,
                                           kh, kw, sh, sw, ph, pw, _lib.HF_F32, st()), "hf_maxpool_adjoint_nhwc")
    gy = (ga.double().sum(0) + gb_[0].double()).view(n, oh, ow, c).permute(0, 3, 1, 2)
    want_g = torch.zeros(n, c, h * w, dtype=torch.float64).scatter_add_(2, widx.flatten(2), gy.flatten(2))
    Mg = torch.zeros(n, c, h * w, dtype=torch.float64).scatter_add_(
        2, widx.flatten(2), (ga.double().abs().sum(0) + gb_[0].double().abs()).view(n, oh, ow, c).permute(0, 3, 1, 2)
        .flatten(2))
    to_rows = lambda v: v.view(n, c, h, w).permute(0, 2, 3, 1).reshape(-1, c)  # noqa: E731
    # per window: one slab addition + the addition of the two cotangents, then up to kh*kw windows accumulated
    within(L.ratio(g.val, to_rows(want_g), to_rows(Mg), 2 + kh * kw), 1.0, strict=False, note=geom)
    assert g.untouched()


@pytest.mark.parametrize("n,hw,k", L.HEAD_SHAPES)
@pytest.mark.parametrize("with_jv", [0, 1])
def test_pool_ce_head_against_float64(n, hw, k, with_jv):
    """``hf_pool_ce_head``: Jv (R = hw: hw - 1 additions and the division) and g (R = hw + 6)."""
    t, pm = L.head_inputs(n, hw, k)
    ref = L.pool_ce_head(t, pm, 1.0 / n)
    td, pd = dv(t), dv(pm)
    lib = _lib.load()

    def launch():
        g, jv = RowOut(n * hw, k), (RowOut(n, k) if with_jv else None)
        _lib.check(lib.hf_pool_ce_head(g.ptr, optr(jv), p(td), p(pd), 1.0 / n, n, hw, k, _lib.HF_F32, st()),
                   "hf_pool_ce_head")
        return g, jv

    g, jv = twice(launch)
    rj, rg = L.r_pool_ce_head(hw)
    within(L.ratio(g.val, ref.g.reshape(n * hw, k), ref.Mg.reshape(n * hw, k), rg), 1.0, strict=False, note=(n, hw, k))
    if jv is not None:
        within(L.ratio(jv.val, ref.jv, ref.Mjv, rj), 1.0, strict=False, note=(n, hw, k))


def test_pool_ce_head_refuses_what_it_does_not_cover():
    lib = _lib.load()
    z = torch.zeros(4096, device=DEV)
    assert lib.hf_pool_ce_head(p(z), None, p(z), p(z), 1.0, 1, 1, 1025, _lib.HF_F32, st()) == ERR_ARG   # k > 1024
    assert lib.hf_pool_ce_head(p(z), None, p(z), p(z), 1.0, 1 << 20, 1 << 10, 4, _lib.HF_F32, st()) == ERR_ARG  # 2^32
    assert lib.hf_pool_ce_head(p(z), None, p(z), p(z), 1.0, 2, 2, 4, _lib.HF_F64, st()) == ERR_ARG     # fp32 only
    assert lib.hf_pool_ce_head(p(z), None, p(z), None, 1.0, 2, 2, 4, _lib.HF_F32, st()) == ERR_ARG


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("cols", [1, 10, 257, 1000])
def test_softmax_ce_hvp_against_float64(dtype, rows, cols):
    """``hf_softmax_ce_hvp``: fp32 against float64 (R = 5), fp64 against longdouble (R = cols + 3)."""
    f64 = dtype == torch.float64
    if f64 and not L.LD_OK:
        pytest.skip("numpy.longdouble is no wider than float64 on this machine")
    pm, v = L.softmax_inputs(rows, cols, dtype)
    want, M = L.softmax_ce_hvp(pm, v, 1.0 / rows, ld=f64)
    pd, vd = dv(pm), dv(v)

    def launch():
        out = RowOut(rows, cols, dtype=dtype)
        _lib.check(_lib.load().hf_softmax_ce_hvp(out.ptr, p(pd), p(vd), 1.0 / rows, rows, cols, _lib.dtype_code(dtype),
                                                 st()), "hf_softmax_ce_hvp")
        return (out,)

    (out,) = twice(launch)
    within(L.ratio(out.val.cpu() if f64 else out.val, want, M, L.r_softmax_ce_hvp(cols, f64), U64 if f64 else U32), 1.0,
           strict=False, note=(rows, cols))


# ---------------------------------------------------------------------------------------------------------------
# merged convolution launches
# ---------------------------------------------------------------------------------------------------------------
def _conv_geoms():
    out = []
    for g in GEOMS:
        n, h, w, c, k, r, s, stride, padding = g
        oh, ow = (h + 2 * padding[0] - r) // stride[0] + 1, (w + 2 * padding[1] - s) // stride[1] + 1
        if c % 4 == 0 and k % 4 == 0 and n * oh * ow <= 8192:
            out.append(g)
    return out


def launcher(device):
    """What an engine is to its launches: a ``_Launcher`` with a device."""
    eng = _Launcher()
    eng.dev = torch.device(device)
    return eng


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("geom", _conv_geoms(), ids=lambda g: str(g[:7]).replace(" ", ""))
def test_merged_convolution_launches_against_float64(geom):
    """``hf_conv2d_nhwc_backward_slabs`` and ``hf_conv2d_nhwc_dw_slabs``: slabs bitwise those of the two
    ``hf_conv2d_nhwc_slabs`` launches, their sums within the convolution suite's 2e-5 of the float64 result's
    max-norm; ``dw_slabs`` also in the Hessian sweep's form (activation = first-c slice of [t_x | x], a data-gradient
    matrix that is not the layer's own)."""
    n, h, w_, c, k, r, s, stride, padding = geom
    gen = L.gen_of("conv", *geom[:7])
    x, t_x = (_cl(L.randn(gen, n, c, h, w_)) for _ in range(2))
    w, v = (_cl(L.randn(gen, k, c, r, s)) for _ in range(2))
    oh, ow = (h + 2 * padding[0] - r) // stride[0] + 1, (w_ + 2 * padding[1] - s) // stride[1] + 1
    gy = _cl(L.randn(gen, n, k, oh, ow))
    _, gx64, gw64 = L.conv_refs(x, w, gy, stride, padding)
    _, gxv64, _ = L.conv_refs(x, v, gy, stride, padding)
    _, _, gwt64 = L.conv_refs(t_x, w, gy, stride, padding)
    xd, gyd = _cl(x.to(DEV)), _cl(gy.to(DEV))
    wT, vT = (m.permute(1, 2, 3, 0).contiguous().to(DEV) for m in (w, v))
    wide_ = _cl(torch.cat([t_x, x], 1).to(DEV))  # NHWC rows of [t_x | x]
    geo = Geometry(n, h, w_, c, k, r, s, stride, padding)
    sd, sw = _lib.conv_plan(1, *geo), _lib.conv_plan(2, *geo)
    nd, nw = x.numel(), w.numel()
    dw_slabs = lambda d, w: launcher(xd.device)._launch("hf_conv2d_nhwc_dw_slabs", [d], [w])  # noqa: E731

    def rel(slabs, ref, shape):
        got = slabs.double().sum(0).view(shape).permute(0, 3, 1, 2).cpu()
        return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))

    def fresh():
        return torch.zeros(sd, nd, device=DEV), torch.zeros(sw, nw, device=DEV)

    dx1, dw1 = fresh()
    _lib.conv2d_nhwc_slabs(1, dx1, gyd, wT, *geo, sd)
    _lib.conv2d_nhwc_slabs(2, dw1, xd, gyd, *geo, sw)
    dx2, dw2 = fresh()
    _lib.check(_lib.load().hf_conv2d_nhwc_backward_slabs(
        p(dx2), p(dw2), p(gyd), p(xd), p(wT), n, h, w_, c, k, r, s, stride[0], stride[1], padding[0], padding[1], sd, nd,
        sw, nw, _lib.HF_F32, st()), "hf_conv2d_nhwc_backward_slabs")
    dx3, dw3 = fresh()
    dw_slabs(conv_problem(1, dx3, gyd, wT, geo, sd), conv_problem(2, dw3, xd, gyd, geo, sw))
    for a, b in ((dx2, dw2), (dx3, dw3)):
        assert torch.equal(a, dx1) and torch.equal(b, dw1)
        within(rel(a, gx64, (n, h, w_, c)), 2e-5, note=geom)
        within(rel(b, gw64, (k, r, s, c)), 2e-5, note=geom)
    # the Hessian sweep's pair: conv_D(g, V), conv_W(t_x, g) with t_x read in place from [t_x | x]
    dx4, dw4 = fresh()
    _lib.conv2d_nhwc_slabs(1, dx4, gyd, vT, *geo, sd)
    _lib.conv2d_nhwc_slabs(2, dw4, wide_, gyd, *geo, sw, act_ld=2 * c)
    dx5, dw5 = fresh()
    dw_slabs(conv_problem(1, dx5, gyd, vT, geo, sd), conv_problem(2, dw5, wide_, gyd, geo, sw, act_ld=2 * c))
    assert torch.equal(dx5, dx4) and torch.equal(dw5, dw4)
    within(rel(dx5, gxv64, (n, h, w_, c)), 2e-5, note=geom)
    within(rel(dw5, gwt64, (k, r, s, c)), 2e-5, note=geom)
