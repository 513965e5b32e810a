"""GPU: ``hf_pool_bn_act_tangent_nhwc`` / ``hf_pool_bn_act_adjoint_nhwc`` (eval-mode BatchNorm + ReLU + max-pool of a
plain stack's pooled unit, one launch per sweep direction) through the C ABI against the float64 references of
``pool_bn_act_refs`` -- no engine, no ``modelprep``.

Operands are dyadic (multiples of 1/8 of magnitude <= 4; ``w``, ``rstd`` in {0.5, 1, 2}): every product and sum is exact
in fp32 in any order (``test_pool_bn_act_refs_cpu.py`` asserts that the references are fp32 numbers), so the results must
equal the float64 reference BITWISE.  ``idx`` and ``y_pool`` come from the reference (ATen's forward on tie-free planes).
One case per kernel runs on standard-normal operands against bounds derived from the header's rounding sequence,
``roundings * 2^-24 * sum |terms|`` per element, and checks the header's bitwise identities against the existing kernels
(``hf_chan_affine_ex``, ``hf_pool_act_adjoint_nhwc``, ``hf_bn_adjoint_v4``) there."""

import itertools

import pytest
import torch
from tol import within

from guarded import DEV, ERR_ARG, NAN, U32, RowOut, p, slabs_dev, st, twice
import pool_bn_act_refs as B
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu

# every geometry x map x channel count (16 bytes per thread), and two element-wise channel counts
SHAPES = [(g, m, c) for g in B.GEOMS for m in B.MAPS for c in (4, 12)] + [((3, 2, 1), (5, 7), 3), ((2, 2, 0), (4, 4), 6)]
# tangent: splits, wide out, relu, v_w, v_b, slab stride pad.   adjoint: gy splits, relu, g, sums, row blocks, slab pad
T_OPTS = list(itertools.product((1, 2, 9), (0, 1), (0, 1), (0, 1), (0, 1), (4, 6)))
A_OPTS = list(itertools.product((1, 2, 9), (0, 1), (0, 1), ("", "b", "w", "wb"), (1, 3, 4), (4, 6)))
T_VALUES, A_VALUES = [3, 2, 2, 2, 2, 2], [3, 2, 2, 4, 3, 2]


def _t_opts(i):
    return T_OPTS[(37 * i + 5 * (i // 6)) % len(T_OPTS)]


def _a_opts(i):
    return A_OPTS[(85 * i + 7 * (i // 6)) % len(A_OPTS)]


# per-axis windows x both channel forms, and the row-sum kernel beyond 256 channel columns (``test_pool_act_kernels_gpu``)
AXIS_SHAPES = [(g, m, c) for g, m in B.AXIS_GEOMS for c in (4, 3)]
WIDE = [(258, 1, 2, 1, "wb"), (258, 3, 1, 0, "wb"), (1028, 1, 1, 1, "wb"), (1028, 3, 2, 0, "wb"),  # c, rb, gy splits, relu
        (258, 3, 2, 1, "w"), (1028, 3, 1, 1, "b")]


def _axis_t_opts(j):
    return T_OPTS[(5 * j + 14) % len(T_OPTS)]


def _axis_a_opts(j):
    return A_OPTS[(17 * j + 5) % len(A_OPTS)]


def _ids(shapes):
    return dict(argvalues=range(len(shapes)), ids=lambda i: "-".join(str(x) for x in shapes[i]).replace(" ", ""))


def _row_blocks(sums, rb):
    return rb if sums else 0  # (without sums: the one-pixel-per-thread form, row_blocks is not read)


def test_every_option_value_is_exercised():
    for opts, values in ((_t_opts, T_VALUES), (_a_opts, A_VALUES)):
        seen = [set() for _ in values]
        for i in range(len(SHAPES)):
            for s, v in zip(seen, opts(i)):
                s.add(v)
        assert [len(s) for s in seen] == values
    # ... and, per geometry class (kernel, stride, padding), both relu values, null and non-null v_w / g, and sums with
    # and without gw, on the 16-byte path
    for geom in B.GEOMS:
        mine = [i for i, (g, _m, c) in enumerate(SHAPES) if g == geom and c % 4 == 0]
        assert {_t_opts(i)[2] for i in mine} == {0, 1} and {_t_opts(i)[3] for i in mine} == {0, 1}, geom
        assert {_a_opts(i)[1] for i in mine} == {0, 1} and {_a_opts(i)[2] for i in mine} == {0, 1}, geom
        assert {"w" in _a_opts(i)[3] for i in mine} == {False, True}, geom
    # row blocks: 1, and several with a ragged last share (rows % row_blocks != 0) somewhere
    ragged = 0
    for i, (_g, (h, w), _c) in enumerate(SHAPES):
        _s, _r, _g_, sums, rb, _p = _a_opts(i)
        ragged += bool(sums) and rb > 1 and (2 * h * w) % rb != 0
    assert ragged >= 3


def test_every_option_value_meets_a_per_axis_window():
    for opts, values in ((_axis_t_opts, T_VALUES), (_axis_a_opts, A_VALUES)):
        seen = [{opts(j)[k] for j in range(len(AXIS_SHAPES))} for k in range(len(values))]
        assert [len(s) for s in seen] == values
    for c in (4, 3):  # ... and in each channel form
        mine = [j for j, (_g, _m, cj) in enumerate(AXIS_SHAPES) if cj == c]
        assert all({_axis_t_opts(j)[k] for j in mine} == {0, 1} for k in (1, 2, 3, 4)), c
        assert {_axis_a_opts(j)[1] for j in mine} == {0, 1} and {_axis_a_opts(j)[2] for j in mine} == {0, 1}, c
        rows = [_axis_a_opts(j) for j in mine if _axis_a_opts(j)[3]]  # (the row-sum kernel: only with sums)
        assert {"w" in o[3] for o in rows} == {False, True} and {o[4] for o in rows} >= {1, 3}, c
        assert {o[1] for o in rows} == {0, 1}, c  # (a pooled unit without the ReLU takes its sums there too)
    for g in range(len(B.AXIS_GEOMS)):  # every window runs through the row-sum kernel in one channel form at least
        assert _axis_a_opts(2 * g)[3] or _axis_a_opts(2 * g + 1)[3]
    assert {(x[0], x[1]) for x in WIDE} == {(258, 1), (258, 3), (1028, 1), (1028, 3)}
    assert {x[2] for x in WIDE} == {1, 2} and {x[3] for x in WIDE} == {0, 1} and {x[4] for x in WIDE} == {"wb", "w", "b"}


def _dev(o, *names):
    return [o[k].to(DEV) for k in names]


@pytest.mark.parametrize("i", **_ids(SHAPES))
def test_tangent_equals_float64_bitwise(i):
    _tangent(SHAPES[i], _t_opts(i))


@pytest.mark.parametrize("j", **_ids(AXIS_SHAPES))
def test_tangent_on_per_axis_windows_equals_float64_bitwise(j):
    _tangent(AXIS_SHAPES[j], _axis_t_opts(j))


def _tangent(shape, opts):
    ((k, s, pd), (h, w), c), n = shape, 2
    splits, wide, relu, with_vw, with_vb, pad = opts
    o = B.case(n, c, h, w, k, s, pd, splits, 1)
    y_pool, idx = B.forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    v_w, v_b = (o["v_w"] if with_vw else None), (o["v_b"] if with_vb else None)
    want, _ = B.tangent(o, v_w, v_b, idx, y_pool, relu)
    stride = n * h * w * c + pad
    sd = slabs_dev(o["slabs"], stride)
    ad, md, rd, wd = _dev(o, "a", "mean", "rstd", "w")
    vwd, vbd = (v_w.to(DEV) if with_vw else None), (v_b.to(DEV) if with_vb else None)
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, ld, orow = _lib.load(), (2 * c if wide else 0), n * oh * ow

    def launch():
        out = RowOut(orow, c, ld)
        _lib.check(lib.hf_pool_bn_act_tangent_nhwc(out.ptr, ld, p(sd), splits, stride, p(ad), p(md), p(rd), p(wd), p(vwd),
                                                   p(vbd), p(idxd), p(yd), relu, n, h, w, oh, ow, c, _lib.HF_F32, st()),
                   "hf_pool_bn_act_tangent_nhwc")
        return out

    assert torch.equal(twice(launch).val.cpu().double(), want.reshape(orow, c))


@pytest.mark.parametrize("i", **_ids(SHAPES))
def test_adjoint_equals_float64_bitwise(i):
    _adjoint(SHAPES[i], 2, *_a_opts(i))


@pytest.mark.parametrize("j", **_ids(AXIS_SHAPES))
def test_adjoint_on_per_axis_windows_equals_float64_bitwise(j):
    """kh, kw, stride_h, stride_w, pad_h, pad_w each reach their own axis: the reference with any unequal pair exchanged
    differs on these operands (asserted), and the kernel equals the right one."""
    _adjoint(AXIS_SHAPES[j], 2, *_axis_a_opts(j))


@pytest.mark.parametrize("c, rb, gy_splits, relu, sums", WIDE, ids=lambda v: str(v))
def test_adjoint_row_sums_beyond_256_channel_columns_equal_float64_bitwise(c, rb, gy_splits, relu, sums):
    """c = 258: the element-wise form, 258 columns -- a second pass with 2 live columns; c = 1028: the 16-byte form, 257
    quads -- a second pass with one.  Both sums per channel share the reduction buffer, reused between the passes."""
    _adjoint(((2, 2, 0), (4, 4), c), 1, gy_splits, relu, 1, sums, rb, 4)


def _adjoint(shape, n, gy_splits, relu, with_g, sums, rb, pad):
    (k, s, pd), (h, w), c = shape
    (kh, kw), (sh, sw), (ph, pw) = B.pair(k), B.pair(s), B.pair(pd)
    row_blocks = _row_blocks(sums, rb)
    o = B.case(n, c, h, w, k, s, pd, 1, gy_splits)
    y_pool, idx = B.forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    want = B.adjoint(o, idx, y_pool, relu, h, w, k, s, pd, row_blocks)
    for name, (k2, s2, p2) in B.R.exchanges((k, s, pd)):
        assert not torch.equal(B.R.adjoint(o["gy"], idx, y_pool, relu, h, w, k2, s2, p2)[0], want["g"]), name
    slab = n * oh * ow * c + pad
    gd = slabs_dev(o["gy"], slab)
    ad, md, rd, wd = _dev(o, "a", "mean", "rstd", "w")
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, rows = _lib.load(), n * h * w

    def launch():
        outs = dict(ga=RowOut(rows, c), g=RowOut(rows, c) if with_g else None, gw=RowOut(row_blocks, c) if "w" in sums else None,
                    gb=RowOut(row_blocks, c) if "b" in sums else None)
        ptr = {name: (t.ptr if t is not None else None) for name, t in outs.items()}
        _lib.check(lib.hf_pool_bn_act_adjoint_nhwc(ptr["ga"], ptr["g"], ptr["gw"], ptr["gb"], row_blocks, p(gd), gy_splits,
                                                   slab, p(ad), p(md), p(rd), p(wd), p(idxd), p(yd), relu, n, h, w, oh, ow,
                                                   c, kh, kw, sh, sw, ph, pw, _lib.HF_F32, st()),
                   "hf_pool_bn_act_adjoint_nhwc")
        return outs

    a, b = launch(), launch()
    torch.cuda.synchronize()
    for name, x in a.items():
        if x is not None:
            assert x.same(b[name]), f"{name}: two launches on the same operands differ"
            assert x.untouched(), name
            assert torch.equal(x.val.cpu().double(), want[name].reshape(-1, c)), name


def test_random_operands_within_the_derived_bounds_and_the_identities():
    """Standard-normal operands.  Bounds per element, ``roundings * 2^-24 * sum |terms|``: the tangent adds ``splits`` slabs
    (splits - 1 roundings), forms w*rstd and multiplies (2), forms xhat*v_w (3) and adds it and the shift (2): splits + 6;
    g adds ``gy_splits`` slabs for each of up to ``windows`` windows (+ 2 of slack, as the bias form's test); ga two more
    (w*rstd, the product); a partial row of gb rounds its fp64 sum once (inside the slack), one of gw also carries xhat's
    two roundings per term.  Identities (bitwise): the tangent is ``hf_chan_affine_ex``'s unmasked dense output gathered at
    idx and masked; g is ``hf_pool_act_adjoint_nhwc``'s ga; ga is ``hf_bn_adjoint_v4``'s scaling of it."""
    n, c, h, w, k, s, pd, splits, gy_splits, rb = 2, 12, 5, 7, 3, 2, 1, 9, 9, 3
    o = B.case(n, c, h, w, k, s, pd, splits, gy_splits, exact=False)
    y_pool, idx = B.forward(o, k, s, pd, 1)
    oh, ow = o["oh"], o["ow"]
    lib, F32 = _lib.load(), _lib.HF_F32
    idxd, yd = idx.to(torch.int32).to(DEV), y_pool.to(DEV)
    ad, md, rd, wd, vwd, vbd = _dev(o, "a", "mean", "rstd", "w", "v_w", "v_b")
    want, M = B.tangent(o, o["v_w"], o["v_b"], idx, y_pool, 1)
    stride = n * h * w * c + 4
    out, sd = RowOut(n * oh * ow, c), slabs_dev(o["slabs"], stride)
    _lib.check(lib.hf_pool_bn_act_tangent_nhwc(out.ptr, 0, p(sd), splits, stride, p(ad), p(md), p(rd), p(wd), p(vwd),
                                               p(vbd), p(idxd), p(yd), 1, n, h, w, oh, ow, c, F32, st()), "tangent")
    err = (out.val.cpu().double() - want.reshape(-1, c)).abs()
    bound = (splits + 6) * U32 * M.reshape(-1, c)
    assert bool((err[bound == 0] == 0).all())
    within(float((err / bound.clamp_min(1e-300)).max()), 1.0, strict=False, note="tangent")
    # the dense tangent of the unpooled kernel, gathered and masked
    dense = torch.full((n, h * w, c), NAN, device=DEV)
    _lib.check(lib.hf_chan_affine_ex(p(dense), p(sd), p(ad), p(md), p(rd), p(wd), p(vwd), p(vbd), None, None, 0, n, c, h * w,
                                     1, 0, 0, splits, stride, F32, st()), "hf_chan_affine_ex")
    gathered = torch.gather(dense, 1, idxd.view(n, oh * ow, c).long())
    gathered = torch.where(yd.view(n, oh * ow, c) > 0, gathered, torch.zeros_like(gathered))
    assert torch.equal(out.val.reshape(n, oh * ow, c).view(torch.int32), gathered.view(torch.int32))

    r = B.adjoint(o, idx, y_pool, 1, h, w, k, s, pd, rb)
    assert r["windows"] >= 2
    slab, rows = n * oh * ow * c + 4, n * h * w
    ga, g, gw, gb, gd = RowOut(rows, c), RowOut(rows, c), RowOut(rb, c), RowOut(rb, c), slabs_dev(o["gy"], slab)
    _lib.check(lib.hf_pool_bn_act_adjoint_nhwc(ga.ptr, g.ptr, gw.ptr, gb.ptr, rb, p(gd), gy_splits, slab, p(ad), p(md), p(rd),
                                               p(wd), p(idxd), p(yd), 1, n, h, w, oh, ow, c, k, k, s, s, pd, pd, F32, st()),
               "adjoint")
    R_ = gy_splits * r["windows"] + 2
    sc = (o["w"].double() * o["rstd"].double()).abs()
    for name, got, ref, bound in (("g", g, r["g"], R_ * U32 * r["M"]), ("ga", ga, r["ga"], (R_ + 2) * U32 * r["M"] * sc),
                                  ("gb", gb, r["gb"], R_ * U32 * r["Mb"]), ("gw", gw, r["gw"], (R_ + 4) * U32 * r["Mw"])):
        err, bound = (got.val.cpu().double() - ref.reshape(-1, c)).abs(), bound.reshape(-1, c)
        assert bool((err[bound == 0] == 0).all()), name
        within(float((err / bound.clamp_min(1e-300)).max()), 1.0, strict=False, note=name)
    ga0 = RowOut(rows, c)
    _lib.check(lib.hf_pool_act_adjoint_nhwc(ga0.ptr, None, 0, p(gd), gy_splits, slab, p(idxd), p(yd), 1, n, h, w, oh, ow, c,
                                            k, k, s, s, pd, pd, F32, st()), "hf_pool_act_adjoint_nhwc")
    assert g.same(ga0), "g is not the bias form's ga"
    scaled = RowOut(rows, c)
    _lib.check(lib.hf_bn_adjoint_v4(None, scaled.ptr, g.ptr, 1, 0, None, 1, 0, None, p(wd), p(rd), rows, c, F32, st()),
               "hf_bn_adjoint_v4")
    assert ga.same(scaled), "ga is not hf_bn_adjoint_v4's scaling of g"
    # the one-pixel-per-thread form (no sums) writes the same g and ga
    ga1, g1 = RowOut(rows, c), RowOut(rows, c)
    _lib.check(lib.hf_pool_bn_act_adjoint_nhwc(ga1.ptr, g1.ptr, None, None, 0, p(gd), gy_splits, slab, p(ad), p(md), p(rd),
                                               p(wd), p(idxd), p(yd), 1, n, h, w, oh, ow, c, k, k, s, s, pd, pd, F32, st()),
               "adjoint, elementwise")
    torch.cuda.synchronize()
    assert ga1.same(ga) and g1.same(g)


def test_refusals_return_err_arg_and_leave_the_outputs_alone():
    n, c, h, w, k, s, pd = 2, 4, 5, 7, 3, 2, 0
    o = B.case(n, c, h, w, k, s, pd, 2, 2)
    y_pool, idx = B.forward(o, k, s, pd, 1)
    oh, ow = o["oh"], o["ow"]
    full, pooled = n * h * w * c, n * oh * ow * c
    sd, gd = slabs_dev(o["slabs"], full + 4), slabs_dev(o["gy"], pooled + 4)
    idxd, yd = idx.to(torch.int32).to(DEV), y_pool.to(DEV)
    ad, md, rd, wd, vwd, vbd = _dev(o, "a", "mean", "rstd", "w", "v_w", "v_b")
    lib, F32, big = _lib.load(), _lib.HF_F32, 1 << 20
    MAXS = 1024  # HF_POOL_ACT_MAX_SPLITS of include/hf_pcg.h

    out = RowOut(n * oh * ow, c, 2 * c)
    good_t = dict(out=out.ptr, out_ld=2 * c, slabs=p(sd), splits=2, stride=full + 4, a=p(ad), mean=p(md), rstd=p(rd),
                  w_=p(wd), v_w=p(vwd), v_b=p(vbd), idx=p(idxd), y=p(yd), relu=1, n=n, h=h, w=w, oh=oh, ow=ow, c=c, dtype=F32)

    def tangent(**kw):
        a = dict(good_t, **kw)
        return lib.hf_pool_bn_act_tangent_nhwc(a["out"], a["out_ld"], a["slabs"], a["splits"], a["stride"], a["a"],
                                               a["mean"], a["rstd"], a["w_"], a["v_w"], a["v_b"], a["idx"], a["y"],
                                               a["relu"], a["n"], a["h"], a["w"], a["oh"], a["ow"], a["c"], a["dtype"], st())

    for bad in (dict(out=None), dict(slabs=None), dict(idx=None), dict(y=None), dict(splits=0), dict(splits=MAXS + 1),
                dict(stride=full - 1), dict(out_ld=c - 1), dict(oh=0), dict(n=big, h=64, w=64), dict(n=big, oh=64, ow=64),
                dict(dtype=_lib.HF_F64), dict(a=None), dict(mean=None), dict(rstd=None), dict(w_=None)):
        assert tangent(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())
    assert tangent() == 0 and tangent(y=None, relu=0) == 0 and tangent(v_b=None) == 0 and tangent(v_w=None) == 0

    outs = dict(ga=RowOut(n * h * w, c), g=RowOut(n * h * w, c), gw=RowOut(3, c), gb=RowOut(3, c))
    good_a = dict({name: t.ptr for name, t in outs.items()}, rb=3, gy=p(gd), splits=2, slab=pooled + 4, a=p(ad), mean=p(md),
                  rstd=p(rd), w_=p(wd), idx=p(idxd), y=p(yd), relu=1, n=n, h=h, w=w, oh=oh, ow=ow, c=c, k=k, s=s, pd=pd,
                  dtype=F32)

    def adjoint(**kw):
        a = dict(good_a, **kw)
        return lib.hf_pool_bn_act_adjoint_nhwc(a["ga"], a["g"], a["gw"], a["gb"], a["rb"], a["gy"], a["splits"], a["slab"],
                                               a["a"], a["mean"], a["rstd"], a["w_"], a["idx"], a["y"], a["relu"], a["n"],
                                               a["h"], a["w"], a["oh"], a["ow"], a["c"], a["k"], a["k"], a["s"], a["s"],
                                               a["pd"], a["pd"], a["dtype"], st())

    for bad in (dict(ga=None), dict(gy=None), dict(idx=None), dict(y=None), dict(splits=0), dict(splits=MAXS + 1),
                dict(slab=pooled - 1), dict(oh=oh + 1), dict(ow=ow - 1), dict(k=0), dict(s=0), dict(pd=-1),
                dict(rb=0), dict(rb=n * h * w + 1), dict(rb=64),  # 70 rows: ceil(70/64) = 2, share 35 starts at row 70
                dict(rb=64, gb=None),  # (gw alone needs the same valid row geometry)
                dict(n=big, h=2049, w=2049, oh=1024, ow=1024), dict(dtype=_lib.HF_F64),
                dict(a=None), dict(mean=None), dict(rstd=None), dict(w_=None)):
        assert adjoint(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t.buf).all()) for t in outs.values())
    assert adjoint() == 0 and adjoint(gw=None, gb=None, rb=0) == 0 and adjoint(y=None, relu=0) == 0
    assert adjoint(g=None) == 0 and adjoint(gw=None) == 0 and adjoint(gb=None) == 0
    torch.cuda.synchronize()
