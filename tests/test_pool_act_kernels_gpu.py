"""GPU: ``hf_pool_act_tangent_nhwc`` / ``hf_pool_act_adjoint_nhwc`` (bias + ReLU + max-pool of a plain stack's pooled
layer, one launch per sweep direction) through the C ABI against the float64 references of ``pool_act_refs`` -- no
engine, no ``modelprep``.

Operands are multiples of 1/8 of magnitude <= 4: every sum is exact in fp32 in any order, so the results must equal the
float64 reference BITWISE.  ``idx`` and ``y_pool`` come from the reference (ATen's forward on tie-free planes).  One case
per kernel runs on standard-normal operands against the derived bound  (terms + 2) * 2^-24 * sum |terms|  per element
(``terms`` additions in fp32, two roundings of slack for the bias / the final rounding of a partial row)."""

import itertools

import pytest
import torch
from tol import within

from guarded import DEV, ERR_ARG, U32, RowOut, p, slabs_dev, st, twice
import pool_act_refs as R
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu

# every geometry x map x channel count; the other options cycle so that each value meets each geometry class
SHAPES = [(g, m, c) for g in R.GEOMS for m in R.MAPS for c in (4, 12)] + [((3, 2, 1), (5, 7), 3), ((2, 2, 0), (4, 4), 6)]
OPTS = list(itertools.product((1, 2, 9), (0, 1), (0, 1), (0, 1), (4, 6)))  # splits, wide out, relu, v_b, stride pad


# per-axis windows (kh != kw, sh != sw or ph != pw, each with its transpose) x both channel forms (16 bytes, element-wise)
AXIS_SHAPES = [(g, m, c) for g, m in R.AXIS_GEOMS for c in (4, 3)]
# the row-sum kernel's second pass over the channel columns (more than 256 per row): channels, row blocks, gy splits, relu
WIDE = [(258, 1, 2, 1), (258, 3, 1, 0), (1028, 1, 1, 1), (1028, 3, 2, 0)]
WIDE_GEOM, WIDE_MAP = (2, 2, 0), (4, 4)


def _opts(i):
    return OPTS[(7 * i + i // len(OPTS)) % len(OPTS)]


def _axis_opts(j):
    return OPTS[(8 * j + 3 * (j // 2)) % len(OPTS)]


def _ids(shapes):
    return dict(argvalues=range(len(shapes)), ids=lambda i: "-".join(str(x) for x in shapes[i]).replace(" ", ""))


def test_every_option_value_is_exercised():
    seen = [set() for _ in range(5)]
    for i in range(len(SHAPES)):
        for s, v in zip(seen, _opts(i)):
            s.add(v)
    assert [len(s) for s in seen] == [3, 2, 2, 2, 2]
    masked = 0  # cases with the ReLU whose pooled map has windows <= 0 (their tangents / cotangents are masked)
    for i, ((k, s, pd), (h, w), c) in enumerate(SHAPES):
        if _opts(i)[2]:
            o = R.case(2, c, h, w, k, s, pd, 1, 1)
            masked += bool((_forward(o, k, s, pd, 1)[0] <= 0).any())
    assert masked >= 8


def test_every_option_value_meets_a_per_axis_window():
    for c in (4, 3):  # in each channel form: both relu values, with and without the sums / v_b, row blocks 1 and 3
        mine = [_axis_opts(j) for j, (_g, _m, cj) in enumerate(AXIS_SHAPES) if cj == c]
        assert [len({o[k] for o in mine}) for k in range(5)] == [3, 2, 2, 2, 2], c
        rows = [o for o in mine if o[1]]  # (the row-sum kernel: only with the sums)
        assert {o[2] for o in rows} == {0, 1} and {o[3] for o in rows} == {0, 1}, c
    for g in range(len(R.AXIS_GEOMS)):  # every window runs through the row-sum kernel in one channel form at least
        assert _axis_opts(2 * g)[1] or _axis_opts(2 * g + 1)[1]
    for j, ((k, s, pd), (h, w), c) in enumerate(AXIS_SHAPES):
        assert R.exchanges((k, s, pd))
        if _axis_opts(j)[2]:
            assert bool((_forward(R.case(2, c, h, w, k, s, pd, 1, 1), k, s, pd, 1)[0] <= 0).any())
    assert {(c, rb) for c, rb, _s, _r in WIDE} == {(258, 1), (258, 3), (1028, 1), (1028, 3)}
    assert {x[2] for x in WIDE} == {1, 2} and {x[3] for x in WIDE} == {0, 1}


def _forward(o, k, s, pd, relu):
    return R.forward(o["a"], o["b"], k, s, pd, relu)


@pytest.mark.parametrize("i", **_ids(SHAPES))
def test_tangent_equals_float64_bitwise(i):
    _tangent(SHAPES[i], _opts(i))


@pytest.mark.parametrize("j", **_ids(AXIS_SHAPES))
def test_tangent_on_per_axis_windows_equals_float64_bitwise(j):
    _tangent(AXIS_SHAPES[j], _axis_opts(j))


def _tangent(shape, opts):
    ((k, s, pd), (h, w), c), n = shape, 2
    splits, wide, relu, with_vb, pad = opts
    o = R.case(n, c, h, w, k, s, pd, splits, 1)
    y_pool, idx = _forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    v_b =o["v_b"] if with_vb else None
    want, _ = R.tangent(o["slabs"], v_b, idx, y_pool, relu)
    stride = n * h * w * c + pad
    sd, vd = slabs_dev(o["slabs"], stride), (v_b.to(DEV) if with_vb else None)
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, ld, orow = _lib.load(), (2 * c if wide else 0), n * oh * ow

    def launch():
        out = RowOut(orow, c, ld)
        _lib.check(lib.hf_pool_act_tangent_nhwc(out.ptr, ld, p(sd), splits, stride, p(vd), p(idxd), p(yd), relu, n, h, w,
                                                oh, ow, c, _lib.HF_F32, st()), "hf_pool_act_tangent_nhwc")
        return out

    assert torch.equal(twice(launch).val.cpu().double(), want.reshape(orow, c))


@pytest.mark.parametrize("i", **_ids(SHAPES))
def test_adjoint_equals_float64_bitwise(i):
    gy_splits, with_gb, relu, rb3, pad = _opts(i)
    _adjoint(SHAPES[i], 2, gy_splits, with_gb, relu, 3 if rb3 else 1, pad)


@pytest.mark.parametrize("j", **_ids(AXIS_SHAPES))
def test_adjoint_on_per_axis_windows_equals_float64_bitwise(j):
    """kh, kw, stride_h, stride_w, pad_h, pad_w each reach their own axis: the reference with any unequal pair exchanged
    differs on these operands (asserted), and the kernel equals the right one."""
    gy_splits, with_gb, relu, rb3, pad = _axis_opts(j)
    _adjoint(AXIS_SHAPES[j], 2, gy_splits, with_gb, relu, 3 if rb3 else 1, pad)


@pytest.mark.parametrize("c, row_blocks, gy_splits, relu", WIDE, ids=lambda v: str(v))
def test_adjoint_row_sums_beyond_256_channel_columns_equal_float64_bitwise(c, row_blocks, gy_splits, relu):
    """c = 258: the element-wise form, 258 columns -- a second pass with 2 live columns; c = 1028: the 16-byte form, 257
    quads -- a second pass with one.  The reduction buffer is reused between the passes."""
    _adjoint((WIDE_GEOM, WIDE_MAP, c), 1, gy_splits, 1, relu, row_blocks, 4)


def _adjoint(shape, n, gy_splits, with_gb, relu, row_blocks, pad):
    (k, s, pd), (h, w), c = shape
    (kh, kw), (sh, sw), (ph, pw) = R.pair(k), R.pair(s), R.pair(pd)
    o = R.case(n, c, h, w, k, s, pd, 1, gy_splits)
    y_pool, idx = _forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    want, _, want_gb, _ = R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, pd, row_blocks)
    for name, (k2, s2, p2) in R.exchanges((k, s, pd)):
        assert not torch.equal(R.adjoint(o["gy"], idx, y_pool, relu, h, w, k2, s2, p2)[0], want), name
    slab = n * oh * ow * c + pad
    gd = slabs_dev(o["gy"], slab)
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, rows = _lib.load(), n * h * w

    def launch():
        ga, gb = RowOut(rows, c), (RowOut(row_blocks, c) if with_gb else None)
        _lib.check(lib.hf_pool_act_adjoint_nhwc(ga.ptr, gb.ptr if gb else None, row_blocks, p(gd), gy_splits, slab,
                                                p(idxd), p(yd), relu, n, h, w, oh, ow, c, kh, kw, sh, sw, ph, pw,
                                                _lib.HF_F32, st()), "hf_pool_act_adjoint_nhwc")
        return ga, gb

    a = twice(launch)
    assert torch.equal(a[0].val.cpu().double(), want.reshape(rows, c))
    if with_gb:
        assert torch.equal(a[1].val.cpu().double(), want_gb)


def test_random_operands_within_the_derived_bound():
    """Standard-normal operands: per element  (additions + 2) * 2^-24 * sum |terms|  -- the tangent adds ``splits`` slabs
    and the bias, the adjoint ``gy_splits`` slabs for each of up to ``windows`` windows; a partial row of the bias sums
    adds its share's elements in fp64 and rounds once (inside the + 2)."""
    n, c, h, w, k, s, pd, splits, gy_splits, rb = 2, 12, 5, 7, 3, 2, 1, 9, 9, 3
    o = R.case(n, c, h, w, k, s, pd, splits, gy_splits, exact=False)
    y_pool, idx = _forward(o, k, s, pd, 1)
    oh, ow = o["oh"], o["ow"]
    lib = _lib.load()
    idxd, yd = idx.to(torch.int32).to(DEV), y_pool.to(DEV)
    want, M = R.tangent(o["slabs"], o["v_b"], idx, y_pool, 1)
    stride = n * h * w * c + 4
    out, sd, vd = RowOut(n * oh * ow, c), slabs_dev(o["slabs"], stride), o["v_b"].to(DEV)
    _lib.check(lib.hf_pool_act_tangent_nhwc(out.ptr, 0, p(sd), splits, stride, p(vd), p(idxd), p(yd), 1, n, h, w, oh, ow,
                                            c, _lib.HF_F32, st()), "hf_pool_act_tangent_nhwc")
    err = (out.val.cpu().double() - want.reshape(-1, c)).abs()
    bound = (splits + 2) * U32 * M.reshape(-1, c)
    assert bool((err[bound == 0] == 0).all())
    within(float((err / bound.clamp_min(1e-300)).max()), 1.0, strict=False, note="tangent")
    want_ga, Mg, want_gb, windows = R.adjoint(o["gy"], idx, y_pool, 1, h, w, k, s, pd, rb)
    assert windows >= 2
    slab = n * oh * ow * c + 4
    ga, gb, gd = RowOut(n * h * w, c), RowOut(rb, c), slabs_dev(o["gy"], slab)
    _lib.check(lib.hf_pool_act_adjoint_nhwc(ga.ptr, gb.ptr, rb, p(gd), gy_splits, slab, p(idxd), p(yd), 1, n, h, w, oh,
                                            ow, c, k, k, s, s, pd, pd, _lib.HF_F32, st()), "hf_pool_act_adjoint_nhwc")
    R_ = gy_splits * windows + 2
    err = (ga.val.cpu().double() - want_ga.reshape(-1, c)).abs()
    bound = R_ * U32 * Mg.reshape(-1, c)
    assert bool((err[bound == 0] == 0).all())
    within(float((err / bound.clamp_min(1e-300)).max()), 1.0, strict=False, note="adjoint")
    rows, per = n * h * w, -(-n * h * w // rb)
    Mb = torch.stack([Mg.reshape(rows, c)[b * per:(b + 1) * per].sum(0) for b in range(rb)])
    errb = (gb.val.cpu().double() - want_gb).abs()
    within(float((errb / (R_ * U32 * Mb).clamp_min(1e-300)).max()), 1.0, strict=False, note="bias rows")


def test_refusals_return_err_arg_and_leave_the_outputs_alone():
    n, c, h, w, k, s, pd = 2, 4, 5, 7, 3, 2, 0
    o = R.case(n, c, h, w, k, s, pd, 2, 2)
    y_pool, idx = _forward(o, k, s, pd, 1)
    oh, ow = o["oh"], o["ow"]
    full, pooled = n * h * w * c, n * oh * ow * c
    sd, gd = slabs_dev(o["slabs"], full + 4), slabs_dev(o["gy"], pooled + 4)
    idxd, yd, vd = idx.to(torch.int32).to(DEV), y_pool.to(DEV), o["v_b"].to(DEV)
    lib, F32, big = _lib.load(), _lib.HF_F32, 1 << 20
    MAXS = 1024  # HF_POOL_ACT_MAX_SPLITS of include/hf_pcg.h

    out = RowOut(n * oh * ow, c, 2 * c)
    good_t = dict(out=out.ptr, out_ld=2 * c, slabs=p(sd), splits=2, stride=full + 4, v_b=p(vd), idx=p(idxd), y=p(yd),
                  relu=1, n=n, h=h, w=w, oh=oh, ow=ow, c=c, dtype=F32)

    def tangent(**kw):
        a = dict(good_t, **kw)
        return lib.hf_pool_act_tangent_nhwc(a["out"], a["out_ld"], a["slabs"], a["splits"], a["stride"], a["v_b"], a["idx"],
                                            a["y"], a["relu"], a["n"], a["h"], a["w"], a["oh"], a["ow"], a["c"], a["dtype"],
                                            st())

    for bad in (dict(out=None), dict(slabs=None), dict(idx=None), dict(y=None), dict(splits=0), dict(splits=MAXS + 1),
                dict(stride=full - 1), dict(out_ld=c - 1), dict(oh=0), dict(n=big, h=64, w=64), dict(n=big, oh=64, ow=64),
                dict(dtype=_lib.HF_F64)):
        assert tangent(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())
    assert tangent() == 0 and tangent(y=None, relu=0) == 0 and tangent(v_b=None) == 0  # (the complete call is taken)

    ga, gb = RowOut(n * h * w, c), RowOut(3, c)
    good_a = dict(ga=ga.ptr, gb=gb.ptr, rb=3, gy=p(gd), splits=2, slab=pooled + 4, idx=p(idxd), y=p(yd), relu=1, n=n, h=h,
                  w=w, oh=oh, ow=ow, c=c, k=k, s=s, pd=pd, dtype=F32)

    def adjoint(**kw):
        a = dict(good_a, **kw)
        return lib.hf_pool_act_adjoint_nhwc(a["ga"], a["gb"], a["rb"], a["gy"], a["splits"], a["slab"], a["idx"], a["y"],
                                            a["relu"], a["n"], a["h"], a["w"], a["oh"], a["ow"], a["c"], a["k"], a["k"],
                                            a["s"], a["s"], a["pd"], a["pd"], a["dtype"], st())

    for bad in (dict(ga=None), dict(gy=None), dict(idx=None), dict(y=None), dict(splits=0), dict(splits=MAXS + 1),
                dict(slab=pooled - 1), dict(oh=oh + 1), dict(ow=ow - 1), dict(k=0), dict(s=0), dict(pd=-1),
                dict(rb=0), dict(rb=n * h * w + 1), dict(rb=64),  # 70 rows: ceil(70/64) = 2, share 35 starts at row 70
                dict(n=big, h=2049, w=2049, oh=1024, ow=1024), dict(dtype=_lib.HF_F64)):
        assert adjoint(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(ga.buf).all()) and bool(torch.isnan(gb.buf).all())
    assert adjoint() == 0 and adjoint(gb=None, rb=0) == 0 and adjoint(y=None, relu=0) == 0
    torch.cuda.synchronize()
