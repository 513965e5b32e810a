"""GPU: ``hf_pool_bn_act_tangent_train_nhwc`` / ``hf_pool_bn_act_adjoint_reduce_nhwc`` (the pooled unit of a plain stack
with a TRAIN-mode BatchNorm) through the C ABI -- no engine, no ``modelprep``.

The header's contracts, bitwise: the tangent is ``hf_chan_affine_train``'s unmasked dense output on the same operands,
gathered at ``idx`` and masked by the pooled map, in the 16-byte and the element-wise form; the reduction pass writes the
``g`` / ``gw`` / ``gb`` of ``hf_pool_bn_act_adjoint_nhwc``.  Against the float64 references of ``pool_bn_train_refs`` the
tangent is held to the bound of the ``hf_chan_affine_train`` tests (``test_layer_kernels_gpu.py``: the same arithmetic,
``layer_refs.r_chan_affine_train`` roundings of 2^-24 on the sum of the terms' magnitudes), the reduction pass to the
bounds of ``test_pool_bn_act_kernels_gpu.py``.  The shapes are the smallest on which the kernels can go wrong (n = 2,
5x5 -> 2x2 by 3/2 windows, 6x4 -> 3x2 by 2/2 windows, 8 and 12 channels)."""

import pytest
import torch
from tol import within

from guarded import DEV, ERR_ARG, NAN, P, U32, RowOut, p, slabs_dev, st, twice
import layer_refs as L
import pool_bn_train_refs as T
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
B = T.B
ERR_ALIGN = -2  # HF_ERR_ALIGN of include/hf_pcg.h
N = 2
# tangent cases: geometry, channels, nparts choice, splits, relu, which of v_w / v_b is null, out_ld form
#   (0: dense, 1: 2c -- the consumer's [t_x | x] operand, 2: 2c + 2 -- no multiple of 4: the element-wise form)
T_CASES = [(i % 2, (8, 12)[(i // 2) % 2], (i // 4) % 3, (1, 3)[(i // 12) % 2], (i + i // 2 + i // 4) % 2,
            ("", "w", "b")[(i + i // 4) % 3], (i // 2 + i // 12) % 3) for i in range(24)]
# reduction cases: geometry, channels, gy splits, relu, row blocks
A_CASES = [(i % 2, (8, 12)[(i // 2) % 2], (1, 3)[(i // 4) % 2], (i + i // 4) % 2, (1, 3)[(i // 2 + i // 8) % 2])
           for i in range(16)]
# per-axis windows (``pool_act_refs.AXIS_GEOMS``: geometry = its index there).  The tangent takes multiples of 4 channels
# only: 4, its 16-byte form on even cases and the element-wise form (out_ld = 2c + 2) on odd ones; the reduction pass runs
# 4 channels (16 bytes) and 3 (element-wise) on every window
AXIS_T_CASES = [(j // 2, 4, (j + j // 6) % 3, (1, 3)[(j // 2 + j // 6) % 2], (j // 2 + j // 4) % 2,
                 ("", "w", "b")[(j // 2) % 3], 2 if j % 2 else (j // 2) % 2) for j in range(12)]
AXIS_A_CASES = [(j // 2, (4, 3)[j % 2], (1, 3)[(j // 2 + j // 6) % 2], (j + j // 4) % 2, (1, 3)[(j // 2 + j // 4) % 2])
                for j in range(12)]
# the row-sum kernel beyond 256 channel columns, in its form without ga: channels, row blocks, gy splits, relu
WIDE = [(258, 1, 2, 1), (258, 3, 1, 0), (1028, 1, 1, 1), (1028, 3, 2, 0)]


def test_every_option_value_is_exercised():
    for c in (8, 12):
        mine = [t for t in T_CASES if t[1] == c]
        assert {t[0] for t in mine} == {0, 1} and {t[2] for t in mine} == {0, 1, 2} and {t[3] for t in mine} == {1, 3}
        assert {t[4] for t in mine} == {0, 1} and {t[5] for t in mine} == {"", "w", "b"} and {t[6] for t in mine} == {0, 1, 2}
        assert T.nparts_choices(c)[2] > T.FCS_BATCH * (T.BLOCK // (c // 4))
        mine = [t for t in A_CASES if t[1] == c]
        assert all({t[j] for t in mine} == vals for j, vals in ((0, {0, 1}), (2, {1, 3}), (3, {0, 1}), (4, {1, 3})))


def test_every_option_value_meets_a_per_axis_window():
    assert {t[0] for t in AXIS_T_CASES} == {t[0] for t in AXIS_A_CASES} == set(range(len(T.AXIS_GEOMS)))
    for quad in (True, False):  # the tangent's two forms
        mine = [t for t in AXIS_T_CASES if (t[6] != 2) == quad]
        assert {t[0] for t in mine} == set(range(len(T.AXIS_GEOMS)))
        assert {t[2] for t in mine} == {0, 1, 2} and {t[3] for t in mine} == {1, 3} and {t[4] for t in mine} == {0, 1}
        assert {t[5] for t in mine} == {"", "w", "b"}
    assert {t[6] for t in AXIS_T_CASES} == {0, 1, 2}
    for c in (4, 3):
        mine = [t for t in AXIS_A_CASES if t[1] == c]
        assert {t[0] for t in mine} == set(range(len(T.AXIS_GEOMS)))
        assert all({t[j] for t in mine} == vals for j, vals in ((2, {1, 3}), (3, {0, 1}), (4, {1, 3})))
        assert {(t[3], t[4]) for t in mine} >= {(0, 3), (1, 1)}
    assert {(c, rb) for c, rb, _s, _r in WIDE} == {(258, 1), (258, 3), (1028, 1), (1028, 3)}


def _dev(o, *names):
    return [o[k].to(DEV) for k in names]


def _slice(t, off):
    """``t`` on the device at ``off`` floats behind a 16-byte boundary: a slice of the flat vector."""
    if t is None:
        return None
    buf = torch.zeros(t.numel() + 8, device=DEV)
    buf[off:off + t.numel()] = t.to(DEV)
    v = buf[off:off + t.numel()]
    assert v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("case", T_CASES, ids=lambda t: "-".join(str(x) for x in t))
def test_tangent_is_the_train_kernels_dense_output_gathered_and_within_its_bound(case):
    _tangent(T.GEOMS[case[0]], case)


@pytest.mark.parametrize("case", AXIS_T_CASES, ids=lambda t: "-".join(str(x) for x in t))
def test_tangent_on_per_axis_windows_is_the_dense_output_gathered_and_within_its_bound(case):
    _tangent(T.AXIS_GEOMS[case[0]], case)


def _tangent(geom, case):
    _gi, c, npi, splits, relu, null, ldk = case
    (k, s, pd), (h, w) = geom
    nparts = T.nparts_choices(c)[npi]
    o = T.case(N, c, h, w, k, s, pd, splits, 1, nparts)
    y_pool, idx = B.forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    v_w, v_b = (None if null == "w" else o["v_w"]), (None if null == "b" else o["v_b"])
    want, M = T.tangent(o, v_w, v_b, idx, y_pool, relu)
    stride = N * h * w * c + 4
    sd = slabs_dev(o["slabs"], stride)
    ad, md, rd, wd, pxd, p1d = _dev(o, "a", "mean", "rstd", "w", "part_x", "part_1")
    # (12 channels: the slices sit 1 and 2 floats behind a 16-byte boundary, as behind odd-sized entries of the vector)
    vwd, vbd = _slice(v_w, 1 if c == 12 else 0), _slice(v_b, 2 if c == 12 else 0)
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, F32, ld, orow = _lib.load(), _lib.HF_F32, (0, 2 * c, 2 * c + 2)[ldk], N * oh * ow

    def launch():
        out = RowOut(orow, c, ld)
        _lib.check(lib.hf_pool_bn_act_tangent_train_nhwc(
            out.ptr, ld, p(sd), splits, stride, p(ad), p(md), p(rd), p(wd), p(vwd), p(vbd), p(pxd), p(p1d), nparts,
            o["count"], p(idxd), p(yd), relu, N, h, w, oh, ow, c, F32, st()), "hf_pool_bn_act_tangent_train_nhwc")
        return out

    a, b = launch(), launch()
    dense = torch.full((N, h * w, c), NAN, device=DEV)
    _lib.check(lib.hf_chan_affine_train(p(dense), p(sd), p(ad), p(md), p(rd), p(wd), p(pxd), p(p1d), nparts, p(vwd), p(vbd),
                                        o["count"], None, None, N, c, h * w, 0, 0, splits, stride, F32, st()),
               "hf_chan_affine_train")
    torch.cuda.synchronize()
    assert a.same(b), "two launches on the same operands differ"
    assert a.untouched(), "the other half of the wider buffer or a guard word was written"
    gathered = torch.gather(dense, 1, idxd.view(N, oh * ow, c).long())
    if relu:
        gathered = torch.where(yd.view(N, oh * ow, c) > 0, gathered, torch.zeros_like(gathered))
    assert torch.equal(a.val.reshape(N, oh * ow, c).contiguous().view(torch.int32), gathered.view(torch.int32))
    R = L.r_chan_affine_train(splits, False)
    ratio = L.ratio(a.val.cpu(), want.reshape(orow, c), M.reshape(orow, c), R)
    print(f"tangent {case}: {ratio:.3f} of the bound (R = {R})")
    within(ratio, 1.0, strict=False, note=case)
    if relu:
        assert bool((a.val[~(yd.view(orow, c) > 0)] == 0).all())


@pytest.mark.parametrize("case", A_CASES, ids=lambda t: "-".join(str(x) for x in t))
def test_reduce_writes_the_fused_entry_points_g_and_sums_and_no_ga(case):
    _reduce(T.GEOMS[case[0]], case)


@pytest.mark.parametrize("case", AXIS_A_CASES, ids=lambda t: "-".join(str(x) for x in t))
def test_reduce_on_per_axis_windows_writes_g_and_sums_and_no_ga(case):
    """kh, kw, stride_h, stride_w, pad_h, pad_w each reach their own axis: with any unequal pair exchanged the reference
    moves by more than 1000 x the bound (``test_pool_bn_train_refs_cpu.py``), and the bound here is the square cases'."""
    _reduce(T.AXIS_GEOMS[case[0]], case)


@pytest.mark.parametrize("c, rb, gy_splits, relu", WIDE, ids=lambda v: str(v))
def test_reduce_row_sums_beyond_256_channel_columns_equal_float64_bitwise(c, rb, gy_splits, relu):
    """c = 258: the element-wise form, 258 columns -- a second pass with 2 live columns; c = 1028: the 16-byte form, 257
    quads.  Dyadic operands (``pool_bn_act_refs.case``): g, gw and gb equal the float64 reference bitwise, and nothing is
    written where the fused entry point's ga would be."""
    n, (k, s, pd), (h, w) = 1, (2, 2, 0), (4, 4)
    o = B.case(n, c, h, w, k, s, pd, 1, gy_splits)
    y_pool, idx = B.forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    want = B.adjoint(o, idx, y_pool, relu, h, w, k, s, pd, rb)
    slab, rows = n * oh * ow * c + 4, n * h * w
    gd = slabs_dev(o["gy"], slab)
    ad, md, rd, wd = _dev(o, "a", "mean", "rstd", "w")
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib = _lib.load()

    def launch():
        both, gw, gb = RowOut(2 * rows, c), RowOut(rb, c), RowOut(rb, c)
        g_ptr = P(both.buf.data_ptr() + 4 * rows * c)
        _lib.check(lib.hf_pool_bn_act_adjoint_reduce_nhwc(
            g_ptr, gw.ptr, gb.ptr, rb, p(gd), gy_splits, slab, p(ad), p(md), p(rd), p(wd), p(idxd), p(yd), relu, n, h, w, oh,
            ow, c, k, k, s, s, pd, pd, _lib.HF_F32, st()), "hf_pool_bn_act_adjoint_reduce_nhwc")
        return both, gw, gb

    both, gw, gb = twice(launch)
    assert bool(torch.isnan(both.val[:rows]).all()), "something was written where ga would be"
    assert torch.equal(both.val[rows:].cpu().double(), want["g"].reshape(rows, c)), "g"
    assert torch.equal(gw.val.cpu().double(), want["gw"]), "gw"
    assert torch.equal(gb.val.cpu().double(), want["gb"]), "gb"


def _reduce(geom, case):
    _gi, c, gy_splits, relu, rb = case
    (k, s, pd), (h, w) = geom
    (kh, kw), (sh, sw), (ph, pw) = B.pair(k), B.pair(s), B.pair(pd)
    o = T.case(N, c, h, w, k, s, pd, 1, gy_splits, 1)
    y_pool, idx = B.forward(o, k, s, pd, relu)
    oh, ow = o["oh"], o["ow"]
    r = T.adjoint_reduce(o, idx, y_pool, relu, h, w, k, s, pd, rb)
    slab, rows = N * oh * ow * c + 4, N * h * w
    gd = slabs_dev(o["gy"], slab)
    ad, md, rd, wd = _dev(o, "a", "mean", "rstd", "w")
    idxd, yd = idx.to(torch.int32).to(DEV), (y_pool.to(DEV) if relu else None)
    lib, F32 = _lib.load(), _lib.HF_F32
    tail = (p(gd), gy_splits, slab, p(ad), p(md), p(rd), p(wd), p(idxd), p(yd), relu, N, h, w, oh, ow, c, kh, kw, sh, sw, ph,
            pw, F32)

    def launch():
        # g sits where the fused entry point's argument order has it: behind a map-sized region where ga would be
        both, gw, gb = RowOut(2 * rows, c), RowOut(rb, c), RowOut(rb, c)
        g_ptr = P(both.buf.data_ptr() + 4 * rows * c)
        _lib.check(lib.hf_pool_bn_act_adjoint_reduce_nhwc(g_ptr, gw.ptr, gb.ptr, rb, *tail, st()),
                   "hf_pool_bn_act_adjoint_reduce_nhwc")
        return both, gw, gb

    (both, gw, gb), second = launch(), launch()
    ga0, g0, gw0, gb0 = RowOut(rows, c), RowOut(rows, c), RowOut(rb, c), RowOut(rb, c)
    _lib.check(lib.hf_pool_bn_act_adjoint_nhwc(ga0.ptr, g0.ptr, gw0.ptr, gb0.ptr, rb, *tail, st()),
               "hf_pool_bn_act_adjoint_nhwc")
    torch.cuda.synchronize()
    for x, y in zip((both, gw, gb), second):
        assert x.same(y), "two launches on the same operands differ"
        assert x.untouched()
    assert bool(torch.isnan(both.val[:rows]).all()), "something was written where ga would be"
    g = both.val[rows:]
    assert torch.equal(g.contiguous().view(torch.int32), g0.val.contiguous().view(torch.int32)), "g"
    assert gw.same(gw0) and gb.same(gb0), "the sum rows are not the fused entry point's"
    assert r["windows"] >= 1
    R_ = gy_splits * r["windows"] + 2
    for name, got, ref, bound in (("g", g, r["g"], R_ * U32 * r["M"]), ("gb", gb.val, r["gb"], R_ * U32 * r["Mb"]),
                                  ("gw", gw.val, r["gw"], (R_ + 4) * U32 * r["Mw"])):
        err, bound = (got.cpu().double() - ref.reshape(-1, c)).abs(), bound.reshape(-1, c)
        assert bool((err[bound == 0] == 0).all()), name
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"reduce {case} {name}: {ratio:.3f} of the bound")
        within(ratio, 1.0, strict=False, note=(case, name))


def test_refusals_come_before_any_launch():
    c, ((k, s, pd), (h, w)) = 8, T.GEOMS[0]
    o = T.case(N, c, h, w, k, s, pd, 2, 2, 3)
    y_pool, idx = B.forward(o, k, s, pd, 1)
    oh, ow = o["oh"], o["ow"]
    full, pooled = N * h * w * c, N * oh * ow * c
    sd, gd = slabs_dev(o["slabs"], full + 4), slabs_dev(o["gy"], pooled + 4)
    idxd, yd = idx.to(torch.int32).to(DEV), y_pool.to(DEV)
    ad, md, rd, wd, vwd, vbd, pxd, p1d = _dev(o, "a", "mean", "rstd", "w", "v_w", "v_b", "part_x", "part_1")
    lib, F32, big = _lib.load(), _lib.HF_F32, 1 << 20
    MAXS = 1024  # HF_POOL_ACT_MAX_SPLITS of include/hf_pcg.h
    off = torch.zeros(3 * c + 4, device=DEV)[1:]  # partial rows one float behind a 16-byte boundary

    out = RowOut(N * oh * ow, c, 2 * c)
    good_t = dict(out=out.ptr, out_ld=2 * c, slabs=p(sd), splits=2, stride=full + 4, a=p(ad), mean=p(md), rstd=p(rd),
                  w_=p(wd), v_w=p(vwd), v_b=p(vbd), px=p(pxd), p1=p(p1d), nparts=3, count=o["count"], idx=p(idxd), y=p(yd),
                  relu=1, n=N, h=h, w=w, oh=oh, ow=ow, c=c, dtype=F32)

    def tangent(**kw):
        a = dict(good_t, **kw)
        return lib.hf_pool_bn_act_tangent_train_nhwc(
            a["out"], a["out_ld"], a["slabs"], a["splits"], a["stride"], a["a"], a["mean"], a["rstd"], a["w_"], a["v_w"],
            a["v_b"], a["px"], a["p1"], a["nparts"], a["count"], a["idx"], a["y"], a["relu"], a["n"], a["h"], a["w"], a["oh"],
            a["ow"], a["c"], a["dtype"], st())

    for bad in (dict(out=None), dict(slabs=None), dict(idx=None), dict(y=None), dict(splits=0), dict(splits=MAXS + 1),
                dict(stride=full - 1), dict(out_ld=c - 1), dict(oh=0), dict(n=big, h=64, w=64), dict(n=big, oh=64, ow=64),
                dict(dtype=_lib.HF_F64), dict(a=None), dict(mean=None), dict(rstd=None), dict(w_=None),
                dict(px=None), dict(p1=None), dict(nparts=0), dict(nparts=-1), dict(count=0.0), dict(count=-50.0),
                dict(count=NAN), dict(c=6, out_ld=12), dict(c=1028, out_ld=2056)):
        assert tangent(**bad) == ERR_ARG, bad
    assert tangent(px=p(off)) == ERR_ALIGN and tangent(p1=p(off)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())
    assert tangent() == 0 and tangent(y=None, relu=0) == 0 and tangent(v_b=None) == 0 and tangent(v_w=None) == 0

    outs = dict(g=RowOut(N * h * w, c), gw=RowOut(3, c), gb=RowOut(3, c))
    good_a = dict({name: t.ptr for name, t in outs.items()}, rb=3, gy=p(gd), splits=2, slab=pooled + 4, a=p(ad), mean=p(md),
                  rstd=p(rd), w_=p(wd), idx=p(idxd), y=p(yd), relu=1, n=N, h=h, w=w, oh=oh, ow=ow, c=c, k=k, s=s, pd=pd,
                  dtype=F32)

    def reduce(**kw):
        a = dict(good_a, **kw)
        return lib.hf_pool_bn_act_adjoint_reduce_nhwc(a["g"], a["gw"], a["gb"], a["rb"], a["gy"], a["splits"], a["slab"],
                                                      a["a"], a["mean"], a["rstd"], a["w_"], a["idx"], a["y"], a["relu"],
                                                      a["n"], a["h"], a["w"], a["oh"], a["ow"], a["c"], a["k"], a["k"],
                                                      a["s"], a["s"], a["pd"], a["pd"], a["dtype"], st())

    rows = N * h * w
    for bad in (dict(g=None), dict(gw=None), dict(gb=None), dict(gy=None), dict(idx=None), dict(y=None), dict(splits=0),
                dict(splits=MAXS + 1), dict(slab=pooled - 1), dict(oh=oh + 1), dict(ow=ow - 1), dict(k=0), dict(s=0),
                dict(pd=-1), dict(rb=0), dict(rb=rows + 1), dict(rb=rows - 1),  # (an empty last share)
                dict(n=big, h=2049, w=2049, oh=1024, ow=1024), dict(dtype=_lib.HF_F64),
                dict(a=None), dict(mean=None), dict(rstd=None), dict(w_=None)):
        assert reduce(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t.buf).all()) for t in outs.values())
    assert reduce() == 0 and reduce(y=None, relu=0) == 0
    torch.cuda.synchronize()
