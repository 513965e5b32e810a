"""GPU: the train-mode BatchNorm forward kernels (``hf_bn_stats_rows``, ``hf_bn_forward_train``) and the linear
classifier head (``hf_linear_ce_head``) through the C ABI against the references of ``layer_refs`` -- the sibling of
``test_layer_kernels_gpu.py`` (same house style: CPU-seeded inputs, bounds ``R * u * M`` derived from the
kernel's order, NaN-filled destinations, guard words, two launches bitwise equal).  ``test_layer_refs_cpu.py`` shows on
the same inputs that an fp32 evaluation sits inside every bound used here and that the named wrong variants do not."""

import numpy as np
import pytest
import torch
from tol import within

from guarded import DEV, ERR_ARG, NAN, RowOut, _ids, dv, optr, p, st, twice, wide
import layer_refs as L
from layer_refs import U64
from pytorchhessianfree_amd import _lib
from pytorchhessianfree_amd.engine.tangent import head_fused_shape_ok

pytestmark = pytest.mark.gpu
ERR_ALIGN = -2  # hf_status of include/hf_pcg.h
f32 = np.float32


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _filled(values, rows, c, ld=0):
    """a ``RowOut`` that already holds ``values`` (an in-place operand: the guard words behind it still apply)"""
    out = RowOut(rows, c, ld)
    out.val.copy_(values.view(rows, c))
    return out


# ---------------------------------------------------------------------------------------------------------------
# hf_bn_stats_rows
# ---------------------------------------------------------------------------------------------------------------
def _slab_buffer(a, gap, tail):
    """the slabs [splits, rows*c] at a stride of rows*c (+ 12 floats of NaN), + one whole NaN slab behind the last"""
    splits, n = a.shape[0], a[0].numel()
    stride = n + (12 if gap else 0)
    buf = torch.full((splits + tail, stride), NAN)
    buf[:splits, :n] = a.reshape(splits, n)
    return buf.to(DEV), stride


def _stats_launch(lib, a_dev, stride, splits, rows, c, rb, want_a_out):
    part, a_out = RowOut(rb * 2, c, dtype=torch.float64), (RowOut(rows, c) if want_a_out else None)
    _lib.check(lib.hf_bn_stats_rows(optr(a_out), p(a_dev), splits, stride, part.ptr, rows, c, rb, _lib.HF_F32, st()),
               "hf_bn_stats_rows")
    return part, a_out


@pytest.mark.parametrize("rows,c,splits,rb,form", L.stats_cases(), ids=_ids)
def test_bn_stats_rows_against_exact_sums(rows, c, splits, rb, form):
    """``a_out`` bitwise the split-order fp32 sum; every partial row (sum a | sum a^2 of ITS share) within
    ``rows of the share * U64 * M`` of the exact sums, empty shares exact zeros; then the total."""
    f = L.STATS_FORMS[form]
    a = L.stats_inputs(rows, c, splits)
    ref = L.bn_stats(a, rb)
    a_dev, stride = _slab_buffer(a, f.gap, f.tail)
    lib = _lib.load()
    part, a_out = twice(lambda: _stats_launch(lib, a_dev, stride, splits, rows, c, rb, f.a_out))
    if a_out is not None:
        assert torch.equal(_bits(a_out.val.cpu()), _bits(ref.s)), "a_out is not the split-order fp32 sum"
    got = part.val.cpu().view(rb, 2, c)
    note = (rows, c, splits, rb, form)
    within(L.ratio_rows(got, ref.part, ref.Mpart, ref.R, U64), 1.0, strict=False, note=note)
    within(L.ratio(got.numpy().astype(L.LDT).sum(0), ref.part.sum(0), ref.Mpart.sum(0), rows, U64), 1.0, strict=False,
           note=note)
    for i, (lo, hi) in enumerate(L.row_shares(rows, rb)):
        if lo >= hi:
            assert not bool(got[i].any()), "an empty share is not exactly zero"


# ---------------------------------------------------------------------------------------------------------------
# hf_bn_forward_train
# ---------------------------------------------------------------------------------------------------------------
def _fwd_problem(rows, c, nparts, i, part=None):
    o, f = L.train_fwd_inputs(rows, c, nparts), L.fwd_form(i)
    if part is not None:
        o.part = part
    k = L.NS(o=o, f=f, rows=rows, c=c, nparts=nparts)
    k.b, k.res = (o.b if f.b else None), (o.res if f.res != "none" else None)
    k.mom = L.BN_MOMENTUM if f.stat != "neg" else -1.0
    k.res_ld = 2 * c if f.res == "strided" else 0
    k.ref = L.bn_forward_train(o.s, o.part, float(rows), L.BN_EPS, k.mom, o.w, k.b, k.res, f.relu,
                               *((o.rm, o.rv) if f.stat != "null" else (None, None)))
    k.R = L.r_bn_forward_train(nparts, f.b, k.res is not None)
    k.dev = L.NS(s=dv(o.s), part=dv(o.part), w=dv(o.w), b=dv(k.b), res=wide(k.res, k.res_ld))
    return k


def _fwd_launch(lib, k):
    f, rows, c, d = k.f, k.rows, k.c, k.dev
    y = RowOut(rows, c) if f.out != "y2" else None
    y2 = RowOut(rows, c, 2 * c) if f.out != "y" else None
    mean, rstd = RowOut(1, c), RowOut(1, c)
    rm, rv = _filled(dv(k.o.rm), 1, c), _filled(dv(k.o.rv), 1, c)
    give = f.stat != "null"
    _lib.check(lib.hf_bn_forward_train(optr(y), optr(y2), 2 * c if y2 is not None else 0, p(d.s), p(d.part), k.nparts,
                                       mean.ptr, rstd.ptr, rm.ptr if give else None, rv.ptr if give else None,
                                       float(rows), L.BN_EPS, k.mom, p(d.w), p(d.b), p(d.res), k.res_ld, f.relu, rows, c,
                                       _lib.HF_F32, st()), "hf_bn_forward_train")
    return y, y2, mean, rstd, rm, rv


def _check_fwd(k, outs):
    y, y2, mean, rstd, rm, rv = outs
    ref, R, f, o = k.ref, k.R, k.f, k.o
    note = (k.rows, k.c, k.nparts, vars(f))
    My = L.mixed(ref.My, R.y[0], ref.My64, R.y[1])
    if y is not None:
        within(L.ratio(y.val, ref.y, My, 1), 1.0, strict=False, note=note)
    if y2 is not None:
        within(L.ratio(y2.val, ref.y, My, 1), 1.0, strict=False, note=note)
    if y is not None and y2 is not None:
        assert torch.equal(_bits(y.val), _bits(y2.val))
    # the constant channel: the variance clamps to 0, a - mean is exactly 0 and y exactly b + res
    exact = f32(k.b[0].item() if f.b else 0.0) + (k.res[:, 0].numpy() if k.res is not None else np.zeros(k.rows, f32))
    exact = np.maximum(exact, f32(0)) if f.relu else exact
    for out in (y, y2):
        assert out is None or np.array_equal(out.val[:, 0].cpu().numpy(), exact), "constant channel: y != b + res"
    assert float(mean.val[0, 0]) == L.CONST_VALUE
    within(L.ratio(mean.val[0], ref.mean, L.mixed(ref.Mmean, R.mean[0], ref.Mmean, R.mean[1]), 1), 1.0, strict=False,
           note=note)
    within(L.ratio(rstd.val[0], ref.rstd, L.mixed(ref.Mrstd, R.rstd[0], ref.Mrstd64, R.rstd[1]), 1), 1.0, strict=False,
           note=note)
    if f.stat == "move":
        within(L.ratio(rm.val[0], ref.rm, L.mixed(ref.Mrm, R.rm[0], ref.Mrm, R.rm[1]), 1), 1.0, strict=False, note=note)
        within(L.ratio(rv.val[0], ref.rv, L.mixed(ref.Mrv, R.rv[0], ref.Mrv64, R.rv[1]), 1), 1.0, strict=False, note=note)
    else:  # momentum < 0, or no running pointers: nothing is moved
        assert torch.equal(_bits(rm.val[0].cpu()), _bits(o.rm)) and torch.equal(_bits(rv.val[0].cpu()), _bits(o.rv))


@pytest.mark.parametrize("rows,c,nparts,i", L.fwd_cases(), ids=_ids)
def test_bn_forward_train_against_longdouble(rows, c, nparts, i):
    """Fed the REFERENCE's partial rows (rounded once to fp64): y / y2, mean, rstd, running mean and running variance
    each within its own bound per channel (``r_bn_forward_train``), the guards behind every [c] vector intact (mean,
    rstd and the running statistics are written once, not once per workgroup's tail), nothing moved with momentum < 0
    or NULL running pointers."""
    k = _fwd_problem(rows, c, nparts, i)
    lib = _lib.load()
    _check_fwd(k, twice(lambda: _fwd_launch(lib, k)))


def test_bn_stats_rows_feeds_bn_forward_train():
    """The chained pair: the statistics kernel's OWN partial rows (9 slabs, 7 row shares) into the normalising launch;
    the reference takes those rows as given."""
    rows, c, splits, rb = 200, 96, 9, 7
    a = L.stats_inputs(rows, c, splits)
    lib = _lib.load()
    a_dev, stride = _slab_buffer(a, 0, 0)
    part, a_out = _stats_launch(lib, a_dev, stride, splits, rows, c, rb, True)
    assert torch.equal(_bits(a_out.val.cpu()), _bits(L.f32_slab_sum(a)))
    k = _fwd_problem(rows, c, rb, 0, part=part.val.cpu().view(rb, 2, c).clone())
    k.o.s = a_out.val.cpu().clone()
    k.ref = L.bn_forward_train(k.o.s, k.o.part, float(rows), L.BN_EPS, k.mom, k.o.w, k.b, k.res, k.f.relu, k.o.rm, k.o.rv)
    k.dev.s, k.dev.part = a_out.val.contiguous(), part.val.contiguous()
    assert k.f.stat == "move"
    _check_fwd(k, twice(lambda: _fwd_launch(lib, k)))


# ---------------------------------------------------------------------------------------------------------------
# hf_linear_ce_head
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,features,classes,bias", L.LIN_HEAD_CASES, ids=_ids)
def test_linear_ce_head_against_float64(rows, features, classes, bias):
    """g_feat, every single g_w / g_b slab (rows past the end of the last workgroup contribute exact zeros) and the
    slabs' sums, each within its bound (``r_linear_ce_head``).  Cases without a bias pass v_b = g_b = NULL: the
    bias-gradient buffer stays untouched.  One class: every output exactly zero."""
    o = L.linear_head_inputs(rows, features, classes, bias)
    ref = L.linear_ce_head(o.t_feat, o.feat, o.w, o.v_w, o.v_b, o.p, o.scale)
    R = L.r_linear_ce_head(features, classes, bias)
    lib = _lib.load()
    groups = lib.hf_linear_ce_head_slabs(rows)
    assert groups == ref.g_w.shape[0]
    d = [dv(t) for t in (o.t_feat, o.feat, o.w, o.v_w, o.v_b, o.p)]

    def launch():
        gf, gw, gb = RowOut(rows, features), RowOut(groups * classes, features), RowOut(groups, classes)
        _lib.check(lib.hf_linear_ce_head(gf.ptr, gw.ptr, gb.ptr if bias else None, *(p(t) for t in d), o.scale, rows,
                                         features, classes, _lib.HF_F32, st()), "hf_linear_ce_head")
        return gf, gw, gb

    gf, gw, gb = twice(launch)
    note = (rows, features, classes, bias)
    within(L.ratio(gf.val, ref.g_feat, ref.Mg_feat, R.g_feat), 1.0, strict=False, note=note)
    slabs = gw.val.view(groups, classes, features)
    within(L.ratio(slabs, ref.g_w, ref.Mg_w, R.g_w), 1.0, strict=False, note=note)
    within(L.ratio(slabs[-1], ref.g_w[-1], ref.Mg_w[-1], R.g_w), 1.0, strict=False, note=note)  # (the partial workgroup)
    within(L.ratio(slabs.double().sum(0), ref.g_w.sum(0), ref.Mg_w.sum(0), R.g_w), 1.0, strict=False, note=note)
    if bias:
        within(L.ratio(gb.val, ref.g_b, ref.Mg_b, R.g_b), 1.0, strict=False, note=note)
        within(L.ratio(gb.val[-1], ref.g_b[-1], ref.Mg_b[-1], R.g_b), 1.0, strict=False, note=note)
        within(L.ratio(gb.val.double().sum(0), ref.g_b.sum(0), ref.Mg_b.sum(0), R.g_b), 1.0, strict=False, note=note)
    else:
        assert bool(torch.isnan(gb.buf).all()), "g_b == NULL, and the bias-gradient buffer was written"
    if classes == 1:
        for out in (gf, gw) + ((gb,) if bias else ()):
            assert bool((out.val == 0).all()), "one class: the Hessian is zero"


# ---------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched, the documented status comes back
# ---------------------------------------------------------------------------------------------------------------
def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, device=DEV, dtype=dtype)


def _off(t):
    """4 bytes (8 for doubles) into the allocation: no 16-byte alignment"""
    return _lib.c_void_p(t.data_ptr() + t.element_size())


def test_statistics_entries_refuse_what_they_do_not_cover():
    lib = _lib.load()
    rows, c, rb = 8, 12, 2
    big = 2 * 16 * 1032  # (room for any c named below, should a launch happen after all)
    a, w = torch.zeros(2 * big, device=DEV), torch.zeros(2 * big, device=DEV)
    a_out, y, y2, mean, rstd = (_nan(2 * big) for _ in range(5))
    part = _nan(2 * big, torch.float64)
    ok_part = torch.zeros(2 * big, device=DEV, dtype=torch.float64)

    def stats(a_out_=None, a_=None, splits=2, stride=rows * c, rows_=rows, c_=c, rb_=rb):
        return lib.hf_bn_stats_rows(a_out_ if a_out_ is not None else p(a_out), a_ if a_ is not None else p(a), splits,
                                    stride, p(part), rows_, c_, rb_, _lib.HF_F32, st())

    assert stats(c_=6) == ERR_ARG and stats(c_=1028) == ERR_ARG          # c % 4, c > 1024
    assert stats(rb_=0) == ERR_ARG and stats(rb_=-1) == ERR_ARG
    assert stats(splits=0) == ERR_ARG and stats(stride=0) == ERR_ARG and stats(rows_=0) == ERR_ARG
    assert stats(stride=rows * c + 2) == ERR_ALIGN                       # slab_stride & 3
    assert stats(a_=_off(a)) == ERR_ALIGN and stats(a_out_=_off(a_out)) == ERR_ALIGN

    def fwd(**kw):
        q = dict(y=p(y), y2=p(y2), y2_ld=2 * c, a=p(a), part=p(ok_part), nparts=rb, count=float(rows), w=p(w), b=p(w),
                 res=p(a), res_ld=2 * c, c=c)
        q.update(kw)
        return lib.hf_bn_forward_train(q["y"], q["y2"], q["y2_ld"], q["a"], q["part"], q["nparts"], p(mean), p(rstd),
                                       None, None, q["count"], 1e-5, 0.1, q["w"], q["b"], q["res"], q["res_ld"], 1, rows,
                                       q["c"], _lib.HF_F32, st())

    assert fwd(c=6, y2_ld=12, res_ld=12) == ERR_ARG and fwd(c=1028, y2_ld=2056, res_ld=2056) == ERR_ARG
    assert fwd(nparts=0) == ERR_ARG and fwd(count=0.0) == ERR_ARG and fwd(count=-1.0) == ERR_ARG
    assert fwd(y2_ld=c - 4) == ERR_ARG and fwd(y2_ld=c + 2) == ERR_ARG
    assert fwd(res_ld=c - 4) == ERR_ARG and fwd(res_ld=c + 2) == ERR_ARG
    assert fwd(y=None, y2=None) == ERR_ARG
    for name, t in (("y", y), ("y2", y2), ("a", a), ("part", ok_part), ("w", w), ("b", w), ("res", a)):
        assert fwd(**{name: _off(t)}) == ERR_ALIGN, name
    torch.cuda.synchronize()
    for t in (a_out, y, y2, mean, rstd, part):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    assert fwd() == 0 and stats() == 0                                    # (the unmodified calls are accepted)
    torch.cuda.synchronize()


HEAD_REFUSED = [(0, 4, 1), (4097, 4, 1), (1, 4, 65), (1, 2, 1), (1, 6, 1), (1, 516, 1), (1, 124, 64), (1, 512, 14)]


def test_linear_ce_head_refuses_what_it_does_not_cover():
    """rows 0 / 4097, 65 classes, features 2 / 6 / 516, (64, 124) and (14, 512) over the LDS limit, and each operand
    the kernel reads or writes in quads 4 bytes off the 16-byte grid: -1, nothing launched."""
    lib = _lib.load()
    z = torch.zeros(1 << 16, device=DEV)
    gf, gw, gb = _nan(1 << 16), _nan(1 << 16), _nan(1 << 16)

    def head(rows=4, features=8, classes=5, **kw):
        q = dict(gf=p(gf), gw=p(gw), t=p(z), f=p(z), w=p(z), vw=p(z))
        q.update(kw)
        return lib.hf_linear_ce_head(q["gf"], q["gw"], p(gb), q["t"], q["f"], q["w"], q["vw"], p(z), p(z), 1.0, rows,
                                     features, classes, _lib.HF_F32, st())

    for rows, features, classes in HEAD_REFUSED:
        assert not L.head_shape_ok_ref(rows, features, classes)
        assert head(rows, features, classes) == -1, (rows, features, classes)
    for name, t in (("gf", gf), ("gw", gw), ("t", z), ("f", z), ("w", z), ("vw", z)):
        assert head(**{name: _off(t)}) == -1, name
    torch.cuda.synchronize()
    for t in (gf, gw, gb):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    assert head() == 0
    torch.cuda.synchronize()


def test_host_predicate_of_the_fused_head_agrees_with_the_library():
    """``engine.tangent.head_fused_shape_ok`` (what ``_head_fused`` asks before it takes the fused path) says yes
    exactly where ``hf_linear_ce_head`` returns 0 on properly sized, aligned buffers: the boundary points of every
    limit (classes, features, rows, LDS)."""
    lib = _lib.load()
    for classes in (1, 13, 14, 64, 65):
        for features in (2, 4, 120, 124, 512, 516):
            for rows in (1, 4096, 4097):
                groups = -(-rows // 4)
                gf, gw, gb = (torch.empty(n, device=DEV) for n in (rows * features, groups * classes * features,
                                                                   groups * classes))
                t, w, pm = (torch.zeros(n, device=DEV) for n in (rows * features, classes * features, rows * classes))
                rc = lib.hf_linear_ce_head(p(gf), p(gw), p(gb), p(t), p(t), p(w), p(w), None, p(pm), 1.0, rows, features,
                                           classes, _lib.HF_F32, st())
                assert rc in (0, -1), (rc, rows, features, classes)
                assert (rc == 0) == head_fused_shape_ok(rows, features, classes), (rows, features, classes, rc)
                assert head_fused_shape_ok(rows, features, classes) == L.head_shape_ok_ref(rows, features, classes)
    torch.cuda.synchronize()
