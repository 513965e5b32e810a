"""The machinery of the exact convolution-kernel tests (``test_conv_kernels_gpu.py``, ``test_conv_loop_gpu.py``): device
operands and float64 references per problem, the planner's answers, the checked slab output, launch-check-launch-again
on the same buffers, and the four test bodies that both files run on their own case tables."""

import ctypes

import numpy as np
import torch

import conv_refs as cr
from guarded import DEV, GUARD, NAN, SlabOut, P as PTR, dev as _dev, st as _st
from pytorchhessianfree_amd import _lib


def _bits(t):
    return t.view(torch.int32)


_OPS, _REFS, _INFO = {}, {}, {}


def _ops(p):
    """Device operands of problem ``p`` (computed once per problem; never written)."""
    if p not in _OPS:
        host = cr.operands(p)
        _OPS[p] = (host, {name: _dev(host[name]) for name in ("act", "mat")})
    return _OPS[p]


def _ref(p):
    """Float64 reference of problem ``p`` on the device, flattened (computed once per geometry and direction)."""
    key = p[:10]
    if key not in _REFS:
        ref = cr.reference(p, _ops(p)[0], DEV).reshape(-1)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < cr.EXACT_LIMIT and cr.exact(p)
        _REFS[key] = ref
    return _REFS[key]


def _info(p, scratch=None):
    key = (p, scratch)
    if key not in _INFO:
        kw = dict(splits=p.splits, act_ld=p.act_ld, mat_ld=p.mat_ld)
        if scratch:
            kw.update(tickets=scratch[:2], target_blocks=scratch[2])
        _INFO[key] = _lib.conv_plan_info(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad, **kw)
    return _INFO[key]


class Out(SlabOut):
    """The slabs of problem ``p``'s output."""

    def __init__(self, p, splits):
        super().__init__(int(np.prod(cr.out_shape(p))), splits)
        self.p = p

    def check(self, what):
        """Guards, gaps, complete slabs, dead taps, exact sum."""
        p = self.p
        assert bool(torch.isnan(self.buf[~self.inside]).all()), "%s: a guard or a gap between slabs was written" % what
        slabs = self.slabs()
        unwritten = torch.isnan(slabs)
        if p.d == 2:
            dead = torch.from_numpy(cr.dead_mask(p).reshape(-1)).to(DEV)
            assert bool((unwritten == dead.expand_as(unwritten)).all()), \
                "%s: the unwritten entries are not exactly those of the dead taps" % what
            assert not bool(_ref(p)[dead].any())
        else:
            assert not bool(unwritten.any()), "%s: %d entries of the slabs were not written" % (what, int(unwritten.sum()))
        got = torch.nan_to_num(slabs, nan=0.0).double().sum(0)
        want = _ref(p)
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).reshape(-1)
            i = int(bad[0])
            raise AssertionError("%s: %d of %d elements differ from the float64 reference, first at %s: %r != %r" % (
                what, bad.numel(), got.numel(), np.unravel_index(i, cr.out_shape(p)), float(got[i]), float(want[i])))



def _geo(p):
    return [p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride[0], p.stride[1], p.pad[0], p.pad[1]]


def _fill(q, p, out, splits):
    ops = _ops(p)[1]
    q.direction, q.out, q.act, q.mat = p.d, out.ptr, ops["act"].data_ptr(), ops["mat"].data_ptr()
    (q.n, q.h, q.w, q.c, q.k, q.r, q.s, q.stride_h, q.stride_w, q.pad_h, q.pad_w) = _geo(p)
    q.act_ld, q.mat_ld, q.out_c, q.splits, q.slab_stride = p.act_ld, p.mat_ld, 0, splits, out.stride


def _launch_slabs(p, out):
    ops = _ops(p)[1]
    _lib.check(_lib.load().hf_conv2d_nhwc_slabs(
        p.d, PTR(out.ptr), PTR(ops["act"].data_ptr()), PTR(ops["mat"].data_ptr()), *_geo(p), p.act_ld, p.mat_ld, 0,
        out.splits, out.stride, _lib.HF_F32, _st()), "hf_conv2d_nhwc_slabs")


def _twice(launch, outs, what, scratch=()):
    """Launch, check everything, launch again on the same buffers: the same bits."""
    launch()
    torch.cuda.synchronize()
    for o in outs:
        o.check(what)
    for sc in scratch:
        sc.check(what)
    first = [o.buf.clone() for o in outs]
    launch()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(_bits(o.buf), _bits(f)), "%s: a second launch on the same buffers gives other bits" % what
    for sc in scratch:
        sc.check(what + " (second launch)")
    return first


_SINGLE = {}


def _single(p):
    """The slab-mode single launch of problem ``p``, checked; returns the bits of its whole guarded buffer (once per
    problem: the merged forms compare with it)."""
    if p not in _SINGLE:
        out = Out(p, _info(p)["splits"])
        (bits,) = _twice(lambda: _launch_slabs(p, out), [out], "hf_conv2d_nhwc_slabs %r" % (p,))
        _SINGLE[p] = bits
    return _SINGLE[p]


def _expect_plan(case):
    """The planner answers on this machine what the table says (the CPU test's assertion, repeated where the kernels run:
    a case that drifted to another instantiation must not pass as a test of the one it names)."""
    for idx, (p, want) in enumerate(zip(case.problems, case.expect)):
        got = _info(p, cr.scratch_of(case, idx) if case.tickets else None)
        have = cr.Expect(got["config"], got["scalar"], got["cls_taps"], got["live_taps"], got["splits"],
                         -(-got["steps"] // got["splits"]))
        assert have == want, (case.name, p, have, want)


def slab_launch_equals_float64_exactly(case):
    _expect_plan(case)
    _single(case.problems[0])


def slab_pair_equals_the_single_launches_and_float64(case):
    """``hf_conv2d_nhwc_backward_slabs`` / ``hf_conv2d_nhwc_dw_slabs`` (``k_conv_dw``)."""
    _expect_plan(case)
    d, w = case.problems
    outs = [Out(p, _info(p)["splits"]) for p in case.problems]
    od, ow = _ops(d)[1], _ops(w)[1]
    assert torch.equal(od["act"], ow["mat"].view_as(od["act"]))  # one dY
    lib = _lib.load()
    if case.form == "backward_slabs":
        def launch():
            _lib.check(lib.hf_conv2d_nhwc_backward_slabs(
                PTR(outs[0].ptr), PTR(outs[1].ptr), PTR(od["act"].data_ptr()), PTR(ow["act"].data_ptr()),
                PTR(od["mat"].data_ptr()), *_geo(d), outs[0].splits, outs[0].stride, outs[1].splits, outs[1].stride,
                _lib.HF_F32, _st()), "hf_conv2d_nhwc_backward_slabs")
    else:
        arr = (_lib.ConvProblem * 2)()
        for q, p, o in zip(arr, case.problems, outs):
            _fill(q, p, o, o.splits)

        def launch():
            _lib.check(lib.hf_conv2d_nhwc_dw_slabs(ctypes.byref(arr[0]), ctypes.byref(arr[1]), _lib.HF_F32, _st()),
                       "hf_conv2d_nhwc_dw_slabs")

    merged = _twice(launch, outs, case.name)
    for p, m in zip(case.problems, merged):
        assert torch.equal(_bits(m), _bits(_single(p))), (case.name, p)


def grouped_launch_equals_the_single_launches_and_float64(case):
    """``hf_conv2d_nhwc_group_slabs`` (``k_conv_group``): 1 to 4 problems of any direction in one launch."""
    _expect_plan(case)
    outs = [Out(p, _info(p)["splits"]) for p in case.problems]
    arr = (_lib.ConvProblem * len(outs))()
    for q, p, o in zip(arr, case.problems, outs):
        _fill(q, p, o, o.splits)

    def launch():
        _lib.check(_lib.load().hf_conv2d_nhwc_group_slabs(ctypes.cast(arr, PTR), len(outs), _lib.HF_F32, _st()),
                   "hf_conv2d_nhwc_group_slabs")

    merged = _twice(launch, outs, case.name)
    for p, m in zip(case.problems, merged):
        assert torch.equal(_bits(m), _bits(_single(p))), (case.name, p)


class Parts:
    """The two partial-sum arrays [rows, k] of one BNSUM problem, each between guards, NaN."""

    def __init__(self, rows, k):
        self.rows, self.k = rows, k
        self.buf = torch.full((2, 2 * GUARD + rows * k), NAN, device=DEV)
        self.ptr = [self.buf[i].data_ptr() + 4 * GUARD for i in range(2)]

    def get(self, i):
        return self.buf[i, GUARD:GUARD + self.rows * self.k].view(self.rows, self.k)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:, :GUARD]).all()) and bool(torch.isnan(self.buf[:, GUARD + self.rows * self.k:]).all())


def bnsum_launch_equals_the_single_launches_and_exact_partial_sums(case):
    """``hf_conv2d_nhwc_group_slabs_bnsum``: the slabs are bitwise those of the plain launch; row ``tile * splits + split``
    of the partial sums is EXACTLY the float64 column sum of that split's slab over the 64 rows of the tile (sum t and
    sum t * xhat), the rows of a tile summed over its splits those of the reference; every row is written, ragged last
    tiles and column tiles included; a problem without sums gets none."""
    _expect_plan(case)
    for p, s in zip(case.problems, case.sums):
        assert not s or cr.bn_exact(p)
    outs = [Out(p, _info(p)["splits"]) for p in case.problems]
    n = len(outs)
    arr, bn = (_lib.ConvProblem * n)(), (_lib.ConvBnSum * n)()
    keep, parts, bns = [], [], []
    for q, b, p, o, with_sums in zip(arr, bn, case.problems, outs, case.sums):
        _fill(q, p, o, o.splits)
        parts.append(None)
        bns.append(None)
        if with_sums:
            info = _info(p)
            host = cr.bn_operands(p)
            dev = {name: _dev(host[name]) for name in ("x", "mean", "rstd")}
            pt = Parts(info["tiles_m"] * info["splits"], p.k)
            keep.append(dev)
            parts[-1], bns[-1] = pt, host
            b.x, b.mean, b.rstd = (dev[name].data_ptr() for name in ("x", "mean", "rstd"))
            b.part_1, b.part_x, b.part_rows = pt.ptr[0], pt.ptr[1], pt.rows

    def launch():
        rc = _lib.load().hf_conv2d_nhwc_group_slabs_bnsum(ctypes.cast(arr, PTR), n, ctypes.cast(bn, PTR), _lib.HF_F32,
                                                          _st())
        _lib.check(rc, "hf_conv2d_nhwc_group_slabs_bnsum")

    merged = _twice(launch, outs, case.name)
    first_parts = [pt.buf.clone() if pt else None for pt in parts]
    for p, m, o, pt, host in zip(case.problems, merged, outs, parts, bns):
        assert torch.equal(_bits(m), _bits(_single(p))), (case.name, p)
        if pt is None:
            continue
        assert pt.guards_intact()
        splits, tiles = o.splits, pt.rows // o.splits
        slabs = o.slabs().double().cpu().numpy().reshape(splits, -1, p.k)
        total = [0.0, 0.0]
        for sp in range(splits):
            want = cr.bn_partial_ref(slabs[sp], host)
            for kind in (0, 1):
                got = pt.get(kind).view(tiles, splits, p.k)[:, sp].double().cpu().numpy()
                assert np.array_equal(got, want[kind]), (case.name, p, "split", sp, "sum t" if kind == 0 else "sum t*xhat")
                total[kind] = total[kind] + got
        want = cr.bn_partial_ref(_ref(p).cpu().numpy().reshape(-1, p.k), host)
        assert np.array_equal(total[0], want[0]) and np.array_equal(total[1], want[1])
    launch()
    torch.cuda.synchronize()
    for pt, f in zip(parts, first_parts):
        assert pt is None or torch.equal(_bits(pt.buf), _bits(f))
