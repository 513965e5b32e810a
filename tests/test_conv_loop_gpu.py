"""GPU: the K loops of the 64 x 64 convolution kernels (``hf_conv.hip``: the software-pipelined ``pipelined_share`` of the
weight-gradient body, the three-deep ring of the forward / data-gradient body) on the cases of ``conv_loop_refs.py`` --
shares of 5 to 12 steps (odd and even, several ring rounds), shorter last shares, ragged channel steps and rows,
dead taps, residue classes, merged launches with mixed share lengths, the BNSUM epilogue and the launch that carries
the weight scatter -- against the float64 reference, EXACTLY, with the machinery of ``conv_harness.py``: integer
operands in [-3, 3] (every partial sum exact), every output between NaN guards, NaN gaps between the slabs, every slab
completely written, a second launch bitwise equal, merged launches bitwise equal to the single launches of their
problems.  ``test_conv_loop_refs_cpu.py`` asserts that the planner gives every case the share length it is named for;
each test repeats that where the kernels run.

Repeatability on N(0, 1) operands (no reference: the order of the additions is fixed, so two launches give the same
bits) at three geometries of the ResNet-18 product scaled to batch 2."""

import numpy as np
import pytest
import torch

import conv_harness as ch
import conv_loop_refs as lr
import conv_refs as cr
from guarded import DEV
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
_BY_FORM = {form: [c for c in lr.CASES if c.form == form] for form in {c.form for c in lr.CASES}}


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", _BY_FORM["slabs"], ids=_ids(_BY_FORM["slabs"]))
def test_loop_slab_launch_equals_float64_exactly(case):
    ch.slab_launch_equals_float64_exactly(case)


@pytest.mark.parametrize("case", _BY_FORM["dw_slabs"], ids=_ids(_BY_FORM["dw_slabs"]))
def test_loop_pair_equals_the_single_launches_and_float64(case):
    ch.slab_pair_equals_the_single_launches_and_float64(case)


@pytest.mark.parametrize("case", _BY_FORM["group_slabs"], ids=_ids(_BY_FORM["group_slabs"]))
def test_loop_group_equals_the_single_launches_and_float64(case):
    ch.grouped_launch_equals_the_single_launches_and_float64(case)


@pytest.mark.parametrize("case", _BY_FORM["group_slabs_bnsum"], ids=_ids(_BY_FORM["group_slabs_bnsum"]))
def test_loop_bnsum_equals_the_single_launches_and_exact_partial_sums(case):
    ch.bnsum_launch_equals_the_single_launches_and_exact_partial_sums(case)


def test_loop_launch_carrying_the_weight_scatter_equals_float64_and_the_two_launches():
    """``hf_conv2d_nhwc_slabs_unpack``: the convolution's weight operand is a slice of the flat vector, the launch carries
    the scatter of two other tensors.  The slabs: guards and gaps untouched, completely written, their sum the float64
    reference, bitwise those of the plain slab launch; the scattered tensors bitwise those of ``hf_unpack_weights``."""
    p, want = lr.UNPACK
    case = cr.Case("loop_unpack", "slabs", (p,), (want,), None, None)
    ch._expect_plan(case)
    single = ch._single(p)
    host = cr.operands(p)
    rng = np.random.RandomState(7)
    k2, c2 = 24, 16
    tail = rng.randint(-cr.VMAX, cr.VMAX + 1, size=5 + k2 * c2 * 9 + k2 * c2).astype(np.float32)
    v = ch._dev(np.concatenate([host["mat"].reshape(-1), tail]))
    n_w = host["mat"].size
    vw = v[:n_w]
    off3, off1 = n_w + 5, n_w + 5 + k2 * c2 * 9

    def buffers():
        b3 = torch.full((k2, 2 * c2, 3, 3), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
        b1 = torch.full((k2, 2 * c2, 1, 1), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
        return [(off3, b3, c2, 0b000111010), (off1, b1, c2, 0)]

    slots_a = buffers()
    _lib.unpack_tangent(v, slots_a)
    slots_b = buffers()
    out = ch.Out(p, want.splits)
    act = ch._ops(p)[1]["act"]

    def launch():
        rc = _lib.load().hf_conv2d_nhwc_slabs_unpack(
            ch.PTR(out.ptr), ch.PTR(act.data_ptr()), ch.PTR(vw.data_ptr()), *ch._geo(p), 0, 0, out.splits, out.stride,
            ch.PTR(v.data_ptr()), *_lib.unpack_table(v, slots_b), _lib.HF_F32, ch._st())
        _lib.check(rc, "hf_conv2d_nhwc_slabs_unpack")

    (bits,) = ch._twice(launch, [out], "hf_conv2d_nhwc_slabs_unpack %r" % (p,))
    assert torch.equal(ch._bits(bits), ch._bits(single))
    for (_, ba, _, _), (_, bb, _, _) in zip(slots_a, slots_b):
        assert torch.equal(ba, bb)
    assert not torch.equal(slots_b[0][1], torch.full_like(slots_b[0][1], 7.0))  # (the scatter really ran)


@pytest.mark.parametrize("p", lr.PRODUCT_GEOMETRIES, ids=lambda p: "d%d_%dx%d_c%d_k%d" % (p.d, p.h, p.w, p.c, p.k))
def test_two_launches_on_normal_operands_give_the_same_bits(p):
    gen = torch.Generator(device=DEV).manual_seed(19)
    oh, ow = cr.out_hw(p)
    cs = (p.c, p.k, p.c)[p.d]
    act_shape = (p.n, oh, ow, cs) if p.d == 1 else (p.n, p.h, p.w, cs)
    mat_shape = ((p.k, p.r, p.s, p.c), (p.c, p.r, p.s, p.k), (p.n, oh, ow, p.k))[p.d]
    act = torch.randn(act_shape, device=DEV, generator=gen)
    mat = torch.randn(mat_shape, device=DEV, generator=gen)
    splits = ch._info(p)["splits"]
    out = ch.Out(p, splits)

    def launch():
        _lib.check(_lib.load().hf_conv2d_nhwc_slabs(
            p.d, ch.PTR(out.ptr), ch.PTR(act.data_ptr()), ch.PTR(mat.data_ptr()), *ch._geo(p), 0, 0, 0, splits,
            out.stride, _lib.HF_F32, ch._st()), "hf_conv2d_nhwc_slabs")

    launch()
    torch.cuda.synchronize()
    first = out.buf.clone()
    assert bool(torch.isnan(first[~out.inside]).all())
    assert bool(torch.isfinite(out.slabs()).all()) and float(out.slabs().abs().max()) > 0  # (3 x 3 on >= 2 x 2: no dead taps)
    launch()
    torch.cuda.synchronize()
    assert torch.equal(ch._bits(out.buf), ch._bits(first))
