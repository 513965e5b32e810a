"""Exact references of the squared-sum kernels behind the batched diagonal empirical Fisher
(``hf_conv2d_nhwc_sqsum_slabs`` in ``hf_conv.hip``, ``hf_chan_sqsum`` in ``hf_bn.hip``) and the table of their cases.
Shared by ``test_diag_sq_refs_cpu.py`` (references against per-sample autograd, table against the host planner) and
``test_diag_sq_kernels_gpu.py`` (kernels against the references).  Plain module: numpy and torch on the CPU.

Nothing here has a tolerance.  The operands are integers in [-3, 3] and ``pre`` is a power of two.  A per-sample weight
gradient entry is a sum of ``P = oh * ow`` products of magnitude <= 9: an integer below ``9 P``; its square is below
``81 P^2`` and the sum over ``n`` samples below ``81 P^2 n``.  While that is below 2**24 every intermediate of any
split, in any order, is exactly representable in fp32 (scaling by a power of two changes no mantissa), so the fp32
result IS the float64 reference (``conv_exact``: a condition on the inputs, not a bound on an error).  The squared-operand
form (``P == 1``) sums products of two squares <= 9: below ``81 n``, the same condition.  The channel sums multiply by
``xhat = (x - mean) * rstd`` with integer ``x``, ``mean`` in [-2, 2] and ``rstd`` from {0.5, 1, 2}: a multiple of 0.5 of
magnitude <= 10, so a sample's sum is a multiple of 0.5 below ``30 hw``, its square a multiple of 0.25 below
``(30 hw)^2``, and the sum over the samples exact while ``(60 hw)^2 n < 2**24`` (``chan_exact``)."""

import zlib
from collections import namedtuple

import numpy as np
import torch

NAN = float("nan")
VMAX = 3
EXACT_LIMIT = 2 ** 24
PRE = 2.0            # the factor the exact tests run with; 0.5 * PRE must scale the result by exactly 0.25

# act_ld / out_c: 0 = c
ConvCase = namedtuple("ConvCase", "name n h w c k r s stride pad act_ld out_c")
ChanCase = namedtuple("ChanCase", "name n hw c")


def C(name, n, h, w, c, k, r, s, stride=1, pad=0, act_ld=0, out_c=0):
    return ConvCase(name, n, h, w, c, k, r, s, (stride, stride), (pad, pad), act_ld, out_c)


CONV_CASES = [
    C("p64_sample_ends_on_step_ends", 3, 8, 8, 8, 8, 3, 3, 1, 1),
    C("p25_sample_ends_inside_a_step", 5, 5, 5, 12, 20, 3, 3, 1, 1),
    C("p16_stride_2", 4, 7, 7, 4, 36, 3, 3, 2, 1),
    C("p4", 6, 2, 2, 8, 8, 3, 3, 1, 1),
    C("p256_several_steps_per_sample", 2, 16, 16, 4, 8, 3, 3, 1, 1),
    C("two_row_tiles", 8, 4, 4, 64, 128, 1, 1, 1, 0),
    C("p1_one_live_tap_of_nine", 37, 1, 1, 16, 24, 3, 3, 1, 1),
    C("p1_1x1", 9, 1, 1, 8, 8, 1, 1, 1, 0),
    C("scalar_gathers", 4, 8, 8, 3, 8, 3, 3, 1, 1),
    C("stem_form_padded_columns", 4, 5, 5, 12, 8, 1, 1, 1, 0, act_ld=12, out_c=9),
]
CHAN_CASES = [
    ChanCase("hw25_c20", 5, 25, 20),
    ChanCase("hw16_two_channel_blocks", 3, 16, 70),
    ChanCase("hw1", 6, 1, 8),
    ChanCase("hw9_c3", 4, 9, 3),
]
# (n, splits) a launch must refuse: no split, more splits than samples, a split left without a sample
REFUSED_SPLITS = [(5, 0), (5, 6), (5, 4), (37, 36), (8, 7)]
# geometries hf_conv2d_nhwc_sqsum_plan must refuse: (n, h, w, c, k, r, s, stride, pad)
REFUSED_GEOMETRIES = [(0, 4, 4, 8, 8, 3, 3, 1, 1), (2, 4, 4, 8, 8, 9, 9, 1, 4), (2, 2, 2, 8, 8, 3, 3, 1, 0),
                      (2, 4, 4, 0, 8, 3, 3, 1, 1), (2, 4, 4, 8, 8, 3, 3, 0, 1)]


def shares_ok(n, splits):
    """The library's rule: split s takes samples [s * ceil(n / splits), ...), and none of them is empty."""
    return 1 <= splits <= n and -(-n // splits) * (splits - 1) < n


def forced_splits(n):
    """The split counts every case runs with besides the planned one."""
    return sorted({1, 2, n} & set(range(1, n + 1)))


def out_hw(p):
    return (p.h + 2 * p.pad[0] - p.r) // p.stride[0] + 1, (p.w + 2 * p.pad[1] - p.s) // p.stride[1] + 1


def out_c(p):
    return p.out_c or p.c


def conv_exact(p):
    oh, ow = out_hw(p)
    return (VMAX * VMAX * oh * ow) ** 2 * p.n < EXACT_LIMIT


def chan_exact(p):
    return (2 * VMAX * 10 * p.hw) ** 2 * p.n < EXACT_LIMIT


def live_taps(p):
    oh, ow = out_hw(p)
    rows = [r for r in range(p.r) if any(0 <= y * p.stride[0] - p.pad[0] + r < p.h for y in range(oh))]
    cols = [q for q in range(p.s) if any(0 <= x * p.stride[1] - p.pad[1] + q < p.w for x in range(ow))]
    return [(r, q) for r in rows for q in cols]


def dead_mask(p):
    """Boolean [k, r, s, out_c]: True at the entries of taps that never meet data (not written by the kernel)."""
    m = np.ones((p.k, p.r, p.s, out_c(p)), bool)
    for r, q in live_taps(p):
        m[:, r, q, :] = False
    return m


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _ints(rng, shape, lo=-VMAX, hi=VMAX):
    return rng.randint(lo, hi + 1, size=shape).astype(np.float32)


def conv_operands(p):
    """``x`` [n, h, w, act_ld or c] and ``gy`` [n, oh, ow, k], float32 integers in [-3, 3].  The channels of ``x`` from
    ``out_c`` on (the stem's padding columns) and those beyond ``c`` hold integers too: no output column reads them."""
    rng = np.random.RandomState(_seed("sqconv", *p[1:]))
    oh, ow = out_hw(p)
    return dict(x=_ints(rng, (p.n, p.h, p.w, p.act_ld or p.c)), gy=_ints(rng, (p.n, oh, ow, p.k)))


def per_sample_wgrad(p, ops):
    """Float64 per-sample weight gradients [n, k, r, s, c] by the im2col product."""
    x = torch.from_numpy(ops["x"][..., :p.c]).double().permute(0, 3, 1, 2)
    gy = torch.from_numpy(ops["gy"]).double().reshape(p.n, -1, p.k)
    cols = torch.nn.functional.unfold(x, (p.r, p.s), padding=p.pad, stride=p.stride)    # [n, c*r*s, P]
    dw = torch.einsum("npk,njp->nkj", gy, cols).reshape(p.n, p.k, p.c, p.r, p.s)
    return dw.permute(0, 1, 3, 4, 2).contiguous()


def conv_reference(p, ops, pre=PRE):
    """Float64 ``sum_i (pre * dW_i)^2`` in the kernel's layout [k, r, s, out_c]."""
    dw = per_sample_wgrad(p, ops)[..., :out_c(p)]
    return ((pre * dw) ** 2).sum(0)


def chan_operands(p):
    rng = np.random.RandomState(_seed("sqchan", *p[1:]))
    return dict(g=_ints(rng, (p.n, p.hw, p.c)), x=_ints(rng, (p.n, p.hw, p.c)), mean=_ints(rng, (p.c,), -2, 2),
                rstd=np.asarray([0.5, 1.0, 2.0], np.float32)[rng.randint(0, 3, size=p.c)])


def chan_reference(p, ops, pre=PRE, with_x=True):
    """Float64 ``(gw2, gb2)`` [c] each (``gw2`` None without ``x``)."""
    g = ops["g"].astype(np.float64)
    gb2 = ((pre * g.sum(1)) ** 2).sum(0)
    if not with_x:
        return None, gb2
    xhat = (ops["x"].astype(np.float64) - ops["mean"].astype(np.float64)) * ops["rstd"].astype(np.float64)
    return ((pre * (g * xhat).sum(1)) ** 2).sum(0), gb2
