"""CPU: the float64 references of the squared-sum kernels (``diag_sq_refs.py``) against per-sample ``torch.autograd.grad``
of a float64 ``conv2d`` / ``batch_norm``, the exactness condition of every case, and the case table against the library's
host arithmetic: ``hf_conv2d_nhwc_sqsum_plan`` answers every case with a count the launch rule accepts, every forced
count of the table is one the rule accepts, and every refusal case is refused -- by the planner for the geometries, by
the launching entry points (which refuse before they launch anything) for the split counts."""

import ctypes

import numpy as np
import pytest
import torch

import diag_sq_refs as dr
from pytorchhessianfree_amd import _lib

PTR = _lib.c_void_p


def _ids(cases):
    return [c.name for c in cases]


def _geo(p):
    return [p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride[0], p.stride[1], p.pad[0], p.pad[1]]


@pytest.mark.parametrize("p", dr.CONV_CASES, ids=_ids(dr.CONV_CASES))
def test_conv_reference_is_the_sum_of_squared_per_sample_autograd_gradients(p):
    ops = dr.conv_operands(p)
    w = torch.zeros(p.k, p.c, p.r, p.s, dtype=torch.float64, requires_grad=True)
    want = torch.zeros(p.k, p.r, p.s, p.c, dtype=torch.float64)
    for i in range(p.n):
        x = torch.from_numpy(ops["x"][i:i + 1, ..., :p.c]).double().permute(0, 3, 1, 2)
        y = torch.nn.functional.conv2d(x, w, None, p.stride, p.pad)
        (g,) = torch.autograd.grad(y, w, torch.from_numpy(ops["gy"][i:i + 1]).double().permute(0, 3, 1, 2))
        want += (dr.PRE * g.permute(0, 2, 3, 1)) ** 2
    got = dr.conv_reference(p, ops)
    assert got.shape == (p.k, p.r, p.s, dr.out_c(p))
    assert torch.equal(got, want[..., :dr.out_c(p)])
    assert not bool(got[torch.from_numpy(dr.dead_mask(p))].any())       # dead taps: a zero reference
    assert bool(got.any())
    assert torch.equal(dr.conv_reference(p, ops, 0.5 * dr.PRE), 0.25 * got)


@pytest.mark.parametrize("p", dr.CHAN_CASES, ids=_ids(dr.CHAN_CASES))
def test_chan_reference_is_the_sum_of_squared_per_sample_batchnorm_gradients(p):
    ops = dr.chan_operands(p)
    eps = 2.0 ** -20   # (batch_norm wants a positive eps: var + eps is exactly 1 / rstd^2 in float64)
    mean, var = torch.from_numpy(ops["mean"]).double(), 1.0 / torch.from_numpy(ops["rstd"]).double() ** 2 - eps
    gamma = torch.ones(p.c, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros(p.c, dtype=torch.float64, requires_grad=True)
    want_w, want_b = torch.zeros(p.c, dtype=torch.float64), torch.zeros(p.c, dtype=torch.float64)
    for i in range(p.n):
        x = torch.from_numpy(ops["x"][i]).double().t().reshape(1, p.c, p.hw, 1)
        y = torch.nn.functional.batch_norm(x, mean, var, gamma, beta, False, 0.0, eps)
        gw, gb = torch.autograd.grad(y, (gamma, beta), torch.from_numpy(ops["g"][i]).double().t().reshape(1, p.c, p.hw, 1))
        want_w += (dr.PRE * gw) ** 2
        want_b += (dr.PRE * gb) ** 2
    gw2, gb2 = dr.chan_reference(p, ops)
    assert np.array_equal(gw2, want_w.numpy()) and np.array_equal(gb2, want_b.numpy())
    assert gw2.any() and gb2.any()
    none, gb2_only = dr.chan_reference(p, ops, with_x=False)
    assert none is None and np.array_equal(gb2_only, gb2)


def test_every_case_meets_its_exactness_condition():
    for p in dr.CONV_CASES:
        assert dr.conv_exact(p), p.name
        ref = dr.conv_reference(p, dr.conv_operands(p))
        assert torch.equal(ref, ref.round()) and float(ref.max()) < dr.EXACT_LIMIT, p.name
    for p in dr.CHAN_CASES:
        assert dr.chan_exact(p), p.name
        for ref in dr.chan_reference(p, dr.chan_operands(p)):
            assert np.array_equal(ref * 4, np.round(ref * 4)) and ref.max() < dr.EXACT_LIMIT, p.name
    near = next(p for p in dr.CONV_CASES if p.name.startswith("p256"))
    assert 81 * 256 ** 2 * near.n > dr.EXACT_LIMIT // 2     # (the case that sits near the limit)


def test_the_table_covers_what_it_names():
    by = {p.name: p for p in dr.CONV_CASES}
    P = lambda p: dr.out_hw(p)[0] * dr.out_hw(p)[1]  # noqa: E731
    assert [P(by[n]) for n in ("p64_sample_ends_on_step_ends", "p25_sample_ends_inside_a_step", "p16_stride_2", "p4",
                               "p256_several_steps_per_sample")] == [64, 25, 16, 4, 256]
    assert P(by["p1_one_live_tap_of_nine"]) == 1 and len(dr.live_taps(by["p1_one_live_tap_of_nine"])) == 1
    assert by["two_row_tiles"].k > 64 and by["scalar_gathers"].c % 4
    stem = by["stem_form_padded_columns"]
    assert (stem.c, stem.out_c, stem.act_ld, stem.r * stem.s) == (12, 9, 12, 1)
    assert dr.forced_splits(5) == [1, 2, 5] and -(-5 // 2) == 3   # n = 5 in two splits: shares of 3 + 2


@pytest.mark.parametrize("p", dr.CONV_CASES, ids=_ids(dr.CONV_CASES))
def test_planned_and_forced_split_counts_are_accepted(p):
    lib = _lib.load()
    planned = lib.hf_conv2d_nhwc_sqsum_plan(*_geo(p), 0)
    assert planned >= 1 and dr.shares_ok(p.n, planned), (p.name, planned)
    for target in (1, 7, 64, 1024, 1 << 20):
        sp = lib.hf_conv2d_nhwc_sqsum_plan(*_geo(p), target)
        assert 1 <= sp <= p.n and dr.shares_ok(p.n, sp), (p.name, target, sp)
    assert lib.hf_conv2d_nhwc_sqsum_plan(*_geo(p), 1) == 1
    for sp in dr.forced_splits(p.n):
        assert dr.shares_ok(p.n, sp), (p.name, sp)
    assert _lib.conv_sqsum_plan(p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad) == planned


def test_refusal_cases_are_refused_before_any_launch():
    lib = _lib.load()
    for g in dr.REFUSED_GEOMETRIES:
        n, h, w, c, k, r, s, st, pd = g
        assert lib.hf_conv2d_nhwc_sqsum_plan(n, h, w, c, k, r, s, st, st, pd, pd, 0) == _lib.HF_ERR_ARG, g
    # host buffers: a refused call reads and writes nothing
    buf = (ctypes.c_float * 64)()
    ptr = PTR((ctypes.addressof(buf) + 15) & ~15)
    for n, splits in dr.REFUSED_SPLITS:
        assert not dr.shares_ok(n, splits)
        rc = lib.hf_conv2d_nhwc_sqsum_slabs(ptr, ptr, ptr, n, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1, 0, 0, 1.0, splits, 1 << 20,
                                            _lib.HF_F32, None)
        assert rc == _lib.HF_ERR_ARG, (n, splits)
        rc = lib.hf_chan_sqsum(ptr, ptr, ptr, ptr, ptr, ptr, n, 8, 4, 1.0, splits, _lib.HF_F32, None)
        assert rc == _lib.HF_ERR_ARG, (n, splits)
    ok = (4, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1)
    sq = lib.hf_conv2d_nhwc_sqsum_slabs
    assert sq(None, ptr, ptr, *ok, 0, 0, 1.0, 1, 0, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert sq(ptr, ptr, ptr, *ok, 0, 0, float("nan"), 1, 0, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert sq(ptr, ptr, ptr, *ok, 0, 0, float("inf"), 1, 0, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert sq(ptr, ptr, ptr, *ok, 0, 9, 1.0, 1, 0, _lib.HF_F32, None) == _lib.HF_ERR_ARG            # out_c > c
    assert sq(ptr, ptr, ptr, *ok, 4, 0, 1.0, 1, 0, _lib.HF_F32, None) == _lib.HF_ERR_ARG            # act_ld < c
    assert sq(ptr, ptr, ptr, *ok, 0, 0, 1.0, 2, 8 * 9 * 8 - 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG  # slabs overlap
    assert sq(ptr, ptr, ptr, *ok, 0, 0, 1.0, 1, 0, _lib.HF_F32 + 1, None) == _lib.HF_ERR_ARG
    ch = lib.hf_chan_sqsum
    assert ch(None, None, ptr, ptr, ptr, ptr, 4, 8, 4, 1.0, 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG   # no output
    assert ch(ptr, ptr, None, ptr, ptr, ptr, 4, 8, 4, 1.0, 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert ch(ptr, ptr, ptr, None, None, None, 4, 8, 4, 1.0, 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG  # gw2 without xhat
    assert ch(None, ptr, ptr, ptr, None, ptr, 4, 8, 4, 1.0, 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG   # x without mean
    assert ch(ptr, ptr, ptr, ptr, ptr, ptr, 4, 8, 4, float("nan"), 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert ch(ptr, ptr, ptr, ptr, ptr, ptr, 4, 8, 0, 1.0, 1, _lib.HF_F32, None) == _lib.HF_ERR_ARG
    assert not np.asarray(buf).any()


def test_engine_argument_builders_match_the_prototypes():
    """``engine/problems.py``: the positional argument lists (without ``dtype, stream``) of the two launching entry points,
    every value where the prototype of include/hf_pcg.h has it."""
    from pytorchhessianfree_amd.engine import problems as P

    out, act, mat = torch.zeros(3, 40), torch.zeros(8), torch.zeros(8)
    args = P.conv_sqsum_args(out, act, mat, (5, 6, 7, 8, 9, 3, 2, (2, 1), (1, 0)), 3, 16.0, act_ld=12, out_c=7)
    assert len(args) == len(_lib.SIGNATURES["hf_conv2d_nhwc_sqsum_slabs"][1]) - 2
    assert args == (out, act, mat, 5, 6, 7, 8, 9, 3, 2, 2, 1, 1, 0, 12, 7, 16.0, 3, 40)
    g, gb2 = torch.zeros(4), torch.zeros(4)
    args = P.chan_sqsum_args(g, 5, 8, 9, 2, 0.5, gb2=gb2)
    assert len(args) == len(_lib.SIGNATURES["hf_chan_sqsum"][1]) - 2
    assert args == (None, gb2, g, None, None, None, 5, 8, 9, 0.5, 2)
    x, mean, rstd, gw2 = (torch.zeros(4) for _ in range(4))
    assert P.chan_sqsum_args(g, 5, 8, 9, 2, 0.5, gw2=gw2, x=x, mean=mean, rstd=rstd)[:6] == (gw2, None, g, x, mean, rstd)
