"""GPU: the squared-sum kernels behind the batched diagonal empirical Fisher -- ``hf_conv2d_nhwc_sqsum_slabs``
(``k_conv_tn_sq``: per-sample form, squared-operand form, element-wise gathers) and ``hf_chan_sqsum`` -- through the C
ABI against the float64 references of ``diag_sq_refs.py``, EXACTLY: the operands are small integers and ``pre`` a power of
two, so every intermediate of every split is exactly representable (the module states the condition) and the result
must equal the reference at every element whatever the split count.

The outputs are ``guarded.SlabOut``, as in the convolution tests: every output lies between GUARD NaN sentinels, slabs are
SLAB_GAP floats apart and the gaps are NaN too.  After a launch: guards and gaps untouched; every slab completely written except the
entries of dead taps, which keep the sentinel and have a zero reference; the float64 sum of the slabs IS the reference; a
second launch gives the same bits; ``0.5 * pre`` scales the result by exactly 0.25; a refused launch leaves the outputs
untouched.  Every case runs with the planned split count and with the forced counts 1, 2 and n."""

import numpy as np
import pytest
import torch

import diag_sq_refs as dr
from guarded import DEV, GUARD, NAN, P, SlabOut, bits_equal, dev, st
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name for c in cases]


class Out(SlabOut):
    def check(self, what, want, dead=None):
        """Guards, gaps, complete slabs, dead entries, exact sum (``want``: float64, flat)."""
        assert bool(torch.isnan(self.buf[~self.inside]).all()), "%s: a guard or a gap between slabs was written" % what
        slabs = self.slabs()
        unwritten = torch.isnan(slabs)
        if dead is None:
            dead = torch.zeros(self.numel, dtype=torch.bool, device=DEV)
        assert bool((unwritten == dead.expand_as(unwritten)).all()), \
            "%s: the unwritten entries are not exactly those of the dead taps" % what
        assert not bool(want[dead].any())
        got = torch.nan_to_num(slabs, nan=0.0).double().sum(0)
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).reshape(-1)
            i = int(bad[0])
            raise AssertionError("%s: %d of %d elements differ from the float64 reference, first at %d: %r != %r" % (
                what, bad.numel(), got.numel(), i, float(got[i]), float(want[i])))

_CONV = {}


def _conv(p):
    """Device operands, float64 reference (flat, on the device) and dead-tap mask of case ``p`` (once per case)."""
    if p.name not in _CONV:
        assert dr.conv_exact(p)
        host = dr.conv_operands(p)
        ref = dr.conv_reference(p, host).reshape(-1).to(DEV)
        assert torch.equal(ref, ref.round()) and float(ref.max()) < dr.EXACT_LIMIT
        _CONV[p.name] = (dev(host["x"]), dev(host["gy"]), ref, torch.from_numpy(dr.dead_mask(p).reshape(-1)).to(DEV))
    return _CONV[p.name]


def _geo(p):
    return [p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride[0], p.stride[1], p.pad[0], p.pad[1]]


def _sqsum(p, out, pre, splits=None):
    x, gy = _conv(p)[:2]
    return _lib.load().hf_conv2d_nhwc_sqsum_slabs(
        P(out.ptr), P(x.data_ptr()), P(gy.data_ptr()), *_geo(p), p.act_ld, p.out_c, pre,
        out.splits if splits is None else splits, out.stride, _lib.HF_F32, st())


def _split_counts(p):
    planned = _lib.load().hf_conv2d_nhwc_sqsum_plan(*_geo(p), 0)
    assert planned >= 1
    return [("planned", planned)] + [("forced", sp) for sp in dr.forced_splits(p.n)]


@pytest.mark.parametrize("p", dr.CONV_CASES, ids=_ids(dr.CONV_CASES))
def test_conv_sqsum_equals_float64_exactly_at_every_split_count(p):
    _x, _gy, ref, dead = _conv(p)
    numel = p.k * p.r * p.s * dr.out_c(p)
    for kind, splits in _split_counts(p):
        what = "%s, %s %d splits" % (p.name, kind, splits)
        out = Out(numel, splits)
        _lib.check(_sqsum(p, out, dr.PRE), what)
        torch.cuda.synchronize()
        out.check(what, ref, dead)
        first = out.buf.clone()
        _lib.check(_sqsum(p, out, dr.PRE), what)
        torch.cuda.synchronize()
        assert bits_equal(out.buf, first), "%s: a second launch gives other bits" % what
        half = Out(numel, splits)
        _lib.check(_sqsum(p, half, 0.5 * dr.PRE), what)
        torch.cuda.synchronize()
        half.check(what + ", pre / 2", 0.25 * ref, dead)
        assert torch.equal(torch.nan_to_num(half.slabs()) * 4.0, torch.nan_to_num(out.slabs())), \
            "%s: half the factor is not a quarter of every slab" % what


def test_conv_sqsum_shares_are_the_samples_in_order():
    """n = 5 in two splits: slab 0 holds samples 0..2, slab 1 samples 3..4 -- each slab IS the reference of its share."""
    p = next(c for c in dr.CONV_CASES if c.n == 5)
    host = dr.conv_operands(p)
    dw = dr.per_sample_wgrad(p, host)
    out = Out(p.k * p.r * p.s * p.c, 2)
    _lib.check(_sqsum(p, out, dr.PRE), p.name)
    torch.cuda.synchronize()
    for sl, share in ((0, slice(0, 3)), (1, slice(3, 5))):
        want = ((dr.PRE * dw[share]) ** 2).sum(0).reshape(-1).to(DEV)
        assert torch.equal(out.slabs()[sl].double(), want), sl


@pytest.mark.parametrize("n,splits", dr.REFUSED_SPLITS)
def test_refused_split_counts_leave_the_outputs_untouched(n, splits):
    p = next(c for c in dr.CONV_CASES if c.n == n)
    assert not dr.shares_ok(n, splits)
    out = Out(p.k * p.r * p.s * dr.out_c(p), max(splits, 1))
    assert _sqsum(p, out, dr.PRE, splits) == _lib.HF_ERR_ARG
    ch = dr.CHAN_CASES[0]
    g = torch.zeros(n, ch.hw, ch.c, device=DEV)
    rows = Out(ch.c * max(splits, 1), 1)
    rc = _lib.load().hf_chan_sqsum(None, P(rows.ptr), P(g.data_ptr()), None, None, None, n, ch.c, ch.hw, dr.PRE,
                                   splits, _lib.HF_F32, st())
    assert rc == _lib.HF_ERR_ARG
    torch.cuda.synchronize()
    assert out.pristine() and rows.pristine()


def _chan(p, row_blocks, pre, gw2=True, gb2=True, x=True):
    host = dr.chan_operands(p)
    ops = {k: dev(v) for k, v in host.items()}
    # (partial rows are c elements apart by the ABI: dense rows between guards)
    bw = torch.full((2 * GUARD + row_blocks * p.c,), NAN, device=DEV)
    bb = torch.full((2 * GUARD + row_blocks * p.c,), NAN, device=DEV)

    def launch():
        _lib.check(_lib.load().hf_chan_sqsum(
            P(bw.data_ptr() + 4 * GUARD) if gw2 else None, P(bb.data_ptr() + 4 * GUARD) if gb2 else None,
            P(ops["g"].data_ptr()), *((P(ops[k].data_ptr()) if x else None) for k in ("x", "mean", "rstd")),
            p.n, p.c, p.hw, pre, row_blocks, _lib.HF_F32, st()), "hf_chan_sqsum")
        torch.cuda.synchronize()

    launch()
    first = (bw.clone(), bb.clone())
    launch()
    assert bits_equal(bw, first[0]) and bits_equal(bb, first[1]), "second launch: other bits"
    want_w, want_b = dr.chan_reference(p, host, pre, with_x=x)
    for buf, on, want in ((bw, gw2, want_w), (bb, gb2, want_b)):
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + row_blocks * p.c:]).all())
        rows = buf[GUARD:GUARD + row_blocks * p.c].view(row_blocks, p.c)
        if not on:
            assert bool(torch.isnan(rows).all())
            continue
        assert not bool(torch.isnan(rows).any()), "a partial row was not completely written"
        assert np.array_equal(rows.double().sum(0).cpu().numpy(), want), (p.name, row_blocks)
    return bw, bb


@pytest.mark.parametrize("p", dr.CHAN_CASES, ids=_ids(dr.CHAN_CASES))
def test_chan_sqsum_equals_float64_exactly_at_every_row_block_count(p):
    assert dr.chan_exact(p)
    for rb in dr.forced_splits(p.n):
        bw, bb = _chan(p, rb, dr.PRE)
        hw_, hb = _chan(p, rb, 0.5 * dr.PRE)
        assert torch.equal(torch.nan_to_num(hw_) * 4.0, torch.nan_to_num(bw))
        assert torch.equal(torch.nan_to_num(hb) * 4.0, torch.nan_to_num(bb))


@pytest.mark.parametrize("null", ["gw2", "gb2", "x"])
def test_chan_sqsum_with_each_nullable_operand_null(null):
    p = dr.CHAN_CASES[0]
    if null == "x":  # (a convolution bias: no xhat, so no scale entry either)
        _chan(p, 2, dr.PRE, gw2=False, x=False)
    else:
        _chan(p, 2, dr.PRE, gw2=null != "gw2", gb2=null != "gb2")
