"""GPU: ``hf_flatten_nhwc_rows`` / ``hf_unflatten_slabs_nhwc`` (the boundary between a conv stack's NHWC maps and a
classifier tail's rows) through the C ABI against ``flatten_refs`` -- no engine, no ``modelprep``.

Both comparisons are ``torch.equal``: the flatten is a permutation, the unflatten forms the same fp32 additions in the
same order as the reference.  Outputs lie in sentinel-filled buffers with guard words behind them; every launch runs
twice and the two results are compared bitwise."""

import pytest
import torch

import flatten_refs as R
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = -7.5  # (no operand holds it: flatten operands are positive integers)
P = _lib.c_void_p
ERR_ARG, ERR_ALIGN = _lib.HF_ERR_ARG, -2  # hf_status of include/hf_pcg.h
F32 = _lib.HF_F32


def p(t):
    return P(t.data_ptr()) if t is not None else None


def st():
    return _lib.current_stream_ptr(torch.device(DEV))


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("n,hw,c", R.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("wide,half", [(0, 0), (1, 0), (1, 1)], ids=["plain", "tx_half", "x_half"])
@pytest.mark.parametrize("pad", [0, 4])
def test_flatten_is_the_permutation(n, hw, c, wide, half, pad):
    in_ld, out_ld = (2 * c if wide else c), c * hw + pad
    buf, off = R.operand(n, hw, c, in_ld, half)
    want = R.flatten(buf, off, in_ld, n, hw, c, out_ld, SENT)
    src, lib = buf.to(DEV), _lib.load()

    def launch():
        out = torch.full((n * out_ld + GUARD,), SENT, device=DEV)
        _lib.check(lib.hf_flatten_nhwc_rows(p(out), out_ld, P(src.data_ptr() + 4 * off), in_ld, n, hw, c, F32, st()),
                   "hf_flatten_nhwc_rows")
        return out

    a, b = launch(), launch()
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)), "two launches on the same operands differ"
    assert torch.equal(a[:n * out_ld].cpu(), want)  # (the rows' padding still holds the sentinel)
    assert bool((a[n * out_ld:] == SENT).all()), "a guard word was written"
    assert torch.equal(src.cpu(), buf)


@pytest.mark.parametrize("n,hw,c", R.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("splits", R.SPLITS)
def test_unflatten_is_the_ordered_slab_sum(n, hw, c, splits):
    numel = n * c * hw
    stride = numel + 12  # (above n*c*hw; any 4-byte boundary)
    s = R.slabs(n, hw, c, splits, seed=11 * splits + hw)
    want = R.unflatten(s, n, hw, c)
    sd = torch.full((splits, stride), float("nan"))
    sd[:, :numel] = s
    sd, lib = sd.to(DEV), _lib.load()

    def launch():
        out = torch.full((numel + GUARD,), SENT, device=DEV)
        _lib.check(lib.hf_unflatten_slabs_nhwc(p(out), p(sd), splits, stride, n, hw, c, F32, st()),
                   "hf_unflatten_slabs_nhwc")
        return out

    a, b = launch(), launch()
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)), "two launches on the same operands differ"
    assert torch.equal(a[:numel].cpu(), want)
    assert bool((a[numel:] == SENT).all()), "a guard word was written"


def test_unflatten_inverts_flatten():
    n, hw, c = 3, 30, 8
    buf, _ = R.operand(n, hw, c, c, 0)
    src, lib = buf.to(DEV), _lib.load()
    rows, back = torch.empty(n * c * hw, device=DEV), torch.empty(n * hw * c, device=DEV)
    _lib.check(lib.hf_flatten_nhwc_rows(p(rows), c * hw, p(src), c, n, hw, c, F32, st()), "hf_flatten_nhwc_rows")
    _lib.check(lib.hf_unflatten_slabs_nhwc(p(back), p(rows), 1, 0, n, hw, c, F32, st()), "hf_unflatten_slabs_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(back, src)


def test_refusals_launch_nothing():
    n, hw, c = 2, 4, 8
    numel, lib = n * hw * c, _lib.load()
    src = torch.arange(2 * numel + 8, dtype=torch.float32, device=DEV)
    out = torch.full((n * (c * hw + 4) + GUARD,), SENT, device=DEV)
    good_f = dict(out=p(out), out_ld=c * hw + 4, src=p(src), in_ld=2 * c, n=n, hw=hw, c=c, dtype=F32)

    def flat(**kw):
        a = dict(good_f, **kw)
        return lib.hf_flatten_nhwc_rows(a["out"], a["out_ld"], a["src"], a["in_ld"], a["n"], a["hw"], a["c"], a["dtype"], st())

    for bad in (dict(out=None), dict(src=None), dict(c=6, in_ld=12), dict(c=0), dict(in_ld=c - 4), dict(in_ld=c + 2),
                dict(out_ld=c * hw - 1), dict(n=0), dict(hw=0), dict(hw=(1 << 17) + 1, out_ld=1 << 21),
                dict(c=1 << 20, hw=2, in_ld=1 << 20, out_ld=1 << 21), dict(n=1 << 20, hw=1 << 10, out_ld=1 << 13),
                dict(dtype=_lib.HF_F64)):
        assert flat(**bad) == ERR_ARG, bad
    assert flat(src=P(src.data_ptr() + 4)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert flat() == 0 and flat(in_ld=c, out_ld=c * hw) == 0  # (the complete call is taken)

    g = torch.full((numel + GUARD,), SENT, device=DEV)
    good_u = dict(out=p(g), slabs=p(src), splits=2, stride=numel + 8, n=n, hw=hw, c=c, dtype=F32)

    def unflat(**kw):
        a = dict(good_u, **kw)
        return lib.hf_unflatten_slabs_nhwc(a["out"], a["slabs"], a["splits"], a["stride"], a["n"], a["hw"], a["c"],
                                           a["dtype"], st())

    for bad in (dict(out=None), dict(slabs=None), dict(c=6), dict(splits=0), dict(splits=1025), dict(stride=numel - 1),
                dict(n=0), dict(hw=0), dict(hw=(1 << 17) + 1), dict(n=1 << 20, hw=1 << 10, stride=1 << 40),
                dict(dtype=_lib.HF_F64)):
        assert unflat(**bad) == ERR_ARG, bad
    assert unflat(out=P(g.data_ptr() + 4)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((g == SENT).all())
    assert unflat() == 0 and unflat(splits=1, stride=0) == 0  # (one slab: the stride is not read)
    torch.cuda.synchronize()
