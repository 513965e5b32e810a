"""CPU: the numpy references of the dense-stack session's kernels (``dense_session_refs``) against float64 torch.

Bounds come from the number format alone (``u = 2**-24``, ``R`` = spread of a row's logits):

* softmax: the argument ``x - m`` carries one rounding (``<= u R`` absolute), float32 ``exp`` is taken as accurate to two
  ulp (``4 u``), the fp64 sum of positive terms is no worse than its worst term, its rounding to fp32 and the division
  add ``u`` each: ``|p - p64| <= (2 R + 10) u p64``;
* cross-entropy: a row's term ``log S - (x_t - m)`` inherits the sum's relative error as an absolute one,
  ``(R + 4) u``; the loss adds one rounding of its own;
* mean-squared error: one rounding in ``d``, hence ``2 u`` in its square and in the fp64 sum, one for the rounding of
  the sum, one for ``coef``, one for the product: ``6 u`` relative."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_session_refs as sr

U = sr.U32


def _spread(x):
    return float((x.max(1) - x.min(1)).max())


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("rows,c", [(1, 2), (2, 10), (65, 100), (256, 1024)])
def test_ce_head_against_float64(rows, c, reduction):
    x, t = sr.logits_case(rows, c)
    sg, sps, _ = sr.loss_scales(sr.CE, rows, c, reduction)
    p, dl, dl_ps, loss, flag = sr.ce_head(x, t, sg, sps, reduction)
    x64, t64 = torch.from_numpy(x).double(), torch.from_numpy(t)
    p64 = torch.softmax(x64, 1).numpy()
    R = _spread(x)
    assert flag == 0 and p.dtype == np.float32 and loss.dtype == np.float32
    assert (abs(p.astype(np.float64) - p64) <= (2 * R + 10) * U * p64).all()
    l64 = float(F.cross_entropy(x64, t64, reduction=reduction))
    n = rows if reduction == "sum" else 1
    assert abs(float(loss) - l64) <= n * (R + 4) * U + U * abs(l64)
    onehot = F.one_hot(t64, c).numpy().astype(np.float32)
    assert np.array_equal(dl, ((p - onehot).astype(np.float32) * np.float32(sg)).astype(np.float32))
    assert np.array_equal(dl_ps, ((p - onehot).astype(np.float32) * np.float32(sps)).astype(np.float32))
    # d loss / d logits of torch in float64: (p - onehot) * scale
    x64.requires_grad_(True)
    (g64,) = torch.autograd.grad(F.cross_entropy(x64, t64, reduction=reduction), x64)
    assert (abs(dl.astype(np.float64) - g64.numpy()) <= ((2 * R + 10) * p64 + 3 * abs(g64.numpy() / sg)) * U * sg).all()


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("rows,c", [(1, 1), (17, 3), (256, 100), (3, 4097)])
def test_mse_head_against_float64(rows, c, reduction):
    x, t = sr.mse_case(rows, c)
    sg, sps, _ = sr.loss_scales(sr.MSE, rows, c, reduction)
    dl, dl_ps, loss, flag = sr.mse_head(x, t, sg, sps, reduction)
    x64, t64 = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(t).double()
    l64 = F.mse_loss(x64, t64, reduction=reduction)
    (g64,) = torch.autograd.grad(l64, x64)
    assert flag == 0 and abs(float(loss) - float(l64)) <= 6 * U * float(l64)
    assert (abs(dl.astype(np.float64) - g64.numpy()) <= 3 * U * abs(g64.numpy())).all()
    per_sample = rows if reduction == "mean" else 1
    assert (abs(dl_ps.astype(np.float64) - per_sample * g64.numpy()) <= 3 * U * per_sample * abs(g64.numpy())).all()


def test_out_of_range_targets_set_the_flag_and_add_nothing():
    x, t = sr.logits_case(5, 7)
    for bad in (-100, 7):
        tb = t.copy()
        tb[2] = bad
        p, dl, _, loss, flag = sr.ce_head(x, tb, 1.0, 1.0, "sum")
        keep = [0, 1, 3, 4]
        p0, dl0, _, loss0, flag0 = sr.ce_head(x[keep], t[keep], 1.0, 1.0, "sum")
        assert flag == 1 and flag0 == 0
        assert np.isfinite(p).all() and np.isfinite(dl).all() and np.isfinite(loss)
        assert np.array_equal(dl[2], p[2])          # no one in the row's one-hot
        assert np.array_equal(dl[keep], dl0) and loss == loss0  # the other rows and the loss do not see it


def test_large_logits_stay_finite():
    x, t = sr.logits_case(9, 33, offset=1e4)
    p, dl, dl_ps, loss, flag = sr.ce_head(x, t, 1.0 / 9, 1.0, "mean")
    assert all(np.isfinite(a).all() for a in (p, dl, dl_ps)) and np.isfinite(loss) and flag == 0
    l64 = float(F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(t)))
    assert abs(float(loss) - l64) <= (_spread(x) + 4) * U + U * abs(l64)


@pytest.mark.parametrize("splits", [1, 2, 5, 32])
@pytest.mark.parametrize("with_b", [True, False])
def test_act_forward_against_torch_and_numpy(splits, with_b):
    g = np.random.default_rng(splits)
    slabs = g.standard_normal((splits, 3, 65)).astype(np.float32)
    b = g.standard_normal(65).astype(np.float32) if with_b else None
    pre = sr.act_forward(slabs, b, sr.IDENTITY)
    # the slab sum against float64: (splits - 1) + bias additions, each one rounding of the running magnitude
    s64 = slabs.astype(np.float64).sum(0) + (b.astype(np.float64)[None, :] if with_b else 0.0)
    mag = abs(slabs).astype(np.float64).sum(0) + (abs(b).astype(np.float64)[None, :] if with_b else 0.0)
    assert (abs(pre.astype(np.float64) - s64) <= max(splits - 1 + int(with_b), 1) * U * mag).all()
    relu = sr.act_forward(slabs, b, sr.RELU)
    assert np.array_equal(relu, F.relu(torch.from_numpy(pre)).numpy()) and not np.signbit(relu).any()
    tanh = sr.act_forward(slabs, b, sr.TANH)
    assert np.array_equal(tanh, np.tanh(pre))
    assert (abs(tanh.astype(np.float64) - np.tanh(pre.astype(np.float64))) <= 4 * U).all()  # (two ulp of values < 1)
