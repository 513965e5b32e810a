"""CPU: the float64 references of the pooled-layer kernels (``pool_act_refs``) against ``torch.autograd.functional``'s
``jvp`` / ``vjp`` of ``max_pool2d(relu(a + b))`` -- to equality: the operands are multiples of 1/8, every sum is exact
-- for every pool geometry and map size of the kernel tests, with and without the ReLU, and the partial-row convention
of the bias sums (shares of the full-resolution rows, ``hf_chan_affine_bwd_ex``'s)."""

import pytest
import torch
from torch.autograd.functional import jvp, vjp

import pool_act_refs as R


def _f(relu, k, s, p):
    def f(a, b):
        z = a + b
        z = torch.relu(z) if relu else z
        return torch.nn.functional.max_pool2d(z.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    return f


@pytest.mark.parametrize("hw", R.MAPS)
@pytest.mark.parametrize("geom", R.GEOMS)
@pytest.mark.parametrize("relu", [0, 1])
def test_references_equal_autograd_in_float64(geom, hw, relu):
    (k, s, p), (h, w) = geom, hw
    n, c = 2, 4
    o = R.case(n, c, h, w, k, s, p, 2, 3)
    y_pool, idx = R.forward(o["a"], o["b"], k, s, p, relu)
    if relu:
        assert bool((y_pool <= 0).any()) or (h, w) == (3, 3), "no masked window in this case"
    a64, b64 = o["a"].double(), o["b"].double()
    f = _f(relu, k, s, p)
    # tangent
    t_a, v_b = o["slabs"].double().sum(0), o["v_b"].double()
    _, want_t = jvp(f, (a64, b64), (t_a, v_b))
    got_t, M = R.tangent(o["slabs"], o["v_b"], idx, y_pool, relu)
    assert torch.equal(got_t, want_t)
    assert bool((M >= got_t.abs()).all())
    got_nb, _ = R.tangent(o["slabs"], None, idx, y_pool, relu)
    _, want_nb = jvp(f, (a64, b64), (t_a, torch.zeros_like(v_b)))
    assert torch.equal(got_nb, want_nb)
    # adjoint
    g_pool = o["gy"].double().sum(0)
    _, (want_ga, want_gb) = vjp(f, (a64, b64), g_pool)
    for rb in (1, 3):
        ga, Mg, gb, windows = R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, p, rb)
        assert torch.equal(ga, want_ga)
        assert tuple(gb.shape) == (rb, c) and torch.equal(gb.sum(0), want_gb)
        rows, per = n * h * w, -(-n * h * w // rb)
        for b in range(rb):  # share b = rows [b*per, (b+1)*per) of the full-resolution map
            assert torch.equal(gb[b], want_ga.reshape(rows, c)[b * per:(b + 1) * per].sum(0))
        assert 1 <= windows <= ((k + s - 1) // s) ** 2
    assert R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, p, 0)[2] is None


def test_an_empty_share_is_an_error():
    o = R.case(1, 4, 3, 3, 2, 1, 0, 1, 1)
    y_pool, idx = R.forward(o["a"], o["b"], 2, 1, 0)
    with pytest.raises(ValueError):
        R.adjoint(o["gy"], idx, y_pool, 1, 3, 3, 2, 1, 0, 7)  # 9 rows: ceil(9/7) = 2, share 6 starts at row 12


def test_wrong_variants_are_told_apart():
    """What the references must not be confused with: the mask taken from the cotangent's own position, the bias added
    behind the mask, pooled rows instead of full-resolution rows for the shares."""
    k, s, p, h, w = 3, 2, 0, 5, 7
    o = R.case(2, 4, h, w, k, s, p, 2, 2)
    y_pool, idx = R.forward(o["a"], o["b"], k, s, p)
    got, _ = R.tangent(o["slabs"], o["v_b"], idx, y_pool, 1)
    unmasked, _ = R.tangent(o["slabs"], o["v_b"], idx, y_pool, 0)
    assert not torch.equal(got, unmasked)
    behind = R.tangent(o["slabs"], None, idx, y_pool, 1)[0] + o["v_b"].double()
    assert not torch.equal(got, behind)
    ga, _, gb, _ = R.adjoint(o["gy"], idx, y_pool, 1, h, w, k, s, p, 3)
    oh, ow = o["oh"], o["ow"]
    pooled_rows = o["gy"].double().sum(0).reshape(2 * oh * ow, 4)
    per = -(-2 * oh * ow // 3)
    assert not torch.equal(gb[0], pooled_rows[:per].sum(0))
