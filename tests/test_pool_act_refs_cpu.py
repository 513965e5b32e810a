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


def _anchor(geom, hw, relu, c):
    (k, s, p), (h, w) = geom, hw
    n = 2
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
        (kh, kw), (sh, sw) = R.pair(k), R.pair(s)
        assert 1 <= windows <= ((kh + sh - 1) // sh) * ((kw + sw - 1) // sw)
    assert R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, p, 0)[2] is None


@pytest.mark.parametrize("hw", R.MAPS)
@pytest.mark.parametrize("geom", R.GEOMS)
@pytest.mark.parametrize("relu", [0, 1])
def test_references_equal_autograd_in_float64(geom, hw, relu):
    _anchor(geom, hw, relu, 4)


AXIS_IDS = [str(e).replace(" ", "") for e in R.AXIS_GEOMS]


@pytest.mark.parametrize("geom, hw", R.AXIS_GEOMS, ids=AXIS_IDS)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", [4, 3])
def test_references_equal_autograd_on_per_axis_windows(geom, hw, relu, c):
    _anchor(geom, hw, relu, c)


def test_an_int_is_the_pair_of_itself():
    """Integer geometries keep their operands (the seed string is the int's) and mean what the pair means."""
    for (k, s, p) in R.GEOMS:
        h, w = 5, 7
        assert R.out_hw(h, w, k, s, p) == R.out_hw(h, w, (k, k), (s, s), (p, p))
        o = R.case(2, 4, h, w, k, s, p, 1, 2)
        y_pool, idx = R.forward(o["a"], o["b"], k, s, p)
        a = R.adjoint(o["gy"], idx, y_pool, 1, h, w, k, s, p, 3)
        b = R.adjoint(o["gy"], idx, y_pool, 1, h, w, (k, k), (s, s), (p, p), 3)
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert R._seed("pool-act", 2, 4, 5, 7, 3, 2, 1) != R._seed("pool-act", 2, 4, 5, 7, (3, 3), (2, 2), (1, 1))
    # the first plane of an integer case is the first draw behind the seed string of the int, as it always was
    gen = torch.Generator().manual_seed(R._seed("pool-act", 2, 4, 5, 7, 3, 2, 1, 1, 2, True, ""))
    first = (torch.randperm(35, generator=gen).view(5, 7).float() - 0.75 * 35) / 8.0
    o = R.case(2, 4, 5, 7, 3, 2, 1, 1, 2)
    assert torch.equal(o["a"][0, :, :, 0] + o["b"][0], first)


def test_axis_geoms_hold_every_entry_with_its_transpose():
    assert len(R.AXIS_GEOMS) >= 6 and len(set(R.AXIS_GEOMS)) == len(R.AXIS_GEOMS)
    for geom, (h, w) in R.AXIS_GEOMS:
        assert (tuple((b, a) for a, b in geom), (w, h)) in R.AXIS_GEOMS
        assert R.exchanges(geom), "a square entry"
        oh, ow = R.out_hw(h, w, *geom)
        assert oh >= 1 and ow >= 1 and all(2 * pd <= k for k, pd in zip(geom[0], geom[2]))
    for need in ((((3, 2), (2, 1), (1, 0)), (5, 7)), (((2, 3), (2, 2), (0, 1)), (6, 5)), (((1, 2), (1, 2), (0, 0)), (2, 9)),
                 (((2, 3), (1, 2), (0, 1)), (7, 5))):
        assert need in R.AXIS_GEOMS


@pytest.mark.parametrize("geom, hw", R.AXIS_GEOMS, ids=AXIS_IDS)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", [4, 3])
def test_per_axis_cases_tell_an_exchanged_window_apart(geom, hw, relu, c):
    """The adjoint with (kh, kw), (sh, sw) or (ph, pw) exchanged in the window predicate alone -- the map, oh, ow and
    idx as they are: what ``pool_act_adjoint_at`` would compute from the other axis' parameter -- differs from the right
    one, in ga and in every number of row blocks' sums, on the operands of the GPU tests."""
    (k, s, p), (h, w) = geom, hw
    o = R.case(2, c, h, w, k, s, p, 1, 2)
    y_pool, idx = R.forward(o["a"], o["b"], k, s, p, relu)
    ga, _, gb, _ = R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, p, 1)
    for name, (k2, s2, p2) in R.exchanges(geom):
        ga2, _, gb2, _ = R.adjoint(o["gy"], idx, y_pool, relu, h, w, k2, s2, p2, 1)
        assert not torch.equal(ga2, ga), name
        assert not torch.equal(gb2, gb), name


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
