"""CPU: the cases of ``geometry_nets.py`` reach what they are named for, and its float64 reference is one -- without a
GPU.

Per case the map sizes, the live-tap masks (``common._live_taps``) and the BatchNorm adjoint's row-block counts equal the
literals of ``geometry_nets.GEOMETRY`` (the row-block rule is restated there: the engine's own ``u.rb`` is compared with
the same literals by the GPU tests); the library's planner (host arithmetic) takes every layer in all three directions;
the fp32 and the float64 forward pass take the same ReLU decisions (what lets the GPU tests cap the replayed decisions at
a handful); the reference's GGN product is ``J^T H J v`` of an explicitly built Jacobian, symmetric, its diagonal Fisher
the diagonal of the summed outer products; and ``row_map`` / ``col_map`` are each other's transpose, told apart without
the transposition.

The classifier-tail cases (``geometry_nets.TAILS``, at the end of the file): the same against ``TAIL_GEOMETRY``, with the
offsets of the tail's tensors in the flat vector and the dense kernels' split counts (the rule restated in
``geometry_nets.dense_plan`` against the library's ``hf_dense_plan``); fp32 and float64 take the same pool positions too;
the replay of pool positions is bounded; and a net whose first tail weight has its columns in another feature order than
(c, h, w) is told apart."""

import copy

import geometry_nets as gn
import pytest
import torch
from torch import nn

from pytorchhessianfree_amd import _lib
from pytorchhessianfree_amd.engine.common import _live_taps

POOLED = {"nonsquare_odd": (6, 3), "asym_stride": (4, 3), "row_map": (2, 6), "col_map": (6, 2), "batch_one": (4, 4),
          "wide_rows": (6, 5), "stem7": (4, 3), "plain_rect": (3, 9), "plain_quads_in": (2, 4)}
IM2COL_COLUMNS = {"nonsquare_odd": 9, "asym_stride": 27, "row_map": 9, "col_map": 9, "batch_one": 9, "wide_rows": 9,
                  "stem7": 147, "plain_rect": 9, "plain_quads_in": None}  # (4 input channels: no im2col)


def _layers(case):
    model, batches = gn.make(case)
    x = batches[0][0]
    mods = dict(model.named_modules())
    return model, x, [(mods[name], name, h, w, r, s, st, pd, oh, ow)
                      for name, h, w, r, s, st, pd, oh, ow in gn.conv_geometry(model, x)]


def test_the_case_list_is_the_issues():
    assert gn.CASES == list(gn.GEOMETRY) and len(gn.CASES) == 9
    assert {"row_map", "col_map"} <= set(gn.CASES)  # (each alone is symmetric to a swap of the other kind)
    assert gn.RESNETS["row_map"]["x"] == (5, 1, 4, 12) and gn.RESNETS["col_map"]["x"] == (5, 1, 12, 4)
    assert {k: v for k, v in gn.RESNETS["row_map"].items() if k != "x"} == {
        k: v for k, v in gn.RESNETS["col_map"].items() if k != "x"}


@pytest.mark.parametrize("case", gn.CASES)
def test_map_sizes_live_taps_and_row_blocks(case):
    model, x, layers = _layers(case)
    n = x.shape[0]
    got = [(name, (h, w), (oh, ow), _live_taps(h, w, r, s, st, pd), gn.adjoint_row_blocks(n * oh * ow, m.out_channels))
           for m, name, h, w, r, s, st, pd, oh, ow in layers]
    assert got == gn.GEOMETRY[case]
    # the map behind the (first) max-pool, and the first layer's im2col
    pools = [m for m in model.modules() if isinstance(m, nn.MaxPool2d)]
    assert len(pools) == 1
    seen = []
    hook = pools[0].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape[2:])))
    with torch.no_grad():
        out = model(x)
    hook.remove()
    assert seen == [POOLED[case]]
    first = layers[0][0]
    cols = first.in_channels * first.kernel_size[0] * first.kernel_size[1]
    assert (cols if (case in gn.RESNETS or first.in_channels < 4) else None) == IM2COL_COLUMNS[case]
    classes = (gn.RESNETS.get(case) or gn.STACKS[case])["classes"]
    assert tuple(out.shape) == (n, classes)
    # what the table names, in the model's own terms
    if case == "asym_stride":
        assert tuple(model.conv1.stride) == (1, 2) and tuple(model.maxpool.stride) == (2, 1)
        assert tuple(model.layers[0].conv1.stride) == tuple(model.layers[0].downsample[0].stride) == (2, 1)
        assert -(-cols // 4) * 4 == 28
    if case == "plain_rect":
        assert [tuple(m.kernel_size) for m, *_ in layers] == [(1, 3), (3, 1), (3, 3), (1, 1)]
        assert tuple(pools[0].kernel_size) == (3, 2) and tuple(pools[0].stride) == (2, 1)


@pytest.mark.parametrize("case", gn.CASES)
def test_the_planner_accepts_every_layer_in_every_direction(case):
    """``hf_conv2d_nhwc_plan`` as ``buffers._Buffers._plan`` asks it: direction 0 with ``c`` (forward) and ``2c``
    (the ``[t_x | x]`` operand), 1 and 2; the im2col'd first layer as a 1x1 product over its columns (padded to a
    multiple of 4 for the weight gradient)."""
    plan = _lib.load().hf_conv2d_nhwc_plan
    model, x, layers = _layers(case)
    n = x.shape[0]
    for i, (m, name, h, w, r, s, st, pd, oh, ow) in enumerate(layers):
        c, k = m.in_channels, m.out_channels
        if i == 0 and IM2COL_COLUMNS[case] is not None:
            j = c * r * s
            asked = [(0, n * oh * ow, 1, 1, j, k, 1, 1, 1, 1, 0, 0), (2, n * oh * ow, 1, 1, -(-j // 4) * 4, k, 1, 1, 1, 1, 0, 0)]
        else:
            asked = [(d, n, h, w, cc, k, r, s, st[0], st[1], pd[0], pd[1]) for d, cc in ((0, c), (0, 2 * c), (1, c), (2, c))]
        for args in asked:
            assert plan(*args, 0) >= 1, (name, args)


def _differing_decisions(model, x):
    a32 = gn.relu_inputs(copy.deepcopy(model), x)
    a64 = gn.relu_inputs(copy.deepcopy(model).double(), x.double())
    assert len(a32) == len(a64) > 0
    return sum(int(((p > 0) != (q > 0)).sum()) for p, q in zip(a32, a64))


@pytest.mark.parametrize("case", gn.CASES)
def test_fp32_and_float64_take_the_same_relu_decisions(case):
    for train in ([False, True] if case in gn.TRAIN_CASES else [False]):
        model, batches = gn.make(case, train)
        for x, _ in batches:
            assert _differing_decisions(model, x) == 0, (case, train)


def _flat_jacobian(model, x):
    """d logits / d theta, ``[n * classes, P]``, in float64 by ``torch.autograd.functional.jacobian``."""
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = tuple(dict(model.named_parameters())[n].detach() for n in names)

    def fn(*ps):
        return torch.func.functional_call(model, dict(zip(names, ps)), (x,)).reshape(-1)

    jac = torch.autograd.functional.jacobian(fn, params)
    return torch.cat([j.reshape(j.shape[0], -1) for j in jac], dim=1)


@pytest.mark.parametrize("case", ["nonsquare_odd", "plain_rect"])
def test_the_reference_is_the_explicit_ggn_symmetric_and_its_diagonal_the_summed_outer_products(case):
    model, batches = gn.make(case)
    x, t = batches[0]
    ref = gn.Reference(model, x, t)
    n = ref.gradient().numel()
    J = _flat_jacobian(ref.model, ref.x)
    H = torch.autograd.functional.hessian(lambda z: nn.functional.cross_entropy(z.view_as(ref.out), ref.t),
                                          ref.out.detach().reshape(-1))
    u, v = gn.probe(n, 1).double(), gn.probe(n, 2).double()
    gv, gu = ref.ggn(v), ref.ggn(u)
    want = J.t() @ (H @ (J @ v))
    assert float((gv - want).abs().max() / want.abs().max()) < 1e-10
    a, b = float(u @ gv), float(v @ gu)
    assert abs(a - b) <= 1e-12 * abs(a)
    # the gradient and the loss by the same Jacobian
    dl = torch.autograd.grad(nn.functional.cross_entropy(z := ref.out.detach().clone().requires_grad_(True), ref.t), z)[0]
    assert float((ref.gradient() - J.t() @ dl.reshape(-1)).abs().max() / ref.gradient().abs().max()) < 1e-10
    # diagonal Fisher: single-sample passes (another route than the reference's batch pass), outer products summed
    G = []
    for i in range(x.shape[0]):
        g = torch.autograd.grad(nn.functional.cross_entropy(ref.model(ref.x[i:i + 1]), ref.t[i:i + 1]), ref.params)
        G.append(torch.cat([a.reshape(-1) for a in g]))
    idx = torch.arange(0, n, 1 if n < 4000 else 7)  # (every entry of the small net; every 7th of the larger one)
    outer = sum(torch.outer(g[idx], g[idx]) for g in G) / x.shape[0]
    d = ref.diag_ef()
    assert float((d[idx] - outer.diagonal()).abs().max() / d.abs().max()) < 1e-12
    assert float(ref.loss()) > 0 and bool((d >= 0).all())


def _transposed_twin():
    """``col_map``'s net holding ``row_map``'s parameters with every kernel transposed, and ``row_map``'s input
    transposed: the same function of the same numbers, with the two map axes exchanged."""
    row, rb = gn.make("row_map")
    col, _ = gn.make("col_map")
    state = {k: (v.transpose(2, 3).contiguous() if v.dim() == 4 else v.clone()) for k, v in row.state_dict().items()}
    col.load_state_dict(state)
    for a, b in zip(row.modules(), col.modules()):
        if isinstance(a, nn.BatchNorm2d):
            b.eps = a.eps
    x, t = rb[0]
    return row, col, x, t


def _transpose_kernels(vec, model):
    out, off = [], 0
    for p in (p for p in model.parameters() if p.requires_grad):
        piece = vec[off:off + p.numel()].view_as(p)
        out.append((piece.transpose(2, 3) if p.dim() == 4 else piece).reshape(-1))
        off += p.numel()
    return torch.cat(out)


def test_row_map_and_col_map_are_transposes_and_the_reference_tells_them_apart():
    row, col, x, t = _transposed_twin()
    ref_r = gn.Reference(row, x, t)
    ref_c = gn.Reference(col, x.transpose(2, 3).contiguous(), t)
    assert tuple(ref_c.x.shape) == gn.RESNETS["col_map"]["x"]
    n = ref_r.gradient().numel()
    v = gn.probe(n, 3).double()
    got = ref_c.ggn(_transpose_kernels(v, row))   # v in col_map's layout
    want = _transpose_kernels(ref_r.ggn(v), row)  # row_map's product in col_map's layout
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    assert abs(ref_r.loss() - ref_c.loss()) < 1e-13
    # without the permutation the two products are far apart: a reference (or an engine) that exchanged the axes
    # somewhere cannot pass for the other
    plain = ref_c.ggn(v)
    assert float((plain - ref_r.ggn(v)).abs().max() / want.abs().max()) > 1e-2
    with pytest.raises(AssertionError, match="exactly zero"):  # (dead kernel ROWS of one are live in the other)
        gn.per_tensor_errors(plain, ref_r.ggn(v), gn.named_sizes(row))


def test_per_tensor_measure_sees_a_small_block_and_demands_exact_zeros():
    sizes = [("big", 6), ("small", 2)]
    want = torch.tensor([100.0, -50.0, 0.0, 3.0, 2.0, 1.0, 1e-6, -2e-6], dtype=torch.float64)
    got = want.clone()
    got[6] = 2e-6  # the small block wrong by half of its own size: 1e-8 of the whole vector's max-norm
    errs = gn.per_tensor_errors(got, want, sizes)
    assert errs["big"] == 0.0 and abs(errs["small"] - 0.5) < 1e-12
    assert float((got - want).abs().max() / want.abs().max()) < 1.1e-8
    got[2] = 1e-30
    with pytest.raises(AssertionError, match="exactly zero"):
        gn.per_tensor_errors(got, want, sizes)
    assert gn.per_tensor_errors(torch.zeros(8), torch.zeros(8, dtype=torch.float64), sizes) == {"big": 0.0, "small": 0.0}


def test_replayed_decisions_are_bounded():
    """A replayed mask may differ from the float64 net's own in at most ``MAX_FLIPS`` entries, all next to zero."""
    model, batches = gn.make("nonsquare_odd")
    x, t = batches[0]
    masks = gn.own_masks(copy.deepcopy(model).double(), x.double())
    assert gn.Reference(model, x, t, masks=masks).flips == [0]
    far = [m.clone() for m in masks]
    far[1].view(-1)[0] = ~far[1].view(-1)[0]  # one decision the other way, at an input that is not next to zero
    with pytest.raises(AssertionError, match="far from zero"):
        gn.Reference(model, x, t, masks=far)


# ---- the classifier-tail cases (``geometry_nets.TAILS``) -----------------------------------------------------------
def test_the_tail_case_list_is_the_issues():
    assert gn.TAIL_CASES == list(gn.TAIL_GEOMETRY) == ["tail_rect_pooled", "tail_wide_first", "tail_pixel",
                                                       "tail_rows_256", "tail_col_map"]
    assert not set(gn.TAIL_CASES) & set(gn.CASES) and set(gn.TAIL_CAPTURED_CASES) <= set(gn.TAIL_CASES)


def _pool_tuple(m):
    pair = lambda a: list(a) if isinstance(a, (tuple, list)) else [a, a]  # noqa: E731
    return tuple(pair(m.kernel_size) + pair(m.stride) + pair(m.padding))


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_tail_map_sizes_live_taps_offsets_and_plan(case):
    """Map sizes, live taps, row blocks, the pools, the offsets in the flat vector and the restated dense plan equal the
    literals of ``geometry_nets.TAIL_GEOMETRY``; the net's output is ``[batch, classes]``."""
    model, x, layers = _layers(case)
    lit, n = gn.TAIL_GEOMETRY[case], x.shape[0]
    got = [(name, (h, w), (oh, ow), _live_taps(h, w, r, s, st, pd), gn.adjoint_row_blocks(n * oh * ow, m.out_channels))
           for m, name, h, w, r, s, st, pd, oh, ow in layers]
    assert got == lit["convs"]
    assert gn.linear_geometry(model) == lit["linears"]
    assert gn.last_map(model, x) == lit["last"]
    assert sum(k for _, k in gn.named_sizes(model)) == lit["n"]
    leaves = [m for m in model.modules() if not list(m.children())]
    pools = []
    for a, b in zip(leaves, leaves[1:] + [None]):  # per convolution: the pool behind it (behind its ReLU), or None
        if isinstance(a, nn.Conv2d):
            pools.append(None)
        elif isinstance(a, nn.MaxPool2d):
            pools[-1] = _pool_tuple(a)
    assert pools == lit["pools"]
    rows, hw, c = lit["last"]
    assert lit["linears"][0][0] == hw * c and rows == n
    assert [b[0] for b in lit["linears"][1:]] == [a[1] for a in lit["linears"][:-1]]
    with torch.no_grad():
        assert tuple(model(x).shape) == (n, gn.TAILS[case]["classes"]) == (n, lit["linears"][-1][1])


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_the_librarys_dense_plan_is_the_restated_rule(case):
    """``hf_dense_plan`` (host arithmetic) counts the slabs ``geometry_nets.dense_plan`` restates."""
    lib = _lib.load()
    rows = gn.TAIL_GEOMETRY[case]["last"][0]
    for c_in, c_out, s_t, s_d, _, _ in gn.TAIL_GEOMETRY[case]["linears"]:
        st, sd = _lib.c_int(), _lib.c_int()
        assert lib.hf_dense_plan(rows, c_in, c_out, st, sd) == 0
        assert (st.value, sd.value) == (s_t, s_d) == gn.dense_plan(c_in, c_out), (c_in, c_out)


def test_the_tail_cases_reach_what_they_are_named_for():
    G = gn.TAIL_GEOMETRY
    # data-gradient slabs that are summed: by hf_unflatten_slabs_nhwc (a FIRST tail layer) and by the layer in front
    assert G["tail_wide_first"]["linears"][0][3] == 3 and G["tail_wide_first"]["linears"][1][3] == 2
    assert G["tail_col_map"]["linears"][0][3] == 2
    assert [(a[2], a[3]) for a in G["tail_wide_first"]["linears"]] == [(20, 3), (3, 2), (2, 1)]
    assert [(a[2], a[3]) for a in G["tail_col_map"]["linears"]] == [(1, 2), (2, 1)]
    # operands off the 16-byte grid, row pitches that are no multiple of 4
    c_in, _, _, _, w_off, b_off = G["tail_rect_pooled"]["linears"][1]
    assert (w_off, w_off % 4, c_in % 4) == (2057, 1, 1) and b_off % 4 == 0
    c_in, _, _, _, w_off, b_off = G["tail_wide_first"]["linears"][1]
    assert (w_off, w_off % 4, c_in % 4, b_off) == (88630, 2, 2, None)
    assert G["tail_wide_first"]["linears"][2][5] == 91105 and 91105 % 4 == 1
    # two flatten tiles with a partial last one, both ways
    _, hw, c = G["tail_wide_first"]["last"]
    for d in (hw, c):
        assert -(-d // gn.FLATTEN_TILE) == 2 and d % gn.FLATTEN_TILE
    assert G["tail_wide_first"]["pools"] == [None] and len(G["tail_wide_first"]["linears"]) == 3
    # the last map pooled and non-square; a Dropout leaf behind Flatten
    assert G["tail_rect_pooled"]["pools"][-1] is not None and G["tail_rect_pooled"]["last"] == (3, 2 * 3, 12)
    model, _ = gn.make("tail_rect_pooled")
    kinds = [type(m) for m in model.net]
    assert kinds.index(nn.Dropout) == kinds.index(nn.Flatten) + 1 and not model.training
    # one pixel, one sample, no ReLU behind the last convolution, four input channels (no im2col)
    assert G["tail_pixel"]["last"][:2] == (1, 1)
    model, _ = gn.make("tail_pixel")
    kinds = [type(m) for m in model.net]
    assert kinds[kinds.index(nn.Flatten) - 1] is nn.Conv2d and model.net[0].in_channels == 4
    assert G["tail_rows_256"]["last"][0] == 256
    # a one-column map: the outer kernel columns of both convolutions meet only padding
    assert [a[3] for a in G["tail_col_map"]["convs"]] == [0b010010010] * 2


def _differing_positions(model, x):
    p32 = gn.pool_positions(copy.deepcopy(model), x)
    p64 = gn.pool_positions(copy.deepcopy(model).double(), x.double())
    assert len(p32) == len(p64)
    return sum(int((a != b).sum()) for a, b in zip(p32, p64))


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_tail_fp32_and_float64_take_the_same_relu_decisions_and_pool_positions(case):
    model, batches = gn.make(case)
    assert len(gn.pool_positions(model, batches[0][0])) == sum(p is not None for p in gn.TAIL_GEOMETRY[case]["pools"])
    for x, t in batches:
        assert _differing_decisions(model, x) == 0, case
        assert _differing_positions(model, x) == 0, case
        # ... and the reference on the fp32 pass's decisions is the reference on its own, with nothing replayed
        ref = gn.Reference(model, x, t, masks=gn.own_masks(model, x), pools=gn.pool_positions(model, x))
        assert ref.flips == [0] and abs(ref.loss() - gn.Reference(model, x, t).loss()) == 0.0


@pytest.mark.parametrize("case", ["tail_rect_pooled", "tail_wide_first"])
def test_the_tail_reference_is_the_explicit_ggn(case):
    """``J^T H J v`` of an explicitly built Jacobian, symmetric; gradient and diagonal Fisher by the same Jacobian."""
    model, batches = gn.make(case)
    x, t = batches[0]
    ref = gn.Reference(model, x, t)
    n = ref.gradient().numel()
    assert n == gn.TAIL_GEOMETRY[case]["n"]
    J = _flat_jacobian(ref.model, ref.x)
    H = torch.autograd.functional.hessian(lambda z: nn.functional.cross_entropy(z.view_as(ref.out), ref.t),
                                          ref.out.detach().reshape(-1))
    u, v = gn.probe(n, 1).double(), gn.probe(n, 2).double()
    gv, gu = ref.ggn(v), ref.ggn(u)
    want = J.t() @ (H @ (J @ v))
    assert float((gv - want).abs().max() / want.abs().max()) < 1e-10
    a, b = float(u @ gv), float(v @ gu)
    assert abs(a - b) <= 1e-12 * abs(a)
    dl = torch.autograd.grad(nn.functional.cross_entropy(z := ref.out.detach().clone().requires_grad_(True), ref.t), z)[0]
    assert float((ref.gradient() - J.t() @ dl.reshape(-1)).abs().max() / ref.gradient().abs().max()) < 1e-10
    # diagonal Fisher: sample i's gradient is J_i^T (d loss_i / d logits_i) -- rows of the same Jacobian, unaveraged
    rows, classes = ref.out.shape
    gi = torch.einsum("ikp,ik->ip", J.view(rows, classes, n), dl * rows)
    d = ref.diag_ef()
    assert float((d - (gi ** 2).sum(0) / rows).abs().max() / d.abs().max()) < 1e-12
    assert float(ref.loss()) > 0 and bool((d >= 0).all())


def _misordered_twin(order):
    """``tail_rect_pooled`` as an engine would compute it that flattened the last map's features in ``order`` instead of
    (c, h, w) and read the first Linear's weight in place: the net whose first tail weight has its columns permuted;
    returns it with the maps of a flat vector into its layout and back."""
    model, batches = gn.make("tail_rect_pooled")
    _, hw, c = gn.TAIL_GEOMETRY["tail_rect_pooled"]["last"]
    h, w = 2, 3
    assert h * w == hw
    true = torch.arange(c * h * w).view(c, h, w)
    perm = true.permute(*["chw".index(a) for a in order]).reshape(-1)  # wrong flat position j holds true feature perm[j]
    inv = torch.argsort(perm)
    assert not torch.equal(perm, torch.arange(c * hw))
    first = next(m for m in model.modules() if isinstance(m, nn.Linear))
    twin = copy.deepcopy(model)
    with torch.no_grad():
        next(m for m in twin.modules() if isinstance(m, nn.Linear)).weight.copy_(first.weight[:, inv])
    off = gn.TAIL_GEOMETRY["tail_rect_pooled"]["linears"][0][4]

    def columns(vec, index):
        out = vec.clone()
        out[off:off + first.weight.numel()] = vec[off:off + first.weight.numel()].view_as(first.weight)[:, index].reshape(-1)
        return out

    return model, twin, batches[0], (lambda vec: columns(vec, inv)), (lambda vec: columns(vec, perm))


@pytest.mark.parametrize("order", ["cwh", "hwc"])
def test_the_measure_sees_a_wrong_feature_order(order):
    """The analogue of the transposed twin for the ``nn.Flatten`` boundary: with the columns of the first tail weight
    and of the vector permuted as if the features ran (c, w, h) or (h, w, c), the reference product is far from the
    true one -- an engine that flattened in another order than (c, h, w) cannot pass for the right one."""
    model, twin, (x, t), into, back = _misordered_twin(order)
    ref, ref_p = gn.Reference(model, x, t), gn.Reference(twin, x, t)
    n = ref.gradient().numel()
    v = gn.probe(n, 3).double()
    assert torch.equal(back(into(v)), v)
    true = ref.ggn(v)
    wrong = back(ref_p.ggn(into(v)))
    assert float((wrong - true).abs().max() / true.abs().max()) > 1e-2
    assert float((ref_p.ggn(v) - true).abs().max() / true.abs().max()) > 1e-2  # (nor without the way back)
    off = 0
    for name, k in gn.named_sizes(model):  # every tensor: the tail's and the convolutions' in front of it
        a, b = wrong[off:off + k], true[off:off + k]
        assert float((a - b).abs().max() / b.abs().max()) > 1e-2, name
        off += k
    assert gn.scalar_error(ref_p.loss(), ref.loss()) > 1e-2
    g = back(ref_p.gradient())
    assert float((g - ref.gradient()).abs().max() / ref.gradient().abs().max()) > 1e-2


def test_replayed_pool_positions_are_bounded():
    """A replayed position may leave its window's own maximum only next to a tie, and counts as a differing decision."""
    model, batches = gn.make("tail_rect_pooled")
    x, t = batches[0]
    pools = gn.pool_positions(copy.deepcopy(model).double(), x.double())
    assert [tuple(p.shape) for p in pools] == [(3, 8, 4, 3), (3, 12, 2, 3)]
    assert gn.Reference(model, x, t, pools=pools).flips == [0]
    far = [p.clone() for p in pools]
    own = far[1][0, 0, 0, 0].item()  # (the second pool: windows of two rows, one column of a 4x3 map)
    far[1][0, 0, 0, 0] = 3 - own if own in (0, 3) else own  # the window's other entry
    values = gn.relu_inputs(copy.deepcopy(model).double(), x.double())[1].clamp_min(0)[0, 0].reshape(-1)
    assert far[1][0, 0, 0, 0] != own and values[own] - values[3 - own] > 1e-3 * values.max()
    with pytest.raises(AssertionError, match="far from the window's maximum"):
        gn.Reference(model, x, t, pools=far)
    with pytest.raises(AssertionError):  # (a position outside the map is no decision at all)
        gn.Reference(model, x, t, pools=[pools[0], pools[1] + 12])


# ---- the BatchNorm plain stacks (``geometry_nets.BN_STACKS``) ------------------------------------------------------
def test_the_bn_case_list_is_the_issues():
    assert gn.BN_CASES == list(gn.BN_GEOMETRY) == ["bn_rect_pooled", "bn_col_map", "bn_row_map", "bn_wide_rows",
                                                   "bn_pixel_one", "bn_tail_rect"]
    assert not set(gn.BN_CASES) & (set(gn.CASES) | set(gn.TAIL_CASES))
    assert gn.BN_TRAIN_CASES == [c for c in gn.BN_CASES if c != "bn_pixel_one"]
    assert gn.BN_HESSIAN_CASES == [c for c in gn.BN_CASES if c != "bn_tail_rect"]
    assert gn.BN_CAPTURED_CASES == [("bn_rect_pooled", True), ("bn_wide_rows", False)]
    assert [gn.BN_STACKS[c]["x"] for c in gn.BN_CASES] == [(3, 3, 7, 10), (5, 1, 12, 1), (5, 1, 1, 12), (4, 1, 12, 10),
                                                           (1, 4, 4, 4), (3, 3, 9, 7)]
    assert [gn.BN_STACKS[c]["classes"] for c in gn.BN_CASES] == [12, 8, 8, 16, 8, 7]


def _units(model):
    """Per convolution in module order: (conv, BatchNorm or None, ReLU?, MaxPool2d or None) of the leaves behind it, up
    to ``nn.Flatten``."""
    units = []
    for m in (m for m in model.modules() if not list(m.children())):
        if isinstance(m, nn.Conv2d):
            units.append([m, None, False, None])
        elif isinstance(m, nn.BatchNorm2d):
            units[-1][1] = m
        elif isinstance(m, nn.ReLU):
            units[-1][2] = True
        elif isinstance(m, nn.MaxPool2d):
            units[-1][3] = m
        elif isinstance(m, nn.Flatten):
            break
    return units


@pytest.mark.parametrize("case", gn.BN_CASES)
def test_bn_map_sizes_live_taps_row_blocks_and_pools(case):
    model, x, layers = _layers(case)
    lit, n = gn.BN_GEOMETRY[case], x.shape[0]
    units = _units(model)
    assert [u[0] for u in units] == [m for m, *_ in layers]
    pooled = {}
    hooks = [u[3].register_forward_hook(lambda m, i, o, key=u[0]: pooled.__setitem__(key, tuple(o.shape[2:])))
             for u in units if u[3] is not None]
    with torch.no_grad():
        out = model(x)
    for h in hooks:
        h.remove()
    got = [(name, (h, w), (oh, ow), _live_taps(h, w, r, s, st, pd), gn.adjoint_row_blocks(n * oh * ow, m.out_channels),
            None if u[3] is None else _pool_tuple(u[3]), pooled.get(m))
           for (m, name, h, w, r, s, st, pd, oh, ow), u in zip(layers, units)]
    assert got == lit["convs"]
    assert sum(k for _, k in gn.named_sizes(model)) == lit["n"]
    assert tuple(out.shape) == (n, gn.BN_STACKS[case]["classes"])
    assert (layers[0][0].in_channels < 4) == lit["im2col"]
    # every convolution but a global-average-pool net's last one is a BatchNorm unit without a bias
    bn = [u[1] is not None for u in units]
    assert bn == ([True] * len(units) if case == "bn_tail_rect" else [True] * (len(units) - 1) + [False])
    assert all((u[0].bias is None) == (u[1] is not None) for u in units)
    assert all(u[1].eps == 0.1 and float(u[1].running_mean.abs().max()) > 0 for u in units if u[1] is not None)


def test_the_bn_cases_reach_what_they_are_named_for():
    G = {case: gn.BN_GEOMETRY[case]["convs"] for case in gn.BN_CASES}
    # every pair of axis parameters unequal somewhere behind a BatchNorm; a padded pool; a pooled unit without ReLU
    model, _ = gn.make("bn_rect_pooled")
    units = _units(model)
    convs = [u[0] for u in units]
    assert [tuple(c.kernel_size) for c in convs] == [(1, 3), (3, 1), (3, 3), (1, 1)]
    assert tuple(convs[1].stride) == (2, 1) and [tuple(c.padding) for c in convs[:2]] == [(0, 1), (1, 0)]
    assert [g[5] for g in G["bn_rect_pooled"]] == [(3, 2, 2, 1, 1, 0), (1, 2, 1, 2, 0, 0), None, None]
    kh, kw, sh, sw, ph, pw = G["bn_rect_pooled"][0][5]
    assert kh != kw and sh != sw and ph != pw and G["bn_rect_pooled"][0][1][0] != G["bn_rect_pooled"][0][1][1]
    assert [(u[2], u[3] is not None) for u in units] == [(True, True), (False, True), (True, False), (False, False)]
    assert [(g[1], g[2], g[6]) for g in G["bn_rect_pooled"][:3]] == [((7, 10), (7, 10), (4, 9)), ((4, 9), (2, 9), (2, 4)),
                                                                    ((2, 4), (2, 4), None)]
    assert G["bn_rect_pooled"][0][4] == 2 and gn.BN_GEOMETRY["bn_rect_pooled"]["im2col"]
    # dead kernel columns / rows under a BatchNorm; statistics over 15 rows
    assert [g[3] for g in G["bn_col_map"]] == [0b010010010, 0b010010010, 0]
    assert [g[3] for g in G["bn_row_map"]] == [0b000111000, 0b000111000, 0]
    assert 5 * G["bn_col_map"][1][2][0] * G["bn_col_map"][1][2][1] == 15
    # many row blocks with an uneven row stride, ph != pw, 65 quads per row
    (_, _, o0, _, rb0, p0, _), (_, _, o1, _, rb1, p1, _) = G["bn_wide_rows"][:2]
    assert (rb0, rb1) == (60, 40) and -(-4 * o0[0] * o0[1] // rb0) == 8 and 132 // 4 == 33 and 260 // 4 == 65
    assert p1 == (2, 3, 2, 2, 0, 1) and p0 == (3, 3, 2, 2, 1, 1)
    # batch 1, a 1x1 map, no im2col
    assert gn.BN_STACKS["bn_pixel_one"]["x"][0] == 1 and G["bn_pixel_one"][1][2] == (1, 1)
    assert not gn.BN_GEOMETRY["bn_pixel_one"]["im2col"]
    # pooled BatchNorm units in front of a tail, the last map 2x4
    assert [g[6] for g in G["bn_tail_rect"]] == [(4, 4), (2, 4)] and G["bn_tail_rect"][1][5] == (2, 1, 2, 1, 0, 0)
    model, batches = gn.make("bn_tail_rect")
    assert gn.last_map(model, batches[0][0]) == (3, 8, 12) and gn.linear_geometry(model)[0][:2] == (96, 21)


@pytest.mark.parametrize("case", gn.BN_CASES)
def test_the_planner_accepts_every_bn_layer_in_every_direction(case):
    plan = _lib.load().hf_conv2d_nhwc_plan
    model, x, layers = _layers(case)
    n = x.shape[0]
    for i, (m, name, h, w, r, s, st, pd, oh, ow) in enumerate(layers):
        c, k = m.in_channels, m.out_channels
        if i == 0 and gn.BN_GEOMETRY[case]["im2col"]:
            j = c * r * s
            asked = [(0, n * oh * ow, 1, 1, j, k, 1, 1, 1, 1, 0, 0), (2, n * oh * ow, 1, 1, -(-j // 4) * 4, k, 1, 1, 1, 1, 0, 0)]
        else:
            asked = [(d, n, h, w, cc, k, r, s, st[0], st[1], pd[0], pd[1]) for d, cc in ((0, c), (0, 2 * c), (1, c), (2, c))]
        for args in asked:
            assert plan(*args, 0) >= 1, (name, args)


@pytest.mark.parametrize("case", gn.BN_CASES)
def test_bn_fp32_and_float64_take_the_same_relu_decisions_and_pool_positions(case):
    """In eval and in train mode, on both batches: nothing to replay (0 of the ``MAX_FLIPS`` = 4 the cap allows)."""
    assert (gn.MAX_FLIPS, gn.MARGIN) == (4, 1e-5)
    for train in ([False, True] if case in gn.BN_TRAIN_CASES else [False]):
        model, batches = gn.make(case, train)
        assert model.training == train
        assert len(gn.pool_positions(copy.deepcopy(model), batches[0][0])) == sum(
            g[5] is not None for g in gn.BN_GEOMETRY[case]["convs"])
        for x, t in batches:
            assert _differing_decisions(model, x) == 0, (case, train)
            assert _differing_positions(model, x) == 0, (case, train)
            own = copy.deepcopy(model)
            ref = gn.Reference(model, x, t, masks=gn.own_masks(own, x), pools=gn.pool_positions(own, x))
            assert ref.flips == [0] and abs(ref.loss() - gn.Reference(model, x, t).loss()) == 0.0
        # (make()'s model is untouched by all of the above: every pass ran on a copy)
        assert all(int(m.num_batches_tracked) == 0 for m in model.modules() if isinstance(m, nn.BatchNorm2d))


@pytest.mark.parametrize("case, train", [("bn_rect_pooled", False), ("bn_rect_pooled", True), ("bn_col_map", True),
                                         ("bn_tail_rect", False)])
def test_the_bn_reference_is_the_explicit_ggn_and_its_diagonal_the_summed_outer_products(case, train):
    """``J^T H J v`` of an explicitly built Jacobian (train mode: the Jacobian of the batch's pass, batch statistics
    included), symmetric; the gradient by the same Jacobian; eval mode: the diagonal Fisher from its per-sample rows."""
    model, batches = gn.make(case, train)
    x, t = batches[0]
    ref = gn.Reference(model, x, t)
    n = ref.gradient().numel()
    assert n == gn.BN_GEOMETRY[case]["n"] and ref.model.training == train
    J = _flat_jacobian(ref.model, ref.x)
    H = torch.autograd.functional.hessian(lambda z: nn.functional.cross_entropy(z.view_as(ref.out), ref.t),
                                          ref.out.detach().reshape(-1))
    u, v = gn.probe(n, 1).double(), gn.probe(n, 2).double()
    gv, gu = ref.ggn(v), ref.ggn(u)
    want = J.t() @ (H @ (J @ v))
    assert float((gv - want).abs().max() / want.abs().max()) < 1e-10
    a, b = float(u @ gv), float(v @ gu)
    assert abs(a - b) <= 1e-12 * abs(a)
    dl = torch.autograd.grad(nn.functional.cross_entropy(z := ref.out.detach().clone().requires_grad_(True), ref.t), z)[0]
    assert float((ref.gradient() - J.t() @ dl.reshape(-1)).abs().max() / ref.gradient().abs().max()) < 1e-10
    if not train:
        rows, classes = ref.out.shape
        gi = torch.einsum("ikp,ik->ip", J.view(rows, classes, n), dl * rows)
        d = ref.diag_ef()
        assert float((d - (gi ** 2).sum(0) / rows).abs().max() / d.abs().max()) < 1e-12
        assert bool((d >= 0).all())
    assert float(ref.loss()) > 0


def _bn_transposed_twin(train):
    """``bn_col_map``'s net holding ``bn_row_map``'s parameters and BatchNorm state with every kernel transposed."""
    row, rb = gn.make("bn_row_map", train)
    col, _ = gn.make("bn_col_map", train)
    col.load_state_dict({k: (v.transpose(2, 3).contiguous() if v.dim() == 4 else v.clone())
                         for k, v in row.state_dict().items()})
    x, t = rb[0]
    return row, col, x, t


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_bn_row_map_and_bn_col_map_are_transposes_and_the_reference_tells_them_apart(train):
    assert gn.BN_STACKS["bn_row_map"]["x"] == gn.BN_STACKS["bn_col_map"]["x"][:2] + gn.BN_STACKS["bn_col_map"]["x"][:1:-1]
    for a, b in zip(gn.BN_GEOMETRY["bn_row_map"]["convs"], gn.BN_GEOMETRY["bn_col_map"]["convs"]):
        flip = lambda hw: None if hw is None else hw[::-1]  # noqa: E731
        pool = None if a[5] is None else tuple(a[5][i ^ 1] for i in range(6))
        assert (a[0], flip(a[1]), flip(a[2]), a[4], pool, flip(a[6])) == (b[0], b[1], b[2], b[4], b[5], b[6])
    row, col, x, t = _bn_transposed_twin(train)
    ref_r = gn.Reference(row, x, t)
    ref_c = gn.Reference(col, x.transpose(2, 3).contiguous(), t)
    assert tuple(ref_c.x.shape) == gn.BN_STACKS["bn_col_map"]["x"]
    n = ref_r.gradient().numel()
    v = gn.probe(n, 3).double()
    got = ref_c.ggn(_transpose_kernels(v, row))
    want = _transpose_kernels(ref_r.ggn(v), row)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    assert abs(ref_r.loss() - ref_c.loss()) < 1e-13
    if train:
        assert all(float((a.double() - b.double()).abs().max()) < 1e-13
                   for a, b in zip(ref_r.running().values(), ref_c.running().values()))
    plain = ref_c.ggn(v)
    assert float((plain - ref_r.ggn(v)).abs().max() / want.abs().max()) > 1e-2
    with pytest.raises(AssertionError, match="exactly zero"):  # (dead kernel ROWS of one are live in the other)
        gn.per_tensor_errors(plain, ref_r.ggn(v), gn.named_sizes(row))


def _shift_blocks(model, sizes):
    names = [name for name, _ in sizes]
    for bn in (name for name, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)):
        i = names.index(bn + ".bias")
        yield bn + ".bias", sum(k for _, k in sizes[:i]), sizes[i][1]


@pytest.mark.parametrize("case", gn.BN_CASES)
def test_the_per_tensor_measure_sees_one_batchnorm_shift_off_by_a_thousandth(case):
    """One BatchNorm shift's block wrong by 1e-3 of ITSELF.  The per-tensor measure reports 1e-3 for that tensor and 0 for
    every other one, whatever the quantity.  The whole-vector max-norm of ``stack_harness.rel`` reports 1e-3 times the
    block's share of the vector's largest entry (printed): of the diagonal Fisher at least 50 times less for some shift of
    every case, and on ``bn_wide_rows`` 1.5e-6 -- below the 2e-6 that ``stack_harness.check_point`` allows that quantity:
    such a block passes there entirely unseen.  (Of a GGN product the shifts' shares are 2 to 20 per cent.)"""
    model, batches = gn.make(case)
    ref = gn.Reference(model, *batches[0])
    sizes = gn.named_sizes(model)
    quantities = {"ggn": ref.ggn(gn.probe(sum(k for _, k in sizes), 11).double()), "diag_ef": ref.diag_ef()}
    whole = {q: [] for q in quantities}
    for q, want in quantities.items():
        for name, off, k in _shift_blocks(model, sizes):
            got = want.clone()
            got[off:off + k] *= 1.0 + 1e-3
            errs = gn.per_tensor_errors(got, want, sizes)
            assert abs(errs[name] - 1e-3) < 1e-9 and all(e == 0.0 for other, e in errs.items() if other != name)
            whole[q].append(float((got - want).abs().max() / want.abs().max()))
    print(case, {q: [f"{e:.1e}" for e in v] for q, v in whole.items()})
    assert max(whole["ggn"] + whole["diag_ef"]) <= 1e-3 * (1 + 1e-9) and min(whole["diag_ef"]) < 1e-3 / 50
    if case == "bn_wide_rows":
        assert min(whole["diag_ef"]) < 2e-6
