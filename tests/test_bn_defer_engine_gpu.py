"""GPU: the engine with the BatchNorm parameter sums taken off the adjoint chain (``HF_BN_SUMS_DEFER``, default on) against
the same engine with today's fused launches (``=0``), bit for bit, on small ResNet-style nets: stem + max-pool and residual
blocks, one of them with a downsample branch.

``small``: 8x8 inputs, batch 8, 8 / 16 channels (two blocks) -- at these sizes the stem is the one unit on the row-major
kernel.  ``wide``: 8x8 inputs, batch 16, 32 / 64 channels and a third block on a 1x1 map -- the stem, an identity block, a
downsample block whose two adjoints share one launch (all deferred), and units with ``rb == 1`` that keep today's launch;
its dead taps give the compact layout ``local_compact`` needs."""

import numpy as np
import pack_refs as pr
import pytest
import torch

from engine_nets import DEV, build

pytestmark = pytest.mark.gpu


def products(op):
    """(local, gradient, local_compact or None) of fixed vectors, cloned."""
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    res = [op.local(v).clone(), op.gradient().clone()]
    assert torch.equal(op.local(v), res[0]), "the product is not repeatable"
    lay = None if op.hessian else op.compact_layout()
    if lay is not None:
        idx = torch.from_numpy(np.asarray(pr.live_index(lay["table"]))).to(DEV)
        vz = torch.zeros_like(v)
        vz[idx] = v[idx]
        out = torch.full((lay["n_live"],), float("nan"), device=DEV)
        op.local_compact(vz[idx].contiguous(), out)
        assert torch.equal(out, op.local(vz)[idx]), "local_compact(gather(v)) != gather(local(v))"
        res.append(out.clone())
    else:
        res.append(None)
    return res


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("net,pattern", [("small", "plain"), ("small", "stem"), ("small", "scale_shift"),
                                         ("wide", "plain"), ("wide", "stem"), ("wide", "scale_shift")])
def test_deferred_sums_equal_the_fused_launches_bit_for_bit(net, pattern, monkeypatch):
    """``local``, ``gradient()`` and ``local_compact`` with HF_BN_SUMS_DEFER=1 (the default) against =0."""
    monkeypatch.setenv("HF_BN_SUMS_DEFER", "0")
    fused = build(net, pattern)
    rep0 = fused.bn_adjoint_report()
    assert rep0["elementwise"] == [] and rep0["deferred"] == []
    want = products(fused)
    assert fused.bn_adjoint_report()["sums_launches"] == 0
    monkeypatch.setenv("HF_BN_SUMS_DEFER", "1")
    op = build(net, pattern)
    rep = op.bn_adjoint_report()
    live_rows = [u.name for u in op.units if u.rb > 1 and not u.dead]
    assert rep["elementwise"] == live_rows
    no_sums = [u.name for u in op.units if u.pg is None and u.pb is None]
    assert sorted(rep["deferred"]) == sorted(n for n in live_rows if n not in no_sums)
    if net == "wide":
        assert len(rep["deferred"]) >= (3 if pattern == "stem" else 4), rep
        assert op.compact_layout() is not None and want[2] is not None
        assert any(u.rb == 1 for u in op.units), "no unit keeps the one-block launch"
    if pattern == "plain":
        assert "stem" in rep["deferred"]
    before = rep["sums_launches"]
    got = products(op)
    for name, g, w in zip(("local", "gradient", "local_compact"), got, want):
        assert (g is None) == (w is None)
        assert g is None or same_bits(g, w), f"{name}: deferred sums change the result"
    # one sums launch per sweep (every deferred unit is one contiguous range of the table)
    sweeps = 5 if got[2] is not None else 3
    assert op.bn_adjoint_report()["sums_launches"] - before == (sweeps if rep["deferred"] else 0)
    assert not op._sums_pending


# the parameter in front of which the arena stops being 16-byte aligned -> per sweep of the ``wide`` net: (sums launches,
# adjoint launches planned as elementwise that take the fused launch).  Its sweep has five such launches: block 1's second
# unit, block 1's first unit and its downsample branch as a pair, block 0's two units, the stem; block 2 (rb == 1) has none.
ARENA_CASES = {
    "conv1.weight": (0, 5),                  # every scale misaligned: nothing is deferred at run time
    "layers.1.conv1.weight": (1, 2),         # block 1 misaligned; block 0 and the stem are one range of the table
    "layers.1.downsample.1.weight": (2, 1),  # the pair's second scale alone: two ranges, one on each side of the pair
}


@pytest.mark.parametrize("where", list(ARENA_CASES))
def test_scale_bound_into_an_arena_off_a_16_byte_boundary_takes_the_fused_launch(where, monkeypatch):
    """``utils.ParameterArena`` binds the parameters at unpadded offsets: behind a parameter with 10 entries a BatchNorm
    scale sits 8 bytes off a 16-byte boundary.  Such a unit keeps the fused launch (scalar loads of the scale), decided at
    call time, its sums are not pending, and the products equal HF_BN_SUMS_DEFER=0 bit for bit."""
    launches, fallbacks = ARENA_CASES[where]
    monkeypatch.setenv("HF_BN_SUMS_DEFER", "0")
    want = products(build("wide", arena_at=where))
    monkeypatch.setenv("HF_BN_SUMS_DEFER", "1")
    op = build("wide", arena_at=where)
    rep = op.bn_adjoint_report()
    split = [u for u in op.units if u.split]
    assert len(rep["deferred"]) == 6 and len(split) == 6, rep
    off = [u.name for u in split if u.scale.data_ptr() % 16]
    assert off and all(u.cout % 4 == 0 and u.rb > 1 for u in split)
    assert (len(off) == len(split)) == (launches == 0)
    got = products(op)
    for name, g, w in zip(("local", "gradient", "local_compact"), got, want):
        assert (g is None) == (w is None)
        assert g is None or same_bits(g, w), f"{name}: {off} misaligned"
    after = op.bn_adjoint_report()
    sweeps = 5 if got[2] is not None else 3
    assert after["sums_launches"] - rep["sums_launches"] == sweeps * launches
    assert after["fused_fallbacks"] - rep["fused_fallbacks"] == sweeps * fallbacks
    assert not op._sums_pending


def test_captured_and_replayed_product_equals_the_eager_one():
    op = build("wide")
    assert op.bn_adjoint_report()["deferred"]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out = torch.empty(op.n, device=DEV)
    eager = op.local(v).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op.local(v, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op.local(v, out=out)
    for _ in range(2):
        out.fill_(float("nan"))
        for u in op.units:  # (the replay must recompute the deferred sums, not find them)
            u.gw.fill_(float("nan"))
            u.gb.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager)
    v2 = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    want2 = op.local(v2).clone()
    v.copy_(v2)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want2)


@pytest.mark.parametrize("kind", ["train", "hessian"])
def test_train_mode_and_hessian_builds_launch_no_deferred_kernel(kind, monkeypatch):
    """By the engine's own report: no unit takes the elementwise launch, no table, no sums launch after products and a
    gradient sweep."""
    monkeypatch.setenv("HF_ENGINE_VERIFY", "never")  # (the first-use check against autograd is not what is tested here)
    op = build("wide", train=kind == "train", hessian=kind == "hessian")
    rep = op.bn_adjoint_report()
    assert rep["elementwise"] == [] and rep["deferred"] == [] and op._sums_tab is None
    assert all(not u.split and not u.defer for u in op.units)
    products(op)
    assert op.bn_adjoint_report()["sums_launches"] == 0
