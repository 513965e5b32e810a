"""GPU: the same buffers rewritten launch after launch.  Inside one PCG iteration every launch reads what the launch
before it wrote -- split-K slabs, activation tangents and cotangents, partial rows, the parameter-sized vectors -- and
the next iteration writes the same addresses again.  The exact single-launch suites cannot see a consumer that reads a
stale line there, whatever the cache policy of the producer's stores (``chain_store`` in ``csrc/hf_store.h``): here a
product captured as a graph is replayed 24 times, each time on a fresh seeded ``v`` copied into the static input, and
every result must equal the eager product of the same ``v`` bit for bit; likewise a graph-replayed ``cg()`` against the
eager one."""

import warnings

import numpy as np
import pack_refs as pr
import pytest
import torch

import pytorchhessianfree_amd as hf
from engine_nets import DEV, build
from pytorchhessianfree_amd import curvature

pytestmark = pytest.mark.gpu

REPLAYS = 24


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def capture(product):
    """``product()`` once on a side stream (argument tables, lazy allocations), then captured."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        product()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        product()
    return graph


def replay_against_eager(graph, v_static, out, eager, fresh):
    """24 replays on fresh vectors, then the first vector again: every result is the eager product's, and two replays
    of one ``v`` agree."""
    first = None
    for k in range(REPLAYS + 1):
        v = fresh(k % REPLAYS)
        want = eager(v).clone()
        v_static.copy_(v)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want), f"replay {k} differs from the eager product of the same v"
        if k == 0:
            first = out.clone()
    assert same_bits(out, first), "two replays of the same v differ"


@pytest.mark.parametrize("net,train", [("small", False), ("wide", False), ("wide", True)])
def test_replayed_product_equals_the_eager_product_of_every_fresh_vector(net, train, monkeypatch):
    if train:
        monkeypatch.setenv("HF_ENGINE_VERIFY", "never")  # (the first-use check against autograd is not what is tested)
    op = build(net, train=train)
    v_static = torch.zeros(op.n, device=DEV)
    out = torch.empty(op.n, device=DEV)
    graph = capture(lambda: op.local(v_static, out=out))

    def fresh(k):
        return torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(100 + k))

    replay_against_eager(graph, v_static, out, lambda v: op.local(v), fresh)


def test_replayed_compact_product_equals_the_eager_compact_product():
    op = build("wide")
    lay = op.compact_layout()
    assert lay is not None and lay["n_live"] < op.n
    idx = torch.from_numpy(np.asarray(pr.live_index(lay["table"]))).to(DEV)
    vc_static = torch.zeros(lay["n_live"], device=DEV)
    out = torch.empty(lay["n_live"], device=DEV)
    graph = capture(lambda: op.local_compact(vc_static, out))

    def fresh(k):
        return torch.randn(lay["n_live"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(200 + k))

    def eager(vc):
        res = torch.full((lay["n_live"],), float("nan"), device=DEV)
        op.local_compact(vc.contiguous(), res)
        return res

    replay_against_eager(graph, vc_static, out, eager, fresh)
    # and the compact product is the compact image of the full one (dead entries of v zero)
    vc = fresh(0)
    vz = torch.zeros(op.n, device=DEV)
    vz[idx] = vc
    assert same_bits(eager(vc), op.local(vz)[idx])


class LowRank:
    """``B v = d * v + U (U^T v)`` in fp64, rounded once (the system of ``__graft_entry__.smoke()``), with what
    ``curvature.GraphedOperator`` asks of an operator."""

    group = None

    def __init__(self, n=20011, rank=8):
        g = torch.Generator().manual_seed(0)
        self.n = n
        self.U = (torch.randn(n, rank, generator=g) / rank**0.5).double().to(DEV)
        self.d = torch.rand(n, generator=g).double().to(DEV)
        self.b = torch.randn(n, generator=g).to(DEV)
        self.diag = (self.d + (self.U * self.U).sum(1)).float()
        self.params = [self.b]

    def local(self, v, out=None):
        v64 = v.double()
        res = (self.d * v64 + self.U @ (self.U.T @ v64)).to(v.dtype)
        if out is None:
            return res
        return out.copy_(res)

    __call__ = local


def test_graph_replayed_cg_iterates_equal_the_eager_solve_bit_for_bit():
    """24 PCG iterations: product -> K1 -> K2 -> K3 as one graph launch per iteration against separate eager launches.
    x, r and p are rewritten in every iteration; every iterate is compared."""
    lam, iters = 0.5, REPLAYS
    low = LowRank()
    M = hf.DiagonalPreconditioner(low.diag, lam)
    kw = dict(max_iter=iters, tol=0.0, store_x_at_iters=list(range(iters + 1)))  # (ends by the iteration count)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ex, _, ereason = hf.cg(hf.DampedCurvature(low, lam), low.b, M=M, **kw)
        graphed = curvature.GraphedOperator(lambda: low, params=None)
        assert graphed.raw_graph() is not None
        gx, _, greason = hf.cg(hf.DampedCurvature(graphed, lam), low.b, M=M, **kw)
        assert graphed.__dict__.get("_iteration_graphs"), "cg() did not fuse the product into its iteration graph"
    assert ereason == greason and len(ex) == len(gx) == iters + 1
    for i, (a, b) in enumerate(zip(ex, gx)):
        assert a is not None and b is not None
        assert same_bits(a, b), f"iterate {i} differs"
