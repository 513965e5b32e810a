"""What the engine-level tests of the plain-stack engine (``engine/plain.py``) share -- ``test_pooled_stack_engine_gpu.py``,
``test_convfc_engine_gpu.py``, ``test_convbn_engine_gpu.py``, ``test_convbn_train_engine_gpu.py`` --, one copy of each:

* ``engine``: the test problem built on the CPU, prepared on the GPU, and its operator;
* ``decisions`` / ``replay`` / ``float64_twin``: float64 autograd of the STOCK model on the engine's own ReLU and pooling
  decisions -- the yardstick of every plain-stack product, gradient and diagonal; every replayed decision is bounded (it
  may differ from the float64 model's own only within rounding of a tie).  ``test_stack_harness_cpu.py`` checks the
  replay itself without a GPU;
* ``check_point``: product, gradient, logits, loss and diagonal at one linearisation point against that twin and against
  the fixture the real reference wrote, at the project's bounds (``test_engine_gpu.py``): 1e-6 (GGN) and 2e-6 (Hessian,
  gradient, logits, loss, diagonal) against float64, 1e-5 against the reference's fp32 results;
* ``LaunchRecorder`` / ``record_launches``: the names of the ``hf_*`` calls an operation issues;
* ``run_steps``: three optimizer steps on fresh batches of a fixture's trace;
* ``declined`` / ``declined_net``: a model the engines decline keeps the autograd path, and the reason is named.

No test file imports another test file: what two of them need stands here (or in ``engine_nets.py``)."""

import copy
import types
import warnings

import torch
from tol import within

import pytorchhessianfree_amd as hf
from helpers import RefTrace
from pytorchhessianfree_amd import _lib, curvature, modelprep
from pytorchhessianfree_amd.engine import FusedGGNEngine

DEV = "cuda"


def engine(make, batch, hessian=False, prep=None, train=False, lossf=None, onehot=False):
    """``make(batch_size=batch)`` on the CPU, ``train`` mode first and ``prep(model)`` then, prepared on the GPU, one
    forward pass, ``curvature.ggn_operator`` / ``hessian_operator``: (op, model, (x, t), lossf, the parameters' CPU
    clones).  ``lossf`` replaces the problem's loss; ``onehot`` makes the targets one-hot rows of 10 classes."""
    model, (x, t), lossf0 = make(batch_size=batch, device="cpu")
    lossf = lossf0 if lossf is None else lossf
    if train:
        model.train()
    if prep is not None:
        prep(model)
    cpu_params = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    if onehot:
        t = torch.nn.functional.one_hot(t, 10).to(torch.float32)
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    make_op = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make_op(lossf(out, t), out, params)
    return op, model, (x, t), lossf, cpu_params


def decisions(op):
    """The engine's ReLU masks in call order (the units' at full resolution, then the tail's) and pool positions
    ([n, c, oh, ow], int64)."""
    masks = [(u.y > 0) for u in op.units if u.relu] + [(u.y > 0) for u in op.classifier if u.act == 1]
    pools = [u.pidx.permute(0, 3, 1, 2).long() for u in op.units if u.pool is not None]
    return masks, pools


def replay(model, masks, pools, margin=1e-5):
    """Make every ``nn.ReLU`` / ``nn.MaxPool2d`` call of the float64 ``model`` take the given decisions (in call order),
    and bound what is replayed: a ReLU decision may differ from the model's own only where its input lies within
    ``margin`` x the layer's max-norm of zero, a pool position only where the value there is within the same distance
    of the window's own maximum.  (A condition on the float64 model, not a tolerance.)  Returns ``rewind``: it starts
    the lists over for another forward pass and returns how many (ReLU, pool) calls were replayed since the last start."""
    rc, pc = [0], [0]

    def relu_forward(self, inp):
        m = masks[rc[0]]
        rc[0] += 1
        diff = (inp > 0) != m
        if bool(diff.any()):
            within(float(inp[diff].abs().max() / inp.abs().max()), margin, note="replayed ReLU decision far from zero")
        return inp * m.to(inp.dtype)

    def pool_forward(self, inp):
        idx = pools[pc[0]]
        pc[0] += 1
        own = torch.nn.functional.max_pool2d(inp, self.kernel_size, self.stride, self.padding)
        got = inp.flatten(2).gather(2, idx.flatten(2)).view_as(own)
        within(float((own - got).detach().abs().max() / inp.detach().abs().max().clamp_min(1e-30)), margin,
               note="replayed pool position far from the window's maximum")
        return got

    for mod in model.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.forward = types.MethodType(relu_forward, mod)
        elif isinstance(mod, torch.nn.MaxPool2d):
            mod.forward = types.MethodType(pool_forward, mod)

    def rewind():
        done = rc[0], pc[0]
        rc[0], pc[0] = 0, 0
        return done
    return rewind


def float64_twin(make, batch, op, prep=None, train=False):
    """The float64 twin (same modes, same ``prep``) on the engine's decisions: (params, out, loss, t)."""
    model, (x, t), lossf = make(batch_size=batch, device=DEV)
    if train:
        model.train()
    if prep is not None:
        prep(model)
    model, x = model.double(), x.double()
    replay(model, *decisions(op))
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    return params, out, lossf(out, t), t


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def product64(p64, out64, loss64, v, hessian=False):
    """The twin's Hessian / GGN product of ``v`` by this package's autograd operators in float64."""
    op64 = curvature.HessianOperator(loss64, p64) if hessian else curvature.GGNOperator(loss64, out64, p64)
    return op64(v.double())


def grad64(loss64, p64):
    return torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss64, p64, retain_graph=True)])


def diag64(lossf, p64, out64, t64, batch, n):
    """Per-sample float64 gradients on the same decisions (eval mode: the samples do not interact, so the gradient of
    sample i's loss through the batch's pass IS its per-sample gradient)."""
    want = torch.zeros(n, dtype=torch.float64, device=out64.device)
    for i in range(batch):
        g_i = torch.autograd.grad(lossf(out64[i:i + 1], t64[i:i + 1]), p64, retain_graph=True)
        want += torch.cat([g.reshape(-1) for g in g_i]) ** 2
    return want / batch


def check_point(op, make, batch, x, lossf, cpu_params, fixture, label):
    """Product (bitwise repeatable over 4 calls, symmetric), gradient, logits, loss and ``diag_ef`` of the eval-mode
    ``op`` against float64 on its own decisions and against the reference's results under ``fixture`` = (family, key)
    -- the fixture's own probe vector --, or, ``fixture`` None, against float64 alone on a seeded probe vector.  Every
    figure is printed before it is asserted, in both line forms the files had."""
    kind = "hessian" if op.hessian else "ggn"
    ref = rp = None
    if fixture is not None:
        ref, rp = RefTrace(*fixture), RefTrace(fixture[0], f"{fixture[1]}/{kind}")
        ref.check_inputs(cpu_params, x.cpu())
        v = rp.probe().to(DEV)
    else:
        v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(DEV)
    got = op(v).clone()
    for _ in range(3):
        assert torch.equal(op(v), got)  # bitwise repeatable (4 calls)
    p64, out64, loss64, t64 = float64_twin(make, batch, op)
    tight = 2e-6 if op.hessian else 1e-6
    e = rel(got, product64(p64, out64, loss64, v, op.hessian))
    print(f"{label}: {kind} vs float64 {e:.2e}")
    if rp is not None:
        print(f"{label}-{kind}: product vs float64 {e:.2e}, vs the reference's float64 {rp.vec_err64('', got):.2e}, "
              f"fp32 {rp.vec_err('', got):.2e}")
    within(e, tight)
    if rp is not None:  # the reference's own results: its float64 twin and its fp32 product
        within(rp.vec_err64("", got), tight)
        within(rp.vec_err("", got), 1e-5)
    # symmetric operator
    u = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    gu = op(u).clone()
    a, b = float(u.double() @ got.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    # gradient, logits, loss
    grad = op.gradient().clone()
    e_grad, e_logits = rel(grad, grad64(loss64, p64)), rel(op.logits, out64.detach())
    print(f"{label}: gradient vs float64 {e_grad:.2e}")
    print(f"{label}: logits vs float64 {e_logits:.2e}")
    print(f"  gradient vs float64 {e_grad:.2e}, logits {e_logits:.2e}")
    within(e_grad, 2e-6)
    within(e_logits, 2e-6)
    within(abs(float(op.loss_buf) - float(loss64.detach())), 2e-6 * abs(float(loss64.detach())), strict=False)
    if ref is not None:
        within(ref.vec_err64("grad", grad), 2e-6)
        within(ref.vec_err("grad", grad), 1e-5)
        within(rel(op.logits.cpu(), torch.from_numpy(ref.array("logits"))), 1e-5)
        within(abs(float(op.loss_buf) - ref.scalar("loss")), 1e-5 * abs(ref.scalar("loss")), strict=False)
    # diagonal empirical Fisher
    got_d = op.diag_ef("mean").clone()
    e = rel(got_d, diag64(lossf, p64, out64, t64, batch, op.n))
    print(f"{label}: diag_ef vs float64 {e:.2e}")
    print(f"  diag_ef vs float64 {e:.2e}")
    within(e, 2e-6)
    if ref is not None:
        within(ref.vec_err64("diag", got_d), 2e-6)
        within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)
    assert torch.equal(op(v), got)  # (the products are untouched by the first-order sweeps)


class LaunchRecorder:
    """Forwards every attribute to the real library; a call of an ``hf_*`` function appends its name to ``names``."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hf_"):
            return fn

        def call(*args):
            self._names.append(name)
            return fn(*args)

        return call


def record_launches(monkeypatch):
    """``_lib.load`` returns a ``LaunchRecorder`` around the library from here on: the list its names go to."""
    names = []
    proxy = LaunchRecorder(_lib.load(), names)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return names


def run_steps(make, seeds, batch, fixture, train=False, session=True, **opt_kw):
    """Three ``HessianFree(**opt_kw).step()`` calls of the prepared model, step i on the batch of data seed ``seeds[i]``;
    parameters and every batch are the ones of the reference's trace under ``fixture`` = (family, key).  ``session``: every
    step reports the persistent session's path; without it the session is switched off.  Returns (opt, finals, model,
    the trace) -- for ``compare_trace(opt.state, finals, trace)``."""
    ref = RefTrace(*fixture)
    model, _, lossf = make(batch_size=batch, device="cpu", data_seed=seeds[0])
    if train:
        model.train()
    ref.check_inputs([p for p in model.parameters() if p.requires_grad])
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), **opt_kw)
    if not session:
        opt._session_off = True
    finals = []
    for i in range(3):
        _, (x, t), _ = make(batch_size=batch, device="cpu", data_seed=seeds[i])
        ref.check_inputs(x=x, step=i)
        x, t = x.to(DEV), t.to(DEV)

        def forward():
            out = model(x)
            return lossf(out, t), out

        finals.append(opt.step(forward))
        if session:
            assert opt.path_report()["step"]["path"] == "session", opt.path_report()
    return opt, finals, model, ref


def declined(model, x, t, lossf, reason, hessian=False, who=""):
    """The prepared ``model`` is declined: ``FusedGGNEngine.try_build`` returns None and an entry of ``why`` (one that
    names the engine kind ``who``) carries ``reason``; a ``HessianFree`` step takes the eager path and reports it."""
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    why = []
    assert FusedGGNEngine.try_build(lossf(out, t), out, params, why=why, hessian=hessian) is None
    assert any(who in w and reason in w for w in why), why
    opt = hf.HessianFree(params, cg_max_iter=3, curvature_opt="hessian" if hessian else "ggn")

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    rep = opt.path_report()["step"]
    assert rep["path"] == "eager" and reason in rep["declined"], rep


def declined_net(build, reason):
    """``build()`` (seeded, eval mode, 3x8x8 inputs, 4 classes) is declined for ``reason``: its operator is the autograd
    ``GGNOperator``, whose product matches float64, and ``declined`` holds."""
    torch.manual_seed(0)
    model = build().eval()
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(2, 3, 8, 8, generator=gen), torch.randint(0, 4, (2,), generator=gen)
    m64 = copy.deepcopy(model).double().to(DEV)
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    lossf = torch.nn.CrossEntropyLoss()
    out = model(x)
    op = curvature.ggn_operator(lossf(out, t), out, list(model.parameters()))
    assert type(op) is curvature.GGNOperator
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out64 = m64(x.double())
    want = curvature.GGNOperator(lossf(out64, t), out64, list(m64.parameters()))(v.double())
    within(rel(op(v), want), 1e-6)
    declined(model, x, t, lossf, reason)


class _Net(torch.nn.Module):
    """A ``Sequential`` of the given layers, flattened like the test problems' stacks (the declined variants)."""

    def __init__(self, layers, detour=False):
        super().__init__()
        self.net, self.detour = torch.nn.Sequential(*layers), detour

    def forward(self, x):
        if self.detour:  # the pool reads a COPY of the unit's output: its record is not the unit's
            x = self.net[1](self.net[0](x)) * 1.0
            return torch.flatten(self.net[2:](x), -3)
        return torch.flatten(self.net(x), -3)
