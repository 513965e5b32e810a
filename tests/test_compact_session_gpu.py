"""GPU: the PCG solve on the entries of the parameter vector that can be non-zero (``EngineSession.compact``,
``curvature.CompactFacet``, the compact path of ``cg()``) on a small prepared residual net whose last stage runs 3x3 kernels
on 1x1 maps: a 3x3 stride-2 convolution from a 2x2 map to a 1x1 map (4 live taps of 9), a residual block of 3x3
convolutions on the 1x1 map (the centre tap only), pool, linear head; 8 channels, batch 4; eval- and train-mode BatchNorm.

Products are compared bit for bit.  Solves are compared with the full-length path (``HF_COMPACT_PCG=0``) in everything
discrete, and BOTH paths with a float64 solve of the same system (a float64 CPU copy of the model, autograd GGN products,
``oracle.pcg``): relative l2 error of every stored iterate below 1e-4 -- the bound the suite already states for the iterates
of an engine solve against the reference's CPU solve (test_optimizer_gpu.py, the deterministic ResNet-18 solve)."""

import copy
import warnings

import pack_refs as pr
import pytest
import torch
from tol import within
from torch import nn

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.curvature import CompactFacet
from pytorchhessianfree_amd.session import EngineSession

pytestmark = pytest.mark.gpu
DEV = "cuda"
SOLVE_BOUND = 1e-4
LAM = 1.0  # (the optimizer's default damping)


class TinyResNet(nn.Module):
    def __init__(self, ch=8, classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, ch, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(ch)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(3, 2, 1)                                           # 4x4 -> 2x2
        self.layers = nn.Sequential(tp._BasicBlock(ch, ch, 2), tp._BasicBlock(ch, ch, 1))  # 2x2 -> 1x1, then 1x1
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(ch, classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return self.fc(torch.flatten(x, -3))


def _make(train, l2=0.0, hessian=False):
    torch.manual_seed(3)
    model = TinyResNet()
    with torch.no_grad():
        for m in model.modules():  # (statistics and scales away from their trivial initial values)
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.7, 1.4)
                m.weight.uniform_(0.6, 1.3)
                m.bias.uniform_(-0.2, 0.2)
            if isinstance(m, nn.BatchNorm2d):
                # batch 4 on a 1x1 map: a channel's batch variance over 4 values can be next to nothing, and
                # 1 / sqrt(var + 1e-5) = 316 per layer then amplifies fp32 rounding -- STOCK fp32 autograd solves of this net
                # are 1e-2 ... 4e-1 from their float64 twins with the default eps, 4e-7 with eps = 0.1 (CPU, seeds 3 ... 11)
                m.eps = 0.1
    model.train(train)
    x, t = torch.randn(4, 3, 4, 4), torch.randint(0, 10, (4,))
    ref = copy.deepcopy(model).double()
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, curvature_opt="hessian" if hessian else "ggn")
    opt._ensure_arena()
    params = opt._params_list
    lossf = nn.CrossEntropyLoss()
    if l2:
        lossf = tp.l2_regularized(lossf, model, l2)
    out = model(x.to(DEV))
    why = []
    sess = EngineSession.try_create(lossf(out, t.to(DEV)), out, params, hessian=hessian, why=why)
    assert sess is not None, why
    return sess, opt, ref, x, t


class Problem:
    def __init__(self, train):
        self.sess, self.opt, ref, x, t = _make(train)
        sess = self.sess
        assert sess.compact is not None, sess.compact_decline
        self.n, self.n_live = sess.n, sess.compact.n_live
        self.idx = torch.from_numpy(pr.live_index(sess.compact.layout["table"])).to(DEV)
        self.dead = torch.ones(self.n, dtype=torch.bool, device=DEV)
        self.dead[self.idx] = False
        assert int(self.dead.sum()) == self.n - self.n_live > 0
        self.b = (-sess.gradient()).clone()
        # float64 twin on the CPU: autograd GGN products
        rparams = [p for p in ref.parameters() if p.requires_grad]
        rout = ref(x.double())
        self._keep = (ref, rout)
        self.op64 = curvature.GGNOperator(nn.functional.cross_entropy(rout, t), rout, rparams)
        assert self.op64.n == self.n

    def oracle(self, lam, x0=None, minv=None, **kw):
        from oracle import pcg as oracle

        b64 = self.b.double().cpu()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return oracle.pcg(lambda v: self.op64.local(v).clone() + lam * v, b64,
                              x0=None if x0 is None else x0.double().cpu(),
                              M=None if minv is None else (lambda v, m=minv.double().cpu(): m * v), **kw)


_PROBLEMS = {}


@pytest.fixture(params=["eval", "train"])
def problem(request):
    if request.param not in _PROBLEMS:  # (built once per mode, shared by the tests below and left unchanged)
        _PROBLEMS[request.param] = Problem(request.param == "train")
    return _PROBLEMS[request.param]


def test_layout_of_the_small_net(problem):
    """4 of 9 taps of the strided convolution, the centre tap of the three convolutions on the 1x1 map."""
    lay = problem.sess.compact.layout
    assert sorted(lay["nl"].values()) == [1, 1, 1, 4]
    assert problem.n - problem.n_live == 64 * 5 + 3 * 64 * 8
    assert "n_live = %d" % problem.n_live in problem.sess.mode


def test_compact_product_is_the_gathered_full_product(problem):
    sess, c = problem.sess, problem.sess.compact
    gen = torch.Generator(device=DEV).manual_seed(8)
    v = torch.randn(problem.n, device=DEV, generator=gen)
    full = sess.local(v).clone()
    assert not full[problem.dead].any() and full[problem.idx].abs().max() > 0  # exactly zero on every dead entry
    vc = c.gather(v)
    assert torch.equal(vc, v[problem.idx])
    calls = sess.calls
    got = c(vc).clone()
    assert sess.calls == calls + 1  # (products are counted on the session)
    assert torch.equal(got, full[problem.idx]) and torch.equal(got, c.gather(full))
    assert torch.equal(c(vc), got) and torch.equal(sess.local(v), full)  # bitwise repeatable, both graphs intact
    back = torch.full((problem.n,), 7.0, device=DEV)
    c.scatter(got, back)
    assert torch.equal(back[problem.idx], got) and bool((back[problem.dead] == 7.0).all())
    assert c.dead_entries_zero(full) and c.dead_entries_zero(full, full) and not c.dead_entries_zero(v)


def _solve(problem, compact, monkeypatch, x0=None, M=None, **kw):
    monkeypatch.setenv("HF_COMPACT_PCG", "1" if compact else "0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return hf.cg(hf.DampedCurvature(problem.sess, LAM), problem.b, x0=x0, M=M, **kw)


VARIANTS = {
    "x0": dict(max_iter=8, tol=0.0, store_x_at_iters=[0, 2, 5]),
    "diag_precond": dict(max_iter=8, tol=0.0, store_x_at_iters=[1, 8]),
    "grid": dict(max_iter=12, tol=0.0, store_x_at_iters=None),
    "martens": dict(max_iter=50, martens_conv_crit=True, store_x_at_iters=None),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cg_on_the_compact_vector_against_the_full_path(problem, variant, monkeypatch):
    """``cg()`` through the compact facet against ``HF_COMPACT_PCG=0``: same reason, same iteration count, the same
    iterates stored; iterates exactly zero on the dead entries (full-length snapshots); both paths within SOLVE_BOUND of
    the float64 solve.  With ``x0``, with a ``DiagonalPreconditioner``, with the backtracking grid, with Martens'
    criterion."""
    kw = VARIANTS[variant]
    gen = torch.Generator(device=DEV).manual_seed(5)
    x0 = M = minv = None
    if variant == "x0":
        x0 = torch.randn(problem.n, device=DEV, generator=gen) * 0.1
        x0[problem.dead] = 0.0
    if variant == "diag_precond":
        M = hf.DiagonalPreconditioner(torch.rand(problem.n, device=DEV, generator=gen) + 0.1, LAM, 0.75)
        minv = M.minv
    graphs = len(problem.sess.__dict__.get("_iteration_graphs", {}))
    xs_c, ms_c, reason_c = _solve(problem, True, monkeypatch, x0=x0, M=M, **kw)
    assert len(problem.sess._iteration_graphs) >= max(graphs, 1)  # (the fused iteration graph, kept on the session)
    xs_f, ms_f, reason_f = _solve(problem, False, monkeypatch, x0=x0, M=M, **kw)
    ox, om, oreason = problem.oracle(LAM, x0=x0, minv=minv, **kw)
    assert reason_c == reason_f and len(xs_c) == len(xs_f)
    assert [x is None for x in xs_c] == [x is None for x in xs_f]
    assert (ms_c is None) == (ms_f is None)
    # (the float64 solve may cross a termination threshold one iteration earlier or later than an fp32 one: iterates are
    # compared where both solves have them; the final iterate of the fp32 solves against the float64 iterate of that index)
    worst = {"compact": 0.0, "full": 0.0}
    for i, want in enumerate(ox[:len(xs_c)]):
        if want is None or xs_c[i] is None:
            continue
        assert xs_c[i].shape == (problem.n,) and not xs_c[i][problem.dead].any(), i
        for name, got in (("compact", xs_c[i]), ("full", xs_f[i])):
            den = float(want.norm())
            err = float((got.double().cpu() - want).norm()) / den if den > 0 else float(got.abs().max())
            worst[name] = max(worst[name], err)
    print(f"[compact-solve] {variant}: iterations {len(ox) - 1}, worst relative l2 error against float64: {worst}")
    within(worst["full"], SOLVE_BOUND)
    within(worst["compact"], SOLVE_BOUND)
    if ms_c is not None:
        assert len(ms_c) == len(ms_f)
        for a, b in zip(ms_c, om):  # the quadratic's values against the float64 solve's
            within(abs(float(a) - float(b)), 1e-4 * abs(float(b)) + 1e-7, strict=False)


def test_dirty_dead_entry_and_generic_preconditioner_take_the_full_path(problem, monkeypatch):
    sess = problem.sess
    kw = dict(max_iter=6, tol=0.0, store_x_at_iters=[0])
    b = problem.b.clone()
    b[int(torch.nonzero(problem.dead)[3])] = 0.5  # one non-zero dead entry: silently the full path, same result
    monkeypatch.setenv("HF_COMPACT_PCG", "1")
    seen, orig = [], CompactFacet.gather
    monkeypatch.setattr(CompactFacet, "gather", lambda self, *a, **k: seen.append(1) or orig(self, *a, **k))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xs, _, reason = hf.cg(hf.DampedCurvature(sess, LAM), b, **kw)
        assert not seen
        monkeypatch.setenv("HF_COMPACT_PCG", "0")
        xs0, _, reason0 = hf.cg(hf.DampedCurvature(sess, LAM), b, **kw)
        assert reason == reason0 and torch.equal(xs[-1], xs0[-1])
        # a generic M callable expects full-length vectors
        monkeypatch.setenv("HF_COMPACT_PCG", "1")
        scale = torch.full((problem.n,), 0.5, device=DEV)
        xs1, _, r1 = hf.cg(hf.DampedCurvature(sess, LAM), problem.b, M=lambda r: scale * r, **kw)
        assert not seen and xs1[-1].shape == (problem.n,)
        # ... and the plain call does take the compact path
        hf.cg(hf.DampedCurvature(sess, LAM), problem.b, **kw)
        assert seen


def test_l2_loss_and_hessian_mode_decline_with_a_reason():
    sess, opt, *_ = _make(False, l2=5e-4)
    assert sess.compact is None and "L2" in sess.compact_decline
    opt._session = sess
    opt._note_path("step", "session")
    rep = opt.path_report()["pcg_solve"]
    assert rep["path"] == "full-length" and rep["n_live"] is None and "L2" in rep["declined"]
    sess_h, *_ = _make(False, hessian=True)
    assert sess_h.compact is None and "transposed" in sess_h.compact_decline
