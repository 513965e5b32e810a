"""The small ResNet-style nets the engine's GPU tests build (stem + max-pool and residual blocks, one of them with a
downsample branch), one conv + bias stack for the plain-stack engine and the five-layer MLPs of the dense-stack engine's
launch tests (``net_and_loss``).

``small``: 8x8 inputs, batch 8, 8 / 16 channels (two blocks) -- at these sizes the stem is the one unit on the row-major
kernel.  ``wide``: 8x8 inputs, batch 16, 32 / 64 channels and a third block on a 1x1 map -- the stem, an identity block, a
downsample block whose two adjoints share one launch, and units with ``rb == 1``; its dead taps give the compact layout
``local_compact`` needs."""

import copy

import torch
from torch import nn

from pytorchhessianfree_amd import modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine
from pytorchhessianfree_amd.utils import ParameterArena

DEV = "cuda"
NETS = {"small": dict(batch=8, ch=8, blocks=[(8, 8, 1), (8, 16, 2)]),
        "wide": dict(batch=16, ch=32, blocks=[(32, 32, 1), (32, 64, 2), (64, 64, 2)])}


class SmallResNet(nn.Module):
    def __init__(self, ch, blocks, classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(1, ch, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(ch)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(3, 2, 1)  # 8x8 -> 4x4
        self.layers = nn.Sequential(*[tp._BasicBlock(a, b, s) for a, b, s in blocks])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(blocks[-1][1], classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return self.fc(torch.flatten(x, -3))


def _freeze(model, pattern):
    if pattern == "stem":  # a dead stem: the sweep ends in front of it
        for p in (*model.conv1.parameters(), *model.bn1.parameters()):
            p.requires_grad_(False)
    elif pattern == "scale_shift":  # one unit without sums at all, one with each of the two alone
        bns = [model.bn1, model.layers[0].bn1, model.layers[0].bn2]
        bns[0].weight.requires_grad_(False)
        bns[0].bias.requires_grad_(False)
        bns[1].weight.requires_grad_(False)
        bns[2].bias.requires_grad_(False)
    else:
        assert pattern == "plain"


def _arena_order(model, where):
    """The trainable parameters with the head's 10-entry bias -- the one count that is no multiple of 4 -- moved in front
    of the parameter named ``where``: bound into a ``ParameterArena`` in this order, every parameter behind it sits 8 bytes
    off a 16-byte boundary."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad and n != "fc.bias"]
    at = [n for n, _ in named].index(where)
    return [p for _, p in named[:at]] + [model.fc.bias] + [p for _, p in named[at:]]


def _resnet(net):
    """The stock net of ``NETS[net]`` on the CPU, seeded."""
    spec = NETS[net]
    torch.manual_seed(5)
    model = SmallResNet(spec["ch"], spec["blocks"])
    with torch.no_grad():
        for m in model.modules():  # (statistics and scales away from their trivial initial values)
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.7, 1.4)
                m.weight.uniform_(0.6, 1.3)
                m.bias.uniform_(-0.2, 0.2)
                m.eps = 0.1
    return model


def build(net, pattern="plain", train=False, hessian=False, arena_at=None):
    spec = NETS[net]
    model = _resnet(net)
    _freeze(model, pattern)
    model.train(train)
    x, t = torch.randn(spec["batch"], 1, 8, 8), torch.randint(0, 10, (spec["batch"],))
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    if arena_at is not None:
        params = _arena_order(model, arena_at)
        model._arena = ParameterArena(params)  # (kept alive with the model: the parameters are views into it now)
        at = next(i for i, p in enumerate(params) if p is model.fc.bias)
        assert all(p.data_ptr() % 16 == (8 if i > at else 0) for i, p in enumerate(params))
    out = model(x.to(DEV))
    why = []
    op = FusedGGNEngine.try_build(nn.functional.cross_entropy(out, t.to(DEV)), out, params, hessian=hessian, why=why)
    assert isinstance(op, FusedGGNEngine), why
    return op


class SmallConvStack(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.Conv2d(8, 16, 3, 2, 1), nn.ReLU(),
                                 nn.Conv2d(16, 12, 1), nn.ReLU(), nn.AdaptiveAvgPool2d((1, 1)))

    def forward(self, x):
        return torch.flatten(self.net(x), -3)


def three_forms(kind, train=False, prepared=True):
    """One net in three forms: the stock fp32 model on the CPU, a float64 CPU twin with the same parameters and
    buffers (a deep copy: nothing is shared), and a copy on the GPU prepared for the engine (``None`` without
    ``prepared``: the tests that run without a GPU).  ``kind``: "resnet" (``SmallResNet`` of ``NETS["small"]``: 8x8
    inputs of one channel, 10 classes) or "plain" (``SmallConvStack``: 8x8 inputs of three channels, 12 classes), in
    eval or train mode."""
    if kind == "resnet":
        model = _resnet("small")
    else:
        assert kind == "plain"
        torch.manual_seed(7)
        model = SmallConvStack()
    model.train(train)
    twin = copy.deepcopy(model).double()
    gpu = None
    if prepared:
        gpu = copy.deepcopy(model).to(DEV)
        modelprep.prepare_model(gpu, channels_last=True)
    return model, twin, gpu


def build_plain(hessian=False):
    """conv + bias + ReLU x 3 (12 classes: channel counts in quads) -> global average pool on 8x8 inputs, batch 4: a
    ``PlainStackEngine``."""
    from pytorchhessianfree_amd.engine import PlainStackEngine

    torch.manual_seed(7)
    model = SmallConvStack()
    model.eval()
    x, t = torch.randn(4, 3, 8, 8), torch.randint(0, 12, (4,))
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    out = model(x.to(DEV))
    why = []
    op = FusedGGNEngine.try_build(nn.functional.cross_entropy(out, t.to(DEV)), out, list(model.parameters()),
                                  hessian=hessian, why=why)
    assert isinstance(op, PlainStackEngine) and op.hessian == hessian, why
    return op


# the dense stack's nets A-E (``test_dense_launch_order_gpu.py`` describes them): frozen parameters per net as (index in
# the Sequential, attribute)
DENSE_FROZEN = {"A": (), "B": ((0, "weight"), (0, "bias")), "C": ((2, "weight"),), "D": ((0, "weight"),), "E": ()}
DENSE_ROWS = 3


def net_and_loss(net):
    """(prepared model, its outputs, the loss) of dense net ``net`` on the GPU, seeded on the CPU."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(7, 5), nn.ReLU(), nn.Linear(5, 5), nn.Tanh(), nn.Linear(5, 3))
    for index, attr in DENSE_FROZEN[net]:
        getattr(model[index], attr).requires_grad = False
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(DENSE_ROWS, 7, generator=gen).to(DEV)
    if net == "E":
        t, lossf = torch.randn(DENSE_ROWS, 3, generator=gen).to(DEV), nn.MSELoss()
    else:
        t, lossf = torch.randint(0, 3, (DENSE_ROWS,), generator=gen).to(DEV), nn.CrossEntropyLoss()
    model = model.to(DEV)
    modelprep.prepare_model(model)
    out = model(x)
    return model, out, lossf(out, t)
