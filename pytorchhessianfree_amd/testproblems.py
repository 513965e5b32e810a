"""Synthetic workloads of the shapes BASELINE.json names (random-init weights,
random data: there is no network for datasets).  The reference builds these from
torchvision / DeepOBS (``examples/example_utils.py:59-109``), neither of which
is installed here, so the topologies are re-declared.

* ``resnet18_mnist``  : torchvision ResNet-18 topology, conv1 1->64 7x7/2 without
  bias, fc 512->10: 11 175 370 trainable parameters in 62 tensors
  (example_utils.py:86-109).
* ``allcnnc_cifar100``: DeepOBS ``cifar100_allcnnc`` topology (dropout is inert in
  eval mode, which the reference example sets): 1 387 108 parameters
  (example_utils.py:59-83).
* ``mwe_mlp`` / ``small_nn``: examples/run_mwe.py:16-20, example_utils.py:23-56.
"""

import torch
from torch import nn


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=False)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(
                nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout)
            )

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + idt)


class ResNet18(nn.Module):
    def __init__(self, in_channels=1, num_classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cfg = [(64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1),
               (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1)]
        self.layers = nn.Sequential(*[_BasicBlock(a, b, s) for a, b, s in cfg])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():  # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return self.fc(torch.flatten(x, -3))


class _Bottleneck(nn.Module):
    def __init__(self, cin, width, stride):
        super().__init__()
        cout = 4 * width
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=False)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(
                nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout)
            )

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + idt)


class ResNet50(nn.Module):
    """torchvision ResNet-50 topology: 25 557 032 parameters at 1000 classes."""

    def __init__(self, in_channels=3, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        blocks, cin = [], 64
        for width, count, stride in [(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]:
            for i in range(count):
                blocks.append(_Bottleneck(cin, width, stride if i == 0 else 1))
                cin = 4 * width
        self.layers = nn.Sequential(*blocks)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return self.fc(torch.flatten(x, -3))


class AllCNNC(nn.Module):
    def __init__(self, num_classes=100):
        super().__init__()

        def c(i, o, k, s=1, p=0):
            return [nn.Conv2d(i, o, k, s, p), nn.ReLU()]

        self.net = nn.Sequential(
            nn.Dropout(0.2),
            *c(3, 96, 3, 1, 1), *c(96, 96, 3, 1, 1), *c(96, 96, 3, 2, 1),
            nn.Dropout(0.5),
            *c(96, 192, 3, 1, 1), *c(192, 192, 3, 1, 1), *c(192, 192, 3, 2, 1),
            nn.Dropout(0.5),
            *c(192, 192, 3, 1, 0), *c(192, 192, 1), *c(192, num_classes, 1),
            nn.AdaptiveAvgPool2d((1, 1)),
        )

    def forward(self, x):
        return torch.flatten(self.net(x), -3)  # also for one unbatched sample [C,H,W]


class ConvPoolCNNC(nn.Module):
    """ConvPool-CNN-C (Springenberg et al., "Striving for Simplicity", table 2): the net All-CNN-C was derived from, with
    a 3x3 / stride-2 max-pool where All-CNN-C has a strided convolution.  Dropout as in ``AllCNNC``."""

    def __init__(self, num_classes=100):
        super().__init__()

        def c(i, o, k, p=0):
            return [nn.Conv2d(i, o, k, 1, p), nn.ReLU()]

        self.net = nn.Sequential(
            nn.Dropout(0.2),
            *c(3, 96, 3, 1), *c(96, 96, 3, 1), *c(96, 96, 3, 1), nn.MaxPool2d(3, 2),
            nn.Dropout(0.5),
            *c(96, 192, 3, 1), *c(192, 192, 3, 1), *c(192, 192, 3, 1), nn.MaxPool2d(3, 2),
            nn.Dropout(0.5),
            *c(192, 192, 3, 0), *c(192, 192, 1), *c(192, num_classes, 1),
            nn.AdaptiveAvgPool2d((1, 1)),
        )

    def forward(self, x):
        return torch.flatten(self.net(x), -3)


class ConvPoolSmall(nn.Module):
    """The smallest pooled stack that takes every path of the pooled-layer kernels: conv3(3->8, pad 1) + ReLU +
    MaxPool(3, 2) (the im2col'd first layer pooled, overlapping windows, 12x12 -> 5x5: an odd map), conv3(8->8, pad 1) +
    ReLU + MaxPool(2, 2) (disjoint windows that leave the last row and column out, 5x5 -> 2x2), conv1(8->classes), global
    average pool."""

    def __init__(self, num_classes=4):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(3, 2),
            nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2),
            nn.Conv2d(8, num_classes, 1),
            nn.AdaptiveAvgPool2d((1, 1)),
        )

    def forward(self, x):
        return torch.flatten(self.net(x), -3)


def _batched(net, x):
    """``net(x)``, also for one unbatched sample [C,H,W] (``nn.Flatten`` keeps dimension 0)."""
    return net(x[None])[0] if x.dim() == 3 else net(x)


class ConvFCSmall(nn.Module):
    """The smallest conv stack with a classifier tail (LeNet / DeepOBS 2c2d shape): ``ConvPoolSmall``'s two pooled units
    (12x12 -> 5x5 -> 2x2: the last unit is pooled), ``Flatten`` to 32 features, ``Linear(32->20) ReLU Linear(20->10)``.
    10 and 20 are no multiples of 4: the dense kernels' unaligned paths, and later parameters off 16-byte boundaries in an
    arena."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(3, 2),
            nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2),
            nn.Flatten(),
            nn.Linear(32, 20), nn.ReLU(), nn.Linear(20, num_classes),
        )

    def forward(self, x):
        return _batched(self.net, x)


class ConvFCFlat(nn.Module):
    """One unpooled, im2col'd unit that is first and last, a non-square 6x5 map (hw = 30) and a one-layer tail:
    ``Conv(3->8, 3, pad 1) ReLU Flatten Linear(240->10)`` on 3x6x5 inputs."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.Flatten(), nn.Linear(240, num_classes))

    def forward(self, x):
        return _batched(self.net, x)


def seed_batchnorm(model, seed=0):
    """Non-trivial eval-mode state for every BatchNorm of ``model``: running mean ~ N(0, 0.25), running variance
    U[0.5, 2], weight U[0.5, 1.5], bias ~ N(0, 0.25), from a generator of its own.  The constructors' 0 / 1 / 1 / 0 would
    hide every error in how a kernel uses ``mean``, ``rstd`` and the scale.  Returns the model."""
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                k = m.num_features
                for t, val in ((m.running_mean, 0.5 * torch.randn(k, generator=g)),
                               (m.running_var, 0.5 + 1.5 * torch.rand(k, generator=g)),
                               (m.weight, 0.5 + torch.rand(k, generator=g)), (m.bias, 0.5 * torch.randn(k, generator=g))):
                    if t is not None:  # (no running statistics / not affine)
                        t.copy_(val)
    return model


class ConvBNSmall(nn.Module):
    """The smallest plain stack with BatchNorm units of every kind: conv3(3->8, pad 1, no bias) + BN + ReLU +
    MaxPool(3, 2) (the im2col'd first layer, pooled, overlapping windows, 12x12 -> 5x5), conv3(8->8) + BN + ReLU (unpooled),
    conv3(8->12) + BN + MaxPool(2, 2) (pooled without a ReLU, 5x5 -> 2x2), conv1(12->classes) with a bias, global average
    pool."""

    def __init__(self, num_classes=4):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(3, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d(3, 2),
            nn.Conv2d(8, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(),
            nn.Conv2d(8, 12, 3, 1, 1, bias=False), nn.BatchNorm2d(12), nn.MaxPool2d(2, 2),
            nn.Conv2d(12, num_classes, 1),
            nn.AdaptiveAvgPool2d((1, 1)),
        )

    def forward(self, x):  # (BatchNorm2d takes no unbatched sample)
        return torch.flatten(_batched(self.net, x), -3)


class ConvBNFCSmall(nn.Module):
    """``ConvBNSmall``'s first unit, conv3(8->8) + BN + ReLU + MaxPool(2, 2) (5x5 -> 2x2: the last unit is pooled),
    ``Flatten`` to 32 features, ``Linear(32->20) ReLU Linear(20->10)``."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(3, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d(3, 2),
            nn.Conv2d(8, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d(2, 2),
            nn.Flatten(),
            nn.Linear(32, 20), nn.ReLU(), nn.Linear(20, num_classes),
        )

    def forward(self, x):
        return _batched(self.net, x)


class VGG11BN(nn.Module):
    """VGG-11 with BatchNorm for 32x32 inputs (the usual CIFAR form): conv3 + BN + ReLU units of 64, 128, 256, 256, 512,
    512, 512, 512 channels, a MaxPool(2, 2) behind units 1, 2, 4, 6 and 8 (32 -> 1), ``Flatten``, ``Linear(512->classes)``.
    The convolutions carry no bias (the BatchNorm's shift takes its place)."""

    CFG = (64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M")

    def __init__(self, num_classes=10):
        super().__init__()
        layers, c = [], 3
        for k in self.CFG:
            if k == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(c, k, 3, 1, 1, bias=False), nn.BatchNorm2d(k), nn.ReLU()]
                c = k
        self.net = nn.Sequential(*layers, nn.Flatten(), nn.Linear(512, num_classes))

    def forward(self, x):
        return _batched(self.net, x)


class C3D3(nn.Module):
    """A DeepOBS ``3c3d``-sized net from stock modules: three conv + ReLU + MaxPool(3, 2, 1) units (32x32 -> 14 -> 6 -> 3),
    ``Flatten`` to 1152 features, ``Linear(1152->512) ReLU Linear(512->256) ReLU Linear(256->classes)``."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(3, 64, 5), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
            nn.Conv2d(64, 96, 3), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
            nn.Conv2d(96, 128, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
            nn.Flatten(),
            nn.Linear(1152, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, num_classes),
        )

    def forward(self, x):
        return _batched(self.net, x)


def l2_regularized(loss_function, model, l2=5e-4):
    """``loss + 0.5 * l2 * sum ||W||^2`` over the WEIGHTS (no biases): the regularised
    loss the reference's All-CNN-C example trains (examples/example_utils.py:77-81 adds
    DeepOBS' ``get_regularization_loss()``; DeepOBS -- not vendored, PyPI ``deepobs`` --
    sums ``factor * ||p||_2^2`` over the non-bias parameters and halves the total;
    ``cifar100_allcnnc`` defaults to ``l2_reg = 5e-4``).  The GGN ignores the term (it
    does not depend on the network output); the Hessian gains ``l2 * I`` on the weights."""
    weights = [p for name, p in model.named_parameters() if "bias" not in name]

    def regularized(outputs, targets):
        reg = sum((w * w).sum() for w in weights)
        total = loss_function(outputs, targets) + (0.5 * l2) * reg
        # what the curvature engine may assume about this loss (checked numerically on first use):
        # base loss + sum 0.5 * coef * ||w||^2 over the listed tensors
        total._hf_quadratic = ((float(l2), tuple(weights)),)
        return total

    return regularized


def relu_margin(model, inputs):
    """Smallest |x| over the inputs of every ``nn.ReLU`` module in one forward pass of
    ``model`` (run it in float64).  A ReLU whose input sits within fp32 rounding of zero
    (1e-7 here) may get a different sign from two correct fp32 implementations, which changes
    first-order gradients and curvature products by 1e-4-ish of their max-norm; with ~1.3 M
    pre-activations in the ResNet-18 workload this happens on roughly every third random
    batch.  Parity tests against float64 / the CPU path therefore use data seeds for which
    this margin is comfortably above fp32 rounding (scripts/experiments/margin_search.py)."""
    smallest = [float("inf")]

    def hook(_, args):
        smallest[0] = min(smallest[0], float(args[0].detach().abs().min()))

    handles = [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, nn.ReLU)]
    try:
        with torch.no_grad():
            model(inputs)
    finally:
        for h in handles:
            h.remove()
    return smallest[0]


# data seeds of ``resnet18_mnist(batch_size=32, seed=0)`` whose smallest |ReLU input| in float64 is
# 1.0e-6 ... 5.7e-7 (found by scripts/experiments/margin_search.py over seeds 1000-3999; fp32
# forward passes are good to 1e-7 ... 6e-7 there): bench.py's rank r uses entry r
RESNET18_B32_SEPARATED_SEEDS = (1483, 1377, 2116, 1101, 3097, 1322, 1192, 1187)


def freeze_stem_and_layer1(model):
    """``requires_grad = False`` on the stem (conv1, bn1) and layer1 of a ResNet: the optimizer then works "in the
    subspace of trainable parameters" (reference optimizer.py:121-123, utils.py:31-32; its own test problem freezes
    its first layer, tests/test_utils.py:39-43).  Returns the model."""
    if hasattr(model, "layers"):  # (torchvision's layer1 = the blocks in front of the first STRIDED block)
        blocks = list(model.layers)
        n1 = next((i for i, b in enumerate(blocks) if i > 0 and getattr(b, "downsample", None) is not None), len(blocks))
        layer1 = blocks[:n1]
    else:
        layer1 = [model.layer1]
    for mod in (model.conv1, model.bn1, *layer1):
        for p in mod.parameters():
            p.requires_grad_(False)
    return model


def count_trainable(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def resnet18_mnist(batch_size=32, seed=0, device="cpu", data_seed=None):
    """Model in eval mode (BatchNorm then uses running statistics, which makes the
    curvature a plain sum over samples -- required for batch sharding, SURVEY.md
    section 7), inputs U[0,1) [B,1,28,28], integer targets, CE-mean."""
    torch.manual_seed(seed)
    model = ResNet18(1, 10).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 1, 28, 28, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def resnet18_mnist_mse(batch_size=32, seed=0, device="cpu", data_seed=None):
    """The same model and inputs with the loss of the reference's own examples and tests (``nn.MSELoss``,
    examples/run_mwe.py:19, tests/test_utils.py:47): targets = the one-hot rows of the same integer targets."""
    model, (inputs, targets), _ = resnet18_mnist(batch_size, seed, "cpu", data_seed)
    onehot = torch.nn.functional.one_hot(targets, 10).to(torch.float32)
    return model.to(device), (inputs.to(device), onehot.to(device)), nn.MSELoss()


def resnet50_small_images(batch_size=32, seed=0, device="cpu", data_seed=None, image=64):
    """BASELINE.json configs[4]: a ResNet-50-sized parameter vector (25 557 032);
    eval-mode BN, inputs U[0,1) [B,3,image,image], 1000 classes, CE-mean."""
    torch.manual_seed(seed)
    model = ResNet50(3, 1000).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, image, image, generator=g)
    targets = torch.randint(0, 1000, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def allcnnc_cifar100(batch_size=32, seed=0, device="cpu", data_seed=None):
    torch.manual_seed(seed)
    model = AllCNNC(100).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 32, 32, generator=g)
    targets = torch.randint(0, 100, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convpoolcnnc_cifar100(batch_size=32, seed=0, device="cpu", data_seed=None):
    torch.manual_seed(seed)
    model = ConvPoolCNNC(100).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 32, 32, generator=g)
    targets = torch.randint(0, 100, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convpool_small(batch_size=2, seed=0, device="cpu", data_seed=None):
    """``ConvPoolSmall`` in eval mode; inputs U[0,1) [B,3,12,12], 4 classes, CE-mean."""
    torch.manual_seed(seed)
    model = ConvPoolSmall(4).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 12, 12, generator=g)
    targets = torch.randint(0, 4, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convfc_small(batch_size=2, seed=0, device="cpu", data_seed=None):
    """``ConvFCSmall`` in eval mode; inputs U[0,1) [B,3,12,12], 10 classes, CE-mean."""
    torch.manual_seed(seed)
    model = ConvFCSmall(10).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 12, 12, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convfc_flat(batch_size=3, seed=0, device="cpu", data_seed=None):
    """``ConvFCFlat`` in eval mode; inputs U[0,1) [B,3,6,5], 10 classes, CE-mean."""
    torch.manual_seed(seed)
    model = ConvFCFlat(10).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 6, 5, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convbn_small(batch_size=2, seed=0, device="cpu", data_seed=None):
    """``ConvBNSmall`` in eval mode with seeded BatchNorm state; inputs U[0,1) [B,3,12,12], 4 classes, CE-mean."""
    torch.manual_seed(seed)
    model = seed_batchnorm(ConvBNSmall(4), seed).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 12, 12, generator=g)
    targets = torch.randint(0, 4, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def convbn_fc_small(batch_size=2, seed=0, device="cpu", data_seed=None):
    """``ConvBNFCSmall`` in eval mode with seeded BatchNorm state; inputs U[0,1) [B,3,12,12], 10 classes, CE-mean."""
    torch.manual_seed(seed)
    model = seed_batchnorm(ConvBNFCSmall(10), seed).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 12, 12, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def vgg11bn_cifar10(batch_size=32, seed=0, device="cpu", data_seed=None):
    """``VGG11BN`` in eval mode with seeded BatchNorm state; inputs U[0,1) [B,3,32,32], 10 classes, CE-mean."""
    torch.manual_seed(seed)
    model = seed_batchnorm(VGG11BN(10), seed).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 32, 32, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def c3d3_cifar10(batch_size=32, seed=0, device="cpu", data_seed=None):
    """``C3D3`` in eval mode; inputs U[0,1) [B,3,32,32], 10 classes, CE-mean."""
    torch.manual_seed(seed)
    model = C3D3(10).eval()
    g = torch.Generator().manual_seed(seed if data_seed is None else data_seed)
    inputs = torch.rand(batch_size, 3, 32, 32, generator=g)
    targets = torch.randint(0, 10, (batch_size,), generator=g)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.CrossEntropyLoss()


def mwe_mlp(batch_size=16, dim=10, seed=0, device="cpu"):
    torch.manual_seed(seed)
    model = nn.Sequential(nn.Linear(dim, dim, bias=False), nn.ReLU(), nn.Linear(dim, dim))
    inputs, targets = torch.rand(batch_size, dim), torch.rand(batch_size, dim)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.MSELoss()


def small_nn(batch_size=32, seed=0, device="cpu", freeze_layer1=True):
    torch.manual_seed(seed)
    model = nn.Sequential(
        nn.Linear(7, 5), nn.ReLU(), nn.Sequential(nn.Linear(5, 5), nn.ReLU()), nn.Linear(5, 3)
    )
    if freeze_layer1:
        for p in next(model.children()).parameters():
            p.requires_grad = False
    inputs, targets = torch.rand(batch_size, 7), torch.rand(batch_size, 3)
    return model.to(device), (inputs.to(device), targets.to(device)), nn.MSELoss()
