"""Nets with non-square inputs, per-axis strides / paddings / kernels and degenerate maps (one row, one column, one
pixel, one sample) for the engine-level tests, and their float64 reference.

Every other engine test has ``h == w``, ``stride[0] == stride[1]``, ``padding[0] == padding[1]`` and ``r == s``: the host
code between ``engine/topology.py`` and the launches (``buffers._plan`` / ``_allocate``, ``common._live_taps``,
``problems.py``, ``plain._pool_dims``, ``diag_ef``'s per-sample geometry, the compact layout, the head's one-pixel view)
hands ``h, w, r, s, stride_h, stride_w, pad_h, pad_w, oh, ow`` on again and again, and a swap of two of them passes a
suite of square cases.  ``row_map`` and ``col_map`` are each other's transpose: dead kernel ROWS only in one, dead
kernel COLUMNS only in the other.

``CASES``: seven ResNet-family nets (``GeometryResNet``: the module tree of ``engine_nets.SmallResNet`` with the stem's
and the pool's ``(kernel, stride, padding)`` and the block strides free, ints or pairs) and two plain conv + bias stacks
(``GeometryStack``).  Seeding and BatchNorm state as ``engine_nets._resnet``: seed 5, statistics and scales off their
trivial values, ``eps = 0.1``, input from ``torch.randn`` drawn after the model.

``TAIL_CASES``: five plain stacks that end in ``nn.Flatten`` and ``Linear [ReLU] ... Linear`` (``GeometryTail``), for
the classifier tail of the plain-stack engine: what ``convfc_small`` / ``convfc_flat`` never reach at engine level --
summed data-gradient slabs, tail tensors off the 16-byte grid of the flat vector, partial flatten tiles, a 1x1 and a
pooled non-square last map, batch 1 and 256 (``TAIL_GEOMETRY`` says which case reaches what).  Same seeding; kept apart
from ``CASES`` (GGN products only, bounds of their own).

``BN_CASES``: six plain stacks with BatchNorm units (``BN_STACKS``; five end in the global average pool, one in a
classifier tail), eval and train mode, on per-axis windows / strides / paddings, dead taps, many row blocks, one-row /
one-column / 1x1 maps (``BN_GEOMETRY`` says which case reaches what).  Same seeding and BatchNorm state as the ResNets;
kept apart from ``CASES`` (bounds of their own).

The reference (``Reference``): float64 autograd of a deep copy of the STOCK model on the CPU -- loss, gradient, GGN
product (``curvature.GGNOperator``), Hessian product (``curvature.HessianOperator``), diagonal empirical Fisher by
per-sample gradients --, optionally on replayed ReLU decisions and max-pool positions (``_replay_relu_decisions``,
``_replay_pool_positions``: bounded).

The measure (``per_tensor_errors``): per parameter tensor ``T``, ``max|got_T - want_T| / max|want_T|`` -- a whole-vector
max-norm lets a small block (a BatchNorm shift) be entirely wrong below 1e-6 of the classifier's entries --, and exactly
zero wherever the reference is exactly zero (dead taps)."""

import copy
import types

import torch
from tol import within
from torch import nn

from pytorchhessianfree_amd import curvature
from pytorchhessianfree_amd import testproblems as tp

SEED = 5

#   input [n, c, h, w] | stem (k, s, p) | pool (k, s, p) | blocks (cin, cout, stride) | classes
RESNETS = {
    "nonsquare_odd": dict(x=(3, 1, 11, 6), stem=(3, 1, 1), pool=(3, 2, 1), blocks=[(12, 12, 1), (12, 20, 2)], classes=7),
    "asym_stride": dict(x=(2, 3, 9, 8), stem=(3, (1, 2), 1), pool=((2, 2), (2, 1), 0),
                        blocks=[(8, 16, (2, 1)), (16, 16, 1)], classes=10),
    "row_map": dict(x=(5, 1, 4, 12), stem=(3, 1, 1), pool=(3, 2, 1), blocks=[(8, 8, 1), (8, 16, 2), (16, 16, 1)],
                    classes=3),
    "col_map": dict(x=(5, 1, 12, 4), stem=(3, 1, 1), pool=(3, 2, 1), blocks=[(8, 8, 1), (8, 16, 2), (16, 16, 1)],
                    classes=3),
    "batch_one": dict(x=(1, 1, 8, 8), stem=(3, 1, 1), pool=(3, 2, 1), blocks=[(32, 32, 1), (32, 64, 2), (64, 64, 2)],
                      classes=10),
    "wide_rows": dict(x=(4, 1, 12, 10), stem=(3, 1, 1), pool=(3, 2, 1), blocks=[(132, 132, 1), (132, 260, 2)],
                      classes=17),
    "stem7": dict(x=(2, 3, 13, 9), stem=(7, 2, 3), pool=(3, 2, 1), blocks=[(16, 16, 1), (16, 36, 2)], classes=5),
}
STACKS = {
    "plain_rect": dict(x=(3, 3, 7, 10), classes=12, layers=lambda: [
        nn.Conv2d(3, 8, (1, 3), 1, (0, 1)), nn.ReLU(), nn.MaxPool2d((3, 2), (2, 1)),
        nn.Conv2d(8, 12, (3, 1), (2, 1), (1, 0)), nn.ReLU(), nn.Conv2d(12, 20, 3, 1, 1), nn.ReLU(),
        nn.Conv2d(20, 12, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "plain_quads_in": dict(x=(1, 4, 5, 9), classes=8, layers=lambda: [
        nn.Conv2d(4, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Conv2d(8, 16, 3, (1, 2), 1), nn.ReLU(),
        nn.Conv2d(16, 8, 1), nn.AdaptiveAvgPool2d((1, 1))]),
}
CASES = list(RESNETS) + list(STACKS)

# Plain stacks with a classifier tail (``nn.Flatten``, then ``Linear [ReLU] ... Linear``; ``GeometryTail``), at the
# shapes the tail's host arithmetic and kernels meet nowhere else at engine level -- what each reaches stands with its
# literals in ``TAIL_GEOMETRY``
TAILS = {
    "tail_rect_pooled": dict(x=(3, 3, 9, 7), classes=7, layers=lambda: [
        nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d((2, 3), (2, 2)),
        nn.Conv2d(8, 12, (3, 1), 1, (1, 0)), nn.ReLU(), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Flatten(), nn.Dropout(0.5), nn.Linear(72, 21), nn.ReLU(), nn.Linear(21, 7)]),
    "tail_wide_first": dict(x=(2, 1, 5, 7), classes=5, layers=lambda: [
        nn.Conv2d(1, 36, 3, 1, 1), nn.ReLU(), nn.Flatten(), nn.Linear(1260, 70), nn.ReLU(),
        nn.Linear(70, 33, bias=False), nn.ReLU(), nn.Linear(33, 5)]),
    "tail_pixel": dict(x=(1, 4, 4, 4), classes=10, layers=lambda: [
        nn.Conv2d(4, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Conv2d(8, 16, 2), nn.Flatten(), nn.Linear(16, 10)]),
    "tail_rows_256": dict(x=(256, 1, 3, 2), classes=3, layers=lambda: [
        nn.Conv2d(1, 4, 3, 1, 1), nn.ReLU(), nn.Flatten(), nn.Linear(24, 3)]),
    "tail_col_map": dict(x=(4, 1, 12, 1), classes=6, layers=lambda: [
        nn.Conv2d(1, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d((2, 1), (2, 1)), nn.Conv2d(8, 8, 3, (2, 1), 1), nn.ReLU(),
        nn.Flatten(), nn.Linear(24, 40), nn.ReLU(), nn.Linear(40, 6)]),
}
TAIL_CASES = list(TAILS)


def _C(cin, cout, k, s=1, p=0):
    return nn.Conv2d(cin, cout, k, s, p, bias=False)


# Plain stacks with BatchNorm units (``Conv2d(bias=False) BatchNorm2d [ReLU] [MaxPool2d]``; BatchNorm state as the
# ResNets'), in eval and in train mode: per-axis windows, strides and paddings behind a BatchNorm, a pooled unit without
# ReLU, dead kernel taps, many row blocks in the pooled adjoint, one-row / one-column / 1x1 maps, batch statistics over
# 15 rows, a first unit that is not im2col'd, pooled BatchNorm units in front of a classifier tail -- what each reaches
# stands with its literals in ``BN_GEOMETRY``.  ``bn_row_map`` is ``bn_col_map``'s transpose.
BN_STACKS = {
    "bn_rect_pooled": dict(x=(3, 3, 7, 10), classes=12, layers=lambda: [
        _C(3, 8, (1, 3), 1, (0, 1)), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((3, 2), (2, 1), (1, 0)),
        _C(8, 12, (3, 1), (2, 1), (1, 0)), nn.BatchNorm2d(12), nn.MaxPool2d((1, 2), (1, 2)),
        _C(12, 20, 3, 1, 1), nn.BatchNorm2d(20), nn.ReLU(), nn.Conv2d(20, 12, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "bn_col_map": dict(x=(5, 1, 12, 1), classes=8, layers=lambda: [
        _C(1, 8, 3, 1, 1), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((2, 1), (2, 1)),
        _C(8, 8, 3, (2, 1), 1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 8, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "bn_row_map": dict(x=(5, 1, 1, 12), classes=8, layers=lambda: [
        _C(1, 8, 3, 1, 1), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((1, 2), (1, 2)),
        _C(8, 8, 3, (1, 2), 1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 8, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "bn_wide_rows": dict(x=(4, 1, 12, 10), classes=16, layers=lambda: [
        _C(1, 132, 3, 1, 1), nn.BatchNorm2d(132), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
        _C(132, 260, 3, 1, 1), nn.BatchNorm2d(260), nn.ReLU(), nn.MaxPool2d((2, 3), (2, 2), (0, 1)),
        nn.Conv2d(260, 16, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "bn_pixel_one": dict(x=(1, 4, 4, 4), classes=8, layers=lambda: [
        _C(4, 8, 3, 1, 1), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d(2, 2),
        _C(8, 16, 2), nn.BatchNorm2d(16), nn.ReLU(), nn.Conv2d(16, 8, 1), nn.AdaptiveAvgPool2d((1, 1))]),
    "bn_tail_rect": dict(x=(3, 3, 9, 7), classes=7, layers=lambda: [
        _C(3, 8, 3, 1, 1), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((2, 3), (2, 2), (0, 1)),
        _C(8, 12, (3, 1), 1, (1, 0)), nn.BatchNorm2d(12), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Flatten(), nn.Linear(96, 21), nn.ReLU(), nn.Linear(21, 7)]),
}
BN_CASES = list(BN_STACKS)
BN_TRAIN_CASES = [c for c in BN_CASES if c != "bn_pixel_one"]  # (a 1x1 map of ONE sample has no batch statistics)
BN_HESSIAN_CASES = [c for c in BN_CASES if c != "bn_tail_rect"]  # (no Hessian products through a classifier tail)
BN_CAPTURED_CASES = [("bn_rect_pooled", True), ("bn_wide_rows", False)]  # (case, train mode)

# per convolution in call order: (module, input map, output map, live-tap mask (0: all live), row blocks of the adjoint)
GEOMETRY = {
    "nonsquare_odd": [
        ("conv1", (11, 6), (11, 6), 0, 3),
        ("layers.0.conv1", (6, 3), (6, 3), 0, 1),
        ("layers.0.conv2", (6, 3), (6, 3), 0, 1),
        ("layers.1.downsample.0", (6, 3), (3, 2), 0, 1),
        ("layers.1.conv1", (6, 3), (3, 2), 0, 1),
        ("layers.1.conv2", (3, 2), (3, 2), 0, 1),
    ],
    "asym_stride": [
        ("conv1", (9, 8), (9, 4), 0, 1),
        ("layers.0.downsample.0", (4, 3), (2, 3), 0, 1),
        ("layers.0.conv1", (4, 3), (2, 3), 0, 1),
        ("layers.0.conv2", (2, 3), (2, 3), 0, 1),
        ("layers.1.conv1", (2, 3), (2, 3), 0, 1),
        ("layers.1.conv2", (2, 3), (2, 3), 0, 1),
    ],
    "row_map": [
        ("conv1", (4, 12), (4, 12), 0, 2),
        ("layers.0.conv1", (2, 6), (2, 6), 0, 1),
        ("layers.0.conv2", (2, 6), (2, 6), 0, 1),
        ("layers.1.downsample.0", (2, 6), (1, 3), 0, 1),
        ("layers.1.conv1", (2, 6), (1, 3), 504, 1),   # 0b111111000: kernel row 0 never meets data
        ("layers.1.conv2", (1, 3), (1, 3), 56, 1),    # 0b000111000: the middle kernel row only
        ("layers.2.conv1", (1, 3), (1, 3), 56, 1),
        ("layers.2.conv2", (1, 3), (1, 3), 56, 1),
    ],
    "col_map": [
        ("conv1", (12, 4), (12, 4), 0, 2),
        ("layers.0.conv1", (6, 2), (6, 2), 0, 1),
        ("layers.0.conv2", (6, 2), (6, 2), 0, 1),
        ("layers.1.downsample.0", (6, 2), (3, 1), 0, 1),
        ("layers.1.conv1", (6, 2), (3, 1), 438, 1),   # 0b110110110: kernel column 0 never meets data
        ("layers.1.conv2", (3, 1), (3, 1), 146, 1),   # 0b010010010: the middle kernel column only
        ("layers.2.conv1", (3, 1), (3, 1), 146, 1),
        ("layers.2.conv2", (3, 1), (3, 1), 146, 1),
    ],
    "batch_one": [
        ("conv1", (8, 8), (8, 8), 0, 2),
        ("layers.0.conv1", (4, 4), (4, 4), 0, 1),
        ("layers.0.conv2", (4, 4), (4, 4), 0, 1),
        ("layers.1.downsample.0", (4, 4), (2, 2), 0, 1),
        ("layers.1.conv1", (4, 4), (2, 2), 0, 1),
        ("layers.1.conv2", (2, 2), (2, 2), 0, 1),
        ("layers.2.downsample.0", (2, 2), (1, 1), 0, 1),
        ("layers.2.conv1", (2, 2), (1, 1), 432, 1),   # 0b110110000: the four taps below / right of the padding
        ("layers.2.conv2", (1, 1), (1, 1), 16, 1),    # the centre tap
    ],
    "wide_rows": [
        ("conv1", (12, 10), (12, 10), 0, 60),
        ("layers.0.conv1", (6, 5), (6, 5), 0, 18),    # 120 rows in shares of 7: the last share is ONE row
        ("layers.0.conv2", (6, 5), (6, 5), 0, 18),
        ("layers.1.downsample.0", (6, 5), (3, 3), 0, 1),
        ("layers.1.conv1", (6, 5), (3, 3), 0, 1),
        ("layers.1.conv2", (3, 3), (3, 3), 0, 1),
    ],
    "stem7": [
        ("conv1", (13, 9), (7, 5), 0, 2),
        ("layers.0.conv1", (4, 3), (4, 3), 0, 1),
        ("layers.0.conv2", (4, 3), (4, 3), 0, 1),
        ("layers.1.downsample.0", (4, 3), (2, 2), 0, 1),
        ("layers.1.conv1", (4, 3), (2, 2), 0, 1),
        ("layers.1.conv2", (2, 2), (2, 2), 0, 1),
    ],
    "plain_rect": [
        ("net.0", (7, 10), (7, 10), 0, 2),
        ("net.3", (3, 9), (2, 9), 0, 1),
        ("net.5", (2, 9), (2, 9), 0, 1),
        ("net.7", (2, 9), (2, 9), 0, 1),
    ],
    "plain_quads_in": [
        ("net.0", (5, 9), (5, 9), 0, 1),
        ("net.3", (2, 4), (2, 2), 0, 1),
        ("net.5", (2, 2), (2, 2), 0, 1),
    ],
}
# per tail case -- "convs": as GEOMETRY; "linears", per Linear: (c_in, c_out, sT, sD, weight offset, bias offset or None)
# (split counts of the tangent / data-gradient GEMM by ``dense_plan``, offsets in the flat vector); "last": (rows, hw, c)
# of the map ``nn.Flatten`` reads; "pools": per unit (kh, kw, sh, sw, ph, pw) or None; "n": entries of the flat vector
TAIL_GEOMETRY = {
    # the last map pooled and non-square (2x3); Linear(21,7) at offset 2057 (1 mod 4) with row pitch 21: the dense
    # kernels' element-wise operand form; a Dropout leaf inside the tail
    "tail_rect_pooled": dict(
        convs=[("net.0", (9, 7), (9, 7), 0, 2), ("net.3", (4, 3), (4, 3), 0, 1)],
        linears=[(72, 21, 3, 1, 524, 2036), (21, 7, 1, 1, 2057, 2204)],
        last=(3, 6, 12), pools=[(2, 3, 2, 2, 0, 0), (2, 1, 2, 1, 0, 0)], n=2211),
    # an unpooled map of the im2col'd first unit; hw = 35 and c = 36: two flatten tiles each way, the last one partial;
    # the first data-gradient split counts above 1 (3, 2); a bias-free Linear at offset 88630 (2 mod 4), the last bias at
    # 91105 (1 mod 4); three tail layers
    "tail_wide_first": dict(
        convs=[("net.0", (5, 7), (5, 7), 0, 3)],
        linears=[(1260, 70, 20, 3, 360, 88560), (70, 33, 3, 2, 88630, None), (33, 5, 2, 1, 90940, 91105)],
        last=(2, 35, 36), pools=[None], n=91110),
    # hw = 1, batch 1, the last unit without ReLU, the first unit not im2col'd (4 input channels)
    "tail_pixel": dict(
        convs=[("net.0", (4, 4), (4, 4), 0, 1), ("net.3", (2, 2), (1, 1), 0, 1)],
        linears=[(16, 10, 1, 1, 824, 984)],
        last=(1, 1, 16), pools=[(2, 2, 2, 2, 0, 0), None], n=994),
    # 256 rows: the dense kernels' limit, eight row tiles
    "tail_rows_256": dict(
        convs=[("net.0", (3, 2), (3, 2), 0, 6)],
        linears=[(24, 3, 1, 1, 40, 112)],
        last=(256, 6, 4), pools=[None], n=115),
    # a one-column map: kernel columns 0 and 2 of both convolutions meet only padding (0b010010010); sD = 2
    "tail_col_map": dict(
        convs=[("net.0", (12, 1), (12, 1), 146, 1), ("net.3", (6, 1), (3, 1), 146, 1)],
        linears=[(24, 40, 1, 2, 664, 1624), (40, 6, 2, 1, 1664, 1904)],
        last=(4, 3, 8), pools=[(2, 1, 2, 1, 0, 0), None], n=1910),
}
# per BatchNorm-stack case -- "convs", per convolution in call order: (module, input map, output map, live-tap mask, row
# blocks of the adjoint (``adjoint_row_blocks``), pool (kh, kw, sh, sw, ph, pw) or None, pooled map or None); "im2col":
# whether the first unit is im2col'd (fewer than 4 input channels); "n": entries of the flat vector
BN_GEOMETRY = {
    # every pair of axis parameters unequal (kernels 1x3 / 3x1, stride (2,1), paddings (0,1) / (1,0), pools 3x2 by (2,1)
    # padded (1,0) and 1x2 by (1,2)); a padded pool; a pooled unit WITHOUT ReLU; an im2col'd pooled first unit, rb = 2
    "bn_rect_pooled": dict(convs=[
        ("net.0", (7, 10), (7, 10), 0, 2, (3, 2, 2, 1, 1, 0), (4, 9)),
        ("net.4", (4, 9), (2, 9), 0, 1, (1, 2, 1, 2, 0, 0), (2, 4)),
        ("net.7", (2, 4), (2, 4), 0, 1, None, None),
        ("net.10", (2, 4), (2, 4), 0, 1, None, None)], im2col=True, n=2852),
    # a one-column map: kernel columns 0 and 2 meet only padding (0b010010010) under a BatchNorm; the second unit's
    # train-mode statistics run over 5 x 3 x 1 = 15 rows
    "bn_col_map": dict(convs=[
        ("net.0", (12, 1), (12, 1), 146, 1, (2, 1, 2, 1, 0, 0), (6, 1)),
        ("net.4", (6, 1), (3, 1), 146, 1, None, None),
        ("net.7", (3, 1), (3, 1), 0, 1, None, None)], im2col=True, n=752),
    # its transpose: kernel rows 0 and 2 (0b000111000)
    "bn_row_map": dict(convs=[
        ("net.0", (1, 12), (1, 12), 56, 1, (1, 2, 1, 2, 0, 0), (1, 6)),
        ("net.4", (1, 6), (1, 3), 56, 1, None, None),
        ("net.7", (1, 3), (1, 3), 0, 1, None, None)], im2col=True, n=752),
    # the pooled adjoint with 60 row blocks (480 rows in shares of 8, 33 channel quads) and 40 (120 rows in shares of 3,
    # 65 quads); a pool padded (0, 1)
    "bn_wide_rows": dict(convs=[
        ("net.0", (12, 10), (12, 10), 0, 60, (3, 3, 2, 2, 1, 1), (6, 5)),
        ("net.4", (6, 5), (6, 5), 0, 40, (2, 3, 2, 2, 0, 1), (3, 3)),
        ("net.8", (3, 3), (3, 3), 0, 1, None, None)], im2col=True, n=315028),
    # batch 1, a 1x1 map behind the second unit, four input channels: the first unit is not im2col'd (eval mode only)
    "bn_pixel_one": dict(convs=[
        ("net.0", (4, 4), (4, 4), 0, 1, (2, 2, 2, 2, 0, 0), (2, 2)),
        ("net.4", (2, 2), (1, 1), 0, 1, None, None),
        ("net.7", (1, 1), (1, 1), 0, 1, None, None)], im2col=False, n=984),
    # pooled BatchNorm units (the second without ReLU) in front of a classifier tail; the last map 2x4 (GGN only)
    "bn_tail_rect": dict(convs=[
        ("net.0", (9, 7), (9, 7), 0, 2, (2, 3, 2, 2, 0, 1), (4, 4)),
        ("net.4", (4, 4), (4, 4), 0, 1, (2, 1, 2, 1, 0, 0), (2, 4))], im2col=True, n=2735),
}
TAIL_CAPTURED_CASES = ["tail_wide_first", "tail_rect_pooled"]
FLATTEN_TILE = 32  # (hf_head.hip: the flatten kernels move 32 x 32 tiles of the [hw, c] plane of one sample)

TRAIN_CASES = ["nonsquare_odd", "row_map", "col_map", "wide_rows", "stem7"]  # (batch_one: a 1x1 map of ONE sample has no
COMPACT_CASES = ["row_map", "col_map", "batch_one"]                           # batch statistics; ``STACKS``: no BatchNorm)
CAPTURED_CASES = ["asym_stride", "plain_rect"]


class GeometryResNet(nn.Module):
    def __init__(self, cin, stem, pool, blocks, classes):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, blocks[0][0], *stem, bias=False)
        self.bn1 = nn.BatchNorm2d(blocks[0][0])
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(*pool)
        self.layers = nn.Sequential(*[tp._BasicBlock(a, b, s) for a, b, s in blocks])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(blocks[-1][1], classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return self.fc(torch.flatten(x, -3))


class GeometryStack(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return torch.flatten(self.net(x), -3)


class GeometryTail(nn.Module):
    """(``nn.Flatten`` is one of ``layers``: the net's output is the last ``Linear``'s, unchanged)"""

    def __init__(self, layers):
        super().__init__()
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return self.net(x)


def make(case, train=False):
    """The stock fp32 net of ``case`` on the CPU, seeded, and two batches ``[(x, t), (x2, t2)]`` drawn after it (the
    second: for the tests that hand the engine a new batch)."""
    torch.manual_seed(SEED)
    if case in TAILS:
        spec = TAILS[case]
        model = GeometryTail(spec["layers"]())
    elif case in BN_STACKS:
        spec = BN_STACKS[case]
        model = (GeometryTail if case == "bn_tail_rect" else GeometryStack)(spec["layers"]())
    elif case in RESNETS:
        spec = RESNETS[case]
        model = GeometryResNet(spec["x"][1], spec["stem"], spec["pool"], spec["blocks"], spec["classes"])
    else:
        spec = STACKS[case]
        model = GeometryStack(spec["layers"]())
    with torch.no_grad():
        for m in model.modules():  # (statistics and scales away from their trivial initial values)
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.7, 1.4)
                m.weight.uniform_(0.6, 1.3)
                m.bias.uniform_(-0.2, 0.2)
                m.eps = 0.1
    model.train(train)
    batches = []
    for _ in range(2):
        x = torch.randn(*spec["x"])
        batches.append((x, torch.randint(0, spec["classes"], (spec["x"][0],))))
    return model, batches


def named_sizes(model):
    return [(n, p.numel()) for n, p in model.named_parameters() if p.requires_grad]


def conv_geometry(model, x):
    """Per convolution, in call order: ``(name, h, w, r, s, stride, padding, oh, ow)`` of one forward pass."""
    names = {m: n for n, m in model.named_modules()}
    rows, hooks = [], []

    def hook(m, inp, out):
        rows.append((names[m], inp[0].shape[2], inp[0].shape[3], m.kernel_size[0], m.kernel_size[1], tuple(m.stride),
                     tuple(m.padding), out.shape[2], out.shape[3]))

    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return rows


def adjoint_row_blocks(rows, k, bytes_per_wg=32768):
    """``rb`` of a unit with ``rows`` output positions and ``k`` channels by the rule of ``buffers._allocate`` (restated:
    that code runs with a GPU only; the GPU tests compare the engine's own ``u.rb`` with the same literals)."""
    if not (k % 4 == 0 and k // 4 <= 256 and rows >= 64):
        return 1
    rp = 256 // (k // 4)
    tgt = min(1024, max(64, rows * k * 4 // bytes_per_wg))
    per = max(rp, -(-rows // tgt))
    rb = -(-rows // per)
    return rb if rb >= 2 else 1


def dense_planned_splits(length, out_cols, kstep=32, target_blocks=512, max_splits=32):
    """Slabs of one skinny GEMM of a ``Linear`` layer that reduces over ``length`` entries into ``out_cols`` columns, by
    the rule of hf_dense.hip (``dense_kper`` / ``dense_split_ok`` / ``dense_planned_splits``, restated: the library's
    own ``hf_dense_plan`` is compared with it on the CPU, the engine's ``u.sT`` / ``u.sD`` with the same literals on the
    GPU): about ``target_blocks`` workgroups of one 32-column tile each, every split a multiple of ``kstep`` entries,
    none starting behind the end."""
    def kper(splits):
        return -(-(-(-length // splits)) // kstep) * kstep

    s = min(max_splits, -(-target_blocks // (-(-out_cols // 32))))
    while s > 1 and not (s - 1) * kper(s) < length:
        s -= 1
    return s


def dense_plan(c_in, c_out):
    """``(sT, sD)`` of a ``Linear(c_in, c_out)``: the tangent / forward GEMM reduces over ``c_in``, the data gradient
    over ``c_out``."""
    return dense_planned_splits(c_in, c_out), dense_planned_splits(c_out, c_in)


def linear_geometry(model):
    """Per ``nn.Linear`` in module order: ``(c_in, c_out, sT, sD, weight offset, bias offset or None)`` -- the offsets
    in the flat vector of the trainable parameters, in the order of ``model.parameters()``."""
    offs, o = {}, 0
    for p in model.parameters():
        if p.requires_grad:
            offs[id(p)] = o
            o += p.numel()
    return [(m.in_features, m.out_features, *dense_plan(m.in_features, m.out_features), offs.get(id(m.weight)),
             None if m.bias is None else offs.get(id(m.bias)))
            for m in model.modules() if isinstance(m, nn.Linear)]


def last_map(model, x):
    """``(rows, hw, c)`` of the map ``nn.Flatten`` turns into the first ``Linear``'s rows."""
    seen = []
    flat = next(m for m in model.modules() if isinstance(m, nn.Flatten))
    hook = flat.register_forward_hook(lambda m, inp, out: seen.append(tuple(inp[0].shape)))
    with torch.no_grad():
        model(x)
    hook.remove()
    (n, c, h, w), = seen
    return n, h * w, c


def relu_inputs(model, x):
    """The input of every ``nn.ReLU`` call of one forward pass, in call order."""
    seen, hooks = [], []
    for m in model.modules():
        if isinstance(m, nn.ReLU):
            hooks.append(m.register_forward_hook(lambda m, inp, out: seen.append(inp[0].detach().clone())))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return seen


def _replay_relu_decisions(model, masks, max_flips=200, margin=1e-5):
    """Make every ``nn.ReLU`` call of ``model`` take the sign decisions ``masks`` (in call order) -- and BOUND what is
    being replayed: a decision may differ from the model's own (``input > 0``) only where the model's own input lies
    within ``margin`` x the layer's max-norm of zero (an fp32 forward pass is good to ~1e-6 of that), and in at most
    ``max_flips`` entries over the whole network.  A wrong mask -- a kernel bug -- would flip decisions of inputs far
    from zero, or many of them, and is not inherited by the reference product."""
    cursor, flips = [0], [0]

    def relu_forward(self, inp):
        m = masks[cursor[0]].to(device=inp.device)
        cursor[0] += 1
        own = inp > 0
        diff = own != (m > 0)
        n = int(diff.sum())
        if n:
            flips[0] += n
            worst = float(inp[diff].abs().max() / inp.abs().max())
            within(worst, margin, note=("replayed ReLU decision far from zero", cursor[0] - 1, n))
            within(flips[0], max_flips, strict=False, note="replayed ReLU decisions that differ from the model's own")
        return inp * m.to(dtype=inp.dtype)

    for mod in model.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.forward = types.MethodType(relu_forward, mod)
    return flips


def pool_positions(model, x):
    """The positions every ``nn.MaxPool2d`` call of one forward pass takes, in call order: ``[n, c, oh, ow]`` int64,
    flat ``y * w + x`` inside the ``(n, c)`` plane (ATen's ``return_indices``)."""
    seen, hooks = [], []

    def hook(m, inp, out):
        seen.append(nn.functional.max_pool2d(inp[0].detach(), m.kernel_size, m.stride, m.padding, return_indices=True)[1])

    for m in model.modules():
        if isinstance(m, nn.MaxPool2d):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return seen


def _replay_pool_positions(model, pools, flips, max_flips=200, margin=1e-5):
    """Make every ``nn.MaxPool2d`` call of ``model`` read its windows at the positions ``pools`` (in call order, as
    ``pool_positions`` gives them) -- bounded as the ReLU decisions are: the value at a replayed position may lie below
    the window's own maximum only within ``margin`` x the map's max-norm, and the positions that differ from the
    model's own count against the same ``max_flips`` (``flips``: the counter ``_replay_relu_decisions`` returned)."""
    cursor = [0]

    def pool_forward(self, inp):
        idx = pools[cursor[0]].to(device=inp.device, dtype=torch.int64)
        cursor[0] += 1
        own, own_idx = nn.functional.max_pool2d(inp, self.kernel_size, self.stride, self.padding, return_indices=True)
        assert idx.shape == own_idx.shape, (cursor[0] - 1, tuple(idx.shape), tuple(own_idx.shape))
        assert int(idx.min()) >= 0 and int(idx.max()) < inp.shape[2] * inp.shape[3]
        got = inp.flatten(2).gather(2, idx.flatten(2)).view_as(own)
        n = int((idx != own_idx).sum())
        if n:
            flips[0] += n
            worst = float((own - got).detach().abs().max() / inp.detach().abs().max().clamp_min(1e-300))
            within(worst, margin, note=("replayed pool position far from the window's maximum", cursor[0] - 1, n))
            within(flips[0], max_flips, strict=False, note="replayed decisions that differ from the model's own")
        return got

    for mod in model.modules():
        if isinstance(mod, nn.MaxPool2d):
            mod.forward = types.MethodType(pool_forward, mod)


# The fp32 and the float64 forward pass of every case take the SAME ReLU decisions (test_geometry_nets_cpu.py; the tail
# cases: the same pool positions too): what an engine replays into the reference may differ from the float64 net's own
# in a handful of entries next to zero (of positions next to their window's maximum), no more
MAX_FLIPS, MARGIN = 4, 1e-5


class Reference:
    """float64 autograd of a deep copy of ``model`` on the CPU at the batch ``(x, t)``; ``masks``: the ReLU decisions to
    take instead of the float64 net's own, ``pools``: the ``nn.MaxPool2d`` positions (``pool_positions``' form), both in
    call order and replayed under ``MAX_FLIPS`` / ``MARGIN`` (one count for both).  Every result is a flat float64
    vector in the order of ``model.parameters()`` (the trainable ones)."""

    def __init__(self, model, x, t, masks=None, pools=None):
        self.model = copy.deepcopy(model).cpu().double()
        self.x, self.t = x.detach().cpu().double(), t.detach().cpu()
        self.flips = None
        if masks is not None:
            self.flips = _replay_relu_decisions(self.model, [m.cpu() for m in masks], max_flips=MAX_FLIPS, margin=MARGIN)
        if pools is not None:
            self.flips = [0] if self.flips is None else self.flips
            _replay_pool_positions(self.model, [p.cpu() for p in pools], self.flips, max_flips=MAX_FLIPS, margin=MARGIN)
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        self.out = self.model(self.x)
        self.loss_t = nn.functional.cross_entropy(self.out, self.t)
        self._cache = {}

    @property
    def logits(self):
        return self.out.detach()

    def loss(self):
        return float(self.loss_t.detach())

    def gradient(self):
        if "grad" not in self._cache:
            g = torch.autograd.grad(self.loss_t, self.params, retain_graph=True)
            self._cache["grad"] = torch.cat([a.reshape(-1) for a in g])
        return self._cache["grad"]

    def ggn(self, v):
        return curvature.GGNOperator(self.loss_t, self.out, self.params)(v.detach().cpu().double()).clone()

    def hessian(self, v):
        return curvature.HessianOperator(self.loss_t, self.params)(v.detach().cpu().double()).clone()

    def running(self):
        """``{name: buffer}`` of every BatchNorm's ``running_mean`` / ``running_var`` / ``num_batches_tracked`` behind the
        reference's ONE forward pass (train mode: moved once from the state ``model`` was handed over in)."""
        return {f"{n}.{k}": getattr(m, k).detach().clone() for n, m in self.model.named_modules()
                if isinstance(m, nn.BatchNorm2d) for k in ("running_mean", "running_var", "num_batches_tracked")}

    def diag_ef(self):
        """``(1/N) sum_i g_i^2`` over the per-sample gradients (eval mode: the samples do not interact, so the gradient
        of sample i's loss through the batch's pass is its per-sample gradient)."""
        assert not self.model.training
        if "diag" not in self._cache:
            d = torch.zeros_like(self.gradient())
            for i in range(self.x.shape[0]):
                g = torch.autograd.grad(nn.functional.cross_entropy(self.out[i:i + 1], self.t[i:i + 1]), self.params,
                                        retain_graph=True)
                d += torch.cat([a.reshape(-1) for a in g]) ** 2
            self._cache["diag"] = d / self.x.shape[0]
        return self._cache["diag"]


def per_tensor_errors(got, want, sizes):
    """``{name: max|got_T - want_T| / max|want_T|}`` over the parameter tensors ``sizes = [(name, numel), ...]`` of the
    flat vectors ``got`` / ``want`` (float64 reference).  Wherever the reference is EXACTLY zero -- the taps that never
    meet data, a tensor whose product is zero -- ``got`` must be exactly zero too (asserted here)."""
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    assert got.numel() == want.numel() == sum(k for _, k in sizes), (got.numel(), want.numel())
    assert bool(torch.isfinite(got).all())
    errs, off = {}, 0
    for name, k in sizes:
        a, b = got[off:off + k], want[off:off + k]
        off += k
        zero = b == 0
        assert not bool(a[zero].any()), (name, "non-zero where the reference is exactly zero", int((a[zero] != 0).sum()))
        top = float(b.abs().max())
        errs[name] = float((a - b).abs().max()) / top if top > 0 else 0.0
    return errs


def running_errors(model, ref):
    """``{buffer: max|got - want| / max|want|}`` of ``model``'s running statistics against ``ref.running()``;
    ``num_batches_tracked`` must be equal (asserted)."""
    mods, errs = dict(model.named_modules()), {}
    for key, want in ref.running().items():
        name, attr = key.rsplit(".", 1)
        got = getattr(mods[name], attr).detach().cpu()
        if attr == "num_batches_tracked":
            assert int(got) == int(want), (key, int(got), int(want))
        else:
            errs[key] = float((got.double() - want).abs().max() / want.abs().max())
    return errs


def scalar_error(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def own_masks(model, x):
    """The ReLU decisions of ``model``'s own forward pass at ``x``, in call order."""
    return [a > 0 for a in relu_inputs(model, x)]


def probe(n, seed, device="cpu"):
    """The vector the products are taken of: drawn on the CPU (the same entries on every device)."""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(device)


def stock_fp32_errors(case, device, train=False, seeds=(11, 12)):
    """What STOCK fp32 autograd on ``device`` -- the unprepared model, ``GGNOperator``, ``HessianOperator``, per-sample
    gradients -- is away from the float64 reference on its own ReLU decisions, in the measure of the engine tests:
    ``{quantity: {tensor: error}}``.  The yardstick the bounds of test_engine_geometry_gpu.py are 3x of."""
    model, batches = make(case, train)
    x, t = batches[0]
    sizes = named_sizes(model)
    own = copy.deepcopy(model).to(device)
    # (the tail and BatchNorm-stack cases: on its own pool positions too, as the engine's reference is on the engine's)
    ref = Reference(model, x, t, masks=own_masks(own, x.to(device)),
                    pools=pool_positions(own, x.to(device)) if (case in TAILS or case in BN_STACKS) else None)
    model, x, t = model.to(device), x.to(device), t.to(device)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    loss = nn.functional.cross_entropy(out, t)
    res = {"logits": {"logits": float((out.detach().cpu().double() - ref.logits).abs().max() / ref.logits.abs().max())},
           "loss": {"loss": scalar_error(loss, ref.loss())}}
    if train:  # (the one train-mode pass above moved the running statistics, as the reference's one pass moved its own)
        res["running"] = running_errors(model, ref)
    grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, params, retain_graph=True)])
    res["gradient"] = per_tensor_errors(grad, ref.gradient(), sizes)
    n = grad.numel()
    for name, op, want in (("ggn", curvature.GGNOperator(loss, out, params), ref.ggn),
                           ("hessian", curvature.HessianOperator(loss, params), ref.hessian)):
        if name == "hessian" and case == "bn_tail_rect":
            continue  # (the engine makes no Hessian products through a classifier tail: no bound to take)
        worst = {}
        for seed in seeds:
            v = probe(n, seed, device)
            for k, e in per_tensor_errors(op(v), want(v), sizes).items():
                worst[k] = max(worst.get(k, 0.0), e)
        res[name] = worst
    if not train:
        d = torch.zeros_like(grad)
        for i in range(x.shape[0]):
            g = torch.autograd.grad(nn.functional.cross_entropy(model(x[i:i + 1]), t[i:i + 1]), params)
            d += torch.cat([a.reshape(-1) for a in g]) ** 2
        res["diag_ef"] = per_tensor_errors(d / x.shape[0], ref.diag_ef(), sizes)
    return res
