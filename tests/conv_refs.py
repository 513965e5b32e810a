"""Exact references of the implicit-GEMM convolution kernels (``hf_conv.hip``: ``k_conv_nt``, ``k_conv_tn``, ``k_conv_dw``,
``k_conv_group``), the table of cases that reaches every instantiation the launchers can dispatch, and a mirror of the
launchers' dispatch rules.  Shared by ``test_conv_refs_cpu.py`` (table against the library's planner, on the CPU) and
``test_conv_kernels_gpu.py`` (kernels against the references).  Plain module: numpy and torch on the CPU unless a caller
names a device.

Nothing here has a tolerance.  ``v_mfma_f32_32x32x2f32`` is true fp32 and the operands are integers in [-3, 3]: every
product is an integer of magnitude <= 9, every partial sum of any subset of them, in any order, is an integer below
``9 * L`` (``L``: the longest reduction), and while ``9 * L < 2**24`` all of them are exactly representable -- the fp32
result of every split, of the last arriver's sum and of the consumer's slab sum IS the float64 reference (``exact``
checks the condition per problem; it is a condition on the inputs, not a bound on an error).  The BatchNorm partial sums
of the BNSUM epilogue multiply the outputs by ``xhat = (x - mean) * rstd`` with integer ``x`` and ``mean`` and ``rstd``
a power of two, so ``t * xhat`` is exact too; their condition is on the 64-row column sums (``bn_exact``)."""

import zlib
from collections import namedtuple

import numpy as np
import torch

NAN = float("nan")
VMAX = 3            # operands are integers in [-VMAX, VMAX]
EXACT_LIMIT = 2 ** 24
CONFIGS = ("Small", "Big", "Big96", "Flat96")
TILE = {0: (64, 64), 1: (128, 128), 2: (128, 96), 3: (96, 128)}   # (BM, BN) per configuration (hf_conv.hip: Cfg)
BK = {0: 32, 1: 16, 2: 16, 3: 16}

# the geometries of the float-operand tests (``test_conv_gpu.py``, the merged launches of ``test_layer_kernels_gpu.py``,
# the planner sweep of ``test_host_logic_cpu.py``): (N, H, W, C, K, R, S, stride, padding)
GEOMS = [
    (32, 7, 7, 64, 64, 3, 3, (1, 1), (1, 1)),      # ResNet-18 layer1
    (32, 7, 7, 64, 128, 3, 3, (2, 2), (1, 1)),     # layer2.0.conv1 (7 -> 4)
    (32, 7, 7, 64, 128, 1, 1, (2, 2), (0, 0)),     # layer2.0.downsample
    (32, 4, 4, 128, 128, 3, 3, (1, 1), (1, 1)),    # layer2
    (32, 2, 2, 256, 256, 3, 3, (1, 1), (1, 1)),    # layer3: every tap meets data somewhere
    (32, 2, 2, 256, 512, 3, 3, (2, 2), (1, 1)),    # layer4.0.conv1: 4 of 9 taps live
    (32, 1, 1, 512, 512, 3, 3, (1, 1), (1, 1)),    # layer4: centre tap only
    (32, 7, 7, 128, 64, 3, 3, (1, 1), (1, 1)),     # tangent operands: 2*Cin channels
    (4, 5, 6, 12, 20, 3, 2, (2, 1), (1, 0)),       # ragged everything
    (2, 9, 9, 8, 100, 5, 5, (1, 1), (2, 2)),       # K not a multiple of the tile
    (3, 6, 5, 36, 8, 1, 1, (1, 1), (0, 0)),
    (8, 16, 16, 96, 96, 3, 3, (1, 1), (1, 1)),     # All-CNN-C-like: many tiles, no split needed
    (1, 3, 3, 4, 4, 3, 3, (1, 1), (0, 0)),         # one output pixel
    (3, 8, 8, 3, 6, 3, 3, (1, 1), (1, 1)),         # channel counts not multiples of 4: scalar gathers
    (32 * 196, 1, 1, 49, 64, 1, 1, (1, 1), (0, 0)),  # the stem as a 1x1 product over its im2col
    # large-M problems: the 128x128-tile configuration (four accumulators per wave)
    (32, 32, 32, 96, 96, 3, 3, (1, 1), (1, 1)),    # All-CNN-C conv2: 32768 rows
    (32, 16, 16, 96, 192, 3, 3, (2, 2), (1, 1)),   # strided, 96 -> 192
    (8, 16, 16, 192, 192, 3, 3, (1, 1), (0, 0)),   # no padding, ragged row tile (8*14*14 = 1568 rows: small config)
    (32, 16, 16, 192, 192, 3, 3, (1, 1), (1, 1)),  # All-CNN-C conv5: weight gradient on 96 x 128 tiles, columns flat over (tap, c)
    (32, 12, 12, 192, 100, 1, 1, (1, 1), (0, 0)),  # 1x1, 100 output channels (ragged column tile)
    (16, 16, 16, 256, 128, 1, 1, (1, 1), (0, 0)),  # ResNet-50-like 1x1 reduction
]

# d: 0 forward, 1 data gradient, 2 weight gradient; act_ld / mat_ld: 0 = dense; splits: 0 = the planner's choice
Problem = namedtuple("Problem", "d n h w c k r s stride pad act_ld mat_ld splits")
# what the planner must answer: configuration, scalar gathers, taps per residue class (() = plain enumeration), live
# taps, splits and steps per split
Expect = namedtuple("Expect", "config scalar cls_taps live splits per")
# form: slabs | tickets | backward | backward_slabs | dw_slabs | group_slabs | group_slabs_bnsum
# tickets: (workspace bytes, ticket counters, target_blocks) of a ticket-mode form;  sums: per problem, whether the
# BNSUM launch writes its partial sums
Case = namedtuple("Case", "name form problems expect tickets sums")


def P(d, n, h, w, c, k, r, s, stride=1, pad=0, act_ld=0, mat_ld=0, splits=0):
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    pd = (pad, pad) if isinstance(pad, int) else tuple(pad)
    return Problem(d, n, h, w, c, k, r, s, st, pd, act_ld, mat_ld, splits)


def E(config, splits, per, live, cls_taps=(), scalar=0):
    return Expect(config, scalar, tuple(cls_taps), live, splits, per)


def out_hw(p):
    return (p.h + 2 * p.pad[0] - p.r) // p.stride[0] + 1, (p.w + 2 * p.pad[1] - p.s) // p.stride[1] + 1


def out_shape(p):
    """Shape of the output tensor in the kernel's own layout."""
    oh, ow = out_hw(p)
    return ((p.n, oh, ow, p.k), (p.n, p.h, p.w, p.c), (p.k, p.r, p.s, p.c))[p.d]


def reduction_length(p):
    """Longest sum of products behind one output element."""
    oh, ow = out_hw(p)
    return (p.r * p.s * p.c, p.r * p.s * p.k, p.n * oh * ow)[p.d]


def exact(p):
    """The exactness condition of the module docstring for problem ``p``."""
    return reduction_length(p) * VMAX * VMAX < EXACT_LIMIT


def live_taps(p):
    """Taps (r, q) of the window that meet data for at least one output position, by brute force."""
    oh, ow = out_hw(p)
    rows = [r for r in range(p.r) if any(0 <= y * p.stride[0] - p.pad[0] + r < p.h for y in range(oh))]
    cols = [q for q in range(p.s) if any(0 <= x * p.stride[1] - p.pad[1] + q < p.w for x in range(ow))]
    return [(r, q) for r in rows for q in cols]


def class_taps(p):
    """Per residue class (py, px) of the input pixel, in the kernel's class order: how many live taps reach it --
    tap (r, q) reaches pixel (y, x) iff (y + pad - r) % stride == 0, both ways."""
    out = []
    for py in range(p.stride[0]):
        for px in range(p.stride[1]):
            if (p.h - py + p.stride[0] - 1) // p.stride[0] <= 0 or (p.w - px + p.stride[1] - 1) // p.stride[1] <= 0:
                continue
            out.append(sum(1 for r, q in live_taps(p)
                           if (py + p.pad[0] - r) % p.stride[0] == 0 and (px + p.pad[1] - q) % p.stride[1] == 0))
    return tuple(out)


# ---- seeded generators ---------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _ints(rng, shape, lo=-VMAX, hi=VMAX):
    return rng.randint(lo, hi + 1, size=shape).astype(np.float32)


def operands(p, key=""):
    """The tensors of problem ``p`` on the CPU, float32 with integer values in [-3, 3], seeded by the geometry alone (the
    three directions of one layer share x, wt and gy, as the merged launches need; two cases with the same problem share
    operands and reference):
      x  [n, h, w, c]  NHWC activations,   wt [k, r, s, c]  weights (O, H, W, I),   gy [n, oh, ow, k]  cotangent
    and ``act`` / ``mat``, the two operands of direction ``p.d`` in the layouts the entry points take -- ``act`` with a
    pixel stride of ``act_ld``, ``mat`` ([k][r][s][c] forward, [c][r][s][k] data gradient) with ``mat_ld`` floats per
    tap, the channels beyond the tensor's own filled with other integers that a correct kernel never reads."""
    rng = np.random.RandomState(_seed("conv", key, *p[1:10]))
    oh, ow = out_hw(p)
    x, wt, gy = _ints(rng, (p.n, p.h, p.w, p.c)), _ints(rng, (p.k, p.r, p.s, p.c)), _ints(rng, (p.n, oh, ow, p.k))

    def widen(t, ld):
        if not ld or ld == t.shape[-1]:
            return np.ascontiguousarray(t)
        wide = _ints(rng, t.shape[:-1] + (ld,), 1, VMAX)
        wide[..., :t.shape[-1]] = t
        return wide

    if p.d == 0:
        act, mat = widen(x, p.act_ld), widen(wt, p.mat_ld)
    elif p.d == 1:
        act, mat = widen(gy, p.act_ld), widen(wt.transpose(3, 1, 2, 0), p.mat_ld)
    else:
        act, mat = widen(x, p.act_ld), gy
    return dict(x=x, wt=wt, gy=gy, act=act, mat=mat)


def reference(p, ops, device="cpu"):
    """Float64 result of problem ``p`` in the kernel's output layout (``out_shape``), from ``F.conv2d`` and autograd in
    double on ``device``; returned on that device."""
    x = torch.from_numpy(ops["x"]).to(device).double().permute(0, 3, 1, 2).requires_grad_(p.d == 1)
    w = torch.from_numpy(ops["wt"]).to(device).double().permute(0, 3, 1, 2).requires_grad_(p.d == 2)
    y = torch.nn.functional.conv2d(x, w, None, p.stride, p.pad)
    if p.d == 0:
        return y.detach().permute(0, 2, 3, 1).contiguous()
    gy = torch.from_numpy(ops["gy"]).to(device).double().permute(0, 3, 1, 2)
    (g,) = torch.autograd.grad(y, x if p.d == 1 else w, gy)
    return g.permute(0, 2, 3, 1).contiguous()


def dead_mask(p):
    """Direction 2: boolean [k, r, s, c], True at the entries of taps that never meet data (not written by the kernels)."""
    m = np.ones((p.k, p.r, p.s, p.c), bool)
    for r, q in live_taps(p):
        m[:, r, q, :] = False
    return m


# ---- BatchNorm partial sums of the BNSUM epilogue ------------------------------------------------------------------------
def bn_operands(p):
    """``x`` [rows, k] integers in [-3, 3] (the layer's recorded output), ``mean`` [k] integers in [-2, 2], ``rstd`` [k]
    from {0.5, 1, 2}: xhat = (x - mean) * rstd is exact in fp32, a multiple of 0.5 of magnitude <= 10."""
    rng = np.random.RandomState(_seed("bn", *p[:10]))
    oh, ow = out_hw(p)
    rows = p.n * oh * ow
    return dict(x=_ints(rng, (rows, p.k)), mean=_ints(rng, (p.k,), -2, 2),
                rstd=np.asarray([0.5, 1.0, 2.0], np.float32)[rng.randint(0, 3, size=p.k)])


def bn_partial_ref(t, bn):
    """Per 64-row tile of ``t`` [rows, k] (float64 numpy: one split's partial output, or the whole output) the column
    sums ``(sum t, sum t * xhat)``, each [ceil(rows / 64), k] float64."""
    xhat = (bn["x"].astype(np.float64) - bn["mean"].astype(np.float64)) * bn["rstd"].astype(np.float64)
    rows, k = t.shape
    tiles = -(-rows // 64)
    pad = np.zeros((tiles * 64 - rows, k))
    t1 = np.concatenate([t, pad]).reshape(tiles, 64, k)
    tx = np.concatenate([t * xhat, pad]).reshape(tiles, 64, k)
    return t1.sum(1), tx.sum(1)


def bn_exact(p):
    """64 rows of |t| <= 9 * L times |xhat| <= 10, in units of 0.5: the column sums are exact in fp32."""
    return 64 * reduction_length(p) * VMAX * VMAX * 10 * 2 < EXACT_LIMIT


# ---- the launchers' dispatch, mirrored -------------------------------------------------------------------------------------
def _nt(info, cls_kernel=None):
    """Name of the NT body a forward / data-gradient problem runs; ``cls_kernel``: inside a merged kernel, whether that
    kernel is a CLS instantiation (a problem without classes then runs the CLS body in plain enumeration)."""
    cfg = CONFIGS[info["config"]]
    if info["scalar"]:
        return "nt<scalar,Small>"
    cls = info["ncls"] > 0 if cls_kernel is None else cls_kernel
    return "nt<%s%s>%s" % (cfg, ",CLS" if cls else "", ":plain" if cls and not info["ncls"] else "")


def _tn(info):
    return "tn<scalar,Small>" if info["scalar"] else "tn<%s>" % CONFIGS[info["config"]]


def instantiations(case, infos):
    """The kernel instantiation a case launches, and inside the merged kernels the body of each problem: what
    ``launch_one`` / ``launch_dw`` / ``launch_group`` of hf_conv.hip dispatch for these plan infos (``infos``: one dict of
    ``_lib.conv_plan_info`` per problem)."""
    dirs = [p.d for p in case.problems]
    if case.form in ("slabs", "tickets"):
        return {"k_conv_" + (_nt(infos[0]) if dirs[0] <= 1 else _tn(infos[0]))}
    big = int(any(i["config"] for i in infos))
    if case.form in ("backward", "backward_slabs", "dw_slabs"):
        cls = int(infos[0]["ncls"] > 0)
        kernel = "k_conv_dw<ANYBIG=%d,CLS=%d>" % (big, cls)
        return {kernel, kernel + "/" + _nt(infos[0], bool(cls)), kernel + "/" + _tn(infos[1])}
    if case.form == "group_slabs_bnsum":
        if len(infos) == 1 and case.sums[0]:
            return {"k_conv_nt<Small,BNSUM>"}
        return {"k_conv_group<BNSUM>"} | {"k_conv_group<BNSUM>/" + ("nt<Small,BNSUM>" if s else "nt<Small>")
                                          for s in case.sums}
    assert case.form == "group_slabs"
    cls = int(any(i["ncls"] > 0 for i in infos))
    kernel = "k_conv_group<ANYBIG=%d,CLS=%d>" % (big, cls)
    out = {kernel, "%s/%d problems" % (kernel, len(infos))}
    for slot, (d, i) in enumerate(zip(dirs, infos)):
        body = _tn(i) if d == 2 else _nt(i, bool(cls))
        out |= {kernel + "/" + body, "k_conv_group/slot %d %s" % (slot, "tn" if d == 2 else "nt")}
    return out


def ring_phases(case, infos):
    """Per problem on the hand-counted prefetch ring (the vector bodies): (body, configuration, steps of the FIRST split)
    -- the ring's end phase is decided by the step count of a workgroup modulo 3, its short forms by counts below 3.
    With residue classes every class has its own count: all of them are reported."""
    out = set()
    for p, i in zip(case.problems, infos):
        if i["scalar"]:
            continue
        body = "tn" if p.d == 2 else "nt"
        if i["ncls"]:
            csteps = i["steps"] // max(i["cls_taps"])
            counts = {-(-(t * csteps) // i["splits"]) for t in i["cls_taps"]}
        else:
            counts = {-(-i["steps"] // i["splits"])}
        out |= {(body, CONFIGS[i["config"]], c) for c in counts}
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------
MB = 1 << 20
_CLS = (8, 16, 16, 8, 8)               # 2048 pixels: the threshold of the residue-class enumeration
_T = (4, 6, 6, 64, 24, 3, 3, 1, 1)     # the ticket-mode workhorse: 144 rows = 3 row tiles, 18 steps
_BIG = (8, 32, 32, 176, 128, 3, 3, 1, 1)  # 8192 rows, 64 tiles of 128 x 128, 99 steps
_S = (4, 6, 6, 16, 24, 3, 3, 1, 1)     # a Small layer for the merged forms: 144 rows, 9 taps

# problems that several cases share
D_S, W_S, F_S = P(1, *_S), P(2, *_S), P(0, *_S)
D_CLS, W_CLS = P(1, *_CLS, 3, 3, 2, 1), P(2, *_CLS, 3, 3, 2, 1)
D_96, W_96 = P(1, 8, 32, 32, 96, 96, 3, 3, 1, 1), P(2, 8, 32, 32, 96, 96, 3, 3, 1, 1)
D_BIGCLS, W_BIGCLS = P(1, 8, 32, 32, 128, 384, 3, 3, 2, 1), P(2, 8, 32, 32, 128, 384, 3, 3, 2, 1)
F_BIG = P(0, *_BIG)
W_DEAD = P(2, 4, 2, 2, 16, 16, 3, 3, 2, 1)
F_BN36, F_BN200, F_BN1568 = P(0, 4, 3, 3, 32, 96, 3, 3, 1, 1), P(0, 8, 5, 5, 32, 96, 1, 1), P(0, 32, 7, 7, 16, 64, 3, 3, 1, 1)

# expectations of the shared problems
E_D_S, E_W_S, E_F_S = E(0, 3, 3, 9), E(0, 2, 3, 9), E(0, 3, 3, 9)
E_D_CLS, E_W_CLS = E(0, 2, 2, 9, (1, 2, 2, 4)), E(0, 8, 2, 9)
E_D_96, E_W_96 = E(0, 1, 27, 9), E(3, 64, 8, 9)
E_D_BIGCLS, E_W_BIGCLS = E(1, 8, 12, 9, (1, 2, 2, 4)), E(0, 3, 22, 9)
E_F_BIG = E(1, 8, 13, 9)
E_W_DEAD = E(0, 1, 1, 4)
E_F_BN36, E_F_BN200, E_F_BN1568 = E(0, 3, 3, 9), E(0, 1, 1, 1), E(0, 3, 3, 9)


def _one(name, problem, expect, tickets=None):
    return Case(name, "tickets" if tickets else "slabs", (problem,), (expect,), tickets, None)


def _cases():
    c = [
        # -- k_conv_nt: forward and data gradient
        _one("nt_small_one_step_one_tile", P(0, 2, 4, 4, 32, 8, 1, 1), E(0, 1, 1, 1)),
        _one("nt_small_one_output_row", P(0, 1, 3, 3, 4, 4, 3, 3), E(0, 3, 3, 9)),
        _one("nt_big", F_BIG, E_F_BIG),
        _one("nt_big96", P(0, 8, 32, 32, 176, 96, 3, 3, 1, 1), E(2, 8, 13, 9)),
        _one("nt_big_dgrad", P(1, 8, 32, 32, 128, 176, 3, 3, 1, 1), E(1, 8, 13, 9)),
        _one("nt_scalar_forward", P(0, 3, 8, 8, 3, 6, 3, 3, 1, 1), E(0, 3, 3, 9, scalar=1)),
        _one("nt_scalar_dgrad", P(1, 3, 8, 8, 3, 6, 3, 3, 1, 1), E(0, 3, 3, 9, scalar=1)),
        _one("nt_scalar_forward_c49", P(0, 200, 1, 1, 49, 8, 1, 1), E(0, 1, 2, 1, scalar=1)),
        _one("nt_scalar_dgrad_k49", P(1, 200, 1, 1, 8, 49, 1, 1), E(0, 1, 2, 1, scalar=1)),
        # -- k_conv_tn: weight gradient
        _one("tn_small_dead_taps", W_DEAD, E_W_DEAD),
        _one("tn_small_ragged", P(2, 3, 5, 7, 12, 20, 3, 2, (2, 1), (1, 0)), E(0, 1, 2, 6)),
        _one("tn_scalar", P(2, 3, 8, 8, 3, 6, 3, 3, 1, 1), E(0, 3, 2, 9, scalar=1)),
        _one("tn_big", P(2, 8, 32, 32, 256, 128, 3, 3, 1, 1), E(1, 29, 18, 9)),
        _one("tn_big96", P(2, 8, 32, 32, 192, 128, 3, 3, 1, 1), E(2, 29, 18, 9)),
        _one("tn_flat96", W_96, E_W_96),
        _one("tn_flat96_two_row_tiles", P(2, 8, 32, 32, 48, 192, 3, 3, 1, 1), E(3, 64, 8, 9)),
        _one("tn_flat96_strided", P(2, 32, 32, 32, 96, 96, 3, 3, 2, 1), E(3, 64, 8, 9)),
        _one("tn_flat96_tickets", P(2, 16, 32, 32, 96, 96, 3, 3, 1, 1), E(3, 64, 16, 9), (32 * MB, 8192, 0)),
        # -- residue classes of strided data gradients on 64 x 64 tiles
        _one("cls_3x3_s2_p1", D_CLS, E_D_CLS),
        _one("cls_3x3_s2_p0", P(1, *_CLS, 3, 3, 2, 0), E(0, 2, 2, 9, (4, 2, 2, 1))),
        _one("cls_1x1_s2_empty_classes", P(1, *_CLS, 1, 1, 2, 0), E(0, 1, 1, 1, (1, 0, 0, 0))),
        _one("cls_2x2_s2", P(1, *_CLS, 2, 2, 2, 0), E(0, 1, 1, 4, (1, 1, 1, 1))),
        _one("cls_5x5_s2", P(1, *_CLS, 5, 5, 2, 2), E(0, 3, 3, 25, (9, 6, 6, 4))),
        _one("cls_stride_2_1", P(1, *_CLS, 3, 3, (2, 1), 1), E(0, 3, 2, 9, (3, 6))),
        _one("cls_stride_1_3", P(1, *_CLS, 3, 3, (1, 3), 1), E(0, 1, 3, 9, (3, 3, 3))),
        _one("cls_stride_3_1", P(1, 8, 18, 16, 8, 8, 3, 3, (3, 1), 1), E(0, 1, 3, 9, (3, 3, 3))),
        _one("cls_1x3_stride_4_1", P(1, *_CLS, 1, 3, (4, 1), (0, 1)), E(0, 1, 3, 3, (3, 0, 0, 0))),
        _one("cls_odd_sizes", P(1, 9, 15, 17, 8, 12, 3, 3, 2, 1), E(0, 2, 2, 9, (1, 2, 2, 4))),
        _one("cls_below_threshold", P(1, 7, 16, 16, 8, 8, 3, 3, 2, 1), E(0, 3, 3, 9)),
        # -- ... on the 128-wide tiles
        _one("cls_big", D_BIGCLS, E_D_BIGCLS),
        _one("cls_big96", P(1, 8, 32, 32, 96, 384, 3, 3, 2, 1), E(2, 8, 12, 9, (1, 2, 2, 4))),
        _one("cls_big_two_classes", P(1, 8, 32, 32, 128, 256, 3, 3, (2, 1), 1), E(1, 8, 12, 9, (3, 6))),
        _one("cls_big_empty_classes_8_splits", P(1, 8, 32, 32, 128, 1536, 1, 1, 2, 0), E(1, 8, 12, 1, (1, 0, 0, 0))),
        _one("cls_big_nosplit", P(1, 32, 32, 32, 128, 96, 3, 3, 2, 1), E(1, 1, 24, 9, (1, 2, 2, 4))),
        # -- wide operands
        _one("wide_forward", P(0, *_S, act_ld=32, mat_ld=32), E(0, 3, 3, 9)),
        _one("wide_dgrad", P(1, *_S, act_ld=48, mat_ld=48), E(0, 3, 3, 9)),
        _one("wide_wgrad", P(2, *_S, act_ld=32), E(0, 2, 3, 9)),
    ]
    # -- ring phases: 1 .. 5 steps in ONE workgroup (slab mode, the caller's single split), both vector bodies
    for steps in (1, 2, 3, 4, 5):
        c.append(_one("ring_nt_%d_steps" % steps, P(0, 2, 4, 4, 32 * steps, 8, 1, 1, splits=1), E(0, 1, steps, 1)))
        c.append(_one("ring_tn_%d_steps" % steps, P(2, 2 * steps, 4, 4, 8, 8, 3, 3, 1, 1, splits=1), E(0, 1, steps, 9)))
    # -- ticket mode: split counts 2 .. 9 (the last arriver sums slab 0, then four at a time, then the rest)
    for target, splits, per in ((6, 2, 9), (9, 3, 6), (12, 4, 5), (15, 5, 4), (18, 6, 3), (27, 9, 2)):
        c.append(_one("tickets_small_%d_splits" % splits, P(0, *_T), E(0, splits, per, 9), (4 * MB, 64, target)))
    c += [
        _one("tickets_small_cost_model", P(0, *_T), E(0, 9, 2, 9), (4 * MB, 64, 0)),
        _one("tickets_workspace_admits_2_splits", P(0, *_T), E(0, 2, 9, 9), (2 * 3 * 64 * 64 * 4 + 16, 64, 27)),
        _one("tickets_fewer_tickets_than_tiles", P(0, *_T), E(0, 1, 18, 9), (4 * MB, 2, 27)),
        _one("tickets_small_dgrad", P(1, *_S), E(0, 3, 3, 9), (4 * MB, 64, 12)),
        _one("tickets_small_wgrad", P(2, *_S), E(0, 2, 3, 9), (4 * MB, 64, 18)),
    ]
    for target, splits, per in ((128, 2, 50), (320, 5, 20), (448, 7, 15), (576, 9, 11)):
        c.append(_one("tickets_big_%d_splits" % splits, F_BIG, E(1, splits, per, 9), (64 * MB, 64, target)))
    c.append(_one("tickets_big96_6_splits", P(0, 8, 32, 32, 176, 96, 3, 3, 1, 1), E(2, 6, 17, 9), (64 * MB, 64, 384)))
    # -- k_conv_dw: a data gradient and a weight gradient in one launch
    c += [
        Case("pair_tickets_small", "backward", (D_S, W_S), (E(0, 3, 3, 9), E(0, 2, 3, 9)), (4 * MB, 128, 12), None),
        Case("pair_small", "dw_slabs", (D_S, P(2, *_S, act_ld=32)), (E_D_S, E_W_S), None, None),
        Case("pair_small_cls", "backward_slabs", (D_CLS, W_CLS), (E_D_CLS, E_W_CLS), None, None),
        Case("pair_anybig_small_and_flat96", "dw_slabs", (D_96, W_96), (E_D_96, E_W_96), None, None),
        Case("pair_anybig_cls_big_and_small", "backward_slabs", (D_BIGCLS, W_BIGCLS), (E_D_BIGCLS, E_W_BIGCLS), None,
             None),
        # -- k_conv_group: 1 .. 4 problems
        Case("group_1_small", "group_slabs", (W_DEAD,), (E_W_DEAD,), None, None),
        Case("group_4_small", "group_slabs", (F_S, D_S, P(0, 2, 4, 4, 32, 8, 1, 1), W_S),
             (E_F_S, E_D_S, E(0, 1, 1, 1), E_W_S), None, None),
        Case("group_2_cls_with_plain", "group_slabs", (W_CLS, D_CLS), (E_W_CLS, E_D_CLS), None, None),
        Case("group_3_cls_with_plain_nt", "group_slabs", (D_CLS, W_S, F_S), (E_D_CLS, E_W_S, E_F_S), None, None),
        Case("group_3_anybig_with_small", "group_slabs", (F_BIG, D_S, W_96), (E_F_BIG, E_D_S, E_W_96), None, None),
        Case("group_3_anybig_cls", "group_slabs", (W_BIGCLS, F_S, D_BIGCLS), (E_W_BIGCLS, E_F_S, E_D_BIGCLS), None,
             None),
        # -- BNSUM: tangent convolutions that also write the BatchNorm partial sums
        Case("bnsum_single_36_rows", "group_slabs_bnsum", (F_BN36,), (E_F_BN36,), None, (True,)),
        Case("bnsum_single_200_rows_96_columns", "group_slabs_bnsum", (F_BN200,), (E_F_BN200,), None, (True,)),
        Case("bnsum_single_1568_rows", "group_slabs_bnsum", (F_BN1568,), (E_F_BN1568,), None, (True,)),
        Case("bnsum_group_mixed", "group_slabs_bnsum", (F_S, F_BN36, F_BN200), (E_F_S, E_F_BN36, E_F_BN200), None,
             (False, True, True)),
        Case("bnsum_group_without_sums_first", "group_slabs_bnsum", (F_BN200, F_S), (E_F_BN200, E_F_S), None,
             (True, False)),
    ]
    return c


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def scratch_of(case, idx):
    """Ticket mode: (workspace bytes, ticket counters, target_blocks) that problem ``idx`` of the case plans with --
    ``hf_conv2d_nhwc_backward`` gives each half of the pair half of the workspace (rounded down to 16 bytes) and half of
    the counters."""
    ws_bytes, n_tickets, target = case.tickets
    if case.form == "backward":
        return (ws_bytes // 2) & ~15, n_tickets // 2, target
    return ws_bytes, n_tickets, target


def plan_infos(case, conv_plan_info):
    """The planner's answer for every problem of the case; ``conv_plan_info``: ``_lib.conv_plan_info``."""
    out = []
    for idx, p in enumerate(case.problems):
        kw = dict(splits=p.splits, act_ld=p.act_ld, mat_ld=p.mat_ld)
        if case.tickets:
            ws_bytes, n_tickets, target = scratch_of(case, idx)
            kw.update(tickets=(ws_bytes, n_tickets), target_blocks=target)
        out.append(conv_plan_info(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad, **kw))
    return out
