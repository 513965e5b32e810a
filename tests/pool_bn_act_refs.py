"""float64 references of the pooled BatchNorm unit's kernels (``hf_pool_bn_act_tangent_nhwc`` /
``hf_pool_bn_act_adjoint_nhwc``, include/hf_pcg.h), written from the header's formulas with explicit loops -- no autograd,
no ``max_pool2d`` backward -- and the seeded operands of their tests.  ``test_pool_bn_act_refs_cpu.py`` anchors both to
``torch.autograd.functional``'s ``jvp`` / ``vjp`` of ``max_pool2d(relu(batch_norm_eval(a)))`` with respect to ``a``, ``w``
and ``b``.

Layouts are the kernels': NHWC, ``idx`` int [n, oh, ow, c] holding the flat position ``y*w + x`` of the window's maximum.
The geometries, the cycling helpers and the bias form's adjoint (whose ``ga`` is this unit's unscaled ``g``) are
``pool_act_refs``'."""

import numpy as np
import torch

import pool_act_refs as R

GEOMS, MAPS, out_hw = R.GEOMS, R.MAPS, R.out_hw
AXIS_GEOMS, pair = R.AXIS_GEOMS, R.pair  # (every k / s / p below: an int or an (h, w) pair, as in ``pool_act_refs``)


def xhat(o):
    """(a - mean) * rstd, float64 [n, h, w, c]."""
    return (o["a"].double() - o["mean"].double()) * o["rstd"].double()


def forward(o, k, s, p, relu=True):
    """(y_pool, idx) NHWC of ``max_pool2d(relu?(xhat*w + b))`` in fp32 by ATen's forward (exact on the dyadic operands;
    the planes have no ties, so the positions are the only possible ones)."""
    z = ((o["a"] - o["mean"]) * o["rstd"]) * o["w"] + o["b"]
    z = torch.relu(z) if relu else z
    y, idx = torch.nn.functional.max_pool2d(z.permute(0, 3, 1, 2), k, s, p, return_indices=True)
    return y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous()


def tangent(o, v_w, v_b, idx, y_pool, relu):
    """out[n,oy,ox,c] = m * (T*(w*rstd) + xhat[n,idx,c]*v_w + v_b),  T = sum_s slabs[s][n,idx,c]; float64 (out, M): ``M``
    the sum of the magnitudes of the terms (each slab's share, the scale's and the shift's)."""
    sl = o["slabs"].double().numpy()
    S, n, h, w, c = sl.shape
    _, oh, ow, _ = idx.shape
    sl = sl.reshape(S, n, h * w, c)
    xh = xhat(o).numpy().reshape(n, h * w, c)
    sc = (o["w"].double() * o["rstd"].double()).numpy()
    ix = idx.numpy()
    out, M = np.zeros((n, oh, ow, c)), np.zeros((n, oh, ow, c))
    for ni in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for ci in range(c):
                    pos = ix[ni, oy, ox, ci]
                    t, m = 0.0, 0.0
                    for s_ in range(S):
                        t += sl[s_, ni, pos, ci]
                        m += abs(sl[s_, ni, pos, ci])
                    t, m = t * sc[ci], m * abs(sc[ci])
                    if v_w is not None:
                        t += xh[ni, pos, ci] * float(v_w[ci])
                        m += abs(xh[ni, pos, ci] * float(v_w[ci]))
                    if v_b is not None:
                        t += float(v_b[ci])
                        m += abs(float(v_b[ci]))
                    on = (not relu) or float(y_pool[ni, oy, ox, ci]) > 0
                    out[ni, oy, ox, ci] = t if on else 0.0
                    M[ni, oy, ox, ci] = m if on else 0.0
    return torch.from_numpy(out), torch.from_numpy(M)


def adjoint(o, idx, y_pool, relu, h, w, k, s, p, row_blocks=0):
    """``g`` = the bias form's ga (``pool_act_refs.adjoint``), ``ga = g * (w*rstd)``, and per share ``b`` of the n*h*w
    full-resolution rows ``gb[b] = sum g``, ``gw[b] = sum g * xhat``.  Returns float64 dict ``g, ga, M`` (sum of the
    magnitudes of g's terms), ``gw, gb`` ([row_blocks, c]; None for row_blocks = 0), ``Mw`` (sum over the share of
    M * |xhat|), ``Mb``, ``windows``."""
    g, M, gb, windows = R.adjoint(o["gy"], idx, y_pool, relu, h, w, k, s, p, row_blocks)
    n, c = g.shape[0], g.shape[3]
    sc = o["w"].double() * o["rstd"].double()
    res = dict(g=g, ga=g * sc, M=M, gb=gb, gw=None, Mw=None, Mb=None, windows=windows)
    if row_blocks:
        rows = n * h * w
        per = -(-rows // row_blocks)
        xh = xhat(o).reshape(rows, c).numpy()
        gf, Mf = g.reshape(rows, c).numpy(), M.reshape(rows, c).numpy()
        gw, Mw, Mb = np.zeros((row_blocks, c)), np.zeros((row_blocks, c)), np.zeros((row_blocks, c))
        for b in range(row_blocks):
            for r in range(b * per, min((b + 1) * per, rows)):
                for ci in range(c):
                    gw[b, ci] += gf[r, ci] * xh[r, ci]
                    Mw[b, ci] += Mf[r, ci] * abs(xh[r, ci])
                    Mb[b, ci] += Mf[r, ci]
        res.update(gw=torch.from_numpy(gw), Mw=torch.from_numpy(Mw), Mb=torch.from_numpy(Mb))
    return res


def case(n, c, h, w, k, s, p, splits, gy_splits, exact=True, tag=""):
    """Seeded operands of one kernel case.  ``exact``: dyadic -- ``a``, ``mean``, ``b``, the slabs, ``v_w``, ``v_b`` and
    ``gy`` multiples of 1/8 of magnitude <= 4, ``w`` and ``rstd`` in {0.5, 1, 2}: every product and sum of the two formulas
    is exact in fp32 --, else standard normal (``w``, ``rstd`` U[0.5, 2]).  ``a`` has distinct values inside every (n, c)
    plane (a permutation of distinct multiples of 1/8, most of them negative) and the affine map is increasing, so the
    windows' positions are unambiguous and a share of the windows' maxima is <= 0: those windows are masked."""
    gen = torch.Generator().manual_seed(R._seed("pool-bn-act", n, c, h, w, k, s, p, splits, gy_splits, exact, tag))
    oh, ow = out_hw(h, w, k, s, p)
    hw = h * w
    planes = torch.stack([torch.randperm(hw, generator=gen) for _ in range(n * c)]).view(n, c, h, w)
    a = (planes.to(torch.float32) - float(round(0.75 * hw))) / 8.0
    a = a.permute(0, 2, 3, 1).contiguous()
    if exact:
        rnd = lambda *sh: R.eighths(gen, *sh)  # noqa: E731
        pow2 = lambda: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=gen)]  # noqa: E731
        w_, rstd = pow2(), pow2()
        mean, b = R.eighths(gen, c, lim=1), R.eighths(gen, c, lim=1)
    else:
        rnd = lambda *sh: torch.randn(*sh, generator=gen)  # noqa: E731
        w_, rstd = 0.5 + 1.5 * torch.rand(c, generator=gen), 0.5 + 1.5 * torch.rand(c, generator=gen)
        mean, b = 0.5 * torch.randn(c, generator=gen), 0.5 * torch.randn(c, generator=gen)
    return dict(a=a, mean=mean, rstd=rstd, w=w_, b=b, oh=oh, ow=ow, slabs=rnd(splits, n, h, w, c), v_w=rnd(c), v_b=rnd(c),
                gy=rnd(gy_splits, n, oh, ow, c))
