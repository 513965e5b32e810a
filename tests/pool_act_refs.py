"""float64 references of the pooled-layer kernels (``hf_pool_act_tangent_nhwc`` / ``hf_pool_act_adjoint_nhwc``,
include/hf_pcg.h), written from the header's formulas with explicit loops -- no autograd, no ``max_pool2d`` backward --
and the seeded operands of their tests.  ``test_pool_act_refs_cpu.py`` anchors both to ``torch.autograd.functional``'s
``jvp`` / ``vjp`` of ``max_pool2d(relu(a + b))``.

Layouts are the kernels': NHWC, ``idx`` int [n, oh, ow, c] holding the flat position ``y*w + x`` of the window's maximum."""

import numpy as np
import torch

GEOMS = [(2, 2, 0), (3, 2, 0), (3, 2, 1), (2, 1, 0), (3, 3, 1)]  # (kernel, stride, padding)
MAPS = [(5, 7), (4, 4), (3, 3)]


def _transposed(geom, hw):
    return tuple((a[1], a[0]) for a in geom), (hw[1], hw[0])


# per-axis windows, ((kh, kw), (sh, sw), (ph, pw)), (h, w): every pair that differs is told from its exchange by the
# adjoint (``test_pool_act_refs_cpu.py``), and each entry is followed by its transpose, so an exchange shows both ways
AXIS_GEOMS = [e for g in [(((3, 2), (2, 1), (1, 0)), (5, 7)), (((2, 3), (2, 2), (0, 1)), (6, 5)),
                          (((1, 2), (1, 2), (0, 0)), (2, 9))] for e in (g, _transposed(*g))]


def exchanges(geom):
    """(name, geometry) for each of (kh, kw), (sh, sw), (ph, pw) of ``geom`` whose two values differ, with that pair
    exchanged: what a kernel that reads the wrong axis' parameter would take the windows to be."""
    out = []
    for j, name in enumerate(("kernel", "stride", "padding")):
        a, b = pair(geom[j])
        if a != b:
            out.append((name, tuple((b, a) if i == j else pair(g) for i, g in enumerate(geom))))
    return out


def pair(v):
    """A geometry parameter, an int (both axes) or an (h, w) pair, as the pair."""
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_hw(h, w, k, s, p):
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def _seed(*key):
    h = 1469598103934665603
    for ch in "|".join(str(x) for x in key):
        h = ((h ^ ord(ch)) * 1099511628211) % (2 ** 64)
    return h % (2 ** 31)


def eighths(gen, *shape, lim=4):
    """Multiples of 1/8 in [-lim, lim]: every sum of a few thousand of them is exact in fp32."""
    return torch.randint(-8 * lim, 8 * lim + 1, shape, generator=gen).to(torch.float32) / 8.0


def forward(a, b, k, s, p, relu=True):
    """(y_pool, idx) NHWC of ``max_pool2d(relu(a + b))`` (``a`` NHWC [n,h,w,c], ``b`` [c] or None) by ATen's forward --
    what the engine's forward launches reproduce; the pre-activations of the tests have no ties inside a window's
    positive part, so the positions are unambiguous where they matter."""
    z = a if b is None else a + b
    z = torch.relu(z) if relu else z
    y, idx = torch.nn.functional.max_pool2d(z.permute(0, 3, 1, 2), k, s, p, return_indices=True)
    return y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous()


def tangent(slabs, v_b, idx, y_pool, relu):
    """out[n,oy,ox,c] = m * (sum_s slabs[s][n, idx, c] + v_b[c]); slabs [S, n, h, w, c]; float64 (out, M): ``M`` the sum
    of the magnitudes of the terms."""
    S, n, h, w, c = slabs.shape
    _, oh, ow, _ = idx.shape
    sl = slabs.double().numpy().reshape(S, n, h * w, c)
    ix = idx.numpy()
    out = np.zeros((n, oh, ow, c))
    M = np.zeros((n, oh, ow, c))
    for ni in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for ci in range(c):
                    pos = ix[ni, oy, ox, ci]
                    t, m = 0.0, 0.0
                    for s_ in range(S):
                        t += sl[s_, ni, pos, ci]
                        m += abs(sl[s_, ni, pos, ci])
                    if v_b is not None:
                        t += float(v_b[ci])
                        m += abs(float(v_b[ci]))
                    on = (not relu) or float(y_pool[ni, oy, ox, ci]) > 0
                    out[ni, oy, ox, ci] = t if on else 0.0
                    M[ni, oy, ox, ci] = m if on else 0.0
    return torch.from_numpy(out), torch.from_numpy(M)


def adjoint(gy, idx, y_pool, relu, h, w, k, s, p, row_blocks=0):
    """ga[n,y,x,c] = sum over the windows containing (y,x) whose idx is (y,x) of m * sum_s gy[s][n,oy,ox,c]; gy
    [S, n, oh, ow, c].  Returns float64 (ga [n,h,w,c], M, gb, windows): ``gb`` [row_blocks, c] the partial rows of
    sum ga over the shares ``[b*per, (b+1)*per)`` of the n*h*w full-resolution rows, per = ceil(rows / row_blocks)
    (None for row_blocks = 0; an empty share raises), ``windows`` the largest number of windows one pixel collected.
    ``k``, ``s``, ``p``: an int or an (h, w) pair each; they enter the window predicate only."""
    S, n, oh, ow, c = gy.shape
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    g = gy.double().numpy()
    ix = idx.numpy()
    ga = np.zeros((n, h, w, c))
    M = np.zeros((n, h, w, c))
    cnt = np.zeros((n, h, w, c), dtype=np.int64)
    for ni in range(n):
        for y in range(h):
            for x in range(w):
                for oy in range(oh):
                    if not oy * sh - ph <= y <= oy * sh - ph + kh - 1:
                        continue
                    for ox in range(ow):
                        if not ox * sw - pw <= x <= ox * sw - pw + kw - 1:
                            continue
                        for ci in range(c):
                            if ix[ni, oy, ox, ci] != y * w + x:
                                continue
                            cnt[ni, y, x, ci] += 1
                            if relu and not float(y_pool[ni, oy, ox, ci]) > 0:
                                continue
                            ga[ni, y, x, ci] += g[:, ni, oy, ox, ci].sum()
                            M[ni, y, x, ci] += np.abs(g[:, ni, oy, ox, ci]).sum()
    gb = None
    if row_blocks:
        rows = n * h * w
        per = -(-rows // row_blocks)
        if (row_blocks - 1) * per >= rows:
            raise ValueError("an empty share")
        flat = ga.reshape(rows, c)
        gb = np.stack([flat[b * per:(b + 1) * per].sum(0) for b in range(row_blocks)])
        gb = torch.from_numpy(gb)
    return torch.from_numpy(ga), torch.from_numpy(M), gb, int(cnt.max())


def case(n, c, h, w, k, s, p, splits, gy_splits, exact=True, tag=""):
    """Seeded operands of one kernel case.  ``exact``: multiples of 1/8 (every sum exact in fp32), else standard normal.
    The pre-activation ``a + b`` has distinct values inside every window (a permutation of distinct multiples of 1/8
    per plane, shifted so that roughly a third of the windows' maxima are <= 0: those windows are masked).  ``k``, ``s``,
    ``p``: an int or an (h, w) pair each (an int seeds as it always did)."""
    gen = torch.Generator().manual_seed(_seed("pool-act", n, c, h, w, k, s, p, splits, gy_splits, exact, tag))
    oh, ow = out_hw(h, w, k, s, p)
    hw = h * w
    # distinct values per (n, c) plane: no ties, so ATen's positions are the only possible ones
    planes = torch.stack([torch.randperm(hw, generator=gen) for _ in range(n * c)]).view(n, c, h, w)
    z = (planes.to(torch.float32) - 0.75 * hw) / 8.0  # most of a plane is negative: whole windows stay <= 0
    z = z.permute(0, 2, 3, 1).contiguous()
    b = eighths(gen, c, lim=1)
    a = z - b  # exact: both multiples of 1/8 of small magnitude
    rnd = (lambda *sh: eighths(gen, *sh)) if exact else (lambda *sh: torch.randn(*sh, generator=gen))
    return dict(a=a, b=b, oh=oh, ow=ow, slabs=rnd(splits, n, h, w, c), v_b=rnd(c), gy=rnd(gy_splits, n, oh, ow, c))
