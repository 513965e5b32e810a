"""Float64 references of the dense-layer kernels (``hf_dense.hip``), written from the formulas and rules in
``include/hf_pcg.h``, the error bounds the kernel tests hold them to, and the tests' inputs.  Plain module, no GPU.

Every reference computes in numpy float64 from the fp32 operands (converted exactly) and returns, next to each result,
its per-element MAGNITUDE SUM ``M`` (the same formula with every term replaced by its absolute value).  The bound of a
comparison is the forward bound ``(L + R) * u * M`` as in ``layer_refs.py``: ``L`` = the number of products summed into
the element (any order of an fp32 sum of L terms, fused or not, stays within ``L * u * sum|a_i b_i|`` to first order),
``R`` = the further roundings the header's formula spells out, ``u = 2**-24``.  The ``r_*`` functions count them."""

import numpy as np

U32 = 2.0 ** -24
KSTEP, MAX_SPLITS, MAX_ROWS = 32, 32, 256
IDENTITY, RELU, TANH = 0, 1, 2
ACTS = (IDENTITY, RELU, TANH)

# (rows, c_in, c_out): one element | odd everything | the mwe net | small_nn's last layer | just over one row tile with
# ragged columns | whole tiles | c_in over two 128-column blocks, c_out over one | one row over two tiles | full batch
SHAPES = [(1, 1, 1), (3, 7, 5), (16, 10, 10), (32, 5, 3), (33, 65, 31), (64, 128, 96), (64, 260, 132), (65, 64, 64),
          (256, 36, 68)]


# ---- the split rule of the header ----------------------------------------------------------------------------------
def kper(length, splits):
    per = -(-length // splits)
    return -(-per // KSTEP) * KSTEP


def split_ok(length, splits):
    return 1 <= splits <= MAX_SPLITS and (splits - 1) * kper(length, splits) < length


def split_counts(length, planned):
    """The counts the kernel tests run: 1, the planned one, and every count up to 5 the rule accepts."""
    return sorted({1, planned} | {s for s in range(2, 6) if split_ok(length, s)})


def split_ranges(length, splits):
    k = kper(length, splits)
    return [(s * k, min((s + 1) * k, length)) for s in range(splits)]


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ---- the GEMMs -----------------------------------------------------------------------------------------------------
def tangent_slabs(t_x, x, W, V, splits):
    """hf_dense_tangent_slabs: slab s = t_x[:, ks] W[:, ks]^T + x[:, ks] V[:, ks]^T over split s's share ``ks`` of c_in
    (a NULL ``t_x`` or ``V`` drops its term).  Returns (slabs, M, L): [splits, rows, c_out] twice and the number of
    products per element of the LONGEST split."""
    t_x, x, W, V = f64(t_x), f64(x), f64(W), f64(V)
    c_in = (W if W is not None else V).shape[1]
    out, mag = [], []
    for lo, hi in split_ranges(c_in, splits):
        s = m = 0.0
        if t_x is not None:
            s, m = s + t_x[:, lo:hi] @ W[:, lo:hi].T, m + abs(t_x[:, lo:hi]) @ abs(W[:, lo:hi]).T
        if V is not None:
            s, m = s + x[:, lo:hi] @ V[:, lo:hi].T, m + abs(x[:, lo:hi]) @ abs(V[:, lo:hi]).T
        out.append(s)
        mag.append(m)
    terms = int(t_x is not None) + int(V is not None)
    return np.stack(out), np.stack(mag), terms * min(kper(c_in, splits), c_in)


def dgrad_slabs(g, W, splits):
    """hf_dense_dgrad_slabs: slab s = g[:, ks] W[ks, :] over split s's share of c_out."""
    g, W = f64(g), f64(W)
    c_out = W.shape[0]
    out = [g[:, lo:hi] @ W[lo:hi] for lo, hi in split_ranges(c_out, splits)]
    mag = [abs(g[:, lo:hi]) @ abs(W[lo:hi]) for lo, hi in split_ranges(c_out, splits)]
    return np.stack(out), np.stack(mag), min(kper(c_out, splits), c_out)


R_SLAB = 3  # the four waves' partial sums are joined by three more additions


def wgrad(g, x, scale):
    """hf_dense_wgrad: scale * g^T x with ``scale`` rounded to fp32; L = rows, R = 1 (the multiplication)."""
    g, x, sc = f64(g), f64(x), float(np.float32(scale))
    return sc * (g.T @ x), abs(sc) * (abs(g).T @ abs(x)), g.shape[0]


R_WGRAD = 1


# ---- the elementwise passes ----------------------------------------------------------------------------------------
def act_factor(y, act):
    """act'(y) and its magnitude: relu ``y > 0``; tanh ``1 - y*y`` (|1| + |y*y|)."""
    if act == IDENTITY:
        return 1.0, 1.0
    y = f64(y)
    if act == RELU:
        d = (y > 0).astype(np.float64)
        return d, d
    return 1.0 - y * y, 1.0 + y * y


def r_act(splits, has_b, act):
    """Roundings: slab additions, the bias addition; tanh adds y*y, 1 - (.), s * (.); the relu mask is exact."""
    return (splits - 1) + int(has_b) + (3 if act == TANH else 0) or 1


def act_tangent(slabs, v_b, y, act):
    """hf_dense_act_tangent: (sum of slabs + v_b[col]) * act'(y)."""
    slabs = f64(slabs)
    s, m = slabs.sum(0), abs(slabs).sum(0)
    if v_b is not None:
        s, m = s + f64(v_b)[None, :], m + abs(f64(v_b))[None, :]
    d, md = act_factor(y, act)
    return s * d, m * md


def act_adjoint(slabs, y, act, scale):
    """hf_dense_act_adjoint: g_a = (sum of slabs) * act'(y); g_b = scale * column sums of g_a (scale rounded to fp32).
    Returns (g_a, M_a, g_b, M_b)."""
    slabs = f64(slabs)
    d, md = act_factor(y, act)
    ga, ma = slabs.sum(0) * d, abs(slabs).sum(0) * md
    sc = float(np.float32(scale))
    return ga, ma, sc * ga.sum(0), abs(sc) * ma.sum(0)


def r_bias(splits, act):
    """g_b: every g_a carries r_act roundings; the fp64 column sum adds rows * 2**-53 (counted as one fp32 rounding, far
    more than it is), then the rounding to fp32 and the multiplication by scale."""
    return r_act(splits, False, act) + 3


def ratio(got, want, M, R):
    """max |got - want| / (R u M); where the bound is zero the element must be exact."""
    got, want = f64(got), f64(want)
    M = np.broadcast_to(f64(M), want.shape)
    err, bound = abs(got - want), R * U32 * M
    if got.shape != want.shape or not np.isfinite(err).all() or ((bound == 0) & (err > 0)).any():
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- the tests' inputs ---------------------------------------------------------------------------------------------
def case(rows, c_in, c_out, seed=0):
    """fp32 operands of one layer, from a seed: activations / tangents / cotangents of unit scale, weights of scale
    1/sqrt(c_in), pre-activations that the three activations turn into the layer output ``y``."""
    g = np.random.default_rng(1000 * seed + 7 * rows + 3 * c_in + c_out)
    f = lambda *sh, s=1.0: (s * g.standard_normal(sh)).astype(np.float32)  # noqa: E731
    c = dict(t_x=f(rows, c_in), x=f(rows, c_in), W=f(c_out, c_in, s=c_in ** -0.5), V=f(c_out, c_in, s=c_in ** -0.5),
             g=f(rows, c_out), v_b=f(c_out), pre=f(rows, c_out), scale=0.37)
    c["y"] = {IDENTITY: c["pre"], RELU: np.maximum(c["pre"], 0), TANH: np.tanh(c["pre"]).astype(np.float32)}
    return c


def slabs_for(shape, splits, seed=1):
    """Random fp32 slabs [splits, rows, c] for the elementwise passes."""
    g = np.random.default_rng(seed + 31 * splits + shape[0] + shape[1])
    return g.standard_normal((splits,) + tuple(shape)).astype(np.float32)
