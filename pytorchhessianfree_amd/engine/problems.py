"""The one place a layer launch of the conv-unit engines is described: per struct kind of include/hf_pcg.h ONE builder
that fills the struct (from a unit; a convolution's from its operands and its ``Geometry``), and one ``*_args`` function
that takes a filled struct apart into the positional argument list (without ``dtype, stream``) of the one-problem entry
point.  The one-problem form launches ``*_args(problem)``, the array forms a list of the same problems (``_Launcher``).

Nothing here touches the device: a unit is anything with the attributes read below."""

from collections import namedtuple

from .. import _lib


class Geometry(namedtuple("Geometry", "n h w c k r s stride padding")):
    """A convolution's geometry: input [n, h, w, c] (NHWC), ``k`` filters of ``r`` x ``s`` taps, ``stride`` and ``padding``
    per axis as (along h, along w)."""

    __slots__ = ()

    def doubled(self):
        """Over the ``[t_x | x]`` operand: twice the input channels."""
        return self._replace(c=2 * self.c)

    def with_n(self, n):
        """The same layer on ``n`` samples (rows, for an im2col'd layer)."""
        return self._replace(n=n)

    def dims(self):
        """``n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w``: as every positional entry point lists them."""
        return self[:7] + (self.stride[0], self.stride[1], self.padding[0], self.padding[1])


_DIMS = ("n", "h", "w", "c", "k", "r", "s", "stride_h", "stride_w", "pad_h", "pad_w")  # ... and hf_conv_problem names them


def problem(kind, **fields):
    """A problem struct from named fields: tensors go as their addresses, what is not named stays NULL / 0."""
    return kind(**{k: (v.data_ptr() if hasattr(v, "data_ptr") else v) for k, v in fields.items()})


def sources(name, srcs):
    """``(a, a_splits, a_slab, b, b_splits, b_slab)`` of the one or two ``(tensor, splits, slab stride)`` cotangents of a
    unit's output."""
    if not 1 <= len(srcs) <= 2:
        raise RuntimeError(f"{name}: {len(srcs)} consumers")
    return tuple(srcs[0]) + (tuple(srcs[1]) if len(srcs) == 2 else (None, 1, 0))


def _nchw(u):
    n, k, oh, ow = u.a.shape
    return dict(n=n, c=k, hw=oh * ow)


# ---- hf_affine_problem: the eval-mode tangent -----------------------------------------------------------------
def affine_problem(u, vq, vr, add=None, add_ld=0):
    """t_y = mask * (sum(T slabs) * w*rstd + xhat * vq + vr + add), into the consumer's operand (``vq`` / ``vr``: the
    scale's / shift's slice of ``v``, None where frozen)."""
    return problem(_lib.AffineProblem, out=u.tout, a=u.tbuf, x=u.a, mean=u.mean, rstd=u.rstd, w=u.scale, q=vq, r=vr,
                   add=add, mask_src=u.y if u.relu else None, out_ld=u.tout_ld, add_ld=add_ld, a_splits=u.sT,
                   a_slab=u.tbuf.shape[1], **_nchw(u))


def affine_args(q, channels_last=1):
    """``hf_chan_affine_ex``."""
    return (q.out, q.a, q.x, q.mean, q.rstd, q.w, q.q, q.r, q.add, q.mask_src, q.relu_self, q.n, q.c, q.hw,
            channels_last, q.out_ld, q.add_ld, q.a_splits, q.a_slab)


# ---- hf_affine_train_problem: the train-mode elementwise pass (tangent and adjoint) ------------------------------
def affine_train_problem(u, out, out_ld, a, a_splits, a_slab, parts, vq=None, vr=None, mask=None, add=None):
    """``parts``: (partial rows of S_x, of S_1, their count).  ``add`` only in the one-problem form."""
    n, k, oh, ow = u.a.shape
    return problem(_lib.AffineTrainProblem, out=out, a=a, x=u.a, mean=u.mean, rstd=u.rstd, w=u.scale, part_x=parts[0],
                   part_1=parts[1], nparts=parts[2], vq=vq, vr=vr, count=float(n * oh * ow), add=add, mask_src=mask,
                   out_ld=out_ld, a_splits=a_splits, a_slab=a_slab, **_nchw(u))


def affine_train_args(q, add_ld=0):
    """``hf_chan_affine_train``."""
    return (q.out, q.a, q.x, q.mean, q.rstd, q.w, q.part_x, q.part_1, q.nparts, q.vq, q.vr, q.count, q.add, q.mask_src,
            q.n, q.c, q.hw, q.out_ld, add_ld, q.a_splits, q.a_slab)


# ---- hf_bn_adjoint_problem: the adjoint (fused, elementwise, train reduction) and the plain row reductions ---------
def bn_adjoint_problem(u, srcs, ga=None, reduce=False, only_needed=False):
    """g = mask * (sum of the cotangents' slabs) -> u.g;  g * w*rstd -> ``ga`` (default ``u.ga``);  per-channel sums ->
    u.gw / u.gb.  ``reduce``: the train-mode reduction pass, no ``ga``.  ``only_needed`` (the fused one-problem launch):
    gw and x only with a BatchNorm, gb only with a trainable shift, g only where ``u.needs_g``; otherwise all four."""
    a, sa, la, b, sb, lb = sources(u.name, srcs)
    bn = u.bn is not None or not only_needed
    return problem(_lib.BnAdjointProblem, gx=None if reduce else (u.ga if ga is None else ga),
                   gw=u.gw if bn else None, gb=u.gb if u.pb is not None or not only_needed else None,
                   gres=u.g if u.needs_g or not only_needed else None, gy=a, gy_splits=sa, gy_slab=la, gy2=b,
                   gy2_splits=sb, gy2_slab=lb, x=u.a if bn else None, mean=u.mean, rstd=u.rstd, w=u.scale,
                   mask_src=u.y if u.relu else None, row_blocks=u.rb, **_nchw(u))


def chan_sums_problem(gy, splits, slab, n, c, hw, row_blocks, gw=None, gb=None, x=None, mean=None, rstd=None):
    """A plain per-channel reduction of ``gy``'s slabs by the adjoint's kernel:  gb = sum_rows gy,  gw = sum_rows gy * xhat
    with xhat = (x - mean) * rstd; ``row_blocks`` partial rows each."""
    return problem(_lib.BnAdjointProblem, gw=gw, gb=gb, gy=gy, gy_splits=splits, gy_slab=slab, gy2_splits=1, x=x,
                   mean=mean, rstd=rstd, n=n, c=c, hw=hw, row_blocks=row_blocks)


def bn_adjoint_args(q, channels_last=1):
    """``hf_chan_affine_bwd_ex``."""
    return (q.gx, q.gw, q.gb, q.gres, q.gy, q.gy_splits, q.gy_slab, q.gy2, q.gy2_splits, q.gy2_slab, q.x, q.mean, q.rstd,
            q.w, q.mask_src, q.n, q.c, q.hw, channels_last, q.row_blocks)


def bn_adjoint_v4_args(q):
    """``hf_bn_adjoint_v4``: the elementwise part (gres -> g_out, gx -> ga_out); the sums' fields are not read."""
    return (q.gres, q.gx, q.gy, q.gy_splits, q.gy_slab, q.gy2, q.gy2_splits, q.gy2_slab, q.mask_src, q.w, q.rstd,
            q.n * q.hw, q.c)


# ---- GroupNorm units (hf_gn.hip; positional entry points, no struct) ---------------------------------------------------
def _gn_dims(u):
    n, k, oh, ow = u.a.shape
    return n, oh * ow, k, u.gn.num_groups


def gn_forward_args(u, a, splits, slab, a_out=None, conv_bias=None):
    """``hf_gn_forward``: statistics and ``y = act(gamma * xhat + beta)`` from the slabs ``a`` (+ the convolution's bias),
    into ``u.y`` and the x half of the consumer's operand; the summed map -> ``a_out``.  ``splits = 1`` on a given map,
    no ``a_out``: the statistics and the output of that map."""
    k = u.a.shape[1]
    return (u.y, u.yout2, 2 * k if u.yout2 is not None else 0, a_out, u.gn_mean, u.gn_rstd, a, splits, slab, conv_bias,
            u.gn.weight, u.gn.bias, float(u.gn.eps), 1 if u.relu else 0, *_gn_dims(u))


def gn_tangent_args(u, v_cb, vg, vb):
    """``hf_gn_act_tangent``: the unit's tangent from the tangent convolution's slabs into the consumer's operand; ``v_cb`` /
    ``vg`` / ``vb``: the convolution bias's, the scale's and the shift's slice of ``v`` (None where frozen)."""
    return (u.tout, u.tout_ld, u.tbuf, u.sT, u.tbuf.shape[1], v_cb, u.a, u.gn_mean, u.gn_rstd, u.gn.weight, vg, vb,
            u.y if u.relu else None, *_gn_dims(u))


def gn_adjoint_args(u, srcs):
    """``hf_gn_act_adjoint``: ``u.ga`` (and ``u.g`` where the unit keeps it) from the one cotangent of the unit's output, and
    the per-sample rows of the trainable ones among scale, shift and convolution bias."""
    (gy, splits, slab), = srcs
    return (u.ga, u.g if u.needs_g else None, u.gw if u.pg is not None else None, u.gb if u.pb is not None else None,
            u.gcb if u.pcb is not None else None, gy, splits, slab, u.a, u.gn_mean, u.gn_rstd, u.gn.weight,
            u.y if u.relu else None, *_gn_dims(u))


def gn_adjoint2_args(u, srcs, v_cb, v_gamma):
    """``hf_gn_act_adjoint2``: inside a Hessian product, ``u.gah`` and the second-order rows of the trainable ones among
    scale, shift and convolution bias from the second sweep's cotangent ``srcs``, the tangent convolution's slabs (still in
    ``u.tbuf``) and the step's first-order masked cotangent ``u.g1``; ``v_cb`` / ``v_gamma``: the vector's slices, None where
    frozen."""
    (gy, splits, slab), = srcs
    return (u.gah, u.gw if u.pg is not None else None, u.gb if u.pb is not None else None,
            u.gcb if u.pcb is not None else None, gy, splits, slab, u.tbuf, u.sT, u.tbuf.shape[1], v_cb, u.a, u.g1,
            u.gn_mean, u.gn_rstd, u.gn.weight, v_gamma, u.y if u.relu else None, *_gn_dims(u))


def gn_split_stats_args(u, a, splits, slab, a_out=None, conv_bias=None):
    """``hf_gn_split_stats``: the parts' partial statistics of the slabs ``a`` (+ the convolution's bias) into ``u.gn_tab``;
    the summed map -> ``a_out``."""
    return (a_out, u.gn_tab, a, splits, slab, conv_bias, *_gn_dims(u))


def gn_split_forward_args(u, s):
    """``hf_gn_split_forward``: the statistics from ``u.gn_tab`` and the unit's output from the summed map ``s``."""
    k = u.a.shape[1]
    return (u.y, u.yout2, 2 * k if u.yout2 is not None else 0, u.gn_mean, u.gn_rstd, s, u.gn_tab, u.gn.weight, u.gn.bias,
            float(u.gn.eps), 1 if u.relu else 0, *_gn_dims(u))


def gn_split_tangent_args(u, v_cb, vg, vb):
    """``hf_gn_split_tangent_sums`` and ``hf_gn_split_act_tangent``: the tangent convolution's sum raw into the consumer's
    operand and its partial sums into ``u.gn_tab``; then the operand rewritten in place."""
    return ((u.tout, u.tout_ld, u.gn_tab, u.tbuf, u.sT, u.tbuf.shape[1], v_cb, u.a, u.gn_mean, u.gn_rstd, *_gn_dims(u)),
            (u.tout, u.tout_ld, u.gn_tab, u.a, u.gn_mean, u.gn_rstd, u.gn.weight, vg, vb, u.y if u.relu else None,
             *_gn_dims(u)))


def gn_split_adjoint_args(u, srcs):
    """``hf_gn_split_adjoint_sums`` and ``hf_gn_split_act_adjoint``: the masked cotangent into ``u.g`` where the unit keeps
    it (else into ``u.ga``, which the second launch rewrites in place), the parts' rows of scale and shift; then ``u.ga``
    and the parts' rows of the convolution bias."""
    (gy, splits, slab), = srcs
    g = u.g if u.needs_g else u.ga
    return ((g, u.gn_tab, u.gw if u.pg is not None else None, u.gb if u.pb is not None else None, gy, splits, slab, u.a,
             u.gn_mean, u.gn_rstd, u.gn.weight, u.y if u.relu else None, *_gn_dims(u)),
            (u.ga, u.gcb if u.pcb is not None else None, g, u.gn_tab, u.a, u.gn_mean, u.gn_rstd, u.gn.weight, *_gn_dims(u)))


def gn_split_adjoint2_args(u, srcs, v_cb, v_gamma):
    """``hf_gn_split_adjoint2_sums`` and ``hf_gn_split_act_adjoint2``: ``gn_adjoint2_args``'s operands for a split unit.  The
    masked cotangent goes to ``u.gah`` (which the second launch rewrites in place) and the tangent convolution's sum to
    ``u.gn_t2``; the parts' five sums to ``u.gn_tab2`` -- E[t] and E[xh t] come from ``u.gn_tab``, where the tangent sweep of
    this product left them --, the parts' rows of scale and shift; then ``u.gah`` and the convolution bias's rows."""
    (gy, splits, slab), = srcs
    return ((u.gah, u.gn_t2, u.gn_tab2, u.gw if u.pg is not None else None, u.gb if u.pb is not None else None, gy, splits,
             slab, u.tbuf, u.sT, u.tbuf.shape[1], v_cb, u.gn_tab, u.a, u.g1, u.gn_mean, u.gn_rstd, u.gn.weight, v_gamma,
             u.y if u.relu else None, *_gn_dims(u)),
            (u.gah, u.gcb if u.pcb is not None else None, u.gah, u.gn_t2, u.gn_tab2, u.gn_tab, u.a, u.g1, u.gn_mean,
             u.gn_rstd, u.gn.weight, v_gamma, *_gn_dims(u)))


def gn_rows_sqsum_args(u, out, offs, pre):
    """``hf_gn_rows_sqsum`` (a split unit: ``hf_gn_split_rows_sqsum``): the unit's entries of ``diag_ef`` straight into ``out`` (``offs``: the parameters' offsets) from
    the per-sample rows the adjoint launch left, each scaled by ``pre`` before it is squared."""
    tabs = [x for pi, rows in ((u.pg, u.gw), (u.pb, u.gb), (u.pcb, getattr(u, "gcb", None)))
            for x in ((out[offs[pi]:], rows) if pi is not None else (None, None))]
    if u.gn_parts:  # (``hf_gn_split_rows_sqsum``: the sample's parts added first)
        return (*tabs, float(pre), u.a.shape[0], u.gn_parts, u.a.shape[1])
    return (*tabs, float(pre), u.a.shape[0], u.a.shape[1])


# ---- hf_conv_problem: every slab-mode convolution, alone, grouped or as a D + W pair --------------------------------
def conv_problem(direction, out, act, mat, geo, splits, act_ld=0, out_c=0, mat_ld=0):
    """Direction 0 (forward / tangent), 1 (data gradient) or 2 (weight gradient) of the layer ``geo``: ``out`` receives
    ``splits`` slabs, ``out.shape[1]`` apart where it is a [splits, numel] buffer; ``act_ld`` / ``mat_ld``: the pixel
    stride of an operand that is a channel slice of a wider buffer, ``out_c``: of a weight gradient with padded rows."""
    return problem(_lib.ConvProblem, direction=int(direction), out=out, act=act, mat=mat, **dict(zip(_DIMS, geo.dims())),
                   act_ld=act_ld, out_c=out_c, splits=int(splits), mat_ld=mat_ld,
                   slab_stride=out.shape[1] if out is not None and out.dim() == 2 else 0)


def conv_args(q):
    """``hf_conv2d_nhwc_slabs``."""
    return (q.direction, q.out, q.act, q.mat, *(getattr(q, name) for name in _DIMS), q.act_ld, q.mat_ld, q.out_c, q.splits,
            q.slab_stride)


def conv_backward_args(d, w):
    """``hf_conv2d_nhwc_backward_slabs``: the data-gradient problem ``d`` and the weight-gradient problem ``w`` of ONE
    layer on dense operands, both from the same cotangent (``d.act`` and ``w.mat``)."""
    dims = tuple(getattr(d, name) for name in _DIMS)
    if dims != tuple(getattr(w, name) for name in _DIMS) or d.act != w.mat or any(
            (q.act_ld, q.out_c, q.mat_ld) != (0, 0, 0) for q in (d, w)):
        raise RuntimeError("conv_backward_args: not the dense D + W pair of one layer")
    return (d.out, w.out, d.act, w.act, d.mat, *dims, d.splits, d.slab_stride, w.splits, w.slab_stride)


def conv_bnsum(x, mean, rstd, part_x, part_1):
    """``hf_conv_bnsum``: the tangent convolution's epilogue leaves the partial sums of a train-mode BatchNorm behind it
    (``x``: the recorded convolution output) in ``part_x`` / ``part_1`` [ceil(rows / 64) * splits, k]; a problem without:
    ``_lib.ConvBnSum()``."""
    return problem(_lib.ConvBnSum, x=x, mean=mean, rstd=rstd, part_x=part_x, part_1=part_1, part_rows=part_1.shape[0])


# ---- depthwise convolutions (positional entry points, no struct): tangent / forward, data + weight gradient, and the
# two-term form of the latter (a Hessian product's second-order backward) ----------------------------------------------
DwConvProblem = namedtuple("DwConvProblem", "geo x act_ld w out t_x v ga ga1 dx slabs splits")


def dwconv_problem(geo, x, act_ld, w, out=None, t_x=None, v=None, ga=None, ga1=None, dx=None, slabs=None, splits=0):
    """A depthwise layer ``geo`` (``k == c``) on the input ``x`` at pixel pitch ``act_ld`` and the weight ``w`` [c, 1, r, s]
    read in place.  With ``out``: ``out = conv(t_x, w) + conv(x, v)`` -- ``t_x`` (same pitch) or ``v`` (the CG vector's slice)
    may be None, not both; the forward pass is ``v = w`` alone.  With ``ga``: the data gradient -> ``dx`` (None: not needed)
    and the weight gradient -> ``slabs`` [splits, c*r*s] of that cotangent, one launch.  With ``ga`` AND ``ga1`` (the step's
    first-order cotangent; ``ga`` is then its tangent): ``dx = D(ga, w) + D(ga1, v)``, ``slabs = W(x, ga) + W(t_x, ga1)``,
    one launch -- ``t_x``, ``v`` and ``dx`` are all needed, ``splits`` is the two-term plan's count."""
    if geo.k != geo.c or (out is None) == (ga is None):
        raise RuntimeError("dwconv_problem: a depthwise geometry, and either an output or a cotangent")
    if ga1 is not None and (ga is None or t_x is None or v is None or dx is None):
        raise RuntimeError("dwconv_problem: the two-term backward needs both cotangents, t_x, v and dx")
    return DwConvProblem(geo, x, act_ld, w, out, t_x, v, ga, ga1, dx, slabs, int(splits))


def _dw_dims(geo):
    return geo.dims()[:4] + geo.dims()[5:]  # (no k)


def dwconv_args(q):
    """The entry point's name, then its arguments: ``hf_dwconv2d_nhwc_tangent``, ``hf_dwconv2d_nhwc_backward_slabs`` or
    ``hf_dwconv2d_nhwc_backward2_slabs``."""
    dims = _dw_dims(q.geo)
    if q.ga is None:
        return ("hf_dwconv2d_nhwc_tangent", q.out, q.t_x, q.x if q.v is not None else None, q.act_ld,
                q.w if q.t_x is not None else None, q.v, *dims)
    if q.ga1 is not None:
        return ("hf_dwconv2d_nhwc_backward2_slabs", q.dx, q.slabs, q.ga, q.ga1, q.x, q.t_x, q.act_ld, q.w, q.v, *dims,
                q.splits, q.slabs.shape[1])
    return ("hf_dwconv2d_nhwc_backward_slabs", q.dx, q.slabs, q.ga, q.x, q.act_ld, q.w if q.dx is not None else None,
            *dims, q.splits, q.slabs.shape[1])


def dwconv_sqsum_args(out, ga, x, act_ld, geo, splits, pre):
    """``hf_dwconv2d_nhwc_sqsum_slabs``: ``out`` [splits, c*r*s] receives split s's partial sum over its samples of the
    squared per-sample weight gradient of the depthwise layer ``geo`` (``x`` at pixel pitch ``act_ld``, cotangent ``ga``),
    each scaled by ``pre`` before it is squared; parameter order."""
    return (out, ga, x, act_ld, *_dw_dims(geo), float(pre), int(splits), out.shape[1])


# ---- grouped convolutions (hf_gconv.hip): the depthwise pair's conventions, with the group count ---------------------
GConvProblem = namedtuple("GConvProblem", "geo groups x act_ld w out t_x v ga ga1 dx slabs splits")


def gconv_problem(geo, groups, x, act_ld, w, out=None, t_x=None, v=None, ga=None, ga1=None, dx=None, slabs=None, splits=0):
    """A grouped layer ``geo`` (``c`` -> ``k`` channels in ``groups`` groups) on the input ``x`` at pixel pitch ``act_ld`` and
    the weight ``w`` [k, c / groups, r, s] read in place.  With ``out``: ``out = conv(t_x, w) + conv(x, v)`` -- ``t_x`` (same
    pitch) or ``v`` (the CG vector's slice) may be None, not both; the forward pass is ``v = w`` alone.  With ``ga``: the data
    gradient -> ``dx`` (None: not needed) and the weight gradient -> ``slabs`` [splits, k*(c/groups)*r*s], one launch.  With
    ``ga`` AND ``ga1`` (the step's first-order cotangent; ``ga`` is then its tangent): ``dx = D(ga, w) + D(ga1, v)``,
    ``slabs = W(x, ga) + W(t_x, ga1)``, one launch -- ``t_x``, ``v`` and ``dx`` are all needed, ``splits`` is the same count."""
    if geo.c % groups or geo.k % groups or (out is None) == (ga is None):
        raise RuntimeError("gconv_problem: channel counts that are multiples of the groups, and either an output or a cotangent")
    if ga1 is not None and (ga is None or t_x is None or v is None or dx is None):
        raise RuntimeError("gconv_problem: the two-term backward needs both cotangents, t_x, v and dx")
    return GConvProblem(geo, int(groups), x, act_ld, w, out, t_x, v, ga, ga1, dx, slabs, int(splits))


def gconv_dims(geo, groups):
    """``n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w``: as the grouped entry points list them."""
    d = geo.dims()
    return d[:5] + (int(groups),) + d[5:]


def gconv_args(q):
    """The entry point's name, then its arguments: ``hf_gconv2d_nhwc_tangent``, ``hf_gconv2d_nhwc_backward_slabs`` or
    ``hf_gconv2d_nhwc_backward2_slabs``."""
    dims = gconv_dims(q.geo, q.groups)
    if q.ga is None:
        return ("hf_gconv2d_nhwc_tangent", q.out, q.t_x, q.x if q.v is not None else None, q.act_ld,
                q.w if q.t_x is not None else None, q.v, *dims)
    if q.ga1 is not None:
        return ("hf_gconv2d_nhwc_backward2_slabs", q.dx, q.slabs, q.ga, q.ga1, q.x, q.t_x, q.act_ld, q.w, q.v, *dims,
                q.splits, q.slabs.shape[1])
    return ("hf_gconv2d_nhwc_backward_slabs", q.dx, q.slabs, q.ga, q.x, q.act_ld, q.w if q.dx is not None else None,
            *dims, q.splits, q.slabs.shape[1])


def gconv_sqsum_args(out, ga, x, act_ld, geo, groups, splits, pre):
    """``hf_gconv2d_nhwc_sqsum_slabs``: ``out`` [splits, k*(c/groups)*r*s] receives split s's partial sum over its samples of
    the squared per-sample weight gradient of the grouped layer ``geo`` (``x`` at pixel pitch ``act_ld``, cotangent ``ga``),
    each scaled by ``pre`` before it is squared; parameter order."""
    return (out, ga, x, act_ld, *gconv_dims(geo, groups), float(pre), int(splits), out.shape[1])


# ---- the squared-sum launches of the batched diagonal empirical Fisher (positional entry points, no struct) ------------
def conv_sqsum_args(out, act, mat, geo, splits, pre, act_ld=0, out_c=0):
    """``hf_conv2d_nhwc_sqsum_slabs``: ``out`` [splits, numel] receives split s's partial sum over its samples of the
    squared per-sample weight gradient of ``act`` (X) and ``mat`` (dY), each scaled by ``pre`` before it is squared."""
    return (out, act, mat, *Geometry(*geo).dims(), act_ld, out_c, float(pre), int(splits), out.shape[1])


def chan_sqsum_args(g, n, c, hw, row_blocks, pre, gw2=None, gb2=None, x=None, mean=None, rstd=None):
    """``hf_chan_sqsum``: the squared per-sample scale (``gw2``, needs ``x`` / ``mean`` / ``rstd``) and shift or bias
    (``gb2``) gradients summed over the samples, ``row_blocks`` partial rows each."""
    return (gw2, gb2, g, x, mean, rstd, n, c, hw, float(pre), int(row_blocks))
