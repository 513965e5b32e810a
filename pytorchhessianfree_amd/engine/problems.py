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


# ---- the squared-sum launches of the batched diagonal empirical Fisher (positional entry points, no struct) ------------
def conv_sqsum_args(out, act, mat, geo, splits, pre, act_ld=0, out_c=0):
    """``hf_conv2d_nhwc_sqsum_slabs``: ``out`` [splits, numel] receives split s's partial sum over its samples of the
    squared per-sample weight gradient of ``act`` (X) and ``mat`` (dY), each scaled by ``pre`` before it is squared."""
    return (out, act, mat, *Geometry(*geo).dims(), act_ld, out_c, float(pre), int(splits), out.shape[1])


def chan_sqsum_args(g, n, c, hw, row_blocks, pre, gw2=None, gb2=None, x=None, mean=None, rstd=None):
    """``hf_chan_sqsum``: the squared per-sample scale (``gw2``, needs ``x`` / ``mean`` / ``rstd``) and shift or bias
    (``gb2``) gradients summed over the samples, ``row_blocks`` partial rows each."""
    return (gw2, gb2, g, x, mean, rstd, n, c, hw, float(pre), int(row_blocks))
