"""Tangent sweep J v: per unit the tangent convolution of ``[t_x | x]`` with ``[W | v_W]`` and the BatchNorm / bias
tangent (+ residual tangent, ReLU mask) (optimizer.py:457-462, R-op).

Mixin of ``_ConvEngine`` (engine/conv.py); see that class for the sweeps' overall structure."""

import os

from .. import _lib
from .problems import (affine_args, affine_problem, affine_train_args, affine_train_problem, conv_args, conv_bnsum,
                       conv_problem)


def head_fused_shape_ok(rows, features, classes):
    """The shapes ``hf_linear_ce_head`` accepts (``hf_head.hip``: its argument check): up to 4096 rows, 64 classes and
    512 features in quads, with W, V_W, the workgroup's four feature rows and its four rows of HJv within 64 KB of LDS.
    A head outside this keeps the GEMM path."""
    lds = (2 * classes * features + 4 * features + 4 * classes) * 4
    return (1 <= rows <= 4096 and 1 <= classes <= 64 and 4 <= features <= 512 and features % 4 == 0
            and lds <= 64 * 1024)


class _TangentSweep:
    def _scale_shift_tangent(self, u, v):
        k = u.a.shape[1]
        return self._param_slice(v, u.pg, k), self._param_slice(v, u.pb, k)

    def _scale_second_order_sum(self, u):
        """rstd * sum_rows g_z * t_a  (g_z: the step's first-order masked cotangent; t_a: the sum of the tangent
        convolution's slabs) as the second ``rb`` rows of gw, where the gather expects the scale's second-order share."""
        n, k, oh, ow = u.a.shape
        self._chan_sums(u.tbuf, u.sT, u.tbuf.shape[1], n, k, oh * ow, u.rb, gw=u.gw[u.rb:], x=u.g1, mean=self._zeros(k),
                        rstd=u.rstd)

    def _train_tangent_sums(self, u):
        """The partial rows ``(of S_x, of S_1, their count)`` of a train-mode unit's tangent sums over all its rows -- by
        the convolution's epilogue (``u.tsum``), else by a reduction launch of their own over the slabs; left in
        ``u.tsums``.  What the elementwise pass of an unpooled unit and the gather of a pooled one add up."""
        n, k, oh, ow = u.a.shape
        parts = (u.gw, u.gb, u.rb)
        if self.hessian:
            # the adjoint of a Hessian product reads these sums again (hf_bn_train_hessian_coeffs): rows of their
            # own -- and the scale's second-order sum
            parts = (u.hx, u.h1, u.rb)
            self._scale_second_order_sum(u)
        if u.tsum:
            parts = (u.tpx, u.tp1, u.tp1.shape[0])
        u.tsums = parts  # (a Hessian product's adjoint reads them again)
        if not u.tsum:
            self._chan_sums(u.tbuf, u.sT, u.tbuf.shape[1], n, k, oh * ow, u.rb, gw=parts[0], gb=parts[1], x=u.a,
                            mean=u.mean, rstd=u.rstd)
        return parts

    def _bn_tangent(self, u, v, add, add_ld):
        """t_y = mask * (sum(T slabs) * w*rstd + xhat * v_w + v_b + add), into the consumer's operand."""
        n, k, oh, ow = u.a.shape
        vg, vb = self._scale_shift_tangent(u, v)
        if u.train:
            # reduction, then the elementwise pass adds the partial rows up in its prologue
            parts = self._train_tangent_sums(u)
            self._launch("hf_chan_affine_train",
                         *affine_train_args(self._train_tangent_problem(u, parts, vg, vb, add), add_ld))
            return
        self._launch("hf_chan_affine_ex", *affine_args(affine_problem(u, vg, vb, add, add_ld)))

    def _train_pair_ok(self, u1, u2):
        return u1.train and u2.train and os.environ.get("HF_BN_TRAIN_PAIR", "1") != "0"

    @staticmethod
    def _train_tangent_problem(u, parts, vg, vb, add=None):
        return affine_train_problem(u, u.tout, u.tout_ld, u.tbuf, u.sT, u.tbuf.shape[1], parts, vg, vb,
                                    u.y if u.relu else None, add)

    def _bn_tangent_pair_train(self, u1, u2, v):
        """Train mode, prologue form: the elementwise passes of two units without residual input in ONE launch (their
        partial sums came from the convolutions' epilogue)."""
        self._launch_pair("hf_chan_affine_train_pair", *(
            self._train_tangent_problem(u, (u.tpx, u.tp1, u.tp1.shape[0]), *self._scale_shift_tangent(u, v))
            for u in (u1, u2)))

    def _bn_tangent_pair(self, u1, u2, v):
        """The BatchNorm tangents of two units without residual input in ONE launch."""
        self._launch_pair("hf_chan_affine_pair",
                          *(affine_problem(u, *self._scale_shift_tangent(u, v)) for u in (u1, u2)))

    def _tangent_convs(self, units):
        """The tangent convolutions ``conv([t_x | x], [W | v_W])`` of one or two units in ONE launch.  In front of a
        train-mode BatchNorm the launch's epilogue also writes the per-channel partial sums of its output tiles
        (``hf_conv2d_nhwc_group_slabs_bnsum``): the reduction launch between convolution and elementwise pass is gone
        (``u.tsum``: ``_bn_tangent`` then adds ``u.tp1 / u.tpx`` up instead of ``u.gb / u.gw``)."""
        probs = [conv_problem(0, u.tbuf, u.xcat, u.wcat, u.geo.doubled(), u.sT) for u in units]
        if any(u.epi for u in units):
            sums = [conv_bnsum(u.a, u.mean, u.rstd, u.tpx, u.tp1) if u.epi else _lib.ConvBnSum() for u in units]
            if self._launch_unless_refused("hf_conv2d_nhwc_group_slabs_bnsum", probs, len(probs), sums):
                for u in units:
                    u.tsum = u.epi
                return
            for u in units:  # (a geometry the 64x64-tile instantiations do not cover: not tried again)
                u.epi = False
        for u in units:
            u.tsum = False
        if len(units) == 1:
            self._launch("hf_conv2d_nhwc_slabs", *conv_args(probs[0]))
        else:
            self._launch("hf_conv2d_nhwc_group_slabs", probs, len(probs))
