"""Diagonal of the empirical Fisher from one adjoint sweep + per-sample weight-gradient launches
(preconditioners.py:11-105) -- or, with ``HF_DIAG_EF_BATCHED=1``, + ONE squared-sum launch per layer and one gather.

Mixin of ``_ConvEngine`` (engine/conv.py); see that class for the sweeps' overall structure."""

import torch

from .. import _lib
from .problems import chan_sqsum_args, conv_sqsum_args


class _DiagEF:
    # ---- diagonal of the empirical Fisher (preconditioners.py:11-105) ---------------------------------------------
    def diag_ef(self, reduction="mean", out=None):
        """``sum_i g_i^2`` (``sum``) / ``(1/N) sum_i g_i^2`` (``mean``) over the per-sample gradients ``g_i`` of the
        engine's CURRENT batch (``set_batch`` + ``forward_own`` must have run): the quantity of the reference's
        ``diag_EF_autograd`` / ``diag_EF_backpack`` (one backward pass per sample / BackPACK's ``SumGradSquared``),
        from ONE adjoint sweep of the whole batch -- in eval mode the samples do not interact, so the batch
        cotangents ARE the per-sample cotangents -- followed, per sample, by the weight-gradient convolutions on that
        sample's rows and one squaring gather (``hf_pack_ex`` mode 1).  A tagged L2 term (each per-sample loss of
        the reference carries it whole) enters in closed form: sum (a_i + b)^2 = sum a_i^2 + 2 b sum a_i + N b^2.

        ``HF_DIAG_EF_BATCHED=1`` (read when the engine is built): instead of the per-sample launches, per unit ONE
        ``hf_conv2d_nhwc_sqsum_slabs`` on the whole-batch operands (it squares and sums the per-sample weight gradients
        inside the launch: BackPACK's ``SumGradSquared``), ONE ``hf_chan_sqsum`` for the BatchNorm / bias entries, and
        ONE plain gather (``hf_pack_ex`` mode 0) for all of them -- a number of launches that does not depend on the
        batch.  The factor that undoes the loss's 1/N goes into the launches (``pre``: applied before squaring)."""
        if self.loss_spec is None or self.train_bn:
            raise RuntimeError("engine.diag_ef needs a softmax cross-entropy / MSE loss and eval-mode BatchNorm")
        if self.loss_spec["reduction"] != reduction:
            raise RuntimeError("engine.diag_ef: the loss's reduction differs from the requested one")
        n = self.x_in.shape[0]
        if out is None:
            out = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        out.zero_()
        if self._diag_batched:
            self._diag_buffers()  # (in front of the sweep: a masked cotangent allocated here is filled by it)
        l2, self._l2 = self._l2, None
        try:
            mean_grad = self.gradient()  # fills the units' cotangents (g / ga, or g1 / ga1 of a Hessian engine)
        finally:
            self._l2 = l2
        scale = float(n) if reduction == "mean" else 1.0   # the sweep's cotangents carry the loss's 1/N
        first_order = self.hessian
        self._diag_buffers()
        tensors, perms, splits = self._diag_pack
        if self._diag_batched:
            self._diag_batched_launches(out, n, scale, first_order)
        for i in range(0 if self._diag_batched else n):
            for u in self.units:
                if u.dead:  # (frozen, behind frozen layers only: the sweep left no cotangent here, nothing is gathered)
                    continue
                ga = (u.ga1 if first_order else u.ga)[i:i + 1]
                if u.pw is None:
                    pass  # (frozen weight: no entry)
                elif u.im2col:
                    self._conv_slabs(2, u.wps, u.cols_pad[i:i + 1], ga, u.geo_w1, u.sW1, out_c=u.jcols)
                else:
                    self._conv_slabs(2, u.wps, u.x[i:i + 1], ga, u.geo1, u.sW1)
                k, hw = u.a.shape[1], u.a.shape[2] * u.a.shape[3]
                if u.pg is None and u.pb is None:
                    continue
                if u.bn is not None:
                    g = (u.g1 if first_order else u.g)[i:i + 1]
                    self._chan_sums(g, 1, 0, 1, k, hw, 1, gw=u.gws, gb=u.gbs, x=u.a[i:i + 1], mean=u.mean, rstd=u.rstd)
                elif u.pb is not None:
                    self._chan_sums(ga, 1, 0, 1, k, hw, 1, gb=u.gbs)
            _lib.pack_ex(out, tensors, perms, splits, scale=scale, live=self._pack_live, mode=1)
        self._diag_head(out, scale)
        if l2 is not None:
            sum_a = mean_grad * (scale / self.weight)  # sum_i a_i
            b = l2 * self._theta()
            out.add_(2.0 * b * sum_a).add_(float(n) * b * b)
        if reduction == "mean":
            out.div_(float(n))
        return out

    def _diag_head_buffers(self, tensors):
        """A kind whose head has parameters: their entries of the gather's table ..."""

    def _diag_head(self, out, scale):
        """... and their values, written straight into ``out``."""

    def _diag_batched_launches(self, out, n, pre, first_order):
        """The batched sweep behind the adjoint sweep: per live unit one squared-sum convolution and one squared channel
        sum on the whole batch, then ONE gather of all their slabs and partial rows."""
        tensors, perms, splits = self._diag_pack
        for u in self.units:
            if u.dead:  # (as below: no cotangent here, nothing is gathered)
                continue
            ga = u.ga1 if first_order else u.ga
            if u.pw is not None:
                act = u.cols_pad if u.im2col else u.x
                self._launch("hf_conv2d_nhwc_sqsum_slabs",
                             *conv_sqsum_args(u.wps, act, ga, u.geo1, u.sW1, pre, out_c=u.jcols if u.im2col else 0))
            if u.pg is None and u.pb is None:
                continue
            k, hw = u.a.shape[1], u.a.shape[2] * u.a.shape[3]
            gb2 = u.gbs if u.pb is not None else None
            if u.bn is not None:
                self._launch("hf_chan_sqsum",
                             *chan_sqsum_args(u.g1 if first_order else u.g, n, k, hw, u.rb1, pre, gb2=gb2,
                                              gw2=u.gws if u.pg is not None else None,
                                              **(dict(x=u.a, mean=u.mean, rstd=u.rstd) if u.pg is not None else {})))
            else:
                self._launch("hf_chan_sqsum", *chan_sqsum_args(ga, n, k, hw, u.rb1, pre, gb2=gb2))
        _lib.pack_ex(out, tensors, perms, splits, scale=1.0, live=self._pack_live, mode=0)

    def _diag_buffers(self):
        """Per-sample (n = 1) geometry, split counts and slab buffers of ``diag_ef`` (allocated on first use).  Batched
        sweep: the whole-batch geometry (the im2col'd stem as a 1x1 convolution over its [n, oh, ow] map of patches), the
        planned sample splits, one slab per split and one partial row per share of the samples."""
        if self._diag_pack is not None:
            return
        f32, dev = torch.float32, self.dev
        tensors, perms, splits = [None] * len(self.params), {}, {}
        for u in self.units:
            k = u.a.shape[1]
            if u.bn is not None and not self.hessian and u.g is None:
                u.g, u.needs_g = torch.empty_like(u.a), True  # (every unit's masked cotangent is needed per sample)
            u.rb1 = 1
            if self._diag_batched:
                n = u.a.shape[0]
                u.geo1 = u.geo_w._replace(n=n, h=u.a.shape[2], w=u.a.shape[3]) if u.im2col else u.geo
                u.sW1 = _lib.conv_sqsum_plan(*u.geo1)
                # shares of the samples for the channel sums: ~one workgroup per CU (64 channels each), none empty
                u.rb1 = max(1, min(n, 256 // -(-k // 64)))
                while -(-n // u.rb1) * (u.rb1 - 1) >= n:
                    u.rb1 -= 1
            elif u.im2col:
                rows1 = u.a.shape[2] * u.a.shape[3]
                u.geo_w1 = u.geo_w.with_n(rows1)
                u.sW1 = self._plan(2, u.geo_w1)
            else:
                u.geo1 = u.geo.with_n(1)
                u.sW1 = self._plan(2, u.geo1, u.name)
            u.wps = torch.zeros((u.sW1, u.conv.weight.numel()), dtype=f32, device=dev)  # dead taps stay 0
            if u.pw is not None:
                tensors[u.pw] = u.wps[0]
                if not u.im2col:
                    k_, c, r, s_ = u.conv.weight.shape
                    if r * s_ > 1:
                        perms[u.pw] = (c, r * s_)
                if u.sW1 > 1:
                    splits[u.pw] = (u.sW1, u.wps.shape[1])
            u.gws = torch.zeros((u.rb1, k), dtype=f32, device=dev)
            u.gbs = torch.zeros((u.rb1, k), dtype=f32, device=dev)
            for pi, buf in ((u.pg, u.gws), (u.pb, u.gbs)):
                if pi is not None:
                    tensors[pi] = buf[0]
                    if u.rb1 > 1:
                        splits[pi] = (u.rb1, k)
        self._diag_head_buffers(tensors)
        self._pack_args()  # (makes sure _pack_live exists)
        self._diag_pack = (tensors, perms, splits)
