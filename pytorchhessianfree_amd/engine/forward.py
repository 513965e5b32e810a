"""The units of the network's forward pass on the engine's static buffers, own kernels only (reference: the ``forward()``
of optimizer.py:216-229 and every ``tfunc`` call, :288-294), eval- and train-mode BatchNorm; the loss head; the
recorded-activation load.

Mixin of ``_ConvEngine`` (engine/conv.py); see that class for the sweeps' overall structure."""

import torch


class _Forward:
    def _bn_forward(self, u, splits, update_running=True):
        n, k, oh, ow = u.a.shape
        res = u.res
        if u.train:
            # ONE pass for the partial sums (the convolution's slabs summed into ``a``, per-channel sum a / sum a^2 in
            # fp64 per row block); the normalising launch adds them up in its prologue -- 2 launches per unit
            bn = u.bn
            move = update_running and bn.track_running_stats
            count = float(n * oh * ow)
            self._launch("hf_bn_stats_rows", u.a, u.tbuf, splits, u.tbuf.shape[1], u.stat_part, n * oh * ow, k, u.rb)
            self._launch("hf_bn_forward_train", u.y, u.yout2, 2 * k if u.yout2 is not None else 0, u.a, u.stat_part, u.rb,
                         u.mean_t, u.rstd, bn.running_mean if move else None, bn.running_var if move else None, count,
                         float(bn.eps), float(bn.momentum) if move else -1.0, u.scale, u.shift, res, 0,
                         1 if u.relu else 0, n * oh * ow, k)
            if move:
                bn.num_batches_tracked.add_(1)
            return
        self._launch("hf_bn_forward", u.y, u.yout2, 2 * k if u.yout2 is not None else 0, u.a, u.tbuf, splits,
                     u.tbuf.shape[1], u.mean, u.rstd, u.scale, u.shift, res, 0, 1 if u.relu else 0, n * oh * ow, k)

    def _conv_forward(self, u):
        if u.im2col:  # 1x1 product over the im2col; the weight is read from the parameter itself
            self._conv_slabs(0, u.tbuf, u.cols, u.conv.weight.detach(), u.geo, u.sF)
            return
        self._conv_slabs(0, u.tbuf, u.x, u.wcat, u.geo, u.sF, mat_ld=u.geo.doubled().c)

    def _loss_head(self):
        """Softmax probabilities and the cross-entropy value of the current logits (the reference's
        ``forward()[0]``, optimizer.py:216-229; same ATen ops as ``F.cross_entropy``)."""
        if self.loss_spec["kind"] == "mse":  # (same ATen op as ``F.mse_loss`` / ``nn.MSELoss``)
            val = torch.nn.functional.mse_loss(self.logits, self._targets, reduction=self.loss_spec["reduction"])
        else:
            torch.softmax(self.logits, 1, out=self._p)
            lsm = torch.log_softmax(self.logits, 1)
            val = torch.nn.functional.nll_loss(lsm, self._targets, reduction=self.loss_spec["reduction"])
        if self._l2 is not None:
            theta = self._theta()
            val = val + 0.5 * torch.dot(self._l2 * theta, theta)
        self.loss_buf.copy_(val)

    def _load_recorded(self, outputs):
        """Overwrite the engine's activations with the ones the MODEL's forward pass recorded, so that a
        product of the engine and one of the autograd operator linearise at bitwise the same point -- same
        ReLU masks, same pooling positions (a kind extends this by its pooling layers').  Two correct fp32 forward
        passes may decide a ReLU whose input is within rounding of zero differently, and one such sign moves a product
        of a deep net by ~1e-4 of its max-norm: not an error of either, but it would drown the comparison below."""
        for u in self.units:
            u.a.copy_(u.ra)
            u.y.copy_(u.ry)
            if u.yout2 is not None:
                u.yout2.copy_(u.ry)
            if u.train:  # (the own forward pass writes its batch statistics into the same buffers)
                u.mean_t.copy_(u.rec_stats[0])
                u.rstd.copy_(u.rec_stats[1])
        self.logits.copy_(outputs.detach())
        if self.loss_spec is not None:
            self._loss_head()
        self._at = "recorded"
