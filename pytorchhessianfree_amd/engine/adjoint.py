"""Adjoint sweep J^T u: per unit the BatchNorm adjoint and data + weight gradient in one launch; the gather of all
parameter gradients into the flat vector -- which also leaves the PCG curvature scalar (optimizer.py:457-462, L-op).

Mixin of ``_ConvEngine`` (engine/conv.py); see that class for the sweeps' overall structure."""

from .. import _lib
from .problems import (affine_args, affine_train_args, affine_train_problem, bn_adjoint_args, bn_adjoint_problem,
                       bn_adjoint_v4_args, conv_args, conv_backward_args, conv_problem, problem)


class _AdjointSweep:
    @staticmethod
    def _train_adjoint_problem(u):
        """Pass 2 of the train-mode adjoint: g_a from the masked cotangent u.g and the partial rows of its sums."""
        return affine_train_problem(u, u.ga, 0, u.g, 1, 0, (u.gw, u.gb, u.rb))

    def _bn_adjoint_pair_train(self, u1, srcs1, u2, srcs2):
        """Train mode, prologue form: both units' reduction passes in one launch, both elementwise passes in one."""
        self._bn_adjoint_pair(u1, srcs1, u2, srcs2, train=True)
        self._launch_pair("hf_chan_affine_train_pair", self._train_adjoint_problem(u1), self._train_adjoint_problem(u2))

    def _bn_adjoint_pair(self, u1, srcs1, u2, srcs2, train=False):
        """The BatchNorm adjoints of two units (row-major kernel) in ONE launch.  ``train``: the reduction pass of the
        train-mode adjoint (masked cotangent and partial sums only)."""
        probs = [bn_adjoint_problem(u, srcs, reduce=train) for u, srcs in ((u1, srcs1), (u2, srcs2))]
        if not train and self._split_now(u1) and self._split_now(u2):
            # the chain's launch is the elementwise one; the per-channel sums wait for _flush_sums
            self._launch_pair("hf_bn_adjoint_v4_pair", *probs)
            self._sums_pending.update(u.sums_slot for u in (u1, u2) if u.defer)
            return
        self._launch_pair("hf_chan_affine_bwd_pair", *probs)

    def _adjoint_unit(self, u, srcs):
        """srcs: up to two (tensor, splits, slab_stride) cotangents of the unit's output."""
        second = self._second
        if u.pool is not None:  # (a pooled unit of a plain stack: bias / ReLU / pool adjoint in one launch)
            self._pool_adjoint(u, srcs)
        else:
            self._bn_adjoint(u, srcs, reduce_only=second and u.train)
        if not second:
            self._conv_adjoint(u)
            return
        # ---- Hessian product: the tangent of the backward sweep through this unit --------------------------
        if u.bn is None:
            # a bias has no second-order term of its own: the convolutions read g_a itself.  (The chain's D + W launch
            # through the two-problem entry point -- the same pair of problems ``_conv_adjoint`` launches --, and in
            # sequence the extras BEHIND it: as the plain stack has always issued them)
            if not u.im2col and not u.first and u.sD:  # (sD == 0, a tangent-free input: the weight gradient alone)
                self._launch("hf_conv2d_nhwc_dw_slabs", *([q] for q in self._dw_problems(u, u.ga)))
            else:
                self._conv_adjoint(u)
            if not self._extras_parallel:
                self._hessian_extras(u)
            return
        n, k, oh, ow = u.a.shape
        v_gamma = self._param_slice(self._v, u.pg, k)
        if v_gamma is None:  # (frozen scale)
            v_gamma = self._zeros(k)
        if not self._extras_parallel:
            self._hessian_extras(u)
        if u.train:
            # batch statistics: the per-channel finalisation of the five row reductions (this pass's g_z' sums, the
            # tangent sweep's a' sums), then  g_a' = c0 g_a + c1 g_z + c2 g_z' + c3 a' + c4 xhat + c5
            rb = u.rb
            tx, t1, nparts_t = u.tsums
            self._launch("hf_bn_train_hessian_coeffs", u.hcoef, u.gw[2 * rb:], u.gw, u.gb, u.gw[rb:], rb, tx, t1, nparts_t,
                         u.gg1, u.gb1, u.scale, v_gamma, u.rstd, float(n * oh * ow), k)
            self._launch("hf_bn_train_hessian_apply", u.gah, u.ga1, u.g1, u.g, u.tbuf, u.sT, u.tbuf.shape[1], u.a, u.mean,
                         u.rstd, u.hcoef, n * oh * ow, k)
        else:
            # the convolution's cotangent tangent:  g_a' + g_z * rstd * v_gamma
            self._launch("hf_chan_affine_ex", *affine_args(problem(
                _lib.AffineProblem, out=u.gah, a=u.g1, rstd=u.rstd, w=v_gamma, add=u.ga, n=n, c=k, hw=oh * ow,
                a_splits=1)))
        if self._extras_mode == 2 and not u.im2col and not u.first and u.sD:
            # the chain's launch also computes conv_D(g_a, V) -- the one extra term the chain itself needs next
            self._launch("hf_conv2d_nhwc_group_slabs", [*self._dw_problems(u, u.gah), self._dgrad_extra(u)], 3)
        else:
            self._conv_adjoint(u, u.gah)

    def _dslabs(self, u):
        """How many data-gradient slabs the consumers of ``u``'s input cotangent must sum in the current sweep."""
        return u.nD if self._second else u.sD

    def _bn_adjoint(self, u, srcs, reduce_only=False):
        """``reduce_only`` (train mode inside a Hessian product): the masked cotangent and its per-channel sums only --
        the elementwise pass is ``hf_bn_train_hessian_apply``'s."""
        self._extras_wait(srcs)
        if u.train:
            # pass 1: g = mask * (sum of the cotangents' slabs) and its per-channel sums (the parameter
            # gradients); pass 2: g_a = rstd*w * [g - mean(g) - xhat * mean(xhat*g)] (the batch statistics'
            # share), by the elementwise kernel with the corrections folded into its per-channel vectors
            # (pass 2 adds the partial rows up in its prologue)
            self._launch("hf_chan_affine_bwd_ex", *bn_adjoint_args(bn_adjoint_problem(u, srcs, reduce=True)))
            if not reduce_only:
                self._launch("hf_chan_affine_train", *affine_train_args(self._train_adjoint_problem(u)))
            return
        if self._split_now(u):
            # g = mask * (sum of both cotangents' slabs) -> u.g; g * w*rstd -> u.ga: all the chain needs.  The per-channel
            # sums (the parameters' gradient: only the gather reads them) wait for _flush_sums
            self._launch("hf_bn_adjoint_v4", *bn_adjoint_v4_args(bn_adjoint_problem(u, srcs)))
            if u.defer:
                self._sums_pending.add(u.sums_slot)
            return
        # g = mask * (sum of both cotangents' slabs) -> u.g; g * w*rstd -> u.ga; per-channel sums
        self._launch("hf_chan_affine_bwd_ex", *bn_adjoint_args(bn_adjoint_problem(u, srcs, only_needed=True)))

    @staticmethod
    def _dw_problems(u, ga, dgrad=True):
        """The data-gradient (``dgrad``) and the weight-gradient problem of the unit's convolution from ``ga``."""
        d = [conv_problem(1, u.dbuf, ga, u.wT, u.geo, u.sD)] if dgrad else []
        return d + [conv_problem(2, u.wbuf, u.x, ga, u.geo, u.sW)]

    def _conv_adjoint(self, u, ga=None):
        """Data + weight gradient of the unit's convolution from ``ga`` (default ``u.ga``), one launch."""
        ga = u.ga if ga is None else ga
        if u.im2col:
            self._conv_slabs(2, u.wbuf, u.cols_pad, ga, u.geo_w, u.sW, out_c=u.jcols)
            return
        if u.first or u.no_dgrad:  # the network input (or the output of frozen layers) needs no gradient
            self._launch("hf_conv2d_nhwc_slabs", *conv_args(*self._dw_problems(u, ga, dgrad=False)))
            return
        # (Measured and rejected, round 4: the weight gradient -- off the adjoint chain, only the gather reads it -- as
        # its own launch on a side branch, the chain's launch computing the data gradient alone: one cross-branch
        # dependency PER UNIT costs far more than the shorter chain saves -- ResNet-18 1 518 -> 1 037 matvecs/s,
        # ResNet-50 topology 314 -> 253, All-CNN-C 753 -> 711.  A side branch pays when it forks ONCE: the Hessian
        # products' extras below.)
        self._launch("hf_conv2d_nhwc_backward_slabs", *conv_backward_args(*self._dw_problems(u, ga)))

    def _gather(self, out, g_fw, g_fb, first_order=False):
        """All parameter gradients into the flat vector (weight-gradient slabs summed on the way)."""
        self._flush_sums()
        tensors, perms, splits = self._pack_args(first_order)
        if g_fw is not None:  # (a head with parameters of its own)
            tensors, splits = self._head_entries(tensors, splits, g_fw, g_fb)
        _lib.pack_ex(out, tensors, perms, splits, scale=self.weight, live=self._pack_live,
                     compact=self._compact_nl)  # (local_compact: the compact layout)
        return out

    def _gather_range(self, out, g_fw, g_fb, lo, hi):
        """``_gather`` for the parameters ``lo ... hi-1`` only (a contiguous range of the flat vector)."""
        self._flush_sums()  # (what this phase of the sweep has deferred)
        tensors, perms, splits = self._pack_args()
        if g_fw is not None:
            tensors, splits = self._head_entries(tensors, splits, g_fw, g_fb)
        sub = lambda d: {i - lo: val for i, val in d.items() if lo <= i < hi}  # noqa: E731
        end = self._offs[hi] if hi < len(self.params) else self.n
        _lib.pack_ex(out[self._offs[lo]:end], tensors[lo:hi], sub(perms), sub(splits), scale=self.weight,
                     live=sub(self._pack_live))

    def _pack_args(self, first_order=False):
        """(tensors, perms, splits) of ``hf_pack_ex``.  ``first_order``: a gradient sweep of a Hessian
        engine fills only the first ``sW`` weight-gradient slabs of each layer."""
        if first_order and self.hessian:
            tensors, perms, splits = self._pack_args()
            splits = dict(splits)
            for u in self.units:
                if u.pw is not None and u.nW != u.sW:
                    if u.sW > 1:
                        splits[u.pw] = (u.sW, u.wbuf.shape[1])
                    else:
                        splits.pop(u.pw, None)
                if u.pg is not None and u.gw_rows != u.rb:
                    if u.rb > 1:
                        splits[u.pg] = (u.rb, u.cout)
                    else:
                        splits.pop(u.pg, None)
            return tensors, perms, splits
        if self._pack is None:
            tensors, perms, splits = [None] * len(self.params), {}, {}
            self._pack_live = {}
            for u in self.units:
                if u.pw is None:  # (frozen weight: its gradient slabs, if the fused launch wrote any, are not gathered)
                    for pi, buf, rows in ((u.pg, u.gw, u.gw_rows), (u.pb, u.gb, u.rb)):
                        if pi is not None:
                            tensors[pi] = buf[0]
                            if rows > 1:
                                splits[pi] = (rows, u.cout)
                    continue
                tensors[u.pw] = u.wbuf[0]
                if not u.im2col:
                    k, c, r, s_ = u.conv.weight.shape
                    if r * s_ > 1:
                        perms[u.pw] = (c, r * s_)  # stored (O, H, W, I); 1x1 kernels: already in order
                        if u.live:
                            self._pack_live[u.pw] = u.live
                if u.nW > 1:
                    splits[u.pw] = (u.nW, u.wbuf.shape[1])
                for pi, buf, rows in ((u.pg, u.gw, u.gw_rows), (u.pb, u.gb, u.rb)):
                    if pi is not None:
                        tensors[pi] = buf[0]
                        if rows > 1:
                            splits[pi] = (rows, u.cout)
            self._pack = (tensors, perms, splits)
        return self._pack
