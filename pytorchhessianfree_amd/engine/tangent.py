"""Tangent sweep J v: per unit the tangent convolution of ``[t_x | x]`` with ``[W | v_W]`` and the BatchNorm / bias
tangent (+ residual tangent, ReLU mask); the classifier head with the loss Hessian (optimizer.py:457-462, R-op).

Mixin of ``FusedGGNEngine`` (engine/core.py); see that class for the sweeps' overall structure."""

import os

import torch

from .. import _lib
from .problems import affine_args, affine_problem, affine_train_args, affine_train_problem


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

    def _bn_tangent(self, u, v, add, add_ld):
        """t_y = mask * (sum(T slabs) * w*rstd + xhat * v_w + v_b + add), into the consumer's operand."""
        n, k, oh, ow = u.a.shape
        vg, vb = self._scale_shift_tangent(u, v)
        if u.train:
            # reduction (partial rows: by the convolution's epilogue, else by its own launch), then the elementwise
            # pass adds them up in its prologue
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

    def _tangent_stem(self, v, carry_scatter=False):
        """Stem: conv(x, v_W) as a 1x1 convolution on the im2col'd input (the input has no tangent; v_W is a
        slice of ``v`` itself).  ``carry_scatter``: the launch also carries the scatter of every other layer's v_W
        into its ``[W | v_W]`` operand (``hf_conv2d_nhwc_slabs_unpack``) -- nothing in the stem reads those."""
        s = self.stem
        if s.dead:  # (frozen stem: its output carries no tangent -- only the scatter it would have carried is left)
            if carry_scatter and self._slot_list:
                _lib.unpack_tangent(v, self._slot_list)
            return
        if s.pw is None:  # (frozen stem weight under a trainable BatchNorm: conv(x, 0) = 0)
            vw = self._zeros(s.conv.weight.numel())
        else:
            vw = v[self._offs[s.pw]: self._offs[s.pw] + s.conv.weight.numel()]
        if not (carry_scatter and self._conv_carrying_scatter(s, vw, s.sT, v, 1)):
            if carry_scatter:
                _lib.unpack_tangent(v, self._slot_list)  # v_W halves of all [W | v_W] operands: one launch
            self._conv_slabs(0, s.tbuf, s.cols, vw, s.geo, s.sT)
        self._bn_tangent(s, v, None, 0)
        pn, ph, pw, poh, pow_, c0 = self._pool_geometry()
        self._launch("hf_maxpool_tangent_nhwc", self.pool_t, s.tout, self.pool_idx32, pn, ph, pw, poh, pow_, c0, 2 * c0)

    def _tangent_convs(self, units):
        """The tangent convolutions ``conv([t_x | x], [W | v_W])`` of one or two units in ONE launch.  In front of a
        train-mode BatchNorm the launch's epilogue also writes the per-channel partial sums of its output tiles
        (``hf_conv2d_nhwc_group_slabs_bnsum``): the reduction launch between convolution and elementwise pass is gone
        (``u.tsum``: ``_bn_tangent`` then adds ``u.tp1 / u.tpx`` up instead of ``u.gb / u.gw``)."""
        probs = [(0, u.tbuf, u.xcat, u.wcat, self._tgeo(u), u.sT, 0, 0) for u in units]
        if any(u.epi for u in units):
            sums = [(u.a, u.mean, u.rstd, u.tpx, u.tp1) if u.epi else None for u in units]
            if _lib.conv_group_slabs_bnsum(probs, sums, self.dev):
                for u in units:
                    u.tsum = u.epi
                return
            for u in units:  # (a geometry the 64x64-tile instantiations do not cover: not tried again)
                u.epi = False
        for u in units:
            u.tsum = False
        if len(units) == 1:
            u = units[0]
            self._conv_slabs(0, u.tbuf, u.xcat, u.wcat, self._tgeo(u), u.sT)
        else:
            _lib.conv_group_slabs(probs, self.dev)

    def _tangent_blocks(self, v):
        group = self._grouping()
        for chain, ds, _x in self.blocks[self.dead_blocks:]:  # (dead blocks: frozen, behind frozen layers -- no tangent)
            head = chain[0]
            paired = False
            if ds is not None and group:
                # the downsample branch and the block's first convolution read the same operand:
                # both tangent convolutions in ONE launch
                self._tangent_convs([ds, head])
                alone = head.res_unit is None and not head.res_identity and len(chain) > 1
                paired = alone and not head.train and not ds.train
                if paired:  # ... and both BatchNorm tangents in one
                    self._bn_tangent_pair(ds, head, v)
                elif alone and self._train_pair_ok(ds, head) and ds.tsum and head.tsum:
                    self._bn_tangent_pair_train(ds, head, v)  # (train mode: the same, prologue form)
                    paired = True
                else:
                    self._bn_tangent(ds, v, None, 0)
            elif ds is not None:
                self._tangent_convs([ds])
                self._bn_tangent(ds, v, None, 0)
            for u in chain:
                if u is head and paired:
                    continue
                if not (u is head and ds is not None and group):
                    self._tangent_convs([u])
                add, add_ld = None, 0
                if u.res_unit is not None:
                    add, add_ld = u.res_unit.tout, u.res_unit.tout_ld
                elif u.res_identity:
                    c = head.x.shape[1]
                    add, add_ld = head.xcat[:, :c], 2 * c
                self._bn_tangent(u, v, add, add_ld)

    # ---- classifier head: logits' tangent, loss Hessian, the head's gradients ----------------------
    def _head(self, v):
        """Returns the cotangent of the last unit's output and the head's weight / bias gradients."""
        tail = self.tail
        t_last = tail.tout
        hw = t_last.shape[2] * t_last.shape[3]
        fw = self.fc.weight
        v_fw = self._param_slice(v, self.pfw, fw.numel()).view_as(fw)
        v_fb = self._param_slice(v, self.pfb, fw.shape[0])

        def loss_hessian_of_jv():
            t_feat = t_last.flatten(1) if hw == 1 else t_last.mean(dim=(2, 3))
            if self.pfb is not None:
                Jv = torch.addmm(v_fb, t_feat, fw.detach().t())
            else:
                Jv = t_feat @ fw.detach().t()
            return t_feat, self._loss_hessian(torch.addmm(Jv, self.feat, v_fw.t()))

        if self.hessian:
            # forward-over-reverse through the linear head: besides H_L J v, the first-order cotangent g of the
            # logits meets the tangents of the layer's two operands (g V -> features, g^T t_feat -> weight)
            t_feat, HJv = loss_hessian_of_jv()
            g_fw = torch.addmm(self._gl1.t() @ t_feat, HJv.t(), self.feat)
            g_fb = HJv.sum(0) if self.pfb is not None else None
            g_feat = torch.addmm(self._gl1 @ v_fw, HJv, fw.detach())
            return self._feature_cotangent(g_feat), g_fw, g_fb
        if self._head_fused(hw, v_fw):
            # ONE launch: logits' tangent, softmax-CE Hessian, the three gradients
            g_feat, g_fw, g_fb = self._head_bufs
            self._launch("hf_linear_ce_head", g_feat, g_fw, g_fb if self.pfb is not None else None, t_last, self.feat,
                         fw, v_fw, v_fb, self._ce[0], float(self._ce[1]), g_feat.shape[0], g_feat.shape[1], fw.shape[0])
            if self.pfb is None:
                g_fb = None
        else:
            _t_feat, HJv = loss_hessian_of_jv()
            g_fw = HJv.t() @ self.feat
            g_fb = HJv.sum(0) if self.pfb is not None else None
            g_feat = HJv @ fw.detach()
        return self._feature_cotangent(g_feat), g_fw, g_fb

    def _head_fused(self, hw, v_fw):
        """Whether ``hf_linear_ce_head`` applies: closed-form softmax-CE Hessian, a 1x1 final map
        (the pooling is then the identity), a small dense head, 16-byte aligned operands."""
        ok = getattr(self, "_head_ok", None)
        if ok is None:
            fw = self.fc.weight
            k, f = fw.shape
            ok = (
                self._ce is not None and hw == 1
                and fw.is_contiguous() and fw.dtype == torch.float32
                and head_fused_shape_ok(self.logits.shape[0], f, k)
                and self.feat.is_contiguous() and tuple(self.feat.shape) == (self.logits.shape[0], f)
                and self._offs[self.pfw] % 4 == 0 and self._ce[0].is_contiguous()
            )
            if ok:
                b = self.logits.shape[0]
                g = _lib.load().hf_linear_ce_head_slabs(b)  # partial sums per workgroup, added up by hf_pack_ex
                kw = dict(dtype=torch.float32, device=self.dev)
                self._head_bufs = (torch.empty((b, f), **kw), torch.empty((g, k, f), **kw),
                                   torch.empty((g, k), **kw))
            self._head_ok = ok
        return ok and v_fw.data_ptr() % 16 == 0

    def _grouping(self):
        # (Hessian products carry extra terms per unit: the plain one-unit launches)
        return not self.hessian
