"""Fused curvature engine: the GGN product ``v -> J^T H_L J v`` of a prepared ResNet-family
model (conv - eval-BatchNorm - ReLU units with residual connections, NHWC fp32) by EXPLICIT
tangent and adjoint sweeps over its layers, issued as direct kernel launches.

Why.  The reference obtains the product from BackPACK's R-op / L-op (optimizer.py:457-462), i.e.
from autograd; so does ``curvature.GGNOperator``.  On an MI355X that product is bound by the
NUMBER of dependent launches (~170 x ~6 us for ResNet-18 on 28x28 inputs), and the convolutions
inside it are MIOpen split-K kernels: a zero-fill launch + a kernel that accumulates with
atomics (not repeatable).  Here every convolution is ONE launch of the package's implicit-GEMM
kernels (hf_conv.hip) whose split-K partial results ("slabs") are summed by the kernel that
CONSUMES them, in its prologue -- the launch boundary publishes them, there is no zero-fill, no
atomic, no in-launch reduction:

    tangent sweep, per unit :  T-conv([t_x | x], [W | v_W]) -> slabs
                               BatchNorm tangent (+ residual tangent, ReLU mask) sums the slabs and
                               writes straight into the next unit's [t_x | x] operand
    adjoint sweep, per unit :  BatchNorm adjoint: g = mask * (sum of the consumers' cotangent slabs),
                               g_a = g * w * rstd, per-channel sums      (hf_chan_affine_bwd_ex)
                               data + weight gradient of the convolution in ONE launch -> slabs
    once per product        :  hf_unpack_tangent_ex (v_W of all layers), hf_maxpool_tangent_nhwc,
                               hf_linear_ce_head (logits' tangent, loss Hessian, the head's three
                               gradients), hf_maxpool_adjoint_nhwc, hf_pack_ex (all parameter
                               gradients, summing the weight-gradient slabs while it gathers);
                               slices of kernel taps that never meet data are skipped throughout

4 launches per conv-BN unit instead of 8 -- 2 where a block's first convolution and its downsample
branch share their launches (grouped kernels) --, 74 per product of ResNet-18; bitwise repeatable.  Under
data parallelism only the entries of the product that can be non-zero are all-reduced (``reduce``).
The layer topology is taken from the prepared model's module tree and from the activations its
patched layers recorded during the step's forward pass (``modelprep`` stores them detached);
anything the engine does not recognise makes ``try_build`` return ``None`` and the caller uses
the autograd operator.  The first product of every model signature is compared with that
operator's product on a random vector.
"""

import torch

from .. import _lib
from .common import _Unsupported, _cl, _pair
from .conv import _ConvEngine
from .problems import sources
from .tangent import head_fused_shape_ok
from .topology import _Topology


class FusedGGNEngine(_Topology, _ConvEngine):
    # (``_Topology``: the residual layout, dead prefix, two-phase split; here its walks, the stem's max-pool, the head)
    mode = ("fused curvature engine: own deterministic convolutions (split-K slabs summed by the consumer "
            "kernel), BatchNorm tangents/adjoints fused, 4 launches per conv-BN unit, downsample branches grouped "
            "with their block's first convolution")

    # Hessian products (optimizer.py:450-455) by forward-over-reverse on the same kernels; residual nets with
    # EVAL-mode BatchNorm (the layer is a per-channel affine map; ReLU masks and max-pool positions are
    # piecewise constant): per unit, besides the GGN's terms, conv_D(g, V) and conv_W(t_x, g) (g: the step's
    # first-order cotangent, kept by the gradient sweep) as MORE SLABS of the same buffers, and the BatchNorm
    # scale's own second-order terms  g_a' += g_z * rstd * v_gamma ,  g_gamma' += sum g_z * rstd * t_a .
    # TRAIN-mode BatchNorm (round 5): the batch statistics' share of the adjoint's tangent in closed form per channel
    # (hf_bn_train_hessian_coeffs / _apply; the formulas stand in csrc/hf_bn.hip and DESIGN.md section 4.3).
    supports_two_phase = True  # (phase_split / local_phase_a / local_phase_b: the chunked, overlapped all-reduce)
    supports_compact = True    # (compact_layout / local_compact)

    # ---- buffers of the stem's max-pool and of the head ---------------------------------------------------
    def _allocate_pool(self):
        self.pool_t = self._xcats.get(id(self.pool_out))
        if self.pool_t is None:
            raise _Unsupported("nothing consumes the pooled stem output")
        if _pair(self.pool_args[3]) != [1, 1] or self.pool_args[4]:
            raise _Unsupported("max-pool with dilation / ceil_mode")
        self.pool_idx32 = torch.empty(tuple(self.pool_out.permute(0, 2, 3, 1).shape), dtype=torch.int32,
                                      device=self.dev)
        self._g_stem = torch.empty_like(self.stem.y)

    def _allocate_head(self):
        """Classifier head: (global average pool ->) linear layer."""
        self._allocate_pool()
        f32, dev = torch.float32, self.dev
        tail = self.tail
        n, k = tail.y.shape[0], tail.y.shape[1]
        self._head_hw = tail.y.shape[2] * tail.y.shape[3]
        if self._head_hw == 1:
            self.feat = tail.y.permute(0, 2, 3, 1).reshape(n, k)  # a view: NHWC with a 1x1 map is [n, k]
            if self.feat.data_ptr() != tail.y.data_ptr():
                raise _Unsupported("feature view")
        else:
            self.feat = torch.empty((n, k), dtype=f32, device=dev)
        self.logits = torch.empty((n, self.fc.weight.shape[0]), dtype=f32, device=dev)
        self._p = torch.empty_like(self.logits)
        self.loss_buf = torch.zeros((), dtype=f32, device=dev)

    def _pool_geometry(self):
        """(n, h, w, oh, ow, c) of the stem's max-pool (window maxima's positions: ``forward_own``)."""
        pn, _, ph, pw = self.stem.y.shape
        return pn, ph, pw, self.pool_out.shape[2], self.pool_out.shape[3], self.pool_out.shape[1]

    def _adjoint_order(self):
        """The units in the order the adjoint sweep visits them."""
        order = []
        for chain, ds, _x in reversed(self.blocks):
            order += list(reversed(chain)) + ([ds] if ds is not None else [])
        return order + [self.stem]

    # ---- forward -----------------------------------------------------------------------------
    def _forward_units(self, refresh, update_running):
        s = self.stem
        flat = self._flat_params
        carried = (refresh and flat is not None and flat.data_ptr() == self.params[0].data_ptr()
                   and self._conv_carrying_scatter(s, s.conv.weight.detach(), s.sF, flat, 0))
        if not carried:
            if refresh:
                self.refresh_weights()
            self._conv_forward(s)
        self._bn_forward(s, s.sF, update_running)
        ks, st_, pd, _dl, _cm = self.pool_args
        pn, ph, pw, poh, pow_, c0 = self._pool_geometry()
        (kh, kw), (sh, sw), (pph, ppw) = _pair(ks), _pair(st_ if st_ is not None else ks), _pair(pd)
        self._launch("hf_maxpool_forward_nhwc", self.pool_out, self.pool_t[:, c0:], 2 * c0, self.pool_idx32, s.y, pn, ph, pw,
                     poh, pow_, c0, kh, kw, sh, sw, pph, ppw)
        for chain, ds, _x in self.blocks:
            if ds is not None:
                self._conv_forward(ds)
                self._bn_forward(ds, ds.sF, update_running)
            for u in chain:
                self._conv_forward(u)
                self._bn_forward(u, u.sF, update_running)
        if self._head_hw > 1:
            torch.mean(self.tail.y, dim=(2, 3), out=self.feat)
        fw = self.fc.weight.detach()
        if self.pfb is not None:
            torch.addmm(self.fc.bias.detach(), self.feat, fw.t(), out=self.logits)
        else:
            torch.mm(self.feat, fw.t(), out=self.logits)

    def _load_recorded(self, outputs):
        super()._load_recorded(outputs)
        ks, st_, pd, dl, cm = self.pool_args  # the positions of the MODEL's windows, its pooled map, its features
        _, idx = torch.nn.functional.max_pool2d(self.stem.ry, ks, st_, pd, dl, cm, return_indices=True)
        self.pool_idx32.copy_(idx.permute(0, 2, 3, 1))
        self.pool_out.copy_(self.stem.rp)
        c0 = self.pool_out.shape[1]
        self.pool_t[:, c0:].copy_(self.stem.rp)
        if self._head_hw > 1:
            torch.mean(self.tail.y, dim=(2, 3), out=self.feat)

    # ---- tangent sweep -------------------------------------------------------------------------
    def _tangent_sweep(self, v):
        self._tangent_stem(v)  # + the v_W halves of all [W | v_W] operands, same launch
        self._tangent_blocks(v)

    def _tangent_stem(self, v):
        """Stem: conv(x, v_W) as a 1x1 convolution on the im2col'd input (the input has no tangent; v_W is a
        slice of ``v`` itself).  The launch also carries the scatter of every other layer's v_W into its ``[W | v_W]``
        operand (``hf_conv2d_nhwc_slabs_unpack``) -- nothing in the stem reads those."""
        s = self.stem
        if s.dead:  # (frozen stem: its output carries no tangent -- only the scatter it would have carried is left)
            if self._slot_list:
                _lib.unpack_tangent(v, self._slot_list)
            return
        vw = self._weight_tangent(v, s)  # (zeros for a frozen stem weight under a trainable BatchNorm)
        if not self._conv_carrying_scatter(s, vw, s.sT, v, 1):
            _lib.unpack_tangent(v, self._slot_list)  # v_W halves of all [W | v_W] operands: one launch
            self._conv_slabs(0, s.tbuf, s.cols, vw, s.geo, s.sT)
        self._bn_tangent(s, v, None, 0)
        pn, ph, pw, poh, pow_, c0 = self._pool_geometry()
        self._launch("hf_maxpool_tangent_nhwc", self.pool_t, s.tout, self.pool_idx32, pn, ph, pw, poh, pow_, c0, 2 * c0)

    def _tangent_blocks(self, v):
        group = self._grouping()
        for chain, ds, _x in self.blocks[self.dead_blocks:]:  # (dead blocks: frozen, behind frozen layers -- no tangent)
            head = chain[0]
            paired = False
            if ds is not None and group:
                # the downsample branch and the block's first convolution read the same operand:
                # both tangent convolutions in ONE launch
                self._tangent_convs([ds, head])
                alone = head.res_unit is None and head.res_identity is None and len(chain) > 1
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
                elif u.res_identity is not None:
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

    def _first_order_seed(self):
        """The gradient sweep's seed: ``d loss / d logits`` through the linear layer."""
        g = self._dlogits()
        fw = self.fc.weight.detach()
        g_fw = g.t() @ self.feat
        g_fb = g.sum(0) if self.pfb is not None else None
        g_feat = g @ fw
        if self.hessian:  # (the head of a Hessian product reads the logits' first-order cotangent)
            if self._gl1 is None:
                self._gl1 = torch.empty_like(g)
            self._gl1.copy_(g)
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

    # ---- adjoint sweep -------------------------------------------------------------------------
    def _adjoint_sweep(self, g_last):
        self._adjoint_stem(self._adjoint_blocks(g_last))

    def _adjoint_blocks(self, g_last, first=None, last_block=0, incoming=None):
        """Walks the blocks ``first`` (default: the last one) ... ``last_block`` backwards; returns the
        two cotangents of the pooled stem output -- or, when the walk stops before block 0, the state
        (``incoming``) a later call continues from (the product in two phases, ``local_phases``)."""
        group = self._grouping()
        tail = self.tail
        if incoming is None:
            incoming = {id(tail): [(g_last, 1, 0)]}
        pool_srcs = None
        first = len(self.blocks) - 1 if first is None else first
        stop = max(last_block, self.dead_blocks)  # (dead blocks: nobody needs their cotangents)
        for bi in range(first, stop - 1, -1):
            chain, ds, _x = self.blocks[bi]
            head, last = chain[0], chain[-1]
            for k in range(len(chain) - 1, -1, -1):
                u = chain[k]
                if k == 0 and ds is not None and group:
                    # both BatchNorm adjoints, then the data + weight gradients of the block's first
                    # convolution AND of its downsample branch in ONE launch (four problems)
                    if u.rb > 1 and ds.rb > 1 and not u.train and not ds.train:
                        self._bn_adjoint_pair(u, incoming.pop(id(u)), ds, [(last.g, 1, 0)])
                    elif u.rb > 1 and ds.rb > 1 and self._train_pair_ok(u, ds):
                        self._bn_adjoint_pair_train(u, incoming.pop(id(u)), ds, [(last.g, 1, 0)])
                    else:
                        self._bn_adjoint(u, incoming.pop(id(u)))
                        self._bn_adjoint(ds, [(last.g, 1, 0)])
                    # (a block input that carries no tangent: the two weight gradients only)
                    probs = [q for b in (u, ds) for q in self._dw_problems(b, b.ga, dgrad=not u.no_dgrad)]
                    self._launch("hf_conv2d_nhwc_group_slabs", probs, len(probs))
                else:
                    self._adjoint_unit(u, incoming.pop(id(u)))
                if k > 0:
                    incoming.setdefault(id(chain[k - 1]), []).append((u.dbuf, self._dslabs(u), u.dbuf.shape[1]))
            if head.no_dgrad:  # (everything in front of this block is frozen: the sweep ends here)
                if ds is not None and not group:
                    self._adjoint_unit(ds, [(last.g, 1, 0)])
                return None
            # the block input receives conv1's data gradient and the residual branch's cotangent
            srcs = [(head.dbuf, self._dslabs(head), head.dbuf.shape[1])]
            if ds is not None:
                if not group:
                    self._adjoint_unit(ds, [(last.g, 1, 0)])
                srcs.append((ds.dbuf, self._dslabs(ds), ds.dbuf.shape[1]))
            else:
                srcs.append((last.g, 1, 0))
            if bi > 0:
                incoming[id(self.blocks[bi - 1][0][-1])] = srcs
            else:
                pool_srcs = srcs
        return pool_srcs if last_block == 0 else incoming

    def _adjoint_stem(self, pool_srcs):
        """Block 0's input is the pooled stem output: sum its two cotangents, undo the max-pool,
        then the stem's own adjoint."""
        s = self.stem
        if s.dead or pool_srcs is None:  # (frozen stem: nothing to differentiate)
            return
        ks, st_, pd, dl, cm = self.pool_args
        pn, ph, pw, poh, pow_, c0 = self._pool_geometry()
        self._extras_wait(pool_srcs)
        # slab sums of both cotangents and the max-pool adjoint (gather form) in one launch
        g_stem = self._g_stem
        (kh, kw), (sh, sw), (pph, ppw) = _pair(ks), _pair(st_ if st_ is not None else ks), _pair(pd)
        self._launch("hf_maxpool_adjoint_nhwc", g_stem, *sources("max-pool", pool_srcs), self.pool_idx32, pn, ph, pw, poh,
                     pow_, c0, kh, kw, sh, sw, pph, ppw)
        self._adjoint_unit(s, [(g_stem, 1, 0)])

    def _feature_cotangent(self, g_feat):
        tail = self.tail
        if self._head_hw == 1:
            return g_feat.view(tail.y.shape)
        return _cl((g_feat / self._head_hw).view(g_feat.shape[0], -1, 1, 1).expand(tail.y.shape))

    def _head_entries(self, tensors, splits, g_fw, g_fb):
        """The head's weight / bias gradients as entries of ``hf_pack_ex``'s tables (copies of them)."""
        tensors, splits = list(tensors), dict(splits)
        if g_fw.dim() == 3:  # the head kernel's per-workgroup partial sums: slabs for hf_pack_ex
            tensors[self.pfw] = g_fw[0]
            splits[self.pfw] = (g_fw.shape[0], g_fw[0].numel())
            if self.pfb is not None:
                tensors[self.pfb] = g_fb[0]
                splits[self.pfb] = (g_fb.shape[0], g_fb.shape[1])
        else:
            tensors[self.pfw] = g_fw
            if self.pfb is not None:
                tensors[self.pfb] = g_fb
        return tensors, splits

    # ---- diag_ef: the linear head in closed form -------------------------------------------------------
    def _diag_head_buffers(self, tensors):
        """(filled in closed form afterwards: zeros here)"""
        self._diag_zero_fw = torch.zeros(self.fc.weight.numel(), dtype=torch.float32, device=self.dev)
        tensors[self.pfw] = self._diag_zero_fw
        if self.pfb is not None:
            self._diag_zero_fb = torch.zeros(self.fc.weight.shape[0], dtype=torch.float32, device=self.dev)
            tensors[self.pfb] = self._diag_zero_fb

    def _diag_head(self, out, scale):
        """The per-sample weight gradient is the outer product g_i x feat_i, so the sum of its squares is
        (g o g)^T (feat o feat)."""
        g = self._dlogits() * scale
        nf = self.fc.weight.numel()
        out[self._offs[self.pfw]: self._offs[self.pfw] + nf].copy_(((g * g).t() @ (self.feat * self.feat)).reshape(-1))
        if self.pfb is not None:
            out[self._offs[self.pfb]: self._offs[self.pfb] + g.shape[1]].copy_((g * g).sum(0))

    # ---- the product in two phases (``phase_split``) -------------------------------------------------
    def local_phase_a(self, v, out, split):
        """Tangent sweep, head, adjoint sweep of blocks ``cut ...``, and the suffix of the product they
        determine (``out[offset:]``)."""
        cut, first, offset = split
        v = v.detach()
        self._tangent_sweep(v)
        g_last, g_fw, g_fb = self._head(v)
        self._phase_state = self._adjoint_blocks(g_last, last_block=cut)
        self._gather_range(out, g_fw, g_fb, first, len(self.params))

    def local_phase_b(self, out, split):
        """The rest of the adjoint sweep and ``out[:offset]``."""
        cut, first, offset = split
        pool_srcs = self._adjoint_blocks(None, first=cut - 1, last_block=0, incoming=self._phase_state)
        self._adjoint_stem(pool_srcs)
        self._gather_range(out, None, None, 0, first)

    # ---- the product between vectors in the compact layout (dataparallel.compact_layout) ----------------
    def local_compact(self, vc, out):
        """``local`` on the entries that can be non-zero: ``vc`` and ``out`` are vectors of ``n_live`` entries in
        the compact layout.  Same launches, same buffers, same kernels as ``local``: only the scatter of the v_W
        halves reads, and the gather of the gradients writes, the compact layout (``hf_unpack_weights_compact``,
        ``hf_pack_compact``), and every slice of the vector is taken at its compact offset.  With dead entries of
        ``v`` zero, ``local_compact(gather(v)) == gather(local(v))`` bit for bit."""
        lay = self.compact_layout()
        if lay is None or self.hessian:
            raise RuntimeError("engine: no compact layout for this product")
        slots = self.__dict__.get("_compact_slots")
        if slots is None:
            slots = self._compact_slots = [
                (lay["offs"][u.pw],) + self._tangent_slots[id(u)][1:] + (lay["nl"].get(u.pw, 0),)
                for u in self.units if id(u) in self._tangent_slots]
        saved = self._offs, self._slot_list
        self._offs, self._slot_list, self._compact_nl = lay["offs"], slots, lay["nl"]
        try:
            return self.local(vc, out=out)
        finally:
            (self._offs, self._slot_list), self._compact_nl = saved, None
