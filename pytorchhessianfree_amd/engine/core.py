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

import os

import torch

from .. import _lib
from ..curvature import GGNOperator
from .common import _Launcher, _Node, _Unsupported, _ce_node, ce_loss_spec, loss_spec_of  # noqa: F401
from .adjoint import _AdjointSweep
from .base import _Engine
from .buffers import _Buffers
from .dataparallel import _DataParallel
from .diag_ef import _DiagEF
from .forward import _Forward
from .hessian import _HessianExtras
from .tangent import _TangentSweep
from .topology import _Topology


class FusedGGNEngine(_Topology, _Buffers, _Forward, _TangentSweep, _AdjointSweep, _HessianExtras, _DiagEF, _DataParallel,
                     _Engine):
    # (the base LAST: ``_DataParallel`` overrides its single-process ``reduce`` / ``reduce_bytes``; ``try_build``, the
    # contract's defaults, ``unavailable`` and the constructors' shared pieces stand in engine/base.py)
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
    supports_hessian = True
    supports_two_phase = True  # (phase_split / local_phase_a / local_phase_b: the chunked, overlapped all-reduce)

    def __init__(self, model, loss, outputs, params, weight, group, hessian=False):
        self._begin(params, weight, group, outputs, hessian)
        self._second = False  # (inside the adjoint sweep of a Hessian product)
        self._diag_batched = os.environ.get("HF_DIAG_EF_BATCHED", "0") == "1"  # (diag_ef: one launch per layer)
        self.dead_blocks = 0
        self._layout(model)
        if self.hessian:
            for u in self.units:
                u.needs_g = True  # (the first-order masked cotangent of every unit is kept)
        self._allocate()
        self.set_batch(getattr(outputs, "_hf_input").detach(), None)
        self.refresh_weights(transposed=True)
        self.train_own = False
        if self.train_bn:
            # train-mode BatchNorm: the engine linearises at the activations and batch statistics the MODEL's
            # forward pass recorded.  Its own forward pass (batch statistics by own kernels, running statistics
            # moved as the layers' forward moves them) lets a persistent session serve such a model too -- if it
            # reproduces the model's output here (with the running statistics left alone)
            if (all(u.bn.momentum is not None and u.bn.track_running_stats for u in self.units if u.train)):
                self.forward_own(update_running=False)
                self.train_own = self._forward_error(outputs) < 1e-4
            self._load_recorded(outputs)
        else:
            # own forward pass on the engine's static buffers; it must reproduce the model's output
            self.forward_own()
            self._check_forward(outputs)
        self._loss_setup(loss, outputs)
        self._verify(loss)
        # ONE linearisation point after construction, whether or not the first-use check ran (it is skipped for a
        # model signature that has passed before): the engine's OWN forward pass where it has one, else -- a
        # train-mode model whose layers the own pass does not reproduce -- everything the model recorded, batch
        # statistics included.  (Round 4 left a train-mode engine whose check was skipped at the recorded
        # activations with its own statistics: 3.65e-6 / one ReLU decision away from the checked one, GPUTEST_r04.)
        if self._at != "own" and (not self.train_bn or self.train_own):
            self.forward_own(update_running=False)  # (eval mode: nothing to move)
            if self.hessian:
                self.gradient()  # the first-order cotangents the Hessian products read, at the same point
        for u in self.units:  # the model's own activations were only needed up to here
            u.rx = u.ry = u.ra = u.rp = None
            u.rec_stats = None
        self._rec_pool = None
        self._release(model)

    # ---- loss Hessian (same contract as GGNOperator) -------------------------------------
    def _loss_setup(self, loss, outputs):
        self._closed_form(loss, outputs)
        # a plain softmax cross-entropy (checked numerically above): the engine can then evaluate
        # loss, probabilities and d loss / d logits itself, on its own forward pass -- which is what
        # lets ONE engine serve many steps and trial points (``session.EngineSession``)
        # ... or a mean-squared error (round 6; the loss of the reference's own examples / tests): gradient
        # 2c (out - t), Hessian 2c I
        self.loss_spec = None
        if not self.train_bn or self.train_own:
            spec = loss_spec_of(loss, outputs)
            if spec is not None and (spec["kind"] == "mse" or self._ce is not None):
                self.loss_spec = spec
                self._set_quadratic(spec.get("quadratic"))
                self.set_targets(spec["targets"])
                if spec["kind"] == "mse":
                    self._ce = None
                    self._mse2 = 2.0 / float(outputs.numel()) if spec["reduction"] == "mean" else 2.0
                self._loss_head()
                if spec["kind"] == "ce":
                    self._ce = (self._p, self._ce[1])  # the static buffer the own forward pass refreshes
                self._dl = None                        # (nothing of this step's autograd graph is kept)
        if self.hessian:
            if self.loss_spec is None:
                raise _Unsupported("Hessian products on the engine need a plain softmax cross-entropy or mean-squared-"
                                   "error loss")
            self.gradient()  # fills the first-order cotangents the Hessian products read

    def gradient(self, out=None):
        """``weight * d loss / d params`` of the softmax cross-entropy by ONE adjoint sweep of the
        engine (the gradient the reference takes with ``torch.autograd.grad``, optimizer.py:231-234),
        on the activations of the last ``forward_own``."""
        if self.loss_spec is None:
            raise RuntimeError("engine.gradient needs a softmax cross-entropy loss")
        if out is None:
            out = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        g = self._dlogits()  # d loss / d logits
        fw = self.fc.weight.detach()
        g_fw = g.t() @ self.feat
        g_fb = g.sum(0) if self.pfb is not None else None
        g_feat = g @ fw
        if self.hessian:
            # the first-order cotangents stay for the step's Hessian products: the sweep below writes the units'
            # g1 / ga1 instead of g / ga (buffers swapped for its duration)
            if getattr(self, "_gl1", None) is None:
                self._gl1 = torch.empty_like(g)
            self._gl1.copy_(g)
            self._swap_first_order()
        try:
            pool_srcs = self._adjoint_blocks(self._feature_cotangent(g_feat))
            self._adjoint_stem(pool_srcs)
        finally:
            if self.hessian:
                self._swap_first_order()
        self._gather(out, g_fw, g_fb, first_order=True)
        if self.hessian and self.train_bn:
            for u in self.units:  # the layer's own first-order parameter gradients: hf_bn_train_hessian_coeffs reads them
                if u.train:
                    torch.sum(u.gw[:u.rb], 0, out=u.gg1)
                    torch.sum(u.gb, 0, out=u.gb1)
        self._add_quadratic(out)
        return out

    def _dlogits(self):
        """``d loss / d logits`` of the engine's own loss head at the current logits."""
        if self.loss_spec["kind"] == "mse":
            return (self.logits - self._targets) * self._mse2
        return (self._p - self._onehot) * self._ce[1]

    def _loss_hessian(self, Jv):
        if self.loss_spec is not None and self.loss_spec["kind"] == "mse":
            return Jv * self._mse2
        return GGNOperator._loss_hessian(self, Jv)

    # ---- the product -------------------------------------------------------------------------
    def local(self, v, out=None):
        v, out = self._product_vectors(v, out)
        self._tangent_stem(v, carry_scatter=True)  # + the v_W halves of all [W | v_W] operands, same launch
        self._tangent_blocks(v)
        if self.hessian:
            if self._vt_slots:
                _lib.unpack_tangent(v, self._vt_slots, half=2)  # V as (I, H, W, O): the operand of conv_D(g, V)
            self._second, self._v = True, v
            self._extras_fork()
        try:
            g_last, g_fw, g_fb = self._head(v)
            pool_srcs = self._adjoint_blocks(g_last)
            self._adjoint_stem(pool_srcs)
            if self.hessian:
                self._extras_join()
        finally:
            self._second, self._v = False, None
        self._gather(out, g_fw, g_fb)
        if self.hessian:  # the regulariser's Hessian: coef on its tensors' entries
            self._add_quadratic(out, v)
        return out

    # ---- the product between vectors in the compact layout (dataparallel.compact_layout) ----------------
    supports_compact = True

    def local_compact(self, vc, out):
        """``local`` on the entries that can be non-zero: ``vc`` and ``out`` are vectors of ``n_live`` entries in
        the compact layout.  Same launches, same buffers, same kernels as ``local``: only the scatter of the v_W
        halves reads, and the gather of the gradients writes, the compact layout (``hf_unpack_weights_compact``,
        ``hf_pack_compact``), and every slice of the vector is taken at its compact offset.  With dead entries of
        ``v`` zero, ``local_compact(gather(v)) == gather(local(v))`` bit for bit."""
        lay = self.compact_layout()
        if lay is None or self.hessian or not self.supports_compact:
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
