"""What is true of a LIST of conv units, whatever wires them: the constructor, the loss head, and the skeleton of the
own forward pass, the product and the gradient.  The unit-level launches stand in the mixins; nothing here or there knows
a stem, a block or a classifier layer.  A conv kind -- ``FusedGGNEngine`` (core.py: residual nets), ``PlainStackEngine``
(plain.py: conv + bias stacks) -- supplies its wiring (the whole list; contracts in DESIGN.md section 4.2): ``_layout``,
``_allocate_head``, ``_forward_units(refresh, update_running)``, its extension of ``_load_recorded``, ``_tangent_sweep(v)``,
``_head(v)`` and ``_first_order_seed()`` (both ``-> (g_last, g_fw, g_fb)``; ``g_fw is None``: no head entries to gather),
``_adjoint_sweep(g_last)``, ``_adjoint_order()`` and, for a head with parameters, ``_diag_head_buffers`` / ``_diag_head``."""

import os

import torch

from .. import _lib
from ..curvature import GGNOperator
from .adjoint import _AdjointSweep
from .base import _Engine
from .buffers import _Buffers
from .common import _Unsupported, loss_spec_of
from .dataparallel import _DataParallel
from .diag_ef import _DiagEF
from .forward import _Forward
from .hessian import _HessianExtras
from .tangent import _TangentSweep


class _ConvEngine(_Buffers, _Forward, _TangentSweep, _AdjointSweep, _HessianExtras, _DiagEF, _DataParallel, _Engine):
    # (the base LAST: ``_DataParallel`` overrides its single-process ``reduce`` / ``reduce_bytes``; ``try_build``, the
    # contract's defaults, ``unavailable`` and the constructors' shared pieces stand in engine/base.py)

    # (a Hessian product forks its side branch in front of the head -- or behind it, where the head is ONE launch)
    _fork_behind_head = False

    def __init__(self, model, loss, outputs, params, weight, group, hessian=False):
        self._begin(params, weight, group, outputs, hessian)
        self._second = False  # (inside the adjoint sweep of a Hessian product)
        self._diag_batched = os.environ.get("HF_DIAG_EF_BATCHED", "0") == "1"  # (diag_ef: one launch per layer)
        self.loss_spec = self._gl1 = self._pack = self._diag_pack = self._compact_nl = None
        self._extras_allowed = True  # (False: the caller runs this engine on one of several parallel capture branches)
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
        self._release(model)

    def layer_signature(self):
        """What the captured graphs of a session bake in about the model's layers besides shapes: module
        identities and every BatchNorm's mode / eps / momentum (kernel arguments).  Compared per step."""
        return tuple((id(u.conv), id(u.bn), None if u.bn is None else (u.bn.training, u.bn.eps, u.bn.momentum))
                     for u in self.units) + (bool(self.model_ref.training) if not self.units[0].bn is None else None,)

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

    def _dlogits(self):
        """``d loss / d logits`` of the engine's own loss head at the current logits."""
        if self.loss_spec["kind"] == "mse":
            return (self.logits - self._targets) * self._mse2
        return (self._p - self._onehot) * self._ce[1]

    def _loss_hessian(self, Jv):
        if self.loss_spec is not None and self.loss_spec["kind"] == "mse":
            return Jv * self._mse2
        return GGNOperator._loss_hessian(self, Jv)

    # ---- own forward pass --------------------------------------------------------------------
    def forward_own(self, refresh=False, update_running=True):
        """The network's forward pass on the engine's static buffers, own kernels only: every
        activation lands where the sweeps read it (dense output = ReLU mask / weight-gradient operand
        / residual, and the x half of the consumer's [t_x | x] operand), max-pool positions, logits
        and -- for a softmax cross-entropy -- probabilities and the loss value.  ``refresh``: first bring
        the W halves of all [W | v_W] operands up to the current parameters (``refresh_weights()``) -- carried
        by the first convolution's launch where possible (an im2col'd layer reads its weight from the parameter)."""
        self._forward_units(refresh, update_running)
        if self.loss_spec is not None:
            self._loss_head()
        self._at = "own"
        return self.logits

    # ---- the product and the gradient: one skeleton ------------------------------------------
    def local(self, v, out=None):
        v, out = self._product_vectors(v, out)
        self._tangent_sweep(v)  # + the v_W halves of all [W | v_W] operands
        if self.hessian:
            if self._vt_slots:
                _lib.unpack_tangent(v, self._vt_slots, half=2)  # V as (I, H, W, O): the operand of conv_D(g, V)
            self._second, self._v = True, v
            if not self._fork_behind_head:
                self._extras_fork()
        try:
            g_last, g_fw, g_fb = self._head(v)
            if self.hessian and self._fork_behind_head:
                self._extras_fork()
            self._adjoint_sweep(g_last)
            if self.hessian:
                self._extras_join()
        finally:
            self._second, self._v = False, None
        self._gather(out, g_fw, g_fb)
        if self.hessian:  # the regulariser's Hessian: coef on its tensors' entries
            self._add_quadratic(out, v)
        return out

    def gradient(self, out=None):
        """``weight * d loss / d params`` of the engine's own loss head by ONE adjoint sweep of the
        engine (the gradient the reference takes with ``torch.autograd.grad``, optimizer.py:231-234),
        on the activations of the last ``forward_own``."""
        if self.loss_spec is None:
            raise RuntimeError("engine.gradient needs a softmax cross-entropy loss")
        if out is None:
            out = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        g_last, g_fw, g_fb = self._first_order_seed()
        if self.hessian:
            # the first-order cotangents stay for the step's Hessian products: the sweep below writes the units'
            # g1 / ga1 instead of g / ga (buffers swapped for its duration)
            self._swap_first_order()
        try:
            self._adjoint_sweep(g_last)
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
