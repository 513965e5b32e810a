"""The dense-stack engine: GGN and Hessian products of a prepared MLP (``Linear [ReLU | Tanh] ... Linear``) on the
package's own skinny-GEMM kernels (csrc/hf_dense.hip) -- the nets of the reference's examples/run_mwe.py, run_small_nn.py and of its
own test problem (tests/test_utils.py:19-52)."""

import os

import torch
from torch import nn

from .base import _Engine
from .common import _Unsupported, _flat_view, _same, loss_spec_of, records_of
from .linear import DIAG_EF, GRADIENT, MAX_CLASSES, PRODUCT, _Chain, _Layer  # noqa: F401  (_Layer: plain.py's tail reads it here)

_OPT_IN = "the dense-stack engine is opt-in (set HF_DENSE_ENGINE=1)"


class DenseStackEngine(_Engine):
    """The sweeps of the GGN product for a stack of fully-connected layers.  Per live layer and product: the tangent GEMM
    ``t_x W^T + x V^T`` (W and the vector's slice V read in place in the flat vectors) -> bias tangent and ``act'``;
    the loss Hessian on the output tangent; in reverse ``act'`` and the bias gradient -> the weight gradient, written
    straight into the product vector -> the data gradient.  5 launches per hidden layer, no gather launch, bitwise
    repeatable.  One process.

    Session mode (opt-in: ``HF_DENSE_SESSION=1``; a plain cross-entropy / MSE loss): ``loss_spec`` is set and the engine
    has what ``session.EngineSession`` replays -- ``set_batch`` / ``set_targets`` (copies into static buffers), its own
    forward pass (per layer the forward GEMM and ``hf_dense_act_forward``) ending in its own loss head
    (``hf_dense_loss_head``: probabilities, ``d loss / d logits``, the per-sample cotangents of ``diag_ef``, the loss
    value and the bad-target flag, at most two launches) and ``gradient()`` in GGN mode too.  The kernels read every
    weight in place, trainable or frozen, so there is nothing to refresh per parameter point.  Without the switch
    ``loss_spec`` stays ``None`` and ``step()`` runs as ``engine-graphed``.

    ``hessian=True`` (opt-in: ``HF_DENSE_HESSIAN=1``): the Hessian product by forward over reverse on the same sweeps.
    ``gradient()`` keeps the first-order cotangents ``g_l = h_l * act'(a_l)`` of every live layer (and ``h_l`` of tanh
    layers); the tangent sweep is the GGN's; the adjoint sweep carries the tangents of those cotangents:
    ``g_l' = h_l' * act'(a_l) - 2 a_l t_l h_l`` (the second term for tanh only: ``hf_dense_act_adjoint2``),
    ``(Hv)_W = weight * (g_l'^T a_{l-1} + g_l^T t_{l-1})`` (``hf_dense_wgrad2``), ``h_{l-1}' = g_l' W_l + g_l V_l``
    (``hf_dense_dgrad2_slabs``) -- the cross-layer terms the GGN drops.  Where a term is absent (the first live layer,
    a frozen weight, no tanh) the launch is the GGN's: still 5 launches per hidden layer.

    ``diag_ef``: the diagonal of the empirical Fisher (Martens' preconditioner) of the same batch from ONE adjoint sweep
    with per-sample cotangents -- per layer the weight-gradient GEMM on squared operands and a column sum of squares,
    written straight into the flat vector: at most 4 launches per live layer, no per-sample gradient is formed."""

    mode = ("fused curvature engine (dense stack): own skinny MFMA GEMMs that read the weights and the vector in place "
            "(split reductions as slabs summed by the consumer kernel), bias / activation fused, 5 launches per hidden "
            "layer, weight gradients written straight into the product; Hessian products by forward over reverse on "
            "the same sweeps")
    supports_hessian = True
    supports_session = False  # (per instance: True once the constructor has set up the session mode)
    supports_two_phase = False
    supports_compact = False  # (no kernel taps, no dead entries: solves stay full-length)
    # acc_step builds one engine per data chunk and sums their products: not served here (asked before anything is built)
    acc_decline = "the dense-stack engine serves step() sessions only"
    session_decline = None    # why THIS engine, built with HF_DENSE_SESSION=1, has no session mode
    has_weight_copies = False  # (weights are read in place: a session captures no refresh graph)

    @classmethod
    def unavailable(cls, hessian, need_session):
        # Opt-in until its speed on large MLPs is measured against the hipGraph-replayed autograd sweeps
        # (scripts/bench_dense_engine.py): products are tested, the gain is not.
        if not cls._engine_switch():
            return _OPT_IN
        # Hessian products: opt-in of their own until they beat the hipGraph-replayed double backward by more than the
        # spread of the measurement (profiles/r12_dense_hessian.jsonl)
        if hessian and os.environ.get("HF_DENSE_HESSIAN", "0") != "1":
            return "no Hessian products unless HF_DENSE_HESSIAN=1 (opt-in on top of HF_DENSE_ENGINE=1)"
        reason = super().unavailable(hessian, False)
        # the session: opt-in of its own until a complete step() on it beats the engine-graphed one by more than the
        # spread of the measurement (profiles/r13_dense_session.jsonl: 4.4-4.5 ms gained on
        # 18.2 ms, 5.5-5.9 ms spread)
        if reason is None and need_session and not cls._session_switch():
            reason = "the dense-stack engine has no session yet (opt-in: set HF_DENSE_SESSION=1)"
        return reason

    @staticmethod
    def _engine_switch():
        return os.environ.get("HF_DENSE_ENGINE", "0") == "1"

    @staticmethod
    def _session_switch():
        return os.environ.get("HF_DENSE_SESSION", "0") == "1"

    def __init__(self, model, loss, outputs, params, weight, group, hessian=False):
        self._begin(params, weight, group, outputs, hessian)
        if group is not None:
            raise _Unsupported("data parallelism is not implemented for dense stacks")
        self.loss_spec = None  # (set by _loss_setup in session mode: no own loss head before)
        self._layout(model)
        self._allocate()
        self.forward_own()
        self._check_forward(outputs)
        self._loss_setup(loss, outputs)
        self._verify(loss)
        if self._at != "own":
            self.forward_own()
        if self.hessian:
            self.gradient()  # the first-order cotangents the Hessian products read, at the final linearisation point
        self.chain.release()
        self._release(model)

    # ---- topology ----------------------------------------------------------------------------
    def _layout(self, model):
        x_in = getattr(self.outputs, "_hf_input", None)
        if not isinstance(x_in, torch.Tensor) or x_in.dtype != torch.float32 or not x_in.is_cuda:
            raise _Unsupported("no recorded float32 GPU input")
        leaves = [m for m in model.modules() if not list(m.children())]
        chain = _Chain(self.dev, self._offs, (nn.ReLU, nn.Tanh), ("linear", "stack", "batch {} > {} rows"))
        layers, cur, i = chain.layers, x_in.detach(), 0
        while i < len(leaves):
            m = leaves[i]
            dropout = isinstance(m, (nn.Dropout, nn.Dropout1d, nn.Dropout2d, nn.Dropout3d, nn.AlphaDropout))
            if isinstance(m, nn.Identity) or (dropout and (not m.training or m.p == 0)):
                i += 1
                continue
            if dropout:
                raise _Unsupported("a training-mode model with active dropout")
            if type(m) is nn.Flatten and not layers:
                fx, fy = records_of(m, with_input=True)
                if not _same(fx, cur) or fy.dim() != 2:
                    raise _Unsupported("Flatten does not turn the input into [batch, features]")
                cur = fy
            elif type(m) is nn.Linear:
                i, cur = chain.layout_layer(leaves, i, cur, self._param)
                continue
            else:
                raise _Unsupported(f"unsupported layer {type(m).__name__}")
            i += 1
        if not layers:
            raise _Unsupported("no Linear layer")
        self.rows = chain.check_end(self.outputs.detach())
        used = {k for u in layers for k in (u.pw, u.pb) if k is not None}
        if used != set(range(len(self.params))):
            raise _Unsupported("the parameter list has entries the engine's layers do not cover")
        self.dead_layers = chain.mark_dead_prefix()
        self.chain, self.layers, self.model_ref, self._in_shape = chain, layers, model, tuple(x_in.shape)

    def _allocate(self):
        # the input in the MODEL's shape (what a session's ``set_batch`` receives); the first layer reads it flattened
        self.x_in = torch.empty(self._in_shape, dtype=torch.float32, device=self.dev)
        x2d = self.x_in.view(self.rows, self.layers[0].c_in)
        self.logits = self.chain.allocate(self.rows, x2d, None, hessian=self.hessian)
        x2d.copy_(self.layers[0].rx)
        self._g_last = torch.empty_like(self.logits)
        # (a tangent GEMM with no live term: only the bias of the first live layer carries a tangent)
        self.chain.zero = torch.zeros(self.rows * max(u.c_out for u in self.layers), dtype=torch.float32, device=self.dev)
        # the parameters as ONE flat vector, when they are consecutive views of one (the optimizer's arena): a session
        # is valid only while they stay where its graphs read them
        self._flat_params = _flat_view(self.params, self.n)

    def _flat(self, noun, *vecs):
        for t in vecs:
            if t.dtype != torch.float32 or t.numel() != self.n or not t.is_contiguous() or t.device != self.dev:
                raise RuntimeError(f"dense-stack engine: {noun} must be contiguous float32 of the parameters' size")

    # ---- forward -----------------------------------------------------------------------------
    def forward_own(self, refresh=False, update_running=True):
        """The model's forward pass on the static buffers (``_Chain.forward``: two launches per layer); in session mode the
        loss head.  Weights are read in place (``refresh``: nothing to do), no running statistics; capturable."""
        self.chain.forward()
        if self.loss_spec is not None:
            self._loss_head()
        self._at = "own"
        return self.logits

    def _load_recorded(self, outputs):
        self.chain.load_recorded()  # (the MODEL's activations: the ReLU decisions of the operator it is compared with)
        if self.loss_spec is not None:
            self._loss_head()
        self._at = "recorded"

    # ---- loss --------------------------------------------------------------------------------
    def _loss_setup(self, loss, outputs):
        self._closed_form(loss, outputs)
        self._mse2 = None
        if self._ce is None:
            spec = loss_spec_of(loss, outputs)
            if spec is None or spec["kind"] != "mse":
                raise _Unsupported("the loss is neither a plain softmax cross-entropy nor a mean-squared error")
            self._mse2 = 2.0 / float(outputs.numel()) if spec["reduction"] == "mean" else 2.0
        elif self._ce[0].shape[1] > MAX_CLASSES:
            raise _Unsupported(f"more than {MAX_CLASSES} classes")
        else:  # (no host read of the targets: a batch with an ignored target has failed the closed form's check)
            spec = loss_spec_of(loss, outputs, check_values=False)
        # diag_ef: the reduction of a PLAIN cross-entropy / MSE (None: no per-sample reading of this loss) and the
        # per-sample cotangents at the logits -- a `mean` loss carries 1/N, `loss_function(model(x_i), t_i)` does not
        self._reduction = spec["reduction"] if spec is not None and "quadratic" not in spec else None
        self._g_ef = None
        if self._reduction is not None:
            per_sample = float(outputs.shape[0]) if self._reduction == "mean" else 1.0
            self._g_ef = (self._dl.detach() * per_sample).contiguous()
        self._h_last = self._dl.detach().contiguous() if self.hessian else None  # d loss / d logits
        self._dl = None
        if not self._session_switch():  # (no own loss head without the session mode: loss_spec stays None)
            return
        if self._reduction is None:
            self.session_decline = ("the dense-stack engine's session takes a plain cross-entropy / MSE loss (no "
                                    "quadratic regulariser)")
            return
        # session mode: the engine's own loss head fills static buffers at every forward pass
        rows, c = self.logits.shape
        mean = self._reduction == "mean"
        if self._ce is not None:
            self._kind, self._scale_g, self._coef = 0, float(self._ce[1]), (1.0 / rows if mean else 1.0)
            self._p = torch.empty_like(self.logits)
            self._ce = (self._p, self._ce[1])  # the static buffer hf_softmax_ce_hvp reads
        else:
            self._kind, self._scale_g, self._coef = 1, self._mse2, (1.0 / (rows * c) if mean else 1.0)
            self._p = None
        self._scale_ps = self._scale_g * (float(rows) if mean else 1.0)
        self._targets = torch.empty_like(spec["targets"], memory_format=torch.contiguous_format)
        self._targets.copy_(spec["targets"])
        self._h_last, self._g_ef = torch.empty_like(self.logits), torch.empty_like(self.logits)
        self.loss_buf = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.bad_targets = torch.zeros((), dtype=torch.int32, device=self.dev)
        self._work = torch.empty(512, dtype=torch.float64, device=self.dev)
        self.loss_spec, self.supports_session = spec, True
        self._sig_slots = self._signature_slots()
        self._sig_frozen = self.chain.frozen_tensors()
        self._loss_head()

    def _loss_head(self):
        """Session mode: probabilities, ``d loss / d logits``, the per-sample cotangents, the loss value and the
        bad-target flag of the current logits and targets -- one call of ``hf_dense_loss_head`` (two launches)."""
        rows, c = self.logits.shape
        self._launch("hf_dense_loss_head", self._kind, self.logits, self._targets, self._p, self._h_last, self._g_ef,
                     self.loss_buf, self.bad_targets, self._work, self._scale_g, self._scale_ps, self._coef, rows, c)

    # ---- per batch / per parameter point (session mode) ----------------------------------------------------------
    def _session_only(self, what):
        if self.loss_spec is None:
            raise RuntimeError(f"the dense-stack engine has no {what} without its session mode (HF_DENSE_SESSION=1, a "
                               "plain cross-entropy / MSE loss): it then serves products of one batch only")

    def set_batch(self, x, targets=None):
        """A new input batch of the same shape (and its targets): copies into the static buffers."""
        self._session_only("set_batch")
        if tuple(x.shape) != tuple(self._in_shape):
            raise RuntimeError("engine: input shape changed")
        self.x_in.copy_(x)
        if targets is not None:
            self.set_targets(targets)

    def set_targets(self, targets):
        self._session_only("set_targets")
        if targets.dtype.is_floating_point != (self._kind == 1) or tuple(targets.shape) != tuple(self._targets.shape):
            raise RuntimeError("engine: the targets are not those of the loss the engine was built for")
        self._targets.copy_(targets)

    def refresh_weights(self, transposed=False):
        """Nothing to do: the kernels read every weight in place, trainable or frozen."""
        self._session_only("refresh_weights")

    def refresh_frozen(self):
        self._session_only("refresh_frozen")

    def _signature_slots(self):
        """Where the model holds its ``Linear`` / activation / Dropout modules -- ``(parent, name)`` per module, found
        by ONE walk at construction: the per-step signature looks the slots up instead of walking the module tree."""
        kinds = (nn.Linear, nn.ReLU, nn.Tanh, nn.Dropout, nn.Dropout1d, nn.Dropout2d, nn.Dropout3d, nn.AlphaDropout)
        return [(parent, name) for parent in self.model_ref.modules() for name, child in parent._modules.items()
                if isinstance(child, kinds)]

    def layer_signature(self):
        """What the captured graphs of a session bake in about the model besides shapes: the identities of the modules
        the MODEL holds now where its ``Linear`` / activation / Dropout modules stood at construction (a swapped layer
        is another stack), every Dropout's ``(training, p)``, the addresses of FROZEN weights and biases (kernel
        arguments; the trainable ones are covered by the flat vector's address) and ``model.training``.  Compared
        several times per step: a few dictionary look-ups, no walk over the module tree (a module ADDED elsewhere shows
        up in the periodic re-verification against the model's own forward pass)."""
        self._session_only("layer_signature")
        now = [parent._modules.get(name) for parent, name in self._sig_slots]
        mods = tuple((id(m), getattr(m, "training", None), getattr(m, "p", None)) for m in now)
        frozen = tuple(t.data_ptr() for t in self._sig_frozen)
        return mods, frozen, bool(self.model_ref.training)

    def gradient(self, out=None):
        """The first-order adjoint sweep from ``d loss / d logits`` at the activations the buffers hold: keeps ``g_l`` of
        every live layer (``h_l`` of tanh layers) for the Hessian products; with ``out`` also ``weight * d loss /
        d params`` in the flat vector.  In session mode also for a GGN engine: its cotangents go through the products'
        own ``ga`` buffers (nothing is kept).  Existing kernels only; no allocation, no host synchronisation."""
        if not self.hessian and self.loss_spec is None:
            raise RuntimeError("the dense-stack engine keeps first-order cotangents in Hessian mode only")
        if out is not None:
            self._flat("the gradient", out)
        self.chain.adjoint(GRADIENT, self._h_last, out, self.weight)
        return out

    # ---- the product -------------------------------------------------------------------------
    def local(self, v, out=None):
        v, out = self._product_vectors(v, out)
        self._flat("vector and product", v, out)
        t_x = self.chain.tangent(v)
        if self._ce is not None:
            self._launch("hf_softmax_ce_hvp", self._g_last, self._ce[0], t_x, float(self._ce[1]), self.rows,
                         self.logits.shape[1])
        else:
            torch.mul(t_x, self._mse2, out=self._g_last)
        self.chain.adjoint(PRODUCT, self._g_last, out, self.weight, v=v)
        return out

    # ---- diagonal of the empirical Fisher ---------------------------------------------------------
    def diag_ef(self, reduction="mean", out=None):
        """``sum_i g_i^2`` (``sum``) / ``(1/N) sum_i g_i^2`` (``mean``) over the per-sample gradients ``g_i`` of the
        engine's batch: the quantity of ``preconditioners.diag_EF_autograd`` / ``diag_EF_backpack``.  The per-sample
        weight gradient of a ``Linear`` layer is the outer product ``g_a[r] (x) x[r]``, so the layer's entries are
        ``sum_r g_a[r][o]^2 x[r][i]^2`` (``hf_dense_sq_wgrad``) and ``sum_r g_a[r][o]^2`` (``hf_dense_sq_colsum``) of ONE
        adjoint sweep whose cotangents are the per-sample ones; the ``1/N`` of ``mean`` is the kernels' ``scale``.
        Frozen parameters have no entry; the rank ``weight`` does not enter.  No allocation (given ``out``), no host
        synchronisation: capturable on one stream."""
        if reduction not in ("sum", "mean"):
            raise ValueError(f"reduction {reduction} is not supported.")
        if self._reduction is None:
            raise RuntimeError("engine.diag_ef needs a plain softmax cross-entropy / MSE loss")
        if self._reduction != reduction:
            raise RuntimeError("engine.diag_ef: the loss's reduction differs from the requested one")
        if self._at != "own":
            raise RuntimeError("engine.diag_ef: the engine's buffers do not hold its own forward pass")
        if out is None:
            out = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        self._flat("the diagonal", out)
        self.chain.adjoint(DIAG_EF, self._g_ef, out, scale=1.0 / self.rows if reduction == "mean" else 1.0)
        return out


def diag_ef_of(model, loss_function, inputs, targets, reduction, why=None):
    """The diagonal of the empirical Fisher of ``loss_function(model(inputs), targets)`` on the dense-stack engine, or
    ``None`` (``why``, a list, receives the reason): the switch is unset, the tensors are not CUDA float32, the model
    has a convolution or is no prepared MLP the engine covers, batch > 256, another loss.  Only this engine kind is
    ever built from here."""
    why = [] if why is None else why
    if not DenseStackEngine._engine_switch():
        why.append(_OPT_IN)
        return None
    if not (isinstance(inputs, torch.Tensor) and inputs.is_cuda and inputs.dtype == torch.float32):
        why.append("the inputs are not a CUDA float32 tensor")
        return None
    params = [p for p in model.parameters() if p.requires_grad]
    if not params or any(not p.is_cuda or p.dtype != torch.float32 for p in params):
        why.append("the parameters are not CUDA float32 tensors")
        return None
    if any(isinstance(m, nn.Conv2d) for m in model.modules()):
        why.append("a model with convolutions is no dense stack")
        return None
    outputs = model(inputs)
    loss = loss_function(outputs, targets)
    if not isinstance(outputs, torch.Tensor) or not isinstance(loss, torch.Tensor) or not loss.requires_grad:
        why.append("the loss does not depend on the parameters")
        return None
    eng = DenseStackEngine.try_build(loss, outputs, params, why=why)
    if eng is None:
        return None
    if eng._reduction is None:
        why.append("DenseStackEngine: the loss has no per-sample reading (neither a plain cross-entropy nor an MSE)")
        return None
    if eng._reduction != reduction:  # (the caller's own construction answers, as with a conv engine's session)
        why.append(f"DenseStackEngine: the loss's reduction ({eng._reduction}) differs from the requested one")
        return None
    return eng.diag_ef(reduction)
