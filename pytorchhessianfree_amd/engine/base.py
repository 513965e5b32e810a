"""What every engine kind is, and nothing about convolutions: the contract sessions and the optimizer read, the choice
of a kind for a model (``try_build``), the shared pieces of the kinds' constructors and the first-use check.

The kinds: ``FusedGGNEngine`` (engine/core.py: residual nets) and ``PlainStackEngine`` (engine/plain.py: conv + bias
stacks), siblings on ``_ConvEngine`` (engine/conv.py: the conv mixins, one constructor, one ``local``, one ``gradient``;
its docstring lists the hooks a conv kind supplies), and ``DenseStackEngine`` (engine/dense.py, this base alone).  A kind
provides ``_layout``, ``_allocate``, ``forward_own``, ``_load_recorded``, ``_loss_setup``, ``local``, ``gradient`` and --
with a ``loss_spec`` -- ``set_batch`` / ``set_targets`` / ``refresh_weights`` / ``layer_signature``."""

import os
import warnings

import torch

from .. import _lib
from ..curvature import GGNOperator, _Operator
from .common import _Launcher, _Node, _Unsupported, _ce_node


class _Engine(_Launcher, _Operator):
    # ---- the contract: what callers read of ANY kind (class defaults; a constructor may set its instance's) ----------
    mode = "fused curvature engine"  # one sentence for ``path_report()``: what runs
    supports_hessian = True      # Hessian products (``hessian=True``) besides the GGN's
    supports_session = True      # own forward pass, loss head and gradient sweep: serves a persistent session
    supports_two_phase = False   # phase_split / local_phase_a / local_phase_b: the chunked, overlapped all-reduce
    supports_compact = False     # compact_layout / local_compact: the product between vectors of the live entries
    acc_decline = None           # why this kind does not serve acc_step's accumulated session, if it does not
    session_decline = None       # why THIS engine, once built, has no session mode, if it has none
    has_weight_copies = True     # refresh_weights launches something (a session captures it as a graph of its own)
    hessian = False              # this engine's products are Hessian products
    train_bn = False             # the model has train-mode BatchNorm layers (batch statistics in the sweeps)
    frozen_any = False           # a layer parameter is frozen: a constant of the product, no entry in the vector
    _l2 = None                   # per-entry coefficients of the loss's quadratic (L2) term, or ``None``
    # relative max-norm distance to the autograd product above which the engine is refused; fp32
    # products of the shipped workloads agree to ~1e-6.  Deep, badly conditioned nets (the random-init
    # ResNet-50) scatter more for EVERY fp32 implementation: callers that have measured what stock
    # fp32 autograd achieves against float64 (bench.py) raise it to max(1e-5, 5 x that error) -- on
    # ``FusedGGNEngine``, for all kinds (``_verify``)
    verify_tol = 1e-5

    @classmethod
    def unavailable(cls, hessian, need_session):
        """Why this kind cannot serve a caller who wants Hessian products / a persistent session, or ``None``."""
        if hessian and not cls.supports_hessian:
            return "no Hessian products (GGN only)"
        if need_session and not cls.supports_session:
            return "no persistent session on this engine yet"
        return None

    @classmethod
    def try_build(cls, loss, outputs, params, weight=1.0, group=None, hessian=False, why=None, need_session=False,
                  for_acc=False):
        """The engine for the model that produced ``outputs``, or ``None``; ``why`` (a list) receives one line per
        reason it was not taken -- what ``HessianFree.path_report()`` and its one-time warning quote.
        ``need_session``: the caller (a persistent session) needs the engine's own forward pass, loss head and
        gradient sweep; kinds without them are not built.  ``for_acc``: the caller is ``acc_step``'s accumulated session
        (one engine per data chunk); kinds that serve ``step()`` sessions only (``acc_decline``) are not built."""
        why = [] if why is None else why
        if os.environ.get("HF_ENGINE", "1") == "0":
            why.append("the fused engine is switched off (HF_ENGINE=0)")
            return None
        ref = getattr(outputs, "_hf_model", None)
        model = ref() if ref is not None else None
        if model is None:
            why.append("the model is not a prepared one (modelprep.prepare_model(model, channels_last=True) installs "
                       "the layers the fused engine reads)")
            return None
        if not outputs.is_cuda or outputs.dtype != torch.float32 or outputs.dim() != 2:
            why.append(f"the model output is not a CUDA float32 [batch, classes] tensor (got {outputs.dtype}, "
                       f"{tuple(outputs.shape)}, {outputs.device})")
            return None
        from .core import FusedGGNEngine
        from .dense import DenseStackEngine
        from .plain import PlainStackEngine

        kinds = [cls] if cls is not FusedGGNEngine else [FusedGGNEngine, PlainStackEngine, DenseStackEngine]
        if any(isinstance(m, torch.nn.Conv2d) for m in model.modules()):
            kinds = [k for k in kinds if k is not DenseStackEngine]  # (a conv net is no dense stack: nothing to say)
        for kind in kinds:
            # (asked of the CLASS, in the kinds' order: nothing is built that the caller could not use)
            reason = kind.unavailable(hessian, need_session)
            if reason is None and for_acc:
                reason = kind.acc_decline
            if reason is not None:
                why.append(f"{kind.__name__}: {reason}")
                continue
            try:
                return kind(model, loss, outputs, params, weight, group, hessian=hessian)
            except _Unsupported as exc:
                # (a model the engine does not cover is the normal case: quiet unless asked;
                # a product that FAILED its check is always reported)
                why.append(f"{kind.__name__}: {exc}")
                if os.environ.get("HF_ENGINE_DEBUG") or getattr(exc, "loud", False):
                    warnings.warn(f"fused curvature engine ({kind.__name__}) not used: {exc}")
                if getattr(exc, "loud", False):
                    return None
            except _lib.Refused as exc:  # a kernel refused its arguments (alignment, size limits ...)
                why.append(f"{kind.__name__}: a kernel refused its arguments: {exc}")
                warnings.warn(f"fused curvature engine ({kind.__name__}) not used: {exc}")
                return None
        return None

    # ---- the shared pieces of the kinds' constructors ----------------------------------------------------
    def _begin(self, params, weight, group, outputs, hessian):
        """The operator part and what every layout reads: where each parameter sits in the list and the flat vector."""
        _Operator.__init__(self, params, weight, group)
        self.hessian = bool(hessian)
        self.outputs, self.dev = outputs, outputs.device
        self._index = {id(p): i for i, p in enumerate(self.params)}
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o += p.numel()
        self._offs = offs
        self.train_bn, self.frozen_any, self._l2 = False, False, None

    def _forward_error(self, outputs):
        """Relative max-norm distance of the engine's logits to the model's output."""
        want = outputs.detach()
        return float((self.logits - want).abs().max() / want.abs().max().clamp_min(1e-30))

    def _check_forward(self, outputs):
        err = self._forward_error(outputs)
        if not err < 1e-4:
            raise _Unsupported(f"the engine's forward pass differs from the model's output by {err:.2e}")

    def _release(self, model):
        """With an own loss head nothing of the step's autograd graph stays alive in the engine."""
        if self.loss_spec is not None:
            self.outputs = None
            from ..modelprep import release_records

            release_records(model)  # (the layers' records pinned this pass's activations until the next one)

    # ---- helpers of the layouts, loss heads and products ---------------------------------------------------
    def _param(self, p):
        """Index of a layer parameter in the optimizer's (trainable) list; ``None``: the layer has no such parameter
        or it is FROZEN (``requires_grad = False``: it is a constant of the product -- no tangent, no gradient entry;
        reference utils.py:31-32 skips it the same way)."""
        if p is None:
            return None
        i = self._index.get(id(p))
        if i is None:
            if p.requires_grad:
                raise _Unsupported("a trainable layer parameter is not among the optimizer's parameters")
            self.frozen_any = True
        return i

    def _closed_form(self, loss, outputs):
        """``_dl``: d loss / d outputs with its graph; ``_ce``: the softmax cross-entropy's Hessian in closed form, or
        ``None`` (same contract as ``GGNOperator``)."""
        (self._dl,) = torch.autograd.grad(loss, outputs, create_graph=True, retain_graph=True)
        self._ce = GGNOperator._closed_form_loss_hessian(self, _Node(_ce_node(loss)), outputs)

    def _set_quadratic(self, terms):
        """``loss = cross-entropy + sum_j 0.5 * coef_j * ||w_j||^2`` (the L2 term of the reference's
        All-CNN-C example, examples/example_utils.py:77-81): per-entry coefficients of the flat vector.
        Loss value, gradient and Hessian product of that term are ``0.5 <d*theta, theta>``,
        ``d*theta`` and ``d*v``."""
        self._l2 = None
        if not terms:
            return
        d = torch.zeros(self.n, dtype=torch.float32, device=self.dev)
        for coef, tensors in terms:
            for w in tensors:
                i = self._index.get(id(w))
                if i is None:
                    # (a frozen tensor would add a constant to the loss value the engine's own loss head reports)
                    raise _Unsupported("a regularised tensor is not among the optimizer's parameters")
                d[self._offs[i]: self._offs[i] + w.numel()] += float(coef)
        self._l2 = d

    def _theta(self):
        flat = self._flat_params
        if flat is not None and flat.data_ptr() == self.params[0].data_ptr():
            return flat
        return torch.cat([p.detach().reshape(-1) for p in self.params])

    def _add_quadratic(self, out, x=None):
        """``out += weight * d * x``: the quadratic term's share of a product with ``x``, or (``x=None``: the
        parameters themselves) of the gradient."""
        if self._l2 is not None:
            out.addcmul_(self._l2, self._theta() if x is None else x, value=self.weight)

    def _product_vectors(self, v, out):
        """``local``'s operands: the vector detached and contiguous, the product allocated unless given."""
        if out is None:
            out = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        v = v.detach()
        if not v.is_contiguous():
            v = v.contiguous()
        return v, out

    # ---- one process: the kinds with data parallelism override both (engine/dataparallel.py) ------------------
    @property
    def reduce_bytes(self):
        return 4 * self.n

    def reduce(self, t, group=None):
        return t

    def __call__(self, v, out=None):
        self.calls += 1
        return self.reduce(self.local(v, out))

    # ---- safety net --------------------------------------------------------------------------
    def _verify(self, loss):
        """First product of every (model, shape) signature against the autograd operator, both on the
        activations the model's own forward pass recorded (``_load_recorded``)."""
        policy = os.environ.get("HF_ENGINE_VERIFY", "first")
        key = ("hessian" if self.hessian else "ggn", self.train_bn,
               tuple(type(m).__name__ for m in self.model_ref.modules()), self.n,
               tuple(tuple(p.shape) for p in self.params), tuple(self.logits.shape), tuple(self.x_in.shape),
               str(self.dev))
        # (kept ON the model: a registry keyed by id(model) outlives the model, and CPython hands the address of a
        # collected model to the next one)
        verified = self.model_ref.__dict__.setdefault("_hf_engine_verified", set())
        if policy == "never" or (policy != "always" and key in verified):
            return
        gen = torch.Generator(device=self.dev).manual_seed(4321)
        v = torch.randn(self.n, device=self.dev, generator=gen)
        weight, self.weight = self.weight, 1.0
        self._load_recorded(self.outputs)
        try:
            if self.hessian:
                self.gradient()  # first-order cotangents at the recorded activations
            got = self.local(v).clone()
        finally:
            self.weight = weight  # (the constructor moves the engine to its final linearisation point afterwards)
        if self.hessian:
            from ..curvature import HessianOperator

            want = HessianOperator(loss, self.params).local(v)
        else:
            want = GGNOperator(loss, self.outputs, self.params).local(v)
        err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
        # (callers raise the tolerance in ONE place, ``FusedGGNEngine.verify_tol``, and it holds for every kind: read
        # there, not on ``type(self)``; imported here because core.py imports this module)
        from .core import FusedGGNEngine

        # (Hessian products through batch statistics: stock fp32 double backward is itself 6e-6 from float64 on the
        # train-mode ResNet-18, this engine 3e-6 ... 7e-6 -- two fp32 results may be the sum of both apart)
        tol = FusedGGNEngine.verify_tol * (3.0 if (self.hessian and self.train_bn) else 1.0)
        if not err < tol:
            exc = _Unsupported(f"engine {'Hessian ' if self.hessian else ''}product differs from the autograd product by {err:.2e} "
                               f"(tolerance {tol:.1e}); using the autograd operator")
            exc.loud = True
            raise exc
        verified.add(key)
