"""A chain of ``Linear [LayerNorm] [activation]`` layers on the skinny GEMMs of csrc/hf_dense.hip (batches up to 256 rows) or, as a
``tall`` chain, on the LDS-tiled GEMMs of csrc/hf_dense_tall.hip (257 .. 8192 rows) -- the layout of one layer, the static
buffers, the forward / tangent / adjoint loops: what the dense-stack engine (engine/dense.py) runs on.  The plain-stack
engine's classifier tail (engine/plain.py) is the same chain and still carries loops of its own.  A layer with a
``LayerNorm`` between the ``Linear`` and its activation (the skinny chain only; a caller's opt-in kind) takes the row-resident
kernels of csrc/hf_ln.hip where a plain layer takes the elementwise passes: 6 launches per product instead of 5."""

import torch
from torch import nn

from .. import _lib
from .common import _P, _Launcher, _Unsupported, _same, mark_dead_prefix, records_of

MAX_ROWS, MAX_CLASSES = 256, 1024  # the skinny dense kernels' row limit; the loss heads' class limit
MAX_TALL_ROWS = 8192               # the tall kernels' (hf_dense_tall.hip)
MAX_LN_FEATURES = 16384            # a LayerNorm layer's row: one workgroup's LDS tile (hf_ln.hip)
_ACT = {None: 0, nn.ReLU: 1, nn.Tanh: 2}
GRADIENT, PRODUCT, DIAG_EF = range(3)  # what an adjoint sweep is for
# the entry points whose arguments are the same in both kernel families, by the chain's form (``tall``)
_NAMES = {False: {"plan": "hf_dense_plan", "slabs": "hf_dense_tangent_slabs", "forward": "hf_dense_act_forward",
                  "tangent": "hf_dense_act_tangent"},
          True: {"plan": "hf_dense_tall_plan", "slabs": "hf_dense_tall_tangent_slabs",
                 "forward": "hf_dense_tall_act_forward", "tangent": "hf_dense_tall_act_tangent"}}


class _Layer:
    """``Linear(+bias) [LayerNorm] [ReLU | Tanh]``: the module, its activation code, parameter indices and static buffers;
    with a LayerNorm (``ln``) the indices of its scale and shift (``pg`` / ``pb_ln``), the recorded output of the ``Linear``
    (``ra``) and the buffers ``xh`` (the normalised row), ``rstd`` and ``s`` (the cotangent behind the activation)."""

    def __init__(self, lin, act, ln=None):
        self.lin, self.act, self.ln = lin, act, ln
        self.c_out, self.c_in = lin.weight.shape
        self.dead = self.first_live = False
        self.g1 = self.h1 = None
        self.pg = self.pb_ln = self.ra = self.xh = self.rstd = self.s = None


class _Chain(_Launcher):
    """The layers of one chain and their launches, on the engine's device and its offsets into the flat vectors.  ``acts``:
    the activations accepted behind a ``Linear``; ``words``: a layer's and the chain's name in decline reasons, the row
    limit's message; ``tall_switch``: the name of the caller's opt-in switch for batches beyond ``MAX_ROWS`` and whether it
    is set (``None``: the caller has no such form); ``ln_switch``: the same for the LayerNorm layer kind."""

    def __init__(self, dev, offs, acts, words, tall_switch=None, ln_switch=None):
        self.dev, self.offs, self.acts, self.tall_switch, self.ln_switch = dev, offs, acts, tall_switch, ln_switch
        self.tall, self.names = False, _NAMES[False]
        self.name, self.whole, self.rows_msg = words
        self.layers, self.dead, self.zero = [], 0, None  # (zero: a slab of zeros, where a first layer may have no ``t_x``)

    def _at(self, vec, index):
        """The address of parameter ``index`` in the flat vector ``vec``; ``None`` without a vector or for a frozen one."""
        return None if vec is None or index is None else _P(vec.data_ptr() + 4 * self.offs[index])

    # ---- layout and static buffers -----------------------------------------------------------------
    def layout_layer(self, leaves, i, cur, param):
        """The ``Linear [LayerNorm] [activation]`` at ``leaves[i]``, which must read ``cur`` (``param``: the engine's
        ``_param``); returns the next index and the layer's output record."""
        m, name = leaves[i], f"{self.name} {len(self.layers)}"
        cx, cy = records_of(m, with_input=True)
        if cx.dim() != 2 or not _same(cx, cur):
            raise _Unsupported(f"{name}: its input is not the previous [batch, features] activation")
        nxt = leaves[i + 1] if i + 1 < len(leaves) else None
        act, y, ln, ra = None, cy, None, None
        if type(nxt) is nn.LayerNorm and self.ln_switch is not None:
            ln, ra, i = nxt, cy, i + 1
            cy = self._layout_ln(m, ln, name, cy)
            nxt, y = leaves[i + 1] if i + 1 < len(leaves) else None, cy
        if type(nxt) in self.acts:
            if getattr(nxt, "inplace", False):
                noun = self.acts[0].__name__ if len(self.acts) == 1 else "activation"
                raise _Unsupported(f"{name}: followed by an in-place {noun}")
            rx, ry = records_of(nxt, with_input=True)
            if not _same(rx, cy):
                raise _Unsupported(f"{type(nxt).__name__} does not read {name}'s output")
            act, y, i = type(nxt), ry, i + 1
        u = _Layer(m, _ACT[act], ln)
        u.name, u.rx, u.ry, u.ra = name, cx, y, ra
        u.pw = param(m.weight)
        u.pb = param(m.bias) if m.bias is not None else None
        if ln is not None:
            u.pg, u.pb_ln = param(ln.weight), param(ln.bias)
        self.layers.append(u)
        return i + 1, y

    def _layout_ln(self, lin, ln, name, cy):
        """What a LayerNorm behind the ``Linear`` ``lin`` must be to join its layer; returns the LayerNorm's output record."""
        switch, on = self.ln_switch
        c = lin.weight.shape[0]
        if not on:
            raise _Unsupported(f"{name}: followed by a LayerNorm (LayerNorm layers are opt-in: {switch}=1)")
        if tuple(ln.normalized_shape) != (c,):
            raise _Unsupported(f"{name}: LayerNorm over {tuple(ln.normalized_shape)}, not over the layer's {c} features")
        if not ln.elementwise_affine or ln.weight is None or ln.bias is None:
            raise _Unsupported(f"{name}: a LayerNorm without elementwise_affine scale and shift is not covered")
        if lin.bias is None:
            raise _Unsupported(f"{name}: a Linear without bias in front of a LayerNorm is not covered")
        if c > MAX_LN_FEATURES:
            raise _Unsupported(f"{name}: LayerNorm over {c} features > {MAX_LN_FEATURES} (one workgroup's LDS tile)")
        lx, ly = records_of(ln, with_input=True)
        if not _same(lx, cy):
            raise _Unsupported(f"LayerNorm does not read {name}'s output")
        return ly

    def check_end(self, out):
        """What the chain as a whole must be; returns its rows."""
        if not self.layers or self.layers[-1].act != 0:
            raise _Unsupported(f"the {self.whole} does not end in a Linear layer")
        last = self.layers[-1].ry
        if out.data_ptr() != last.data_ptr() or tuple(out.shape) != tuple(last.shape):
            raise _Unsupported("the network output is not the last Linear layer's output")
        rows = int(out.shape[0])
        if rows > MAX_ROWS:
            name, on = self.tall_switch or (None, False)
            if not on or rows > MAX_TALL_ROWS:
                hint = "" if name is None else (f" ({name}=1 serves up to {MAX_TALL_ROWS})" if on else
                                                f" (up to {MAX_TALL_ROWS} rows are opt-in: {name}=1)")
                raise _Unsupported(self.rows_msg.format(rows, MAX_ROWS) + hint)
            if any(u.ln is not None for u in self.layers):
                raise _Unsupported(f"batch {rows}: LayerNorm layers are not covered on the tall chain (beyond {MAX_ROWS} rows)")
            self.tall, self.names = True, _NAMES[True]
        return rows

    def mark_dead_prefix(self):
        """Frozen layers at the input end are dead for both sweeps; the first live one needs no data gradient."""
        self.dead = mark_dead_prefix(self.layers)
        self.layers[self.dead].first_live = True
        return self.dead

    def frozen_tensors(self):
        """The FROZEN weights and biases (LayerNorm scales and shifts included): kernel arguments of captured graphs, so
        part of a session's signature."""
        ln = lambda u: ((u.ln.weight, u.pg), (u.ln.bias, u.pb_ln)) if u.ln is not None else ()  # noqa: E731
        return [t for u in self.layers for t, k in ((u.lin.weight, u.pw), (u.lin.bias, u.pb), *ln(u))
                if k is None and t is not None]

    def allocate(self, rows, x, t_x, hessian=False):
        """Per layer the plan's split-K slab counts, output and tangent slabs; per LIVE layer tangent, cotangent
        and (unless ``first_live``) data-gradient slabs, on a Hessian engine ``g1`` / ``h1``; on a tall chain the two
        workspaces the plan sizes (weight-gradient slabs, the row blocks' column partials), shared by the layers.  The
        first layer reads ``x`` (``t_x``: its tangent, or ``None``)."""
        f32, dev, lib = torch.float32, self.dev, _lib.load()
        self.rows, self.hessian = rows, hessian
        ws_w = ws_col = 0
        for u in self.layers:
            counts = [_lib.c_int() for _ in range(4 if self.tall else 2)]
            _lib.check(getattr(lib, self.names["plan"])(rows, u.c_in, u.c_out, *counts), self.names["plan"])
            u.sT, u.sD, u.x, u.t_x = counts[0].value, counts[1].value, x, t_x
            if self.tall:
                u.sW = counts[2].value
                ws_w = max(ws_w, u.sW * u.c_out * u.c_in if u.sW > 1 else 0)
                ws_col = max(ws_col, counts[3].value * u.c_out)
            u.y = torch.empty((rows, u.c_out), dtype=f32, device=dev)
            u.tslabs = torch.empty((u.sT, rows * u.c_out), dtype=f32, device=dev)
            x = u.y
            if u.ln is not None:  # (the forward launch fills both, on a dead layer too)
                u.xh, u.rstd = torch.empty_like(u.y), torch.empty(rows, dtype=f32, device=dev)
            if u.dead:
                continue
            u.ty, u.ga = torch.empty_like(u.y), torch.empty_like(u.y)
            u.s = torch.empty_like(u.y) if u.ln is not None else None
            u.dslabs = None if u.first_live else torch.empty((u.sD, rows * u.c_in), dtype=f32, device=dev)
            if hessian:  # first-order g_l = h_l * act'(a_l); h_l where the activation has a curvature
                u.g1 = torch.empty_like(u.y)
                u.h1 = torch.empty_like(u.y) if u.act == 2 else None
            t_x = u.ty
        if self.tall:  # (launches of one stream: one workspace of each kind serves every layer in turn)
            self.ws_w = torch.empty(max(ws_w, 1), dtype=f32, device=dev)
            self.ws_col = torch.empty(ws_col, dtype=torch.float64, device=dev)
        return self.layers[-1].y

    def release(self):  # (the model's own activations were only needed up to the end of the construction)
        for u in self.layers:
            u.rx = u.ry = None

    # ---- launches ----------------------------------------------------------------------------
    def _slabs(self, u, t_x, v_w):
        """``u.tslabs <- t_x W^T + x V^T`` (either term may be absent, not both)."""
        self._launch(self.names["slabs"], u.tslabs, t_x, u.x, u.lin.weight, v_w, self.rows, u.c_in, u.c_out, 0, u.sT,
                     u.tslabs.shape[1])

    def _ln_forward(self, u, slabs, splits, bias):
        """``u.y, u.xh, u.rstd`` of the pre-activation ``sum of slabs (+ bias)``: the LayerNorm layer's forward launch."""
        self._launch("hf_ln_act_forward", u.y, u.xh, u.rstd, slabs, splits, u.tslabs.shape[1], bias, u.ln.weight, u.ln.bias,
                     float(u.ln.eps), u.act, self.rows, u.c_out)

    def forward(self):
        """The tangent kernel with ``t_x = NULL, V = W`` is the forward GEMM; then slab sum, bias, activation in one pass
        (a LayerNorm layer: slab sum, bias, statistics, normalisation, scale / shift and activation in one pass)."""
        for u in self.layers:
            self._slabs(u, None, u.lin.weight)
            if u.ln is not None:
                self._ln_forward(u, u.tslabs, u.sT, u.lin.bias)
                continue
            self._launch(self.names["forward"], u.y, u.tslabs, u.sT, u.tslabs.shape[1], u.lin.bias, u.act, self.rows,
                         u.c_out)

    def load_recorded(self):
        """The MODEL's recorded activations (the ReLU decisions of the autograd operator the first product is compared with).
        A LayerNorm layer's ``xh`` and ``rstd`` are not recorded: its forward launch runs on the RECORDED output of the
        ``Linear`` (one slab, the bias already in it), then the recorded activation replaces the launch's own."""
        self.layers[0].x.copy_(self.layers[0].rx)
        for u in self.layers:
            if u.ln is not None:
                u.tslabs[0].view(self.rows, u.c_out).copy_(u.ra)
                self._ln_forward(u, u.tslabs, 1, None)
            u.y.copy_(u.ry)

    def tangent(self, v):
        """Through the live layers; V and the bias tangents are read in place in ``v`` (frozen: NULL).  Returns ``t_logits``."""
        for u in self.layers[self.dead:]:
            v_w, v_b = self._at(v, u.pw), self._at(v, u.pb)
            if u.t_x is None and v_w is None:
                slabs, splits = self.zero, 1
            else:
                self._slabs(u, u.t_x, v_w)
                slabs, splits = u.tslabs, u.sT
            if u.ln is not None:
                self._launch("hf_ln_act_tangent", u.ty, slabs, splits, u.tslabs.shape[1], v_b, u.xh, u.rstd, u.ln.weight,
                             self._at(v, u.pg), self._at(v, u.pb_ln), u.y, u.act, self.rows, u.c_out)
                continue
            self._launch(self.names["tangent"], u.ty, slabs, splits, u.tslabs.shape[1], v_b, u.y, u.act, self.rows, u.c_out)
        return u.ty

    # the launches whose arguments differ between the two families: ONE place each that knows both spellings
    def _act_adjoint(self, u, g, o_b, src, y, act, scale, t_y=None, h=None):
        """``g <- (sum of slabs) * act'(y)`` (+ the tanh curvature term where ``t_y`` / ``h`` are given), ``o_b``: its
        column sums times ``scale``."""
        slabs, splits, stride = src
        if self.tall:
            self._launch("hf_dense_tall_act_adjoint", g, o_b, self.ws_col, slabs, splits, stride, y, act, t_y, h, self.rows,
                         u.c_out, scale)
        elif t_y is not None:
            self._launch("hf_dense_act_adjoint2", g, o_b, slabs, splits, stride, y, act, t_y, h, self.rows, u.c_out, scale)
        else:
            self._launch("hf_dense_act_adjoint", g, o_b, slabs, splits, stride, y, act, self.rows, u.c_out, scale)

    def _ln_adjoint(self, u, src, out, diag, scale):
        """A LayerNorm layer's two adjoint launches: the rows (``u.s`` behind the activation, ``u.ga`` at the ``Linear``'s
        output), then the columns -- scale, shift and the ``Linear``'s bias straight into ``out``, times ``scale`` (``diag``:
        their sums of squares); no column launch where all three are frozen."""
        slabs, splits, stride = src
        self._launch("hf_ln_act_adjoint", u.ga, u.s, slabs, splits, stride, u.xh, u.rstd, u.ln.weight, u.y, u.act, self.rows,
                     u.c_out)
        o_g, o_be, o_b = self._at(out, u.pg), self._at(out, u.pb_ln), self._at(out, u.pb)
        if o_g is not None or o_be is not None or o_b is not None:
            self._launch("hf_ln_param_sums", o_g, o_be, o_b, u.s, u.xh, u.ga, int(diag), scale, self.rows, u.c_out)

    def _wgrad(self, u, o_w, mode, g, x, g2, x2, scale):
        """``o_w <- scale * g^T x``; ``mode`` 1: on squared operands, 2: ``+ g2^T x2``."""
        if self.tall:
            self._launch("hf_dense_tall_wgrad", o_w, self.ws_w, g, x, g2, x2, self.rows, u.c_in, u.c_out, mode, scale, u.sW)
        elif mode == 2:
            self._launch("hf_dense_wgrad2", o_w, g, x, g2, x2, self.rows, u.c_in, u.c_out, scale)
        else:
            self._launch(("hf_dense_wgrad", "hf_dense_sq_wgrad")[mode], o_w, g, x, self.rows, u.c_in, u.c_out, scale)

    def _dgrad(self, u, g, g2, v_w):
        """``u.dslabs <- g W`` (``+ g2 V`` where given)."""
        tail = (self.rows, u.c_in, u.c_out, u.sD, u.dslabs.shape[1])
        if self.tall:
            self._launch("hf_dense_tall_dgrad_slabs", u.dslabs, g, u.lin.weight, g2, v_w, *tail)
        elif g2 is not None:
            self._launch("hf_dense_dgrad2_slabs", u.dslabs, g, u.lin.weight, g2, v_w, *tail)
        else:
            self._launch("hf_dense_dgrad_slabs", u.dslabs, g, u.lin.weight, *tail)

    def adjoint(self, what, seed, out=None, weight=1.0, v=None, scale=None):
        """THE adjoint sweep: from the cotangent ``seed`` at the logits through the live layers in reverse, per layer the
        activation adjoint (a LayerNorm layer: its row and column launches, ``_ln_adjoint``, which write every bias-like
        output) -> the weight output -> (``DIAG_EF``) the bias output -> the data gradient, as slabs the next
        activation adjoint sums; a ``first_live`` layer stops before its data gradient.  Weight / bias outputs: the
        parameters' places in the flat ``out`` (none without one), times ``weight``.
        ``GRADIENT`` keeps ``g_l`` (``h_l`` of tanh layers) where a Hessian engine has buffers for them; ``PRODUCT`` carries,
        on a Hessian engine, the second-order terms of ``v``; ``DIAG_EF`` writes sums of squares times ``scale`` (per-sample
        cotangents: ``weight`` does not enter, the bias has a kernel of its own).  Returns the last ``(slabs, splits, stride)``."""
        diag, second = what == DIAG_EF, what == PRODUCT and self.hessian
        src = (seed, 1, 0)
        for u in reversed(self.layers[self.dead:]):
            o_w, o_b = self._at(out, u.pw), self._at(out, u.pb)
            g = u.g1 if what == GRADIENT and u.g1 is not None else u.ga
            if what == GRADIENT and u.h1 is not None:  # h_l itself: the slab sum, no factor
                self._act_adjoint(u, u.h1, None, src, None, 0, 1.0)
            if u.ln is not None:  # (GGN sweeps only: no Hessian engine is built over a LayerNorm layer)
                self._ln_adjoint(u, src, out, diag, scale if diag else weight)
            elif second and u.act == 2:  # tanh: the curvature term -2 a t_a h
                self._act_adjoint(u, g, o_b, src, u.y, u.act, weight, u.ty, u.h1)
            else:
                self._act_adjoint(u, g, None if diag else o_b, src, u.y, u.act, 1.0 if diag else weight)
            if o_w is not None and diag:
                self._wgrad(u, o_w, 1, g, u.x, None, None, scale)
            elif o_w is not None and second and u.t_x is not None:  # + g^T t_x (none enters the first live layer)
                self._wgrad(u, o_w, 2, g, u.x, u.g1, u.t_x, weight)
            elif o_w is not None:
                self._wgrad(u, o_w, 0, g, u.x, None, None, weight)
            if o_b is not None and diag and u.ln is None:
                if self.tall:
                    self._launch("hf_dense_tall_sq_colsum", o_b, self.ws_col, g, self.rows, u.c_out, scale)
                else:
                    self._launch("hf_dense_sq_colsum", o_b, g, self.rows, u.c_out, scale)
            if u.first_live:
                break
            if second and u.pw is not None:  # + g V (a frozen weight has no tangent)
                self._dgrad(u, g, u.g1, self._at(v, u.pw))
            else:
                self._dgrad(u, g, None, None)
            src = (u.dslabs, u.sD, u.dslabs.shape[1])
        return src
