"""A chain of ``Linear [activation]`` layers on the skinny GEMMs of csrc/hf_dense.hip -- the layout of one layer, the static
buffers, the forward / tangent / adjoint loops: what the dense-stack engine (engine/dense.py) runs on.  The plain-stack
engine's classifier tail (engine/plain.py) is the same chain and still carries loops of its own."""

import torch
from torch import nn

from .. import _lib
from .common import _P, _Launcher, _Unsupported, _same, mark_dead_prefix, records_of

MAX_ROWS, MAX_CLASSES = 256, 1024  # the dense kernels' row limit; the loss heads' class limit
_ACT = {None: 0, nn.ReLU: 1, nn.Tanh: 2}
GRADIENT, PRODUCT, DIAG_EF = range(3)  # what an adjoint sweep is for


class _Layer:
    """``Linear(+bias) [ReLU | Tanh]``: the module, its activation code, parameter indices and static buffers."""

    def __init__(self, lin, act):
        self.lin, self.act = lin, act
        self.c_out, self.c_in = lin.weight.shape
        self.dead = self.first_live = False
        self.g1 = self.h1 = None


class _Chain(_Launcher):
    """The layers of one chain and their launches, on the engine's device and its offsets into the flat vectors.  ``acts``:
    the activations accepted behind a ``Linear``; ``words``: a layer's and the chain's name in decline reasons, the row
    limit's message."""

    def __init__(self, dev, offs, acts, words):
        self.dev, self.offs, self.acts = dev, offs, acts
        self.name, self.whole, self.rows_msg = words
        self.layers, self.dead, self.zero = [], 0, None  # (zero: a slab of zeros, where a first layer may have no ``t_x``)

    def _at(self, vec, index):
        """The address of parameter ``index`` in the flat vector ``vec``; ``None`` without a vector or for a frozen one."""
        return None if vec is None or index is None else _P(vec.data_ptr() + 4 * self.offs[index])

    # ---- layout and static buffers -----------------------------------------------------------------
    def layout_layer(self, leaves, i, cur, param):
        """The ``Linear [activation]`` at ``leaves[i]``, which must read ``cur`` (``param``: the engine's ``_param``);
        returns the next index and the layer's output record."""
        m, name = leaves[i], f"{self.name} {len(self.layers)}"
        cx, cy = records_of(m, with_input=True)
        if cx.dim() != 2 or not _same(cx, cur):
            raise _Unsupported(f"{name}: its input is not the previous [batch, features] activation")
        nxt = leaves[i + 1] if i + 1 < len(leaves) else None
        act, y = None, cy
        if type(nxt) in self.acts:
            if getattr(nxt, "inplace", False):
                noun = self.acts[0].__name__ if len(self.acts) == 1 else "activation"
                raise _Unsupported(f"{name}: followed by an in-place {noun}")
            rx, ry = records_of(nxt, with_input=True)
            if not _same(rx, cy):
                raise _Unsupported(f"{type(nxt).__name__} does not read {name}'s output")
            act, y, i = type(nxt), ry, i + 1
        u = _Layer(m, _ACT[act])
        u.name, u.rx, u.ry = name, cx, y
        u.pw = param(m.weight)
        u.pb = param(m.bias) if m.bias is not None else None
        self.layers.append(u)
        return i + 1, y

    def check_end(self, out):
        """What the chain as a whole must be; returns its rows."""
        if not self.layers or self.layers[-1].act != 0:
            raise _Unsupported(f"the {self.whole} does not end in a Linear layer")
        last = self.layers[-1].ry
        if out.data_ptr() != last.data_ptr() or tuple(out.shape) != tuple(last.shape):
            raise _Unsupported("the network output is not the last Linear layer's output")
        if out.shape[0] > MAX_ROWS:
            raise _Unsupported(self.rows_msg.format(out.shape[0], MAX_ROWS))
        return int(out.shape[0])

    def mark_dead_prefix(self):
        """Frozen layers at the input end are dead for both sweeps; the first live one needs no data gradient."""
        self.dead = mark_dead_prefix(self.layers)
        self.layers[self.dead].first_live = True
        return self.dead

    def frozen_tensors(self):
        """The FROZEN weights and biases: kernel arguments of captured graphs, so part of a session's signature."""
        return [t for u in self.layers for t, k in ((u.lin.weight, u.pw), (u.lin.bias, u.pb)) if k is None and t is not None]

    def allocate(self, rows, x, t_x, hessian=False):
        """Per layer ``hf_dense_plan``'s split-K slab counts, output and tangent slabs; per LIVE layer tangent, cotangent
        and (unless ``first_live``) data-gradient slabs, on a Hessian engine ``g1`` / ``h1``.  The first layer reads ``x``
        (``t_x``: its tangent, or ``None``)."""
        f32, dev, lib = torch.float32, self.dev, _lib.load()
        self.rows, self.hessian = rows, hessian
        for u in self.layers:
            st, sd = _lib.c_int(), _lib.c_int()
            _lib.check(lib.hf_dense_plan(rows, u.c_in, u.c_out, st, sd), "hf_dense_plan")
            u.sT, u.sD, u.x, u.t_x = st.value, sd.value, x, t_x
            u.y = torch.empty((rows, u.c_out), dtype=f32, device=dev)
            u.tslabs = torch.empty((u.sT, rows * u.c_out), dtype=f32, device=dev)
            x = u.y
            if u.dead:
                continue
            u.ty, u.ga = torch.empty_like(u.y), torch.empty_like(u.y)
            u.dslabs = None if u.first_live else torch.empty((u.sD, rows * u.c_in), dtype=f32, device=dev)
            if hessian:  # first-order g_l = h_l * act'(a_l); h_l where the activation has a curvature
                u.g1 = torch.empty_like(u.y)
                u.h1 = torch.empty_like(u.y) if u.act == 2 else None
            t_x = u.ty
        return self.layers[-1].y

    def release(self):  # (the model's own activations were only needed up to the end of the construction)
        for u in self.layers:
            u.rx = u.ry = None

    # ---- launches ----------------------------------------------------------------------------
    def _slabs(self, u, t_x, v_w):
        """``u.tslabs <- t_x W^T + x V^T`` (either term may be absent, not both)."""
        self._launch("hf_dense_tangent_slabs", u.tslabs, t_x, u.x, u.lin.weight, v_w, self.rows, u.c_in, u.c_out, 0, u.sT,
                     u.tslabs.shape[1])

    def forward(self):
        """The tangent kernel with ``t_x = NULL, V = W`` is the forward GEMM; then slab sum, bias, activation in one pass."""
        for u in self.layers:
            self._slabs(u, None, u.lin.weight)
            self._launch("hf_dense_act_forward", u.y, u.tslabs, u.sT, u.tslabs.shape[1], u.lin.bias, u.act, self.rows,
                         u.c_out)

    def load_recorded(self):
        """The MODEL's recorded activations (the ReLU decisions of the autograd operator the first product is compared with)."""
        self.layers[0].x.copy_(self.layers[0].rx)
        for u in self.layers:
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
            self._launch("hf_dense_act_tangent", u.ty, slabs, splits, u.tslabs.shape[1], v_b, u.y, u.act, self.rows, u.c_out)
        return u.ty

    def adjoint(self, what, seed, out=None, weight=1.0, v=None, scale=None):
        """THE adjoint sweep: from the cotangent ``seed`` at the logits through the live layers in reverse, per layer the
        activation adjoint -> the weight output -> (``DIAG_EF``) the bias output -> the data gradient, as slabs the next
        activation adjoint sums; a ``first_live`` layer stops before its data gradient.  Weight / bias outputs: the
        parameters' places in the flat ``out`` (none without one), times ``weight``.
        ``GRADIENT`` keeps ``g_l`` (``h_l`` of tanh layers) where a Hessian engine has buffers for them; ``PRODUCT`` carries,
        on a Hessian engine, the second-order terms of ``v``; ``DIAG_EF`` writes sums of squares times ``scale`` (per-sample
        cotangents: ``weight`` does not enter, the bias has a kernel of its own).  Returns the last ``(slabs, splits, stride)``."""
        launch, rows = self._launch, self.rows
        diag, second = what == DIAG_EF, what == PRODUCT and self.hessian
        slabs, splits, stride = seed, 1, 0
        for u in reversed(self.layers[self.dead:]):
            o_w, o_b = self._at(out, u.pw), self._at(out, u.pb)
            g = u.g1 if what == GRADIENT and u.g1 is not None else u.ga
            if what == GRADIENT and u.h1 is not None:  # h_l itself: the slab sum, no factor
                launch("hf_dense_act_adjoint", u.h1, None, slabs, splits, stride, None, 0, rows, u.c_out, 1.0)
            if second and u.act == 2:  # tanh: the curvature term -2 a t_a h
                launch("hf_dense_act_adjoint2", g, o_b, slabs, splits, stride, u.y, u.act, u.ty, u.h1, rows, u.c_out, weight)
            else:
                launch("hf_dense_act_adjoint", g, None if diag else o_b, slabs, splits, stride, u.y, u.act, rows, u.c_out,
                       1.0 if diag else weight)
            if o_w is not None and diag:
                launch("hf_dense_sq_wgrad", o_w, g, u.x, rows, u.c_in, u.c_out, scale)
            elif o_w is not None and second and u.t_x is not None:  # + g^T t_x (none enters the first live layer)
                launch("hf_dense_wgrad2", o_w, g, u.x, u.g1, u.t_x, rows, u.c_in, u.c_out, weight)
            elif o_w is not None:
                launch("hf_dense_wgrad", o_w, g, u.x, rows, u.c_in, u.c_out, weight)
            if o_b is not None and diag:
                launch("hf_dense_sq_colsum", o_b, g, rows, u.c_out, scale)
            if u.first_live:
                break
            if second and u.pw is not None:  # + g V (a frozen weight has no tangent)
                launch("hf_dense_dgrad2_slabs", u.dslabs, g, u.lin.weight, u.g1, self._at(v, u.pw), rows, u.c_in, u.c_out,
                       u.sD, u.dslabs.shape[1])
            else:
                launch("hf_dense_dgrad_slabs", u.dslabs, g, u.lin.weight, rows, u.c_in, u.c_out, u.sD, u.dslabs.shape[1])
            slabs, splits, stride = u.dslabs, u.sD, u.dslabs.shape[1]
        return slabs, splits, stride
