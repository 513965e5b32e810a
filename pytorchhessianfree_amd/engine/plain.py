"""The plain conv-ReLU stack engine (All-CNN-C, BASELINE.json configs[3])."""

import torch
from torch import nn

from .. import _lib
from .common import _Unit, _Unsupported, _cl, _pair, _same, mark_dead_prefix, records_of
from .conv import _ConvEngine
from .dense import _Layer
from .problems import affine_train_args

MAX_TAIL_ROWS, MAX_CLASSES = 256, 1024  # the dense kernels' row limit; the loss head's class limit


class PlainStackEngine(_ConvEngine):
    """The same sweeps for a plain stack ``[inert Dropout] conv(+bias | +BatchNorm) [ReLU] ... -> AdaptiveAvgPool2d(1) ->
    flatten`` with a softmax cross-entropy on the pooled map -- the All-CNN-C of the reference's
    examples (examples/example_utils.py:59-83, BASELINE.json configs[3]).  Per layer: tangent
    convolution -> bias tangent + ReLU mask (into the next layer's operand) / masked slab sum + bias
    gradient -> data + weight gradient; the head (average pool, loss Hessian, broadcast) is ONE launch
    (``hf_pool_ce_head``).  4 launches per layer and product, bitwise repeatable.

    ``nn.MaxPool2d`` layers between the convolutions (ConvPool-CNN-C, Network-in-Network: ``conv [ReLU] MaxPool2d``,
    dilation 1, no ``ceil_mode``, any unit but the last -- the last one too in front of a classifier tail): ReLU masks and pool positions are piecewise constant, so the
    pooled unit's bias / ReLU / pool is ONE launch per direction -- ``hf_pool_act_tangent_nhwc`` gathers the tangent
    convolution's slabs at the windows' positions, masks by the POOLED map and writes into the consumer's operand (no
    full-resolution tangent map), ``hf_pool_act_adjoint_nhwc`` gathers the consumer's data-gradient slabs into the
    full-resolution ``ga`` with the bias sums.  The forward pass adds ``hf_maxpool_forward_nhwc`` (pooled map, its copy
    in the consumer's ``x`` half, positions).  Everything that reads ``u.ga`` / ``u.gb`` / ``u.x`` is unchanged.

    Eval-mode ``BatchNorm2d`` units (VGG-BN style nets): ``Conv2d(bias=False) BatchNorm2d [ReLU] [MaxPool2d]`` is one unit,
    anywhere a bias unit may stand.  Unpooled, it runs on the shared BatchNorm launches of the mixins; pooled, BatchNorm /
    ReLU / pool is ONE launch per direction as for a bias -- ``hf_pool_bn_act_tangent_nhwc`` adds the scale (w*rstd) and the
    ``xhat * v_w`` term at the windows' positions, ``hf_pool_bn_act_adjoint_nhwc`` writes the unscaled masked cotangent
    ``u.g`` (what the sums table, Hessian products and ``diag_ef`` read), ``u.ga = g * w*rstd`` and the scale's / shift's sums.

    Train-mode ``BatchNorm2d`` units (each BatchNorm's own ``bn.training``; eval and train units mix): batch statistics in
    the own forward pass (``hf_bn_stats_rows`` / ``hf_bn_forward_train``, running statistics moved per evaluation), in the
    tangent -- the per-channel sums over ALL full-resolution rows come from the tangent convolution's epilogue or one
    reduction launch (``_train_tangent_sums``); a pooled unit's gather ``hf_pool_bn_act_tangent_train_nhwc`` adds them up in
    its prologue and still forms no full-resolution tangent map -- and in the two-pass adjoint
    (``hf_pool_bn_act_adjoint_reduce_nhwc``: ``u.g`` and its sums; then ``hf_chan_affine_train``, or inside a Hessian product
    ``hf_bn_train_hessian_*``).  5-6 launches per such unit and product; one process; no active ``Dropout``.

    A classifier tail instead of the global average pool (LeNet, VGG-style nets, DeepOBS 2c2d / 3c3d): units as above
    (the last one may be pooled), ``nn.Flatten``, then ``Linear [ReLU] ... Linear``.  The tail is the kind's HEAD, with
    parameters of its own: the last unit writes into a ``[t_x | x]`` NHWC operand as for a conv consumer,
    ``hf_flatten_nhwc_rows`` turns a half of it into the rows the first ``Linear`` reads (features in ``(c, h, w)`` order:
    its weight is read in place), the layers run on the skinny GEMMs of hf_dense.hip (W and the vector's slice V in
    place; 2 launches per layer forward / tangent, 3 adjoint), ``hf_unflatten_slabs_nhwc`` sums the first layer's
    data-gradient slabs into the NHWC cotangent of the last map.  Weight / bias gradients go into buffers of the engine
    and enter the gather as ordinary entries.  GGN products, one process, batch <= 256."""

    mode = ("fused curvature engine (plain conv-ReLU stack): own deterministic convolutions (split-K slabs summed "
            "by the consumer kernel), bias / ReLU / max-pool fused, 4 launches per layer")
    # Hessian products (optimizer.py:450-455) by forward-over-reverse on the same kernels: the tangent
    # sweep, then the TANGENT OF THE BACKWARD SWEEP -- per layer, besides the GGN's conv_D(g', W) and
    # conv_W(x, g'), the two terms that carry the network's own curvature, conv_D(g, V) and conv_W(t_x, g)
    # (g: first-order cotangent of the step, g': its tangent; ReLU masks are piecewise constant), all four
    # in ONE grouped launch whose extra results are simply more split-K slabs for the consumers to sum.
    _extras_default = 1
    _fork_behind_head = True  # (the head is ONE launch: the side branch of a Hessian product forks behind it)

    def _layout(self, model):
        x_in = getattr(self.outputs, "_hf_input", None)
        if x_in is None or x_in.dim() != 4:
            raise _Unsupported("no recorded input")
        leaves = [m for m in model.modules() if not list(m.children())]
        self._dropouts = [m for m in leaves if isinstance(m, (nn.Dropout, nn.Dropout2d))]

        units, cur, prev, pooled, i = [], x_in.detach(), "input", None, 0
        dense = None  # the layers of a classifier tail, once nn.Flatten has been met
        while i < len(leaves):
            m = leaves[i]
            if isinstance(m, (nn.Dropout, nn.Dropout2d, nn.Identity)):
                if not isinstance(m, nn.Identity) and m.training and m.p > 0:
                    where = f"behind {units[-1].name}" if units else "in front of the first convolution"
                    raise _Unsupported(f"{type(m).__name__}(p={m.p}) {where} is active (train mode): a random mask the "
                                       "engine cannot replay")
                i += 1
                continue
            if pooled is not None:
                raise _Unsupported(f"{type(m).__name__} after the pooling layer")
            if dense is not None:
                i, cur = self._layout_tail_layer(leaves, i, dense, cur)
                continue
            if type(m) is nn.Conv2d:
                if m.groups != 1 or tuple(m.dilation) != (1, 1) or not getattr(m, "_hf_channels_last", False):
                    raise _Unsupported(f"conv {len(units)}: needs prepare_model(channels_last=True), groups = dilation = 1")
                cx, cy = records_of(m, with_input=True)
                if not _same(cx, cur):
                    raise _Unsupported(f"conv {len(units)}: input is not the previous activation")
                nxt = leaves[i + 1] if i + 1 < len(leaves) else None
                bn = nxt if type(nxt) is nn.BatchNorm2d else None
                u = _Unit(f"conv{len(units)}", m, bn)
                y, u.relu = cy, False
                if bn is not None:
                    y, u.relu = self._layout_bn(u, bn, cy)
                    i += 1
                    if u.relu:  # (modelprep fused the following ReLU module into the layer: its output is the unit's)
                        nxt = leaves[i + 1] if i + 1 < len(leaves) else None
                        if type(nxt) is not nn.ReLU or nxt.inplace or not _same(records_of(nxt, with_input=True)[1], y):
                            raise _Unsupported(f"{u.name}: the ReLU fused into its BatchNorm2d is not the next layer")
                        i += 1
                elif type(nxt) is nn.ReLU and not nxt.inplace:
                    rx, ry = records_of(nxt, with_input=True)
                    if _same(rx, cy):
                        y, u.relu = ry, True
                        i += 1
                u.kx, u.ky, u.rx, u.ry, u.ra = cx.data_ptr(), y.data_ptr(), cx, y, cy
                # (a BatchNorm unit keeps its masked cotangent, as the residual kind's units do: the sums table and
                # ``diag_ef`` take the scale's sums from it)
                u.a, u.y, u.needs_g = _cl(cy), _cl(y), bn is not None
                u.pw = self._param(m.weight)
                if bn is None:
                    u.pb = self._param(m.bias) if m.bias is not None else None
                    u.pg = None
                else:
                    u.pg, u.pb = self._param(bn.weight), self._param(bn.bias)
                u.src, prev, cur = prev, u, y
                units.append(u)
            elif type(m) is nn.MaxPool2d:
                # directly behind a unit (its ReLU, if it has one): the unit's bias / ReLU and the pool are one launch
                # per sweep direction (hf_pool_act_*_nhwc)
                where = f"MaxPool2d behind {units[-1].name}" if units else "MaxPool2d in front of the first convolution"
                if not units or units[-1].pool is not None:
                    raise _Unsupported(f"{where}: a pool must directly follow a convolution (and its ReLU)")
                if _pair(m.dilation) != [1, 1] or m.ceil_mode or m.return_indices:
                    raise _Unsupported(f"{where}: dilation / ceil_mode / return_indices are not covered")
                px, py = records_of(m, with_input=True)
                if not _same(px, cur):
                    raise _Unsupported(f"{where}: its recorded input is not the unit's output")
                u = units[-1]
                u.pool = tuple(_pair(m.kernel_size) + _pair(m.stride if m.stride is not None else m.kernel_size)
                               + _pair(m.padding))
                u.rp, cur = py, py
            elif isinstance(m, nn.AdaptiveAvgPool2d) and m.output_size in (1, (1, 1)):
                px, py = records_of(m, with_input=True)
                if not units or not _same(px, cur):
                    raise _Unsupported("the pooling layer does not follow the last convolution")
                if units[-1].pool is not None:
                    raise _Unsupported(f"MaxPool2d behind {units[-1].name}: a pool between the last convolution and the "
                                       "global average pool is not covered")
                pooled = py
            elif type(m) is nn.Flatten and units:
                fx, fy = records_of(m, with_input=True)
                if not _same(fx, cur) or fy.dim() != 2 or fy.shape[1] != cur.shape[1] * cur.shape[2] * cur.shape[3]:
                    raise _Unsupported("Flatten does not turn the last unit's output into [batch, c*h*w]")
                dense, cur, self._rec_flat = [], fy, fy
            elif type(m) is nn.BatchNorm2d:
                where = (f"behind {units[-1].name}" + ("'s MaxPool2d" if units[-1].pool is not None else "'s activation")
                         if units else "in front of the first convolution")
                raise _Unsupported(f"BatchNorm2d {where}: a BatchNorm must directly follow a convolution")
            elif type(m) is nn.ReLU and units and units[-1].pool is not None:
                raise _Unsupported(f"ReLU behind the MaxPool2d of {units[-1].name}: the activation must stand in front of "
                                   "the pool")
            else:
                raise _Unsupported(f"unsupported layer {type(m).__name__}")
            i += 1
        out = self.outputs.detach()
        if dense is not None:
            self._layout_tail(units, dense, out)
        elif pooled is None or not units:
            raise _Unsupported("not a conv stack that ends in global average pooling or a classifier tail")
        elif out.data_ptr() != pooled.data_ptr() or tuple(out.shape) != (pooled.shape[0], pooled.shape[1]):
            raise _Unsupported("the network output is not the flattened pooled map")
        self.classifier = dense or []
        first = units[0]
        first.first = True
        first.im2col = first.a.shape[1] > 0 and first.rx.shape[1] < 4
        self.units, self.tail = units, units[-1]
        self.train_bn = any(u.train for u in units)
        self.model_ref, self._in_shape = model, tuple(x_in.shape)
        used = {i for u in units + self.classifier for i in (u.pw, getattr(u, "pg", None), u.pb) if i is not None}
        if used != set(range(len(self.params))):
            raise _Unsupported("the parameter list has entries the engine's layers do not cover")
        # frozen layers at the input end (round 6, as FusedGGNEngine._mark_dead_prefix): dead for both sweeps; the first
        # layer with a trainable parameter reads a tangent-free input and needs no data gradient
        self.dead_units = mark_dead_prefix(units)
        if self.dead_units:
            units[self.dead_units].no_dgrad = True

    def _layout_bn(self, u, bn, cy):
        """The BatchNorm behind ``u``'s convolution (output record ``cy``): what the unit's output record and ReLU flag
        are.  Eval mode: ``modelprep`` fuses a following ``nn.ReLU`` into the layer and leaves one 5-entry record.  Train
        mode (the layer's own ``bn.training``, as ``topology.make_unit``): the layer ran on stock ops and left a 6-entry
        record with its batch statistics, which a following ``nn.ReLU`` completed; the unit gets clones of them that the
        own forward pass rewrites."""
        if u.conv.bias is not None:
            raise _Unsupported(f"{u.name}: a convolution bias in front of a BatchNorm2d is not covered (bias=False)")
        rec = getattr(bn, "_hf_io", None)
        if bn.training:
            if self.group is not None:
                raise _Unsupported(f"{u.name}: train-mode BatchNorm under data parallelism: batch statistics couple the "
                                   "samples of a shard")
            if rec is None or len(rec) != 6:
                raise _Unsupported(f"{u.name}: train-mode BatchNorm without a record of this forward pass (it must be "
                                   "affine, float32, on the GPU)")
            bx, bres, by, brelu, rstd, mean_t = rec
            u.rec_stats = (mean_t, rstd)
            u.rstd, u.mean_t, u.train = rstd.clone(), mean_t.clone(), True
        else:
            if rec is None or len(rec) != 5:
                raise _Unsupported(f"{u.name}: its BatchNorm2d has no fused eval record of this forward pass (it must be "
                                   "affine, with running statistics)")
            bx, bres, by, brelu, _rstd = rec
        if bres is not None or not _same(bx, cy):
            raise _Unsupported(f"{u.name}: the BatchNorm2d does not consume the convolution's output")
        return by, bool(brelu)

    # ---- classifier tail: layout -----------------------------------------------------------------
    def _layout_tail_layer(self, leaves, i, dense, cur):
        """One ``Linear [ReLU]`` of the tail at ``leaves[i]``; returns the next index and the layer's output record."""
        m = leaves[i]
        if type(m) is not nn.Linear:
            raise _Unsupported(f"unsupported layer {type(m).__name__} in the classifier tail (Linear [ReLU] ... Linear)")
        name = f"tail linear {len(dense)}"
        cx, cy = records_of(m, with_input=True)
        if cx.dim() != 2 or not _same(cx, cur):
            raise _Unsupported(f"{name}: its input is not the previous [batch, features] activation")
        nxt = leaves[i + 1] if i + 1 < len(leaves) else None
        act, y = 0, cy
        if type(nxt) is nn.ReLU:
            if nxt.inplace:
                raise _Unsupported(f"{name}: followed by an in-place ReLU")
            rx, ry = records_of(nxt, with_input=True)
            if not _same(rx, cy):
                raise _Unsupported(f"ReLU does not read {name}'s output")
            act, y, i = 1, ry, i + 1
        u = _Layer(m, act)
        u.name, u.rx, u.ry = name, cx, y
        u.pw = self._param(m.weight)
        u.pb = self._param(m.bias) if m.bias is not None else None
        dense.append(u)
        return i + 1, y

    def _layout_tail(self, units, dense, out):
        """What the tail as a whole must be, and what the engine does not cover behind one."""
        if not dense or dense[-1].act != 0:
            raise _Unsupported("the classifier tail does not end in a Linear layer")
        if out.data_ptr() != dense[-1].ry.data_ptr() or tuple(out.shape) != tuple(dense[-1].ry.shape):
            raise _Unsupported("the network output is not the last Linear layer's output")
        if out.shape[0] > MAX_TAIL_ROWS:
            raise _Unsupported(f"Linear tail: batch {out.shape[0]} > {MAX_TAIL_ROWS} rows (the dense kernels' limit)")
        if out.shape[1] > MAX_CLASSES:
            raise _Unsupported(f"Linear tail: more than {MAX_CLASSES} classes")
        c = units[-1].a.shape[1]
        if c % 4:  # (an im2col'd unit's channel count is checked nowhere else; hf_flatten_nhwc_rows would refuse it)
            raise _Unsupported(f"Linear tail: the last map has {c} channels (the flatten kernels take multiples of 4)")
        if self.hessian:
            raise _Unsupported("Hessian products through a classifier tail are not covered")
        if self.group is not None:
            raise _Unsupported("data parallelism is not covered for a classifier tail")
        if all(u.pw is None and u.pg is None and u.pb is None for u in units):
            raise _Unsupported("every convolution in front of the classifier tail is frozen: not covered")

    def _head_operands(self):
        last = self.units[-1]
        return (last.yp if last.pool is not None else last.y,) if self.classifier else ()

    def _allocate_tail(self):
        """Static buffers of the tail: the flattened operand halves, per layer output / tangent / cotangent, split-K
        slabs as ``hf_dense_plan`` counts them, and the weight / bias gradients the gather reads."""
        f32, dev, lib = torch.float32, self.dev, _lib.load()
        last = self.units[-1]
        fmap = last.yp if last.pool is not None else last.y
        rows, c, h, w = fmap.shape
        self._tail_op = self._xcats[id(fmap)]  # [t_x | x], NHWC: pixel pitch 2c
        self._tail_dims = (rows, h * w, c)
        self._flat_x = torch.empty((rows, c * h * w), dtype=f32, device=dev)
        self._flat_t = torch.empty_like(self._flat_x)
        self._g_last = torch.empty_like(fmap)  # (NHWC: the cotangent of the last map)
        x, t_x = self._flat_x, self._flat_t
        for u in self.classifier:
            st, sd = _lib.c_int(), _lib.c_int()
            _lib.check(lib.hf_dense_plan(rows, u.c_in, u.c_out, st, sd), "hf_dense_plan")
            u.sT, u.sD, u.x, u.t_x = st.value, sd.value, x, t_x
            u.y = torch.empty((rows, u.c_out), dtype=f32, device=dev)
            u.ty, u.ga = torch.empty_like(u.y), torch.empty_like(u.y)
            u.tslabs = torch.empty((u.sT, rows * u.c_out), dtype=f32, device=dev)
            u.dslabs = torch.empty((u.sD, rows * u.c_in), dtype=f32, device=dev)
            u.gw = torch.zeros((u.c_out, u.c_in), dtype=f32, device=dev)
            u.gb = torch.zeros(u.c_out, dtype=f32, device=dev)
            x, t_x = u.y, u.ty
        self.logits = self.classifier[-1].y
        self._g_logits = torch.empty_like(self.logits)
        self._p = torch.empty_like(self.logits)
        self.loss_buf = torch.zeros((), dtype=f32, device=dev)
        self._sig_tail = [t for u in self.classifier for t, k in ((u.lin.weight, u.pw), (u.lin.bias, u.pb))
                          if k is None and t is not None]

    def _allocate_head(self):
        if self.classifier:
            self._allocate_tail()
            return
        f32, dev = torch.float32, self.dev
        n, k, h, w = self.tail.y.shape
        self._head_hw = h * w
        self.logits = torch.empty((n, k), dtype=f32, device=dev)
        self._p = torch.empty_like(self.logits)
        self.loss_buf = torch.zeros((), dtype=f32, device=dev)
        self._g_last = torch.empty_like(self.tail.y)
        if k > 1024:
            raise _Unsupported("more than 1024 classes")

    # ---- forward -----------------------------------------------------------------------------
    def _forward_units(self, refresh, update_running):
        first, flat = self.units[0], self._flat_params
        carried = (refresh and flat is not None and flat.data_ptr() == self.params[0].data_ptr()
                   and self._conv_carrying_scatter(first, first.conv.weight.detach(), first.sF, flat, 0))
        if refresh and not carried:
            self.refresh_weights()
        for u in self.units:
            if not (carried and u is first):
                self._conv_forward(u)
            self._bn_forward(u, u.sF, update_running)  # (train mode: batch statistics; moves the running ones)
            if u.pool is not None:
                # the pooled map, its copy in the x half of the consumer's [t_x | x] operand, the positions
                c = u.y.shape[1]
                self._launch("hf_maxpool_forward_nhwc", u.yp, u.pool_out2, 2 * c, u.pidx, u.y, *self._pool_dims(u), *u.pool)
        if not self.classifier:
            torch.mean(self.tail.y, dim=(2, 3), out=self.logits)
            return
        self._flatten(self._flat_x, 1)
        for u in self.classifier:
            self._dense_slabs(u, None, u.lin.weight)  # (t_x = NULL, V = W: the forward GEMM)
            self._launch("hf_dense_act_forward", u.y, u.tslabs, u.sT, u.tslabs.shape[1], u.lin.bias, u.act, u.y.shape[0],
                         u.c_out)

    def _load_recorded(self, outputs):
        if self.classifier:  # (already in row order: copies)
            self._flat_x.copy_(self._rec_flat)
            for u in self.classifier:
                u.y.copy_(u.ry)
        super()._load_recorded(outputs)
        for u in self.units:
            if u.pool is not None:  # the model's pooled map, and the positions of ITS windows (as the stem's, forward.py)
                kh, kw, sh, sw, ph, pw = u.pool
                _, idx = torch.nn.functional.max_pool2d(u.ry, (kh, kw), (sh, sw), (ph, pw), return_indices=True)
                # (ATen: flat y*w + x inside the (n, c) plane -- what hf_maxpool_forward_nhwc writes)
                u.pidx.copy_(idx.permute(0, 2, 3, 1))
                u.yp.copy_(u.rp)
                u.pool_out2.copy_(u.rp)

    # ---- pooled units: bias / ReLU / max-pool in one launch per direction ---------------------------
    @staticmethod
    def _pool_dims(u):
        """(n, h, w, oh, ow, c) of a pooled unit."""
        n, c, h, w = u.y.shape
        return n, h, w, u.yp.shape[2], u.yp.shape[3], c

    def _pool_tangent(self, u, v):
        """t_pool = (y_pool > 0) * (t_a[idx] + v_b) from the tangent convolution's slabs into the consumer's operand; with
        a BatchNorm  (y_pool > 0) * (t_a[idx] * w*rstd + xhat[idx] * v_w + v_b)."""
        tail = (u.pidx, u.yp, 1 if u.relu else 0, *self._pool_dims(u))
        if u.train:
            # batch statistics: the sums over ALL full-resolution rows (partial rows by the convolution's epilogue or one
            # reduction over the slabs), then the gather with the finalisation in its prologue
            vg, vb = self._scale_shift_tangent(u, v)
            part_x, part_1, nparts = self._train_tangent_sums(u)
            n, h, w = tail[3:6]
            self._launch("hf_pool_bn_act_tangent_train_nhwc", u.tout, u.tout_ld, u.tbuf, u.sT, u.tbuf.shape[1], u.a, u.mean,
                         u.rstd, u.scale, vg, vb, part_x, part_1, nparts, float(n * h * w), *tail)
            return
        if u.bn is not None:
            vg, vb = self._scale_shift_tangent(u, v)
            self._launch("hf_pool_bn_act_tangent_nhwc", u.tout, u.tout_ld, u.tbuf, u.sT, u.tbuf.shape[1], u.a, u.mean,
                         u.rstd, u.scale, vg, vb, *tail)
            return
        vb = self._param_slice(v, u.pb, u.cout)
        self._launch("hf_pool_act_tangent_nhwc", u.tout, u.tout_ld, u.tbuf, u.sT, u.tbuf.shape[1], vb, *tail)

    def _pool_adjoint(self, u, srcs):
        """g_a at full resolution from the consumer's data-gradient slabs; the bias sums as partial rows -- or, where
        the unit's sums are deferred, left to the sums table (which reads ``u.ga``).  With a BatchNorm: the unscaled
        masked cotangent -> ``u.g`` (where the unit keeps one: the sums table, Hessian products and ``diag_ef`` read it),
        ``u.ga`` = it times w*rstd, and the scale's and shift's sums."""
        self._extras_wait(srcs)
        (gy, splits, slab), = srcs
        gb = None if (u.defer or u.pb is None) else u.gb
        tail = (u.pidx, u.yp, 1 if u.relu else 0, *self._pool_dims(u), *u.pool)
        if u.train:
            # pass 1: the masked cotangent at full resolution and its sums; pass 2 (a grid-wide sum stands between them):
            # g_a by the elementwise train kernel -- inside a Hessian product ``hf_bn_train_hessian_apply``'s instead
            self._launch("hf_pool_bn_act_adjoint_reduce_nhwc", u.g, u.gw, u.gb, u.rb, gy, splits, slab, u.a, u.mean, u.rstd,
                         u.scale, *tail)
            if not self._second:
                self._launch("hf_chan_affine_train", *affine_train_args(self._train_adjoint_problem(u)))
        elif u.bn is not None:
            gw = None if (u.defer or u.pg is None) else u.gw
            self._launch("hf_pool_bn_act_adjoint_nhwc", u.ga, u.g, gw, gb, u.rb, gy, splits, slab, u.a, u.mean, u.rstd,
                         u.scale, *tail)
        else:
            self._launch("hf_pool_act_adjoint_nhwc", u.ga, gb, u.rb, gy, splits, slab, *tail)
        if u.defer:
            self._sums_pending.add(u.sums_slot)

    # ---- product ------------------------------------------------------------------------------
    def _tangent_sweep(self, v):
        first = self.units[0]
        carried = False
        if first.im2col and not first.dead:  # (the first layer's launch carries the v_W scatter of all the others)
            carried = self._conv_carrying_scatter(first, self._weight_tangent(v, first), first.sT, v, 1)
        if self._slot_list and not carried:
            _lib.unpack_tangent(v, self._slot_list)  # v_W halves of all [W | v_W] operands: one launch
        for u in self.units:
            if u.dead:  # (frozen, behind frozen layers only: no tangent)
                continue
            if u.im2col:  # no input tangent: conv(x, v_W) as a 1x1 product over the im2col
                if not (carried and u is first):
                    self._conv_slabs(0, u.tbuf, u.cols, self._weight_tangent(v, u), u.geo, u.sT)
            elif u.train:  # (the epilogue writes the tangent's per-channel partial sums where it takes the geometry)
                self._tangent_convs([u])
            else:
                self._conv_slabs(0, u.tbuf, u.xcat, u.wcat, u.geo.doubled(), u.sT)
            if u.pool is not None:
                self._pool_tangent(u, v)
            else:
                self._bn_tangent(u, v, None, 0)
        if self.classifier:
            self._tail_tangent(v)

    # ---- classifier tail: launches ------------------------------------------------------------------
    def _flatten(self, out, half):
        """``out`` [rows, c*hw] <- half ``half`` (0: t_x, 1: x) of the last map's NHWC operand, features in (c, h, w) order."""
        rows, hw, c = self._tail_dims
        self._launch("hf_flatten_nhwc_rows", out, c * hw, self._tail_op[:, half * c:], 2 * c, rows, hw, c)

    def _dense_slabs(self, u, t_x, v_w):
        """``u.tslabs <- t_x W^T + x V^T`` (either term may be absent, not both)."""
        self._launch("hf_dense_tangent_slabs", u.tslabs, t_x, u.x, u.lin.weight, v_w, u.y.shape[0], u.c_in, u.c_out, 0,
                     u.sT, u.tslabs.shape[1])

    def _tail_tangent(self, v):
        """The last unit's tangent (in the operand's t_x half) through the tail; V and the bias tangents are slices of
        ``v`` in place (a frozen weight: V = NULL)."""
        self._flatten(self._flat_t, 0)
        for u in self.classifier:
            self._dense_slabs(u, u.t_x, self._param_slice(v, u.pw, u.c_out * u.c_in))
            self._launch("hf_dense_act_tangent", u.ty, u.tslabs, u.sT, u.tslabs.shape[1], self._param_slice(v, u.pb, u.c_out),
                         u.y, u.act, u.y.shape[0], u.c_out)

    def _tail_adjoint(self):
        """From ``self._g_logits`` back through the tail: per layer ``act'`` and the bias sums, the weight gradient, the
        data-gradient slabs; the first layer's slabs are summed into the NHWC cotangent of the last map."""
        slabs, splits, stride = self._g_logits, 1, 0
        for u in reversed(self.classifier):
            rows = u.y.shape[0]
            self._launch("hf_dense_act_adjoint", u.ga, u.gb if u.pb is not None else None, slabs, splits, stride, u.y, u.act,
                         rows, u.c_out, 1.0)
            if u.pw is not None:
                self._launch("hf_dense_wgrad", u.gw, u.ga, u.x, rows, u.c_in, u.c_out, 1.0)
            self._launch("hf_dense_dgrad_slabs", u.dslabs, u.ga, u.lin.weight, rows, u.c_in, u.c_out, u.sD, u.dslabs.shape[1])
            slabs, splits, stride = u.dslabs, u.sD, u.dslabs.shape[1]
        rows, hw, c = self._tail_dims
        self._launch("hf_unflatten_slabs_nhwc", self._g_last, slabs, splits, stride, rows, hw, c)
        return self._g_last, self.classifier, None

    def _head_entries(self, tensors, splits, layers, _g_fb):
        """The tail's weight / bias gradients as entries of ``hf_pack_ex``'s tables (copies of them): dense runs."""
        tensors = list(tensors)
        for u in layers:
            if u.pw is not None:
                tensors[u.pw] = u.gw
            if u.pb is not None:
                tensors[u.pb] = u.gb
        return tensors, splits

    def _diag_head_buffers(self, tensors):
        """(the tail's entries are written straight into ``out`` afterwards: the gathers add / write zeros there)"""
        for u in self.classifier:
            for pi, k in ((u.pw, u.c_out * u.c_in), (u.pb, u.c_out)):
                if pi is not None:
                    tensors[pi] = self._zeros(k)

    def _diag_head(self, out, scale):
        """The per-sample weight gradient of a ``Linear`` is the outer product ``g_a[r] (x) x[r]``: sums of squares by
        ``hf_dense_sq_wgrad`` / ``hf_dense_sq_colsum`` on the gradient sweep's cotangents.  Those carry the loss's 1/N;
        the conv entries undo it BEFORE squaring, the dense kernels scale AFTER: ``scale`` squared."""
        for u in self.classifier:
            rows = u.y.shape[0]
            if u.pw is not None:
                self._launch("hf_dense_sq_wgrad", out[self._offs[u.pw]:], u.ga, u.x, rows, u.c_in, u.c_out, scale * scale)
            if u.pb is not None:
                self._launch("hf_dense_sq_colsum", out[self._offs[u.pb]:], u.ga, rows, u.c_out, scale * scale)

    def layer_signature(self):
        """Besides the units': the tail's module identities and the addresses of its FROZEN tensors (kernel arguments of
        the captured graphs; the trainable ones are covered by the flat vector's address)."""
        sig = super().layer_signature()
        if self._dropouts:  # (skipped as inert: one that becomes active is another network)
            sig = sig + (tuple(bool(m.training and m.p > 0) for m in self._dropouts),)
        if not self.classifier:
            return sig
        return sig + (tuple((id(u.lin), u.act) for u in self.classifier), tuple(t.data_ptr() for t in self._sig_tail))

    def _release(self, model):
        for u in self.classifier:  # the model's own activations were only needed up to here
            u.rx = u.ry = None
        self._rec_flat = None
        super()._release(model)

    def _head(self, v):
        """Average pool, loss Hessian and broadcast back over the last map in ONE launch; no parameters of its own."""
        n, k = self.logits.shape
        if self.classifier:
            self._launch("hf_softmax_ce_hvp", self._g_logits, self._ce[0], self.classifier[-1].ty, float(self._ce[1]), n, k)
            return self._tail_adjoint()
        self._launch("hf_pool_ce_head", self._g_last, None, self.tail.tout, self._ce[0], float(self._ce[1]), n,
                     self._head_hw, k)
        return self._g_last, None, None

    def _first_order_seed(self):
        if self.classifier:  # d loss / d logits, then the same tail adjoint
            torch.sub(self._p, self._onehot, out=self._g_logits)
            self._g_logits.mul_(float(self._ce[1]))
            return self._tail_adjoint()
        n, k, h, w = self.tail.y.shape
        g = (self._p - self._onehot) * (self._ce[1] / self._head_hw)  # d loss / d (last map), per pixel
        self._g_last.permute(0, 2, 3, 1).copy_(g.view(n, 1, 1, k).expand(n, h, w, k))
        return self._g_last, None, None

    def _adjoint_sweep(self, g_last):
        srcs = [(g_last, 1, 0)]
        for u in self._adjoint_order():
            if u.dead:  # (nobody needs a cotangent behind the first trainable layer)
                break
            self._adjoint_unit(u, srcs)
            if u.sD:
                srcs = [(u.dbuf, self._dslabs(u), u.dbuf.shape[1])]

    def _adjoint_order(self):
        return list(reversed(self.units))

    def _loss_setup(self, loss, outputs):
        super()._loss_setup(loss, outputs)
        if self.loss_spec is None or self.loss_spec["kind"] != "ce":
            raise _Unsupported("the plain-stack engine needs a plain softmax cross-entropy loss")
