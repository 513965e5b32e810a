"""Every buffer the sweeps touch -- owned by the engine and STATIC -- and the launches that fill them per batch /
per parameter point: split-K slab buffers, [t_x | x] / [W | v_W] operands, (I,H,W,O) weight copies, targets.

Mixin of ``_ConvEngine`` (engine/conv.py); see that class for the sweeps' overall structure."""

import os

import torch

from .. import _lib
from .common import _Unsupported, _flat_view, _live_taps
from .problems import Geometry, bn_adjoint_args, chan_sums_problem, conv_args, conv_problem


def adjoint_split_ok(train, rb, hessian, map_bytes, max_bytes, enabled=True):
    """Whether a unit's BatchNorm / bias adjoint runs as the ELEMENTWISE launch (``hf_bn_adjoint_v4``): eval mode, on the
    row-major kernel today (``rb > 1``), not inside a Hessian engine (whose ``_swap_first_order`` swaps the buffers a
    static sums table would point to), and a map small enough that reading ``g`` and ``x`` a second time costs less than
    the reduction costs the adjoint chain."""
    return bool(enabled and not train and rb > 1 and not hessian and map_bytes <= max_bytes)


def defer_sums_ok(train, rb, hessian, has_gw, has_gb, map_bytes, max_bytes, enabled=True):
    """Whether a unit's per-channel sums leave the adjoint chain for ``_flush_sums``: it takes the elementwise launch and
    has at least one of gw / gb to produce (a frozen scale and shift have no sums at all)."""
    return bool(adjoint_split_ok(train, rb, hessian, map_bytes, max_bytes, enabled) and (has_gw or has_gb))


def sums_runs(pending, cap):
    """The pending table entries as contiguous sub-ranges ``(first, count)`` of at most ``cap`` entries, ascending."""
    runs = []
    for i in sorted(set(pending)):
        if runs and runs[-1][0] + runs[-1][1] == i and runs[-1][1] < cap:
            runs[-1][1] += 1
        else:
            runs.append([i, 1])
    return [tuple(r) for r in runs]


def sums_table(problems):
    """``(table, total row blocks)``: the ``hf_bn_sums_problem`` array of ``problems`` -- dicts of its fields -- validated
    and completed (rows per block, block prefix) by the library's own host function; ``_lib.Refused`` on a problem the
    sums kernel does not take."""
    tab = (_lib.BnSumsProblem * len(problems))()
    for q, prob in zip(tab, problems):
        for name, val in prob.items():
            setattr(q, name, val)
    blocks = _lib.load().hf_bn_sums_table(_lib.ctypes.cast(tab, _lib.c_void_p), len(problems))
    if blocks < 0:
        _lib.check(int(blocks), "hf_bn_sums_table")
    return tab, int(blocks)


class _Buffers:
    ADJ_BYTES_PER_WG = 32768  # the BatchNorm adjoint's row-major kernel: one workgroup per this many bytes of the map
    # Up to this map size an eval-mode unit's per-channel sums leave the adjoint chain (adjoint_split_ok): the chain runs
    # the elementwise launch, ONE launch in front of the gather takes all units' sums from the stored g.  Above it the
    # fused launch stays: the split form reads g and x a second time.  Four times the largest ResNet-18 map (the stem's,
    # 1.6 MB): measured on the workloads with larger maps, deferral off / 1.6 MB / 6.4 MB -- All-CNN-C 835 / 841 / 844,
    # ResNet-50 topology 341 / 347 / 357 matvecs/s (profiles/r20_bn_defer_threshold.jsonl); ResNet-18 is the same at both.
    DEFER_MAX_BYTES = 4 * 6272 * 64 * 4
    # ---- buffers -------------------------------------------------------------------------
    def _plan(self, direction, geo, name=None):
        """The K-splits a slab-mode launch of this geometry uses; ``name``: the unit's (none: the im2col'd stem)."""
        sp = _lib.load().hf_conv2d_nhwc_plan(direction, *geo.dims(), 0)
        if sp < 1:
            raise _Unsupported(f"{name}: convolution geometry refused ({sp})" if name else f"stem geometry refused ({sp})")
        return sp

    def _allocate(self):
        """Every buffer the sweeps touch is owned by the engine and STATIC: the activations are
        recomputed in place by ``forward_own`` (own kernels), so one engine -- and the hipGraphs
        captured over it -- can serve every Newton step and every trial point of a step."""
        dev, f32 = self.dev, torch.float32
        cl = torch.channels_last

        def nhwc(shape):
            return torch.empty(shape, dtype=f32, device=dev).contiguous(memory_format=cl)

        self._nhwc = nhwc
        self.x_in = nhwc(self._in_shape)
        for u in self.units:
            u.a, u.y = nhwc(u.a.shape), nhwc(u.y.shape)
            if u.pool is not None:  # (plain stack) the pooled map -- what the consumer reads -- and the windows' positions
                u.yp = nhwc(u.rp.shape)
                u.pidx = torch.empty(tuple(u.yp.permute(0, 2, 3, 1).shape), dtype=torch.int32, device=dev)
            if u.train:
                u.rstd_version = None  # (u.rstd: batch statistics -- recorded by the model's pass or the own one's)
            elif u.bn is not None:
                u.rstd = torch.rsqrt(u.bn.running_var + u.bn.eps)
                u.rstd_version = u.bn.running_var._version
        for u in self.units:  # the convolution's input IS its producer's output buffer
            u.x = (self.x_in if u.src == "input" else u.src if isinstance(u.src, torch.Tensor)
                   else u.src.yp if u.src.pool is not None else u.src.y)
        for u in self.units:
            if u.res_unit is not None:
                u.res = u.res_unit.y
            elif u.res_identity is not None:
                u.res = u.res_identity.x  # the block input
            else:
                u.res = None
        xcats = {}
        self._tangent_slots = {}
        for u in self.units:
            n, c, h, w = u.x.shape
            k, _, r, s = u.conv.weight.shape
            if u.im2col:
                if c * r * s > 256:
                    raise _Unsupported(f"{u.name}: too many taps for the im2col formulation")
                oh, ow = u.a.shape[2], u.a.shape[3]
                j = c * r * s
                u.cols = torch.empty((n, oh * ow, j), dtype=f32, device=dev)  # [N, OH*OW, c*r*s]
                u.geo = Geometry(n * oh * ow, 1, 1, j, k, 1, 1, (1, 1), (0, 0))
                # the weight gradient reads the im2col with rows padded to 16-byte multiples (zero
                # channels): 16-byte gathers instead of element-wise ones (28 -> 11 us for the 49-tap stem)
                jp = -(-j // 4) * 4
                u.cols_pad = torch.zeros((n, oh * ow, jp), dtype=f32, device=dev)
                u.geo_w = u.geo._replace(c=jp)
                u.jcols = j
                if not u.conv.weight.is_contiguous():
                    raise _Unsupported(f"{u.name}: weight layout")
            else:
                if c % 4 or k % 4:
                    raise _Unsupported(f"{u.name}: channel counts must be multiples of 4")
                u.geo = Geometry(n, h, w, c, k, r, s, tuple(u.conv.stride), tuple(u.conv.padding))
                key = id(u.x)
                if key not in xcats:
                    xcats[key] = torch.zeros((n, 2 * c, h, w), dtype=f32, device=dev).contiguous(memory_format=cl)
                u.xcat = xcats[key]
                # [W | v_W]; slices of taps that never meet data stay 0
                u.wcat = torch.zeros((k, 2 * c, r, s), dtype=f32, device=dev).contiguous(memory_format=cl)
                u.wT = torch.empty((c, r, s, k), dtype=f32, device=dev)  # (I, H, W, O)
                u.live = _live_taps(h, w, r, s, u.conv.stride, u.conv.padding)
                if u.pw is not None:  # (a frozen weight: its W half is copied from the parameter, its v_W half stays 0)
                    self._tangent_slots[id(u)] = (self._offs[u.pw], u.wcat, c, u.live)
            oh, ow = u.a.shape[2], u.a.shape[3]
            u.rows, u.cout = n * oh * ow, k
            # split-K slab buffers
            if u.im2col:
                u.sT = u.sF = self._plan(0, u.geo)
                u.sW = self._plan(2, u.geo_w)
                u.sD = 0
            else:
                u.sT, u.sW = self._plan(0, u.geo.doubled(), u.name), self._plan(2, u.geo, u.name)
                u.sD = 0 if (u.first or u.no_dgrad or u.dead) else self._plan(1, u.geo, u.name)
                u.sF = self._plan(0, u.geo, u.name)
            u.tbuf = torch.empty((max(u.sT, u.sF), u.rows * k), dtype=f32, device=dev)
            # Hessian products add, per layer, conv_W(t_x, g) to the weight gradient and conv_D(g, V) to the
            # data gradient (g: the step's first-order cotangent): as MORE SLABS of the same buffers, which
            # the consumers sum anyway
            u.nW = u.sW * (2 if (self.hessian and not u.first) else 1)
            u.nD = u.sD * (2 if self.hessian else 1)
            u.wbuf = torch.zeros((u.nW, u.conv.weight.numel()), dtype=f32, device=dev)  # dead taps stay 0
            if u.sD:
                u.dbuf = torch.empty((u.nD, u.x.numel()), dtype=f32, device=dev)
            if self.hessian:
                u.ga1 = torch.empty_like(u.a)  # first-order cotangent of the convolution output (per step)
                if u.bn is not None:
                    u.g1 = torch.empty_like(u.a)   # ... and of the BatchNorm output (masked), per step
                    u.gah = torch.empty_like(u.a)  # g_a' + g_z * rstd * v_gamma: what the convolutions' adjoints read
                if u.sD:
                    # V as (I, H, W, O), per product (a frozen weight has V = 0: zeros, never scattered into)
                    u.vT = torch.zeros((c, r, s, k), dtype=f32, device=dev)
            u.g = torch.empty_like(u.a) if u.needs_g else None  # masked cotangent of the unit's output
            u.ga = torch.empty_like(u.a)   # cotangent of the convolution output
            # the BatchNorm adjoint shares the rows among `rb` workgroups per channel column; the
            # per-channel sums arrive as rb partial rows that hf_pack_ex adds up
            u.rb = 1
            if k % 4 == 0 and k // 4 <= 256 and u.rows >= 64:
                # row-major adjoint kernel: ~64 workgroups, each reading whole contiguous rows, one
                # pass of the row loop where the map is small enough (measured on the ResNet-18
                # bench: 32 workgroups x 2 passes 1124, 64 x 1 1150, 128 x 1 the same, 256 x 1 1138)
                rp = 256 // (k // 4)
                # (64 workgroups suit the <= 1.6 MB maps of ResNet-18; a 12.6 MB map of All-CNN-C needs the
                # whole chip: one workgroup per 32 KB of the map, 64 ... 1024)
                tgt = min(1024, max(64, u.a.numel() * 4 // self.ADJ_BYTES_PER_WG))
                per = max(rp, -(-u.rows // tgt))
                u.rb = -(-u.rows // per)
                if u.rb < 2:
                    u.rb = 1
            enabled = os.environ.get("HF_BN_SUMS_DEFER", "1") != "0"
            u.split = adjoint_split_ok(u.train, u.rb, self.hessian, u.a.numel() * 4, self.DEFER_MAX_BYTES, enabled)
            u.defer = not u.dead and defer_sums_ok(u.train, u.rb, self.hessian, u.bn is not None and u.pg is not None,
                                                   u.pb is not None, u.a.numel() * 4, self.DEFER_MAX_BYTES, enabled)
            # (deferred sums are taken of the STORED g, needed by a residual branch or not; a pooled unit's is its ga)
            if u.defer and u.g is None and u.pool is None:
                u.g = torch.empty_like(u.a)
            # (Hessian: the scale's second-order term arrives as `rb` more partial rows for hf_pack_ex to add)
            u.gw_rows = u.rb * (2 if (self.hessian and u.bn is not None) else 1)
            if self.hessian and u.train:
                u.gw_rows += 1  # (+ the closed-form share of the scale's second-order term: hf_bn_train_hessian_coeffs)
            u.gw = torch.empty((u.gw_rows, k), dtype=f32, device=dev)
            u.gb = torch.empty((u.rb, k), dtype=f32, device=dev)
            if u.train:
                # The per-channel finalisation of a train-mode tangent / adjoint runs in the PROLOGUE of the elementwise
                # pass: its workgroups add the reduction's partial rows up themselves (hf_chan_affine_train).  The
                # forms of round 4 that handed over inside a launch or took a launch of their own were measured slower
                # (profiles/r04_train_bn_forms.jsonl) and are gone.
                if not (k % 4 == 0 and k // 4 <= 256):
                    raise _Unsupported(f"{u.name}: train-mode BatchNorm over {k} channels (the prologue form takes "
                                       "multiples of 4 up to 1024)")
                u.stat_part = torch.empty((u.rb, 2, k), dtype=torch.float64, device=dev)  # one-pass statistics
                # ... and the tangent's partial sums by the convolution's own epilogue (64x64-tile launches; one row per
                # (row tile, split): beyond 256 rows the separate reduction's `rb` rows are cheaper
                # for the elementwise pass to add up)
                tp_rows = -(-u.rows // 64) * u.sT
                u.epi = (not u.im2col and not u.first and hasattr(u, "xcat")
                         and tp_rows <= 256
                         and os.environ.get("HF_BN_EPILOGUE", "1") != "0")
                if self.hessian:
                    # Hessian products (hf_bn_train_hessian_*): the tangent sweep's partial sums must outlive the
                    # adjoint's (which share gw / gb in a GGN product); six coefficient vectors; the layer's
                    # first-order parameter gradients (per step)
                    if u.bn.weight is None or u.bn.bias is None:  # (frozen scale / shift are fine: constants)
                        raise _Unsupported(f"{u.name}: Hessian products need an affine train-mode BatchNorm")
                    u.hx = torch.empty((u.rb, k), dtype=f32, device=dev)
                    u.h1 = torch.empty((u.rb, k), dtype=f32, device=dev)
                    u.hcoef = torch.empty((6, k), dtype=f32, device=dev)
                    u.gg1 = torch.zeros(k, dtype=f32, device=dev)
                    u.gb1 = torch.zeros(k, dtype=f32, device=dev)
                if u.epi:
                    u.tp1 = torch.empty((tp_rows, k), dtype=f32, device=dev)
                    u.tpx = torch.empty((tp_rows, k), dtype=f32, device=dev)
        # a head that reads the last map through an operand of its own (a plain stack's classifier tail) is a consumer
        # like a convolution: the same [t_x | x] NHWC buffer
        for t in self._head_operands():
            if id(t) not in xcats:
                n, c, h, w = t.shape
                xcats[id(t)] = torch.zeros((n, 2 * c, h, w), dtype=f32, device=dev).contiguous(memory_format=cl)
        # where each unit's output goes besides its own dense buffer: the [t_x | x] operand of its
        # consumer -- the tangent into the first half, the value (forward pass) into the second
        for u in self.units:
            xc = xcats.get(id(u.yp if u.pool is not None else u.y))
            c = u.y.shape[1]
            if u.pool is not None:
                # the pooled tangent goes straight into the consumer's operand (no full-resolution tangent map); the
                # value half is the pool launch's second output, not the bias / ReLU launch's
                if xc is None:
                    raise _Unsupported(f"{u.name}: nothing consumes the pooled map")
                u.tout, u.tout_ld, u.yout2, u.pool_out2 = xc[:, :c], 2 * c, None, xc[:, c:]
            elif xc is not None:
                u.tout, u.tout_ld, u.yout2 = xc[:, :c], 2 * c, xc[:, c:]
            else:
                u.tout, u.tout_ld, u.yout2 = torch.empty_like(u.y), 0, None
        self._xcats = xcats
        self._slot_list = list(self._tangent_slots.values())
        self._allocate_sums_table()
        self._carry_ok = True  # (the stem's launch carries the v_W scatter; False once the library refused it)
        # (I, H, W, O) copies: the weights (once per step) and, for Hessian products, V (per product)
        self._wt_slots = [(self._offs[u.pw], u.wT, u.x.shape[1]) for u in self.units
                          if not u.im2col and not u.first and u.pw is not None and u.sD]
        # frozen convolution weights: constants the flat parameter vector does not hold -- their W half / (I, H, W, O)
        # copy come from the parameter itself (`refresh_frozen`: at construction and whenever it was written to)
        self._frozen_w = [u for u in self.units if not u.im2col and u.pw is None]
        self._frozen_seen = {}
        self._vt_slots = [(self._offs[u.pw], u.vT, u.x.shape[1]) for u in self.units
                          if self.hessian and not u.im2col and u.sD and u.pw is not None]
        self._allocate_head()
        # the parameters as ONE flat vector, when they are consecutive views of one (the optimizer's
        # arena): every W half is then refreshed by a single scatter launch
        self._flat_params = _flat_view(self.params, self.n)

    def _head_operands(self):
        """The maps (``u.y`` / ``u.yp`` buffers) a kind's head reads as ``[t_x | x]`` operands; none by default."""
        return ()

    def _allocate_sums_table(self):
        """The deferred units' sums problems as ONE table in device memory, in adjoint-sweep order (static pointers: built
        and uploaded here, outside any captured region); ``u.sums_slot``: the unit's entry."""
        units = [u for u in self._adjoint_order() if u.defer]
        self._sums_pending, self._sums_tab, self._sums_dev, self.sums_launches = set(), None, None, 0
        self._sums_units, self.split_fallbacks = units, 0
        if units:
            self._build_sums_table()

    def _build_sums_table(self):
        problems = []
        for i, u in enumerate(self._sums_units):
            bn = u.bn is not None and u.pg is not None
            u.sums_slot = i
            problems.append(dict(gw=u.gw.data_ptr() if bn else None, gb=u.gb.data_ptr() if u.pb is not None else None,
                                 g=(u.ga if u.pool is not None and u.bn is None else u.g).data_ptr(),
                                 x=u.a.data_ptr() if bn else None, mean=u.mean.data_ptr() if bn else None,
                                 rstd=u.rstd.data_ptr() if bn else None,
                                 rows=u.rows, c=u.cout, row_blocks=u.rb))
        self._sums_tab, _blocks = sums_table(problems)
        host = torch.frombuffer(bytearray(bytes(self._sums_tab)), dtype=torch.uint8)
        if self._sums_dev is None:
            self._sums_dev = host.to(self.dev)
        else:
            self._sums_dev.copy_(host)  # (in place: captured launches hold this pointer)

    def _split_now(self, u):
        """Whether this launch of ``u``'s adjoint is the elementwise one: planned so (``u.split``) AND the scale -- the one
        operand of that launch the model owns -- 16-byte aligned right now.  ``utils.ParameterArena`` binds the parameters
        as views at unpadded offsets of one vector, at any time after the buffers were allocated, so ``bn.weight`` can sit
        on any 4-byte boundary; the elementwise launch loads it by quads and has no scalar form, the fused launch reads
        it by scalar loads.  A misaligned unit takes the fused launch, which leaves its sums itself: nothing is pending."""
        if not u.split:
            return False
        w = u.scale
        if w is None or w.data_ptr() % 16 == 0:
            return True
        self.split_fallbacks += 1
        return False

    def bn_adjoint_report(self):
        """Which units' adjoints are planned as the elementwise launch, whose sums are deferred, how many sums launches
        the engine has issued so far, and how many adjoints planned as elementwise took the fused launch instead (a
        misaligned scale, ``_split_now``)."""
        return {"elementwise": [u.name for u in self.units if u.split and not u.dead],
                "deferred": [u.name for u in self._sums_units], "sums_launches": self.sums_launches,
                "fused_fallbacks": self.split_fallbacks}

    def _flush_sums(self):
        """The per-channel sums of every unit the sweep has deferred since the last flush: one launch per contiguous
        range of the table (one, for a whole sweep).  Runs in front of every gather."""
        if not self._sums_pending:
            return
        for first, count in sums_runs(self._sums_pending, _lib.BN_SUMS_MAX):
            self._launch("hf_bn_sums_multi", self._sums_dev, _lib.ctypes.cast(self._sums_tab, _lib.c_void_p),
                         len(self._sums_tab), first, count)
            self.sums_launches += 1
        self._sums_pending.clear()

    # ---- own forward pass ------------------------------------------------------------------
    def set_batch(self, x, targets=None):
        """A new input batch of the same shape (and its targets): static input, the stem's im2col."""
        if tuple(x.shape) != tuple(self.x_in.shape):
            raise RuntimeError("engine: input shape changed")
        self.x_in.copy_(x)
        s = self.units[0]
        if s.im2col:
            cols = torch.nn.functional.unfold(self.x_in.contiguous(), tuple(s.conv.kernel_size),
                                              padding=tuple(s.conv.padding), stride=tuple(s.conv.stride))
            s.cols.copy_(cols.transpose(1, 2))
            s.cols_pad[:, :, :s.jcols].copy_(s.cols)
        elif getattr(s, "xcat", None) is not None:
            # a first layer that reads the input itself (a plain stack with 4 or more input channels): the x half of its
            # [t_x | x] operand has no producer unit to fill it -- the tangent convolution's conv(x, v_W) reads it here
            # (the t_x half stays zero: the input carries no tangent)
            s.xcat[:, self.x_in.shape[1]:].copy_(self.x_in)
        for u in self.units:  # eval-mode statistics are constants -- unless somebody retrained them
            if u.bn is not None and not u.train and u.bn.running_var._version != u.rstd_version:
                torch.rsqrt(u.bn.running_var + u.bn.eps, out=u.rstd)
                u.rstd_version = u.bn.running_var._version
        # The sums table holds addresses.  All but one are buffers of the engine's own, allocated once and never replaced
        # (u.a, u.g, u.gw, u.gb, u.rstd; diag_ef allocates a u.g only where a unit has none, and a unit in the table has
        # one); the running mean is the one tensor in it that the MODEL owns (a load_state_dict or .to() may re-bind it):
        # rebuilt, eagerly, if that address moved
        if any(u.bn is not None and u.pg is not None and u.mean.data_ptr() != self._sums_tab[u.sums_slot].mean
               for u in self._sums_units):
            self._build_sums_table()
        self.refresh_frozen()
        if targets is not None:
            self.set_targets(targets)

    def refresh_frozen(self):
        """W halves and (I, H, W, O) copies of FROZEN convolution weights (not part of the flat vector the scatter
        launches read): copied when the parameter was written to or re-bound since the last look (eager, once per
        batch: never inside a captured graph)."""
        for u in self._frozen_w:
            w = u.conv.weight
            seen = (w._version, w.data_ptr())
            if self._frozen_seen.get(id(u)) != seen:
                c = u.x.shape[1]
                u.wcat[:, :c].copy_(w.detach())
                if u.sD:
                    u.wT.copy_(w.detach().permute(1, 2, 3, 0))
                self._frozen_seen[id(u)] = seen

    def set_targets(self, targets):
        if targets.dtype.is_floating_point:  # a mean-squared-error loss: targets of the outputs' shape
            if getattr(self, "_targets", None) is None:
                self._targets = torch.empty_like(self.logits)
                self._onehot = None
                self.bad_targets = torch.zeros((), dtype=torch.bool, device=self.dev)
            self._targets.copy_(targets)
            return
        if getattr(self, "_targets", None) is None:
            self._targets = torch.empty_like(targets)
            self._onehot = torch.zeros_like(self.logits)
        self._targets.copy_(targets)
        k = self.logits.shape[1]
        # class indices outside [0, K) (an ``ignore_index``) are not covered by the closed forms: the
        # flag is read back by the caller together with the loss value (no extra sync)
        self.bad_targets = ((self._targets < 0) | (self._targets >= k)).any()
        self._onehot.zero_()
        self._onehot.scatter_(1, self._targets.clamp(0, k - 1).view(-1, 1), 1.0)

    def refresh_weights(self, transposed=False):
        """The W halves of all [W | v_W] operands from the CURRENT parameters (one scatter launch
        when the parameters are views of one flat vector); ``transposed``: also the (I, H, W, O)
        copies the data-gradient convolutions read (once per step; trial points need only W)."""
        flat = self._flat_params
        if flat is not None and flat.data_ptr() == self.params[0].data_ptr():
            _lib.unpack_tangent(flat, self._slot_list, half=0)
        else:
            for u in self.units:
                if not u.im2col and u.pw is not None:
                    c = u.x.shape[1]
                    u.wcat[:, :c].copy_(self.params[u.pw].detach())
        if transposed:
            if flat is not None and flat.data_ptr() == self.params[0].data_ptr() and self._wt_slots:
                _lib.unpack_tangent(flat, self._wt_slots, half=2)
            else:
                for u in self.units:
                    if not u.im2col and not u.first and u.pw is not None and u.sD:
                        u.wT.copy_(self.params[u.pw].detach().permute(1, 2, 3, 0))

    def _zeros(self, k):
        cache = self.__dict__.setdefault("_zeros_cache", {})
        if k not in cache:
            cache[k] = torch.zeros(k, dtype=torch.float32, device=self.dev)
        return cache[k]

    def _param_slice(self, v, index, count):
        """``count`` entries of the flat vector ``v`` at parameter ``index`` (None: a frozen parameter -- no slice)."""
        return None if index is None else v[self._offs[index]: self._offs[index] + count]

    def _weight_tangent(self, v, u):
        """v_W of ``u``'s convolution as a slice of ``v``; zeros for a frozen weight (conv(x, 0) = 0)."""
        vw = self._param_slice(v, u.pw, u.conv.weight.numel())
        return self._zeros(u.conv.weight.numel()) if vw is None else vw

    def _chan_sums(self, gy, splits, slab, n, c, hw, row_blocks, **operands):
        """A plain per-channel reduction by the BatchNorm adjoint's launch (``problems.chan_sums_problem``)."""
        self._launch("hf_chan_affine_bwd_ex",
                     *bn_adjoint_args(chan_sums_problem(gy, splits, slab, n, c, hw, row_blocks, **operands)))

    # ---- kernels ---------------------------------------------------------------------------
    def _conv_slabs(self, direction, out, act, mat, geo, splits, **lds):
        """One slab-mode convolution (``problems.conv_problem``)."""
        self._launch("hf_conv2d_nhwc_slabs", *conv_args(conv_problem(direction, out, act, mat, geo, splits, **lds)))

    def _conv_carrying_scatter(self, u, mat, splits, src, half):
        """The im2col'd first layer's convolution (its weight operand ``mat`` is a slice of a flat vector, no
        scattered operand is read) in ONE launch with the scatter of ``src`` into the v_W (``half=1``) / W
        (``half=0``) halves of every other layer's operand (``hf_conv2d_nhwc_slabs_unpack``): the scatter hides
        behind the latency-bound convolution.  False: not taken (switched off, no scatter to carry, or a
        geometry / tensor count the merged launch refuses) -- the caller issues the two launches."""
        if not (self._carry_ok and u.im2col and self._slot_list):
            return False
        table = _lib.unpack_table(src, self._slot_list, half=half)
        periods = _lib.compact_periods(self._slot_list)
        conv = (u.tbuf, u.cols, mat, *u.geo.dims(), 0, 0, splits, u.tbuf.shape[1], src)
        if periods is not None:  # (local_compact: ``src`` is a vector in the compact layout)
            taken = self._launch_unless_refused("hf_conv2d_nhwc_slabs_unpack_compact", *conv, *table[:-1], periods,
                                                table[-1])
        else:
            taken = self._launch_unless_refused("hf_conv2d_nhwc_slabs_unpack", *conv, *table)
        self._carry_ok = taken  # (a refusal: not tried again)
        return taken
