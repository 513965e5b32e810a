"""CPU: the descriptions of the conv-unit engines' BatchNorm / bias and convolution launches (``engine/problems.py``) and
the launcher (``engine/common._Launcher``).  Per struct kind of include/hf_pcg.h: the builder fills the struct from a
stand-in unit or from stand-in operands (CPU tensors), and the ``*_args`` function puts every field where the one-problem
entry point's prototype has it -- against the literal argument lists below, written from the header."""

import ctypes
import gc

import pytest
import torch

from pytorchhessianfree_amd import _lib
from pytorchhessianfree_amd.engine import problems as P
from pytorchhessianfree_amd.engine.common import _Launcher, _Unit

# the prototypes of include/hf_pcg.h without the trailing ``int dtype, void* stream``
AFFINE_EX = ("out", "a", "x", "mean", "rstd", "w", "q", "r", "add", "mask_src", "relu_self", "n", "c", "hw",
             "channels_last", "out_ld", "add_ld", "a_splits", "a_slab")
AFFINE_TRAIN = ("out", "a", "x", "mean", "rstd", "w", "part_x", "part_1", "nparts", "vq", "vr", "count", "add",
                "mask_src", "n", "c", "hw", "out_ld", "add_ld", "a_splits", "a_slab")
BWD_EX = ("gx", "gw", "gb", "gres", "gy", "gy_splits", "gy_slab", "gy2", "gy2_splits", "gy2_slab", "x", "mean", "rstd",
          "w", "mask_src", "n", "c", "hw", "channels_last", "row_blocks")
ADJOINT_V4 = ("g_out", "ga_out", "gy", "gy_splits", "gy_slab", "gy2", "gy2_splits", "gy2_slab", "mask_src", "w", "rstd",
              "rows", "c")
V4_FROM = {"g_out": "gres", "ga_out": "gx"}  # hf_bn_adjoint_v4_pair's reading of hf_bn_adjoint_problem
GEOMETRY = ("n", "h", "w", "c", "k", "r", "s", "stride_h", "stride_w", "pad_h", "pad_w")
CONV_SLABS = ("direction", "out", "act", "mat") + GEOMETRY + ("act_ld", "mat_ld", "out_c", "splits", "slab_stride")
BACKWARD_SLABS = ("dx", "dw", "dy", "x", "w_t") + GEOMETRY + ("splits_d", "slab_stride_d", "splits_w", "slab_stride_w")
# hf_conv2d_nhwc_backward_slabs's reading of the data-gradient problem ``d`` and the weight-gradient problem ``w``
BACKWARD_FROM = {"dx": "d.out", "dw": "w.out", "dy": "d.act", "x": "w.act", "w_t": "d.mat", "splits_d": "d.splits",
                 "slab_stride_d": "d.slab_stride", "splits_w": "w.splits", "slab_stride_w": "w.slab_stride"}

# entry point -> (prototype, struct, args function, arguments that are no field of the struct)
KINDS = {
    "hf_chan_affine_ex": (AFFINE_EX, _lib.AffineProblem, P.affine_args, {"channels_last": 1}),
    "hf_chan_affine_train": (AFFINE_TRAIN, _lib.AffineTrainProblem, P.affine_train_args, {"add_ld": 0}),
    "hf_chan_affine_bwd_ex": (BWD_EX, _lib.BnAdjointProblem, P.bn_adjoint_args, {"channels_last": 1}),
    "hf_bn_adjoint_v4": (ADJOINT_V4, _lib.BnAdjointProblem, P.bn_adjoint_v4_args, {}),
    "hf_conv2d_nhwc_slabs": (CONV_SLABS, _lib.ConvProblem, P.conv_args, {}),
}


def numbered(kind):
    """A struct whose fields hold 101, 102, ... in declaration order."""
    q = kind()
    for i, (name, ctype) in enumerate(kind._fields_):
        setattr(q, name, float(101 + i) if ctype is ctypes.c_double else 101 + i)
    return q


@pytest.mark.parametrize("entry", sorted(KINDS))
def test_args_have_the_entry_points_length_and_every_field_at_its_position(entry):
    proto, kind, args_of, extra = KINDS[entry]
    q = numbered(kind)
    args = args_of(q)
    assert len(args) == len(proto) == len(_lib.SIGNATURES[entry][1]) - 2
    fields = [name for name, _ in kind._fields_]
    for pos, name in enumerate(proto):
        if name in extra:
            assert args[pos] == extra[name], name
        elif name == "rows":
            assert args[pos] == q.n * q.hw
        else:
            field = V4_FROM.get(name, name)
            assert field in fields and args[pos] == getattr(q, field), name
    if entry != "hf_bn_adjoint_v4":  # (the elementwise launch does not read the sums' fields)
        assert set(fields) == set(proto) - set(extra)
    else:
        assert set(fields) - {V4_FROM.get(n, n) for n in proto} == {"gw", "gb", "x", "mean", "hw", "n", "row_blocks"}


def test_arguments_outside_the_struct_are_passed_on():
    assert P.affine_args(numbered(_lib.AffineProblem), channels_last=0)[AFFINE_EX.index("channels_last")] == 0
    assert P.bn_adjoint_args(numbered(_lib.BnAdjointProblem), channels_last=0)[BWD_EX.index("channels_last")] == 0
    assert P.affine_train_args(numbered(_lib.AffineTrainProblem), add_ld=24)[AFFINE_TRAIN.index("add_ld")] == 24


def unit(bn=True, relu=True, pg=0, pb=1, needs_g=True, train=False):
    """conv -> BatchNorm (or bias) -> ReLU on a [2, 8, 3, 3] map, two tangent slabs, three row blocks."""
    u = _Unit("u", None, torch.nn.BatchNorm2d(8) if bn else None)
    u.a, u.y, u.g, u.ga = (torch.zeros(2, 8, 3, 3) for _ in range(4))
    u.tout, u.tout_ld, u.tbuf, u.sT = torch.zeros(2, 16, 3, 3), 16, torch.zeros(2, 144), 2
    u.rstd = torch.ones(8) if bn else None
    u.mean_t = torch.zeros(8) if train else None
    u.gw, u.gb, u.rb = torch.zeros(3, 8), torch.zeros(3, 8), 3
    u.relu, u.pg, u.pb, u.needs_g, u.train = relu, pg, pb, needs_g, train
    return u


def addr(t):
    return None if t is None else t.data_ptr()


def test_eval_tangent_problem_of_a_unit():
    u, vq, vr, add = unit(), torch.zeros(8), torch.zeros(8), torch.zeros(2, 8, 3, 3)
    q = P.affine_problem(u, vq, vr, add, 8)
    want = dict(out=u.tout, a=u.tbuf, x=u.a, mean=u.bn.running_mean, rstd=u.rstd, w=u.bn.weight, q=vq, r=vr, add=add,
                mask_src=u.y)
    assert {k: getattr(q, k) for k in want} == {k: addr(t) for k, t in want.items()}
    assert (q.relu_self, q.n, q.c, q.hw, q.out_ld, q.add_ld, q.a_splits, q.a_slab) == (0, 2, 8, 9, 16, 8, 2, 144)
    # frozen scale / shift: no tangent; no ReLU: no mask; no residual: no addend
    q = P.affine_problem(unit(relu=False), None, None)
    assert (q.q, q.r, q.add, q.mask_src, q.add_ld) == (None, None, None, None, 0)
    # a bias-only unit has no statistics and no scale
    q = P.affine_problem(unit(bn=False), None, vr)
    assert (q.mean, q.rstd, q.w, q.q, q.r) == (None, None, None, None, vr.data_ptr())
    # train mode: the batch statistics, not the running ones
    u = unit(train=True)
    assert P.affine_problem(u, vq, vr).mean == u.mean_t.data_ptr()


def test_train_elementwise_problem_of_a_unit():
    u, vq, add = unit(train=True), torch.zeros(8), torch.zeros(2, 8, 3, 3)
    px, p1 = torch.zeros(5, 8), torch.zeros(5, 8)
    q = P.affine_train_problem(u, u.tout, u.tout_ld, u.tbuf, u.sT, 144, (px, p1, 5), vq, None, u.y, add)  # the tangent
    want = dict(out=u.tout, a=u.tbuf, x=u.a, mean=u.mean_t, rstd=u.rstd, w=u.bn.weight, part_x=px, part_1=p1, vq=vq,
                vr=None, add=add, mask_src=u.y)
    assert {k: getattr(q, k) for k in want} == {k: addr(t) for k, t in want.items()}
    assert (q.nparts, q.count, q.n, q.c, q.hw, q.out_ld, q.a_splits, q.a_slab) == (5, 18.0, 2, 8, 9, 16, 2, 144)
    q = P.affine_train_problem(u, u.ga, 0, u.g, 1, 0, (u.gw, u.gb, u.rb))  # the adjoint's second pass
    assert (q.out, q.a, q.part_x, q.part_1, q.nparts) == (addr(u.ga), addr(u.g), addr(u.gw), addr(u.gb), 3)
    assert (q.vq, q.vr, q.add, q.mask_src, q.out_ld, q.a_splits, q.a_slab) == (None, None, None, None, 0, 1, 0)


@pytest.mark.parametrize("bn,pb,needs_g", [(True, 1, True), (True, None, True), (False, 1, False), (True, 1, False),
                                           (False, None, True)])
def test_adjoint_problem_optional_fields(bn, pb, needs_g):
    """The fused one-problem launch passes gw and x only with a BatchNorm, gb only with a trainable shift, g only where
    it is read again; the two-problem, elementwise and reduction forms pass all four."""
    u, src = unit(bn=bn, pb=pb, needs_g=needs_g), torch.zeros(4, 144)
    q = P.bn_adjoint_problem(u, [(src, 4, 144)], only_needed=True)
    assert (q.gw, q.x) == ((addr(u.gw), addr(u.a)) if bn else (None, None))
    assert q.gb == (addr(u.gb) if pb is not None else None)
    assert q.gres == (addr(u.g) if needs_g else None)
    q = P.bn_adjoint_problem(u, [(src, 4, 144)])
    assert (q.gx, q.gw, q.gb, q.gres, q.x) == tuple(addr(t) for t in (u.ga, u.gw, u.gb, u.g, u.a))


def test_adjoint_problem_sources_mask_and_forms():
    u, s1, s2, ga = unit(), torch.zeros(4, 144), torch.zeros(2, 8, 3, 3), torch.zeros(2, 8, 3, 3)
    q = P.bn_adjoint_problem(u, [(s1, 4, 144)])
    assert (q.gy, q.gy_splits, q.gy_slab, q.gy2, q.gy2_splits, q.gy2_slab) == (addr(s1), 4, 144, None, 1, 0)
    assert (q.mean, q.rstd, q.w, q.mask_src) == tuple(addr(t) for t in (u.bn.running_mean, u.rstd, u.bn.weight, u.y))
    assert (q.n, q.c, q.hw, q.row_blocks) == (2, 8, 9, 3)
    q = P.bn_adjoint_problem(u, [(s1, 4, 144), (s2, 1, 0)], ga)
    assert (q.gy, q.gy_splits, q.gy_slab, q.gy2, q.gy2_splits, q.gy2_slab) == (addr(s1), 4, 144, addr(s2), 1, 0)
    assert q.gx == addr(ga)
    assert P.bn_adjoint_problem(u, [(s1, 4, 144)], reduce=True).gx is None  # the train-mode reduction pass
    assert P.bn_adjoint_problem(unit(relu=False), [(s1, 4, 144)]).mask_src is None
    for srcs in ([], [(s1, 4, 144)] * 3):
        with pytest.raises(RuntimeError, match=f"u: {len(srcs)} consumers"):
            P.bn_adjoint_problem(u, srcs)
    assert P.sources("u", [(s1, 4, 144)]) == (s1, 4, 144, None, 1, 0)


def test_plain_reduction_problem_names_its_operands():
    gy, gb = torch.zeros(2, 144), torch.zeros(3, 8)
    q = P.chan_sums_problem(gy, 2, 144, 2, 8, 9, 3, gb=gb)
    got = {name: getattr(q, name) for name, _ in _lib.BnAdjointProblem._fields_}
    assert got == dict(gx=None, gw=None, gb=addr(gb), gres=None, gy=addr(gy), gy_splits=2, gy_slab=144, gy2=None,
                       gy2_splits=1, gy2_slab=0, x=None, mean=None, rstd=None, w=None, mask_src=None, n=2, c=8, hw=9,
                       row_blocks=3)


class FakeLib:
    def __init__(self, code=0):
        self.calls, self.code = [], code

    def hf_fake(self, *args):
        self.calls.append(args)
        return self.code

    def hf_fake_pair(self, problems, dtype, stream):  # (the array lives for the duration of the call: copied here)
        self.calls.append(tuple((q.out, q.a_slab) for q in ctypes.cast(problems, ctypes.POINTER(_lib.AffineProblem * 2)).contents))
        return self.code

    def hf_fake_group(self, problems, count, dtype, stream):
        arr = ctypes.cast(problems, ctypes.POINTER(_lib.ConvProblem * count)).contents
        self.calls.append(([(q.out, q.slab_stride) for q in arr], dtype, stream))
        return self.code

    def hf_fake_bnsum(self, problems, count, sums, dtype, stream):
        arr = ctypes.cast(problems, ctypes.POINTER(_lib.ConvProblem * count)).contents
        bn = ctypes.cast(sums, ctypes.POINTER(_lib.ConvBnSum * count)).contents
        self.calls.append(([(q.out, b.part_1, b.part_rows) for q, b in zip(arr, bn)], dtype, stream))
        return self.code

    def hf_fake_dw(self, d, w, dtype, stream):
        self.calls.append(tuple(ctypes.cast(q, ctypes.POINTER(_lib.ConvProblem)).contents.out for q in (d, w)))
        return self.code

    def hf_error_string(self, code):
        return b"refused"


def test_launcher_fetches_the_entry_point_at_call_time(monkeypatch):
    """Tensors go as addresses, None as NULL, ``dtype, stream`` are appended, the return code is checked -- and the entry
    point is looked up in whatever ``_lib.load()`` returns at the moment of the call (what the launch recorders rely on)."""
    eng = _Launcher()
    eng.dev = torch.device("cpu")
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda dev: "stream")
    t = torch.zeros(4)
    first, second = FakeLib(), FakeLib(code=_lib.HF_ERR_ARG)
    monkeypatch.setattr(_lib, "load", lambda: first)
    eng._launch("hf_fake", t, None, 3, 0.5)
    (ptr, null, three, half, dtype, stream), = first.calls
    assert (ptr.value, null, three, half, dtype, stream) == (t.data_ptr(), None, 3, 0.5, _lib.HF_F32, "stream")
    monkeypatch.setattr(_lib, "load", lambda: second)
    assert eng._launch_rc("hf_fake", t) == _lib.HF_ERR_ARG and len(second.calls) == 1 and len(first.calls) == 1
    with pytest.raises(_lib.Refused):
        eng._launch("hf_fake", t)
    # the two-problem form: an array of the same two descriptions
    monkeypatch.setattr(_lib, "load", lambda: first)
    p1, p2 = numbered(_lib.AffineProblem), numbered(_lib.AffineProblem)
    p2.out = 7
    eng._launch_pair("hf_fake_pair", p1, p2)
    assert first.calls[-1] == ((101, p1.a_slab), (7, p1.a_slab))


def test_launcher_passes_lists_of_problems_as_contiguous_arrays(monkeypatch):
    """The array forms (grouped convolutions: ``array, count``; with BatchNorm sums: ``array, count, array``; the D + W
    launch: two pointers): the name is looked up at call time, every list arrives as one contiguous array of the given
    structs, ``dtype, stream`` are appended, and the refusal of a table is a return code the caller reads."""
    eng = _Launcher()
    eng.dev = torch.device("cpu")
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda dev: "stream")
    first, second = FakeLib(), FakeLib(code=_lib.HF_ERR_ARG)
    probs = [numbered(_lib.ConvProblem) for _ in range(3)]
    for i, q in enumerate(probs):
        q.out = 7 + i
    monkeypatch.setattr(_lib, "load", lambda: first)
    eng._launch("hf_fake_group", probs, len(probs))
    assert first.calls == [([(7, probs[0].slab_stride), (8, probs[0].slab_stride), (9, probs[0].slab_stride)],
                            _lib.HF_F32, "stream")]
    sums = [_lib.ConvBnSum(), P.conv_bnsum(*(torch.zeros(5, 8) for _ in range(5)))]
    monkeypatch.setattr(_lib, "load", lambda: second)
    assert eng._launch_rc("hf_fake_bnsum", probs[:2], 2, sums) == _lib.HF_ERR_ARG and not first.calls[1:]
    assert second.calls == [([(7, None, 0), (8, sums[1].part_1, 5)], _lib.HF_F32, "stream")]
    assert eng._launch_unless_refused("hf_fake_bnsum", probs[:2], 2, sums) is False and len(second.calls) == 2
    monkeypatch.setattr(_lib, "load", lambda: FakeLib(code=-3))  # (any other failure is no refusal)
    with pytest.raises(RuntimeError, match="hf_fake_bnsum failed with code -3"):
        eng._launch_unless_refused("hf_fake_bnsum", probs[:2], 2, sums)
    monkeypatch.setattr(_lib, "load", lambda: first)
    assert eng._launch_unless_refused("hf_fake_bnsum", probs[:2], 2, sums) is True
    eng._launch("hf_fake_dw", [probs[2]], [probs[0]])
    assert first.calls[-1] == (9, 7)
    # ... and no launch leaves work for the cycle collector (``ctypes.cast`` would: a captured sweep must not start it)
    gc.collect()
    gc.disable()
    try:
        for _ in range(50):
            eng._launch("hf_fake", probs, len(probs), sums, torch.zeros(1), None)
            eng._launch_pair("hf_fake", probs[0], probs[1])
        assert gc.collect() == 0
    finally:
        gc.enable()


def test_backward_args_take_every_position_from_the_right_problem():
    d, w = numbered(_lib.ConvProblem), numbered(_lib.ConvProblem)
    for q, direction in ((d, 1), (w, 2)):
        q.direction, q.act_ld, q.out_c, q.mat_ld = direction, 0, 0, 0
    for name in ("out", "act", "splits", "slab_stride"):  # what the two problems do not share
        setattr(w, name, getattr(w, name) + 1000)
    w.mat = d.act  # both read the same cotangent
    args = P.conv_backward_args(d, w)
    assert len(args) == len(BACKWARD_SLABS) == len(_lib.SIGNATURES["hf_conv2d_nhwc_backward_slabs"][1]) - 2
    for pos, name in enumerate(BACKWARD_SLABS):
        if name in GEOMETRY:
            assert args[pos] == getattr(d, name) == getattr(w, name), name
        else:
            which, field = BACKWARD_FROM[name].split(".")
            assert args[pos] == getattr({"d": d, "w": w}[which], field), name
    assert len(set(args)) == len(args)  # (no value stands at two positions: none was taken from the other problem)
    for name in GEOMETRY + ("mat", "act_ld", "out_c", "mat_ld"):  # another layer, another cotangent, a sliced operand
        other = _lib.ConvProblem.from_buffer_copy(w)
        setattr(other, name, getattr(w, name) + 1)
        with pytest.raises(RuntimeError, match="not the dense D \\+ W pair of one layer"):
            P.conv_backward_args(d, other)
    d.out_c = 4
    with pytest.raises(RuntimeError, match="not the dense"):
        P.conv_backward_args(d, w)


GEO = P.Geometry(5, 7, 6, 8, 12, 3, 2, (2, 1), (0, 1))  # r != s, per-axis stride and padding


def test_convolution_problem_from_operands_and_geometry():
    out2, out1, out4 = torch.zeros(3, 40), torch.zeros(40), torch.zeros(5, 12, 3, 6)
    act, mat = torch.zeros(5, 8, 7, 6), torch.zeros(12, 8, 3, 2)
    q = P.conv_problem(0, out2, act, mat, GEO, 3)
    assert (q.direction, q.out, q.act, q.mat) == (0, addr(out2), addr(act), addr(mat))
    assert tuple(getattr(q, name) for name in GEOMETRY) == (5, 7, 6, 8, 12, 3, 2, 2, 1, 0, 1)
    assert (q.act_ld, q.out_c, q.mat_ld, q.splits, q.slab_stride) == (0, 0, 0, 3, 40)
    # slabs are ``out.shape[1]`` apart in a [splits, numel] buffer; any other ``out`` is one slab
    assert [P.conv_problem(2, o, act, mat, GEO, 1).slab_stride for o in (out1, out2, out4)] == [0, 40, 0]
    q = P.conv_problem(2, out2, act, None, GEO, 2, act_ld=16, out_c=7, mat_ld=24)
    assert (q.direction, q.mat, q.act_ld, q.out_c, q.mat_ld, q.splits) == (2, None, 16, 7, 24, 2)
    b = P.conv_bnsum(act, None, out1, out2, out4)
    assert (b.x, b.mean, b.rstd, b.part_x, b.part_1, b.part_rows) == (addr(act), None, addr(out1), addr(out2), addr(out4), 5)
    z = _lib.ConvBnSum()  # a problem without sums
    assert (z.x, z.part_1, z.part_rows) == (None, None, 0)


def test_geometry_record():
    assert P.Geometry._fields == ("n", "h", "w", "c", "k", "r", "s", "stride", "padding")
    n, h, w, c, k, r, s, stride, padding = GEO  # (still a tuple: what reads ``u.geo`` positionally keeps working)
    assert (n, h, w, c, k, r, s, stride, padding) == (5, 7, 6, 8, 12, 3, 2, (2, 1), (0, 1)) == tuple(GEO)
    assert GEO.doubled() == GEO._replace(c=16) and GEO.doubled()._replace(c=8) == GEO
    assert GEO.with_n(1) == GEO._replace(n=1) and GEO.with_n(1)._replace(n=5) == GEO
    for g in (GEO.doubled(), GEO.with_n(42), GEO.doubled().with_n(1)):
        assert isinstance(g, P.Geometry) and (g.r, g.s, g.stride, g.padding) == (3, 2, (2, 1), (0, 1))
    assert GEO.dims() == (5, 7, 6, 8, 12, 3, 2, 2, 1, 0, 1) and len(GEO.dims()) == len(GEOMETRY)
    assert P.conv_sqsum_args(torch.zeros(2, 9), None, None, GEO, 2, 0.5, out_c=7)[3:] == GEO.dims() + (0, 7, 0.5, 2, 9)
