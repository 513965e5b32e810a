"""What the GPU tests of the dense-layer kernels (``test_dense_kernels_gpu.py``, ``test_dense_hess_kernels_gpu.py``,
``test_dense_diag_kernels_gpu.py``) share: operands in NaN-filled buffers (a read outside ``rows x c`` would poison the
result), outputs in NaN-filled buffers with guard words, every launch issued twice and compared bitwise."""

import numpy as np
import torch

import dense_refs as dr
from pytorchhessianfree_amd import _lib

DEV = "cuda"
GUARD = 64
NAN = float("nan")
P = _lib.c_void_p
ERR_ARG = _lib.HF_ERR_ARG
F32 = _lib.HF_F32
ACTS = (dr.IDENTITY, dr.RELU, dr.TANH)
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


def st():
    return _lib.current_stream_ptr(torch.device(DEV))


class In:
    """An operand inside a NaN-filled buffer, ``off`` floats behind a 16-byte boundary."""

    def __init__(self, arr, off):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        self.buf = torch.full((arr.size + off + 8,), NAN, device=DEV)
        self.buf[off:off + arr.size].copy_(torch.from_numpy(arr).reshape(-1))
        self.ptr = P(self.buf.data_ptr() + 4 * off)


def ip(arr, off):
    return None if arr is None else In(arr, off)


def pp(op):
    return None if op is None else op.ptr


class Out:
    """``slabs`` outputs of ``numel`` elements, ``stride`` apart, ``off`` floats behind a 16-byte boundary of a NaN-filled
    buffer with GUARD words behind the last one."""

    def __init__(self, numel, off, slabs=1, stride=0):
        self.numel, self.off, self.slabs, self.stride = numel, off, slabs, (stride or numel)
        self.buf = torch.full((off + self.stride * slabs + GUARD,), NAN, device=DEV)
        self.ptr = P(self.buf.data_ptr() + 4 * off)

    def val(self, shape):
        body = self.buf[self.off:self.off + self.stride * self.slabs].view(self.slabs, self.stride)[:, :self.numel]
        return body.reshape((self.slabs,) + tuple(shape)).cpu().numpy()

    def untouched(self):
        body = self.buf[self.off:self.off + self.stride * self.slabs].view(self.slabs, self.stride)[:, self.numel:]
        rest = torch.cat([self.buf[:self.off], self.buf[self.off + self.stride * self.slabs:]])
        return bool(torch.isnan(body).all()) and bool(torch.isnan(rest).all())

    def same(self, other):
        return torch.equal(self.buf.view(torch.int32), other.buf.view(torch.int32))


def twice(launch):
    a, b = launch(), launch()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is not None:
            assert x.same(y), "two launches on the same inputs differ"
            assert x.untouched(), "a guard word or the gap between two slabs was written"
    return a
