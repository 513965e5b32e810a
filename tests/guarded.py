"""What the GPU tests that call a kernel through the C ABI share: operands in NaN-filled buffers (a read outside the
operand would poison the result), outputs in sentinel-filled buffers with guard words, every launch issued twice and
compared bitwise, "nothing outside the payload was written" as ``untouched()``.  Nothing here knows a kernel; the layouts
are pinned on the CPU by ``test_guarded_cpu.py``."""

import numpy as np
import torch

from pytorchhessianfree_amd import _lib

DEV = "cuda"
GUARD = 64     # sentinel words in front of / behind an output
GAP = 8        # NaN words between two staged operand slabs
SLAB_GAP = 96  # NaN words between two split-K output slabs (``SlabOut``)
NAN = float("nan")
U32 = 2.0 ** -24
P = _lib.c_void_p
ERR_ARG = _lib.HF_ERR_ARG
F32 = _lib.HF_F32
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


def st():
    return _lib.current_stream_ptr(torch.device(DEV))


def p(t):
    return P(t.data_ptr()) if t is not None else None


def ptr(t):
    return t.data_ptr() if t is not None else None


def optr(o):
    return o.ptr if o is not None else None


def dv(t):
    return t.to(DEV).contiguous() if t is not None else None


def dev(a, device=DEV):
    """A numpy array on the device, 16-byte aligned."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert t.numel() == 0 or t.data_ptr() % 16 == 0
    return t


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def slabs_dev(t, stride):
    """[S, ...] -> S slabs ``stride`` elements apart on the device, NaN in between and behind (None stays None)."""
    if t is None:
        return None
    S, numel = t.shape[0], t[0].numel()
    buf = torch.full((S, stride), NAN)
    buf[:, :numel] = t.reshape(S, numel)
    return buf.to(DEV)


def wide(t, ld):
    """[rows, c] -> the first-c-channels slice of a [rows, ld] device buffer whose other channels hold NaN."""
    if t is None or not ld:
        return dv(t)
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)


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


class _Out:
    """A device buffer filled with a sentinel: NaN, or -7 for an integer dtype."""

    def _alloc(self, words, dtype, device):
        self.buf = torch.full((words,), NAN if dtype.is_floating_point else -7, dtype=dtype, device=device)

    def _kept(self, t):
        return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == -7).all())

    def same(self, other):
        """Bitwise: -0.0 is not +0.0, a NaN equals only the NaN of the same bits."""
        iv = {4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        return torch.equal(self.buf.view(iv), other.buf.view(iv))

    def pristine(self):
        """Nothing at all was written, the payload included."""
        return self._kept(self.buf)


class RowOut(_Out):
    """An output of ``rows`` x ``c`` elements inside a NaN-filled buffer: pixel stride ``ld`` (0 = dense), ``extra``
    more rows that must stay untouched, and GUARD words behind it."""

    def __init__(self, rows, c, ld=0, extra=0, dtype=torch.float32, device=DEV):
        self.rows, self.c, self.w = rows, c, (ld or c)
        self._alloc((rows + extra) * self.w + GUARD, dtype, device)

    @property
    def ptr(self):
        return P(self.buf.data_ptr())

    @property
    def val(self):
        return self.buf[:self.rows * self.w].view(self.rows, self.w)[:, :self.c]

    def untouched(self):
        body = self.buf[:self.rows * self.w].view(self.rows, self.w)[:, self.c:]
        return self._kept(body) and self._kept(self.buf[self.rows * self.w:])


class FlatOut(_Out):
    """``slabs`` outputs of ``numel`` elements, ``stride`` apart (0 = numel), the first one ``off`` elements behind a
    16-byte boundary: ``front`` guard words, ``off`` words, the slabs, GUARD words; all sentinel.  ``val``: the first
    slab as ``shape``; ``body``: all of them, [slabs, numel]."""

    def __init__(self, numel, off=0, slabs=1, stride=0, front=0, dtype=torch.float32, shape=None, device=DEV):
        self.numel, self.lo, self.slabs, self.stride, self.shape = numel, front + off, slabs, (stride or numel), shape
        self._alloc(self.lo + self.stride * slabs + GUARD, dtype, device)
        self.ptr = P(self.buf.data_ptr() + self.buf.element_size() * self.lo)

    def _slabs(self):
        return self.buf[self.lo:self.lo + self.stride * self.slabs].view(self.slabs, self.stride)

    @property
    def body(self):
        return self._slabs()[:, :self.numel]

    @property
    def val(self):
        v = self.buf[self.lo:self.lo + self.numel]
        return v.view(self.shape) if self.shape else v

    def untouched(self):
        rest = torch.cat([self.buf[:self.lo], self.buf[self.lo + self.stride * self.slabs:]])
        return self._kept(self._slabs()[:, self.numel:]) and self._kept(rest)


class SlabOut(_Out):
    """``splits`` slabs of ``numel`` floats, ``stride`` = numel (rounded up to a 16-byte multiple) + SLAB_GAP apart,
    between GUARD floats on each side; all NaN.  ``ptr`` is an integer, on the 16-byte grid."""

    def __init__(self, numel, splits, device=DEV):
        self.numel, self.splits = numel, splits
        self.stride = -(-numel // 4) * 4 + SLAB_GAP
        self._alloc(2 * GUARD + splits * self.stride, torch.float32, device)
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0
        inside = torch.zeros(splits, self.stride, dtype=torch.bool, device=device)
        inside[:, :numel] = True
        pad = torch.zeros(GUARD, dtype=torch.bool, device=device)
        self.inside = torch.cat([pad, inside.reshape(-1), pad])

    def slabs(self):
        return self.buf[GUARD:GUARD + self.splits * self.stride].view(self.splits, self.stride)[:, :self.numel]

    def untouched(self):
        return self._kept(self.buf[~self.inside])


class Payload:
    """A numpy ``payload`` on the device between GUARD NaN sentinels on each side; the payload (``t``) starts 16-byte
    aligned.  ``before`` is the host image of the whole buffer."""

    def __init__(self, payload, device=DEV):
        guard = np.full(GUARD, NAN, payload.dtype)
        self.size = payload.size
        self.before = np.concatenate([guard, payload, guard])
        self.buf = dev(self.before.copy(), device)  # (a copy: on the CPU the tensor would share ``before``'s memory)
        self.t = self.buf[GUARD:GUARD + payload.size]
        assert self.t.data_ptr() % 16 == 0

    def after(self):
        return self.buf.cpu().numpy()

    def expect(self, payload):
        e = self.before.copy()
        e[GUARD:GUARD + self.size] = np.asarray(payload).ravel()
        return e

    def untouched(self):
        after = self.after()
        return bool(np.isnan(after[:GUARD]).all()) and bool(np.isnan(after[GUARD + self.size:]).all())

    def pristine(self):
        """Nothing at all was written: the buffer is ``before`` (NaN sentinels are compared by position)."""
        return np.array_equal(self.after(), self.before, equal_nan=True)


def twice(launch):
    """``launch`` (returns its fresh output, or a tuple of them with None for an absent one) issued twice: the same bits,
    and nothing outside the payloads written.  Returns the first launch's."""
    a, b = launch(), launch()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for x, y in zip(a, b) if isinstance(a, (tuple, list)) else ((a, b),):
        if x is not None:
            assert x.same(y), "two launches on the same inputs differ"
            assert x.untouched(), "a guard word, a gap or the other half of a wider buffer was written"
    return a
