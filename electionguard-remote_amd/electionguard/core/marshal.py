"""Marshalling of the entry points that come as a host-pointer ``name`` and a device-pointer
``name_dev`` (include/eg_hip_codes.h, _contestdata.h, _range.h, _preencrypt.h), and the small
conversions every wrapper of the C ABI needs.

A wrapper registers its buffers as COLUMNS, as the entry point itself does with csrc/eg_stage.hpp,
each with its per-item shape written once, and makes one call with the arguments in ABI order:

  cols = Columns(group)
  bn = cols.item(ballot_nonces, (32,), "ballot_nonces")   # per item, read; the first fixes mode and n
  dcon = cols.once(dcon_rows)                              # a host table read once per call
  srt = cols.out((nsel, 32))                               # per item, written; allocated by call()
  srt, = cols.call("eg_name", cols.n, nc, dcon, bn, srt)   # eg_name or eg_name_dev

  device mode  the first item column is a DeviceBuffer: every item column must be one, outputs are
               group.device_empty buffers, the once columns go up as ONE buffer of 32-byte rows.
  host mode    anything else: item columns become contiguous arrays of their dtype, outputs are
               numpy arrays (flag outputs bool), once columns are passed as they are.

Both modes check alike, before anything is allocated or called: an item column holds exactly
n x its row (ValueError naming it), and host and device columns do not mix (TypeError).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native


def ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def u32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def be32(x: int) -> bytes:
    """An integer as 32 big-endian bytes."""
    return int(x).to_bytes(32, "big")


def be32_row(x: int) -> np.ndarray:
    return np.frombuffer(be32(x), np.uint8)


def be_int(row) -> int:
    """The integer of a big-endian row."""
    return int.from_bytes(bytes(row), "big")


def q_row(x) -> np.ndarray:
    """One 32-byte element as a row: an integer (big-endian) or 32 bytes as given."""
    if isinstance(x, (int, np.integer)):
        return be32_row(x)
    a = np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)
    if a.shape != (32,):
        raise ValueError("a Q element is 32 bytes")
    return np.ascontiguousarray(a)


def rows32(a, n: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size != n * 32:
        raise ValueError(f"{what}: expected {n} x 32 bytes, got {a.size}")
    return a.reshape(n, 32)


def call(group, name: str, *args) -> None:
    native.check(group._lib, name, getattr(group._lib, name)(group.handle, *args))


def _is_device(x) -> bool:
    from .group import DeviceBuffer  # group imports this module
    return isinstance(x, DeviceBuffer)


class _Col:
    """One registered column: ``value`` is what the library reads or writes (an array, a
    DeviceBuffer, None for an unwanted output), ``arg`` the pointer call() passes."""
    __slots__ = ("value", "arg", "spec")

    def __init__(self, value=None, arg=None, spec=None):
        self.value, self.arg, self.spec = value, arg, spec


class Columns:
    """The columns of one call of a host / _dev pair (see the module's head)."""

    def __init__(self, group):
        self.group = group
        self.device = None   # set, with n, by the first item column
        self.n = 0
        self._outs, self._once = [], []

    def _take(self, value, count: int, shape, dtype, name: str, host) -> _Col:
        """value in this call's mode; it must hold count rows of shape (count None: the first item
        column, whose whole rows are counted into n)."""
        device = _is_device(value)
        if self.device is None:
            self.device = device
        if device != self.device:
            raise TypeError(f"{name}: {'a DeviceBuffer' if self.device else 'a host array'} is needed here, "
                            "host and device columns do not mix")
        if not device:
            value = np.ascontiguousarray(host(value) if host else value, dtype=dtype)
        row = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        if count is None:
            count = self.n = value.nbytes // row
        if value.nbytes != count * row:
            raise ValueError(f"{name}: expected {count} x {row} bytes, got {value.nbytes}")
        return _Col(value, value.ptr) if device else _Col(value.reshape((count,) + tuple(shape)), ptr(value))

    def item(self, value, shape, name: str, dtype=np.uint8, host=None) -> _Col:
        """A per-item input of ``shape`` per item; ``host`` converts a host value first (device
        buffers are taken as they are)."""
        return self._take(value, None if self.device is None else self.n, shape, dtype, name, host)

    def given(self, value, name: str, host=q_row) -> _Col:
        """A 32-byte element read once per call that a device-mode caller holds in HBM already."""
        return self._take(value, 1, (32,), np.uint8, name, host)

    def once(self, rows: np.ndarray) -> _Col:
        """A host table of 32-byte rows read once per call, in either mode."""
        col = _Col(rows)
        self._once.append(col)
        return col

    def out(self, shape, dtype=np.uint8, want: bool = True, per: int = 1, flag: bool = False) -> _Col:
        """A per-item output, (n * per,) + shape in all; not wanted: a null pointer and None.
        flag: ok bytes, bool in host mode."""
        col = _Col(spec=(tuple(shape), dtype, per, flag) if want else None)
        self._outs.append(col)
        return col

    def call(self, name: str, *args) -> list:
        """name or name_dev with args in ABI order, columns as their pointers -> the outputs'
        values in the order they were registered."""
        if self.device and self._once:
            desc = self.group.to_device(np.concatenate([c.value.reshape(-1) for c in self._once]))
            at = desc.ptr
            for c in self._once:
                c.arg, at = at, at + c.value.size
        else:
            for c in self._once:
                c.arg = ptr(c.value)
        for c in self._outs:
            if c.spec is not None:
                shape, dtype, per, _ = c.spec
                shape = (self.n * per,) + shape
                c.value = self.group.device_empty(shape, dtype) if self.device else np.zeros(shape, dtype)
                c.arg = c.value.ptr if self.device else ptr(c.value)
        call(self.group, name + "_dev" if self.device else name,
             *(a.arg if isinstance(a, _Col) else a for a in args))
        # the once buffer's free waits for the stream (eg_dev_free)
        return [c.value.astype(bool) if c.spec and c.spec[3] and not self.device else c.value for c in self._outs]
