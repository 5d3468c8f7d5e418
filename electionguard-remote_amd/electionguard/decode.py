"""Decoding decrypted texts on the device (include/eg_hip_decode.h): a batch
inverse by Montgomery's trick and a baby-step giant-step discrete logarithm to the base g whose
table and giant steps live in HBM.

  batch_inverse(group, a)                  a[i]^-1 mod p, 0 for 0: eg_multinv_batch's bytes at about
                                           3 multiplies per element (variable time: public values)
  DecodeTable(group, max_count).counts(B, M=None)
                                           t in [0, max_count] with g^t = B[i] * M[i]^-1 (B[i] itself
                                           without M), -1 where there is none: np.int64 (n,)
  decode_counts(group, B, M, max_count)    the same through one table kept per (group, max_count)
  plan(n, max_count)                       what would run, and the bound on its multiplies (no GPU)

numpy arrays go through the host entry points, DeviceBuffers through the _dev twins (asynchronous
on the context's stream, a DeviceBuffer back).  ``batch_inverse_host`` and ``counts_host`` restate
the definitions on CPython ints and never call the GPU.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Sequence

import numpy as np

from .core import native
from .core.marshal import Columns

MAX_TEXTS, MAX_COUNT, STOP = 1 << 24, 1 << 32, 16


class Plan(NamedTuple):
    seg_len: int       # S: elements per segment of the inversion
    levels: int        # sweeps down (and up) before a^(p-2)
    pow_jobs: int      # elements that take a^(p-2)
    m: int             # baby steps, floor(sqrt(max_count)) + 1
    slots: int         # entries of the open-addressing table
    load: float        # m / slots
    inv_ops: float     # Montgomery multiplies of the inversion
    mont_ops: float    # upper bound on the multiplies of counts(B, M): inversion, B * M^-1, giant steps


def plan(n: int, max_count: int = 0) -> Plan:
    """eg_decode_plan: pure host code of the library, the function its dispatcher calls."""
    lib = native.load()
    u = [ctypes.c_uint32(0) for _ in range(5)]
    d = [ctypes.c_double(0) for _ in range(3)]
    native.check(lib, "eg_decode_plan", lib.eg_decode_plan(int(n), int(max_count), *(ctypes.byref(x) for x in u),
                                                           *(ctypes.byref(x) for x in d)))
    return Plan(*(x.value for x in u), *(x.value for x in d))


def batch_inverse_host(p: int, a: Sequence[int]) -> list:
    """a[i]^-1 mod p on CPython ints (BigInteger.modInverse, with 0 for a value that is 0 mod p)."""
    return [pow(int(x) % p, -1, p) if int(x) % p else 0 for x in a]


def counts_host(p: int, g: int, ys: Sequence[int], max_count: int) -> list:
    """The t in [0, max_count] with g^t = y mod p for every y, -1 where there is none (baby-step
    giant-step on CPython ints)."""
    m = math.isqrt(max_count) + 1
    baby, x = {}, 1 % p
    for j in range(m):
        baby[x] = j
        x = x * g % p
    step = pow(g, -m, p)
    out = []
    for y in ys:
        y, t = int(y) % p, -1
        for i in range(m + 1):
            j = baby.get(y)
            if j is not None and i * m + j <= max_count:
                t = i * m + j
                break
            y = y * step % p
        out.append(t)
    return out


def batch_inverse(group, a):
    """(n, 512) inverses of the (n, 512) elements a, 0 for 0: a numpy array through
    eg_batch_inverse, a DeviceBuffer through eg_batch_inverse_dev.  Refused while ``group.ct_pow``
    is on (multInv_batch serves secret values)."""
    cols = Columns(group)
    x = cols.item(a, (512,), "a")
    out, = cols.call("eg_batch_inverse", x, cols.out((512,)), cols.n)
    return out


class _Via:
    """A group whose ``handle`` is a table's: Columns passes it as the call's first argument."""

    def __init__(self, group, handle):
        self._group, self.handle, self._lib = group, handle, group._lib

    def __getattr__(self, name):
        return getattr(self._group, name)


class DecodeTable:
    """The baby-step table of g for counts up to ``max_count``, built once on the device
    (eg_decode_table_create).  ``fp_bits``: the fingerprint width, 0 for the default of 64; widths
    down to 8 exist only so that tests can force fingerprint collisions -- answers stay exact.
    Close it before its group."""

    def __init__(self, group, max_count: int, fp_bits: int = 0):
        self.group, self.max_count, self.fp_bits = group, int(max_count), int(fp_bits)
        h = ctypes.c_void_p()
        native.check(group._lib, "eg_decode_table_create",
                     group._lib.eg_decode_table_create(group.handle, self.max_count, self.fp_bits, ctypes.byref(h)))
        self._tab = h

    def counts(self, B, M=None):
        """np.int64 (n,) for (n, 512) B and, if given, (n, 512) M: t with g^t = B[i] * M[i]^-1, else -1."""
        if self._tab is None:
            raise ValueError("the decode table is closed")
        cols = Columns(_Via(self.group, self._tab))
        b = cols.item(B, (512,), "B")
        m = cols.item(M, (512,), "M") if M is not None else None
        out, = cols.call("eg_decode_counts", b, m, cols.n, cols.out((), np.int64))
        return out

    def close(self) -> None:
        if getattr(self, "_tab", None) is not None:
            if getattr(self.group, "_ctx", None):
                self.group._lib.eg_decode_table_destroy(self._tab)
            self._tab = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def decode_counts(group, B, M, max_count: int):
    """DecodeTable(group, max_count).counts(B, M) with the table kept on the group for the next
    call, one per max_count."""
    per = group.__dict__.setdefault("_decode_tables", {})
    tab = per.get(int(max_count))
    if tab is None:
        tab = per[int(max_count)] = DecodeTable(group, max_count)
    return tab.counts(B, M)


def close_tables(group) -> None:
    """Destroy the tables decode_counts keeps on ``group`` (before the group is closed)."""
    for tab in group.__dict__.pop("_decode_tables", {}).values():
        tab.close()
