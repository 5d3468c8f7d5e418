"""Multi-exponentiation: products of powers over many variable bases with ONE exponent vector
shared by every row (include/eg_hip_prodpow.h).

  out[r] = prod_{i<n} B[r, i]^{e_i} mod p
  layout "rows":  bases (rows, row_stride >= n, 512): row r's terms lie side by side (a stack of
                  shares, one row per text)
  layout "terms": bases (N >= n, rows, 512): term i's rows lie side by side (N ciphertext rows of
                  width rows, one product per column)

The exponents are used as given (not reduced mod q) and must be PUBLIC: both methods are variable
time, and the library refuses the call while ``group.ct_pow`` is on.  ``prod_pow_host`` restates the
definition on CPython ints and never calls the GPU; ``plan`` is pure host code of the library.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np

from .core import native
from .core.marshal import Columns, be32, ptr

AUTO, INTERLEAVED, BUCKETS = 0, 1, 2
MAX_TERMS, MAX_ROWS, MAX_ITEMS = 1 << 20, 1 << 16, 1 << 24
LAYOUTS = ("rows", "terms")


class Plan(NamedTuple):
    method: int        # INTERLEAVED or BUCKETS: the method that will run
    window_bits: int   # its window width
    mont_ops: float    # upper bound on the Montgomery multiplies of its schedule, all rows


def plan(rows: int, n: int, method: int = AUTO, window_bits: int = 0) -> Plan:
    """What eg_prod_pow would run for this shape, and the bound on its multiplies (no GPU)."""
    lib = native.load()
    m, w, ops = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
    native.check(lib, "eg_prod_pow_plan", lib.eg_prod_pow_plan(int(rows), int(n), int(method), int(window_bits),
                                                               ctypes.byref(m), ctypes.byref(w), ctypes.byref(ops)))
    return Plan(m.value, w.value, ops.value)


def prod_pow_host(p: int, bases: Sequence[Sequence[int]], exps: Sequence[int]) -> list:
    """out[r] = prod_i bases[r][i]^exps[i] mod p on CPython ints (x^0 = 1 also for x = 0)."""
    out = []
    for row in bases:
        if len(row) != len(exps):
            raise ValueError("every row holds one base per exponent")
        acc = 1 % p
        for b, e in zip(row, exps):
            acc = acc * pow(int(b) % p, int(e), p) % p
        out.append(acc)
    return out


def _exps_array(exps) -> np.ndarray:
    if hasattr(exps, "download") or (isinstance(exps, np.ndarray) and exps.dtype == np.uint8):
        return exps
    return np.frombuffer(b"".join(be32(e) for e in exps), np.uint8).reshape(-1, 32)


def _geometry(bases, layout: str, n: int):
    """-> (rows, row_stride, term_stride) of a 3-d bases array for n terms."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout: one of {LAYOUTS}, got {layout!r}")
    shape = tuple(getattr(bases, "shape", ()))
    if len(shape) != 3 or shape[2] != 512:
        raise ValueError(f"bases: expected a (., ., 512) array, got shape {shape}")
    if layout == "rows":
        rows, rs, ts, room = shape[0], shape[1], 1, shape[1]
    else:
        rows, rs, ts, room = shape[1], 1, shape[1], shape[0]
    if n > room:
        raise ValueError(f"bases: layout {layout!r} of shape {shape} holds {room} terms per row, exps has {n}")
    return rows, rs, ts


def prod_pow(group, bases, exps, layout: str = "rows", method: int = AUTO, window_bits: int = 0, out=None):
    """out (rows, 512) = prod_i B[r, i]^{e_i}: numpy arrays through eg_prod_pow, DeviceBuffers
    through eg_prod_pow_dev (asynchronous on the context's stream, a DeviceBuffer back).  exps:
    (n, 32) big-endian bytes (or, on the host, a sequence of ints).  The strided bases are checked
    against (rows-1) row_stride + (n-1) term_stride + 1 elements and the library's limits before
    anything is allocated or called.  out: where to write instead (rows x 512 bytes of the call's
    kind: a uint8 array or a DeviceBuffer)."""
    cols = Columns(group)
    b = cols.item(bases, (512,), "bases")
    have = cols.n
    if not cols.device:
        exps = _exps_array(exps)
    cols.n = int(np.prod(getattr(exps, "shape", (0,)), dtype=np.int64)) // 32
    e = cols.item(exps, (32,), "exps")
    n = cols.n
    rows, rs, ts = _geometry(bases, layout, n)
    need = (rows - 1) * rs + (n - 1) * ts + 1 if rows and n else 0
    if have < need:
        raise ValueError(f"bases: expected at least {need} x 512 bytes, got {have} x 512")
    if n > MAX_TERMS or rows > MAX_ROWS or rows * n > MAX_ITEMS:
        raise ValueError(f"prod_pow: {rows} rows x {n} terms exceed 2^16 rows, 2^20 terms or 2^24 in all")
    cols.n = rows
    if out is None:
        out, = cols.call("eg_prod_pow", b, rs, ts, e, rows, n, int(method), int(window_bits), cols.out((512,)))
        return out
    if isinstance(out, np.ndarray) == bool(cols.device) or out.nbytes != rows * 512 or \
            (isinstance(out, np.ndarray) and not (out.dtype == np.uint8 and out.flags.c_contiguous)):
        raise ValueError(f"out: expected {rows} x 512 bytes of the call's kind")
    cols.call("eg_prod_pow", b, rs, ts, e, rows, n, int(method), int(window_bits),
              out.ptr if cols.device else ptr(out))
    return out


def lagrange_combine(group, shares, weights):
    """M (texts, 512) with M[t] = prod_k shares[t, k]^{weights[k]}: the mediator's combine of k share
    arrays stacked as (texts, k, 512) in ONE call per 2^16 texts (a weight of 1 for a direct share,
    the Lagrange coefficient for a compensated one).  weights: k ints, or (k, 32) bytes; a
    DeviceBuffer stack takes DeviceBuffer weights and gives a DeviceBuffer."""
    if not hasattr(shares, "download"):
        shares = np.ascontiguousarray(shares, dtype=np.uint8)
    texts = shares.shape[0]
    if texts <= MAX_ROWS:
        return prod_pow(group, shares, weights, layout="rows")
    host = not hasattr(shares, "download")
    out = np.empty((texts, 512), np.uint8) if host else group.device_empty((texts, 512))
    for t0 in range(0, texts, MAX_ROWS):
        prod_pow(group, shares[t0:t0 + MAX_ROWS], weights, layout="rows", out=out[t0:t0 + MAX_ROWS])
    return out
