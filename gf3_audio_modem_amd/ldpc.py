"""Quasi-cyclic LDPC forward error correction on the GPU (gf3_ldpc_* of include/gf3rx.h).

The code family is the project's own (tools/make_qcldpc.py -> data/qcldpc_z<Z>.json): lifting size Z = 64 (the
default), 128 or 256, 24 block columns, n = 24 Z = 1536 / 3072 / 6144 coded bits, rates 1/2, 2/3, 3/4, 5/6
(k = 12 Z, 16 Z, 18 Z, 20 Z), dual-diagonal parity part.
Encoding and the layered normalised min-sum decoder run in hand-written HIP (csrc/gf3rx_ldpc.hip); there is no host
implementation to fall back to.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import Gf3Error, ptr as _ptr

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
RATES = ("1/2", "2/3", "3/4", "5/6")
LIFTINGS = (64, 128, 256)
Z = 64                                  # the default lifting size


def shift_table(rate, Z=64):
    """int16 [mb, 24] shift table of one rate of the family of lifting size Z (-1 = zero block)."""
    if rate not in RATES:
        raise ValueError(f"unknown QC-LDPC rate {rate!r} (one of {', '.join(RATES)})")
    if Z not in LIFTINGS:
        raise ValueError(f"no QC-LDPC family of lifting size Z={Z} (one of {', '.join(map(str, LIFTINGS))})")
    with open(os.path.join(_DATA, f"qcldpc_z{Z}.json")) as f:
        return np.array(json.load(f)["rates"][rate], dtype=np.int16)


class QCLDPC:
    """One code of the family on one GPU.  Immutable; encode / decode are asynchronous on the current stream.

    QCLDPC(rate, device=None, Z=64), or QCLDPC(shifts=<int16 [mb, nb] table>, Z=64) for a code of one's own; Z is the
    lifting size, 64, 128 or 256 (n = Z nb)."""

    def __init__(self, rate="1/2", device=None, shifts=None, Z=64):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise Gf3Error("no GPU visible: QC-LDPC coding has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rate = None if shifts is not None else rate
        self.Z = int(Z)
        sh = np.ascontiguousarray(shift_table(rate, self.Z) if shifts is None else shifts, dtype=np.int16)
        if sh.ndim != 2:
            raise ValueError("shifts must be a 2-D table [mb, nb]")
        self.shifts = sh
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.gf3_ldpc_create(sh.shape[0], sh.shape[1], self.Z, sh.ctypes.data_as(C.c_void_p), C.byref(h))
        _lib.check(rc, prefix=False)
        self._h = h
        self.n = int(self.lib.gf3_ldpc_n(h))
        self.k = int(self.lib.gf3_ldpc_k(h))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gf3_ldpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x, dtype, width, what):
        x = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
        if x.numel() % width:
            raise ValueError(f"{what}: {x.numel()} values are not a whole number of rows of {width}")
        return x.reshape(-1, width)

    def encode(self, msg):
        """[n_cw, k] (or flat n_cw*k) 0/1 message bits -> uint8 [n_cw, n] codewords on the device, systematic first."""
        m = self._rows(msg, torch.uint8, self.k, "encode")
        cw = torch.empty((m.shape[0], self.n), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.gf3_ldpc_encode(self._h, _ptr(m), m.shape[0], _ptr(cw), _lib.stream(self.device)))
        return cw

    def decode(self, llr, max_iter=50, want_app=False, want_iters=False):
        """[n_cw, n] (or flat) float32 LLRs (> 0 <=> bit 0) -> uint8 [n_cw, k] decisions; with want_app / want_iters
        also the float32 [n_cw, n] APP LLRs and the int32 [n_cw] iteration counts (-max_iter: not converged)."""
        x = self._rows(llr, torch.float32, self.n, "decode")
        F = x.shape[0]
        bits = torch.empty((F, self.k), dtype=torch.uint8, device=self.device)
        app = torch.empty((F, self.n), dtype=torch.float32, device=self.device) if want_app else None
        its = torch.empty((F,), dtype=torch.int32, device=self.device) if want_iters else None
        _lib.check(self.lib.gf3_ldpc_decode(self._h, _ptr(x), F, int(max_iter), _ptr(bits), _ptr(app), _ptr(its),
                                             _lib.stream(self.device)))
        if not (want_app or want_iters):
            return bits
        return (bits,) + ((app,) if want_app else ()) + ((its,) if want_iters else ())
