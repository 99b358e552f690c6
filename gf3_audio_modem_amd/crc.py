"""Per-codeword CRC-32 (gf3_crc_* of include/gf3rx.h).

The last 32 of a codeword's k message bits are the CRC-32/IEEE (zlib's crc32) of the k - 32 payload bits before them, taken
as bytes most significant bit first.  A codeword the LDPC decoder converged on wrongly has a zero syndrome and looks good;
its CRC does not match, and check() turns its iteration count negative, which is what the outer code erases.  Both
directions run in hand-written HIP (csrc/gf3rx_crc.hip); there is no host implementation to fall back to.
"""
import torch

from . import _lib
from ._lib import Gf3Error, ptr as _ptr

CRC_BITS = 32


class CodewordCRC:
    """The CRC on messages of k bits (payload k - 32), on one GPU.  Stateless in the library; this object only carries
    the geometry.  k a multiple of 8 in [40, 7936] (ValueError otherwise)."""

    def __init__(self, k, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise Gf3Error("no GPU visible: the codeword CRC has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.k = int(k)
        _lib.check(self.lib.gf3_crc_attach(None, 0, self.k, None, None))                       # (the geometry alone)
        self.k_payload = self.k - CRC_BITS

    def _rows(self, x, width, what):
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.uint8).contiguous()
        if x.numel() % width:
            raise ValueError(f"{what}: {x.numel()} bits are not whole rows of {width}")
        return x.reshape(x.numel() // width, width)

    def attach(self, payload):
        """[n_cw, k - 32] (or flat) 0/1 payload bits -> uint8 [n_cw, k] on the device: each row followed by its CRC field."""
        p = self._rows(payload, self.k_payload, "attach")
        msg = torch.empty((p.shape[0], self.k), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gf3_crc_attach(_ptr(p), p.shape[0], self.k, _ptr(msg), _lib.stream(self.device)))
        return msg

    def check(self, msg, iters=None):
        """[n_cw, k] (or flat) 0/1 message bits -> (payload uint8 [n_cw, k - 32], bad uint8 [n_cw], iters or None).
        bad: the field is not the CRC of the row's payload.  iters [n_cw]: v > 0 on a bad row becomes -v, every other
        value stays; a contiguous int32 tensor on this device is updated in place and returned, anything else is copied
        first."""
        m = self._rows(msg, self.k, "check")
        n_cw = m.shape[0]
        it = None
        if iters is not None:
            it = torch.as_tensor(iters).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
            if it.numel() != n_cw:
                raise ValueError(f"check: {it.numel()} iteration counts for {n_cw} rows")
        payload = torch.empty((n_cw, self.k_payload), dtype=torch.uint8, device=self.device)
        bad = torch.empty((n_cw,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gf3_crc_check(_ptr(m), n_cw, self.k, _ptr(payload), _ptr(it), _ptr(bad), _lib.stream(self.device)))
        return payload, bad, it
