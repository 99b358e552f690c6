"""Outer Reed-Solomon erasure code across LDPC codewords (gf3_outer_* of include/gf3rx.h).

R parity codewords per group of G data codewords, computed over GF(2^8) on the message bytes, repair any R members of
the group whose inner decoding failed (iters < 0).  Both directions run in hand-written HIP (csrc/gf3rx_outer.hip);
there is no host implementation to fall back to.  layout() is the arithmetic the façade places groups in packets with.
"""
import torch

from . import _lib
from ._lib import Gf3Error, ptr as _ptr


def layout(F, per_packet, n, G, R):
    """(cap, NG): whole codewords of n coded bits in F packets of per_packet coded bits, and the groups of G + R among them."""
    cap = F * per_packet // n
    return cap, cap // (G + R)


def packets_for(n_bits, per_packet, n, k, G, R):
    """The smallest packet count F whose NG(F) >= 1 groups hold n_bits message bits."""
    F = 1
    while True:
        NG = layout(F, per_packet, n, G, R)[1]
        if NG >= 1 and NG * G * k >= n_bits:
            return F
        F += 1


def transmitted_index(g, t, NG):
    """Codeword number of member t (t < G: data, then parity) of group g: the groups are strided, so a run of up to NG
    consecutive failed codewords costs each group one member."""
    return t * NG + g


def to_transmitted(data, parity):
    """data [NG, G, k], parity [NG, R, k] (tensors) -> [(G + R) NG, k]: row transmitted_index(g, t, NG) is member t of group g."""
    return torch.cat([data.transpose(0, 1), parity.transpose(0, 1)]).reshape(-1, data.shape[-1])


def from_transmitted(rows, NG, G):
    """The inverse on the data members: rows in transmitted order -> [NG G, k], member t of group g in row g G + t."""
    return rows[: NG * G].reshape(G, NG, rows.shape[-1]).transpose(0, 1).reshape(NG * G, rows.shape[-1])


class OuterRS:
    """The code of G data + R parity members on messages of k bits, on one GPU.  Stateless in the library; this object
    only carries the geometry.  1 <= R <= 16, G >= 1, G + R <= 255, k a multiple of 8 (ValueError otherwise)."""

    def __init__(self, G, R, k, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise Gf3Error("no GPU visible: the outer code has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.G, self.R, self.k = int(G), int(R), int(k)
        _lib.check(self.lib.gf3_outer_encode(None, 0, self.G, self.R, self.k, None, None))     # (the geometry alone)

    def _rows(self, x, per_group, what):
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.uint8).contiguous()
        if x.numel() % (per_group * self.k):
            raise ValueError(f"{what}: {x.numel()} bits are not whole groups of {per_group} rows of {self.k}")
        return x.reshape(x.numel() // self.k, self.k)

    def encode(self, msg_bits):
        """[NG*G, k] (or flat) 0/1 message bits, member j of group g in row g*G + j -> uint8 [NG*R, k] parity bits, row
        g*R + r, on the device."""
        m = self._rows(msg_bits, self.G, "encode")
        NG = m.shape[0] // self.G
        par = torch.empty((NG * self.R, self.k), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gf3_outer_encode(_ptr(m), NG, self.G, self.R, self.k, _ptr(par), _lib.stream(self.device)))
        return par

    def recover(self, bits, iters):
        """bits [(G+R)*NG, k] (or flat) in transmitted order (member t of group g in row t*NG + g), iters [(G+R)*NG]
        (< 0: erased) -> (bits, int32 status [NG]).  A contiguous uint8 tensor on this device is repaired in place and
        returned; anything else is copied first.  status: 0 nothing to do, e_d > 0 members rewritten, -e_d beyond repair."""
        b = self._rows(bits, self.G + self.R, "recover")
        NG = b.shape[0] // (self.G + self.R)
        it = torch.as_tensor(iters).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        if it.numel() != b.shape[0]:
            raise ValueError(f"recover: {it.numel()} iteration counts for {b.shape[0]} rows")
        status = torch.empty((NG,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gf3_outer_recover(_ptr(b), _ptr(it), NG, self.G, self.R, self.k, _ptr(status), _lib.stream(self.device)))
        return b, status
