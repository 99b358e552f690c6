"""Engine: torch-tensor front end of libgf3rx (include/gf3rx.h).

PyTorch is used for device memory, streams and (in dist.py) RCCL only; every
arithmetic step of the receive path runs in the hand-written HIP kernels behind
the C ABI.  There is no CPU path here: without a GPU or without the built
library, constructing an Engine raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, ingest
from ._lib import Gf3Error, ptr as _ptr  # noqa: F401  (Gf3Error is importable from here as before)
from .ingest import DIRECT_PIECE_BYTES, host_pieces  # noqa: F401  (the cut of a host stream, importable from here as before)

def _table(xs):
    """The branches' device tensors -> the table of their addresses the library takes (None stays None)."""
    return None if xs is None else (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])


_TORCH_DT = {_lib.DT_F64: torch.float64, _lib.DT_F32: torch.float32,
             _lib.DT_I16: torch.int16, _lib.DT_U8: torch.uint8}
_DT_OF = {v: k for k, v in _TORCH_DT.items()}


def qpsk_table():
    """QPSK Gray table in the reference's mapping_table order (OFDM.py:72-77)."""
    pts = np.array([(1 + 1j) / np.sqrt(2), (1 - 1j) / np.sqrt(2),
                    (-1 - 1j) / np.sqrt(2), (-1 + 1j) / np.sqrt(2)])
    bits = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.uint8)
    return pts, bits


def square_qam_table(mu):
    """Gray-coded square 2^mu-QAM, unit average energy, points in ascending label
    order (the reference's demap is table-generic, OFDM.py:484-500)."""
    if mu % 2 or mu < 2:
        raise ValueError("Invalid Modulation Type")
    h = mu // 2
    L = 1 << h
    lv = np.zeros(L)
    for i in range(L):
        lv[i ^ (i >> 1)] = 2 * i - (L - 1)
    scale = np.sqrt(2.0 * (L * L - 1) / 3.0)
    pts, bits = [], []
    for lab in range(1 << mu):
        pts.append((lv[lab >> h] + 1j * lv[lab & (L - 1)]) / scale)
        bits.append([(lab >> (mu - 1 - b)) & 1 for b in range(mu)])
    return np.array(pts), np.array(bits, dtype=np.uint8)


def map_bits(bits2d, const_points, const_bits):
    """transmitter.map (OFDM.py:196-197): rows of mu bits -> constellation points.  A label that no point carries
    (a table of M < 2^mu points) maps to the table's first point, as gf3_tx_frames maps it."""
    const_bits = np.asarray(const_bits)
    const_points = np.asarray(const_points, dtype=complex)
    mu = const_bits.shape[1]
    w = 1 << np.arange(mu - 1, -1, -1)
    lut = np.full(1 << mu, const_points[0], dtype=complex)
    lut[(const_bits * w).sum(axis=1)] = const_points
    return lut[(np.asarray(bits2d, dtype=np.int64) * w).sum(axis=-1)]


@dataclass
class RxConfig:
    """Python image of gf3_config == the attributes CamG.__init__ sets (OFDM.py:18-101)."""
    N: int = 4096
    CP: int = 224
    P: int = 20
    D: int = 180
    data_bins: np.ndarray = None            # data_carriers (OFDM.py:47)
    const_points: np.ndarray = field(default_factory=lambda: qpsk_table()[0])
    const_bits: np.ndarray = field(default_factory=lambda: qpsk_table()[1])
    known_bits: np.ndarray = None           # known_sequence, >= K*mu bits (OFDM.py:99-101)
    fs: float = 48000.0
    f0: float = 0.0
    f1: float = 8000.0
    thresh: float = 0.4
    fit_lo: int = 500
    fit_hi: int = 1000
    Lc: int = 0
    in_dtype: torch.dtype = torch.float64
    max_window: int = 512

    @property
    def K(self): return self.N // 2 - 1
    @property
    def S(self): return self.N + self.CP
    @property
    def M(self): return 2 * self.P + self.D
    @property
    def mu(self): return int(np.asarray(self.const_bits).shape[1])
    @property
    def C(self): return len(self.data_bins)
    @property
    def chirp_length(self): return self.Lc if self.Lc > 0 else 5 * self.S
    @property
    def frame_len(self): return self.chirp_length + self.M * self.S
    @property
    def bits_per_frame(self): return self.D * self.C * self.mu

    def known_symbols(self):
        kb = np.asarray(self.known_bits[: self.K * self.mu]).reshape(self.K, self.mu)
        return map_bits(kb, self.const_points, self.const_bits)


class ListOverflow(Gf3Error):
    """GF3_ERANGE of Engine.detect_chunk: `wanted` entries did not fit the list."""

    def __init__(self, text, wanted):
        super().__init__(text)
        self.wanted = wanted


class Loading:
    """One gf3_loading of an engine (Engine.loading): handle, the order table (uint8 [C]) and bits = Bs."""

    def __init__(self, engine, handle, order, bits):
        self.engine, self.handle, self.order, self.bits = engine, handle, order, bits
        self.order.setflags(write=False)


class Engine:
    """One gf3_ctx on one GPU."""

    def __init__(self, cfg: RxConfig, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise Gf3Error("no GPU visible: the gf3rx receive path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if cfg.data_bins is None:
            raise ValueError("RxConfig.data_bins is required")
        if cfg.known_bits is None or len(cfg.known_bits) < cfg.K * cfg.mu:
            raise ValueError("known_bits must hold at least K*mu bits")
        if cfg.in_dtype not in _DT_OF:
            raise ValueError(f"unsupported sample dtype {cfg.in_dtype}")
        self.cfg = cfg
        pts = np.ascontiguousarray(cfg.const_points, dtype=np.complex128)
        self._re = np.ascontiguousarray(pts.real)
        self._im = np.ascontiguousarray(pts.imag)
        self._bits = np.ascontiguousarray(cfg.const_bits, dtype=np.uint8)
        kn = cfg.known_symbols()
        self._kre = np.ascontiguousarray(kn.real)
        self._kim = np.ascontiguousarray(kn.imag)
        self._bins = np.ascontiguousarray(cfg.data_bins, dtype=np.int32)
        g = _lib.Gf3Config(
            N=cfg.N, CP=cfg.CP, P=cfg.P, D=cfg.D, Lc=cfg.Lc, fs=cfg.fs, f0=cfg.f0, f1=cfg.f1,
            thresh=cfg.thresh, fit_lo=cfg.fit_lo, fit_hi=cfg.fit_hi, mu=cfg.mu, M=len(pts),
            const_re=self._re.ctypes.data_as(_lib.c_double_p), const_im=self._im.ctypes.data_as(_lib.c_double_p),
            const_bits=self._bits.ctypes.data_as(C.POINTER(C.c_uint8)),
            known_re=self._kre.ctypes.data_as(_lib.c_double_p), known_im=self._kim.ctypes.data_as(_lib.c_double_p),
            data_bins=self._bins.ctypes.data_as(C.POINTER(C.c_int32)), C=len(self._bins),
            in_dtype=_DT_OF[cfg.in_dtype], max_window=cfg.max_window)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.gf3_ctx_create(C.byref(g), C.byref(h))
        _lib.check(rc, prefix=False)
        self._h = h
        self._sync_mode = 0
        self._tls = threading.local()
        self._loadings = {}                     # bytes of an order table -> Loading (Engine.loading), least recently used first
        self.n_cu = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        self.bytes_per_frame = int(self.lib.gf3_bytes_per_frame(h))
        self.max_window = int(self.lib.gf3_sync_max_window(h))

    def close(self):
        ingest.release(self)
        self._tls = threading.local()
        for ld in getattr(self, "_loadings", {}).values():
            self.lib.gf3_loading_destroy(ld.handle)
            ld.handle = None
        self._loadings = {}
        if getattr(self, "_h", None):
            self.lib.gf3_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    _check = staticmethod(_lib.check)

    def _stream(self):
        return _lib.stream(self.device)

    def _samples(self, x):
        """1-D (or any-D contiguous) device tensor of samples in the configured dtype."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not isinstance(x, torch.Tensor):
            raise TypeError("samples must be a torch tensor or numpy array")
        if x.dtype != self.cfg.in_dtype:
            x = x.to(self.cfg.in_dtype)
        return x.to(self.device).contiguous()

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _dev(self, x, dtype=torch.complex128):
        """x as a contiguous tensor of `dtype` (complex128 unless said otherwise) on this engine's device."""
        return torch.as_tensor(x, dtype=dtype).to(self.device).contiguous()

    def _out(self, out, shape, dtype, what, name="out"):
        """`out` if it is contiguous, of `dtype` and of prod(shape) = `what` elements (else ValueError); a fresh tensor for None."""
        if out is None:
            return self._new(shape, dtype)
        if out.dtype != dtype or out.numel() != math.prod(shape) or not out.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[1]} tensor of {what} elements")
        return out

    def _wanted(self, want, F, names):
        """The optional demodulator outputs among `names` that `want` asks for, allocated for F packets."""
        cfg, c128 = self.cfg, torch.complex128
        kinds = {"eq": ((F * cfg.D, cfg.C), c128), "Hs": ((F, cfg.K), c128), "He": ((F, cfg.K), c128),
                 "slope": ((F,), torch.float64), "Hest": ((F, cfg.D, cfg.K), c128)}
        o = {k: self._new(*kinds[k]) for k in names if k in want and k in kinds}
        if "status" in want:                                       # (the kernels only ever set bits in it)
            o["status"] = torch.zeros((1,), dtype=torch.int32, device=self.device)
        return o

    def _split_work(self, F, split):
        """(workspace, mode) of a demodulator call.  The two-phase form needs a workspace (pilot sums, and Hs / He / slope
        when they are not asked for): allocated exactly when the library would choose that form (at most 2 x CUs packets)."""
        work = None
        if F and (split or (split is None and self.lib.gf3_demod_split_plan(self._h, F, 0, None, None))):
            work = self._new((int(self.lib.gf3_demod_workspace_bytes(self._h, F)),), torch.uint8)
        return work, 0 if split is None else (2 if split else 1)

    def _last_call(self, query, cap_name):
        """Answer of a screened dispatcher's *_last query on the current stream: dict(path, <cap_name>).  No device read."""
        path, cap = C.c_int32(-1), C.c_int32(0)
        self._check(query(self._h, self._stream(), C.byref(path), C.byref(cap)))
        return {"path": int(path.value), cap_name: int(cap.value)}

    @staticmethod
    def _listed(work):
        """The numbers a screen left in its list workspace [count | pad to 64 bytes | int32 list], sorted."""
        n = int(work[:4].view(torch.int32).item())
        return torch.sort(work[64: 64 + 4 * n].view(torch.int32)).values

    # ------------------------------------------------------------------ ABI calls
    def chirp_replica(self):
        out = np.empty(self.cfg.chirp_length)
        self._check(self.lib.gf3_chirp_replica(self._h, out.ctypes.data_as(_lib.c_double_p)))
        return out

    def rfft_batch(self, x, offsets, out=None):
        """[n_sym, N/2+1] complex128 spectra of the N samples starting at each offset."""
        x = self._samples(x)
        offsets = self._dev(offsets, torch.int64)
        n = offsets.numel()
        out = self._out(out, (n, self.cfg.N // 2 + 1), torch.complex128, "n_sym * (N/2+1)")
        self._check(self.lib.gf3_rfft_batch(self._h, _ptr(x), x.numel(), _ptr(offsets), n, _ptr(out), self._stream()))
        return out

    @staticmethod
    def check_denoise(threshold):
        """ValueError for a denoising threshold that is not a finite number > 0 -> the threshold as a float."""
        number = isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, (bool, np.bool_))
        if not number or not math.isfinite(float(threshold)) or float(threshold) <= 0.0:
            raise ValueError(f"denoising threshold must be a finite number > 0, not {threshold!r}")
        return float(threshold)

    def denoise_pilots(self, x, frame_offsets, threshold=9.0):
        """The delay-domain denoiser of the pilot channel estimate on its own (gf3_denoise_pilots): per packet and side the
        time-domain sum of the P pilot symbols, with every delay-domain tap of its channel estimate below `threshold`
        times the tap noise variance -- measured from the pilot repeats -- set to zero.
        -> (psum float64 [F, 2, N], report float64 [F, 2, 5] = (v, kept, post, pre, applied)): noise variance, taps kept,
        the largest kept delay and the largest kept precursor (the measured delay spread), and whether the row was
        rewritten (not when v is not finite, the packet is ragged or more than N/4 taps are kept).  Needs P >= 2.  Fixed
        summation order: two calls give identical bytes."""
        threshold = self.check_denoise(threshold)
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        psum = self._new((F, 2, self.cfg.N), torch.float64)
        report = self._new((F, 2, 5), torch.float64)
        self._check(self.lib.gf3_denoise_pilots(self._h, _ptr(x), x.numel(), _ptr(off), F, threshold, _ptr(psum), _ptr(report),
                                                self._stream()))
        return psum, report

    def demod_frames(self, x, frame_offsets, want=(), out_bits=None, split=None, precision=None, denoise=None):
        """Fused a3-a10.  Returns dict with 'bits' (packed uint8
        [F, bytes_per_frame]) plus any of 'eq','Hs','He','slope','Hest','status'.
        split: None -- the library chooses between one packet per workgroup and the two-phase form for long packets,
        few at a time (gf3_demod_frames_ex: pilot sums, estimate, data symbols spread over the chip; the reference's own
        geometry of 3 packets x 220 symbols); False / True force the one or the other.
        precision: None -- the library decides (gf3_demod_frames_px precision -1): with the reference QPSK table, bits-only
        output and f32 / i16 / u8 samples the data symbols are transformed in fp32 under a proven bound and the fp64 kernel
        runs only on the packets the bound cannot decide -- the all-fp64 outputs, bit for bit.  "fp64": the all-fp64 kernel
        on every packet.  "screen": ask for the screened path (it still runs all fp64 where it does not apply).
        demod_frames_last() tells which way a call went.
        denoise: None, or the threshold of the delay-domain denoiser (denoise_pilots; 9.0 is 3 sigma): the call then takes
        the two-phase form (gf3_demod_frames_dn) with the pilot sums denoised ahead of the channel estimate, and the dict
        gains 'denoise_report' float64 [F, 2, 5].  Not with split=False or precision="screen" (the two-phase form has no
        fp32 screen): ValueError."""
        if precision not in (None, "fp64", "screen"):
            raise ValueError(f"precision must be None, 'fp64' or 'screen', not {precision!r}")
        if denoise is not None:
            denoise = self.check_denoise(denoise)
            if split is False or precision == "screen":
                raise ValueError("denoise runs in the two-phase form: not with split=False or precision='screen'")
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        bits = out_bits if out_bits is not None else self._new((F, self.bytes_per_frame), torch.uint8)
        o = {"bits": bits, **self._wanted(want, F, ("eq", "Hs", "He", "slope", "Hest", "status"))}
        if denoise is not None:
            work = self._new((int(self.lib.gf3_demod_workspace_bytes(self._h, F)),), torch.uint8)     # (_split_work(F, True), also for F = 0)
            o["denoise_report"] = self._new((F, 2, 5), torch.float64)
            self._check(self.lib.gf3_demod_frames_dn(
                self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(bits), _ptr(o.get("eq")), _ptr(o.get("Hs")),
                _ptr(o.get("He")), _ptr(o.get("slope")), _ptr(o.get("Hest")), _ptr(o.get("status")),
                _ptr(work), denoise, _ptr(o["denoise_report"]), self._stream()))
            return o
        work, mode = self._split_work(F, split)
        self._check(self.lib.gf3_demod_frames_px(
            self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(bits), _ptr(o.get("eq")), _ptr(o.get("Hs")),
            _ptr(o.get("He")), _ptr(o.get("slope")), _ptr(o.get("Hest")), _ptr(o.get("status")),
            _ptr(work), mode, {None: -1, "fp64": 0, "screen": 1}[precision], self._stream()))
        return o

    def demod_frames_last(self):
        """Of the calling thread's last demod_frames call on the current stream: dict(path = 0 screened | 2 all fp64 | -1 no
        such call, listed_capacity = packets its fp64 pass could take).  No device read."""
        return self._last_call(self.lib.gf3_demod_frames_last, "listed_capacity")

    def debug_rfft32_batch(self, x, offsets):
        """The screened demodulation's fp32 transform alone (tests): [n_sym, N/2+1] complex64 spectra of the N samples
        starting at each offset; f32 / i16 / u8 samples."""
        x = self._samples(x)
        offsets = self._dev(offsets, torch.int64)
        n = offsets.numel()
        out = self._new((n, self.cfg.N // 2 + 1), torch.complex64)
        self._check(self.lib.gf3_debug_rfft_sp_batch(self._h, _ptr(x), x.numel(), _ptr(offsets), n, _ptr(out), self._stream()))
        return out

    def debug_rfft32_pair_batch(self, x, offsets):
        """debug_rfft32_batch through the transform the screened demodulation runs: symbols 2w, 2w + 1 as the two halves of
        one pair transform (tests); same output."""
        x = self._samples(x)
        offsets = self._dev(offsets, torch.int64)
        n = offsets.numel()
        out = self._new((n, self.cfg.N // 2 + 1), torch.complex64)
        self._check(self.lib.gf3_debug_rfft_sp_pair_batch(self._h, _ptr(x), x.numel(), _ptr(offsets), n, _ptr(out), self._stream()))
        return out

    def debug_demod_screen(self, x, frame_offsets):
        """The fp32 screening pass of the QPSK demodulation alone (tests): dict(bits: the screen's own rows, ep32 [F, D, C]
        complex64 -- the rotated fp32 symbols 2 X conj(g) of the data carriers --, E [F, D] float32 -- the bound on
        |ep32 - exact| of each symbol's transform --, cls int32 [F] (0 decided, 1 listed), listed: sorted packet numbers
        the fp64 kernel would be run on)."""
        cfg = self.cfg
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        o = dict(bits=self._new((F, self.bytes_per_frame), torch.uint8),
                 ep32=torch.zeros((F, cfg.D, cfg.C), dtype=torch.complex64, device=self.device),
                 E=torch.zeros((F, cfg.D), dtype=torch.float32, device=self.device),
                 cls=torch.full((F,), -1, dtype=torch.int32, device=self.device))
        work = self._new((int(self.lib.gf3_demod_screen_workspace_bytes(self._h, F)),), torch.uint8)
        self._check(self.lib.gf3_debug_demod_screen(self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(o["bits"]), _ptr(o["ep32"]),
                                                    _ptr(o["E"]), _ptr(o["cls"]), _ptr(work), self._stream()))
        o["listed"] = self._listed(work)
        return o

    def demod_frames_llr(self, x, frame_offsets, weight="csi", want=(), split=None, out=None):
        """Samples to weighted max-log LLRs in one launch (gf3_demod_frames_llr: the fused kernel's soft output mode).
        Returns dict with 'llr' (float32 [F*D*C*mu], the reference's bit order, LLR > 0 <=> bit 0) plus any of 'Hs', 'He',
        'slope', 'status'.  weight: "csi" -- |H^|^2, what demod_frames(want eq, Hs, He) + soft_demap_csi give -- or "none"
        (soft_demap(eq, 1.0)); an int goes to the library as it is.  split: as in demod_frames.  out: optional contiguous
        float32 tensor of F*D*C*mu elements to write into."""
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        if isinstance(weight, str):
            if weight not in ("csi", "none"):
                raise ValueError(f"weight must be 'csi' or 'none', not {weight!r}")
            weight = 1 if weight == "csi" else 0
        llr = self._llr_out(out, F)
        o = {"llr": llr, **self._wanted(want, F, ("Hs", "He", "slope", "status"))}
        work, mode = self._split_work(F, split)
        rc = self.lib.gf3_demod_frames_llr(
            self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(llr), int(weight), _ptr(o.get("Hs")), _ptr(o.get("He")),
            _ptr(o.get("slope")), _ptr(o.get("status")), _ptr(work), mode, self._stream())
        if rc != 0:                                                # (a bad `weight` is the library's to refuse: Gf3Error)
            raise Gf3Error(f"gf3rx error {rc}: {_lib.last_error()}")
        return o

    def demod_plan(self, F, split=None):
        """How demod_frames(F packets, split=...) runs: dict(split: two-phase form or not, Dc: data symbols per workgroup of
        its data stage, chunks: workgroups per packet)."""
        dc, nch = C.c_int32(0), C.c_int32(0)
        two = self.lib.gf3_demod_split_plan(self._h, int(F), 0 if split is None else (2 if split else 1), C.byref(dc), C.byref(nch))
        return dict(split=bool(two), Dc=int(dc.value), chunks=int(nch.value))

    def equalise(self, data, start, end, want=("Hest",)):
        """receiver.equalise on frequency-domain symbols [F,D,K], [F,P,K], [F,P,K]."""
        cfg = self.cfg
        data, start, end = self._dev(data), self._dev(start), self._dev(end)
        F = data.shape[0]
        if tuple(data.shape) != (F, cfg.D, cfg.K) or tuple(start.shape) != (F, cfg.P, cfg.K) or tuple(end.shape) != (F, cfg.P, cfg.K):
            raise ValueError("equalise: shapes must be [F,D,K], [F,P,K], [F,P,K]")
        o = {"eq_all": self._new((F * cfg.D, cfg.K), torch.complex128), "bits": self._new((F, self.bytes_per_frame), torch.uint8),
             **self._wanted(("Hs", "He", "slope") + tuple(want), F, ("Hs", "He", "slope", "Hest"))}
        self._check(self.lib.gf3_equalise(
            self._h, _ptr(data), _ptr(start), _ptr(end), F, _ptr(o["eq_all"]), _ptr(o["Hs"]), _ptr(o["He"]),
            _ptr(o["slope"]), _ptr(o.get("Hest")), _ptr(o["bits"]), self._stream()))
        return o

    def sync_frames(self, x, F, stride, win_lo, win_hi, want_peak=False, out_starts=None, screened=None, work=None):
        """Batched windowed chirp sync: first-pilot sample index per frame (int64, -1 = none).
        out_starts: optional preallocated int64 [F] device tensor to write into.
        screened: None (default): the library decides (gf3_sync_frames_ex mode -1) -- the windows are evaluated in fp32 with
        a proven bound first, in a workspace the library keeps per stream, and the fp64 kernel runs only on the windows the
        bound cannot decide: the all-fp64 indices.  False: the all-fp64 kernel on every window (mode 0).  True: the screen in
        the caller's workspace (mode 1).  work: uint8 workspace of sync_frames_workspace(F) for screened=True (allocated
        here when absent); its first int32 then holds the number of windows that went to fp64.
        want_peak: the fp64 peak VALUES are asked for, so the all-fp64 kernel runs whatever `screened` says (and a `work`
        given reports 0).  sync_frames_last() tells which way a call went."""
        x = self._samples(x)
        starts = self._out(out_starts, (F,), torch.int64, "F", name="out_starts")
        peak = self._new((F,), torch.float64) if want_peak else None
        if screened and work is None:
            work = self.sync_frames_workspace(F)
        if screened and (work.dtype != torch.uint8 or not work.is_contiguous() or not work.is_cuda
                         or work.numel() < int(self.lib.gf3_sync_frames_workspace_bytes(self._h, F))):
            raise ValueError("work must be a contiguous uint8 device tensor of at least sync_frames_workspace(F) bytes")
        mode = -1 if screened is None else (1 if screened else 0)
        self._check(self.lib.gf3_sync_frames_ex(self._h, _ptr(x), x.numel(), F, stride, win_lo, win_hi,
                                                _ptr(starts), _ptr(peak), mode, _ptr(work) if screened else None, self._stream()))
        return (starts, peak) if want_peak else starts

    def sync_frames_last(self):
        """Of the calling thread's last sync_frames call on the current stream: dict(path = 0 screened | 2 all fp64 | -1 no
        such call, unresolved_capacity = windows its fp64 pass could take).  No device read."""
        return self._last_call(self.lib.gf3_sync_frames_last, "unresolved_capacity")

    def sync_frames_workspace(self, F):
        return self._new((int(self.lib.gf3_sync_frames_workspace_bytes(self._h, F)),), torch.uint8)

    def debug_frames_screen(self, x, F, stride, win_lo, win_hi):
        """The fp32 screening pass of the frames sync alone (tests): dict(starts int64 [F] (resolved windows only), y32
        [F, W] float32, err [F] float32 -- the bound on |y32 - exact| --, cls int32 [F] (0 resolved with a detection, 1
        resolved without, 2 unresolved), unresolved: sorted window numbers the fp64 kernel would be run on)."""
        x = self._samples(x)
        W = win_hi - win_lo
        o = dict(starts=torch.full((F,), -7, dtype=torch.int64, device=self.device), y32=self._new((F, W), torch.float32),
                 err=self._new((F,), torch.float32), cls=self._new((F,), torch.int32))
        work = self.sync_frames_workspace(F)
        self._check(self.lib.gf3_debug_frames_screen(self._h, _ptr(x), x.numel(), F, stride, win_lo, win_hi, _ptr(o["starts"]),
                                                     _ptr(o["y32"]), _ptr(o["err"]), _ptr(o["cls"]), _ptr(work), self._stream()))
        o["unresolved"] = self._listed(work)
        return o

    def sync_stream(self, x, cap=None, want_corr=False, mode=None, want_info=False):
        """chirp_method on one stream: indices i with zeros[i] True (int64 tensor).
        mode: how the matched filter is evaluated for THIS call (gf3_sync_stream_ex; None = the engine's default set by
        sync_stream_mode): 0 fp32 screening + fp64 decisions from 2^23 samples on, all-fp64 below; 1 always the all-fp64
        overlap-save; 2 screened at any length; 3 as 2 with the general screening kernel.  want_info adds the call's
        diagnostics dict (as sync_stream_info) to the result.  Nothing of a call is stored in the C context, so several
        threads may run this on one engine, each on its own stream."""
        x = self._samples(x).reshape(-1)
        n = x.numel()
        Lc = self.cfg.chirp_length
        cap = cap or max(4, n // Lc + 4)
        peaks = self._new((cap,), torch.int64)
        ws = int(self.lib.gf3_sync_stream_workspace_bytes(self._h, n))
        work = self._new((ws,), torch.uint8)
        corr = self._new((n + Lc - 1,), torch.float64) if want_corr else None
        cnt = C.c_int64(0)
        info = (C.c_int64 * 4)()
        self._check(self.lib.gf3_sync_stream_ex(self._h, _ptr(x), n, _ptr(peaks), cap, C.byref(cnt), _ptr(work),
                                                _ptr(corr), int(self._sync_mode if mode is None else mode), info, self._stream()))
        peaks = peaks[: cnt.value]
        d = dict(path=int(info[0]), cells=int(info[1]), cells_hit=int(info[2]), candidates=int(info[3]))
        self._tls.sync_info = d
        out = (peaks,) + ((corr,) if want_corr else ()) + ((d,) if want_info else ())
        return out[0] if len(out) == 1 else out

    def sync_stream_mode(self, mode):
        """Default `mode` of sync_stream for this Engine object (a Python-side default: the C context is not touched)."""
        if int(mode) not in (0, 1, 2, 3):
            raise ValueError("sync_stream_mode: mode must be 0 (by length), 1 (fp64 only), 2 (always screen) or 3 (always screen, general kernel)")
        self._sync_mode = int(mode)
        self._check(self.lib.gf3_sync_stream_mode(self._h, int(mode)))      # (keeps debug_stream_screen's kernel choice in step)

    def sync_stream_info(self):
        """Of the calling thread's last sync_stream call: dict(path=0 screened | 1 fp64 after a non-selective screen |
        2 fp64, cells = cells of 14 lags re-evaluated in fp64, cells_hit = those holding a candidate, candidates)."""
        return dict(getattr(self._tls, "sync_info", dict(path=2, cells=0, cells_hit=0, candidates=0)))

    # ------------------------------------------------------------------ self-normalised detection
    @staticmethod
    def check_detect(threshold):
        """ValueError for a detection threshold that is not a finite number inside (0, 1) -> the threshold as a float."""
        number = isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, (bool, np.bool_))
        if not number or not math.isfinite(float(threshold)) or not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"detection threshold must be a finite number inside (0, 1), not {threshold!r}")
        return float(threshold)

    def detect_chunk(self, buf, lag_lo, lag_hi, lag_offset, vrun, threshold=0.3, cap=1024, rho_all=None):
        """gf3_detect_chunk on one buffer (a piece of a stream with Lc - 1 samples of what came before in front): the
        correlation coefficient rho of every owned full-window lag with the chirp, the lags with rho > threshold listed.
        vrun: float64 device tensor of one element, the largest window variance so far (zero before the first piece),
        updated in place.  rho_all: optional float64 [n + Lc - 1] device tensor; rho[g] of every owned lag is written at [g].
        -> (idx int64 [m] = g - 1 + lag_offset, rho float64 [m]), ascending.  ListOverflow (a Gf3Error; .wanted = the
        entries to make room for) when more than `cap` lags are to be listed: nothing was listed, vrun is unchanged."""
        threshold = self.check_detect(threshold)
        buf = self._samples(buf).reshape(-1)
        n = buf.numel()
        idx, rho = self._new((max(cap, 1),), torch.int64), self._new((max(cap, 1),), torch.float64)
        work = self._new((int(self.lib.gf3_detect_chunk_workspace_bytes(self._h, n)),), torch.uint8)
        cnt = C.c_int64(0)
        rc = self.lib.gf3_detect_chunk(self._h, _ptr(buf), n, int(lag_lo), int(lag_hi), int(lag_offset), threshold, _ptr(vrun),
                                       _ptr(idx), _ptr(rho), int(cap), C.byref(cnt), _ptr(rho_all), _ptr(work), self._stream())
        if rc == _lib.GF3_ERANGE:
            raise ListOverflow(f"gf3rx error {rc}: {_lib.last_error()}", int(cnt.value))
        self._check(rc)
        return idx[: cnt.value], rho[: cnt.value]

    def detect_decide(self, idx, rho, final_below=(1 << 62) - 1, cap=None):
        """gf3_detect_decide: the windowed-maximum rule on a list as detect_chunk returns it -> the detections (int64 device
        tensor) whose neighbourhood of Lc - 1 indices to either side lies below `final_below` (the default: the stream has
        ended, INT64_MAX / 2)."""
        idx, rho = self._dev(idx, torch.int64), self._dev(rho, torch.float64)
        m = idx.numel()
        if rho.numel() != m:
            raise ValueError("detect_decide: idx and rho must have the same length")
        cap = cap or max(4, m)
        peaks = self._new((cap,), torch.int64)
        work = self._new((64,), torch.uint8)
        cnt = C.c_int64(0)
        self._check(self.lib.gf3_detect_decide(self._h, _ptr(idx) if m else None, _ptr(rho) if m else None, m, int(final_below),
                                               _ptr(peaks), cap, C.byref(cnt), _ptr(work), self._stream()))
        return peaks[: cnt.value]

    def detect_stream(self, x, threshold=0.3, want_rho=False, want_peak_rho=False):
        """The self-normalised chirp detection on one whole stream, as a single piece: indices i = g - 1 of the detected
        lags (int64 tensor, what sync_stream returns under the reference's rule), with want_rho the coefficient of every
        lag, float64 [n + Lc - 1] (0 on the partial windows at both ends), and with want_peak_rho the coefficients of the
        detections.  A list that overflows is retried once with the reported size; ValueError if it overflows again."""
        threshold = self.check_detect(threshold)
        x = self._samples(x).reshape(-1)
        n, Lc = x.numel(), self.cfg.chirp_length
        rho_all = torch.zeros((n + Lc - 1,), dtype=torch.float64, device=self.device) if want_rho else None
        cap = 64 * (n // Lc + 4)
        for attempt in (0, 1):
            vrun = torch.zeros((1,), dtype=torch.float64, device=self.device)
            try:
                idx, rho = self.detect_chunk(x, 0, n + Lc - 1, 0, vrun, threshold, cap, rho_all)
                break
            except ListOverflow as e:
                if attempt:
                    raise ValueError(f"detect_stream: the list overflowed twice ({e.wanted} lags above the threshold)")
                cap = e.wanted
        peaks = self.detect_decide(idx, rho)
        out = (peaks,) + ((rho_all,) if want_rho else ()) + ((rho[torch.searchsorted(idx, peaks)],) if want_peak_rho else ())
        return out[0] if len(out) == 1 else out

    def debug_stream_screen(self, x):
        """The fp32 screening pass alone (tests): (P32 [n+Lc-1] float32, block maxima, block error bounds, hop)."""
        x = self._samples(x).reshape(-1)
        n = x.numel()
        plen = n + self.cfg.chirp_length - 1
        p32 = self._new((plen,), torch.float32)
        nb_max = plen // 16 + 2                                  # (hop >= 16: more than enough room)
        blk = self._new((2 * nb_max,), torch.float32)
        hop = C.c_int32(0)
        self._check(self.lib.gf3_debug_stream_screen(self._h, _ptr(x), n, _ptr(p32), _ptr(blk), C.byref(hop), self._stream()))
        nblk = -(-plen // hop.value)
        return p32, blk[:nblk], blk[nblk: 2 * nblk], hop.value

    def tx_frames(self, bits_packed, filler, stride=None, gaps=None, out_dtype=torch.float32, tones=None, body_gain=1.0):
        """Synthesise chirp-prefixed packets (transmit side of the reference, OFDM.py:196-259).
        bits_packed: uint8 [F, bytes_per_frame] (the format demod_frames writes); filler: complex [K],
        value of every non-data carrier.  Returns [F, stride] samples: row f =
        [gaps[f] zeros | chirp | P known symbols | D data symbols | P known symbols | zeros].
        tones: complex [F, D, Ku] (tone_reserve) -- the carriers outside data_bins of data symbol (f, l) then carry
        tones[f, l] instead of the filler; pilots and chirp are untouched.  body_gain (finite, > 0) multiplies the x2 of
        the pilot and data symbols, not the chirp.  The defaults are gf3_tx_frames as it always was."""
        bits = self._dev(bits_packed, torch.uint8)
        if bits.dim() != 2 or bits.shape[1] != self.bytes_per_frame:
            raise ValueError("bits_packed must be [F, bytes_per_frame]")
        F = bits.shape[0]
        fill = self._dev(filler)
        if fill.numel() != self.cfg.K:
            raise ValueError("filler must hold K values (one per carrier)")
        stride = stride or self.cfg.frame_len
        g = None if gaps is None else self._dev(gaps, torch.int64)
        if g is not None and F and int(g.max()) + self.cfg.frame_len > stride:
            raise ValueError("gap + packet does not fit the row stride")
        out = self._new((F, stride), out_dtype)
        if tones is None and body_gain == 1.0:
            self._check(self.lib.gf3_tx_frames(self._h, _ptr(bits), _ptr(fill), _ptr(g), F, _ptr(out), stride,
                                               _DT_OF[out_dtype], self._stream()))
            return out
        if tones is not None:
            tones = self._dev(tones)
            if tuple(tones.shape) != (F, self.cfg.D, self.cfg.K - self.cfg.C):
                raise ValueError("tones must be [F, D, Ku] (Ku = K - C, the carriers outside data_bins)")
        self._check(self.lib.gf3_tx_frames_ex(self._h, _ptr(bits), _ptr(fill), _ptr(g), F, _ptr(out), stride,
                                              _DT_OF[out_dtype], _ptr(tones), float(body_gain), self._stream()))
        return out

    @staticmethod
    def check_papr(target_db, tone_limit_db, iterations):
        """ValueError for a peak target that is not a finite number in [3, 13] dB, a tone limit not in [-20, 20] dB or
        iterations that are not an integer in [0, 64] -> (target_db, tone_limit_db, iterations) as float, float, int."""
        def number(x, lo, hi):
            ok = isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))
            return ok and math.isfinite(float(x)) and lo <= float(x) <= hi
        if not number(target_db, 3.0, 13.0):
            raise ValueError(f"papr target must be a finite number of dB in [3, 13], not {target_db!r}")
        if not number(tone_limit_db, -20.0, 20.0):
            raise ValueError(f"papr tone limit must be a finite number of dB in [-20, 20], not {tone_limit_db!r}")
        if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= 64:
            raise ValueError(f"papr iterations must be an integer in [0, 64], not {iterations!r}")
        return float(target_db), float(tone_limit_db), int(iterations)

    def tone_reserve(self, bits_packed, target_db=6.0, tone_limit_db=6.0, iterations=16):
        """Tone reservation (gf3_tone_reserve): for every data symbol of the packets bits_packed (uint8 [F, bytes_per_frame]),
        values for the Ku = K - C carriers outside data_bins -- which no receiver reads in a data symbol -- that lower the
        symbol's peak: `iterations` steps of clip at target_db above the data's rms, project the clipped part on the
        reserved carriers, limit every tone to tone_limit_db (relative to a unit-energy point), and keep the iterate of
        the smallest peak, zero tones included.  -> (tones complex128 [F, D, Ku] for tx_frames(tones=...), report float64
        [F, D, 4] = (peak with zero tones, best peak, its iterate, rms of the best symbol), all before the frame's x2).
        ValueError when there is no reserved carrier.  Fixed reduction order: two calls give identical bytes."""
        target_db, tone_limit_db, iterations = self.check_papr(target_db, tone_limit_db, iterations)
        bits = self._dev(bits_packed, torch.uint8)
        if bits.dim() != 2 or bits.shape[1] != self.bytes_per_frame:
            raise ValueError("bits_packed must be [F, bytes_per_frame]")
        F = bits.shape[0]
        tones = self._new((F, self.cfg.D, self.cfg.K - self.cfg.C), torch.complex128)
        report = self._new((F, self.cfg.D, 4), torch.float64)
        self._check(self.lib.gf3_tone_reserve(self._h, _ptr(bits), F, target_db, tone_limit_db, iterations, _ptr(tones),
                                              _ptr(report), self._stream()))
        return tones, report

    def schmidl_cox(self, x, search_length=None):
        """receiver.schmidlcox_method (OFDM.py:376-387): first arg-max of |P| + N - 1, as a Python int."""
        x = self._samples(x).reshape(-1)
        S = int(5 * self.cfg.fs) if search_length is None else int(search_length)
        out = self._new((1,), torch.int64)
        self._check(self.lib.gf3_schmidl_cox(self._h, _ptr(x), x.numel(), S, _ptr(out), self._stream()))
        return int(out.item())

    def equalise_known_h(self, x, sym_offsets, h):
        """Known-channel zero forcing (Weekend Challenge.ipynb cells 9-17): FFT(rx) / fft(h, N) on the data carriers,
        then demap.  Returns (eq [n_sym, C] complex128, bits [n_sym, C, mu] uint8, idx [n_sym, C] uint8)."""
        x = self._samples(x)
        off = self._dev(sym_offsets, torch.int64)
        taps = self._dev(np.asarray(h, dtype=np.float64), torch.float64)
        n = off.numel()
        eq = self._new((n, self.cfg.C), torch.complex128)
        bits = self._new((n, self.cfg.C, self.cfg.mu), torch.uint8)
        idx = self._new((n, self.cfg.C), torch.uint8)
        work = self._new((int(self.lib.gf3_known_h_workspace_bytes(self._h, n)),), torch.uint8)
        self._check(self.lib.gf3_equalise_known_h(self._h, _ptr(x), x.numel(), _ptr(off), n, _ptr(taps), taps.numel(),
                                                  _ptr(eq), _ptr(bits), _ptr(idx), _ptr(work), self._stream()))
        return eq, bits, idx

    def demap_hard(self, sym):
        sym = self._dev(sym)
        n = sym.numel()
        bits = self._new(tuple(sym.shape) + (self.cfg.mu,), torch.uint8)
        idx = self._new(tuple(sym.shape), torch.uint8)
        self._check(self.lib.gf3_demap_hard(self._h, _ptr(sym), n, _ptr(bits), _ptr(idx), self._stream()))
        return bits, idx

    def soft_demap(self, sym, noise_var, out=None):
        sym = self._dev(sym)
        llr = self._out(out, tuple(sym.shape) + (self.cfg.mu,), torch.float32, "n * mu")
        self._check(self.lib.gf3_soft_demap(self._h, _ptr(sym), sym.numel(), float(noise_var), _ptr(llr), self._stream()))
        return llr

    def soft_demap_csi(self, eq, Hs, He, out=None):
        """Channel-state-weighted max-log LLRs (gf3_soft_demap_csi): maxlog(eq; sigma^2 = 1) * |H^_{f,l,k}|^2 with the
        reference's magnitude model |Hs| + (|He| - |Hs|)(l + P/2)/(D + P), from demod_frames' 'eq' [F*D, C] and 'Hs' /
        'He' [F, K].  -> float32 [F*D*C*mu] in the reference's bit order (packet -> symbol -> carrier -> bit)."""
        cfg = self.cfg
        eq, Hs, He = self._dev(eq), self._dev(Hs), self._dev(He)
        F = Hs.numel() // cfg.K
        if Hs.numel() != F * cfg.K or He.numel() != Hs.numel() or eq.numel() != F * cfg.D * cfg.C:
            raise ValueError("soft_demap_csi: need Hs, He [F, K] and eq [F*D, C]")
        llr = self._llr_out(out, F)
        self._check(self.lib.gf3_soft_demap_csi(self._h, _ptr(eq), _ptr(Hs), _ptr(He), F, _ptr(llr), self._stream()))
        return llr

    def _llr_out(self, out, F):
        return self._out(out, (F * self.cfg.D * self.cfg.C * self.cfg.mu,), torch.float32, "F*D*C*mu")

    def _eq_packets(self, eq, who):
        eq = self._dev(eq)
        per = self.cfg.D * self.cfg.C
        if eq.numel() % per:
            raise ValueError(f"{who}: need eq [F*D, C]")
        return eq, eq.numel() // per

    def noise_estimate(self, eq):
        """Decision-directed per-carrier noise variance of each packet (gf3_noise_estimate): the mean over the packet's D
        data symbols of |eq - nearest constellation point|^2, from demod_frames' 'eq' [F*D, C].  -> float64 [F, C];
        summed in a fixed order, so two calls give identical bits."""
        eq, F = self._eq_packets(eq, "noise_estimate")
        var = self._new((F, self.cfg.C), torch.float64)
        self._check(self.lib.gf3_noise_estimate(self._h, _ptr(eq), F, _ptr(var), self._stream()))
        return var

    def soft_demap_nw(self, eq, var, out=None):
        """Noise-weighted max-log LLRs (gf3_soft_demap_nw): maxlog(eq; sigma^2 = 1) / max(var[f, c], 1e-6 mean_c var[f])
        in one pass over eq [F*D, C] with var [F, C] from noise_estimate; weight 1 for a packet whose mean variance is 0
        or not finite, LLR 0 on a carrier whose variance is not finite.  -> float32 [F*D*C*mu], order and sign as
        soft_demap_csi."""
        eq, F = self._eq_packets(eq, "soft_demap_nw")
        var = self._dev(var, torch.float64)
        if var.numel() != F * self.cfg.C:
            raise ValueError("soft_demap_nw: need var [F, C] for eq [F*D, C]")
        llr = self._llr_out(out, F)
        self._check(self.lib.gf3_soft_demap_nw(self._h, _ptr(eq), _ptr(var), F, _ptr(llr), self._stream()))
        return llr

    # ---- adaptive bit loading (gf3_loading_*) ----
    LOADING_CACHE = 8                           # loading objects an engine keeps at most

    def loading(self, order):
        """The loading object (gf3_loading_create) of a table of per-carrier orders, uint8 [C] of 0 / 2 / 4 / 6 in
        data_bins order: cached by the table's bytes, immutable.  The cache keeps the LOADING_CACHE tables used last (a
        receiver that allocates anew after every probe does not grow): a table beyond that is destroyed once the device
        has finished the work queued on it -- a Loading still held for it is then refused like one of a closed engine --
        and the rest with the engine.  ValueError for a table the library refuses (wrong length, another value, no loaded
        carrier)."""
        if isinstance(order, Loading):
            if order.engine is not self or order.handle is None:
                raise ValueError("the loading belongs to another engine, a closed one, or has left this engine's cache")
            return order
        a = np.ascontiguousarray(order)
        if a.ndim != 1 or a.dtype.kind not in "iub" or (a.size and (a.min() < 0 or a.max() > 255)):
            raise ValueError("a loading is a one-dimensional table of integer orders (0, 2, 4 or 6)")
        a = a.astype(np.uint8)
        key = a.tobytes()
        ld = self._loadings.pop(key, None)
        if ld is not None:
            self._loadings[key] = ld            # (used last)
        else:
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                rc = self.lib.gf3_loading_create(self._h, a.ctypes.data_as(C.c_void_p), len(a), C.byref(h))
            self._check(rc)
            ld = self._loadings[key] = Loading(self, h, a, int(self.lib.gf3_loading_bits(h)))
            while len(self._loadings) > self.LOADING_CACHE:
                old = self._loadings.pop(next(iter(self._loadings)))
                with torch.cuda.device(self.device):
                    torch.cuda.synchronize()    # (kernels in flight may still read its tables)
                self.lib.gf3_loading_destroy(old.handle)
                old.handle = None
        return ld

    def noise_estimate_loaded(self, eq, loading):
        """noise_estimate for a loaded packet (gf3_noise_estimate_loaded): each carrier's residual against its OWN table's
        decision, against the known pilot symbol on a carrier of order 0.  -> float64 [F, C]."""
        ld = self.loading(loading)
        eq, F = self._eq_packets(eq, "noise_estimate_loaded")
        var = self._new((F, self.cfg.C), torch.float64)
        self._check(self.lib.gf3_noise_estimate_loaded(self._h, ld.handle, _ptr(eq), F, _ptr(var), self._stream()))
        return var

    def soft_demap_loaded(self, eq, loading, Hs=None, He=None, var=None, out=None):
        """Max-log LLRs of a loaded packet (gf3_soft_demap_loaded), each carrier by its own table, times the weight the
        arguments choose: var [F, C] (noise_estimate_loaded) -> soft_demap_nw's rule; Hs and He [F, K] -> soft_demap_csi's
        |H^|^2; neither -> 1.  -> float32 [F*D*Bs], Bs = loading.bits, order packet -> symbol -> carrier -> bit; carriers of
        order 0 have no entries."""
        ld = self.loading(loading)
        cfg = self.cfg
        eq, F = self._eq_packets(eq, "soft_demap_loaded")
        if var is not None:
            var = self._dev(var, torch.float64)
            if var.numel() != F * cfg.C:
                raise ValueError("soft_demap_loaded: need var [F, C] for eq [F*D, C]")
        if Hs is not None:
            Hs = self._dev(Hs)
            if Hs.numel() != F * cfg.K:
                raise ValueError("soft_demap_loaded: need Hs [F, K] for eq [F*D, C]")
        if He is not None:
            He = self._dev(He)
            if He.numel() != F * cfg.K:
                raise ValueError("soft_demap_loaded: need He [F, K] for eq [F*D, C]")
        llr = self._out(out, (F * cfg.D * ld.bits,), torch.float32, "F*D*Bs")
        self._check(self.lib.gf3_soft_demap_loaded(self._h, ld.handle, _ptr(eq), _ptr(Hs), _ptr(He), _ptr(var), F, _ptr(llr),
                                                   self._stream()))
        return llr

    @staticmethod
    def _branches(who, xs):
        """One argument per branch -> (list, B): 1 to GF3_MAX_BRANCHES of them."""
        xs = list(xs)
        if not 1 <= len(xs) <= _lib.GF3_MAX_BRANCHES:
            raise ValueError(f"{who}: 1 to {_lib.GF3_MAX_BRANCHES} branches, not {len(xs)}")
        return xs, len(xs)

    def combine_branches(self, eqs, Hs=None, He=None, var=None, out=None, want=("eq", "llr")):
        """Receive diversity (gf3_combine_branches): maximal-ratio combining of B = len(eqs) <= 4 branches' equalised
        symbols, eqs[b] = demod_frames' 'eq' [F*D, C] of recording b of ONE transmission (each synchronised and demodulated
        on its own).  z = sum_b w_b z_b / W, W = sum_b w_b.  Give either Hs and He (B tensors [F, K] each: w_b = the
        |H^|^2 of soft_demap_csi) or var (B tensors [F, C] from noise_estimate: w_b = 1 / max(var_b, 1e-6 vbar), vbar the
        packet's mean variance over all branches and carriers; 1 where vbar is 0 or not finite).  A weight whose input is
        not finite and a symbol that is not finite drop out of both sums (w_b = 0); where every branch does, z = 0 and the
        LLRs are +0.  want: any of "eq" (z, complex128 [F*D, C]), "w" (W, float64 [F*D, C]), "llr" (maxlog(z; 1) W,
        float32 [F*D*C*mu], order and sign as soft_demap_csi).  out: optional dict of tensors to write the wanted entries
        into; out["eq"] must be none of eqs.  -> dict of the wanted entries.  Fixed summation order: two calls give
        identical bytes."""
        cfg = self.cfg
        if (Hs is None) != (He is None):
            raise ValueError("combine_branches: Hs and He go together")
        if (Hs is None) == (var is None):
            raise ValueError("combine_branches: give either Hs and He (csi weights) or var (noise weights), not both or neither")
        eqs, B = self._branches("combine_branches", eqs)
        want = tuple(want)
        if not want or any(k not in ("eq", "w", "llr") for k in want):
            raise ValueError(f"combine_branches: want must name at least one of 'eq', 'w', 'llr', not {want!r}")
        eqs = [self._dev(e) for e in eqs]
        eq0, F = self._eq_packets(eqs[0], "combine_branches")
        if any(e.numel() != eq0.numel() for e in eqs):
            raise ValueError("combine_branches: every branch needs eq [F*D, C] of the same F")
        sides = []
        for name, xs, dtype, per, dim in (("Hs", Hs, torch.complex128, cfg.K, "K"), ("He", He, torch.complex128, cfg.K, "K"),
                                          ("var", var, torch.float64, cfg.C, "C")):
            if xs is None:
                sides.append(None)
                continue
            xs = [self._dev(x, dtype) for x in xs]
            if len(xs) != B:
                raise ValueError(f"combine_branches: {name} holds {len(xs)} branches, eqs {B}")
            if any(x.numel() != F * per for x in xs):
                raise ValueError(f"combine_branches: every {name} must be [F, {dim}] for eq [F*D, C]")
            sides.append(xs)
        out = dict(out or {})
        if any(k not in want for k in out):
            raise ValueError(f"combine_branches: out holds {sorted(out)}, want is {want!r}")
        kinds = {"eq": ((F * cfg.D, cfg.C), torch.complex128, "F*D*C"), "w": ((F * cfg.D, cfg.C), torch.float64, "F*D*C"),
                 "llr": ((F * cfg.D * cfg.C * cfg.mu,), torch.float32, "F*D*C*mu")}
        o = {k: self._out(out.get(k), kinds[k][0], kinds[k][1], kinds[k][2], name=f"combine_branches: out[{k!r}]") for k in want}
        if F and "eq" in o and any(o["eq"].data_ptr() == e.data_ptr() for e in eqs):
            raise ValueError("combine_branches: out['eq'] must be none of eqs (the other branches' sums still read it)")
        mode = _lib.GF3_COMBINE_NOISE if var is not None else _lib.GF3_COMBINE_CSI
        self._check(self.lib.gf3_combine_branches(self._h, B, _table(eqs), mode, _table(sides[0]), _table(sides[1]), _table(sides[2]), F,
                                                  _ptr(o.get("eq")), _ptr(o.get("w")), _ptr(o.get("llr")), self._stream()))
        return o

    def mimo_pilots(self, x, frame_offsets):
        """The two-column pilot estimate of 2 x 2 spatial multiplexing (gf3_mimo_pilots): speaker 1 negates its pilot symbols
        of odd index, so at one microphone cover t = mean_p (-1)^(t p) Y_p / X is its channel from speaker t.
        -> (H complex128 [F, 2 sides, 2 covers, K], status int32 [F]): side 0 is the start block, 1 the end block; cover 0 is
        demod_frames' Hs / He.  status 1 marks a packet whose body leaves the samples at either end; its rows are NaN.
        Needs an even P >= 2 (ValueError).  Fixed summation order: two calls give identical bytes."""
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        H = self._new((F, 2, _lib.GF3_MIMO_STREAMS, self.cfg.K), torch.complex128)
        status = self._new((F,), torch.int32)
        self._check(self.lib.gf3_mimo_pilots(self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(H), _ptr(status), self._stream()))
        return H, status

    def mimo_pilot_noise(self, x, frame_offsets, H):
        """The per-carrier noise variance of one recording of two loudspeakers, measured on the covered pilots
        (gf3_mimo_pilot_noise): with H = mimo_pilots(x, frame_offsets)[0],
        v[f, side, k] = 1 / (P - 2) sum_p |Y_p[k] / X[k] - H[f, side, 0, k] - (-1)^p H[f, side, 1, k]|^2 over the side's P
        pilot symbols -- what the two covers leave of them, so nothing has to be decided.  In the unit of |H|^2: white noise
        of deviation sigma per sample gives N sigma^2.  -> (var float64 [F, 2 sides, K], status int32 [F]); status and the NaN
        rows of a packet that leaves the samples are mimo_pilots' rule.  Needs an even P >= 4 (ValueError: P = 2 leaves no
        degree of freedom).  Fixed summation order: two calls give identical bytes."""
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F = off.numel()
        H = self._dev(H)
        if H.numel() != F * 2 * _lib.GF3_MIMO_STREAMS * self.cfg.K:
            raise ValueError("mimo_pilot_noise: H must be mimo_pilots' [F, 2, 2, K] for the F offsets")
        var = self._new((F, 2, self.cfg.K), torch.float64)
        status = self._new((F,), torch.int32)
        self._check(self.lib.gf3_mimo_pilot_noise(self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(H), _ptr(var), _ptr(status),
                                                  self._stream()))
        return var, status

    def joint_noise_weights(self, vars):
        """The weights of the joint detectors under coloured noise (gf3_joint_noise_weights) from B = len(vars) <= 4
        recordings' mimo_pilot_noise output [F, 2, K]: v_b[f, c] = the mean of the two sides at data carrier c's bin, then
        combine_branches' rule under `var` -- vbar[f] the mean over all branches and data carriers, w = 1 / max(v, 1e-6
        vbar); 1 for the whole packet where vbar is 0 or not finite; 0 where v is not finite.  -> float64 [B, F, C], what
        mimo_detect and stbc_detect take as `weights`.  Fixed summation order: two calls give identical bytes."""
        vars, B = self._branches("joint_noise_weights", vars)
        vars = [self._dev(v, torch.float64) for v in vars]
        per = 2 * self.cfg.K
        if vars[0].numel() % per or any(v.numel() != vars[0].numel() for v in vars):
            raise ValueError("joint_noise_weights: every branch needs var [F, 2, K] of the same F")
        F = vars[0].numel() // per
        w = self._new((B, F, self.cfg.C), torch.float64)
        self._check(self.lib.gf3_joint_noise_weights(self._h, B, _table(vars), F, _ptr(w), self._stream()))
        return w

    def _joint_weights(self, weights, B, F, who):
        """`weights` of the joint detectors -> one contiguous float64 tensor [B, F, C] on the device"""
        w = self._dev(weights, torch.float64)
        if w.numel() != B * F * self.cfg.C:
            raise ValueError(f"{who}: weights must be [B, F, C] for {B} branches of Y [F*D, N/2+1]")
        return w

    def mimo_detect(self, Ys, Hs, slopes, out=None, weights=None):
        """Joint max-log ML detection of the two streams of 2 x 2 spatial multiplexing (gf3_mimo_detect) from B = len(Ys)
        <= 4 recordings: Ys[b] the data symbols' spectra [F*D, N/2+1] as rfft_batch writes them, Hs[b] mimo_pilots' H
        [F, 2, 2, K], slopes[b] demod_frames' slope [F] of recording b.  Per cell the reference's channel model gives the
        B x 2 channel entries; the metric sum_b |y_b - h_b0 x0 - h_b1 x1|^2 is minimised over the 4 x 4 pairs of points.
        A branch whose spectrum value or estimates are not finite at a cell drops out there; where all do, the LLRs are +0.
        -> float32 [F, 2 streams, D, C, mu]: flattened, the coded order of packets 2f, 2f + 1; LLR > 0 <=> bit 0.  out:
        optional contiguous float32 tensor of that many elements.  weights: None, or joint_noise_weights' [B, F, C]
        (gf3_mimo_detect_nw): branch b's term of the metric at carrier c is multiplied by w[b, f, c] -- maximum likelihood
        for noise of variance 1 / w --, and a branch whose weight is 0 drops out there as a non-finite estimate does.
        Needs a table of 4 points with mu = 2 (ValueError)."""
        B, F, Ys, Hs, slopes, llr = self._mimo_detect_args("mimo_detect", Ys, Hs, slopes, out)
        if weights is None:
            self._check(self.lib.gf3_mimo_detect(self._h, B, _table(Ys), _table(Hs), _table(slopes), F, _ptr(llr), self._stream()))
        else:
            w = self._joint_weights(weights, B, F, "mimo_detect")
            self._check(self.lib.gf3_mimo_detect_nw(self._h, B, _table(Ys), _table(Hs), _table(slopes), _ptr(w), F, _ptr(llr),
                                                    self._stream()))
        return llr

    def _mimo_detect_args(self, who, Ys, Hs, slopes, out):
        """What mimo_detect and mimo_detect_known check of their common arguments -> (B, F, the branches' tensors on the
        device, the output [F, 2, D, C, mu])"""
        cfg = self.cfg
        Ys, B = self._branches(who, Ys)
        Hs, slopes = list(Hs), list(slopes)
        if len(Hs) != B or len(slopes) != B:
            raise ValueError(f"{who}: Hs holds {len(Hs)} branches and slopes {len(slopes)}, Ys {B}")
        F, Ys, Hs = self._joint_args(who, Ys, Hs)
        slopes = [self._dev(s, torch.float64) for s in slopes]
        if any(s.numel() != F for s in slopes):
            raise ValueError(f"{who}: every slope must be [F] for Y [F*D, N/2+1]")
        shape = (F, _lib.GF3_MIMO_STREAMS, cfg.D, cfg.C, cfg.mu)
        return B, F, Ys, Hs, slopes, self._out(out, shape, torch.float32, "F*2*D*C*mu", name=f"{who}: out")

    def _joint_args(self, who, Ys, Hs, pairs=False):
        """What both joint detectors check of a context (pairs: the space-time code's geometry as well) and of as many
        spectra as estimates -> (F, both on the device)"""
        cfg = self.cfg
        if cfg.mu != 2 or len(self._re) != 4:
            raise ValueError(f"{who}: the joint detector scans 4 x 4 pairs: a table of 4 points with mu = 2, not {len(self._re)} "
                             f"points with mu = {cfg.mu}")
        if pairs:
            self._stbc_geometry(who)
        Ys = [self._dev(y) for y in Ys]
        per = cfg.D * (cfg.N // 2 + 1)
        if Ys[0].numel() % per:
            raise ValueError(f"{who}: Ys must be [F*D, N/2+1] for whole packets")
        F = Ys[0].numel() // per
        if any(y.numel() != F * per for y in Ys):
            raise ValueError(f"{who}: every branch needs Y [F*D, N/2+1] of the same F")
        Hs = [self._dev(h) for h in Hs]
        if any(h.numel() != F * 4 * cfg.K for h in Hs):
            raise ValueError(f"{who}: every H must be [F, 2, 2, K] " + ("of the same F" if pairs else "for Y [F*D, N/2+1]"))
        return F, Ys, Hs

    def mimo_detect_known(self, Ys, Hs, slopes, bits, known, out=None, weights=None):
        """mimo_detect told what is already known (gf3_mimo_detect_known): `bits` and `known` are uint8 tensors of F*2*D*C*mu
        elements on the engine's device, one byte per coded bit in the layout of the LLRs -- the transmitted order of packets
        2f, 2f + 1.  A non-zero `known` byte: the bit is known, and is 1 where its `bits` byte is non-zero.  The metric,
        the branches' rules and `weights` are mimo_detect's; a pair of points that contradicts a known bit of either
        stream is left out of every minimum.  An unknown bit gets min over the pairs left with it 1 - min with it 0 (+0 where
        no branch is left), a known bit -+GF3_LLR_KNOWN (1e30: finite).  With `known` all zero the bytes are mimo_detect's.
        Everything else -- arguments, output, ValueError -- as mimo_detect."""
        who = "mimo_detect_known"
        B, F, Ys, Hs, slopes, llr = self._mimo_detect_args(who, Ys, Hs, slopes, out)
        for name, plane in (("bits", bits), ("known", known)):
            if (not isinstance(plane, torch.Tensor) or plane.dtype != torch.uint8 or plane.device.type != self.device.type
                    or not plane.is_contiguous() or plane.numel() != llr.numel()):
                raise ValueError(f"{who}: {name} must be a contiguous uint8 tensor of F*2*D*C*mu = {llr.numel()} elements on {self.device}")
        w = None if weights is None else self._joint_weights(weights, B, F, who)
        self._check(self.lib.gf3_mimo_detect_known(self._h, B, _table(Ys), _table(Hs), _table(slopes), _ptr(w), _ptr(bits), _ptr(known),
                                                   F, _ptr(llr), self._stream()))
        return llr

    def _stbc_geometry(self, who):
        """What both calls of transmit diversity refuse of a context: the pilot cover and the pairing of the data symbols."""
        cfg = self.cfg
        if cfg.P < 2 or cfg.P % 2:
            raise ValueError(f"{who}: the two covers need an even number of pilot symbols, P >= 2, not {cfg.P}")
        if cfg.D % 2:
            raise ValueError(f"{who}: the code pairs the data symbols: an even D, not {cfg.D}")

    def stbc_slope(self, Hs):
        """The joint phase slope of transmit diversity (gf3_stbc_slope) from B = len(Hs) <= 4 recordings' mimo_pilots output
        [F, 2, 2, K]: per packet d[k] = sum_b sum_t conj(H_b[f, 0, t, k]) H_b[f, 1, t, k], y = unwrap(angle d), the
        first-degree least-squares coefficient of y over the context's [fit_lo, fit_hi) -- what demod_frames' slope means,
        fitted once on all paths together, so it breaks only where every path has a null.  -> float64 [F]; NaN for a packet
        with a non-finite d in the fit range.  Needs an even P >= 2 and an even D (ValueError).  Fixed summation order: two
        calls give identical bytes."""
        self._stbc_geometry("stbc_slope")
        Hs, B = self._branches("stbc_slope", Hs)
        Hs = [self._dev(h) for h in Hs]
        per = 4 * self.cfg.K
        if Hs[0].numel() % per:
            raise ValueError("stbc_slope: every H must be [F, 2, 2, K]")
        F = Hs[0].numel() // per
        if any(h.numel() != F * per for h in Hs):
            raise ValueError("stbc_slope: every H must be [F, 2, 2, K] of the same F")
        slope = self._new((F,), torch.float64)
        self._check(self.lib.gf3_stbc_slope(self._h, B, _table(Hs), F, _ptr(slope), self._stream()))
        return slope

    def stbc_detect(self, Ys, Hs, slope, out=None, weights=None):
        """Joint max-log ML detection of the Alamouti pairs of transmit diversity (gf3_stbc_detect) from B = len(Ys) <= 4
        recordings: Ys[b] the data symbols' spectra [F*D, N/2+1] as rfft_batch writes them, Hs[b] mimo_pilots' H
        [F, 2, 2, K], slope ONE array [F] for every branch (stbc_slope).  Symbols 2j and 2j + 1 of a packet carry x0, x1 as
        (x0, x1) then (-conj(x1), conj(x0)) on the two speakers; per carrier the statistics of both slots and all branches go
        into mimo_detect's metric over the 4 x 4 pairs of points.  A branch whose spectrum value at either slot or whose
        estimates are not finite drops out of the pair; where all do (or the slope is not finite), the LLRs are +0.
        -> float32 [F, D, C, mu]: flattened, the coded order of one stream; LLR > 0 <=> bit 0.  out: optional contiguous
        float32 tensor of that many elements.  weights: None, or joint_noise_weights' [B, F, C] (gf3_stbc_detect_nw), as
        mimo_detect takes them; both slots of a pair carry the branch's one weight.  Needs a table of 4 points with mu = 2,
        an even P >= 2, an even D (ValueError)."""
        cfg = self.cfg
        Ys, B = self._branches("stbc_detect", Ys)
        Hs = list(Hs)
        if len(Hs) != B:
            raise ValueError(f"stbc_detect: Hs holds {len(Hs)} branches, Ys {B}")
        F, Ys, Hs = self._joint_args("stbc_detect", Ys, Hs, pairs=True)
        slope = self._dev(slope, torch.float64)
        if slope.numel() != F:
            raise ValueError("stbc_detect: the slope must be ONE array [F] for Y [F*D, N/2+1]")
        llr = self._out(out, (F, cfg.D, cfg.C, cfg.mu), torch.float32, "F*D*C*mu", name="stbc_detect: out")
        if weights is None:
            self._check(self.lib.gf3_stbc_detect(self._h, B, _table(Ys), _table(Hs), _ptr(slope), F, _ptr(llr), self._stream()))
        else:
            w = self._joint_weights(weights, B, F, "stbc_detect")
            self._check(self.lib.gf3_stbc_detect_nw(self._h, B, _table(Ys), _table(Hs), _ptr(slope), _ptr(w), F, _ptr(llr),
                                                    self._stream()))
        return llr

    def noise_estimate2(self, eq):
        """Per-carrier AND per-symbol noise variance of each packet from one pass over eq [F*D, C]
        (gf3_noise_estimate_cs): var_c [F, C] is noise_estimate's output bit for bit, var_s [F, D] the mean over the
        carriers of the same residuals.  Fixed summation order: two calls give identical bits."""
        eq, F = self._eq_packets(eq, "noise_estimate2")
        var_c = self._new((F, self.cfg.C), torch.float64)
        var_s = self._new((F, self.cfg.D), torch.float64)
        self._check(self.lib.gf3_noise_estimate_cs(self._h, _ptr(eq), F, _ptr(var_c), _ptr(var_s), self._stream()))
        return var_c, var_s

    def soft_demap_nw2(self, eq, var_c, var_s, deinterleave=False, out=None):
        """Carrier x symbol noise-weighted max-log LLRs (gf3_soft_demap_nw_cs): maxlog(eq; sigma^2 = 1) /
        max(var_c[f, c] var_s[f, l] / vbar[f], 1e-6 vbar[f]), vbar = mean_c var_c; weight 1 for a packet whose vbar is 0
        or not finite, LLR 0 where var_c or var_s is not finite.  deinterleave: write each packet's LLRs in coded order
        (the packet interleaver undone), else in transmitted order.  -> float32 [F*D*C*mu], sign as soft_demap_csi."""
        eq, F = self._eq_packets(eq, "soft_demap_nw2")
        var_c, var_s = self._dev(var_c, torch.float64), self._dev(var_s, torch.float64)
        if var_c.numel() != F * self.cfg.C or var_s.numel() != F * self.cfg.D:
            raise ValueError("soft_demap_nw2: need var_c [F, C] and var_s [F, D] for eq [F*D, C]")
        llr = self._llr_out(out, F)
        self._check(self.lib.gf3_soft_demap_nw_cs(self._h, _ptr(eq), _ptr(var_c), _ptr(var_s), F, int(bool(deinterleave)),
                                                  _ptr(llr), self._stream()))
        return llr

    def track_phase(self, eq, out=None, want_track=False):
        """Per-symbol phase and timing tracking inside each packet (gf3_track_phase): a decision-directed loop with a
        velocity term follows a common phase a and a phase slope b (rad per bin, around the centre of the data bins)
        through the packet's D symbols of eq [F*D, C] and takes them out, out = eq exp(-i (a + b kappa_c)); a symbol whose
        decision-directed error energy exceeds its signal energy (a click, a dropout) coasts.  out: optional contiguous
        complex128 tensor of F*D*C elements to write into; `eq` itself is allowed (in place).  -> out, or with want_track
        (out, phase float64 [F, D, 2] = (a, b) after each symbol, measured uint8 [F, D]).  Fixed summation order: two
        calls give identical bits."""
        eq, F = self._eq_packets(eq, "track_phase")
        cfg = self.cfg
        out = self._out(out, (F * cfg.D, cfg.C), torch.complex128, "F*D*C")
        phase = self._new((F, cfg.D, 2), torch.float64) if want_track else None
        measured = self._new((F, cfg.D), torch.uint8) if want_track else None
        self._check(self.lib.gf3_track_phase(self._h, _ptr(eq), F, _ptr(out), _ptr(phase), _ptr(measured), self._stream()))
        return (out, phase, measured) if want_track else out

    @staticmethod
    def check_feedback_window(half_symbols, half_bins, min_known):
        """ValueError unless half_symbols is an integer in [0, 8], half_bins one in [0, 64] and min_known one >= 1 (the
        ranges of gf3_feedback_equalise) -> the three as ints."""
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not integer(half_symbols) or not 0 <= int(half_symbols) <= 8:
            raise ValueError(f"feedback window: half_symbols must be an integer in [0, 8], not {half_symbols!r}")
        if not integer(half_bins) or not 0 <= int(half_bins) <= 64:
            raise ValueError(f"feedback window: half_bins must be an integer in [0, 64], not {half_bins!r}")
        if not integer(min_known) or int(min_known) < 1 or int(min_known) > 0x7fffffff:
            raise ValueError(f"feedback: min_known must be an integer >= 1, not {min_known!r}")
        return int(half_symbols), int(half_bins), int(min_known)

    def feedback_equalise(self, eq, bits, known, half_symbols=2, half_bins=8, min_known=4, out=None, want_gain=False):
        """Decoder feedback (gf3_feedback_equalise): the residual channel g measured on the KNOWN symbols of eq [F*D, C] --
        those whose mu bytes of `known` are all non-zero, whose value is finite and whose mu `bits` are a label of the
        table -- as sum(eq conj(s)) / sum(|s|^2) over the known symbols within half_symbols symbols and half_bins BINS of
        each symbol (same packet), 1 where fewer than min_known are; out = eq / g.  bits, known: uint8 with F*D*C*mu
        elements, in transmitted order (packet -> symbol -> carrier -> bit: the order of soft_demap_csi's LLRs).  out:
        optional contiguous complex128 tensor of F*D*C elements, NOT eq itself.  -> out, or with want_gain (out, g
        complex128 [F*D, C]).  Fixed summation order: two calls give identical bytes."""
        hs, hb, mk = self.check_feedback_window(half_symbols, half_bins, min_known)
        eq, F = self._eq_packets(eq, "feedback_equalise")
        cfg = self.cfg
        planes = []
        for name, x in (("bits", bits), ("known", known)):
            x = torch.as_tensor(x)
            if x.dtype != torch.uint8 or x.numel() != eq.numel() * cfg.mu:
                raise ValueError(f"feedback_equalise: {name} must be uint8 with F*D*C*mu = {eq.numel() * cfg.mu} elements")
            planes.append(x.to(self.device).contiguous())
        out = self._out(out, (F * cfg.D, cfg.C), torch.complex128, "F*D*C")
        if F and out.data_ptr() == eq.data_ptr():
            raise ValueError("feedback_equalise: out must not be eq (a symbol's neighbours are still being read)")
        gain = self._new((F * cfg.D, cfg.C), torch.complex128) if want_gain else None
        ws = int(self.lib.gf3_feedback_workspace_bytes(self._h, F))
        work = self._new((ws,), torch.uint8) if ws else None
        self._check(self.lib.gf3_feedback_equalise(self._h, _ptr(eq), _ptr(planes[0]), _ptr(planes[1]), F, hs, hb, mk, _ptr(out),
                                                   _ptr(gain), _ptr(work), ws, self._stream()))
        return (out, gain) if want_gain else out

    @staticmethod
    def check_blanking(threshold, guard):
        """ValueError for a blanking threshold that is not a finite number > 0 or a guard that is not an integer in [0, 64]."""
        try:
            ok = math.isfinite(float(threshold)) and float(threshold) > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"blanking threshold must be a finite number > 0, not {threshold!r}")
        if isinstance(guard, bool) or not isinstance(guard, (int, np.integer)) or not 0 <= int(guard) <= 64:
            raise ValueError(f"blanking guard must be an integer in [0, 64], not {guard!r}")
        return float(threshold), int(guard)

    def blank_impulses(self, x, frame_offsets, threshold=4.5, guard=8):
        """Impulse blanking of the samples ahead of the demodulator (gf3_blank_impulses).  Per packet, the symbol at the
        lower quartile of the per-symbol energies of its body (2P + D symbols from frame_offsets[f] on) gives a baseline mu
        and a level sigma; a sample of the body is flagged if it is not finite or |v - mu| > threshold sigma, and every
        sample within `guard` samples of a flagged one of the same body is replaced by mu.  The chirp and the gaps are
        neither read nor written; a packet that runs past the stream is left alone (counts -1).
        -> (out: a copy of x with the blanked samples replaced, counts int32 [F, M] blanked samples per symbol, level
        float64 [F, 2] = (mu, sigma), energy float64 [F, M]).  Fixed summation order: two calls give identical bytes."""
        threshold, guard = self.check_blanking(threshold, guard)
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F, M = off.numel(), self.cfg.M
        out = x.clone()
        counts = self._new((F, M), torch.int32)
        level = self._new((F, 2), torch.float64)
        energy = self._new((F, M), torch.float64)
        self._check(self.lib.gf3_blank_impulses(self._h, _ptr(x), x.numel(), _ptr(off), F, threshold, guard, _ptr(out),
                                                _ptr(energy), _ptr(level), _ptr(counts), self._stream()))
        return out, counts, level, energy

    def resample_frames(self, x, frame_offsets, eps, half_taps=16, out=None):
        """Sampling-clock correction of the packet bodies (gf3_resample_frames): the body of packet f, 2P + D symbols from
        frame_offsets[f] on, is read at the times j / (1 + eps_f) through a Kaiser-windowed sinc of 2 half_taps taps
        (half_taps 16: clean up to 0.74 of Nyquist; 32: up to 0.85).  eps: a Python float for every packet, or a device / host
        array [F]; eps > 0 means this recording's clock took fewer samples than were sent (ppm = 1e6 eps).  out: optional
        contiguous tensor of F * M * S samples in the storage type, not x itself.
        -> (rows [F, M S] in the storage type, offsets int64 [F] = f M S -- what any demodulator call takes next to rows --,
        status int32 [F]: bit 0 the body is not inside the samples (row of zeros), bit 1 eps_f is not finite or beyond 2e-3
        (row copied).)  Two calls give identical bytes."""
        if half_taps not in (16, 32):
            raise ValueError(f"resample_frames: half_taps must be 16 or 32, not {half_taps!r}")
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F, n = off.numel(), self.cfg.M * self.cfg.S
        if isinstance(eps, (int, float, np.floating, np.integer)):
            eps = torch.full((F,), float(eps), dtype=torch.float64, device=self.device)
        else:
            eps = self._dev(eps, torch.float64)
            if eps.numel() != F:
                raise ValueError(f"resample_frames: eps must be a number or hold one value per packet ({F}), not {eps.numel()}")
        rows = self._out(out, (F, n), self.cfg.in_dtype, "F * M * S").reshape(F, n)
        status = self._new((F,), torch.int32)
        self._check(self.lib.gf3_resample_frames(self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(eps), int(half_taps), _ptr(rows),
                                                 _ptr(status), self._stream()))
        return rows, torch.arange(F, dtype=torch.int64, device=self.device) * n, status

    @staticmethod
    def check_window(taper, cp):
        """ValueError unless `taper`, the samples of a receive window's ramp, is an integer (not a bool) in [0, cp] -> the int."""
        if isinstance(taper, (bool, np.bool_)) or not isinstance(taper, (int, np.integer)) or not 0 <= taper <= cp:
            raise ValueError(f"receive_window must be an integer number of samples in [0, cp_length = {cp}], not {taper!r}")
        return int(taper)

    @staticmethod
    def window_ramp(taper):
        """The raised-cosine ramp the receive window takes: r[i] = 0.5 - 0.5 cos(pi (i + 0.5) / L), so r[i] + r[L-1-i] = 1."""
        return 0.5 - 0.5 * np.cos(np.pi * (np.arange(taper, dtype=np.float64) + 0.5) / taper)

    def window_frames(self, x, frame_offsets, taper, out=None):
        """Receive windowing of the packet bodies (gf3_window_frames): in every symbol of packet f, 2P + D symbols from
        frame_offsets[f] on, the last `taper` = L samples fade out by a raised cosine while the L samples one period
        earlier -- the end of the cyclic prefix -- fade in on top of them; every other sample is copied.  Where the prefix
        outlasts the channel by L samples the wanted signal passes unchanged, and what is not periodic in N (a whistle, a
        fan, a neighbour's beep) leaks into the carriers with sidelobes that fall as 1 / distance^3 instead of 1 / distance.
        x may be resample_frames' rows with their offsets.  out: optional contiguous tensor of F * M * S samples in the
        storage type, not x itself.  taper: an integer in [1, CP] (0 is refused: there is nothing to do).
        -> (rows [F, M S] in the storage type, offsets int64 [F] = f M S -- what any demodulator call takes next to rows --,
        status int32 [F]: bit 0 the body is not inside the samples (row of zeros, NaN report), report float64 [F, M, 2]: per
        symbol the squared difference of the two stretches that are blended, summed, and the sum of their squares.)  Two
        calls give identical bytes."""
        taper = self.check_window(taper, self.cfg.CP)
        if taper == 0:
            raise ValueError("window_frames: a taper of 0 samples windows nothing; skip the call")
        x = self._samples(x)
        off = self._dev(frame_offsets, torch.int64)
        F, n = off.numel(), self.cfg.M * self.cfg.S
        ramp = self._dev(self.window_ramp(taper), torch.float64)
        rows = self._out(out, (F, n), self.cfg.in_dtype, "F * M * S").reshape(F, n)
        status = self._new((F,), torch.int32)
        report = self._new((F, self.cfg.M, 2), torch.float64)
        self._check(self.lib.gf3_window_frames(self._h, _ptr(x), x.numel(), _ptr(off), F, _ptr(ramp), taper, _ptr(rows), _ptr(report),
                                               _ptr(status), self._stream()))
        return rows, torch.arange(F, dtype=torch.int64, device=self.device) * n, status, report

    @staticmethod
    def check_ratio(r, half_taps, who="resample_stream"):
        """ValueError unless r is a finite number in [0.25, 4] and half_taps 16 or 32 (what gf3_resample_stream refuses)
        -> (r as a float, half_taps as an int)."""
        if isinstance(half_taps, (bool, np.bool_)) or half_taps not in (16, 32):
            raise ValueError(f"{who}: half_taps must be 16 or 32, not {half_taps!r}")
        number = isinstance(r, (int, float, np.integer, np.floating)) and not isinstance(r, (bool, np.bool_))
        if not number or not 0.25 <= float(r) <= 4.0:       # (NaN fails both comparisons)
            raise ValueError(f"{who}: r must be a finite number of input samples per output sample in [0.25, 4], not {r!r}")
        return float(r), int(half_taps)

    @staticmethod
    def stream_outputs(n_seen, r, half_taps, final=False):
        """How many outputs j = 0, 1, ... of resample_stream are final once n_seen input samples have arrived: those with
        floor((double)j r) + Tw <= n_seen - 1, Tw = ceil(half_taps r) (half_taps where r <= 1).  final=True: the stream has
        ended at n_seen samples -> the whole-recording count, every j with (double)j r <= n_seen - 1.  Integer and double
        arithmetic on the host; no GPU call."""
        r, half_taps = Engine.check_ratio(r, half_taps, "stream_outputs")
        n_seen = int(n_seen)
        if n_seen < 0:
            raise ValueError(f"stream_outputs: n_seen must be >= 0, not {n_seen}")
        reach = 0 if final else (int(math.ceil(half_taps * r)) if r > 1.0 else half_taps)
        last = n_seen - 1 - reach                               # the largest floor(t_j) (final: the largest t_j) that counts
        if last < 0:
            return 0

        def counts(j):                                          # (monotonic in j: the product is rounded monotonically)
            t = float(j) * r
            return t <= last if final else math.floor(t) <= last
        j = int(last / r)
        while counts(j + 1):
            j += 1
        while j >= 0 and not counts(j):
            j -= 1
        return j + 1

    def resample_stream(self, x, r, half_taps=32, in_origin=0, j0=0, n_out=None, out=None):
        """Whole-stream rate conversion (gf3_resample_stream): x, a device tensor (or array) of any of the four storage
        types, holds samples in_origin .. in_origin + len(x) - 1 of a stream taken at r = input_rate / output_rate input
        samples per output sample (0.25 <= r <= 4); outputs j0 .. j0 + n_out - 1 are read at the times j r through a
        Kaiser-windowed sinc of 2 half_taps taps -- widened by r, and low-passing to the output's Nyquist frequency, where
        r > 1 -- with samples outside x read as 0.  Indices are the stream's own, so a stream converted block by block
        (stream_outputs tells how far) gives the bytes of the stream converted whole.  n_out: default the whole-recording
        count of in_origin + len(x) samples, less j0.  out: optional contiguous tensor of n_out samples in the engine's
        storage type, not x itself.  -> n_out samples in the ENGINE's storage type, whatever x's is.  ValueError for what
        the library refuses.  Two calls give identical bytes."""
        r, half_taps = self.check_ratio(r, half_taps)
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not isinstance(x, torch.Tensor) or x.dtype not in _DT_OF:
            raise ValueError("resample_stream: x must be a tensor or array of float64, float32, int16 or uint8 samples")
        x = x.to(self.device).contiguous().reshape(-1)
        in_origin, j0 = int(in_origin), int(j0)
        if n_out is None:
            n_out = max(self.stream_outputs(in_origin + x.numel(), r, half_taps, final=True) - j0, 0) if in_origin >= 0 else 0
        n_out = int(n_out)
        if n_out < 0:
            raise ValueError(f"resample_stream: n_out must be >= 0, not {n_out}")
        y = self._out(out, (n_out,), self.cfg.in_dtype, "n_out").reshape(-1)
        self._check(self.lib.gf3_resample_stream(self._h, _ptr(x) if x.numel() else None, _DT_OF[x.dtype], x.numel(), in_origin, r,
                                                 half_taps, j0, n_out, _ptr(y) if n_out else None, self._stream()))
        return y

    def clock_offset(self, slope):
        """The sampling-clock offset eps a fitted phase slope stands for (demod_frames(want=("slope",))): the slope is the
        phase per carrier index accrued over the (P + D) S samples between the pilot blocks' centres, so
        eps = slope N / (2 pi (P + D) S).  A device expression: nothing is read back."""
        cfg = self.cfg
        return self._dev(slope, torch.float64) * (cfg.N / (2.0 * math.pi * (cfg.P + cfg.D) * cfg.S))

    def interleave(self, x, inverse=False):
        """The packet interleaver on whole packets of nbp = D*C*mu elements (gf3_interleave): x is uint8 or float32 with a
        multiple of nbp elements; coded element i of a packet moves to position (i s) mod nbp, `inverse` moves it back.
        -> a new tensor of x's shape and dtype."""
        x = torch.as_tensor(x)
        if x.dtype not in (torch.uint8, torch.float32):
            raise ValueError("interleave: x must be uint8 or float32")
        x = x.to(self.device).contiguous()
        nbp = self.cfg.D * self.cfg.C * self.cfg.mu
        if x.numel() % nbp:
            raise ValueError(f"interleave: need whole packets of D*C*mu = {nbp} elements")
        out = self._new(tuple(x.shape), x.dtype)
        self._check(self.lib.gf3_interleave(self._h, _ptr(x), _ptr(out), x.numel() // nbp, x.element_size(), int(bool(inverse)),
                                            self._stream()))
        return out

    # ------------------------------------------------------------------ host ingest (streams from host memory / longer than HBM)
    def receive_host(self, samples, chunk_samples=1 << 24, list_cap=None):
        """chirp sync + demodulation (the arithmetic of receiver.receive, OFDM.py:581-603) of a stream that lives in
        HOST memory, piece by piece: pinned, double-buffered H2D copies on a copy stream run under the kernels of the
        previous piece, and the result is that of the one-shot path -- the reference's rule with the GLOBAL maximum
        (OFDM.py:359), the suppression walk, the except-branch, the dropped last detection -- for any stream length.

        How the global rule survives the cut (gf3_sync_chunk / gf3_sync_decide, include/gf3rx.h): every piece folds its
        lags into a running maximum and keeps the few lags that could still pass 0.4 x the FINAL maximum (which can
        only be larger), with their raw fp64 values.  After each piece the rule is applied provisionally with the
        maximum so far and the packets whose samples are resident are demodulated; at the end it is applied once more
        with the final maximum, and only where that changes the detections (a later piece raised the maximum enough to
        kill an earlier candidate, or un-suppressed one) are packets looked at again -- their samples re-read from the
        host array.  Pieces overlap by Lc + one packet, so no chirp and no packet is cut.

        samples: 1-D numpy array or CPU torch tensor.  A pinned tensor is copied from directly.  Pageable memory of 128 MiB
        and more goes to the runtime in equal pieces of at least 128 MiB (which it pins on the fly: the DMA rate; a copy
        thread makes these blocking copies under the previous piece's kernels); less than that is staged through THREE
        pinned buffers by a host copy per piece that a background thread makes two pieces ahead of the kernels: under piece
        c's kernels and piece c+1's DMA, piece c+2 is being staged -- into the buffer piece c-1 was copied from, which is
        idle by then, so that thread makes no HIP call at all.  (Until round 4 a pageable array could also be registered
        with the driver -- hipHostRegister -- for the duration of the call.  Registering and releasing ordinary process
        memory over and over was followed, in this package's own test runs, by GPU memory faults in unrelated kernels
        later in the process, and the default is as fast now: removed)  chunk_samples: new samples per piece
        (raised to two packets if smaller).  Returns dict(peaks int64 [n_det] (device), bits uint8 [n_det - 1,
        bytes_per_frame] (device, packed), info).  Raises ValueError where the reference fails (fewer than two detections;
        a packet that runs past the end of the stream)."""
        return ingest.receive(self, samples, chunk_samples, list_cap)

    def release_host_buffers(self):
        """Drop the calling thread's cached ingest resources (device buffers, workspace, pinned staging, copy stream):
        receive_host keeps them between calls so that a receiver fed one recording after another does not allocate."""
        ingest.release(self)

    # ------------------------------------------------------------------ PS + decode (OFDM.py:504-505, 541-544)
    def unpack_decode(self, packed, mask_bits=None, to_host=True):
        """[F, bytes_per_frame] packed decisions -> the int64 0/1 array receiver.receive returns (packet -> symbol ->
        carrier -> bit), XORed with tile(mask_bits)[:len] when a whitening mask is given.  to_host: the kernel writes
        straight into pinned host memory (gf3_unpack_bits) and a torch CPU tensor over that memory is returned -- valid
        once the stream has been synchronised; else a device tensor."""
        packed = packed.contiguous()
        F = packed.shape[0]
        n = F * self.cfg.bits_per_frame
        mask = None
        if mask_bits is not None:
            key = bytes(np.asarray(mask_bits, dtype=np.uint8))
            cached = getattr(self, "_mask_cache", None)
            if cached is None or cached[0] != key:
                cached = self._mask_cache = (key, torch.from_numpy(np.frombuffer(key, dtype=np.uint8).copy()).to(self.device))
            mask = cached[1]
        out = torch.empty(n, dtype=torch.int64, pin_memory=True) if to_host else self._new((n,), torch.int64)
        self._check(self.lib.gf3_unpack_bits(self._h, _ptr(packed), F, _ptr(mask), 0 if mask is None else mask.numel(),
                                             C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ------------------------------------------------------------------ bit helpers (layout only)
    def unpack_bits(self, packed):
        """[F, bytes_per_frame] uint8 -> [F * D*C*mu] uint8 0/1 (np.unpackbits order), on device."""
        sh = torch.arange(7, -1, -1, device=packed.device, dtype=torch.uint8)
        b = (packed.unsqueeze(-1) >> sh) & 1
        return b.reshape(packed.shape[0], -1)[:, : self.cfg.bits_per_frame].reshape(-1)
