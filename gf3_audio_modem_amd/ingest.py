"""Host ingest (Engine.receive_host): the plan of the pieces, one upload pipeline over one of three sources,
the reference's global-maximum rule across the pieces, and the rows of packed bits."""
import ctypes as C
import time
import warnings
from concurrent.futures import ThreadPoolExecutor, wait

import numpy as np
import torch

from . import _lib

DIRECT_PIECE_BYTES = 128 << 20      # from this size on the runtime pins a pageable source on the fly (its GPU_PINNED_MIN_XFER_SIZE)
PINNED, RUNTIME, STAGED = "pinned", "pageable, copied by the runtime in large pieces", "pageable, staged"


def host_pieces(n, chunk_samples, Lc, L):
    """How Engine.receive_host cuts a stream of n samples (chirp length Lc, packet body L = M*S samples): a list of
    pieces, each dict(lo, hi: the NEW samples [lo, hi) it brings; base: stream index of the first sample of its device
    buffer, which starts with the last `carry` = Lc + L + 8 samples of the previous piece; n_buf; g_lo, g_hi: the lags
    [g_lo, g_hi) of the stream's full convolution P (length n + Lc - 1) it owns).  Every lag 1 .. n+Lc-3 -- the p1 of
    every zeros-index of OFDM.py:360 -- is owned by exactly one piece, with its Lc taps and both neighbours inside that
    piece's buffer (or beyond the stream's true ends, where the convolution's zero extension is the reference's own).
    Pure arithmetic: tested on the CPU (tests/test_abi_cpu.py)."""
    carry = Lc + L + 8
    H = max(int(chunk_samples), 2 * carry)
    k = -(-n // H)
    plen = n + Lc - 1
    out = []
    for c in range(k):
        lo, hi = c * H, min(n, (c + 1) * H)
        ce = min(carry, lo)
        out.append(dict(lo=lo, hi=hi, base=lo - ce, n_buf=ce + hi - lo, g_lo=1 if c == 0 else lo - 1,
                        g_hi=plen - 1 if c == k - 1 else hi - 1))
    return out, H, carry


def plan(n, itemsize, pinned, chunk_samples, Lc, L):
    """-> (source: PINNED, RUNTIME or STAGED; pieces, H, carry as host_pieces).  Pageable memory, a large stream: pieces of
    at least 128 MiB, copied by the runtime itself.  From that size on a plain copy from pageable memory is pinned by the
    runtime on the fly and runs at the DMA rate (55 GB/s measured; below it, it is staged at 13-15 GB/s) -- the path every
    large host-to-device copy of every program takes.  Smaller pageable streams are staged.  Tested on the CPU."""
    if pinned:
        source = PINNED
    elif n * itemsize >= DIRECT_PIECE_BYTES + 65536:
        source = RUNTIME
        min_piece = -(-(DIRECT_PIECE_BYTES + 65536) // itemsize)
        k = max(1, min(n // min_piece, -(-n // max(int(chunk_samples), 1))))     # equal pieces, none below the threshold,
        chunk_samples = -(-n // k)                                                # no more of them than were asked for
    else:
        source = STAGED
    return (source,) + host_pieces(n, chunk_samples, Lc, L)


class _Cache:
    """One host thread's ingest resources, kept between calls so that a receiver fed one recording after another does not
    allocate: a buffer is handed out as a slice while it is large enough, and replaced when it is not."""

    def __init__(self, dev):
        self.dev, self.tensors, self.pools = dev, {}, {}
        # (HIGH priority: the runtime multiplexes streams of one priority onto a handful of hardware queues, and a copy
        #  stream on the compute stream's queue serialises the upload of piece c+1 behind the kernels of piece c)
        self.copier = torch.cuda.Stream(dev, priority=-1)
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]             # per device buffer: its upload has landed

    def take(self, name, numel, dtype, pinned=False):
        t = self.tensors.get(name)
        if t is None or t.numel() < numel:
            t = self.tensors[name] = torch.empty(numel, dtype=dtype, **({"pin_memory": True} if pinned else {"device": self.dev}))
        return t[:numel]

    def pool(self, name, workers):
        if name not in self.pools:
            self.pools[name] = ThreadPoolExecutor(workers)
        return self.pools[name]


def release(eng):
    """Drop the calling thread's cache and shut its executors down."""
    cache = getattr(eng._tls, "ingest", None)
    eng._tls.ingest = None
    for p in cache.pools.values() if cache else ():
        p.shutdown(wait=True)


class _Pinned:
    """A pinned source, read in place by the DMA engine.  Every source: start(c) makes piece c ready early, upload(c, dst,
    ev) issues its copy into a device buffer on the copy stream and records ev, wait(c) waits for that on the calling
    thread, drain() waits for whatever still runs."""
    non_blocking = True

    def __init__(self, x, pieces, cache):
        self.x, self.pieces, self.cache, self.futs = x, pieces, cache, {}

    def new(self, c):
        return self.x[self.pieces[c]["lo"]: self.pieces[c]["hi"]]

    def start(self, c): pass
    def wait(self, c): pass

    def upload(self, c, dst, ev, src=None):
        with torch.cuda.stream(self.cache.copier):
            dst.copy_(self.new(c) if src is None else src, non_blocking=self.non_blocking)
            ev.record(self.cache.copier)

    def drain(self):
        wait(list(self.futs.values()))


class _RuntimeCopied(_Pinned):
    """Pageable, a large stream: the copy blocks its caller while the runtime pins and transfers the piece, so it is made on
    the copy thread, under the previous piece's kernels (the copy stream's wait for the buffer was enqueued before)."""
    non_blocking = False

    def upload(self, c, dst, ev):
        self.futs[c] = self.cache.pool("copy", 1).submit(super().upload, c, dst, ev)

    def wait(self, c):
        self.futs.pop(c).result()


class _Staged(_Pinned):
    """Pageable, a small stream: staged through THREE pinned buffers by a host copy per piece that a background thread
    makes two pieces ahead: piece c + 2 is staged under piece c's kernels and piece c + 1's DMA, into the buffer piece
    c - 1 was copied from -- idle, as the calling thread has synchronised on piece c - 1's kernels, which waited for that
    DMA, before it submits this.  So that thread makes no HIP call at all."""

    def __init__(self, x, pieces, cache):
        super().__init__(x, pieces, cache)
        self.stage = [cache.take(f"stage{i}", pieces[0]["hi"] - pieces[0]["lo"], x.dtype, pinned=True) for i in range(min(3, len(pieces)))]
        self.stager, self.threads = cache.pool("stager", 1), cache.pool("stage copy", 4)

    def _stage(self, c):
        src = self.new(c)
        m, dst = src.numel(), self.stage[c % 3][: src.numel()]
        if m >= (1 << 22):                                                  # four host threads: 24 GB/s on the GPU box against 4 GB/s for one
            q = -(-m // 4)
            list(self.threads.map(lambda k: dst[k * q: (k + 1) * q].copy_(src[k * q: (k + 1) * q]), range(4)))
        else:
            dst.copy_(src)

    def start(self, c):
        self.futs[c] = self.stager.submit(self._stage, c)

    def upload(self, c, dst, ev):
        self.futs.pop(c).result()
        super().upload(c, dst, ev, self.stage[c % 3][: dst.numel()])


SOURCES = {PINNED: _Pinned, RUNTIME: _RuntimeCopied, STAGED: _Staged}


class _Rule:
    """The reference's rule with the GLOBAL maximum (OFDM.py:359) across the pieces (gf3_sync_chunk / gf3_sync_decide,
    include/gf3rx.h): each piece folds its lags into a running maximum and appends its segment of the kept-lag list, the
    lags that could still pass thresh x the final maximum with their raw fp64 values; a piece whose segment does not fit
    keeps only its own maximum, which at the end decides whether it is looked at again."""

    def __init__(self, eng, cache, nbuf, cap_list, cap_peaks):
        self.eng, self.cache, self.cap = eng, cache, cap_list
        self.run_max = torch.full((2,), float("-inf"), dtype=torch.float64, device=eng.device)   # [maximum so far, the last piece's own]
        self.idx = cache.take("list idx", cap_list, torch.int64)
        self.val = cache.take("list val", 3 * cap_list, torch.float64).view(cap_list, 3)
        self.work = cache.take("chunk work", int(eng.lib.gf3_sync_chunk_workspace_bytes(eng._h, nbuf)), torch.uint8)
        self.dwork = cache.take("decide work", int(eng.lib.gf3_sync_decide_workspace_bytes(eng._h, cap_list)), torch.uint8)
        self.peaks = cache.take("peaks", cap_peaks, torch.int64)
        self.segs, self.overflow, self.listed, self.full_pieces, self.below = [], [], 0, 0, 0

    def _chunk(self, buf, q, idx, val, cap):
        """-> (entries listed, None when they do not fit; the piece's own maximum)"""
        eng, cnt, pmax = self.eng, C.c_int64(0), C.c_double(0.0)
        rc = eng.lib.gf3_sync_chunk(eng._h, _lib.ptr(buf), buf.numel(), q["g_lo"] - q["base"], q["g_hi"] - q["base"], q["base"],
                                    _lib.ptr(self.run_max), _lib.ptr(idx), _lib.ptr(val), cap, C.byref(cnt), C.byref(pmax),
                                    _lib.ptr(self.work), eng._stream())
        if rc == _lib.GF3_ERANGE:
            return None, pmax.value
        eng._check(rc)
        return int(cnt.value), pmax.value

    def add(self, c, buf, q):
        room = self.cap - self.listed                   # (a full list: the piece can only report that it overflows, or keep nothing)
        self.full_pieces += int(room == 0)
        got, pmax = self._chunk(buf, q, self.idx[self.listed:] if room else None, self.val[self.listed:] if room else None, room)
        if got is None:
            # no positive maximum yet (leading silence), or one so small that most lags of this piece stay above 0.4 x it
            # (leading noise): nothing is kept of the piece but its own maximum
            self.overflow.append((c, pmax))
            got = 0
        self.segs.append((self.listed, got))
        self.listed += got

    def decide(self, nz, idx=None, val=None):
        """the rule with the maximum so far, on the kept list or on (idx, val); nz: the stream's last lag (1 << 62: not yet known)"""
        eng, cnt = self.eng, C.c_int64(0)
        idx, val, k = (self.idx, self.val, self.listed) if idx is None else (idx, val, idx.numel())
        if k > self.cap:                                # (the merged list of the final pass can be longer)
            self.dwork = self.cache.take("decide work", int(eng.lib.gf3_sync_decide_workspace_bytes(eng._h, k)), torch.uint8)
        eng._check(eng.lib.gf3_sync_decide(eng._h, _lib.ptr(idx), _lib.ptr(val), k, _lib.ptr(self.run_max), nz, _lib.ptr(self.peaks),
                                           self.peaks.numel(), C.byref(cnt), _lib.ptr(self.dwork), eng._stream()))
        return self.peaks[: cnt.value].cpu().numpy()

    def final(self, x, pieces, buf0, nz):
        """The maximum M is final: an overflowed piece whose own maximum can reach thresh x M is copied again (into buf0)
        and listed in full, the segments are merged in stream order, and the rule runs once more.  -> (peaks, pieces
        looked at again)"""
        M = self.M = float(self.run_max[0].item())
        extra, scratch = {}, None
        for c, pmax in self.overflow:
            if np.isfinite(M) and M > 0.0 and pmax < self.eng.cfg.thresh * M * (1.0 - 1e-6):
                self.below += 1                         # no lag of that piece can pass thresh x M: nothing to look at
                continue
            q = pieces[c]
            buf = buf0[: q["n_buf"]]
            buf.copy_(x[q["base"]: q["hi"]])             # (second look: a plain synchronous copy)
            k = q["g_hi"] - q["g_lo"]
            if scratch is None or scratch[0].numel() < k:    # one scratch pair for every piece looked at again
                scratch = (torch.empty(k, dtype=torch.int64, device=buf.device), torch.empty((k, 3), dtype=torch.float64, device=buf.device))
            got, _ = self._chunk(buf, q, scratch[0], scratch[1], k)
            extra[c] = (scratch[0][:got].clone(), scratch[1][:got].clone())   # (what is kept is what was listed, not k x 32 B)
        if not self.overflow:
            return self.decide(nz), []
        parts = [extra.get(c, (self.idx[s0: s0 + k], self.val[s0: s0 + k])) for c, (s0, k) in enumerate(self.segs)]
        return self.decide(nz, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), list(extra)


class _Rows:
    """Packed bits, one row per demodulated detection (row_of: zeros-index -> row; provisional detections that are
    dropped later use rows too)."""

    def __init__(self, eng, cache, cap):
        self.eng, self.row_of = eng, {}
        self.rows = cache.take("rows", cap * eng.bytes_per_frame, torch.uint8).view(cap, eng.bytes_per_frame)

    def demod(self, buf, starts, dets):
        """the packets of the detections `dets`, at the offsets `starts` of buf -> the next free rows"""
        r0, m = len(self.row_of), len(dets)
        if r0 + m > self.rows.shape[0]:
            self.rows = torch.cat([self.rows, self.rows.new_empty((max(m, self.rows.shape[0]), self.rows.shape[1]))])
        self.eng.demod_frames(buf, starts, out_bits=self.rows[r0: r0 + m])
        self.row_of.update((i, r0 + j) for j, i in enumerate(dets))


def _host_tensor(samples, dtype):
    if isinstance(samples, torch.Tensor):
        if samples.is_cuda:
            raise ValueError("receive_host takes host memory; use sync_stream / demod_frames for device tensors")
        x = samples.reshape(-1)
        return x if x.dtype == dtype else x.to(dtype)
    b = np.ascontiguousarray(np.asarray(samples).reshape(-1), dtype=torch.empty(0, dtype=dtype).numpy().dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # (torch warns when it wraps a non-writable array; it is only read)
        return torch.from_numpy(b)


def _run_pieces(eng, src, pieces, bufs, carry, rule, rows, L):
    """The upload of piece c + 1 runs under piece c's kernels, into the other device buffer once the main stream is done
    with it; a buffer starts with the carry, copied device to device from the previous piece's."""
    main, copier, copied = torch.cuda.current_stream(eng.device), src.cache.copier, src.cache.copied

    def upload(c):
        src.upload(c, bufs[c % 2][carry: carry + pieces[c]["hi"] - pieces[c]["lo"]], copied[c % 2])

    copier.wait_stream(main)                            # (a previous call's consumers of these buffers are ordered before the new copies)
    for c in range(min(2, len(pieces))):
        src.start(c)
    upload(0)
    for c, q in enumerate(pieces):
        b, ce = c % 2, q["lo"] - q["base"]
        src.wait(c)
        main.wait_event(copied[b])
        if ce:                                          # (the previous piece's last `ce` new samples end its buffer)
            end = carry + pieces[c - 1]["hi"] - pieces[c - 1]["lo"]
            bufs[b][carry - ce: carry].copy_(bufs[1 - b][end - ce: end])
        if c + 1 < len(pieces):
            order = torch.cuda.Event()
            order.record(main)                          # the other buffer is free once this point is reached
            copier.wait_event(order)
            upload(c + 1)
        if c + 2 < len(pieces):
            src.start(c + 2)
        buf = bufs[b][carry - ce: carry + q["hi"] - q["lo"]]
        rule.add(c, buf, q)
        # provisional decision with the maximum so far (a piece that kept nothing is simply not represented: whatever
        # that gets wrong is put right at the end), then the packets whose samples are resident
        pk = rule.decide(1 << 62)
        k0 = int(np.searchsorted(pk, q["base"] - 2))   # (detections before this buffer were handled, or wait for the end)
        ready = [int(i) for i in pk[k0:] if int(i) + 2 + L <= q["hi"] and int(i) not in rows.row_of]
        if ready:
            rows.demod(buf, [i + 2 - q["base"] for i in ready], ready)


def receive(eng, samples, chunk_samples, list_cap):
    t_start = time.perf_counter()
    cfg, dev = eng.cfg, eng.device
    x = _host_tensor(samples, cfg.in_dtype)
    n, Lc, L, pinned = x.numel(), cfg.chirp_length, cfg.M * cfg.S, x.is_pinned()
    if n < 3:
        raise ValueError("stream too short")
    source, pieces, H, carry = plan(n, x.element_size(), pinned, chunk_samples, Lc, L)
    cache = eng._tls.ingest = getattr(eng._tls, "ingest", None) or _Cache(dev)
    nbuf = carry + min(H, n)
    bufs = [cache.take(f"buf{b}", nbuf, cfg.in_dtype) for b in range(min(2, len(pieces)))]
    rule = _Rule(eng, cache, nbuf, int(list_cap or max(4096, 64 * (n // Lc + 2))), n // Lc + 8)
    rows, src = _Rows(eng, cache, n // Lc + 8), SOURCES[source](x, pieces, cache)
    t_setup = time.perf_counter() - t_start             # (pinned staging, device buffers, workspace: cached after the first call)
    ok = False
    try:
        _run_pieces(eng, src, pieces, bufs, carry, rule, rows, L)
        t_pieces = time.perf_counter() - t_start - t_setup
        peaks, again = rule.final(x, pieces, bufs[0], n + Lc - 3)
        if len(peaks) < 2:
            raise ValueError("need at least one array to concatenate")      # np.vstack([]) in get_symbols (OFDM.py:400)
        det = [int(i) for i in peaks[:-1]]                                 # the last detection is always dropped (OFDM.py:395)
        missing = [i for i in det if i not in rows.row_of]
        if any(i + 2 + L > n for i in missing):
            raise ValueError("packet runs past the end of the stream")
        dropped = len(set(rows.row_of) - set(int(i) for i in peaks))      # (accepted with an earlier maximum, rejected by the final one)
        for k0 in range(0, len(missing), 64):                              # second look at single packets: samples re-read from the host
            grp = missing[k0: k0 + 64]
            rows.demod(torch.stack([x[i + 2: i + 2 + L] for i in grp]).to(dev).reshape(-1), [j * L for j in range(len(grp))], grp)
        bits = rows.rows[torch.tensor([rows.row_of[i] for i in det], dtype=torch.int64, device=dev)]
        torch.cuda.synchronize(dev)
        ok = True
    finally:
        src.drain()                                     # (host copies still running when the call failed)
        if not ok:
            torch.cuda.synchronize(dev)                 # nothing of the call is in flight when its buffers are reused
    info = dict(chunks=len(pieces), chunk_samples=H, overlap_samples=carry, pinned_input=pinned, source=source,
                h2d_bytes=(n + sum(pieces[c]["n_buf"] for c in again) + len(missing) * L) * x.element_size(),
                second_look_chunks=len(again), second_look_packets=len(missing), provisional_detections_dropped=dropped,
                full_list_pieces=rule.full_pieces, setup_seconds=t_setup, pieces_seconds=t_pieces, listed=rule.listed)
    if rule.below:
        info["overflow_pieces_below_threshold"] = rule.below
    info.update(seconds=time.perf_counter() - t_start, max=rule.M)
    return dict(peaks=torch.from_numpy(peaks).to(dev), bits=bits, info=info)
