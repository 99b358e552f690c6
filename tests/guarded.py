"""Guard bands around every array of one ABI call (plain Python on tensors; no fixtures, no GPU needed to import).

One array is one uint8 allocation of GUARD + skew + nbytes + GUARD bytes; the call sees the contiguous typed view at byte
GUARD + skew.  skew is 0 or one element of the array's type (what `x[1:]` of a tensor gives), or `align` bytes where the
header demands an alignment above the element's; a workspace is skewed by WORK_ALIGN bytes.  No pointer is ever below its
type's alignment, no count larger than its array: a violation shows as a changed byte, it is not provoked as a fault.
The same call is dressed twice and run a third time on plain tensors:

    dressing A   bands and `out` / `work` interiors all-ones bytes (NaN in every float type, -1, 0xFF)
    dressing B   bands 0x00, `out` / `work` interiors 0x5A
    plain        torch tensors of the array's own size, `out` interiors 0xC3

and next to an integer SAMPLE array the bands hold the type's extreme values, of opposite signs in A and B, so that a
sample read outside the array changes a sum instead of hiding in it.

`Arrays.check()` holds every band byte and every `in_` byte to its snapshot and every documented not-written element
(`keep`) to its pre-fill; `compare()` holds every other element of every `out` / `inout` array, and every host-side result,
to be bit-for-bit the same in all three runs.  An element the call forgot to write, or one that depends on memory outside
the arrays, differs between the dressings.  Every failure names the array and the byte offset from the view's first byte
(negative: in the band in front)."""
import numpy as np
import torch

GUARD = 65536
WORK_ALIGN = 16                         # what a workspace is owed: the alignment of the widest type carved out of it (complex128)
DRESSINGS = ("A", "B", None)
_BAND = {"A": 0xFF, "B": 0x00}
_FILL = {"A": 0xFF, "B": 0x5A, None: 0xC3}
_EXTREME = {torch.int16: {"A": 32767, "B": -32768}, torch.uint8: {"A": 255, "B": 0}}


class Violation(AssertionError):
    pass


def _tensor(values):
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().contiguous()
    return torch.from_numpy(np.ascontiguousarray(values))


def _bytes(t):
    """The bytes of a contiguous tensor as a flat uint8 tensor (bit patterns: NaNs compare as what they hold)."""
    return t.contiguous().reshape(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8, device=t.device)


def _first(mask):
    return int(torch.nonzero(mask.reshape(-1))[0, 0])


class Arrays:
    """The arrays of one run of one call.  dressing "A", "B" or None (plain tensors, no bands, no skew)."""

    def __init__(self, dressing, skew=False, device="cpu"):
        assert dressing in DRESSINGS
        self.dressing, self.skew, self.device = dressing, bool(skew) and dressing is not None, torch.device(device)
        self.items, self.host = {}, {}

    # ---- roles
    def in_(self, name, values, samples=False, align=0):
        """Values given, never to change."""
        return self._make(name, "in", _tensor(values), None, samples, align)

    def out(self, name, shape, dtype, align=0):
        """Interior pre-filled by the harness; every element is to be written unless keep() names it."""
        return self._make(name, "out", None, (tuple(int(s) for s in np.atleast_1d(shape)), dtype), False, align)

    def inout(self, name, values, samples=False, align=0):
        """Values given, rewritten in place; keep() names the elements that stay."""
        return self._make(name, "inout", _tensor(values), None, samples, align)

    def work(self, name, nbytes, align=0):
        """A workspace of exactly nbytes bytes: only its bands are looked at.  It is a `void *` that the library carves
        doubles, int64 and complex128 arrays out of, so its own type's alignment is theirs: the skew is WORK_ALIGN bytes,
        never one (a count word off its alignment is read by a wave-uniform load from the rounded-down address)."""
        return self._make(name, "work", None, ((int(nbytes),), torch.uint8), False, max(int(align), WORK_ALIGN))

    def keep(self, name, mask):
        """The elements of an out / inout array the header says are NOT written (bool array of the view's shape, or
        anything that indexes one): they must still hold the pre-fill (out) or the values given (inout)."""
        it = self.items[name]
        assert it["role"] in ("out", "inout"), name
        m = np.zeros(tuple(it["view"].shape), dtype=bool)
        m[mask] = True
        it["keep"] |= m

    def keep_all(self):
        """Nothing is written at all (F == 0, a refusal): every out / inout array keeps every element."""
        for name, it in self.items.items():
            if it["role"] in ("out", "inout"):
                self.keep(name, np.s_[...])

    def unspecified(self, name, mask):
        """Elements of an out array whose content after the call the header leaves open (a workspace behind its count word,
        a list after GF3_ERANGE): neither compared nor held; the bands around the array still are."""
        it = self.items[name]
        assert it["role"] == "out", name
        it["open"][mask] = True

    def result(self, name, value):
        """A host-side result of the call (return code, count): compared between the runs."""
        self.host[name] = value

    # ---- construction
    def _make(self, name, role, values, spec, samples, align):
        assert name not in self.items, name
        shape, dtype = (tuple(values.shape), values.dtype) if values is not None else spec
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        if self.dressing is None:
            whole, lo = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device), 0      # (never a null address)
        else:
            lo = GUARD + (max(item, int(align)) if self.skew else 0)
            assert GUARD % item == 0 and lo % item == 0 and (not align or lo % align == 0)
            whole = torch.empty(lo + nbytes + GUARD, dtype=torch.uint8, device=self.device)
            if samples and dtype in _EXTREME:
                whole.view(dtype).fill_(_EXTREME[dtype][self.dressing])
            else:
                whole.fill_(_BAND[self.dressing])
        inner = whole[lo: lo + nbytes]
        if values is not None:
            inner.copy_(_bytes(values).to(self.device))
        else:
            inner.fill_(_FILL[self.dressing])
        view = inner.view(dtype).reshape(shape)
        natural = item // 2 if dtype.is_complex else item           # (a complex element is aligned as its parts are)
        assert view.data_ptr() == whole.data_ptr() + lo and view.data_ptr() % max(natural, int(align)) == 0
        self.items[name] = dict(role=role, whole=whole, view=view, lo=lo, nbytes=nbytes, item=item, snap=whole.clone(),
                                keep=np.zeros(shape, dtype=bool), open=np.zeros(shape, dtype=bool))
        return view

    # ---- after the call
    def check(self):
        """Bands, inputs and kept elements against their snapshots (after a device synchronise)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        tag = f"dressing {self.dressing or 'plain'}, skew {'on' if self.skew else 'off'}"
        for name, it in self.items.items():
            # one comparison of the whole allocation (2 GUARD + n bytes) on the device, per array and run
            changed = it["whole"] != it["snap"]
            lo, n = it["lo"], it["nbytes"]
            band_hit = bool(changed[:lo].any()) or bool(changed[lo + n:].any())
            interior_held = it["role"] == "in" or bool(it["keep"].any())         # (else any interior byte may change)
            if not band_hit and not interior_held:
                continue                                            # the usual case: two flags cross to the host, no mask
            changed = changed.cpu()                                 # a byte to name or an interior to hold: the mask itself
            band = changed.clone()
            band[lo: lo + n] = False
            if band.any():
                raise Violation(f"{name}: band byte at offset {_first(band) - lo} of the view was written ({tag}; the view has {n} bytes)")
            if it["role"] == "in" and changed.any():
                raise Violation(f"{name}: input byte at offset {_first(changed) - lo} was changed ({tag})")
            if it["keep"].any():
                km = torch.from_numpy(np.repeat(it["keep"].reshape(-1), it["item"]))
                bad = changed[lo: lo + n] & km
                if bad.any():
                    raise Violation(f"{name}: byte at offset {_first(bad)} lies in a range the header says is not written, and was ({tag})")

    def written(self, name):
        """(bytes of the view on the host, bool per byte: expected to be written)"""
        it = self.items[name]
        return _bytes(it["view"]).cpu(), torch.from_numpy(~np.repeat((it["keep"] | it["open"]).reshape(-1), it["item"]))


def compare(runs):
    """Every written element of every out / inout array, and every host result, bit for bit the same in every pair of runs."""
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            a, b = runs[i], runs[j]
            tag = f"{a.dressing or 'plain'} against {b.dressing or 'plain'}"
            if a.host != b.host:
                raise Violation(f"host results differ ({tag}): {a.host} != {b.host}")
            assert list(a.items) == list(b.items)
            for name, it in a.items.items():
                if it["role"] not in ("out", "inout"):
                    continue
                (xa, wa), (xb, wb) = a.written(name), b.written(name)
                if not torch.equal(wa, wb):
                    raise Violation(f"{name}: the two runs name different not-written ranges ({tag})")
                diff = (xa != xb) & wa
                if diff.any():
                    k = _first(diff)
                    raise Violation(f"{name}: byte at offset {k} (element {k // it['item']}) differs, {int(xa[k]):#04x} against "
                                    f"{int(xb[k]):#04x} ({tag}): not written, or it depends on memory outside the arrays")


def run(call, device="cpu", skews=(False, True)):
    """call(arrays) makes its arrays through `arrays` and performs the ABI call once.  Dressed A and B and run plain at each
    skew; -> the plain Arrays of the last skew (for a look at the values)."""
    for skew in skews:
        runs = []
        for dressing in DRESSINGS:
            a = Arrays(dressing, skew, device)
            call(a)
            a.check()
            runs.append(a)
        compare(runs)
    return runs[-1]
