"""A poisoned arena for the C ABI's memory contract (include/mi355attn.h, "Conventions": the caller owns every buffer, the
workspace need only hold mi355_<op>_workspace_bytes(...) bytes, its contents are undefined on entry, nothing outside the output
is written).

`Arena(nbytes, device)` is ONE uint8 tensor filled with 0xFF -- a NaN in fp32, fp16 and bf16 -- out of which a test carves every
buffer a call sees.  Every byte of it belongs to exactly one class:

  guard      never handed out: the 4 MiB margins at both ends, the gaps between regions, everything behind the last region
  input      a registered input or parameter; the arena keeps a copy and `verify()` compares bit for bit
  output     handed out by `torch_proxy()` in place of torch.empty / empty_like / zeros / zeros_like
  workspace  handed out by `workspace()`: exactly the declared size rounded up to 16 bytes, pre-filled (0xFF by default)
An input or output may also be ROW-STRIDED (`place_rows` / `place_empty_rows`): rows of `width` elements `ld` elements apart in a region of
exactly (rows - 1) * ld + width elements.  The padding behind each row but the last stays 0xFF and is checked: an input's with the rest
of its copy, an output's against 0xFF.

Every region starts at an address that is 16 mod 256: aligned to 16 bytes, the alignment the header asks for, and to nothing more.
The margins are wider than a full 256-row tile of any tensor the suite uses, so an over-read or an overrun stays inside mapped
memory: the arena never makes a kernel fault, it only observes afterwards.

What it cannot see: between two regions lie only 256 to 511 guard bytes.  A write that runs on from the end of a tensor -- the next row,
the next element of a partial tile -- hits them, and so does the first out-of-range row of a strided overrun; but a stray write that
skips more than that can land inside a neighbouring OUTPUT or WORKSPACE region, where it is noticed only if it changes bits that a test
compares afterwards (a neighbouring input is compared byte for byte).

A helper, not a conftest: tests import it (tests/test_abi_memory_cpu.py checks its bookkeeping on CPU tensors,
tests/test_abi_memory_gpu.py runs every entry point inside it).
"""
import torch

POISON = 0xFF
MARGIN = 4 << 20
ALIGN, PHASE = 256, 16


def _up(n, a):
    return -(-int(n) // a) * a


class ArenaViolation(AssertionError):
    pass


class Region:
    __slots__ = ("name", "kind", "off", "nbytes", "copy", "rows")

    def __init__(self, name, kind, off, nbytes, copy=None, rows=None):
        """`rows`: (row bytes, stride bytes) of a row-strided region (place_rows / place_empty_rows), else None."""
        self.name, self.kind, self.off, self.nbytes, self.copy, self.rows = name, kind, off, nbytes, copy, rows

    @property
    def end(self):
        return self.off + self.nbytes


class Arena:
    def __init__(self, nbytes, device="cpu", forget=None):
        """`forget(ptr, nbytes)`: called by reset() before the arena is refilled -- on the GPU mi355_workspace_forget, which the
        header requires before a buffer that served as a "ws_persistent" workspace is repurposed."""
        if nbytes < 2 * MARGIN + ALIGN:
            raise ValueError("arena smaller than its two margins")
        self.device = torch.device(device)
        self.buf = torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=self.device)
        self.nbytes = int(nbytes)
        self.base = self.buf.data_ptr()
        self.forget = forget
        self.ws_fill = POISON
        self.regions = []
        self._cursor = MARGIN
        self._count = 0

    # ---- placement -------------------------------------------------------------------------------------------------------------
    def _carve(self, nbytes, kind, name, copy=None):
        off = self._cursor
        off += (PHASE - (self.base + off)) % ALIGN                     # address == 16 (mod 256)
        if off + nbytes + MARGIN > self.nbytes:
            raise MemoryError(f"arena of {self.nbytes} bytes is full: {name} needs {nbytes} more")
        r = Region(name, kind, off, int(nbytes), copy)
        self.regions.append(r)
        self._cursor = off + int(nbytes) + ALIGN                       # at least 256 guard bytes between two regions
        return r

    def _view(self, r, shape, dtype):
        return self.buf[r.off:r.end].view(dtype).view(tuple(shape))

    def _name(self, name, kind):
        self._count += 1
        return name if name is not None else f"{kind}{self._count}"

    def place(self, t, name=None):
        """Copy tensor `t` (any device) into the arena as a registered input; returns the view (same shape and type, dense)."""
        src = t.detach().contiguous()
        r = self._carve(src.numel() * src.element_size(), "input", self._name(name, "input"))
        v = self._view(r, src.shape, src.dtype)
        v.copy_(src)
        r.copy = self.buf[r.off:r.end].clone()
        return v

    def place_empty(self, shape, dtype, name=None, zero=False):
        """An output region: left poisoned (or zeroed) for the kernel to write."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        r = self._carve(n * torch.empty((), dtype=dtype).element_size(), "output", self._name(name, "output"))
        v = self._view(r, shape, dtype)
        if zero:
            self.buf[r.off:r.end].zero_()
        return v

    def _carve_rows(self, rows, width, ld, dtype, kind, name):
        rows, width, ld = int(rows), int(width), int(ld)
        if rows < 1 or width < 1 or ld < width:
            raise ValueError(f"row-strided region needs rows >= 1 and ld >= width >= 1 (rows={rows} width={width} ld={ld})")
        esize = torch.empty((), dtype=dtype).element_size()
        r = self._carve(((rows - 1) * ld + width) * esize, kind, self._name(name, kind))
        r.rows = (rows, width, ld, esize)
        flat = self.buf[r.off:r.end].view(dtype)
        return r, flat.as_strided((rows, width), (ld, 1))

    def place_rows(self, t2d, ld, name=None):
        """Copy a 2-D tensor into an input region of exactly (rows - 1) * ld + width elements and return the as_strided view (row stride
        `ld` elements).  The ld - width elements behind every row but the last stay POISON -- a NaN in fp32, fp16 and bf16, so an operand
        read past the row's width poisons the sum it enters -- and belong to the region: verify() compares them byte for byte, too.
        Nothing behind the last row's width belongs to the caller: the guard starts there."""
        src = t2d.detach()
        if src.dim() != 2:
            raise ValueError("place_rows takes a 2-D tensor")
        r, v = self._carve_rows(src.shape[0], src.shape[1], ld, src.dtype, "input", name)
        v.copy_(src)
        r.copy = self.buf[r.off:r.end].clone()
        return v

    def place_empty_rows(self, rows, width, ld, dtype, name=None):
        """An output region of the same minimal extent, left poisoned; returns the strided view.  verify() additionally requires every
        padding byte (the ld - width elements behind each row but the last) to still be POISON."""
        return self._carve_rows(rows, width, ld, dtype, "output", name)[1]

    def workspace(self, nbytes, name=None):
        """A scratch region of exactly `nbytes` rounded up to 16, filled with `ws_fill`, a guard right behind it."""
        r = self._carve(_up(nbytes, 16), "workspace", self._name(name, "workspace"))
        if self.ws_fill != POISON:
            self.buf[r.off:r.end].fill_(self.ws_fill)
        return self.buf[r.off:r.end]

    def reset(self, ws_fill=POISON):
        if self.forget is not None:
            self.forget(self.base, self.nbytes)
        self.buf.fill_(POISON)
        self.regions = []
        self._cursor = MARGIN
        self._count = 0
        self.ws_fill = ws_fill

    # ---- inspection ------------------------------------------------------------------------------------------------------------
    def _where(self, off):
        """'N bytes past the end of `X`' / 'N bytes before the start of `X`' / 'byte N of `X`' for an arena offset."""
        if not self.regions:
            return f"arena offset {off} (nothing placed)"
        for r in self.regions:
            if r.off <= off < r.end:
                text = f"byte {off - r.off:,} of {r.kind} `{r.name}`".replace(",", " ")
                if r.rows is not None:                                 # row-strided: name the row and the column (in elements) as well
                    _, width, ld, esize = r.rows
                    row, col = divmod((off - r.off) // esize, ld)
                    text += f" (row {row}, column {col}: " + ("live)" if col < width else f"padding behind width {width})")
                return text
        best = min(self.regions, key=lambda r: min(abs(off - r.off), abs(off - (r.end - 1))))
        if off >= best.end:
            return f"{off - best.end + 1:,} bytes past the end of {best.kind} `{best.name}`".replace(",", " ")
        return f"{best.off - off:,} bytes before the start of {best.kind} `{best.name}`".replace(",", " ")

    def _gaps(self):
        pos = 0
        for r in self.regions:
            if r.off > pos:
                yield pos, r.off
            pos = r.end
        if pos < self.nbytes:
            yield pos, self.nbytes

    def violations(self):
        """Every broken promise, as text: guard bytes that are no longer 0xFF (the guard behind a workspace included) and inputs that
        differ from their copy (the padding of a row-strided input included), padding bytes of a row-strided output that are no
        longer 0xFF."""
        out = []
        gaps = list(self._gaps())
        dirty = torch.stack([(self.buf[a:b] != POISON).any() for a, b in gaps]).cpu().tolist()
        for (a, b), bad in zip(gaps, dirty):
            if bad:
                idx = torch.nonzero(self.buf[a:b] != POISON).reshape(-1)
                first, last, n = a + int(idx[0]), a + int(idx[-1]), int(idx.numel())
                out.append(f"guard written: {n} byte(s), first {self._where(first)}, last {self._where(last)}")
        ins = [r for r in self.regions if r.kind == "input"]
        if ins:
            same = torch.stack([(self.buf[r.off:r.end] == r.copy).all() for r in ins]).cpu().tolist()
            for r, ok in zip(ins, same):
                if not ok:
                    idx = torch.nonzero(self.buf[r.off:r.end] != r.copy).reshape(-1)
                    out.append(f"input modified: {int(idx.numel())} byte(s), first {self._where(r.off + int(idx[0]))}")
        for r in self.regions:
            if r.kind != "output" or r.rows is None or r.rows[0] < 2 or r.rows[2] == r.rows[1]:
                continue
            rows, width, ld, esize = r.rows
            pad = self.buf[r.off:r.off + (rows - 1) * ld * esize].view(rows - 1, ld * esize)[:, width * esize:]
            if bool((pad != POISON).any()):
                idx = torch.nonzero(pad != POISON)
                first = r.off + int(idx[0, 0]) * ld * esize + width * esize + int(idx[0, 1])
                out.append(f"output padding written: {int(idx.shape[0])} byte(s), first {self._where(first)}")
        return out

    def verify(self):
        bad = self.violations()
        if bad:
            raise ArenaViolation("memory contract violated:\n  " + "\n  ".join(bad))

    # ---- hooks -----------------------------------------------------------------------------------------------------------------
    def owns_device(self, device):
        d = torch.device(device) if device is not None else torch.device("cpu")
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def torch_proxy(self):
        return _TorchProxy(self)

    def workspace_hooks(self):
        """Replacements for _ffi.workspace / workspace_named / workspace_dedicated."""
        def workspace(nbytes, device):
            return self.workspace(nbytes)

        def workspace_named(name, nbytes, device):
            return self.workspace(nbytes, name=f"{name}#{self._count + 1}")

        def workspace_dedicated(op_key, nbytes, device):
            return self.workspace(nbytes, name=f"{op_key[0]}#{self._count + 1}")

        return workspace, workspace_named, workspace_dedicated


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        return tuple(size[0])
    return tuple(size)


class _TorchProxy:
    """`torch` for one module: every attribute is torch's, except the four allocators, which carve from the arena when asked for
    the arena's device (anything else -- another device, pinned memory, a layout -- goes to torch unchanged)."""

    def __init__(self, arena):
        object.__setattr__(self, "_arena", arena)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, real, zero, size, dtype, device, kw):
        a = self._arena
        if kw or not a.owns_device(device):
            return real(*size, dtype=dtype, device=device, **kw)
        return a.place_empty(_shape_of(size), dtype if dtype is not None else torch.get_default_dtype(), zero=zero)

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._alloc(torch.empty, False, size, dtype, device, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        return self._alloc(torch.zeros, True, size, dtype, device, kw)

    def _like(self, real, zero, t, dtype, device, kw):
        a = self._arena
        dev = device if device is not None else t.device
        if kw or not a.owns_device(dev):
            return real(t, dtype=dtype, device=device, **kw)
        return a.place_empty(t.shape, dtype if dtype is not None else t.dtype, zero=zero)

    def empty_like(self, t, dtype=None, device=None, **kw):
        return self._like(torch.empty_like, False, t, dtype, device, kw)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        return self._like(torch.zeros_like, True, t, dtype, device, kw)


class _RecordedCall:
    """One mi355_* function of the library: calls it, and keeps the name and what it returned."""

    def __init__(self, name, fn, log):
        self._name, self._fn, self._log = name, fn, log

    def __call__(self, *args):
        rc = self._fn(*args)
        self._log.append((self._name, rc))
        return rc

    def __getattr__(self, attr):
        return getattr(self._fn, attr)


class RecordingLib:
    """Thin proxy around the loaded library: remembers every mi355_* CALL with its return value.  `reached` holds the symbols that were
    called and returned 0 (MI355_OK): an entry that was looked up only, or that answered MI355_EUNSUPPORTED before a wrapper fell back
    to another one, does not count."""

    def __init__(self, real):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("mi355_") and callable(fn):
            return _RecordedCall(name, fn, self.calls)
        return fn

    @property
    def reached(self):
        return {name for name, rc in self.calls if rc == 0}
