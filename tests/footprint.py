"""Arena helper of the memory-footprint tests (tests/test_hip_footprint.py, tests/test_footprint_harness.py).

A kernel test that hands the library dense tensors at the start of their own allocation cannot see WHERE the kernel reads and
writes.  `Arena` places one operand inside a larger allocation,

    [ guard | window rows with gap columns | guard ]

  * guards: >= 256 rows x ld elements and >= 4 KiB each, so an overrun by one tile stays inside memory the test owns;
  * the window's first byte sits at (256-byte boundary + a), a = the MINIMUM alignment the header states for the pointer:
    the address is aligned to a and not to 2a;
  * ld = used width + `gap` (the smallest step the entry point's checks allow), so every row has gap columns;
  * input guards / gaps are filled with zeros, finite garbage or NaN; output allocations (window included) with a byte
    sentinel that differs between the runs; everything is compared as INTEGERS (NaN == NaN).

`run_footprint(body)` runs `body(fp)` once per fill mode and checks
    P1 independence      output windows of the garbage / nan runs are bit-identical to the zero run,
    P2 containment       every byte outside a declared window is unchanged,
    P3 inputs unchanged  input windows are unchanged too,
    P4 parity            the zero run against a reference (callbacks registered by the body),
raising `FootprintViolation` whose `.prop` names the violated property.  Works on any device (the harness tests run fake
Python kernels on CPU tensors through the same code).
"""
from __future__ import annotations

import torch

FILLS = ("zero", "garbage", "nan")
SENTINEL = {"zero": 0xA5, "garbage": 0x5B, "nan": 0xC6}      # byte patterns of the output pre-fill, one per run
P1, P2, P3, P4 = "P1 independence", "P2 containment", "P3 inputs unchanged", "P4 parity"
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class FootprintViolation(AssertionError):
    def __init__(self, prop, msg):
        super().__init__(f"{prop}: {msg}")
        self.prop = prop


def _poison(n, dtype, fill, seed, device):
    """n elements of input poison as the integer words of `dtype`."""
    size = torch.empty(0, dtype=dtype).element_size()
    it = _INT[size]
    if fill == "zero":
        return torch.zeros(n, dtype=it, device=device)
    if fill == "nan":      # 0x7FFF: a NaN in bf16 and in fp16; 0x7FC00000: fp32 quiet NaN
        word = {2: 0x7FFF, 4: 0x7FC00000, 8: 0x7FF8000000000000, 1: 0xFF}[size]
        return torch.full((n,), word, dtype=torch.int64).to(it).to(device)
    g = torch.Generator(device=device).manual_seed(seed)      # made where it lives: the big arenas hold 10^7 elements
    sign = (torch.randint(0, 2, (n,), generator=g, device=device) * 2 - 1).float()
    if size == 2:          # finite in both 16-bit types: uniform in +-[1e3, 3e4]
        v = (1e3 + torch.rand(n, generator=g, device=device) * 2.9e4) * sign
        return v.to(dtype).view(it)
    if dtype.is_floating_point:
        return (sign * 1e30).to(dtype).view(it)
    return torch.randint(1 << 20, 1 << 30, (n,), generator=g, device=device).to(it)    # integer tensors (counters, tables)


class Arena:
    """One operand [rows][ld] (cols used) of `dtype` inside a poisoned allocation.  role: "in" (read only), "out" (written;
    the whole allocation starts as sentinel bytes) or "inout" (documented in-place operand / caller-initialised output:
    window = data, surroundings = poison)."""

    def __init__(self, name, rows, cols, dtype, *, device, fill, role="in", data=None, gap=None, ld=None, align=16, seed=0,
                 guard_rows=256, compare=True):
        self.compare = compare                                          # False: scratch memory, P2 only (its content is unspecified)
        assert fill in FILLS and role in ("in", "out", "inout")
        self.name, self.rows, self.cols, self.dtype, self.role, self.fill = name, int(rows), int(cols), dtype, role, fill
        size = torch.empty(0, dtype=dtype).element_size()
        self.itemsize, self.int_dtype = size, _INT[size]
        if ld is None:
            ld = cols + ((8 if size == 2 else 4) if gap is None else gap)
        assert ld >= cols and align % size == 0 and 256 % align == 0 and align < 256
        self.ld, self.align = int(ld), align
        guard = max(guard_rows * self.ld * size, 4096)
        guard = -(-guard // 256) * 256                                  # whole 256-byte lines: the window keeps the offset `align`
        self.guard = guard // size
        self.span = (self.rows - 1) * self.ld + self.cols               # elements from the window's first to its last
        nbytes = 2 * guard + self.span * size
        self.buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=device)
        self.start = (align - self.buf.data_ptr()) % 256                # typed region (and window) at 256-byte boundary + align
        self.flat = self.buf[self.start:self.start + nbytes].view(dtype)
        self.base = self.guard                                          # element index of window[0][0] in `flat`
        assert (self.flat.data_ptr() + self.base * size) % 256 == align
        mask = torch.zeros(self.flat.numel(), dtype=torch.bool, device=device)
        mask[self.base:self.base + self.span] = True
        if self.ld > self.cols and self.rows > 1:
            body = mask[self.base:self.base + (self.rows - 1) * self.ld].view(self.rows - 1, self.ld)
            body[:, self.cols:] = False
        self.mask = mask
        if role == "out":
            self.buf.fill_(SENTINEL[fill])
        else:
            self.buf.fill_(SENTINEL[fill])                              # the alignment slack round the typed region
            self.flat.view(self.int_dtype).copy_(_poison(self.flat.numel(), dtype, fill, 1000 + seed, device))
        if data is not None:
            assert role != "out"
            self.window().copy_(data.to(dtype).reshape(self.rows, self.cols))
        else:
            assert role == "out", "an input needs data"
        self.snapshot = self.buf.clone()

    # ---- what the kernel gets
    def window(self):
        """The strided [rows][cols] view handed to the library (`data_ptr()` = the window's first byte)."""
        return self.flat[self.base:self.base + self.span].as_strided((self.rows, self.cols), (self.ld, 1))

    def ptr(self):
        return self.flat.data_ptr() + self.base * self.itemsize

    # ---- checks
    def _first(self, bad):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        rel = i - self.base
        return f"element {rel} from the window start = row {rel // self.ld}, column {rel % self.ld} (ld {self.ld}, window {self.rows} x {self.cols})"

    def outside_untouched(self):
        now, was = self.flat.view(self.int_dtype), self.snapshot[self.start:self.start + self.flat.numel() * self.itemsize].view(self.int_dtype)
        bad = (now != was) & ~self.mask
        if bool(bad.any()):
            raise FootprintViolation(P2, f"`{self.name}` ({self.fill} run): {int(bad.sum())} element(s) outside the window changed, first at {self._first(bad)}")
        head, tail = slice(0, self.start), slice(self.start + self.flat.numel() * self.itemsize, None)
        if not (torch.equal(self.buf[head], self.snapshot[head]) and torch.equal(self.buf[tail], self.snapshot[tail])):
            raise FootprintViolation(P2, f"`{self.name}` ({self.fill} run): bytes beyond the guards changed")

    def inputs_unchanged(self):
        now, was = self.flat.view(self.int_dtype), self.snapshot[self.start:self.start + self.flat.numel() * self.itemsize].view(self.int_dtype)
        bad = (now != was) & self.mask
        if bool(bad.any()):
            raise FootprintViolation(P3, f"input `{self.name}` ({self.fill} run): {int(bad.sum())} element(s) changed, first at {self._first(bad)}")

    def untouched_in_window(self, rows=None, cols=None):
        """Part of an output window the header says is NOT written still holds its initial bytes."""
        r = slice(None) if rows is None else rows
        c = slice(None) if cols is None else cols
        was = self.snapshot[self.start:self.start + self.flat.numel() * self.itemsize].view(self.int_dtype)
        was = was[self.base:self.base + self.span].as_strided((self.rows, self.cols), (self.ld, 1))
        if not torch.equal(self.window().view(self.int_dtype)[r, c], was[r, c]):
            raise FootprintViolation(P2, f"`{self.name}` ({self.fill} run): a region the header leaves untouched was written")


class Footprint:
    """What a case body gets: makes arenas with this run's fill mode and collects them."""

    def __init__(self, fill, device):
        self.fill, self.device = fill, device
        self.arenas, self.parity, self.after = [], [], []

    def _add(self, role, name, rows, cols, dtype, **kw):
        a = Arena(name, rows, cols, dtype, device=self.device, fill=self.fill, role=role, seed=len(self.arenas), **kw)
        self.arenas.append(a)
        return a

    def inp(self, name, data, dtype=None, **kw):
        data = data if data.dim() == 2 else data.reshape(1, -1)
        return self._add("in", name, data.shape[0], data.shape[1], dtype or data.dtype, data=data, **kw)

    def inout(self, name, data, dtype=None, **kw):
        data = data if data.dim() == 2 else data.reshape(1, -1)
        return self._add("inout", name, data.shape[0], data.shape[1], dtype or data.dtype, data=data, **kw)

    def out(self, name, rows, cols, dtype, **kw):
        return self._add("out", name, rows, cols, dtype, **kw)

    def poison(self, n, dtype):
        """n elements of this run's input poison: for padding INSIDE a window that the header says the kernel ignores."""
        return _poison(n, dtype, self.fill, 77, "cpu").view(dtype)

    def expect(self, what, got, ref, check):
        """P4 (zero run only): `got()` -> tensor, `ref()` -> fp32 reference, `check(got, ref, what)` asserts the gate."""
        self.parity.append((what, got, ref, check))

    def finally_check(self, fn):
        """Extra assertion after the launch in EVERY run (documented padding values, library state)."""
        self.after.append(fn)


def run_footprint(body, device="cpu", sync=None, fills=FILLS):
    """Run `body(fp)` once per fill mode and check P1 - P4 (module docstring).  Returns the zero run's output windows."""
    first = None
    for fill in fills:
        fp = Footprint(fill, device)
        body(fp)
        if sync is not None:
            sync()
        for a in fp.arenas:
            a.outside_untouched()
            if a.role == "in":
                a.inputs_unchanged()
        for fn in fp.after:
            fn()
        outs = {a.name: a.window().view(a.int_dtype).cpu().clone() for a in fp.arenas if a.role != "in" and a.compare}
        if first is None:
            first = outs
            for what, got, ref, check in fp.parity:
                try:
                    check(got(), ref(), what)
                except FootprintViolation:
                    raise
                except AssertionError as e:
                    raise FootprintViolation(P4, f"{what}: {e}") from e
        else:
            for name, w in outs.items():
                bad = w != first[name]
                if bool(bad.any()):
                    i = int(torch.nonzero(bad.reshape(-1))[0])
                    raise FootprintViolation(P1, f"output `{name}`: {int(bad.sum())} element(s) of the {fill} run differ from the zero run, "
                                                 f"first at row {i // w.shape[1]}, column {i % w.shape[1]}: the result depends on memory outside the operands")
    return first
