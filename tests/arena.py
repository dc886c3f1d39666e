"""A guarded arena for footprint tests of the device API (include/rbg.h, the *_dev entry points).

One torch.uint8 allocation per test case, filled with a pattern byte.  Everything a call receives -- inputs, outputs, workspaces -- is carved out of
it, each region of exactly the size the header says the caller provides, at the MINIMUM alignment the header allows and off every 64-byte line, with at
least GUARD pattern bytes before and behind it.  A kernel that writes one element too far therefore writes into guard bytes of the same allocation --
never into unmapped memory -- and check() names the region, the side and the byte offset of every guard byte that changed.  A plain helper, not a
fixture; it works on CPU tensors as well (tests/test_arena_host.py).
"""
import numpy as np
import torch

PATTERN = 0xA5
GUARD = 256      # pattern bytes before and behind every carve, at least
LINE = 64


def default_skew(align):
    """the smallest non-zero multiple of `align` below 64: the region then sits at its minimum alignment, off every 64-byte line; 0 for align >= 64"""
    return align if align < LINE else 0


class ArenaError(AssertionError):
    pass


class Region:
    def __init__(self, arena, name, begin, nbytes, align, skew):
        self.arena, self.name, self.begin, self.nbytes, self.align, self.skew = arena, name, begin, nbytes, align, skew
        self.end = begin + nbytes
        self.saved = None

    @property
    def u8(self):
        return self.arena.buf[self.begin:self.end]

    def view(self, dtype):
        return self.u8.view(dtype)

    def data_ptr(self):
        """the region's address (also for nbytes == 0, where a tensor view has no storage of its own to point at)"""
        return self.arena.base + self.begin

    @property
    def ptr(self):
        return self.data_ptr()

    def fill_from(self, array):
        """copy a host array (any dtype, exactly nbytes long) into the region"""
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        if raw.size != self.nbytes:
            raise ArenaError(f"{self.name}: {raw.size} bytes given for a region of {self.nbytes}")
        if raw.size:
            self.u8.copy_(torch.from_numpy(raw.copy()))
        return self

    def fill(self, byte):
        if self.nbytes:
            self.u8.fill_(byte)
        return self

    def numpy(self, dtype=np.uint8):
        return self.u8.cpu().numpy().copy().view(dtype)


class Arena:
    def __init__(self, capacity, device="cpu", pattern=PATTERN):
        self.pattern = pattern
        self.capacity = capacity
        # (512 spare bytes: offset 0 of the arena is put on a 256-byte boundary whatever the allocator returns, and 256 pattern bytes stay behind `capacity`)
        self.raw = torch.full((capacity + 512,), pattern, dtype=torch.uint8, device=device)
        lead = (-self.raw.data_ptr()) % 256
        self.buf = self.raw[lead:lead + capacity + 256]
        self.base = self.buf.data_ptr()
        self.regions = []
        self.cursor = 0      # the end of the last carve

    def carve(self, name, nbytes, align=8, skew=None):
        """`nbytes` bytes at an address = skew (mod 64) -- for align > 64, a multiple of align --, GUARD pattern bytes at least on either side"""
        if skew is None:
            skew = default_skew(align)
        if nbytes < 0 or align <= 0 or (align & (align - 1)):
            raise ArenaError(f"{name}: bad size or alignment")
        if align < LINE and (skew % align or not 0 <= skew < LINE):
            raise ArenaError(f"{name}: skew {skew} is no multiple of the alignment {align} below {LINE}")
        if align >= LINE and skew:
            raise ArenaError(f"{name}: a region aligned to {align} has no skew")
        if any(r.name == name for r in self.regions):
            raise ArenaError(f"{name}: carved twice")
        begin = self.cursor + GUARD
        step = max(align, LINE)
        begin += (skew - (self.base + begin)) % step
        if begin + nbytes + GUARD > self.buf.numel():
            raise ArenaError(f"{name}: the arena of {self.capacity} bytes is full")
        r = Region(self, name, begin, nbytes, align, skew)
        self.regions.append(r)
        self.cursor = r.end
        return r

    def carve_from(self, name, array, align=8, skew=None):
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        return self.carve(name, raw.size, align, skew).fill_from(raw)

    def __getitem__(self, name):
        for r in self.regions:
            if r.name == name:
                return r
        raise KeyError(name)

    # ---- checks ------------------------------------------------------------------------------------------------------
    def guard_faults(self):
        """[(region name, 'before' | 'after', byte offset from the region's edge, value found)] for every guard byte that changed; `before` offsets count
        back from the region's first byte (1 = the byte just below it), `after` offsets up from its end (0 = the first byte behind it)"""
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for r in self.regions:
            inside[r.begin:r.end] = True
        bad = np.flatnonzero((host != self.pattern) & ~inside)
        out = []
        regs = sorted(self.regions, key=lambda r: r.begin)
        for b in bad.tolist():
            prev = [r for r in regs if r.end <= b]
            nxt = [r for r in regs if r.begin > b]
            # the nearer neighbour names the byte
            if prev and (not nxt or b - prev[-1].end < nxt[0].begin - b):
                out.append((prev[-1].name, "after", b - prev[-1].end, int(host[b])))
            elif nxt:
                out.append((nxt[0].name, "before", nxt[0].begin - b, int(host[b])))
            else:
                out.append(("<arena>", "after", b, int(host[b])))
        return out

    def check(self):
        faults = self.guard_faults()
        if faults:
            lines = [f"{name}: byte {off} {side} the region holds 0x{v:02X}, not the pattern 0x{self.pattern:02X}" for name, side, off, v in faults[:20]]
            raise ArenaError(f"{len(faults)} guard byte(s) written:\n  " + "\n  ".join(lines))

    def check_untouched(self, name, byte_ranges, expect=None):
        """the bytes [a, b) of region `name`, for every (a, b) given, still hold the pattern (or the bytes of `expect`, a uint8 array of the whole region)"""
        r = self[name]
        host = r.numpy()
        for a, b in byte_ranges:
            if not 0 <= a <= b <= r.nbytes:
                raise ArenaError(f"{name}: range [{a}, {b}) outside the region of {r.nbytes} bytes")
            want = np.full(b - a, self.pattern, np.uint8) if expect is None else np.asarray(expect, np.uint8)[a:b]
            bad = np.flatnonzero(host[a:b] != want)
            if bad.size:
                raise ArenaError(f"{name}: byte {a + int(bad[0])} inside the region was declared untouched and holds 0x{int(host[a + bad[0]]):02X}, "
                                 f"not 0x{int(want[bad[0]]):02X} ({bad.size} such byte(s) in [{a}, {b}))")

    def snapshot(self, name):
        r = self[name]
        r.saved = r.numpy()
        return r.saved

    def assert_unchanged(self, name):
        r = self[name]
        if r.saved is None:
            raise ArenaError(f"{name}: no snapshot taken")
        bad = np.flatnonzero(r.numpy() != r.saved)
        if bad.size:
            raise ArenaError(f"{name}: input changed at byte {int(bad[0])} ({bad.size} byte(s) differ from the snapshot)")

    def snapshot_all(self, names):
        for n in names:
            self.snapshot(n)

    def assert_all_unchanged(self):
        for r in self.regions:
            if r.saved is not None:
                self.assert_unchanged(r.name)
