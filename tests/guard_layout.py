"""Guarded buffers for the memory-contract tests (tests/test_guard_layout.py, tests/test_gpu_memory_contract.py).

include/aai.h entitles a call to the elements [b * imageStride + y * stride + x], x < W * C, y < H, of each buffer and to nothing
else: not to the row padding, not to the gap between two batch images, not to a row outside a band's footprint.  A GuardedLayout
places such a buffer INSIDE one larger allocation, between two guard margins of 8 rows of the padded stride plus 1024 elements each
(the widest access of any kernel is 16 bytes, the deepest pipeline keeps 8 source rows in flight: an overrun of any plausible size
lands in guard, never outside the allocation), `base_offset` elements past a 256-byte boundary.

  source       every element the call is not entitled to holds POISON: a quiet NaN for fp32 (0 x NaN = NaN reaches the output); for
               8- / 16-bit pixels the case runs once with all-zero and once with all-ones poison, and the outputs must agree bit for bit
  destination  every element starts as SENTINEL_BITS (a NaN with a recognisable payload, compared through an int32 view); check_dst
               returns the output view and where / how many guard elements changed

Plain numpy; a torch tensor (any device) is accepted wherever a buffer is read back, and to_device uploads one.  A band is a
layout whose H is the number of footprint rows: the rows before and after the footprint are then the margins themselves.
"""
import numpy as np

SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN no arithmetic produces (payload 0x45a5a5)
ALIGN = 256                         # bytes: what the device allocator guarantees and the samplers' column shift is relative to
DTYPES = {"f32": np.float32, "u8": np.uint8, "u16": np.uint16}
REGIONS = ("before", "pad", "gap", "after")      # leading margin, row padding, between two images, trailing margin


def poisons(dtype):
    """the poison fills a case runs with, by source type"""
    return ("nan",) if dtype == "f32" else ("zeros", "ones")


def to_numpy(buffer, dtype):
    """a flat numpy view of `dtype` of a numpy array or a torch tensor (copied to the host)"""
    if hasattr(buffer, "detach"):
        buffer = buffer.detach().cpu().numpy()
    return np.ascontiguousarray(buffer).reshape(-1).view(np.uint8).view(dtype)


def to_device(buffer, device="cuda"):
    """upload a host buffer as raw bytes (keeps NaN payloads and 16-bit patterns as they are); returns a torch uint8 tensor"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(buffer).reshape(-1).view(np.uint8).copy()).to(device)
    assert t.data_ptr() % ALIGN == 0, "the allocator returned a block that is not 256-byte aligned"
    return t


class GuardedLayout:
    def __init__(self, shape, dtype="f32", stride=None, image_stride=None, base_offset=0):
        B, H, W, C = (int(v) for v in shape)
        assert B >= 1 and H >= 1 and W >= 1 and 1 <= C <= 4, shape
        self.shape, self.dtype, self.np_dtype = (B, H, W, C), dtype, np.dtype(DTYPES[dtype])
        self.row = W * C
        self.stride = self.row if stride is None else int(stride)
        self.image_stride = H * self.stride if image_stride is None else int(image_stride)
        assert self.stride >= self.row and self.image_stride >= H * self.stride, (self.stride, self.image_stride)
        self.base_offset = int(base_offset)
        assert 0 <= self.base_offset < ALIGN
        self.margin = 8 * self.stride + 1024                         # a condition (see the module text), not a measurement
        per = ALIGN // self.np_dtype.itemsize
        self.lead = -(-self.margin // per) * per + self.base_offset     # index of the first entitled element
        self.span = (B - 1) * self.image_stride + (H - 1) * self.stride + self.row
        self.total = self.lead + self.span + self.margin
        b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(self.row), indexing="ij")
        self.index = (self.lead + b * self.image_stride + y * self.stride + x).astype(np.int64)     # [B, H, W*C] -> flat index
        self.entitled = np.zeros(self.total, dtype=bool)
        self.entitled[self.index.reshape(-1)] = True
        assert int(self.entitled.sum()) == B * H * self.row
        assert self.lead >= self.margin and self.total - (self.lead + self.span) >= self.margin

    # ---- addresses -------------------------------------------------------------------------------------------------------
    def byte_offset(self):
        """bytes from the start of the allocation to the first entitled element"""
        return self.lead * self.np_dtype.itemsize

    def ptr(self, tensor):
        """device address of the first entitled element of an uploaded buffer (to_device)"""
        assert tensor.numel() * tensor.element_size() == self.total * self.np_dtype.itemsize
        return tensor.data_ptr() + self.byte_offset()

    def region(self, offset):
        """which part of the allocation the element `offset` elements from the first entitled one lies in:
        ("entitled" | "before" | "pad" | "gap" | "after", image, row, column)"""
        B, H, W, C = self.shape
        if offset < 0:
            return ("before", 0, offset // self.stride, offset % self.stride)          # (rows count down from row 0)
        if offset >= self.span:
            last = (B - 1) * self.image_stride
            return ("after", B - 1, (offset - last) // self.stride, (offset - last) % self.stride)
        b, r = divmod(offset, self.image_stride)
        y, x = divmod(r, self.stride)
        if y >= H:
            return ("gap", b, y, x)
        return ("entitled" if x < self.row else "pad", b, y, x)

    def describe(self, offset):
        kind, b, y, x = self.region(offset)
        return "element %+d = %s (image %d, row %d, column %d of stride %d, row length %d)" % (offset, kind, b, y, x, self.stride, self.row)

    def region_mask(self, names=REGIONS):
        """bool mask over the allocation of the non-entitled elements in the named regions"""
        idx = np.arange(self.total, dtype=np.int64) - self.lead
        B, H, W, C = self.shape
        before, after = idx < 0, idx >= self.span
        inside = ~before & ~after
        r = np.where(inside, idx % self.image_stride, 0)
        gap = inside & (r >= H * self.stride)
        pad = inside & ~gap & (r % self.stride >= self.row)
        m = np.zeros(self.total, dtype=bool)
        for name, part in (("before", before), ("pad", pad), ("gap", gap), ("after", after)):
            if name in names:
                m |= part
        assert not (m & self.entitled).any()
        return m

    # ---- sources ---------------------------------------------------------------------------------------------------------
    def poison_value(self, poison):
        if poison == "nan":
            assert self.dtype == "f32"
            return np.float32(np.nan)
        if poison == "ones":
            return self.np_dtype.type(np.iinfo(self.np_dtype).max) if self.dtype != "f32" else np.float32(1.0)
        assert poison == "zeros", poison
        return self.np_dtype.type(0)

    def make_src(self, values, poison, where=None):
        """the whole allocation as a flat host array: `values` ([B, H, W, C] or [B, H, W*C]) in the entitled elements, `poison` in
        every other element -- or only in those of `where` (a bool mask over the allocation), zeros in the rest"""
        B, H, W, C = self.shape
        buf = np.zeros(self.total, dtype=self.np_dtype)
        mask = ~self.entitled if where is None else (np.asarray(where, dtype=bool) & ~self.entitled)
        buf[mask] = self.poison_value(poison)
        buf[self.index.reshape(-1)] = np.asarray(values, dtype=self.np_dtype).reshape(-1)
        return buf

    def gather(self, buffer):
        """the entitled view [B, H, W, C] of a buffer (numpy or torch)"""
        return to_numpy(buffer, self.np_dtype)[self.index].reshape(self.shape)

    def locate_reads(self, run, values, poison, limit=8):
        """Which non-entitled elements does `run` read?  run(flat host buffer) -> output array.  Poison is confined to ever smaller
        sets of elements (zeros elsewhere) until single elements are left whose poison changes the output's bits: their offsets
        from the first entitled element, ascending, at most `limit`.  One run per step: for CPU stand-ins, or for the message of a
        case that has already failed."""
        def bits(a):
            return np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()

        clean = bits(run(self.make_src(values, "zeros")))
        found = []

        def search(cand):
            if len(found) >= limit or cand.size == 0:
                return
            where = np.zeros(self.total, dtype=bool)
            where[cand] = True
            if np.array_equal(bits(run(self.make_src(values, poison, where))), clean):
                return
            if cand.size == 1:
                found.append(int(cand[0]) - self.lead)
                return
            search(cand[:cand.size // 2])
            search(cand[cand.size // 2:])

        search(np.flatnonzero(~self.entitled))
        return found

    # ---- destinations ----------------------------------------------------------------------------------------------------
    def make_dst(self):
        """the whole allocation, every element the sentinel; fp32 only (every output is fp32)"""
        assert self.dtype == "f32"
        return np.full(self.total, SENTINEL_BITS, dtype=np.int32).view(np.float32)

    def changed_guards(self, buffer):
        """offsets (from the first entitled element, ascending) of the guard elements whose bits are no longer the sentinel's"""
        a = to_numpy(buffer, np.int32)
        assert a.size == self.total, (a.size, self.total)
        return np.flatnonzero((a != SENTINEL_BITS) & ~self.entitled) - self.lead

    def check_dst(self, buffer):
        """(output view [B, H, W, C] float32, offset of the first changed guard element or None, number of changed guard elements)"""
        changed = self.changed_guards(buffer)
        out = to_numpy(buffer, np.float32)[self.index].reshape(self.shape)
        return out, (int(changed[0]) if changed.size else None), int(changed.size)

    @staticmethod
    def sentinels_left(out):
        """number of output elements that still hold the sentinel: pixels the call did not write"""
        return int((np.ascontiguousarray(out).view(np.int32) == SENTINEL_BITS).sum())
