"""FarBuffer: one device allocation of several GiB in which a test places a few small windows far apart.

test_gpu_device_layouts.py's Placed builds its whole allocation on the host and compares it there; at 8 GiB a row that
is neither possible nor needed.  Here the allocation is made and filled on the device with ONE junk byte, only the windows
travel (put / get), and untouched() counts on the device, a quarter of a GiB at a time, the bytes outside the windows that no
longer equal the fill.  A kernel that forms `row * pitch`, `offset >> 2` or a limit in 32 bits lands somewhere else inside the allocation
(the tests choose extents and bases so that it does), which shows as wrong bytes in a window or changed junk outside them,
not as a fault.
"""
import numpy as np

GIB = 1 << 30
CHUNK = GIB >> 2            # untouched() looks at this many bytes at a time: its temporary, on top of the test's buffers
FILL = 0xA7                 # no codec's idle byte: not 0, not 0xFF, not a frame sync


def need(nbytes):
    """skip the calling test when the device has less free memory than it is about to allocate (and only then)"""
    import pytest
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (GIB >> 1):
        pytest.skip(f"{nbytes / GIB:.1f} GiB needed, {free / GIB:.1f} GiB free on the device")


class FarBuffer:
    """`extent` bytes on the device, every one of them `fill`"""

    def __init__(self, extent, fill=FILL):
        import torch
        self.extent, self.fill = int(extent), int(fill)
        self.t = torch.empty(self.extent, dtype=torch.uint8, device="cuda")
        self.t.fill_(self.fill)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 256 == 0
        self.changed = None

    def put(self, offset, array):
        """the bytes of `array` to [offset, offset + nbytes)"""
        import torch
        a = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert 0 <= offset and offset + a.size <= self.extent
        self.t[offset:offset + a.size].copy_(torch.from_numpy(a.copy()))
        return (int(offset), int(a.size))

    def get(self, offset, nbytes, dtype=np.uint8):
        assert 0 <= offset and offset + nbytes <= self.extent
        return self.t[offset:offset + nbytes].cpu().numpy().view(dtype)

    def untouched(self, windows):
        """windows: (offset, nbytes) pairs.  None when every byte outside them still equals the fill, else the offset of the
        first that does not (their number is left in .changed)."""
        import torch
        gaps, at = [], 0
        for o, n in sorted((int(o), int(n)) for o, n in windows):
            assert 0 <= o and o + n <= self.extent
            if o > at:
                gaps.append((at, o))
            at = max(at, o + n)
        if at < self.extent:
            gaps.append((at, self.extent))
        pieces = [(a, min(a + CHUNK, e)) for s, e in gaps for a in range(s, e, CHUNK)]
        # one flag per piece and one transfer for all of them: .any() reduces the comparison as it is, where .sum() and
        # count_nonzero() widen it to int64 first (2 GiB for a piece); the counting is for the failure's message only
        hit = torch.zeros(len(pieces), dtype=torch.bool, device="cuda")
        for i, (a, b) in enumerate(pieces):
            hit[i] = (self.t[a:b] != self.fill).any()
        hit = np.flatnonzero(hit.cpu().numpy())
        self.changed = 0
        if not hit.size:
            return None
        step = 1 << 24
        for i in hit:
            a, b = pieces[int(i)]
            self.changed += sum(int(torch.count_nonzero(self.t[s:min(s + step, b)] != self.fill)) for s in range(a, b, step))
        a, b = pieces[int(hit[0])]
        for s in range(a, b, step):
            at = torch.nonzero(self.t[s:min(s + step, b)] != self.fill)
            if at.numel():
                return s + int(at[0, 0].item())

    def free(self):
        self.t = None


def release(*buffers):
    """a test's last lines: drop its buffers and give the memory back to the device"""
    import torch
    for b in buffers:
        if b is not None:
            b.free()
    torch.cuda.empty_cache()
