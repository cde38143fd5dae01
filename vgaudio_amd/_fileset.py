"""What the *FileSet classes (sets of files resident on the device) share on the Python side: the optional int64 offsets
argument, the count-then-fetch pair of the work-item hooks, and the handle's life with the images' split."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def i64_or_none(values):
    """(keep-alive array, int64 pointer) of a list of offsets, (None, None) of None"""
    if values is None:
        return None, None
    a = np.ascontiguousarray(values, dtype=np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def fetch_items(call, head, item_type):
    """call(*head, items, capacity, count_out) twice: for the count, then for the items"""
    count = C.c_int64()
    check(call(*head, None, 0, C.byref(count)))
    items = (item_type * max(count.value, 1))()
    check(call(*head, items, count.value, C.byref(count)))
    return list(items[:count.value])


class FileSetHandle:
    """the handle `_h` of a set"""
    _destroy = None                                # the name of the C call that destroys `_h`

    def close(self):
        if self._h:
            getattr(_lib.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    __del__ = close


class FileSetBase(FileSetHandle):
    """a set whose images lie packed in one buffer (`image_offsets`, `image_sizes`)"""

    def images(self, host_buffer):
        """one `bytes` per file from the packed images (a device tensor or a numpy array); synchronises"""
        host = host_buffer.cpu().numpy() if hasattr(host_buffer, "cpu") else np.asarray(host_buffer, dtype=np.uint8)
        return [host[int(at):int(at) + int(size)].tobytes() for at, size in zip(self.image_offsets, self.image_sizes)]
