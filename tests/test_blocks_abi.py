"""vx_block_points and vx_read_region without a GPU: the library exports them, the harness's record has the header's layout (a size and offset
probe compiled from include/voxel_hip.h with gcc, the way the C-ABI client is compiled), and the entry points' argument checks, which come
before any HIP call, name the field they refuse."""
import ctypes as C

import numpy as np

from abi_checks import probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p



def test_the_library_exports_them():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    for name in ("vx_block_points", "vx_read_region"):
        assert hasattr(L, name)
        assert name in hip.SYMBOLS and getattr(hip.lib(), name) is not None


def test_the_record_has_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_block_cell": ["value", "cell_log2"]}, ["VX_CELL_OUTSIDE"])
    assert said["vx_block_cell"] == (8,) == (hip.BLOCK_CELL_DTYPE.itemsize,)
    assert said["VX_CELL_OUTSIDE"] == (hip.VX_CELL_OUTSIDE,) == (0xFFFFFFFF,)
    assert list(hip.BLOCK_CELL_DTYPE.names) == ["value", "cell_log2"]
    for f, at in (("value", 0), ("cell_log2", 4)):
        dt, offset = hip.BLOCK_CELL_DTYPE.fields[f][:2]
        assert said[f"vx_block_cell.{f}"] == (offset, dt.itemsize) == (at, 4) and dt.str == "<u4", f


def test_block_points_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records stay as they are."""
    L = hip.lib()
    pos = np.zeros((4, 4), dtype=np.float32)
    out = np.full(4 * 8 + 8, 0x5a, dtype=np.uint8)

    def call(p=pos.ctypes.data, stride=12, count=4, memory=hip.VX_MEM_HOST, o=out.ctypes.data):
        return L.vx_block_points(None, _vp(p), stride, count, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    for stride in (0, 4, 8, 13, 14, 18, 2):
        refused(b"pos_stride", stride=stride)
    for off in (1, 2, 3):
        refused(b"pos must be aligned", p=pos.ctypes.data + off)
    refused(b"null pos", p=None)
    refused(b"null out", o=None)
    refused(b"count", count=(1 << 24) + 1)
    refused(b"VX_MEM", memory=2)
    refused(b"VX_MEM", memory=-1)
    assert out.ctypes.data % 8 == 0
    for off in (1, 2, 4, 6):
        refused(b"out in device memory must be aligned to 8", memory=hip.VX_MEM_DEVICE, o=out.ctypes.data + off)
    # every rule kept: only the context is missing (records inside vx_entity and vx_ray_hit; the largest count; a host out at any address)
    refused(b"null context", stride=64)
    refused(b"null context", p=pos.ctypes.data + 16, stride=32, memory=hip.VX_MEM_DEVICE)
    refused(b"null context", count=1 << 24)
    refused(b"null context", o=out.ctypes.data + 1)
    assert L.vx_block_points(None, None, 12, 0, hip.VX_MEM_HOST, None) == 1 and b"null context" in L.vx_last_error()
    # no points: nothing is read or written, so no stride, alignment or pointer is refused -- only the context is missing
    refused(b"null context", p=pos.ctypes.data + 1, stride=5, count=0, memory=hip.VX_MEM_DEVICE, o=out.ctypes.data + 3)
    refused(b"VX_MEM", count=0, memory=7)


def test_read_region_argument_checks_need_no_device():
    L = hip.lib()
    out = np.full(64 + 8, 0x5a, dtype=np.uint8)
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def call(lo=(-3, 0, 5), size=(4, 2, 2), memory=hip.VX_MEM_HOST, o=out.ctypes.data):
        return L.vx_read_region(None, C.byref(i3(*lo)) if lo is not None else None, C.byref(u3(*size)) if size is not None else None, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    refused(b"null lo", lo=None)
    refused(b"null size", size=None)
    for size in ((256, 256, 257), (1 << 24, 2, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1 << 16, 1 << 16, 1), (4097, 4096, 1)):
        refused(b"size.x * size.y * size.z", size=size)
    refused(b"null out", o=None)
    refused(b"VX_MEM", memory=5)
    for off in (1, 2, 3):
        refused(b"out in device memory must be aligned to 4", memory=hip.VX_MEM_DEVICE, o=out.ctypes.data + off)
    # every rule kept: only the context is missing (the largest box; a box with no voxel needs no out; a negative corner; a host out at any address)
    refused(b"null context", size=(256, 256, 256))
    refused(b"null context", size=(1 << 24, 1, 1), memory=hip.VX_MEM_DEVICE)
    refused(b"null context", size=(0xFFFFFFFF, 0, 0xFFFFFFFF), o=None)
    refused(b"null context", lo=(-2147483648, 2147483647, -1))
    refused(b"null context", o=out.ctypes.data + 1)


def test_the_binding_describes_its_arguments():
    """Svo.block_points' view of its argument (no library call): addresses and byte strides of packed, padded and record-held positions."""
    e = np.zeros(5, dtype=hip.ENTITY_DTYPE)
    assert hip._ray_vectors("positions", hip.entity_positions(e), 5, 3) == (e.ctypes.data, 64)
    h = np.zeros(5, dtype=hip.RAY_HIT_DTYPE)
    assert hip._ray_vectors("positions", hip.ray_hit_positions(h), 5, 3) == (h.ctypes.data + 16, 32)
    o = np.zeros((5, 4), dtype=np.float32)
    assert hip._ray_vectors("positions", o[:, 1:4], 5, 3) == (o.ctypes.data + 4, 16)
