"""vx_scan_points and vx_scan_columns without a GPU: the library exports them, the binding's record has the header's layout (a size, offset and
constant probe compiled from include/voxel_hip.h with gcc, the way the C-ABI client is compiled), and the entry points' argument checks,
which come before any HIP call, name the field they refuse."""
import ctypes as C

import numpy as np

from abi_checks import probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p



def test_the_library_exports_them():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    for name in ("vx_scan_points", "vx_scan_columns"):
        assert hasattr(L, name)
        assert name in hip.SYMBOLS and getattr(hip.lib(), name) is not None


def test_the_record_has_the_headers_layout(tmp_path):
    constants = ["VX_DIR_NEG_X", "VX_DIR_POS_X", "VX_DIR_NEG_Y", "VX_DIR_POS_Y", "VX_DIR_NEG_Z", "VX_DIR_POS_Z", "VX_SCAN_NONE", "VX_SCAN_TO_EDGE", "VX_CELL_OUTSIDE"]
    said = probe(tmp_path, {"vx_scan_hit": ["coord", "value", "cell_log2", "_pad"]}, constants,
                 more=r'    printf("none_is_int32 %d\n", (int)(sizeof(VX_SCAN_NONE) == 4 && VX_SCAN_NONE < 0));')
    assert said["vx_scan_hit"] == (16,) == (hip.SCAN_HIT_DTYPE.itemsize,)
    assert list(hip.SCAN_HIT_DTYPE.names) == ["coord", "value", "cell_log2", "_pad"]
    for f, at, kind in (("coord", 0, "<i4"), ("value", 4, "<u4"), ("cell_log2", 8, "<u4"), ("_pad", 12, "<u4")):
        dt, offset = hip.SCAN_HIT_DTYPE.fields[f][:2]
        assert said[f"vx_scan_hit.{f}"] == (offset, dt.itemsize) == (at, 4) and dt.str == kind, f
    for k, name in enumerate(("VX_DIR_NEG_X", "VX_DIR_POS_X", "VX_DIR_NEG_Y", "VX_DIR_POS_Y", "VX_DIR_NEG_Z", "VX_DIR_POS_Z")):
        assert said[name] == (getattr(hip, name),) == (k,)
    assert said["VX_SCAN_NONE"] == (hip.VX_SCAN_NONE,) == (-(1 << 31),) and said["none_is_int32"] == (1,)
    assert said["VX_SCAN_TO_EDGE"] == (hip.VX_SCAN_TO_EDGE,) == (0xFFFFFFFF,)
    assert said["VX_CELL_OUTSIDE"] == (hip.VX_CELL_OUTSIDE,)
    assert np.array([hip.VX_SCAN_NONE], dtype=hip.SCAN_HIT_DTYPE["coord"])[0] == hip.VX_SCAN_NONE


def test_scan_points_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records stay as they are."""
    L = hip.lib()
    pos = np.zeros((4, 4), dtype=np.float32)
    out = np.full(4 * 16 + 16, 0x5a, dtype=np.uint8)
    base = out.ctypes.data + (-out.ctypes.data) % 16

    def call(p=pos.ctypes.data, stride=12, count=4, direction=hip.VX_DIR_NEG_Y, reach=hip.VX_SCAN_TO_EDGE, memory=hip.VX_MEM_HOST, o=base):
        return L.vx_scan_points(None, _vp(p), stride, count, direction, reach, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    for stride in (0, 4, 8, 13, 14, 18, 2):
        refused(b"pos_stride", stride=stride)
    for off in (1, 2, 3):
        refused(b"pos must be aligned", p=pos.ctypes.data + off)
    refused(b"null pos", p=None)
    refused(b"null out", o=None)
    refused(b"count", count=(1 << 24) + 1)
    refused(b"reach", reach=0)
    for direction in (-1, 6, 7, 1 << 20):
        refused(b"direction", direction=direction)
    refused(b"VX_MEM", memory=2)
    refused(b"VX_MEM", memory=-1)
    for off in (1, 2, 4, 8, 12):
        refused(b"out in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, o=base + off)
    # every rule kept: only the context is missing (records inside vx_entity and vx_ray_hit; every direction; the largest count; the smallest
    # reach; a host out at any address)
    refused(b"null context", stride=64)
    refused(b"null context", p=pos.ctypes.data + 16, stride=32, memory=hip.VX_MEM_DEVICE)
    for direction in range(6):
        refused(b"null context", direction=direction, reach=1)
    refused(b"null context", count=1 << 24)
    refused(b"null context", o=base + 1)
    assert L.vx_scan_points(None, None, 12, 0, 0, 1, hip.VX_MEM_HOST, None) == 1 and b"null context" in L.vx_last_error()
    # no points: nothing is read or written, so no stride, alignment, pointer or reach is refused -- only the context is missing
    refused(b"null context", p=pos.ctypes.data + 1, stride=5, count=0, reach=0, memory=hip.VX_MEM_DEVICE, o=base + 3)
    refused(b"VX_MEM", count=0, memory=7)
    refused(b"direction", count=0, direction=6)


def test_scan_columns_argument_checks_need_no_device():
    L = hip.lib()
    out = np.full(8 * 16 + 16, 0x5a, dtype=np.uint8)
    base = out.ctypes.data + (-out.ctypes.data) % 16
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def call(lo=(-3, 0, 5), size=(4, 2, 2), direction=hip.VX_DIR_NEG_Y, memory=hip.VX_MEM_HOST, o=base):
        return L.vx_scan_columns(None, C.byref(i3(*lo)) if lo is not None else None, C.byref(u3(*size)) if size is not None else None, direction, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    refused(b"null lo", lo=None)
    refused(b"null size", size=None)
    for direction in (-1, 6, 7, 1 << 20):
        refused(b"direction", direction=direction)
    # size[u] * size[v] beyond 2^24, for each axis; size[a] beyond 2^24
    for direction, size in ((hip.VX_DIR_NEG_Y, (4097, 1, 4096)), (hip.VX_DIR_POS_Y, (1 << 16, 3, 1 << 16)), (hip.VX_DIR_NEG_X, (1, 4097, 4096)), (hip.VX_DIR_POS_Z, ((1 << 24) + 1, 1, 7)),
                            (hip.VX_DIR_NEG_Z, (0xFFFFFFFF, 0xFFFFFFFF, 1))):
        refused(b"size", direction=direction, size=size)
        assert b"columns" in L.vx_last_error()
    for direction, size in ((hip.VX_DIR_NEG_Y, (2, (1 << 24) + 1, 2)), (hip.VX_DIR_POS_X, (0xFFFFFFFF, 1, 1)), (hip.VX_DIR_NEG_Z, (1, 1, (1 << 24) + 1))):
        refused(b"size", direction=direction, size=size)
        assert b"along the scan axis" in L.vx_last_error()
    refused(b"null out", o=None)
    refused(b"VX_MEM", memory=5)
    for off in (1, 2, 4, 8):
        refused(b"out in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, o=base + off)
    # every rule kept: only the context is missing (the largest footprint and extent; a box with no voxel needs no out; a negative corner;
    # every direction; a host out at any address)
    refused(b"null context", size=(4096, 1 << 24, 4096))
    refused(b"null context", size=(1 << 24, 1 << 24, 1), direction=hip.VX_DIR_POS_Y, memory=hip.VX_MEM_DEVICE)
    refused(b"null context", size=(0xFFFFFFFF, 0, 0xFFFFFFFF), o=None)
    refused(b"null context", size=(0, 5, 5), direction=hip.VX_DIR_NEG_X, o=None)
    refused(b"null context", lo=(-2147483648, 2147483647, -1))
    for direction in range(6):
        refused(b"null context", direction=direction)
    refused(b"null context", o=base + 1)
