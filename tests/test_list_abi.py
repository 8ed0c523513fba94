"""vx_list_region without a GPU: the library exports it, the record and the macros have the header's layout and values (a probe compiled from
include/voxel_hip.h with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, and the
entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import re

import numpy as np

from abi_checks import Rust, probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p

# VX_AT_INDEX and VX_AT_FACES on words of the test's own
MACROS = r'''    printf("index %lu\nfaces %lu\nabove %lu\n", (unsigned long)VX_AT_INDEX(0xEAFEDCBAu), (unsigned long)VX_AT_FACES(0xEAFEDCBAu), (unsigned long)VX_AT_FACES(0xC0000000u));'''


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_list_region")
    assert "vx_list_region" in hip.SYMBOLS and hip.lib().vx_list_region is not None
    assert len(hip.SYMBOLS["vx_list_region"][1]) == 8


def test_the_record_and_the_macros_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_block_at": ["where", "value"]}, ["VX_LIST_FACES", "VX_LIST_EXPOSED"], more=MACROS)
    assert said["vx_block_at"] == (8,) == (hip.BLOCK_AT_DTYPE.itemsize,)
    assert said["VX_LIST_FACES"] == (1,) == (hip.VX_LIST_FACES,) and said["VX_LIST_EXPOSED"] == (2,) == (hip.VX_LIST_EXPOSED,)
    assert list(hip.BLOCK_AT_DTYPE.names) == ["where", "value"]
    for f, at in (("where", 0), ("value", 4)):
        dt, offset = hip.BLOCK_AT_DTYPE.fields[f][:2]
        assert said[f"vx_block_at.{f}"] == (offset, dt.itemsize) == (at, 4) and dt.str == "<u4", f
    # VX_AT_INDEX: the low 24 bits; VX_AT_FACES: the six above them, and nothing of bits 30..31
    assert said["index"] == (0xFEDCBA,) and said["faces"] == (0x2A,) and said["above"] == (0,)
    assert hip.split_where(0xEAFEDCBA) == (0xFEDCBA, 0x2A) and hip.split_where(0xC0000000) == (0, 0)
    index, faces = hip.split_where(np.array([0xEAFEDCBA, 0x3F000001], dtype=np.uint32))
    assert index.tolist() == [0xFEDCBA, 1] and faces.tolist() == [0x2A, 0x3F]


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the flag constants (the header writes them with a `u` suffix) and the
    helpers that stand for the two macros."""
    rust = Rust()
    consts = {k: int(v, 0) for k, v in re.findall(r"pub const (VX_LIST_\w+)\s*:\s*u32\s*=\s*(\w+)\s*;", rust.text)}
    assert consts == {"VX_LIST_FACES": hip.VX_LIST_FACES, "VX_LIST_EXPOSED": hip.VX_LIST_EXPOSED}
    assert rust.struct("vx_block_at") == [("where", "u32"), ("value", "u32")]
    assert rust.asserts_size("vx_block_at", 8)
    assert re.search(r"fn vx_at_index\(at: u32\) -> u32 \{ at & 0xFF_FFFF \}", rust.text) and re.search(r"fn vx_at_faces\(at: u32\) -> u32 \{ \(at >> 24\) & 0x3F \}", rust.text)
    assert rust.args("vx_list_region") == ["ctx", "lo", "size", "flags", "memory", "out", "capacity", "total"]


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records and total stay as they are."""
    L = hip.lib()
    out = np.full(64 + 8, 0x5a, dtype=np.uint8)
    total = np.full(8, 0x5a, dtype=np.uint8)
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def call(lo=(-3, 0, 5), size=(4, 2, 2), flags=0, memory=hip.VX_MEM_HOST, o=out.ctypes.data, capacity=8, t=total.ctypes.data):
        return L.vx_list_region(None, C.byref(i3(*lo)) if lo is not None else None, C.byref(u3(*size)) if size is not None else None, flags, memory, _vp(o),
                              capacity, _vp(t))

    refused = refusing(L, call, (out, total))

    refused(b"null context")
    refused(b"null lo", lo=None)
    refused(b"null size", size=None)
    for size in ((256, 256, 257), (1 << 24, 2, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1 << 16, 1 << 16, 1), (4097, 4096, 1)):
        refused(b"size.x * size.y * size.z", size=size)
    for flags in (4, 7, 8, 0x80000000, 0xFFFFFFFF):
        refused(b"flags", flags=flags)
    refused(b"flags", flags=4, size=(2, 0, 2))  # (an unknown bit is refused whatever the box)
    refused(b"null total", t=None)
    refused(b"null total", t=None, capacity=0, o=None)
    refused(b"null out", o=None)
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    assert out.ctypes.data % 8 == 0 and total.ctypes.data % 4 == 0
    for off in (1, 2, 4, 6):
        refused(b"out in device memory must be aligned to 8", memory=hip.VX_MEM_DEVICE, o=out.ctypes.data + off)
    for off in (1, 2, 3):
        refused(b"total in device memory must be aligned to 4", memory=hip.VX_MEM_DEVICE, t=total.ctypes.data + off)
    # every rule kept: only the context is missing (every flag set; the largest box; counting only with no out; a box with no voxel needs neither
    # out nor total; a negative corner; host memory at any address)
    for flags in (1, 2, 3):
        refused(b"null context", flags=flags)
    refused(b"null context", size=(256, 256, 256))
    refused(b"null context", size=(1, 1, 1 << 24), memory=hip.VX_MEM_DEVICE)
    refused(b"null context", o=None, capacity=0)
    refused(b"null context", size=(0xFFFFFFFF, 0, 0xFFFFFFFF), o=None, t=None)
    refused(b"null context", lo=(-2147483648, 2147483647, -1))
    refused(b"null context", o=out.ctypes.data + 1, t=total.ctypes.data + 1)
    refused(b"null context", capacity=0xFFFFFFFF)
