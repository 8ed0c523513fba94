"""vx_move_boxes without a GPU: the library exports it, both structs have the header's layout (a probe compiled from include/voxel_hip.h
with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, and the entry point's
argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C

import numpy as np

from abi_checks import Rust, probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p



def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_move_boxes")
    assert "vx_move_boxes" in hip.SYMBOLS and hip.lib().vx_move_boxes is not None
    assert len(hip.SYMBOLS["vx_move_boxes"][1]) == 8


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_move_shape": ["scale", "skin", "order", "flags"], "vx_move_hit": ["origin", "moved", "contacts", "value", "_pad"], "vx_entity": ["velocity"]},
                 ["VX_MOVE_INVALID", "VX_MOVE_ORDER_YXZ", "VX_MOVE_MAX_TRAVEL"])
    assert said["vx_move_hit"] == (48,) == (hip.MOVE_HIT_DTYPE.itemsize,)
    assert said["vx_move_shape"] == (16,) == (C.sizeof(hip.MoveShape),)
    assert said["VX_MOVE_INVALID"] == (0xFFFFFFFF,) == (hip.VX_MOVE_INVALID,)
    assert said["VX_MOVE_ORDER_YXZ"] == (hip.VX_MOVE_ORDER_YXZ,) == (1 | 0 << 2 | 2 << 4,)
    assert said["VX_MOVE_MAX_TRAVEL"] == (64,) == (hip.VX_MOVE_MAX_TRAVEL,)
    assert (hip.VX_MOVE_ORDER_XYZ, hip.VX_MOVE_ORDER_ZYX) == (0 | 1 << 2 | 2 << 4, 2 | 1 << 2 | 0 << 4)
    assert [n for n, _ in hip.MoveShape._fields_] == ["scale", "skin", "order", "flags"]
    for name, _ in hip.MoveShape._fields_:
        field = getattr(hip.MoveShape, name)
        assert said[f"vx_move_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.MOVE_HIT_DTYPE.names) == ["origin", "moved", "contacts", "value", "_pad"]
    for f, at, size, kind in (("origin", 0, 12, "<f4"), ("moved", 12, 12, "<f4"), ("contacts", 24, 4, "<u4"), ("value", 28, 12, "<u4"), ("_pad", 40, 8, "<u4")):
        dt, offset = hip.MOVE_HIT_DTYPE.fields[f][:2]
        assert said[f"vx_move_hit.{f}"] == (offset, dt.itemsize) == (at, size) and dt.base.str == kind, f
    # a vx_entity's velocity is read in place: entity_velocities' view lies where the header's field does
    e = np.zeros(3, dtype=hip.ENTITY_DTYPE)
    v = hip.entity_velocities(e)
    assert v.ctypes.data - e.ctypes.data == said["vx_entity.velocity"][0] and v.strides == (64, 4) and v.shape == (3, 3)
    s = hip.MOVE_SHAPE()
    assert (s.scale, s.skin, s.order, s.flags) == (1.0, 2.0 ** -10, hip.VX_MOVE_ORDER_YXZ, 0)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them in hexadecimal with a `u` suffix,
    and as a float)."""
    rust = Rust()
    assert rust.const("VX_MOVE_INVALID") == ("u32", "u32::MAX")
    assert rust.const("VX_MOVE_MAX_TRAVEL") == ("f32", "64.0")
    assert rust.const("VX_MOVE_ORDER_YXZ") == ("u32", "0x21")
    assert rust.struct("vx_move_hit") == [("origin", "[f32; 3]"), ("moved", "[f32; 3]"), ("contacts", "u32"), ("value", "[u32; 3]"), ("_pad", "[u32; 2]")]
    assert rust.struct("vx_move_shape") == [("scale", "f32"), ("skin", "f32"), ("order", "u32"), ("flags", "u32")]
    assert rust.asserts_size("vx_move_hit", 48) and rust.asserts_size("vx_move_shape", 16)
    assert rust.args("vx_move_boxes") == ["ctx", "boxes", "motion", "motion_stride", "count", "shape", "memory", "out"]


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records stay as they are."""
    L = hip.lib()
    out = np.full(48 * 4 + 16, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.float32)
    base = v.ctypes.data
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, o=out.ctypes.data, boxes=True, motion=base + 144, motion_stride=12, shape=True, **fields):
        b = hip.BoxBatch(base, base + 12 * 4, base + 24 * 4, 12, 12, 12, 0)
        s = hip.MOVE_SHAPE()
        for k, val in fields.items():
            setattr(s if hasattr(s, k) else b, k, val)
        return L.vx_move_boxes(None, C.byref(b) if boxes else None, _vp(motion), motion_stride, count, C.byref(s) if shape else None, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    refused(b"null shape", shape=False)
    refused(b"null shape", shape=False, count=0)
    refused(b"null motion", motion=None)
    refused(b"null boxes", boxes=False)
    refused(b"null out", o=None)
    refused(b"null origin", origin=None)
    refused(b"null extents", extents=None)
    refused(b"count exceeds", count=(1 << 24) + 1)
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"origin_stride", origin_stride=8)
    refused(b"offset_stride", offset_stride=13)
    refused(b"extents_stride", extents_stride=4)
    for stride in (4, 8, 13, 18):
        refused(b"motion_stride", motion_stride=stride)
    for off in (1, 2, 3):
        refused(b"motion must be aligned", motion=base + 144 + off)
        refused(b"origin must be aligned", origin=base + off)
    for scale in (float("inf"), float("-inf"), float("nan")):
        refused(b"scale", scale=scale)
    for skin in (-1e-6, 1.0000002, float("inf"), float("nan")):
        refused(b"skin", skin=skin)
    for order in (0, 0x15, 0x2a, 0x3f, 0x20, 0x23, 0x21 | 0x40, 0x21 | 0x100, 0x21 | 0x80000000):
        refused(b"order", order=order)
    for flags in (1, 2, 0x80000000):
        refused(b"flags", flags=flags)
    aligned = out.ctypes.data + (-out.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"out in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, o=aligned + off)
    # every rule kept: only the context is missing
    refused(b"null context", motion_stride=0)
    refused(b"null context", motion_stride=16)
    refused(b"null context", origin_stride=64, offset_stride=64, extents_stride=64, motion_stride=64, scale=1.0 / 64.0, only_value=0xFFFFFFFF)
    refused(b"null context", offset=None, offset_stride=7)
    refused(b"null context", scale=0.0, skin=0.0)
    refused(b"null context", scale=-1e30, skin=1.0)
    for order in (0x24, 0x18, 0x21, 0x09, 0x12, 0x06):
        refused(b"null context", order=order)
    refused(b"null context", count=1 << 24, memory=hip.VX_MEM_DEVICE, o=aligned)
    refused(b"null context", count=0, boxes=False, motion=None, o=None)
