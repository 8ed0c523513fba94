"""vx_light_boxes without a GPU: the library exports it, both structs have the header's layout (a probe compiled from include/voxel_hip.h with
gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_light's messages as the
host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from abi_checks import ROOT, Rust, probe, refusing
from helpers import vra  # noqa: F401
from light_cases import harness
from voxel_rs_amd import hip

_vp = C.c_void_p

CONSTANTS = {"VX_LIGHT_MAX_SIDE": 48, "VX_LIGHT_MAX_PROPS": 4096, "VX_LIGHT_TRANSPARENT": 0x10, "VX_LIGHT_NO_SKY": 1, "VX_LIGHT_NO_BLOCKS": 2,
             "VX_LIGHT_INVALID": 0xFFFFFFFF}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_light_boxes")
    assert "vx_light_boxes" in hip.SYMBOLS and hip.lib().vx_light_boxes is not None
    assert len(hip.SYMBOLS["vx_light_boxes"][1]) == 9


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_light_shape": ["size", "flags", "props", "props_count"], "vx_light_info": ["lit", "sources", "open_columns", "faces"]}, CONSTANTS)
    assert said["vx_light_info"] == (16,) == (hip.LIGHT_INFO_DTYPE.itemsize,)
    assert said["vx_light_shape"] == (32,) == (C.sizeof(hip.LightShape),)
    for name, value in CONSTANTS.items():
        assert said[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.LightShape._fields_] == ["size", "flags", "props", "props_count"]
    for name, _ in hip.LightShape._fields_:
        field = getattr(hip.LightShape, name)
        assert said[f"vx_light_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.LIGHT_INFO_DTYPE.names) == ["lit", "sources", "open_columns", "faces"]
    for k, f in enumerate(hip.LIGHT_INFO_DTYPE.names):
        dt, offset = hip.LIGHT_INFO_DTYPE.fields[f][:2]
        assert said[f"vx_light_info.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s, table = hip.light_shape((33, 9, 17), [0, 15, 0x14], flags=2)
    assert (list(s.size), s.flags, s.props, s.props_count) == ([33, 9, 17], 2, table.ctypes.data, 3) and table.tolist() == [0, 15, 0x14]
    s, table = hip.light_shape((1, 1, 1), [])
    assert s.props is None and s.props_count == 0


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them with a `u` suffix)."""
    rust = Rust()
    for name, value in CONSTANTS.items():
        kind, got = rust.const_int(name)
        assert kind in ("u8", "u32") and got == value, name
    assert rust.struct("vx_light_info") == [("lit", "u32"), ("sources", "u32"), ("open_columns", "u32"), ("faces", "u32")]
    assert rust.struct("vx_light_shape") == [("size", "[u32; 3]"), ("flags", "u32"), ("props", "*const u8"), ("props_count", "u32")]
    assert rust.asserts_size("vx_light_info", 16) and rust.asserts_size("vx_light_shape", 32)
    assert rust.args("vx_light_boxes") == ["ctx", "lo", "lo_stride", "count", "shape", "memory", "fields", "field_stride", "info"]


def test_check_light_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["stride 64"] == said["fields only"] == said["info only"] == said["count 0"] == "ok"
    assert said["too many"] == "count exceeds 16777216 (2^24)"
    assert said["lo_stride 8"] == "lo_stride must be a multiple of 4 and >= 12"
    assert said["lo + 2"] == "lo must be aligned to 4 bytes"
    assert said["size[1] 49"] == "size: every component must be 1..48"
    assert said["flags 4"] == "flags holds a bit other than VX_LIGHT_NO_SKY and VX_LIGHT_NO_BLOCKS"
    assert said["flags 3"] == "flags: VX_LIGHT_NO_SKY and VX_LIGHT_NO_BLOCKS together leave nothing to do"
    assert said["props_count 4097"] == "props_count exceeds VX_LIGHT_MAX_PROPS (4096)"
    assert said["null props"] == "null props with props_count > 0"
    assert said["props byte 64"] == "props: a byte has one of bits 5..7 set"
    assert said["field_stride 4080"] == "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z"
    assert said["field bytes 2^24 + 8192"] == "count * field_stride exceeds 16777216 (2^24) bytes"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled outputs stay as they are."""
    L = hip.lib()
    fields = np.full(2 * 4096 + 32, 0x5a, dtype=np.uint8)
    info = np.full(3 * 16, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.int32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    good = np.array([0, 15, 4, 0x10, 0x19], dtype=np.uint8)
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, lo=base, lo_stride=12, f=fields.ctypes.data, field_stride=0, i=info.ctypes.data, shape=True, table=good, **shape_fields):
        s, keep = hip.light_shape((16, 16, 16), table)
        for k, val in shape_fields.items():
            setattr(s, k, val)
        rc = L.vx_light_boxes(None, lo, lo_stride, count, C.byref(s) if shape else None, memory, f, field_stride, i)
        del keep
        return rc

    refused = refusing(L, call, (fields, info))
    refused(b"null context")
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"null shape", shape=False)
    refused(b"null lo", lo=None)
    refused(b"fields and info are both null", f=None, i=None)
    refused(b"count exceeds", count=(1 << 24) + 1)
    for stride in (0, 4, 8, 13, 18):
        refused(b"lo_stride", lo_stride=stride)
    for off in (1, 2, 3):
        refused(b"lo must be aligned", lo=base + off)
    for a in range(3):
        for side in (0, 49, 0xFFFFFFFF):
            size = [16, 16, 16]
            size[a] = side
            refused(b"size", size=u3(*size))
    for flags in (3, 4, 0x80000000):
        refused(b"flags", flags=flags)
    refused(b"props_count", props_count=4097)
    refused(b"null props", props=None)
    for bit in (0x20, 0x40, 0x80):
        for at in (0, 2, 4):
            table = good.copy()
            table[at] |= bit
            refused(b"props: a byte", table=table)
    for stride in (4097, 4104, 4080, 16):
        refused(b"field_stride", field_stride=stride)
    refused(b"count * field_stride", count=4097)
    refused(b"count * field_stride", count=2049, field_stride=8192)
    f16 = fields.ctypes.data + (-fields.ctypes.data) % 16
    i16 = info.ctypes.data + (-info.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"fields in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16 + off, i=i16)
        refused(b"info in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, i=i16 + off)
    # every rule kept: only the context is missing
    refused(b"null context", f=None)
    refused(b"null context", i=None, field_stride=4096 + 16)
    refused(b"null context", f=None, field_stride=7, count=1 << 24)  # (no fields: their stride is not looked at)
    refused(b"null context", lo_stride=64, size=u3(48, 48, 48), flags=1, count=151)
    refused(b"null context", size=u3(1, 1, 1), flags=2, count=1 << 20)
    refused(b"null context", table=np.zeros(0, dtype=np.uint8))
    refused(b"null context", table=np.full(4096, 0x1f, dtype=np.uint8))
    refused(b"null context", memory=hip.VX_MEM_DEVICE, f=f16, i=i16)
    refused(b"null context", f=fields.ctypes.data + 1, i=info.ctypes.data + 1)  # (host memory needs no alignment)
    refused(b"null context", count=0, shape=False, lo=None, f=None, i=None)
