"""vx_flood_points without a GPU: the library exports it, both structs have the header's layout (a probe compiled from include/voxel_hip.h with
gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_flood's messages as the
host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from flood_cases import harness
from abi_checks import ROOT, Rust, probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p

CONSTANTS = {"VX_FLOOD_MAX_STEPS": 250, "VX_FLOOD_NO_POSITION": 0xFD, "VX_FLOOD_UNREACHED": 0xFE, "VX_FLOOD_BLOCKED": 0xFF, "VX_FLOOD_SEED_ALWAYS": 1,
             "VX_FLOOD_INVALID": 0xFFFFFFFF}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_flood_points")
    assert "vx_flood_points" in hip.SYMBOLS and hip.lib().vx_flood_points is not None
    assert len(hip.SYMBOLS["vx_flood_points"][1]) == 9


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_flood_shape": ["size", "seed_at", "max_steps", "pass_value", "flags"], "vx_flood_info": ["reached", "farthest", "faces", "seed_value"]}, CONSTANTS)
    assert said["vx_flood_info"] == (16,) == (hip.FLOOD_INFO_DTYPE.itemsize,)
    assert said["vx_flood_shape"] == (36,) == (C.sizeof(hip.FloodShape),)
    for name, value in CONSTANTS.items():
        assert said[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.FloodShape._fields_] == ["size", "seed_at", "max_steps", "pass_value", "flags"]
    for name, _ in hip.FloodShape._fields_:
        field = getattr(hip.FloodShape, name)
        assert said[f"vx_flood_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.FLOOD_INFO_DTYPE.names) == ["reached", "farthest", "faces", "seed_value"]
    for k, f in enumerate(hip.FLOOD_INFO_DTYPE.names):
        dt, offset = hip.FLOOD_INFO_DTYPE.fields[f][:2]
        assert said[f"vx_flood_info.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.flood_shape((31, 3, 17), max_steps=24, pass_value=9, flags=1)
    assert (list(s.size), list(s.seed_at), s.max_steps, s.pass_value, s.flags) == ([31, 3, 17], [15, 1, 8], 24, 9, 1)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them in hexadecimal with a `u` suffix)."""
    rust = Rust()
    for name, value in CONSTANTS.items():
        kind = "u8" if name in ("VX_FLOOD_NO_POSITION", "VX_FLOOD_UNREACHED", "VX_FLOOD_BLOCKED") else "u32"
        assert rust.const_int(name) == (kind, value), name
    assert rust.struct("vx_flood_info") == [("reached", "u32"), ("farthest", "u32"), ("faces", "u32"), ("seed_value", "u32")]
    assert rust.struct("vx_flood_shape") == [("size", "[u32; 3]"), ("seed_at", "[u32; 3]"), ("max_steps", "u32"), ("pass_value", "u32"), ("flags", "u32")]
    assert rust.asserts_size("vx_flood_info", 16) and rust.asserts_size("vx_flood_shape", 36)
    assert rust.args("vx_flood_points") == ["ctx", "pos", "pos_stride", "count", "shape", "memory", "fields", "field_stride", "info"]


def test_check_flood_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["entities"] == said["fields only"] == said["info only"] == said["count 0"] == "ok"
    assert said["too many"] == "count exceeds 16777216 (2^24)"
    assert said["pos_stride 8"] == "pos_stride must be a multiple of 4 and >= 12"
    assert said["size[1] 33"] == "size: every component must be 1..32"
    assert said["seed_at[2] 17"] == "seed_at: every component must be below size's"
    assert said["max_steps 251"] == "max_steps exceeds VX_FLOOD_MAX_STEPS (250)"
    assert said["flags 2"] == "flags holds a bit other than VX_FLOOD_SEED_ALWAYS"
    assert said["field_stride 4912"] == "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z"
    assert said["field bytes 2^24 + 8192"] == "count * field_stride exceeds 16777216 (2^24) bytes"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled outputs stay as they are."""
    L = hip.lib()
    fields = np.full(2 * 4928 + 32, 0x5a, dtype=np.uint8)
    info = np.full(3 * 16, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.float32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, pos=base, pos_stride=12, f=fields.ctypes.data, field_stride=0, i=info.ctypes.data, shape=True, **shape_fields):
        s = hip.flood_shape((17, 17, 17), (8, 8, 8), 250)
        for k, val in shape_fields.items():
            setattr(s, k, val)
        return L.vx_flood_points(None, pos, pos_stride, count, C.byref(s) if shape else None, memory, f, field_stride, i)

    refused = refusing(L, call, (fields, info))
    refused(b"null context")
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"null shape", shape=False)
    refused(b"null pos", pos=None)
    refused(b"fields and info are both null", f=None, i=None)
    refused(b"count exceeds", count=(1 << 24) + 1)
    for stride in (0, 4, 8, 13, 18):
        refused(b"pos_stride", pos_stride=stride)
    for off in (1, 2, 3):
        refused(b"pos must be aligned", pos=base + off)
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            size, seed_at = [17, 17, 17], [8, 8, 8]
            size[a], seed_at[a] = side, 0
            refused(b"size", size=u3(*size), seed_at=u3(*seed_at))
        seed_at = [8, 8, 8]
        seed_at[a] = 17
        refused(b"seed_at", seed_at=u3(*seed_at))
    refused(b"max_steps", max_steps=251)
    refused(b"max_steps", max_steps=0xFFFFFFFF)
    for flags in (2, 3, 0x80000000):
        refused(b"flags", flags=flags)
    for stride in (4913, 4920, 4912, 16):
        refused(b"field_stride", field_stride=stride)
    refused(b"count * field_stride", count=3405)
    refused(b"count * field_stride", count=2049, field_stride=8192)
    f16 = fields.ctypes.data + (-fields.ctypes.data) % 16
    i16 = info.ctypes.data + (-info.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"fields in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16 + off, i=i16)
        refused(b"info in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, i=i16 + off)
    # every rule kept: only the context is missing
    refused(b"null context", f=None)
    refused(b"null context", i=None, field_stride=4928 + 16)
    refused(b"null context", f=None, field_stride=7, count=1 << 24)  # (no fields: their stride is not looked at)
    refused(b"null context", pos_stride=64, size=u3(32, 32, 32), seed_at=u3(31, 31, 31), max_steps=0, pass_value=0xFFFFFFFF, flags=1, count=512)
    refused(b"null context", size=u3(1, 1, 1), seed_at=u3(0, 0, 0), count=1 << 20)
    refused(b"null context", memory=hip.VX_MEM_DEVICE, f=f16, i=i16)
    refused(b"null context", f=fields.ctypes.data + 1, i=info.ctypes.data + 1)  # (host memory needs no alignment)
    refused(b"null context", count=0, shape=False, pos=None, f=None, i=None)
