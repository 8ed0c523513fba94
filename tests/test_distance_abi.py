"""vx_distance_boxes without a GPU: the library exports it, its two structs have the header's layout (a probe compiled from
include/voxel_hip.h with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them,
check_distance's messages as the host harness prints them, and the entry point's argument checks, which come before any HIP call, name the
field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from abi_checks import ROOT, Rust, probe, refusing
from distance_cases import harness
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

SHAPE_FIELDS = ["size", "pass_value", "match_value", "flags", "_pad"]
INFO_FIELDS = ["targets", "farthest", "where", "faces"]
CONSTANTS = {"VX_DISTANCE_NONE": 0xFFFF, "VX_DISTANCE_TO_AIR": 1}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_distance_boxes")
    assert "vx_distance_boxes" in hip.SYMBOLS and hip.lib().vx_distance_boxes is not None
    assert len(hip.SYMBOLS["vx_distance_boxes"][1]) == 9


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_distance_shape": SHAPE_FIELDS, "vx_distance_info": INFO_FIELDS}, CONSTANTS)
    assert said["vx_distance_info"] == (16,) == (hip.DISTANCE_INFO_DTYPE.itemsize,)
    assert said["vx_distance_shape"] == (32,) == (C.sizeof(hip.DistanceShape),)
    for name, value in CONSTANTS.items():
        assert said[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.DistanceShape._fields_] == SHAPE_FIELDS
    for name, _ in hip.DistanceShape._fields_:
        field = getattr(hip.DistanceShape, name)
        assert said[f"vx_distance_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.DISTANCE_INFO_DTYPE.names) == INFO_FIELDS
    for k, f in enumerate(INFO_FIELDS):
        dt, offset = hip.DISTANCE_INFO_DTYPE.fields[f][:2]
        assert said[f"vx_distance_info.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.distance_shape((31, 3, 17), 9, 0, 1)
    assert (list(s.size), s.pass_value, s.match_value, s.flags, list(s._pad)) == ([31, 3, 17], 9, 0, 1, [0, 0])
    s = hip.distance_shape((1, 1, 1))
    assert (s.pass_value, s.match_value, s.flags) == (0, 0, 0)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them with a `u` suffix)."""
    rust = Rust()
    for name, value in CONSTANTS.items():
        kind, got = rust.const_int(name)
        assert kind in ("u16", "u32") and got == value, name
    assert rust.struct("vx_distance_info") == [(n, "u32") for n in INFO_FIELDS]
    assert rust.struct("vx_distance_shape") == [("size", "[u32; 3]")] + [(n, "u32") for n in SHAPE_FIELDS[1:-1]] + [("_pad", "[u32; 2]")]
    assert rust.asserts_size("vx_distance_info", 16) and rust.asserts_size("vx_distance_shape", 32)
    assert rust.args("vx_distance_boxes") == ["ctx", "lo", "lo_stride", "count", "shape", "memory", "fields", "field_stride", "info"]
    header = (ROOT / "include" / "voxel_hip.h").read_text()
    assert header.index("int vx_label_boxes(") < header.index("int vx_distance_boxes(") < header.index("int vx_physics_step(")


def test_check_distance_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["stride 64"] == said["fields only"] == said["info only"] == said["count 0"] == said["count 2^20"] == "ok"
    assert said["too many"] == "count exceeds 1048576 (2^20)"
    assert said["lo_stride 8"] == "lo_stride must be a multiple of 4 and >= 12"
    assert said["lo + 2"] == "lo must be aligned to 4 bytes"
    assert said["size[1] 33"] == "size: every component must be 1..32"
    assert said["flags 2"] == "flags holds a bit other than VX_DISTANCE_TO_AIR"
    assert said["match_value with pass_value"] == "pass_value must be 0 with a match_value"
    assert said["field_stride 8176"] == "field_stride must be 0, or a multiple of 16 and at least 2 * size.x * size.y * size.z"
    assert said["field bytes 2^24 + 8192"] == "count * field_stride exceeds 16777216 (2^24) bytes"
    assert said["fields on lo"] == "fields overlaps lo" and said["info on lo"] == "info overlaps lo" and said["fields on info"] == "fields overlaps info"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled outputs stay as they are."""
    L = hip.lib()
    fields = np.full(2 * 8192 + 32, 0x5a, dtype=np.uint8)
    info = np.full(3 * 16, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.int32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, lo=base, lo_stride=12, f=fields.ctypes.data, field_stride=0, i=info.ctypes.data, shape=True, **shape_fields):
        s = hip.distance_shape((16, 16, 16))
        for k, val in shape_fields.items():
            setattr(s, k, val)
        return L.vx_distance_boxes(None, lo, lo_stride, count, C.byref(s) if shape else None, memory, f, field_stride, i)

    refused = refusing(L, call, (fields, info))
    refused(b"null context")
    refused(b"distance_boxes", f=None, i=None)  # (the call is named in front of what it refuses)
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"null shape", shape=False)
    refused(b"null lo", lo=None)
    refused(b"fields and info are both null", f=None, i=None)
    refused(b"count exceeds 1048576", count=(1 << 20) + 1, f=None)
    for stride in (0, 4, 8, 13, 18):
        refused(b"lo_stride", lo_stride=stride)
    for off in (1, 2, 3):
        refused(b"lo must be aligned", lo=base + off)
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            size = [16, 16, 16]
            size[a] = side
            refused(b"size", size=u3(*size))
    for flags in (2, 3, 0x80000000):
        refused(b"flags", flags=flags)
    refused(b"pass_value must be 0 with a match_value", pass_value=9, match_value=3)
    for stride in (8193, 8200, 8176, 4096, 16):
        refused(b"field_stride", field_stride=stride)
    refused(b"count * field_stride", count=2049, i=None)
    refused(b"count * field_stride", count=1025, field_stride=16384, i=None)
    refused(b"fields overlaps lo", lo=fields.ctypes.data + (-fields.ctypes.data) % 4)
    refused(b"info overlaps lo", i=base + 16)
    refused(b"fields overlaps info", i=fields.ctypes.data + 16384 - 1)
    f16 = fields.ctypes.data + (-fields.ctypes.data) % 16
    i16 = info.ctypes.data + (-info.ctypes.data) % 16
    for off in (1, 2, 4, 8, 12):
        refused(b"fields in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16 + off, i=i16)
        refused(b"info in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, i=i16 + off)
    # every rule kept: only the context is missing
    refused(b"null context", f=None)
    refused(b"null context", i=None, field_stride=8192 + 16)
    refused(b"null context", f=None, field_stride=7, count=3)  # (no fields: their stride is not looked at)
    refused(b"null context", lo_stride=16, size=u3(32, 32, 32), count=1, f=None, flags=1)
    refused(b"null context", size=u3(1, 1, 1), pass_value=0xFFFFFFFF)
    refused(b"null context", match_value=0xFFFFFFFF, flags=1)
    refused(b"null context", memory=hip.VX_MEM_DEVICE, f=f16, i=i16)
    refused(b"null context", f=fields.ctypes.data + 1, i=info.ctypes.data + 1)  # (host memory needs no alignment)
    refused(b"null context", count=0, shape=False, lo=None, f=None, i=None)
