"""vx_walk_points without a GPU: the library exports it, both structs have the header's layout (a probe compiled from include/voxel_hip.h with
gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_walk's messages as the
host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from abi_checks import ROOT, Rust, probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip
from walk_cases import harness

_vp = C.c_void_p

SHAPE_FIELDS = ["size", "seed_at", "max_steps", "pass_value", "height", "climb", "drop", "path_capacity", "flags"]
INFO_FIELDS = ["reached", "farthest", "faces", "seed_value", "start_ry", "goal_ry", "path_steps", "_pad"]
CONSTANTS = {"VX_WALK_MAX_STEPS": 250, "VX_WALK_NO_POSITION": 0xFD, "VX_WALK_UNREACHED": 0xFE, "VX_WALK_NO_STAND": 0xFF, "VX_WALK_STOP_AT_GOAL": 1, "VX_WALK_NONE": 0xFFFFFFFF}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_walk_points")
    assert "vx_walk_points" in hip.SYMBOLS and hip.lib().vx_walk_points is not None
    assert len(hip.SYMBOLS["vx_walk_points"][1]) == 12


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_walk_shape": SHAPE_FIELDS, "vx_walk_info": INFO_FIELDS}, CONSTANTS)
    assert said["vx_walk_info"] == (32,) == (hip.WALK_INFO_DTYPE.itemsize,)
    assert said["vx_walk_shape"] == (52,) == (C.sizeof(hip.WalkShape),)
    for name, value in CONSTANTS.items():
        assert said[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.WalkShape._fields_] == SHAPE_FIELDS
    for name, _ in hip.WalkShape._fields_:
        field = getattr(hip.WalkShape, name)
        assert said[f"vx_walk_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.WALK_INFO_DTYPE.names) == INFO_FIELDS
    for k, f in enumerate(hip.WALK_INFO_DTYPE.names):
        dt, offset = hip.WALK_INFO_DTYPE.fields[f][:2]
        assert said[f"vx_walk_info.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.walk_shape((31, 3, 17), max_steps=24, pass_value=9, height=1, climb=0, drop=2, path_capacity=8, flags=1)
    assert (list(s.size), list(s.seed_at), s.max_steps, s.pass_value, s.height, s.climb, s.drop, s.path_capacity, s.flags) == ([31, 3, 17], [15, 1, 8], 24, 9, 1, 0, 2, 8, 1)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them in hexadecimal with a `u` suffix)."""
    rust = Rust()
    for name, value in CONSTANTS.items():
        kind = "u8" if name in ("VX_WALK_NO_POSITION", "VX_WALK_UNREACHED", "VX_WALK_NO_STAND") else "u32"
        assert rust.const_int(name) == (kind, value), name
    assert rust.struct("vx_walk_info") == [(f, "u32") for f in INFO_FIELDS]
    assert rust.struct("vx_walk_shape") == [("size", "[u32; 3]"), ("seed_at", "[u32; 3]")] + [(f, "u32") for f in SHAPE_FIELDS[2:]]
    assert rust.asserts_size("vx_walk_info", 32) and rust.asserts_size("vx_walk_shape", 52)
    assert rust.args("vx_walk_points") == ["ctx", "pos", "pos_stride", "goal", "goal_stride", "count", "shape", "memory", "fields", "field_stride",
                                                                   "paths", "info"]


def test_check_walk_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["entities"] == said["fields only"] == said["info only"] == said["paths only"] == said["count 0"] == said["one goal"] == "ok"
    assert said["too many"] == "count exceeds 16777216 (2^24)"
    assert said["no output"] == "fields, info and paths are all null"
    assert said["paths without goal"] == "paths without goal"
    assert said["pos_stride 8"] == "pos_stride must be a multiple of 4 and >= 12"
    assert said["goal_stride 8"] == "goal_stride must be 0, or a multiple of 4 and >= 12"
    assert said["goal + 2"] == "goal must be aligned to 4 bytes"
    assert said["size[1] 33"] == "size: every component must be 1..32"
    assert said["seed_at[2] 17"] == "seed_at: every component must be below size's"
    assert said["height 5"] == "height must be 1..4"
    assert said["31 layers and 2"] == "size[1] + height exceeds 32"
    assert said["max_steps 251"] == "max_steps exceeds VX_WALK_MAX_STEPS (250)"
    assert said["climb 2"] == "climb must be 0 or 1"
    assert said["drop 4"] == "drop must be 0..3"
    assert said["path_capacity 6"] == said["path_capacity 256"] == "path_capacity must be a multiple of 4 and at most 252"
    assert said["flags 2"] == "flags holds a bit other than VX_WALK_STOP_AT_GOAL"
    assert said["field_stride 3456"] == "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z"
    assert said["field bytes 2^24 + 4096"] == "count * field_stride exceeds 16777216 (2^24) bytes"
    assert said["path bytes beyond 2^24"] == "count * path_capacity * 4 exceeds 16777216 (2^24) bytes"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled outputs stay as they are."""
    L = hip.lib()
    fields = np.full(2 * 3472 + 32, 0x5a, dtype=np.uint8)
    paths = np.full(2 * 252 + 8, 0x5a5a5a5a, dtype=np.uint32)
    info = np.full(3 * 32, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.float32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, pos=base, pos_stride=12, goal=base + 64, goal_stride=12, f=fields.ctypes.data, field_stride=0, p=paths.ctypes.data,
                i=info.ctypes.data, shape=True, **shape_fields):
        s = hip.walk_shape((17, 12, 17), (8, 6, 8), 250, path_capacity=252)
        for k, val in shape_fields.items():
            setattr(s, k, val)
        return L.vx_walk_points(None, pos, pos_stride, goal, goal_stride, count, C.byref(s) if shape else None, memory, f, field_stride, p, i)

    refused = refusing(L, call, (fields, paths, info))
    refused(b"null context")
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"null shape", shape=False)
    refused(b"null pos", pos=None)
    refused(b"fields, info and paths are all null", f=None, p=None, i=None)
    refused(b"paths without goal", goal=None)
    refused(b"count exceeds", count=(1 << 24) + 1)
    for stride in (0, 4, 8, 13, 18):
        refused(b"pos_stride", pos_stride=stride)
    for stride in (4, 8, 13, 18):
        refused(b"goal_stride", goal_stride=stride)
    for off in (1, 2, 3):
        refused(b"pos must be aligned", pos=base + off)
        refused(b"goal must be aligned", goal=base + 64 + off)
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            size, seed_at = [17, 12, 17], [8, 6, 8]
            size[a], seed_at[a] = side, 0
            refused(b"size", size=u3(*size), seed_at=u3(*seed_at))
        seed_at = [8, 6, 8]
        seed_at[a] = 17
        refused(b"seed_at", seed_at=u3(*seed_at))
    for h in (0, 5, 0xFFFFFFFF):
        refused(b"height", height=h)
    refused(b"size[1] + height", size=u3(17, 30, 17), height=3)
    refused(b"size[1] + height", size=u3(17, 32, 17), height=1)
    refused(b"max_steps", max_steps=251)
    refused(b"max_steps", max_steps=0xFFFFFFFF)
    refused(b"climb", climb=2)
    refused(b"drop", drop=4)
    for cap in (2, 6, 253, 256, 0xFFFFFFFC):
        refused(b"path_capacity", path_capacity=cap)
    for flags in (2, 3, 0x80000000):
        refused(b"flags", flags=flags)
    for stride in (3468, 3470, 3456, 16):
        refused(b"field_stride", field_stride=stride)
    refused(b"count * field_stride", count=4833)
    refused(b"count * field_stride", count=4097, field_stride=4096)
    refused(b"count * path_capacity * 4", count=16645, f=None)
    f16 = fields.ctypes.data + (-fields.ctypes.data) % 16
    p16 = paths.ctypes.data + (-paths.ctypes.data) % 16
    i16 = info.ctypes.data + (-info.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"fields in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16 + off, p=p16, i=i16)
        refused(b"paths in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, p=p16 + off, i=i16)
        refused(b"info in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, p=p16, i=i16 + off)
    # every rule kept: only the context is missing
    refused(b"null context", f=None)
    refused(b"null context", i=None, field_stride=3472 + 16)
    refused(b"null context", f=None, i=None)
    refused(b"null context", goal=None, p=None, goal_stride=7)  # (no goal: its stride is not looked at)
    refused(b"null context", goal_stride=0)
    refused(b"null context", f=None, field_stride=7, count=16644)  # (no fields: their stride is not looked at)
    refused(b"null context", p=None, count=4832)
    refused(b"null context", pos_stride=64, goal_stride=64, size=u3(32, 28, 32), seed_at=u3(31, 27, 31), height=4, max_steps=0, pass_value=0xFFFFFFFF, flags=1, count=585)
    refused(b"null context", size=u3(1, 1, 1), seed_at=u3(0, 0, 0), height=1, climb=0, drop=0, path_capacity=0, count=1 << 20)
    refused(b"null context", memory=hip.VX_MEM_DEVICE, f=f16, p=p16, i=i16)
    refused(b"null context", f=fields.ctypes.data + 1, p=paths.ctypes.data + 4, i=info.ctypes.data + 1)  # (host memory needs no alignment)
    refused(b"null context", count=0, shape=False, pos=None, goal=None, f=None, p=None, i=None)
