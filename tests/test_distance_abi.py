"""vx_distance_boxes without a GPU: the library exports it, its two structs have the header's layout (a probe compiled from
include/voxel_hip.h with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them,
check_distance's messages as the host harness prints them, and the entry point's argument checks, which come before any HIP call, name the
field they refuse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from distance_cases import harness
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

ROOT = Path(__file__).resolve().parent.parent

SHAPE_FIELDS = ["size", "pass_value", "match_value", "flags", "_pad"]
INFO_FIELDS = ["targets", "farthest", "where", "faces"]
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "voxel_hip.h"
#define F(S, M) printf(#S "." #M " %zu %zu\n", offsetof(S, M), sizeof(((S*)0)->M))
#define K(N) printf(#N " %lu\n", (unsigned long)N)
int main(void) {
    printf("vx_distance_shape %zu\nvx_distance_info %zu\n", sizeof(vx_distance_shape), sizeof(vx_distance_info));
    K(VX_DISTANCE_NONE); K(VX_DISTANCE_TO_AIR);
""" + "".join(f"    F(vx_distance_shape, {f});\n" for f in SHAPE_FIELDS) + "".join(f"    F(vx_distance_info, {f});\n" for f in INFO_FIELDS) + """    return 0;
}
"""
CONSTANTS = {"VX_DISTANCE_NONE": 0xFFFF, "VX_DISTANCE_TO_AIR": 1}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_distance_boxes")
    assert "vx_distance_boxes" in hip.SYMBOLS and hip.lib().vx_distance_boxes is not None
    assert len(hip.SYMBOLS["vx_distance_boxes"][1]) == 9


def test_the_structs_have_the_headers_layout(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/include", str(tmp_path / "probe.c"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout
    probe = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.splitlines()}
    assert probe["vx_distance_info"] == (16,) == (hip.DISTANCE_INFO_DTYPE.itemsize,)
    assert probe["vx_distance_shape"] == (32,) == (C.sizeof(hip.DistanceShape),)
    for name, value in CONSTANTS.items():
        assert probe[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.DistanceShape._fields_] == SHAPE_FIELDS
    for name, _ in hip.DistanceShape._fields_:
        field = getattr(hip.DistanceShape, name)
        assert probe[f"vx_distance_shape.{name}"] == (field.offset, field.size), name
    assert list(hip.DISTANCE_INFO_DTYPE.names) == INFO_FIELDS
    for k, f in enumerate(INFO_FIELDS):
        dt, offset = hip.DISTANCE_INFO_DTYPE.fields[f][:2]
        assert probe[f"vx_distance_info.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.distance_shape((31, 3, 17), 9, 0, 1)
    assert (list(s.size), s.pass_value, s.match_value, s.flags, list(s._pad)) == ([31, 3, 17], 9, 0, 1, [0, 0])
    s = hip.distance_shape((1, 1, 1))
    assert (s.pass_value, s.match_value, s.flags) == (0, 0, 0)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them with a `u` suffix)."""
    text = (ROOT / "integration" / "rust" / "voxel_hip_sys.rs").read_text()
    for name, value in CONSTANTS.items():
        m = re.search(rf"pub const {name}\s*:\s*(u16|u32)\s*=\s*([^;]+);", text)
        assert m, name
        assert int(m.group(2).strip().replace("_", ""), 0) == value, name
    body = re.search(r"pub struct vx_distance_info\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub\s+(?:r#)?(\w+)\s*:\s*([^,\n]+),", body) == [(n, "u32") for n in INFO_FIELDS]
    body = re.search(r"pub struct vx_distance_shape\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:\s*([^,\n]+),", body) == [("size", "[u32; 3]")] + [(n, "u32") for n in SHAPE_FIELDS[1:-1]] + [("_pad", "[u32; 2]")]
    assert "size_of::<vx_distance_info>() == 16" in text and "size_of::<vx_distance_shape>() == 32" in text
    decl = re.search(r"pub fn vx_distance_boxes\((.*?)\)\s*->\s*c_int;", text, flags=re.S).group(1)
    assert [a.split(":")[0].strip() for a in decl.split(",")] == ["ctx", "lo", "lo_stride", "count", "shape", "memory", "fields", "field_stride", "info"]
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
    sentinel = fields.tobytes() + info.tobytes()
    v = np.arange(64, dtype=np.int32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def refused(word, count=2, memory=hip.VX_MEM_HOST, lo=base, lo_stride=12, f=fields.ctypes.data, field_stride=0, i=info.ctypes.data, shape=True, **shape_fields):
        s = hip.distance_shape((16, 16, 16))
        for k, val in shape_fields.items():
            setattr(s, k, val)
        rc = L.vx_distance_boxes(None, lo, lo_stride, count, C.byref(s) if shape else None, memory, f, field_stride, i)
        assert rc == 1 and word in L.vx_last_error(), (word, rc, L.vx_last_error())
        assert fields.tobytes() + info.tobytes() == sentinel

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
