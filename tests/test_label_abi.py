"""vx_label_boxes without a GPU: the library exports it, its three structs have the header's layout (a probe compiled from include/voxel_hip.h
with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_label's messages as
the host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from helpers import vra  # noqa: F401
from label_cases import harness
from voxel_rs_amd import hip

ROOT = Path(__file__).resolve().parent.parent
_vp = C.c_void_p

SHAPE_FIELDS = ["size", "anchor_faces", "max_pieces", "max_steps", "pass_value", "flags"]
PIECE_FIELDS = ["cells", "lo", "hi", "where"]
INFO_FIELDS = ["solid", "held", "pieces", "loose", "more", "steps", "faces", "flags"]
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "voxel_hip.h"
#define F(S, M) printf(#S "." #M " %zu %zu\n", offsetof(S, M), sizeof(((S*)0)->M))
#define K(N) printf(#N " %lu\n", (unsigned long)N)
int main(void) {
    printf("vx_label_shape %zu\nvx_label_piece %zu\nvx_label_info %zu\n", sizeof(vx_label_shape), sizeof(vx_label_piece), sizeof(vx_label_info));
    K(VX_LABEL_MAX_PIECES); K(VX_LABEL_MAX_STEPS); K(VX_LABEL_AIR); K(VX_LABEL_MORE); K(VX_LABEL_HELD); K(VX_LABEL_ALL_FACES); K(VX_LABEL_CUT);
""" + "".join(f"    F(vx_label_shape, {f});\n" for f in SHAPE_FIELDS) + "".join(f"    F(vx_label_piece, {f});\n" for f in PIECE_FIELDS) + "".join(
    f"    F(vx_label_info, {f});\n" for f in INFO_FIELDS) + """    return 0;
}
"""
CONSTANTS = {"VX_LABEL_MAX_PIECES": 250, "VX_LABEL_MAX_STEPS": 4096, "VX_LABEL_AIR": 0, "VX_LABEL_MORE": 0xFE, "VX_LABEL_HELD": 0xFF, "VX_LABEL_ALL_FACES": 0x3F,
             "VX_LABEL_CUT": 1}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_label_boxes")
    assert "vx_label_boxes" in hip.SYMBOLS and hip.lib().vx_label_boxes is not None
    assert len(hip.SYMBOLS["vx_label_boxes"][1]) == 10


def test_the_structs_have_the_headers_layout(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/include", str(tmp_path / "probe.c"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout
    probe = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.splitlines()}
    assert probe["vx_label_info"] == (32,) == (hip.LABEL_INFO_DTYPE.itemsize,)
    assert probe["vx_label_piece"] == (16,) == (hip.LABEL_PIECE_DTYPE.itemsize,)
    assert probe["vx_label_shape"] == (32,) == (C.sizeof(hip.LabelShape),)
    for name, value in CONSTANTS.items():
        assert probe[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.LabelShape._fields_] == SHAPE_FIELDS
    for name, _ in hip.LabelShape._fields_:
        field = getattr(hip.LabelShape, name)
        assert probe[f"vx_label_shape.{name}"] == (field.offset, field.size), name
    for struct, dtype, names in (("vx_label_piece", hip.LABEL_PIECE_DTYPE, PIECE_FIELDS), ("vx_label_info", hip.LABEL_INFO_DTYPE, INFO_FIELDS)):
        assert list(dtype.names) == names
        for k, f in enumerate(names):
            dt, offset = dtype.fields[f][:2]
            assert probe[f"{struct}.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.label_shape((31, 3, 17), 0x04, 4, 24, 9)
    assert (list(s.size), s.anchor_faces, s.max_pieces, s.max_steps, s.pass_value, s.flags) == ([31, 3, 17], 4, 4, 24, 9, 0)
    s = hip.label_shape((1, 1, 1))
    assert (s.anchor_faces, s.max_pieces, s.max_steps, s.pass_value, s.flags) == (0x3F, 250, 4096, 0, 0)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them with a `u` suffix)."""
    text = (ROOT / "integration" / "rust" / "voxel_hip_sys.rs").read_text()
    for name, value in CONSTANTS.items():
        m = re.search(rf"pub const {name}\s*:\s*(u8|u32)\s*=\s*([^;]+);", text)
        assert m, name
        assert int(m.group(2).strip().replace("_", ""), 0) == value, name
    for struct, names in (("vx_label_piece", PIECE_FIELDS), ("vx_label_info", INFO_FIELDS)):
        body = re.search(rf"pub struct {struct}\s*\{{(.*?)\}}", text, flags=re.S).group(1)
        assert re.findall(r"pub\s+(?:r#)?(\w+)\s*:\s*([^,\n]+),", body) == [(n, "u32") for n in names], struct
    body = re.search(r"pub struct vx_label_shape\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:\s*([^,\n]+),", body) == [("size", "[u32; 3]")] + [(n, "u32") for n in SHAPE_FIELDS[1:]]
    assert "size_of::<vx_label_info>() == 32" in text and "size_of::<vx_label_piece>() == 16" in text and "size_of::<vx_label_shape>() == 32" in text
    decl = re.search(r"pub fn vx_label_boxes\((.*?)\)\s*->\s*c_int;", text, flags=re.S).group(1)
    assert [a.split(":")[0].strip() for a in decl.split(",")] == ["ctx", "lo", "lo_stride", "count", "shape", "memory", "fields", "field_stride", "pieces", "info"]


def test_check_label_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["stride 64"] == said["fields only"] == said["pieces only"] == said["info only"] == said["count 0"] == said["count 2^20"] == "ok"
    assert said["too many"] == "count exceeds 1048576 (2^20)"
    assert said["lo_stride 8"] == "lo_stride must be a multiple of 4 and >= 12"
    assert said["lo + 2"] == "lo must be aligned to 4 bytes"
    assert said["size[1] 33"] == "size: every component must be 1..32"
    assert said["anchor_faces 64"] == "anchor_faces holds a bit above bit 5"
    assert said["max_pieces 251"] == "max_pieces exceeds VX_LABEL_MAX_PIECES (250)"
    assert said["max_steps 4097"] == "max_steps exceeds VX_LABEL_MAX_STEPS (4096)"
    assert said["flags 1"] == "flags must be 0"
    assert said["pieces with max_pieces 0"] == "pieces with max_pieces == 0"
    assert said["field_stride 4080"] == "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z"
    assert said["field bytes 2^24 + 8192"] == "count * field_stride exceeds 16777216 (2^24) bytes"
    assert said["piece bytes 2^24 + 2784"] == "count * max_pieces * 16 exceeds 16777216 (2^24) bytes"
    assert said["fields on lo"] == "fields overlaps lo" and said["pieces on info"] == "pieces overlaps info"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled outputs stay as they are."""
    L = hip.lib()
    fields = np.full(2 * 4096 + 32, 0x5a, dtype=np.uint8)
    pieces = np.full(2 * 250 * 16 + 16, 0x5a, dtype=np.uint8)
    info = np.full(3 * 32, 0x5a, dtype=np.uint8)
    sentinel = fields.tobytes() + pieces.tobytes() + info.tobytes()
    v = np.arange(64, dtype=np.int32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def refused(word, count=2, memory=hip.VX_MEM_HOST, lo=base, lo_stride=12, f=fields.ctypes.data, field_stride=0, p=pieces.ctypes.data, i=info.ctypes.data, shape=True,
                **shape_fields):
        s = hip.label_shape((16, 16, 16))
        for k, val in shape_fields.items():
            setattr(s, k, val)
        rc = L.vx_label_boxes(None, lo, lo_stride, count, C.byref(s) if shape else None, memory, f, field_stride, p, i)
        assert rc == 1 and word in L.vx_last_error(), (word, rc, L.vx_last_error())
        assert fields.tobytes() + pieces.tobytes() + info.tobytes() == sentinel

    refused(b"null context")
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    refused(b"null shape", shape=False)
    refused(b"null lo", lo=None)
    refused(b"fields, pieces and info are all null", f=None, p=None, i=None)
    refused(b"count exceeds 1048576", count=(1 << 20) + 1, f=None, p=None)
    for stride in (0, 4, 8, 13, 18):
        refused(b"lo_stride", lo_stride=stride)
    for off in (1, 2, 3):
        refused(b"lo must be aligned", lo=base + off)
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            size = [16, 16, 16]
            size[a] = side
            refused(b"size", size=u3(*size))
    for faces in (0x40, 0x100, 0x80000000):
        refused(b"anchor_faces", anchor_faces=faces)
    refused(b"max_pieces exceeds", max_pieces=251)
    refused(b"max_steps exceeds", max_steps=4097)
    refused(b"pieces with max_pieces == 0", max_pieces=0)
    for flags in (1, 2, 0x80000000):
        refused(b"flags", flags=flags)
    for stride in (4097, 4104, 4080, 16):
        refused(b"field_stride", field_stride=stride)
    refused(b"count * field_stride", count=4097, p=None)
    refused(b"count * field_stride", count=2049, field_stride=8192, p=None)
    refused(b"count * max_pieces * 16", count=4195, f=None)
    refused(b"fields overlaps lo", lo=fields.ctypes.data + (-fields.ctypes.data) % 4)
    refused(b"info overlaps lo", i=base + 16)
    refused(b"fields overlaps pieces", p=fields.ctypes.data + 4096)
    refused(b"fields overlaps info", i=fields.ctypes.data + 8191 - 63)
    refused(b"pieces overlaps info", i=pieces.ctypes.data + 2 * 250 * 16 - 1)
    f16 = fields.ctypes.data + (-fields.ctypes.data) % 16
    p16 = pieces.ctypes.data + (-pieces.ctypes.data) % 16
    i16 = info.ctypes.data + (-info.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"fields in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16 + off, p=p16, i=i16)
        refused(b"pieces in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, p=p16 + off, i=i16, max_pieces=200)
        refused(b"info in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, f=f16, p=p16, i=i16 + off)
    # every rule kept: only the context is missing
    refused(b"null context", f=None)
    refused(b"null context", p=None, max_pieces=0)
    refused(b"null context", i=None, field_stride=4096 + 16)
    refused(b"null context", f=None, p=None, field_stride=7, count=3)  # (no fields: their stride is not looked at)
    refused(b"null context", lo_stride=16, size=u3(32, 32, 32), anchor_faces=0, max_steps=0, count=1, f=None)
    refused(b"null context", size=u3(1, 1, 1), anchor_faces=0x3F, pass_value=0xFFFFFFFF)
    refused(b"null context", memory=hip.VX_MEM_DEVICE, f=f16, p=p16, i=i16)
    refused(b"null context", f=fields.ctypes.data + 1, p=pieces.ctypes.data + 1, i=info.ctypes.data + 1)  # (host memory needs no alignment)
    refused(b"null context", count=0, shape=False, lo=None, f=None, p=None, i=None)
