"""vx_label_boxes without a GPU: the library exports it, its three structs have the header's layout (a probe compiled from include/voxel_hip.h
with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_label's messages as
the host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from abi_checks import ROOT, Rust, probe, refusing
from helpers import vra  # noqa: F401
from label_cases import harness
from voxel_rs_amd import hip

_vp = C.c_void_p

SHAPE_FIELDS = ["size", "anchor_faces", "max_pieces", "max_steps", "pass_value", "flags"]
PIECE_FIELDS = ["cells", "lo", "hi", "where"]
INFO_FIELDS = ["solid", "held", "pieces", "loose", "more", "steps", "faces", "flags"]
CONSTANTS = {"VX_LABEL_MAX_PIECES": 250, "VX_LABEL_MAX_STEPS": 4096, "VX_LABEL_AIR": 0, "VX_LABEL_MORE": 0xFE, "VX_LABEL_HELD": 0xFF, "VX_LABEL_ALL_FACES": 0x3F,
             "VX_LABEL_CUT": 1}


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_label_boxes")
    assert "vx_label_boxes" in hip.SYMBOLS and hip.lib().vx_label_boxes is not None
    assert len(hip.SYMBOLS["vx_label_boxes"][1]) == 10


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_label_shape": SHAPE_FIELDS, "vx_label_piece": PIECE_FIELDS, "vx_label_info": INFO_FIELDS}, CONSTANTS)
    assert said["vx_label_info"] == (32,) == (hip.LABEL_INFO_DTYPE.itemsize,)
    assert said["vx_label_piece"] == (16,) == (hip.LABEL_PIECE_DTYPE.itemsize,)
    assert said["vx_label_shape"] == (32,) == (C.sizeof(hip.LabelShape),)
    for name, value in CONSTANTS.items():
        assert said[name] == (value,) == (getattr(hip, name),), name
    assert [n for n, _ in hip.LabelShape._fields_] == SHAPE_FIELDS
    for name, _ in hip.LabelShape._fields_:
        field = getattr(hip.LabelShape, name)
        assert said[f"vx_label_shape.{name}"] == (field.offset, field.size), name
    for struct, dtype, names in (("vx_label_piece", hip.LABEL_PIECE_DTYPE, PIECE_FIELDS), ("vx_label_info", hip.LABEL_INFO_DTYPE, INFO_FIELDS)):
        assert list(dtype.names) == names
        for k, f in enumerate(names):
            dt, offset = dtype.fields[f][:2]
            assert said[f"{struct}.{f}"] == (offset, dt.itemsize) == (4 * k, 4) and dt.str == "<u4", f
    s = hip.label_shape((31, 3, 17), 0x04, 4, 24, 9)
    assert (list(s.size), s.anchor_faces, s.max_pieces, s.max_steps, s.pass_value, s.flags) == ([31, 3, 17], 4, 4, 24, 9, 0)
    s = hip.label_shape((1, 1, 1))
    assert (s.anchor_faces, s.max_pieces, s.max_steps, s.pass_value, s.flags) == (0x3F, 250, 4096, 0, 0)


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constants (the header writes them with a `u` suffix)."""
    rust = Rust()
    for name, value in CONSTANTS.items():
        kind, got = rust.const_int(name)
        assert kind in ("u8", "u32") and got == value, name
    for struct, names in (("vx_label_piece", PIECE_FIELDS), ("vx_label_info", INFO_FIELDS)):
        assert rust.struct(struct) == [(n, "u32") for n in names], struct
    assert rust.struct("vx_label_shape") == [("size", "[u32; 3]")] + [(n, "u32") for n in SHAPE_FIELDS[1:]]
    assert rust.asserts_size("vx_label_info", 32) and rust.asserts_size("vx_label_piece", 16) and rust.asserts_size("vx_label_shape", 32)
    assert rust.args("vx_label_boxes") == ["ctx", "lo", "lo_stride", "count", "shape", "memory", "fields", "field_stride", "pieces", "info"]


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
    v = np.arange(64, dtype=np.int32)
    base = v.ctypes.data
    u3 = C.c_uint32 * 3
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, lo=base, lo_stride=12, f=fields.ctypes.data, field_stride=0, p=pieces.ctypes.data, i=info.ctypes.data, shape=True,
                **shape_fields):
        s = hip.label_shape((16, 16, 16))
        for k, val in shape_fields.items():
            setattr(s, k, val)
        return L.vx_label_boxes(None, lo, lo_stride, count, C.byref(s) if shape else None, memory, f, field_stride, p, i)

    refused = refusing(L, call, (fields, pieces, info))
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
