"""vx_overlap_boxes without a GPU: the library exports it, both structs have the header's layout (a probe compiled from include/voxel_hip.h
with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, check_boxes' messages as
the host harness prints them, and the entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import subprocess

import numpy as np

from boxes_cases import harness
from abi_checks import Rust, probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p



def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_overlap_boxes")
    assert "vx_overlap_boxes" in hip.SYMBOLS and hip.lib().vx_overlap_boxes is not None
    assert len(hip.SYMBOLS["vx_overlap_boxes"][1]) == 5


def test_the_structs_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_box_batch": ["origin", "offset", "extents", "origin_stride", "offset_stride", "extents_stride", "only_value"], "vx_box_hit": ["blocks", "value", "lo", "hi"],
                             "vx_entity": ["position", "aabb_offset", "aabb_extents"]}, ["VX_BOX_INVALID"])
    assert said["vx_box_hit"] == (32,) == (hip.BOX_HIT_DTYPE.itemsize,)
    assert said["vx_box_batch"] == (40,) == (C.sizeof(hip.BoxBatch),)
    assert said["VX_BOX_INVALID"] == (0xFFFFFFFF,) == (hip.VX_BOX_INVALID,)
    assert [n for n, _ in hip.BoxBatch._fields_] == ["origin", "offset", "extents", "origin_stride", "offset_stride", "extents_stride", "only_value"]
    for name, _ in hip.BoxBatch._fields_:
        field = getattr(hip.BoxBatch, name)
        assert said[f"vx_box_batch.{name}"] == (field.offset, field.size), name
    assert list(hip.BOX_HIT_DTYPE.names) == ["blocks", "value", "lo", "hi"]
    for f, at, size, kind in (("blocks", 0, 4, "<u4"), ("value", 4, 4, "<u4"), ("lo", 8, 12, "<i4"), ("hi", 20, 12, "<i4")):
        dt, offset = hip.BOX_HIT_DTYPE.fields[f][:2]
        assert said[f"vx_box_hit.{f}"] == (offset, dt.itemsize) == (at, size) and dt.base.str == kind, f
    # a vx_entity is read in place: entity_boxes' views lie where the header's fields do
    e = np.zeros(3, dtype=hip.ENTITY_DTYPE)
    origin, extents, offset = hip.entity_boxes(e)
    for view, field in ((origin, "position"), (offset, "aabb_offset"), (extents, "aabb_extents")):
        assert view.ctypes.data - e.ctypes.data == said[f"vx_entity.{field}"][0] and view.strides == (64, 4) and view.shape == (3, 3), field


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the constant (the header writes it in hexadecimal with a `u` suffix)."""
    rust = Rust()
    assert rust.const("VX_BOX_INVALID") == ("u32", "u32::MAX")
    assert rust.struct("vx_box_hit") == [("blocks", "u32"), ("value", "u32"), ("lo", "[i32; 3]"), ("hi", "[i32; 3]")]
    assert [n for n, _ in rust.struct("vx_box_batch")] == [n for n, _ in hip.BoxBatch._fields_]
    assert rust.asserts_size("vx_box_hit", 32) and rust.asserts_size("vx_box_batch", 40)
    assert rust.args("vx_overlap_boxes") == ["ctx", "boxes", "count", "memory", "out"]


def test_check_boxes_messages_through_the_harness():
    out = subprocess.run([str(harness()), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    assert said["packed"] == said["entities"] == said["no offset"] == said["count 0"] == "ok"
    assert said["too many"] == "count exceeds 16777216 (2^24)"
    assert said["origin_stride 8"] == "origin_stride must be a multiple of 4 and >= 12"
    assert said["offset_stride 8"] == "offset_stride must be 0, or a multiple of 4 and >= 12"
    assert said["extents_stride 13"] == "extents_stride must be 0, or a multiple of 4 and >= 12"
    assert said["origin + 2"] == "origin must be aligned to 4 bytes" and said["extents + 1"] == "extents must be aligned to 4 bytes"


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records stay as they are."""
    L = hip.lib()
    out = np.full(32 * 4 + 16, 0x5a, dtype=np.uint8)
    v = np.arange(64, dtype=np.float32)
    base = v.ctypes.data
    assert base % 4 == 0

    def call(count=2, memory=hip.VX_MEM_HOST, o=out.ctypes.data, boxes=True, **fields):
        b = hip.BoxBatch(base, base + 12 * 4, base + 24 * 4, 12, 12, 12, 0)
        for k, val in fields.items():
            setattr(b, k, val)
        return L.vx_overlap_boxes(None, C.byref(b) if boxes else None, count, memory, _vp(o))

    refused = refusing(L, call, (out,))

    refused(b"null context")
    refused(b"null boxes", boxes=False)
    refused(b"null out", o=None)
    refused(b"null origin", origin=None)
    refused(b"null extents", extents=None)
    refused(b"count exceeds", count=(1 << 24) + 1)
    refused(b"VX_MEM", memory=5)
    refused(b"VX_MEM", memory=-1)
    refused(b"VX_MEM", memory=7, count=0)
    for stride in (0, 4, 8, 13, 18):
        refused(b"origin_stride", origin_stride=stride)
    for stride in (4, 8, 13, 18):
        refused(b"offset_stride", offset_stride=stride)
        refused(b"extents_stride", extents_stride=stride)
    for off in (1, 2, 3):
        refused(b"origin must be aligned", origin=base + off)
        refused(b"offset must be aligned", offset=base + 48 + off)
        refused(b"extents must be aligned", extents=base + 96 + off)
    aligned = out.ctypes.data + (-out.ctypes.data) % 16
    for off in (1, 4, 8, 12):
        refused(b"out in device memory must be aligned to 16", memory=hip.VX_MEM_DEVICE, o=aligned + off)
    # every rule kept: only the context is missing (no offset, whatever its stride; shared vectors; entity strides; the largest count; nothing to do)
    refused(b"null context", offset=None, offset_stride=7)
    refused(b"null context", offset_stride=0, extents_stride=0)
    refused(b"null context", origin_stride=64, offset_stride=64, extents_stride=64, only_value=0xFFFFFFFF)
    refused(b"null context", count=1 << 24, memory=hip.VX_MEM_DEVICE, o=aligned)
    refused(b"null context", o=out.ctypes.data + 1)
    refused(b"null context", count=0, boxes=False, o=None)
