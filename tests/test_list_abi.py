"""vx_list_region without a GPU: the library exports it, the record and the macros have the header's layout and values (a probe compiled from
include/voxel_hip.h with gcc, the way the C-ABI client is compiled) and the Python binding and the Rust declarations agree with them, and the
entry point's argument checks, which come before any HIP call, name the field they refuse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

ROOT = Path(__file__).resolve().parent.parent
_vp = C.c_void_p

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "voxel_hip.h"
#define F(S, M) printf(#S "." #M " %zu %zu\n", offsetof(S, M), sizeof(((S*)0)->M))
int main(void) {
    printf("vx_block_at %zu\nVX_LIST_FACES %lu\nVX_LIST_EXPOSED %lu\n", sizeof(vx_block_at), (unsigned long)VX_LIST_FACES, (unsigned long)VX_LIST_EXPOSED);
    F(vx_block_at, where);
    F(vx_block_at, value);
    printf("index %lu\nfaces %lu\nabove %lu\n", (unsigned long)VX_AT_INDEX(0xEAFEDCBAu), (unsigned long)VX_AT_FACES(0xEAFEDCBAu), (unsigned long)VX_AT_FACES(0xC0000000u));
    return 0;
}
"""


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_list_region")
    assert "vx_list_region" in hip.SYMBOLS and hip.lib().vx_list_region is not None
    assert len(hip.SYMBOLS["vx_list_region"][1]) == 8


def test_the_record_and_the_macros_have_the_headers_layout(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/include", str(tmp_path / "probe.c"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout
    probe = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.splitlines()}
    assert probe["vx_block_at"] == (8,) == (hip.BLOCK_AT_DTYPE.itemsize,)
    assert probe["VX_LIST_FACES"] == (1,) == (hip.VX_LIST_FACES,) and probe["VX_LIST_EXPOSED"] == (2,) == (hip.VX_LIST_EXPOSED,)
    assert list(hip.BLOCK_AT_DTYPE.names) == ["where", "value"]
    for f, at in (("where", 0), ("value", 4)):
        dt, offset = hip.BLOCK_AT_DTYPE.fields[f][:2]
        assert probe[f"vx_block_at.{f}"] == (offset, dt.itemsize) == (at, 4) and dt.str == "<u4", f
    # VX_AT_INDEX: the low 24 bits; VX_AT_FACES: the six above them, and nothing of bits 30..31
    assert probe["index"] == (0xFEDCBA,) and probe["faces"] == (0x2A,) and probe["above"] == (0,)
    assert hip.split_where(0xEAFEDCBA) == (0xFEDCBA, 0x2A) and hip.split_where(0xC0000000) == (0, 0)
    index, faces = hip.split_where(np.array([0xEAFEDCBA, 0x3F000001], dtype=np.uint32))
    assert index.tolist() == [0xFEDCBA, 1] and faces.tolist() == [0x2A, 0x3F]


def test_the_rust_declarations_agree():
    """What tests/test_rust_shim.py's parser cannot see of this call: the flag constants (the header writes them with a `u` suffix) and the
    helpers that stand for the two macros."""
    text = (ROOT / "integration" / "rust" / "voxel_hip_sys.rs").read_text()
    consts = {k: int(v, 0) for k, v in re.findall(r"pub const (VX_LIST_\w+)\s*:\s*u32\s*=\s*(\w+)\s*;", text)}
    assert consts == {"VX_LIST_FACES": hip.VX_LIST_FACES, "VX_LIST_EXPOSED": hip.VX_LIST_EXPOSED}
    body = re.search(r"pub struct vx_block_at\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub\s+(?:r#)?(\w+)\s*:\s*(\w+)", body) == [("where", "u32"), ("value", "u32")]
    assert "size_of::<vx_block_at>() == 8" in text
    assert re.search(r"fn vx_at_index\(at: u32\) -> u32 \{ at & 0xFF_FFFF \}", text) and re.search(r"fn vx_at_faces\(at: u32\) -> u32 \{ \(at >> 24\) & 0x3F \}", text)
    decl = re.search(r"pub fn vx_list_region\((.*?)\)\s*->\s*c_int;", text, flags=re.S).group(1)
    assert [a.split(":")[0].strip() for a in decl.split(",")] == ["ctx", "lo", "size", "flags", "memory", "out", "capacity", "total"]


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled records and total stay as they are."""
    L = hip.lib()
    out = np.full(64 + 8, 0x5a, dtype=np.uint8)
    total = np.full(8, 0x5a, dtype=np.uint8)
    sentinel = out.tobytes(), total.tobytes()
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def refused(word, lo=(-3, 0, 5), size=(4, 2, 2), flags=0, memory=hip.VX_MEM_HOST, o=out.ctypes.data, capacity=8, t=total.ctypes.data):
        rc = L.vx_list_region(None, C.byref(i3(*lo)) if lo is not None else None, C.byref(u3(*size)) if size is not None else None, flags, memory, _vp(o),
                              capacity, _vp(t))
        assert rc == 1 and word in L.vx_last_error(), (word, rc, L.vx_last_error())
        assert (out.tobytes(), total.tobytes()) == sentinel

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
