"""vx_raycast_batch without a GPU: the library exports it, the harness's records have the header's layout (a size and offset probe
compiled from include/voxel_hip.h with gcc, the way the C-ABI client is compiled), and the entry point's argument checks, which come
before any HIP call, name the field they refuse."""
import ctypes as C

import numpy as np

from abi_checks import probe, refusing
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p

BATCH_FIELDS = ["origin", "dir", "max_dst", "origin_stride", "dir_stride", "max_dst_stride", "max_dst_all", "flags"]
HIT_FIELDS = ["dst", "value", "face_id", "inside_voxel", "pos", "_pad"]


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_raycast_batch")
    assert "vx_raycast_batch" in hip.SYMBOLS and hip.lib().vx_raycast_batch is not None


def test_records_have_the_headers_layout(tmp_path):
    said = probe(tmp_path, {"vx_ray_batch": BATCH_FIELDS, "vx_ray_hit": HIT_FIELDS}, ["VX_RAYS_TRANSLUCENT"])
    assert said["vx_ray_batch"] == (48,) and said["vx_ray_hit"] == (32,) and said["VX_RAYS_TRANSLUCENT"] == (hip.VX_RAYS_TRANSLUCENT,)
    assert C.sizeof(hip.RayBatch) == 48 and [n for n, _ in hip.RayBatch._fields_] == BATCH_FIELDS
    for f in BATCH_FIELDS:
        d = getattr(hip.RayBatch, f)
        assert said[f"vx_ray_batch.{f}"] == (d.offset, d.size), f
    assert hip.RAY_HIT_DTYPE.itemsize == 32 and list(hip.RAY_HIT_DTYPE.names) == HIT_FIELDS
    for f in HIT_FIELDS:
        dt, offset = hip.RAY_HIT_DTYPE.fields[f][:2]
        assert said[f"vx_ray_hit.{f}"] == (offset, dt.itemsize), f
    assert [hip.RAY_HIT_DTYPE.fields[f][1] for f in HIT_FIELDS] == [0, 4, 8, 12, 16, 28]
    kinds = {f: hip.RAY_HIT_DTYPE.fields[f][0].base.str for f in HIT_FIELDS}
    assert kinds == {"dst": "<f4", "value": "<u4", "face_id": "<i4", "inside_voxel": "<u4", "pos": "<f4", "_pad": "<u4"}


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named; the
    sentinel-filled hits stay as they are."""
    L = hip.lib()
    o, d, m = np.zeros((4, 3), dtype=np.float32), np.ones((4, 3), dtype=np.float32), np.full(4, 9.0, dtype=np.float32)
    hits = np.full(4 * 32, 0x5a, dtype=np.uint8)

    def call(memory=hip.VX_MEM_HOST, **kw):
        b = hip.RayBatch(o.ctypes.data, d.ctypes.data, m.ctypes.data, 12, 12, 4, -1.0, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.vx_raycast_batch(None, C.byref(b), 4, memory, hits.ctypes.data_as(_vp))

    refused = refusing(L, call, (hits,))

    refused(b"null context")
    for stride in (0, 4, 8, 13, 14):
        refused(b"origin_stride", origin_stride=stride)
    for stride in (4, 8, 13, 18):
        refused(b"dir_stride", dir_stride=stride)
    for stride in (1, 2, 7):
        refused(b"max_dst_stride", max_dst_stride=stride)
    refused(b"flags", flags=2)
    refused(b"flags", flags=0x80000000 | hip.VX_RAYS_TRANSLUCENT)
    refused(b"VX_MEM", memory=2)
    refused(b"VX_MEM", memory=-1)
    refused(b"null origin", origin=None)
    refused(b"null dir", dir=None)
    # every rule kept: only the context is missing (a stride of 0 for dir and max_dst, any stride where there is no distance array)
    refused(b"null context", dir_stride=0, max_dst_stride=0, flags=hip.VX_RAYS_TRANSLUCENT, memory=hip.VX_MEM_DEVICE)
    refused(b"null context", origin_stride=64, dir_stride=48, max_dst_stride=48)
    refused(b"null context", max_dst=None, max_dst_stride=3)
    assert L.vx_raycast_batch(None, None, 0, hip.VX_MEM_HOST, None) == 1 and b"null context" in L.vx_last_error()


def test_the_binding_reads_strides_from_the_arrays():
    """Svo.raycast_batch's view of its arguments (no library call): addresses and byte strides of packed, padded and record-held vectors."""
    o = np.zeros((5, 4), dtype=np.float32)
    assert hip._ray_vectors("origins", o[:, :3], 5, 3) == (o.ctypes.data, 16)
    assert hip._ray_vectors("origins", o[:, 1:4], 5, 3) == (o.ctypes.data + 4, 16)
    e = np.zeros(5, dtype=hip.ENTITY_DTYPE)
    assert hip._ray_vectors("origins", hip.entity_positions(e), 5, 3) == (e.ctypes.data, 64)
    t = np.zeros(5, dtype=hip.PICKER_TASK_DTYPE)
    assert hip._ray_vectors("dirs", t["dir"], 5, 3) == (t.ctypes.data + 32, 48)
    assert hip._ray_vectors("max_dst", t["max_dst"], 5, 1) == (t.ctypes.data, 48)
    one = np.float32([0, -1, 0])
    assert hip._ray_vectors("dirs", one, 5, 3) == (one.ctypes.data, 0)
    for bad, width in ((o[:, :3].astype(np.float64), 3), (o[:4, :3], 3), (np.zeros((5, 6), dtype=np.float32)[:, ::2], 3), (o[::-1, :3], 3), (np.zeros((5, 1), dtype=np.float32), 1)):
        try:
            hip._ray_vectors("x", bad, 5, width)
        except TypeError:
            continue
        raise AssertionError(f"accepted {bad.shape} {bad.strides}")
