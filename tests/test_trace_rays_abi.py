"""vx_trace_rays without a GPU: the library exports it, the records it takes and gives have the header's sizes, and the entry point's argument
checks, which come before any HIP call, name the field they refuse and come in the documented order."""
import ctypes as C

import numpy as np

from abi_checks import probe
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p

# what the probe prints beside the sizes, and what the compiler checks behind it: the declaration has the documented signature
PRINTS = r"""    printf("shadow_t %zu\nsteps %zu\nuv %zu\npos %zu\n", offsetof(vx_hit, shadow_t), offsetof(vx_hit, steps), offsetof(vx_hit, uv), offsetof(vx_hit, pos));
    printf("formats %d %d\nmemory %d %d\n", VX_FORMAT_RGBA32F, VX_FORMAT_RGBA8, VX_MEM_HOST, VX_MEM_DEVICE);"""
SIGNATURE = r"""typedef int (*trace_rays_fn)(vx_context*, const vx_uniforms*, const vx_ray_batch*, uint32_t, int, void*, int, vx_hit*);
_Static_assert(__builtin_types_compatible_p(__typeof__(&vx_trace_rays), trace_rays_fn), "the documented signature");"""


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_trace_rays")
    assert "vx_trace_rays" in hip.SYMBOLS and hip.lib().vx_trace_rays is not None
    assert len(hip.SYMBOLS["vx_trace_rays"][1]) == 8


def test_record_and_descriptor_sizes(tmp_path):
    said = probe(tmp_path, ["vx_hit", "vx_ray_batch", "vx_uniforms"], more=PRINTS, after=SIGNATURE, std="gnu11")
    assert said["vx_hit"] == (48,) == (hip.HIT_DTYPE.itemsize,) and said["vx_ray_batch"] == (48,) == (C.sizeof(hip.RayBatch),)
    assert said["vx_uniforms"] == (C.sizeof(hip.Uniforms),)
    for f in ("pos", "uv", "shadow_t", "steps"):
        assert said[f] == (hip.HIT_DTYPE.fields[f][1],), f
    assert said["formats"] == (hip.VX_FORMAT_RGBA32F, hip.VX_FORMAT_RGBA8) and said["memory"] == (hip.VX_MEM_HOST, hip.VX_MEM_DEVICE)
    # three 16-byte stores a record: {t, value, face_id, flags} {pos, lod} {uv, shadow_t, steps}
    assert [hip.HIT_DTYPE.fields[f][1] for f in hip.HIT_DTYPE.names] == [0, 4, 8, 12, 16, 28, 32, 40, 44]


class Args:
    """A valid call's arguments but for the context, with the outputs prefilled."""

    def __init__(self):
        self.o, self.d, self.m = np.zeros((4, 3), dtype=np.float32), np.ones((4, 3), dtype=np.float32), np.full(4, 9.0, dtype=np.float32)
        self.rgba = np.full(4 * 16, 0x5a, dtype=np.uint8)
        self.hits = np.full(4 * 48, 0xa5, dtype=np.uint8)
        self.sentinel = self.rgba.tobytes() + self.hits.tobytes()
        self.u = hip.make_uniforms(np.eye(4).ravel(), 1.0, 1.0, 0.3, (0, -1, 0), (0, 0, 0), True, 100.0)

    def batch(self, **kw):
        b = hip.RayBatch(self.o.ctypes.data, self.d.ctypes.data, self.m.ctypes.data, 12, 12, 4, -1.0, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(self, ctx=None, uniforms=True, rays=True, count=4, memory=hip.VX_MEM_HOST, rgba=True, fmt=hip.VX_FORMAT_RGBA32F, hits=True, **kw):
        b = self.batch(**kw)
        rc = hip.lib().vx_trace_rays(ctx, C.byref(self.u) if uniforms else None, C.byref(b) if rays else None, count, memory,
                                     self.rgba.ctypes.data_as(_vp) if rgba else None, fmt, self.hits.ctypes.data_as(_vp) if hits else None)
        assert self.rgba.tobytes() + self.hits.tobytes() == self.sentinel  # nothing is ever written here
        return rc, hip.lib().vx_last_error()

    def refused(self, word, **kw):
        rc, msg = self.call(**kw)
        assert rc == 1 and word in msg, (word, rc, msg)


def test_argument_checks_need_no_device():
    """With a null context (and so no device): what can be refused before any HIP call is refused first, with the field named."""
    a = Args()
    a.refused(b"null context")
    for stride in (0, 4, 8, 13, 14):
        a.refused(b"origin_stride", origin_stride=stride)
    for stride in (4, 8, 13, 18):
        a.refused(b"dir_stride", dir_stride=stride)
    for stride in (1, 2, 7):
        a.refused(b"max_dst_stride", max_dst_stride=stride)
    a.refused(b"flags", flags=2)
    a.refused(b"flags", flags=0x80000000 | hip.VX_RAYS_TRANSLUCENT)
    a.refused(b"VX_MEM", memory=2)
    a.refused(b"VX_MEM", memory=-1)
    a.refused(b"VX_FORMAT", fmt=2)
    a.refused(b"VX_FORMAT", fmt=-1)
    a.refused(b"null origin", origin=None)
    a.refused(b"null dir", dir=None)
    a.refused(b"count", count=(1 << 24) + 1)
    a.refused(b"count", count=0xffffffff)
    # every rule kept: only the context is missing
    a.refused(b"null context", dir_stride=0, max_dst_stride=0, flags=hip.VX_RAYS_TRANSLUCENT, memory=hip.VX_MEM_DEVICE, fmt=hip.VX_FORMAT_RGBA8)
    a.refused(b"null context", origin_stride=64, dir_stride=48, max_dst_stride=48)
    a.refused(b"null context", max_dst=None, max_dst_stride=3)
    a.refused(b"null context", count=1 << 24)
    a.refused(b"null context", rgba=False)
    a.refused(b"null context", hits=False)
    a.refused(b"null context", count=0, uniforms=False, rays=False, rgba=False, hits=False)


def test_the_order_of_the_checks():
    """The call's own arguments (memory, format, count), then the batch's rules (flags, null origin, null dir, the strides in their order), then
    the null context; what is missing of a call with a context (uniforms, rays, both outputs) is refused after that -- shown here as far as a
    call without a context can show it: each check wins over every later one."""
    a = Args()
    later = dict(fmt=7, count=1 << 25, flags=4, origin=None, dir=None, origin_stride=2, dir_stride=2, max_dst_stride=2, uniforms=False, rgba=False, hits=False)
    order = [(b"VX_MEM", dict(memory=9)), (b"VX_FORMAT", dict(fmt=7)), (b"count", dict(count=1 << 25)), (b"flags", dict(flags=4)), (b"null origin", dict(origin=None)),
             (b"null dir", dict(dir=None)), (b"origin_stride", dict(origin_stride=2)), (b"dir_stride", dict(dir_stride=2)), (b"max_dst_stride", dict(max_dst_stride=2))]
    for k, (word, bad) in enumerate(order):
        kw = dict(bad)
        for _, rest in order[k + 1:]:
            kw.update(rest)
        kw.update({key: later[key] for key in ("uniforms", "rgba", "hits")})
        a.refused(word, **kw)
    a.refused(b"null context", uniforms=False, rays=False, rgba=False, hits=False)  # (the null context comes before what a call lacks)
