"""vx_trace_views without a GPU: the library exports it, the records it takes and gives keep the header's sizes, and the entry point's argument
checks, all of which come before the context is looked at and before any HIP call, name the field they refuse and write nothing."""
import ctypes as C

import numpy as np

from abi_checks import probe
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p

# what the probe prints beside the sizes, and what the compiler checks behind it: the declaration has the documented signature
PRINTS = r"""    printf("fovy %zu\naspect %zu\nambient %zu\nlight_dir %zu\ncam_pos %zu\nrender_shadows %zu\nshadow_distance %zu\nhighlight_pos %zu\n", offsetof(vx_uniforms, fovy),
           offsetof(vx_uniforms, aspect), offsetof(vx_uniforms, ambient), offsetof(vx_uniforms, light_dir), offsetof(vx_uniforms, cam_pos),
           offsetof(vx_uniforms, render_shadows), offsetof(vx_uniforms, shadow_distance), offsetof(vx_uniforms, highlight_pos));
    printf("formats %d %d\nmemory %d %d\n", VX_FORMAT_RGBA32F, VX_FORMAT_RGBA8, VX_MEM_HOST, VX_MEM_DEVICE);"""
SIGNATURE = r"""typedef int (*trace_views_fn)(vx_context*, const vx_uniforms*, uint32_t, uint32_t, uint32_t, int, void*, int, vx_hit*);
_Static_assert(__builtin_types_compatible_p(__typeof__(&vx_trace_views), trace_views_fn), "the documented signature");"""


def test_the_library_exports_it():
    L = C.CDLL(str(hip.lib_path("libvoxelhip.so")))
    assert hasattr(L, "vx_trace_views")
    assert "vx_trace_views" in hip.SYMBOLS and hip.lib().vx_trace_views is not None
    assert len(hip.SYMBOLS["vx_trace_views"][1]) == 9


def test_struct_sizes_are_unchanged(tmp_path):
    said = probe(tmp_path, ["vx_hit", "vx_uniforms"], more=PRINTS, after=SIGNATURE, std="gnu11")
    assert said["vx_hit"] == (48,) == (hip.HIT_DTYPE.itemsize,)
    assert said["vx_uniforms"] == (120,) == (C.sizeof(hip.Uniforms),)
    for f in ("fovy", "aspect", "ambient", "light_dir", "cam_pos", "render_shadows", "shadow_distance", "highlight_pos"):
        assert said[f] == (getattr(hip.Uniforms, f).offset,), f
    assert said["formats"] == (hip.VX_FORMAT_RGBA32F, hip.VX_FORMAT_RGBA8) and said["memory"] == (hip.VX_MEM_HOST, hip.VX_MEM_DEVICE)


class Args:
    """A valid call's arguments but for the context (two 4 x 3 views), with the outputs prefilled."""

    def __init__(self):
        u = hip.make_uniforms(np.eye(4).ravel(), 1.0, 1.0, 0.3, (0, -1, 0), (0, 0, 0), True, 100.0)
        self.views = (hip.Uniforms * 2)(u, u)
        self.rgba = np.full(2 * 12 * 16, 0x5a, dtype=np.uint8)
        self.hits = np.full(2 * 12 * 48, 0xa5, dtype=np.uint8)
        self.sentinel = self.rgba.tobytes() + self.hits.tobytes()

    def call(self, ctx=None, views=True, count=2, width=4, height=3, memory=hip.VX_MEM_HOST, rgba=True, fmt=hip.VX_FORMAT_RGBA32F, hits=True,
             rgba_at=0, hits_at=0):
        p_rgba = _vp(self.rgba.ctypes.data + rgba_at) if rgba else None
        p_hits = _vp(self.hits.ctypes.data + hits_at) if hits else None
        rc = hip.lib().vx_trace_views(ctx, self.views if views else None, count, width, height, memory, p_rgba, fmt, p_hits)
        assert self.rgba.tobytes() + self.hits.tobytes() == self.sentinel  # nothing is ever written here
        return rc, hip.lib().vx_last_error()

    def refused(self, word, **kw):
        rc, msg = self.call(**kw)
        assert rc == 1 and word in msg and (word == b"null context" or b"trace_views" in msg), (word, rc, msg)


def test_argument_checks_need_no_device():
    """With a null context (and so no device): every check of the arguments is made before the context is looked at, with the field named."""
    a = Args()
    assert a.rgba.ctypes.data % 16 == 0 and a.hits.ctypes.data % 16 == 0
    a.refused(b"null context")
    a.refused(b"VX_MEM", memory=2)
    a.refused(b"VX_MEM", memory=-1)
    a.refused(b"VX_FORMAT", fmt=2)
    a.refused(b"VX_FORMAT", fmt=-1)
    for bad in (0, 8193, 0xffffffff):
        a.refused(b"width must", width=bad)
        a.refused(b"height must", height=bad)
    a.refused(b"count * width * height", count=65536, width=8192, height=8192)  # 2^42: a 32-bit product would be 0
    a.refused(b"count * width * height", count=(1 << 24) + 1, width=1, height=1)
    a.refused(b"count * width * height", count=257, width=256, height=256)
    a.refused(b"count * width * height", count=0xffffffff, width=8192, height=8192)
    a.refused(b"null views", views=False)
    a.refused(b"null rgba", rgba=False, hits=False)
    # device outputs: rgba aligned to a pixel of the format, hits to 16 bytes (never dereferenced: the context is missing)
    a.refused(b"rgba in device memory", memory=hip.VX_MEM_DEVICE, rgba_at=4)
    a.refused(b"rgba in device memory", memory=hip.VX_MEM_DEVICE, rgba_at=8, hits=False)
    a.refused(b"rgba in device memory", memory=hip.VX_MEM_DEVICE, fmt=hip.VX_FORMAT_RGBA8, rgba_at=2)
    a.refused(b"hits in device memory", memory=hip.VX_MEM_DEVICE, hits_at=8)
    a.refused(b"hits in device memory", memory=hip.VX_MEM_DEVICE, hits_at=4, rgba=False)
    # every rule kept: only the context is missing
    a.refused(b"null context", memory=hip.VX_MEM_DEVICE, fmt=hip.VX_FORMAT_RGBA8, rgba_at=4)
    a.refused(b"null context", memory=hip.VX_MEM_HOST, rgba_at=4, hits_at=4)  # (host outputs have no alignment rule)
    a.refused(b"null context", count=1 << 24, width=1, height=1)
    a.refused(b"null context", count=256, width=256, height=256)
    a.refused(b"null context", count=1, width=8192, height=2048)
    a.refused(b"null context", rgba=False)
    a.refused(b"null context", hits=False)
    a.refused(b"null context", count=0, views=False, rgba=False, hits=False)


def test_the_order_of_the_checks():
    """memory, format, width, height, the number of pixels, null views, both outputs null, the alignment of device outputs, the null context:
    each check wins over every later one."""
    a = Args()
    order = [(b"VX_MEM", dict(memory=9)), (b"VX_FORMAT", dict(fmt=7)), (b"width must", dict(width=0)), (b"height must", dict(height=9000)),
             (b"count * width * height", dict(count=1 << 30)), (b"null views", dict(views=False)), (b"null rgba", dict(rgba=False, hits=False))]
    for k, (word, bad) in enumerate(order):
        kw = dict(bad)
        for _, rest in order[k + 1:]:
            kw.update(rest)
        a.refused(word, **kw)
    a.refused(b"null views", views=False, memory=hip.VX_MEM_DEVICE, rgba_at=4)
    a.refused(b"rgba in device memory", memory=hip.VX_MEM_DEVICE, rgba_at=4, hits_at=4)
