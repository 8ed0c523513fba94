"""The Python side of the batch and block calls (voxel-rs_amd/hip.py, Svo.raycast_batch to Svo.physics_step) without a GPU and without the
library: hip.lib is replaced by a recorder whose every vx_* notes its arguments and returns VX_OK, an Svo is made without vx_create, and
each method's one call is held against the arrays it was given -- every pointer, stride, count, memory kind and struct field -- and its
return against what the docstring promises. Device memory is a CPU torch tensor behind a wrapper that says is_cuda. Then the refusals,
the size rule of every output (exact or at-least, per memory kind) and what None, True and False mean for fields, info, pieces and paths."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

HOST, DEVICE = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE
SIDES = ("host", "device")
COUNTS = (0, 1, 5)
F32 = np.float32
U = hip.Uniforms()
PROPS = [0x10, 0x1F, 0x00]


class Recorder:
    """Stands in for the library: every vx_* attribute notes (name, arguments) and returns VX_OK; a host vx_list_region stores `total`."""

    def __init__(self):
        self.calls, self.total = [], 0

    def __getattr__(self, name):
        if not name.startswith("vx_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "vx_list_region" and args[4] == HOST:
                args[7]._obj.value = self.total
            return hip.VX_OK

        return fn


class Dev:
    """A CPU torch tensor that says it lies on the device."""
    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(hip, "lib", lambda: r)
    return r


@pytest.fixture
def svo(rec):
    s = hip.Svo.__new__(hip.Svo)
    s._h, s.svo_type = C.c_void_p(0x1234), 0
    yield s
    s._h = None  # (close would call the recorder)


def val(a):
    """What a recorded argument holds: the struct behind a byref, the address in a c_void_p, anything else as it is."""
    if hasattr(a, "_obj"):
        return a._obj
    return a.value if isinstance(a, C.c_void_p) else a


def call(rec, fn, *args, **kw):
    """(what fn returned, the one library call it made: its name, its arguments through val)."""
    del rec.calls[:]
    got = fn(*args, **kw)
    assert len(rec.calls) == 1
    name, a = rec.calls[0]
    return got, name, [val(x) for x in a]


def struct(s):
    return {n: (list(getattr(s, n)) if isinstance(getattr(s, n), C.Array) else getattr(s, n)) for n, _ in s._fields_}


def dev(a):
    """The NumPy array's memory as a device tensor (uint32 as the int32 the binding hands out)."""
    return Dev(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a))


def addr(x):
    """Where x's first byte lies; None for the null pointer of an empty tensor, as a c_void_p reads."""
    return (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()) or None


def zeros(side, shape, dtype):
    """An output of plain numbers: uint8, uint32 (int32 on the device) or float32."""
    a = np.zeros(shape, dtype=dtype)
    return a if side == "host" else dev(a)


def records(side, shape, dtype):
    """An output of records: a NumPy array of the dtype, or the int32 tensor of shape + (words,) the binding hands out."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    return np.zeros(shape, dtype=dtype) if side == "host" else dev(np.zeros(shape + (dtype.itemsize // 4,), dtype=np.int32))


def vec_forms(side, n, one=False, width=3):
    """[(label, vectors, address expected, byte stride expected)]: packed, padded, held in records; `one`: and a single (3,) vector."""
    a, b = np.zeros((n, 3), dtype=F32), np.zeros((n, 4), dtype=F32)
    e, h = np.zeros(n, dtype=hip.ENTITY_DTYPE), np.zeros(n, dtype=hip.RAY_HIT_DTYPE)
    if side == "host":
        forms = [("packed", a, a.ctypes.data, 12), ("padded", b[:, :3], b.ctypes.data, 16), ("padded + 4", b[:, 1:], b.ctypes.data + 4, 16),
                 ("entity_positions", hip.entity_positions(e), e.ctypes.data, 64), ("entity_velocities", hip.entity_velocities(e), e.ctypes.data + 12, 64),
                 ("ray_hit_positions", hip.ray_hit_positions(h), h.ctypes.data + 16, 32)]
        # (NumPy gives an empty array of plain numbers strides of 0, which reads as components that are not adjacent: only the record views pass)
        forms = forms[3 if n == 0 else 0:]
    else:
        ta, tb, te, th = (torch.from_numpy(x.view(np.uint8).reshape(-1).view(F32).reshape(-1, w)) for x, w in ((a, 3), (b, 4), (e, 16), (h, 8)))
        forms = [("packed", Dev(ta), ta.data_ptr(), 12), ("padded", Dev(tb[:, :3]), tb.data_ptr(), 16), ("padded + 4", Dev(tb[:, 1:]), tb.data_ptr() + 4, 16)]
        if n:  # (the record views of an empty device tensor are refused by torch's view(-1, 16) on the parent)
            forms += [("entity_positions", Dev(hip.entity_positions(te)), te.data_ptr(), 64), ("entity_velocities", Dev(hip.entity_velocities(te)), te.data_ptr() + 12, 64),
                      ("ray_hit_positions", Dev(hip.ray_hit_positions(th)), th.data_ptr() + 16, 32)]
    # (nobody steps by the stride of one row; an empty view lies wherever its library says)
    forms = [(label, x, at if n else addr(x), stride if n > 1 else 12) for label, x, at, stride in forms]
    if one:
        v = np.array([1, 2, 3], dtype=F32)
        forms.append(("one vector", v if side == "host" else dev(v), addr(v), 0))
    for _, x, _, _ in forms:
        assert tuple(x.shape) in ((n, 3), (3,)) and str(x.dtype).endswith("float32")
    return forms


def lo_forms(side, n):
    """[(label, int32 rows, address, byte stride)] of light_boxes' and label_boxes' lo: packed, and padded to 16 and 20 bytes."""
    a, b = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 5), dtype=np.int32)
    if side == "host":
        forms = [("packed", a, a.ctypes.data, 12), ("padded", b[:, :3], b.ctypes.data, 20), ("padded + 8", b[:, 2:], b.ctypes.data + 8, 20)]
    else:
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        forms = [("packed", Dev(ta), ta.data_ptr(), 12), ("padded", Dev(tb[:, :3]), tb.data_ptr(), 20), ("padded + 8", Dev(tb[:, 2:]), tb.data_ptr() + 8, 20)]
    return [(label, x, at if n else addr(x), stride if n else 12) for label, x, at, stride in forms]  # (lo's own stride from one row on)


def fresh(got, dtype, shape):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == shape and got.flags.c_contiguous and got.flags.writeable


# ---- the record views ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", COUNTS)
def test_record_views_read_the_records_in_place(n):
    """entity_positions, entity_boxes, entity_velocities, ray_hit_positions: (N, 3) float32 views at the record's stride, on both sides."""
    e, h = np.zeros(n, dtype=hip.ENTITY_DTYPE), np.zeros(n, dtype=hip.RAY_HIT_DTYPE)
    views = {"position": hip.entity_positions(e), "velocity": hip.entity_velocities(e)}
    views["position"], views["aabb_extents"], views["aabb_offset"] = hip.entity_boxes(e)
    for field, v in views.items():
        assert v.shape == (n, 3) and v.dtype == F32 and v.ctypes.data == e.ctypes.data + hip.ENTITY_DTYPE.fields[field][1]
        assert v.strides == (64, 4)
    p = hip.ray_hit_positions(h)
    assert p.shape == (n, 3) and p.ctypes.data == h.ctypes.data + 16 and p.strides == (32, 4)
    if n:
        te, th = torch.from_numpy(e.view(np.uint8)), torch.from_numpy(h.view(np.int32).reshape(n, 8))
        views = {"position": hip.entity_positions(te), "velocity": hip.entity_velocities(te)}
        views["position"], views["aabb_extents"], views["aabb_offset"] = hip.entity_boxes(te)
        for field, v in views.items():
            assert tuple(v.shape) == (n, 3) and v.dtype == torch.float32 and v.stride() == (16, 1)
            assert v.data_ptr() == te.data_ptr() + hip.ENTITY_DTYPE.fields[field][1]
        p = hip.ray_hit_positions(th)
        assert tuple(p.shape) == (n, 3) and p.dtype == torch.float32 and p.stride() == (8, 1) and p.data_ptr() == th.data_ptr() + 16
    for fn, bad in ((hip.entity_positions, h), (hip.entity_boxes, h), (hip.entity_velocities, h), (hip.ray_hit_positions, e)):
        with pytest.raises(TypeError, match=f"^{fn.__name__}: a host array"):
            fn(bad)
        with pytest.raises(TypeError, match=f"^{fn.__name__}: a device tensor"):
            fn(torch.zeros(7, dtype=torch.uint8))
        with pytest.raises(TypeError, match=f"^{fn.__name__}: a device tensor"):
            fn(torch.zeros((4, 64), dtype=torch.uint8)[:, ::2])


def test_to_numpy_gives_the_records_of_a_tensor():
    """The ten *_to_numpy functions: the tensor's bytes as records, flat -- label_pieces_to_numpy [N, max_pieces], scan_hits_to_numpy in
    the tensor's shape without its last axis."""
    flat = {hip.box_hits_to_numpy: hip.BOX_HIT_DTYPE, hip.move_hits_to_numpy: hip.MOVE_HIT_DTYPE, hip.flood_infos_to_numpy: hip.FLOOD_INFO_DTYPE,
            hip.walk_infos_to_numpy: hip.WALK_INFO_DTYPE, hip.light_infos_to_numpy: hip.LIGHT_INFO_DTYPE, hip.label_infos_to_numpy: hip.LABEL_INFO_DTYPE,
            hip.ray_hits_to_numpy: hip.RAY_HIT_DTYPE, hip.trace_hits_to_numpy: hip.HIT_DTYPE, hip.block_cells_to_numpy: hip.BLOCK_CELL_DTYPE,
            hip.block_ats_to_numpy: hip.BLOCK_AT_DTYPE}
    for fn, dtype in flat.items():
        words = dtype.itemsize // 4
        t = torch.arange(6 * words, dtype=torch.int32).reshape(2, 3, words)
        got = fn(t)
        assert got.dtype == dtype and got.shape == (6,) and got.tobytes() == t.numpy().tobytes(), fn.__name__
    t = torch.arange(3 * 2 * 4, dtype=torch.int32).reshape(3, 2, 4)
    got = hip.label_pieces_to_numpy(t)
    assert got.dtype == hip.LABEL_PIECE_DTYPE and got.shape == (3, 2) and got.tobytes() == t.numpy().tobytes()
    got = hip.scan_hits_to_numpy(t)
    assert got.dtype == hip.SCAN_HIT_DTYPE and got.shape == (3, 2) and got.tobytes() == t.numpy().tobytes()
    assert hip.scan_hits_to_numpy(t.reshape(6, 4)).shape == (6,)


# ---- every method's call, argument by argument ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_raycast_batch(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    tasks = np.zeros(n, dtype=hip.PICKER_TASK_DTYPE)
    reach = tasks["max_dst"] if side == "host" else Dev(torch.from_numpy(tasks.view(F32).reshape(n, 12))[:, 0])
    dirs = vec_forms(side, n, one=True)
    for k, (label, o, o_at, o_stride) in enumerate(vec_forms(side, n)):
        _, d, d_at, d_stride = dirs[k % len(dirs)]
        for max_dst, translucent in ((7.5, False), (reach, True)):
            for given in (records(side, n, hip.RAY_HIT_DTYPE), None):
                if given is None and side == "device":
                    continue
                got, name, a = call(rec, svo.raycast_batch, o, d, max_dst, translucent, given)
                assert name == "vx_raycast_batch" and a[0] == svo._h.value and a[2:4] == [n, mem] and a[4] == addr(got), label
                b = struct(a[1])
                assert (b["origin"], b["origin_stride"], b["dir"], b["dir_stride"]) == (o_at, o_stride, d_at, d_stride), label
                if max_dst is reach:
                    assert (b["max_dst"], b["max_dst_stride"], b["flags"]) == (addr(tasks) if n else addr(reach), 48 if n > 1 else 4, hip.VX_RAYS_TRANSLUCENT)
                else:
                    assert (b["max_dst"], b["max_dst_stride"], b["max_dst_all"], b["flags"]) == (None, 0, 7.5, 0)
                if given is None:
                    fresh(got, hip.RAY_HIT_DTYPE, (n,))
                else:
                    assert got is given
    got, _, a = call(rec, svo.raycast_batch, *(vec_forms(side, n)[0][1],) * 2, out=records(side, n, hip.RAY_HIT_DTYPE))
    assert struct(a[1])["max_dst_all"] == -1.0  # the default: to the world's edge


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_trace_rays(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    _, o, o_at, o_stride = vec_forms(side, n)[1]
    _, d, d_at, d_stride = vec_forms(side, n, one=True)[-1]
    for fmt, px, px_shape in ((hip.VX_FORMAT_RGBA32F, F32, (n, 4)), (hip.VX_FORMAT_RGBA8, np.uint8, (n, 4))):
        for want_rgba, want_hits in ((True, False), (False, True), (True, True)):
            for supplied in (True, False):
                if not supplied and side == "device":
                    continue
                rgba, hits = (zeros(side, (n + 2, 4), px), records(side, n + 1, hip.HIT_DTYPE)) if supplied else (None, None)  # (they may be longer)
                (g_rgba, g_hits), name, a = call(rec, svo.trace_rays, U, o, d, 3.0, want_hits, fmt, (rgba, hits) if supplied else None, want_rgba)
                assert name == "vx_trace_rays" and a[0] == svo._h.value and a[1] is U and a[3:5] == [n, mem] and a[6] == fmt
                b = struct(a[2])
                assert (b["origin"], b["origin_stride"], b["dir"], b["dir_stride"]) == (o_at, o_stride, d_at, d_stride)
                assert (b["max_dst"], b["max_dst_stride"], b["max_dst_all"], b["flags"]) == (None, 0, 3.0, 0)
                assert a[5] == (addr(g_rgba) if want_rgba else None) and a[7] == (addr(g_hits) if want_hits else None)
                assert (g_rgba is None) == (not want_rgba) and (g_hits is None) == (not want_hits)
                if supplied:
                    assert g_rgba is (rgba if want_rgba else None) and g_hits is (hits if want_hits else None)
                else:
                    if want_rgba:
                        fresh(g_rgba, px, px_shape)
                    if want_hits:
                        fresh(g_hits, hip.HIT_DTYPE, (n,))
    # one of the pair given, the other fresh
    if side == "host":
        hits = records(side, n, hip.HIT_DTYPE)
        (g_rgba, g_hits), _, a = call(rec, svo.trace_rays, U, o, d, want_hits=True, out=(None, hits))
        assert g_hits is hits and a[7] == addr(hits) and a[5] == addr(g_rgba)
        fresh(g_rgba, F32, (n, 4))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_trace_views(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    w, h = 3, 2
    for views in ([hip.make_uniforms(range(16), 1.0 + i, 1.5, 0.1, (0, 1, 0), (i, 2, 3), 1, 9.0) for i in range(n)], (hip.Uniforms * max(n, 1))()):
        count = len(views)
        for fmt, px in ((hip.VX_FORMAT_RGBA32F, F32), (hip.VX_FORMAT_RGBA8, np.uint8)):
            for want_rgba, want_hits in ((True, False), (False, True), (True, True)):
                for supplied in (True, False):
                    if not supplied and side == "device":
                        continue
                    rgba, hits = (zeros(side, (count, h, w, 4), px), records(side, (count, h * w), hip.HIT_DTYPE)) if supplied else (None, None)
                    (g_rgba, g_hits), name, a = call(rec, svo.trace_views, views, w, h, want_hits, want_rgba, fmt, (rgba, hits) if supplied else None)
                    assert name == "vx_trace_views" and a[0] == svo._h.value and a[2:6] == [count, w, h, mem] and a[7] == fmt
                    if isinstance(views, C.Array):
                        assert a[1] is views
                    else:
                        assert isinstance(a[1], C.Array) and len(a[1]) == max(count, 1) and all(bytes(a[1][i]) == bytes(views[i]) for i in range(count))
                    assert a[6] == (addr(g_rgba) if want_rgba else None) and a[8] == (addr(g_hits) if want_hits else None)
                    if supplied:
                        assert g_rgba is (rgba if want_rgba else None) and g_hits is (hits if want_hits else None)
                    else:
                        assert (g_rgba is None) == (not want_rgba) and (g_hits is None) == (not want_hits)
                        if want_rgba:
                            fresh(g_rgba, px, (count, h, w, 4))
                        if want_hits:
                            fresh(g_hits, hip.HIT_DTYPE, (count, h * w))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_block_points_and_scan_points(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    for label, p, at, stride in vec_forms(side, n):
        for given in (True, False):
            if not given and side == "device":
                continue
            out = records(side, n, hip.BLOCK_CELL_DTYPE) if given else None
            got, name, a = call(rec, svo.block_points, p, out)
            assert name == "vx_block_points" and a == [svo._h.value, at, stride, n, mem, addr(got)], label
            assert got is out if given else fresh(got, hip.BLOCK_CELL_DTYPE, (n,)) is None
            out = records(side, n, hip.SCAN_HIT_DTYPE) if given else None
            got, name, a = call(rec, svo.scan_points, p, hip.VX_DIR_POS_Z, 9, out)
            assert name == "vx_scan_points" and a == [svo._h.value, at, stride, n, hip.VX_DIR_POS_Z, 9, mem, addr(got)], label
            assert got is out if given else fresh(got, hip.SCAN_HIT_DTYPE, (n,)) is None
    _, _, a = call(rec, svo.scan_points, vec_forms(side, n)[0][1], hip.VX_DIR_NEG_Y, out=records(side, n, hip.SCAN_HIT_DTYPE))
    assert a[4:6] == [hip.VX_DIR_NEG_Y, hip.VX_SCAN_TO_EDGE]


@pytest.mark.parametrize("side", SIDES)
def test_read_region_and_scan_columns(svo, rec, side):
    mem = HOST if side == "host" else DEVICE
    lo, size = (-3, 4, 5), (2, 3, 7)
    for given in (True, False):
        if not given and side == "device":
            continue
        out = zeros(side, (7, 3, 2), np.uint32) if given else None
        got, name, a = call(rec, svo.read_region, lo, size, out)
        assert name == "vx_read_region" and a[0] == svo._h.value and list(a[1]) == list(lo) and list(a[2]) == list(size) and a[3:] == [mem, addr(got)]
        assert isinstance(a[1], C.c_int32 * 3) and isinstance(a[2], C.c_uint32 * 3)
        assert got is out if given else fresh(got, np.uint32, (7, 3, 2)) is None
        for direction, shape in ((hip.VX_DIR_NEG_X, (7, 3)), (hip.VX_DIR_POS_X, (7, 3)), (hip.VX_DIR_NEG_Y, (7, 2)), (hip.VX_DIR_POS_Z, (3, 2))):
            out = records(side, shape, hip.SCAN_HIT_DTYPE) if given else None
            got, name, a = call(rec, svo.scan_columns, lo, size, direction, out)
            assert name == "vx_scan_columns" and list(a[1]) == list(lo) and list(a[2]) == list(size) and a[3:] == [direction, mem, addr(got)]
            assert got is out if given else fresh(got, hip.SCAN_HIT_DTYPE, shape) is None
        # an empty box, and a direction that names no axis: no columns (the library refuses the latter)
        for sz, direction in (((2, 0, 7), hip.VX_DIR_NEG_X), (size, 6)):
            out = records(side, (0, 0), hip.SCAN_HIT_DTYPE) if given else None
            got, _, a = call(rec, svo.scan_columns, lo, sz, direction, out)
            assert a[3:5] == [direction, mem] and (got is out if given else fresh(got, hip.SCAN_HIT_DTYPE, (0, 0)) is None)
    if side == "device":  # device=True with no tensor: a fresh one needs a GPU; a NumPy `out` with it is refused
        with pytest.raises(TypeError, match="^read_region: out must be a contiguous CUDA tensor"):
            svo.read_region(lo, size, np.zeros((7, 3, 2), dtype=np.uint32), device=True)
        with pytest.raises(TypeError, match="^scan_columns: out must be a contiguous CUDA tensor"):
            svo.scan_columns(lo, size, 0, np.zeros((7, 3), dtype=hip.SCAN_HIT_DTYPE), device=True)


def test_list_region_on_the_host(svo, rec):
    lo, size = (1, -2, 3), (4, 2, 3)  # 24 voxels
    head = lambda a: (a[0], list(a[1]), list(a[2]), a[3], a[4])  # noqa: E731
    # count first: two calls, the array as long as the list
    for total in (0, 7, 24):
        rec.total = total
        del rec.calls[:]
        got, n = svo.list_region(lo, size, hip.VX_LIST_FACES)
        assert n == total and isinstance(n, int)
        fresh(got, hip.BLOCK_AT_DTYPE, (total,))
        (n1, a1), (n2, a2) = rec.calls
        a1, a2 = [val(x) for x in a1], [val(x) for x in a2]
        assert n1 == n2 == "vx_list_region" and head(a1) == head(a2) == (svo._h.value, list(lo), list(size), hip.VX_LIST_FACES, HOST)
        assert a1[5:7] == [None, 0] and a2[5:7] == [addr(got) if total else None, total] and isinstance(a2[7], C.c_uint32)
    # a capacity given: one call, a fresh array of min(capacity, voxels), of which the first min(total, capacity) come back
    for capacity, total, held, back in ((5, 7, 5, 5), (5, 3, 5, 3), (0, 7, 0, 0), (99, 7, 24, 7)):
        rec.total = total
        (got, n), _, a = call(rec, svo.list_region, lo, size, capacity=capacity)
        assert n == total and a[3:5] == [0, HOST] and a[6] == held and (a[5] is None if not held else a[5] == addr(got))
        fresh(got, hip.BLOCK_AT_DTYPE, (back,))
    # the caller's array: capacity is what it holds, or what was asked for; whole records come back as a view of it
    out = np.zeros(6, dtype=hip.BLOCK_AT_DTYPE)
    for capacity, total, asked, back in ((None, 9, 6, 6), (None, 2, 6, 2), (4, 9, 4, 4), (6, 9, 6, 6), (0, 9, 0, 0)):
        rec.total = total
        (got, n), _, a = call(rec, svo.list_region, lo, size, hip.VX_LIST_EXPOSED, capacity, out)
        assert n == total and a[3] == hip.VX_LIST_EXPOSED and a[6] == asked and a[5] == (out.ctypes.data if asked else None)
        assert got.base is out and got.shape == (back,) and got.dtype == hip.BLOCK_AT_DTYPE and (not back or got.ctypes.data == out.ctypes.data)
    with pytest.raises(TypeError, match="^list_region: out holds fewer"):
        svo.list_region(lo, size, capacity=7, out=out)  # one over
    two_d = np.zeros((2, 3), dtype=hip.BLOCK_AT_DTYPE)
    rec.total = 4
    (got, n), _, a = call(rec, svo.list_region, lo, size, out=two_d)
    assert got.shape == (4,) and a[5] == two_d.ctypes.data and a[6] == 6


def test_list_region_on_the_device(svo, rec):
    lo, size = (1, -2, 3), (4, 2, 3)
    out = records("device", 6, hip.BLOCK_AT_DTYPE)
    for capacity, asked in ((None, 6), (4, 4), (6, 6), (0, 0)):
        (got, total), name, a = call(rec, svo.list_region, lo, size, hip.VX_LIST_FACES, capacity, out)
        assert name == "vx_list_region" and (a[0], list(a[1]), list(a[2])) == (svo._h.value, list(lo), list(size))
        assert a[3:5] == [hip.VX_LIST_FACES, DEVICE] and a[5] == (out.data_ptr() if asked else None) and a[6] == asked
        assert got is out and isinstance(total, torch.Tensor) and total.dtype == torch.int32 and tuple(total.shape) == (1,) and a[7] == total.data_ptr()
        assert int(total[0]) == 0
    with pytest.raises(TypeError, match="^list_region: out holds fewer"):
        svo.list_region(lo, size, capacity=7, out=out)
    # whole records: 12 int32 are six records under any shape, 13 are not
    (got, _), _, a = call(rec, svo.list_region, lo, size, out=Dev(torch.zeros(12, dtype=torch.int32)))
    assert a[6] == 6
    with pytest.raises(TypeError, match="^list_region: out must be a contiguous CUDA tensor of whole 8-byte records"):
        svo.list_region(lo, size, out=Dev(torch.zeros(13, dtype=torch.int32)))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_overlap_boxes_and_move_boxes(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    forms, others = vec_forms(side, n), vec_forms(side, n, one=True)
    for k, (label, o, o_at, o_stride) in enumerate(forms):
        _, e, e_at, e_stride = others[(k + 1) % len(others)]
        _, f, f_at, f_stride = others[(k + 2) % len(others)]
        _, m, m_at, m_stride = others[(k + 3) % len(others)]
        for offset in (None, f):
            for given in (True, False):
                if not given and side == "device":
                    continue
                out = records(side, n, hip.BOX_HIT_DTYPE) if given else None
                got, name, a = call(rec, svo.overlap_boxes, o, e, offset, 7, out)
                assert name == "vx_overlap_boxes" and a[0] == svo._h.value and a[2:] == [n, mem, addr(got)], label
                expected = {"origin": o_at, "origin_stride": o_stride, "extents": e_at, "extents_stride": e_stride, "only_value": 7,
                            "offset": None if offset is None else f_at, "offset_stride": 0 if offset is None else f_stride}
                assert struct(a[1]) == expected, label
                assert got is out if given else fresh(got, hip.BOX_HIT_DTYPE, (n,)) is None
                out = records(side, n, hip.MOVE_HIT_DTYPE) if given else None
                got, name, a = call(rec, svo.move_boxes, o, e, m, offset, 0.05, 0.25, hip.VX_MOVE_ORDER_ZYX, 7, out)
                assert name == "vx_move_boxes" and a[0] == svo._h.value and a[2:5] == [m_at, m_stride, n] and a[6:] == [mem, addr(got)], label
                assert struct(a[1]) == expected, label
                assert struct(a[5]) == {"scale": F32(0.05), "skin": 0.25, "order": hip.VX_MOVE_ORDER_ZYX, "flags": 0}
                assert got is out if given else fresh(got, hip.MOVE_HIT_DTYPE, (n,)) is None
    _, o, _, _ = forms[0]
    _, _, a = call(rec, svo.move_boxes, o, o, o, out=records(side, n, hip.MOVE_HIT_DTYPE))
    assert struct(a[5]) == {"scale": 1.0, "skin": 2.0 ** -10, "order": hip.VX_MOVE_ORDER_YXZ, "flags": 0} and struct(a[1])["only_value"] == 0
    # entity_boxes gives all three of the records in place
    ents = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    if side == "host" or n:
        src = ents if side == "host" else torch.from_numpy(ents.view(np.uint8))
        boxes = hip.entity_boxes(src) if side == "host" else tuple(Dev(x) for x in hip.entity_boxes(src))
        _, _, a = call(rec, svo.overlap_boxes, *boxes, out=records(side, n, hip.BOX_HIT_DTYPE))
        stride = 64 if n > 1 else 12
        assert struct(a[1]) == {"origin": addr(ents), "origin_stride": stride, "extents": addr(ents) + 36, "extents_stride": stride, "offset": addr(ents) + 24,
                                "offset_stride": stride, "only_value": 0}


FIELD_STRIDES = ((0, 64), (64, 64), (80, 80))  # (field_stride as given, the row's bytes): 4 x 4 x 4 cells


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_flood_points_and_walk_points(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    goals = vec_forms(side, n, one=True)
    for k, (label, p, at, stride) in enumerate(vec_forms(side, n)):
        _, g, g_at, g_stride = goals[(k + 2) % len(goals)]
        given_stride, row = FIELD_STRIDES[k % 3]
        for given in (True, False):
            if not given and side == "device":
                continue
            fields, info = (zeros(side, (n, row), np.uint8), records(side, n, hip.FLOOD_INFO_DTYPE)) if given else (True, True)
            (g_fields, g_info), name, a = call(rec, svo.flood_points, p, (4, 4, 4), (1, 2, 3), 77, 5, hip.VX_FLOOD_SEED_ALWAYS, fields, info, given_stride)
            assert name == "vx_flood_points" and a[:4] == [svo._h.value, at, stride, n] and a[5:] == [mem, addr(g_fields), given_stride, addr(g_info)], label
            assert struct(a[4]) == {"size": [4, 4, 4], "seed_at": [1, 2, 3], "max_steps": 77, "pass_value": 5, "flags": hip.VX_FLOOD_SEED_ALWAYS}
            if given:
                assert g_fields is fields and g_info is info
            else:
                fresh(g_fields, np.uint8, (n, row))
                fresh(g_info, hip.FLOOD_INFO_DTYPE, (n,))
            fields, info, paths = (zeros(side, (n, row), np.uint8), records(side, n, hip.WALK_INFO_DTYPE), zeros(side, (n, 6), np.uint32)) if given else (True, True, True)
            (g_fields, g_info, g_paths), name, a = call(rec, svo.walk_points, p, (4, 4, 4), g, (1, 2, 3), 77, 5, 3, 2, 4, 6, hip.VX_WALK_STOP_AT_GOAL, fields, info, paths,
                                                        given_stride)
            assert name == "vx_walk_points" and a[:6] == [svo._h.value, at, stride, g_at, g_stride, n], label
            assert a[7:] == [mem, addr(g_fields), given_stride, addr(g_paths), addr(g_info)], label
            assert struct(a[6]) == {"size": [4, 4, 4], "seed_at": [1, 2, 3], "max_steps": 77, "pass_value": 5, "height": 3, "climb": 2, "drop": 4, "path_capacity": 6,
                                    "flags": hip.VX_WALK_STOP_AT_GOAL}
            if given:
                assert g_fields is fields and g_info is info and g_paths is paths
            else:
                fresh(g_fields, np.uint8, (n, row))
                fresh(g_info, hip.WALK_INFO_DTYPE, (n,))
                fresh(g_paths, np.uint32, (n, 6))
    # the defaults, no goals: the centre cell, nothing for the paths
    _, p, at, stride = vec_forms(side, n)[0]
    (_, _), _, a = call(rec, svo.flood_points, p, (4, 6, 9), fields=zeros(side, (n, 224), np.uint8), info=records(side, n, hip.FLOOD_INFO_DTYPE))
    assert struct(a[4]) == {"size": [4, 6, 9], "seed_at": [2, 3, 4], "max_steps": hip.VX_FLOOD_MAX_STEPS, "pass_value": 0, "flags": 0} and a[7] == 0
    (_, _, g_paths), _, a = call(rec, svo.walk_points, p, (4, 6, 9), fields=zeros(side, (n, 224), np.uint8), info=records(side, n, hip.WALK_INFO_DTYPE))
    assert struct(a[6]) == {"size": [4, 6, 9], "seed_at": [2, 3, 4], "max_steps": hip.VX_WALK_MAX_STEPS, "pass_value": 0, "height": 2, "climb": 1, "drop": 3,
                            "path_capacity": 0, "flags": 0}
    assert a[3:5] == [None, 0] and a[9:11] == [0, None] and g_paths is None


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("side", SIDES)
def test_light_boxes_and_label_boxes(svo, rec, side, n):
    mem = HOST if side == "host" else DEVICE
    for k, (label, lo, at, stride) in enumerate(lo_forms(side, n)):
        given_stride, row = FIELD_STRIDES[k % 3]
        for given in (True, False):
            if not given and side == "device":
                continue
            fields, info = (zeros(side, (n, row), np.uint8), records(side, n, hip.LIGHT_INFO_DTYPE)) if given else (None, None)
            (g_fields, g_info), name, a = call(rec, svo.light_boxes, lo, (4, 4, 4), PROPS, hip.VX_LIGHT_NO_SKY, fields, info, given_stride)
            assert name == "vx_light_boxes" and a[:4] == [svo._h.value, at, stride, n] and a[5:] == [mem, addr(g_fields), given_stride, addr(g_info)], label
            shape = struct(a[4])
            assert (shape["size"], shape["flags"], shape["props_count"]) == ([4, 4, 4], hip.VX_LIGHT_NO_SKY, 3)
            assert C.string_at(shape["props"], 3) == bytes(PROPS)  # (the table is alive for as long as the struct is looked at here)
            if given:
                assert g_fields is fields and g_info is info
            else:
                fresh(g_fields, np.uint8, (n, row))
                fresh(g_info, hip.LIGHT_INFO_DTYPE, (n,))
            fields, pieces, info = ((zeros(side, (n, row), np.uint8), records(side, (n, 2), hip.LABEL_PIECE_DTYPE), records(side, n, hip.LABEL_INFO_DTYPE)) if given
                                    else (None, None, None))
            (g_fields, g_pieces, g_info), name, a = call(rec, svo.label_boxes, lo, (4, 4, 4), 0x15, 2, 99, 5, fields, pieces, info, given_stride)
            assert name == "vx_label_boxes" and a[:4] == [svo._h.value, at, stride, n], label
            assert a[5:] == [mem, addr(g_fields), given_stride, addr(g_pieces), addr(g_info)], label
            assert struct(a[4]) == {"size": [4, 4, 4], "anchor_faces": 0x15, "max_pieces": 2, "max_steps": 99, "pass_value": 5, "flags": 0}
            if given:
                assert g_fields is fields and g_pieces is pieces and g_info is info
            else:
                fresh(g_fields, np.uint8, (n, row))
                fresh(g_pieces, hip.LABEL_PIECE_DTYPE, (n, 2))
                fresh(g_info, hip.LABEL_INFO_DTYPE, (n,))
    _, lo, _, _ = lo_forms(side, n)[0]
    _, _, a = call(rec, svo.light_boxes, lo, (4, 6, 9), [], fields=zeros(side, (n, 224), np.uint8), info=records(side, n, hip.LIGHT_INFO_DTYPE))
    shape = struct(a[4])
    assert (shape["size"], shape["flags"], shape["props"], shape["props_count"]) == ([4, 6, 9], 0, None, 0) and a[7] == 0
    _, _, a = call(rec, svo.label_boxes, lo, (4, 6, 9), fields=zeros(side, (n, 224), np.uint8), pieces=records(side, (n, 250), hip.LABEL_PIECE_DTYPE),
                   info=records(side, n, hip.LABEL_INFO_DTYPE))
    assert struct(a[4]) == {"size": [4, 6, 9], "anchor_faces": hip.VX_LABEL_ALL_FACES, "max_pieces": hip.VX_LABEL_MAX_PIECES, "max_steps": hip.VX_LABEL_MAX_STEPS,
                            "pass_value": 0, "flags": 0}


@pytest.mark.parametrize("n", COUNTS)
def test_physics_step(svo, rec, n):
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    for want in (False, True):
        got, name, a = call(rec, svo.physics_step, e, 0.05, 3, want)
        assert name == "vx_physics_step" and a == [svo._h.value, e.ctypes.data, n, HOST, F32(0.05), 3, addr(got) if want else None]
        assert got is None if not want else fresh(got, hip.AABB_RESULT_DTYPE, (n,)) is None
    t = Dev(torch.from_numpy(e.view(np.uint8)))
    contacts = Dev(torch.zeros((n, 6), dtype=torch.float32))
    got, _, a = call(rec, svo.physics_step, t, 0.05)
    assert got is None and a == [svo._h.value, addr(t), n, DEVICE, F32(0.05), 1, None]
    got, _, a = call(rec, svo.physics_step, t, 0.05, 2, True, None, contacts)
    assert got is contacts and a == [svo._h.value, addr(t), n, DEVICE, F32(0.05), 2, addr(contacts)]
    got, _, a = call(rec, svo.physics_step, 0x7000, 0.05, 2, True, 9, 0x9000)  # raw pointers
    assert got == 0x9000 and a == [svo._h.value, 0x7000, 9, DEVICE, F32(0.05), 2, 0x9000]
    got, _, a = call(rec, svo.physics_step, t, 0.05, want_contacts=True)  # a fresh tensor on the entities' device (the CPU, here)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (n, 6) and a[6] == (got.data_ptr() or None)


# ---- what every method refuses ----------------------------------------------------------------------------------------------------------------

N = 5


def items(side, dtype, count):
    """A flat output of `count` items: records (int32 words on the device), or plain numbers."""
    return records(side, count, dtype) if dtype.names else zeros(side, (count,), dtype)


def arguments(method, side, n=N, delta=None):
    """The keyword arguments of a valid call of `method` with every output supplied, flat; delta: {output: items more or fewer than it needs}."""
    d = delta or {}
    out = lambda name, dtype, count: items(side, np.dtype(dtype), count + d.get(name, 0))  # noqa: E731
    f32 = lambda: zeros(side, (n, 3), F32)  # noqa: E731
    i32 = lambda: zeros(side, (n, 3), np.int32)  # noqa: E731
    if method == "raycast_batch":
        return dict(origins=f32(), dirs=f32(), out=out("out", hip.RAY_HIT_DTYPE, n))
    if method == "trace_rays":
        return dict(uniforms=U, origins=f32(), dirs=f32(), want_hits=True, out=(out("rgba", F32, 4 * n), out("hits", hip.HIT_DTYPE, n)))
    if method == "trace_views":
        return dict(views=[U] * n, width=3, height=2, want_hits=True, out=(out("rgba", F32, 4 * 6 * n), out("hits", hip.HIT_DTYPE, 6 * n)))
    if method == "block_points":
        return dict(positions=f32(), out=out("out", hip.BLOCK_CELL_DTYPE, n))
    if method == "read_region":
        return dict(lo=(1, 2, 3), size=(n, 2, 3), out=out("out", np.uint32, 6 * n))
    if method == "list_region":
        return dict(lo=(1, 2, 3), size=(n, 2, 3), out=out("out", hip.BLOCK_AT_DTYPE, n))
    if method == "scan_points":
        return dict(positions=f32(), direction=hip.VX_DIR_NEG_Y, out=out("out", hip.SCAN_HIT_DTYPE, n))
    if method == "scan_columns":
        return dict(lo=(1, 2, 3), size=(n, 2, 3), direction=hip.VX_DIR_NEG_Y, out=out("out", hip.SCAN_HIT_DTYPE, 3 * n))
    if method == "overlap_boxes":
        return dict(origin=f32(), extents=f32(), offset=f32(), out=out("out", hip.BOX_HIT_DTYPE, n))
    if method == "move_boxes":
        return dict(origin=f32(), extents=f32(), motion=f32(), offset=f32(), out=out("out", hip.MOVE_HIT_DTYPE, n))
    if method == "flood_points":
        return dict(positions=f32(), size=(4, 4, 4), fields=out("fields", np.uint8, 64 * n), info=out("info", hip.FLOOD_INFO_DTYPE, n))
    if method == "light_boxes":
        return dict(lo=i32(), size=(4, 4, 4), props=PROPS, fields=out("fields", np.uint8, 64 * n), info=out("info", hip.LIGHT_INFO_DTYPE, n))
    if method == "label_boxes":
        return dict(lo=i32(), size=(4, 4, 4), max_pieces=2, fields=out("fields", np.uint8, 64 * n), pieces=out("pieces", hip.LABEL_PIECE_DTYPE, 2 * n),
                    info=out("info", hip.LABEL_INFO_DTYPE, n))
    if method == "walk_points":
        return dict(positions=f32(), size=(4, 4, 4), goals=f32(), path_capacity=4, fields=out("fields", np.uint8, 64 * n), info=out("info", hip.WALK_INFO_DTYPE, n),
                    paths=out("paths", np.uint32, 4 * n))
    raise KeyError(method)


METHODS = ("raycast_batch", "trace_rays", "trace_views", "block_points", "read_region", "list_region", "scan_points", "scan_columns", "overlap_boxes", "move_boxes",
           "flood_points", "light_boxes", "label_boxes", "walk_points")
VECTORS = {"raycast_batch": ("origins", "dirs"), "trace_rays": ("origins", "dirs"), "block_points": ("positions",), "scan_points": ("positions",),
           "overlap_boxes": ("origin", "extents", "offset"), "move_boxes": ("origin", "extents", "motion", "offset"), "flood_points": ("positions",),
           "walk_points": ("positions", "goals")}
FIRST = {m: v[0] for m, v in VECTORS.items()}  # the argument that says how many, and on which side
OUTPUTS = {"raycast_batch": ("out",), "trace_rays": ("rgba", "hits"), "trace_views": ("rgba", "hits"), "block_points": ("out",), "read_region": ("out",),
           "list_region": ("out",), "scan_points": ("out",), "scan_columns": ("out",), "overlap_boxes": ("out",), "move_boxes": ("out",),
           "flood_points": ("fields", "info"), "light_boxes": ("fields", "info"), "label_boxes": ("fields", "pieces", "info"),
           "walk_points": ("fields", "info", "paths")}


def every_method_accepts_its_arguments(svo, rec, side):
    for m in METHODS:
        getattr(svo, m)(**arguments(m, side))


@pytest.mark.parametrize("side", SIDES)
def test_the_refusal_table_starts_from_calls_that_pass(svo, rec, side):
    every_method_accepts_its_arguments(svo, rec, side)
    assert [name for name, _ in rec.calls] == ["vx_" + m for m in METHODS]


def with_output(kw, name, change):
    """kw with the output `name` put through change (trace_*: a member of the `out` pair)."""
    if name in ("rgba", "hits") and "out" in kw:
        pair = list(kw["out"])
        pair[name == "hits"] = change(pair[name == "hits"])
        return dict(kw, out=tuple(pair))
    return dict(kw, **{name: change(kw[name])})


def strided(x, rows, row_stride, last=1):
    """(rows, 3) over x's memory at a row stride and a component stride in elements, on either side."""
    if isinstance(x, np.ndarray):
        return np.lib.stride_tricks.as_strided(x, (rows, 3), (row_stride * x.itemsize, last * x.itemsize))
    return Dev(torch.as_strided(x.t, (rows, 3), (row_stride, last)))


def refusals():
    """(id, method, side, the keyword arguments' change): every one a TypeError that names the method called."""
    rows = []
    add = lambda what, m, side, change: rows.append(pytest.param(m, side, change, id=f"{m}-{side}-{what}"))  # noqa: E731
    for side in SIDES:
        for m, names in VECTORS.items():
            for name in names:
                add(f"{name} float64", m, side, lambda kw, name=name, side=side: dict(kw, **{name: zeros(side, (N, 3), np.float64)}))
                add(f"{name} not adjacent", m, side, lambda kw, name=name, side=side: dict(kw, **{name: strided(zeros(side, (N, 6), F32), N, 6, 2)}))
                if name != FIRST[m]:
                    add(f"{name} of another count", m, side, lambda kw, name=name, side=side: dict(kw, **{name: zeros(side, (N - 1, 3), F32)}))
                    add(f"{name} of two components", m, side, lambda kw, name=name, side=side: dict(kw, **{name: zeros(side, (N, 2), F32)}))
            if m != "trace_rays":  # (its origins' shape and side are refused in raycast_batch's name: _ray_batch's own messages, which stay)
                add("wrong shape", m, side, lambda kw, m=m, side=side: dict(kw, **{FIRST[m]: zeros(side, (N, 2), F32)}))
                add("one axis", m, side, lambda kw, m=m, side=side: dict(kw, **{FIRST[m]: zeros(side, (N * 3,), F32)}))
                other = "device" if side == "host" else "host"
                for name in names[1:]:
                    add(f"{name} on the other side", m, side, lambda kw, name=name, other=other: dict(kw, **{name: zeros(other, (N, 3), F32)}))
        for m in ("raycast_batch", "trace_rays"):
            add("max_dst float64", m, side, lambda kw, side=side: dict(kw, max_dst=zeros(side, (N,), np.float64)))
            add("max_dst of another count", m, side, lambda kw, side=side: dict(kw, max_dst=zeros(side, (N + 1,), F32)))
            add("max_dst two-dimensional", m, side, lambda kw, side=side: dict(kw, max_dst=zeros(side, (N, 1), F32)))
        for m in ("light_boxes", "label_boxes"):
            add("lo wrong shape", m, side, lambda kw, side=side: dict(kw, lo=zeros(side, (N, 4), np.int32)))
            add("lo int64", m, side, lambda kw, side=side: dict(kw, lo=zeros(side, (N, 3), np.int64)))
            add("lo float32", m, side, lambda kw, side=side: dict(kw, lo=zeros(side, (N, 3), F32)))
            add("lo at 8 bytes", m, side, lambda kw, side=side: dict(kw, lo=strided(zeros(side, (N, 3), np.int32), N, 2)))
            add("lo not adjacent", m, side, lambda kw, side=side: dict(kw, lo=strided(zeros(side, (N, 6), np.int32), N, 6, 2)))
        for m in ("trace_rays", "trace_views"):
            add("nothing asked for", m, side, lambda kw: dict(kw, want_hits=False, want_rgba=False))
    # negative row strides: NumPy only (torch has none)
    for m, names in VECTORS.items():
        for name in names:
            add(f"{name} backwards", m, "host", lambda kw, name=name: dict(kw, **{name: kw[name][::-1]}))
    for m in ("light_boxes", "label_boxes"):
        add("lo backwards", m, "host", lambda kw: dict(kw, lo=kw["lo"][::-1]))
        add("lo at 6 bytes", m, "host", lambda kw: dict(kw, lo=np.lib.stride_tricks.as_strided(np.zeros((N, 3), dtype=np.int32), (N, 3), (14, 4))))
    # a CPU torch tensor where a CUDA one is required
    for m in METHODS:
        if m in FIRST and m != "trace_rays":
            add("a CPU tensor", m, "device", lambda kw, m=m: dict(kw, **{FIRST[m]: kw[FIRST[m]].t}))
        if m in ("light_boxes", "label_boxes"):
            add("lo a CPU tensor", m, "device", lambda kw: dict(kw, lo=kw["lo"].t))
        for name in OUTPUTS[m]:
            add(f"{name} a CPU tensor", m, "device", lambda kw, name=name: with_output(kw, name, lambda x: x.t))
    for m in ("overlap_boxes", "move_boxes"):
        add("device=True with NumPy boxes", m, "host", lambda kw: dict(kw, device=True))
        add("extents a CPU tensor", m, "device", lambda kw: dict(kw, extents=kw["extents"].t))
    for m in ("read_region", "scan_columns", "trace_views"):
        add("the outputs of the other side under device=True", m, "host", lambda kw: dict(kw, device=True) if "views" not in kw else dict(kw, out=(kw["out"][0], Dev(torch.zeros(1)))))
    return rows


def smaller(m, side, name):
    """A valid call's arguments with the output `name` one item short."""
    return arguments(m, side, delta={name: -1})


def output_refusals():
    """Every output: too small, of another dtype, not contiguous, read-only, no array at all."""
    rows = []
    add = lambda what, m, side, change: rows.append(pytest.param(m, side, change, id=f"{m}-{side}-{what}"))  # noqa: E731

    def other_dtype(x):  # the same bytes under another dtype
        return x.view(np.int8) if x.dtype == np.uint8 else x.view(np.uint8)

    def every_second(x):  # as many items, not contiguous
        if isinstance(x, np.ndarray):
            return np.zeros(2 * x.size, dtype=x.dtype)[::2]
        return Dev(torch.zeros((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype)[::2])

    def read_only(x):
        x = x.copy()
        x.setflags(write=False)
        return x

    for side in SIDES:
        for m in METHODS:
            for name in OUTPUTS[m]:
                if m != "list_region":  # (whatever it holds is its capacity: test_list_region_*)
                    add(f"{name} too small", m, side, lambda kw, m=m, side=side, name=name: smaller(m, side, name))
                add(f"{name} not contiguous", m, side, lambda kw, name=name: with_output(kw, name, every_second))
                if side == "host":
                    add(f"{name} read-only", m, side, lambda kw, name=name: with_output(kw, name, read_only))
                    add(f"{name} a list", m, side, lambda kw, name=name: with_output(kw, name, lambda x: x.tolist()))
                    if not m.startswith("trace_"):  # (their outputs are so many bytes: float32 or uint8 pixels by fmt)
                        add(f"{name} of another dtype", m, side, lambda kw, name=name: with_output(kw, name, other_dtype))
    return rows


def refused(svo, rec, m, side, change):
    kw = arguments(m, side)
    getattr(svo, m)(**kw)  # (passes as it is)
    del rec.calls[:]
    with pytest.raises(TypeError) as e:
        getattr(svo, m)(**change(kw))
    assert not rec.calls
    return str(e.value)


@pytest.mark.parametrize("m, side, change", refusals())
def test_refusals_of_the_inputs(svo, rec, m, side, change):
    message = refused(svo, rec, m, side, change)
    assert message.startswith(m + ": "), message


@pytest.mark.parametrize("m, side, change", output_refusals())
def test_refusals_of_the_outputs(svo, rec, m, side, change):
    message = refused(svo, rec, m, side, change)
    assert message.startswith(m + ": "), message


def test_physics_step_refusals(svo, rec):
    e = np.zeros(4, dtype=hip.ENTITY_DTYPE)
    read_only = e.copy()
    read_only.setflags(write=False)
    for bad in (e.view(np.uint8), np.zeros(8, dtype=hip.ENTITY_DTYPE)[::2], read_only):
        with pytest.raises(TypeError, match="^physics_step: host entities"):
            svo.physics_step(bad, 0.05)
    with pytest.raises(TypeError, match="^physics_step: a raw device pointer needs count"):
        svo.physics_step(0x7000, 0.05)
    with pytest.raises(TypeError, match="^physics_step: contacts of a raw device pointer"):
        svo.physics_step(0x7000, 0.05, want_contacts=True, count=4)
    for bad in (torch.zeros(65, dtype=torch.uint8), torch.zeros((4, 128), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(TypeError, match="^physics_step: a device tensor"):
            svo.physics_step(Dev(bad), 0.05)
    assert not rec.calls


# ---- the size rule of every output: one item over, one item under ------------------------------------------------------------------------------

EXACT, AT_LEAST = "exact", "at least"
SIZE_RULES = [  # (method, output, on the host, on the device)
    ("raycast_batch", "out", EXACT, EXACT), ("block_points", "out", EXACT, EXACT), ("scan_points", "out", EXACT, EXACT), ("scan_columns", "out", EXACT, EXACT),
    ("read_region", "out", EXACT, EXACT),
    ("overlap_boxes", "out", EXACT, AT_LEAST), ("move_boxes", "out", EXACT, AT_LEAST),
    ("flood_points", "info", EXACT, AT_LEAST), ("light_boxes", "info", EXACT, AT_LEAST), ("label_boxes", "info", EXACT, AT_LEAST), ("walk_points", "info", EXACT, AT_LEAST),
    ("label_boxes", "pieces", EXACT, AT_LEAST),
    ("flood_points", "fields", AT_LEAST, AT_LEAST), ("light_boxes", "fields", AT_LEAST, AT_LEAST), ("label_boxes", "fields", AT_LEAST, AT_LEAST),
    ("walk_points", "fields", AT_LEAST, AT_LEAST), ("walk_points", "paths", AT_LEAST, AT_LEAST),
    ("trace_rays", "rgba", AT_LEAST, AT_LEAST), ("trace_rays", "hits", AT_LEAST, AT_LEAST), ("trace_views", "rgba", AT_LEAST, AT_LEAST),
    ("trace_views", "hits", AT_LEAST, AT_LEAST),
]


def test_the_size_rules_cover_every_output():
    assert sorted((m, o) for m, o, _, _ in SIZE_RULES) == sorted((m, o) for m in METHODS if m != "list_region" for o in OUTPUTS[m])


@pytest.mark.parametrize("m, name, on_host, on_device", SIZE_RULES, ids=[f"{m}-{o}" for m, o, _, _ in SIZE_RULES])
def test_size_rule(svo, rec, m, name, on_host, on_device):
    for side, rule in (("host", on_host), ("device", on_device)):
        with pytest.raises(TypeError, match=f"^{m}: "):  # one item under: never
            getattr(svo, m)(**arguments(m, side, delta={name: -1}))
        del rec.calls[:]
        over = arguments(m, side, delta={name: 1})
        if rule == EXACT:  # one item over: refused
            with pytest.raises(TypeError, match=f"^{m}: "):
                getattr(svo, m)(**over)
            assert not rec.calls
        else:  # one item over: accepted, and handed back as it is
            got = getattr(svo, m)(**over)
            given = dict(zip(("rgba", "hits"), over["out"]))[name] if m.startswith("trace_") else over[name]
            assert len(rec.calls) == 1 and any(g is given for g in (got if isinstance(got, tuple) else (got,)))


# ---- None, True and False for fields, info, pieces and paths ------------------------------------------------------------------------------------

FRESH, NONE = "fresh", "none"
CONVENTIONS = [  # (method, argument, what None means, its place in the call, its place in what comes back)
    ("flood_points", "fields", NONE, 6, 0), ("flood_points", "info", NONE, 8, 1),
    ("walk_points", "fields", NONE, 8, 0), ("walk_points", "info", NONE, 11, 1),
    ("light_boxes", "fields", FRESH, 6, 0), ("light_boxes", "info", FRESH, 8, 1),
    ("label_boxes", "fields", FRESH, 6, 0), ("label_boxes", "pieces", FRESH, 8, 1), ("label_boxes", "info", FRESH, 9, 2),
]


@pytest.mark.parametrize("m, name, none_means, at, back", CONVENTIONS, ids=[f"{m}-{o}" for m, o, _, _, _ in CONVENTIONS])
def test_none_true_false(svo, rec, m, name, none_means, at, back):
    kw = arguments(m, "host")
    for value, means in ((True, FRESH), (False, NONE), (None, none_means)):
        got, _, a = call(rec, getattr(svo, m), **dict(kw, **{name: value}))
        others = [i for i in range(len(got)) if i != back]
        assert all(got[i] is kw[OUTPUTS[m][i]] for i in others)
        if means == NONE:
            assert got[back] is None and a[at] is None
        else:
            assert isinstance(got[back], np.ndarray) and got[back] is not kw[name] and a[at] == got[back].ctypes.data
    # the device side reads the three values alike: none stays none (fresh needs a GPU)
    kw = arguments(m, "device")
    for value in (False,) + ((None,) if none_means == NONE else ()):
        got, _, a = call(rec, getattr(svo, m), **dict(kw, **{name: value}))
        assert got[back] is None and a[at] is None


def test_walk_points_paths_none(svo, rec):
    """paths=None: fresh memory when goals are given and path_capacity > 0, else none; True and False as everywhere."""
    kw = arguments("walk_points", "host")
    for goals, capacity, paths, means in ((kw["goals"], 4, None, FRESH), (None, 4, None, NONE), (kw["goals"], 0, None, NONE), (None, 0, None, NONE),
                                          (kw["goals"], 4, False, NONE), (None, 4, True, FRESH), (kw["goals"], 0, True, FRESH), (None, 0, False, NONE)):
        (_, _, got), _, a = call(rec, svo.walk_points, **dict(kw, goals=goals, path_capacity=capacity, paths=paths))
        if means == NONE:
            assert got is None and a[10] is None
        else:
            fresh(got, np.uint32, (N, capacity))
            assert a[10] == got.ctypes.data
    kw = arguments("walk_points", "device")
    (_, _, got), _, a = call(rec, svo.walk_points, **dict(kw, goals=None, paths=None))
    assert got is None and a[10] is None


def test_label_boxes_pieces_none(svo, rec):
    """pieces=None: fresh memory, but none with max_pieces == 0; True with max_pieces == 0: an array of no records."""
    kw = arguments("label_boxes", "host")
    for most, pieces, shape in ((2, None, (N, 2)), (0, None, None), (0, False, None), (0, True, (N, 0)), (3, True, (N, 3))):
        (_, got, _), _, a = call(rec, svo.label_boxes, **dict(kw, max_pieces=most, pieces=pieces))
        if shape is None:
            assert got is None and a[8] is None
        else:
            fresh(got, hip.LABEL_PIECE_DTYPE, shape)
            assert a[8] == got.ctypes.data
    kw = arguments("label_boxes", "device")
    (_, got, _), _, a = call(rec, svo.label_boxes, **dict(kw, max_pieces=0, pieces=None))
    assert got is None and a[8] is None
