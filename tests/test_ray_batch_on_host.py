"""What a ray batch is (voxel-rs_amd/csrc/raycast/vx_ray_batch.hpp) without a GPU: the header vx_raycast_batch and vx_trace_rays share, compiled
for the host by the test-only harness tests/cpp/batch_on_host.cpp. A batch of strided arrays is packed the way the host-memory calls pack it and
read back the way the kernels' lanes read it: that must give the arrays' own values, and the same bytes as the gather over the arrays where they
lie (the device-memory calls). The plan's end is held against the formula stated here, and the rules against every value the ABI tests refuse.
`make sanitize` runs the same round on heap blocks under ASan (tests/cpp/sanitize_stress.cpp)."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import ROOT, vra  # noqa: F401
from voxel_rs_amd import hip

BUILD = Path(ROOT) / "tests" / "_build"
_vp = C.c_void_p
MAX_DST_ALL = 7.5

ORIGIN_STRIDES = [12, 16, 48, 64]  # packed, padded to a vec4, inside vx_picker_task records (at +16), inside vx_entity records
DIR_STRIDES = [0, 12, 20, 48]
MAX_DST = [None, 0, 4, 48]  # no array; else its stride


class RayBatchArgs(C.Structure):  # vxk::RayBatchArgs
    _fields_ = [("origin", _vp), ("dir", _vp), ("max_dst", _vp), ("origin_stride", C.c_uint32), ("dir_stride", C.c_uint32), ("max_dst_stride", C.c_uint32),
                ("max_dst_all", C.c_float), ("has_max_dst", C.c_uint32), ("translucent", C.c_uint32)]


@pytest.fixture(scope="module")
def batchhost():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libbatch_on_host.so"
    csrc = Path(ROOT) / "voxel-rs_amd" / "csrc"
    deps = [Path(ROOT) / "tests" / "cpp" / "batch_on_host.cpp", csrc / "raycast" / "vx_ray_batch.hpp", csrc / "hip" / "vx_args.hpp",
            Path(ROOT) / "tests" / "cpp" / "shims" / "hip_on_host.hpp", Path(ROOT) / "include" / "voxel_hip.h"]
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", f"-I{ROOT}/include", f"-I{ROOT}/tests/cpp/shims",
               f"-I{csrc}/hip", f"-I{csrc}/raycast", str(deps[0]), "-o", str(so)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    lib = C.CDLL(str(so))
    lib.batchhost_last_error.restype = C.c_char_p
    return lib


def exact(rng, n, stride, width, lead=0):
    """`n` values of `width` floats at `stride` bytes (0: the one value), in a buffer of exactly lead + (n - 1) * stride + 4 * width bytes -- it ends
    with its last value, so a reader of whole strides runs off its end. Returns (buffer, the values as a strided view of it, the first one's address)."""
    count = n if stride else 1
    buf = np.zeros(lead + (count - 1) * stride + 4 * width, dtype=np.uint8)
    view = np.ndarray((count, width), dtype=np.float32, buffer=buf.data, offset=lead, strides=(stride if stride else 4 * width, 4))
    view[:] = rng.uniform(-100.0, 100.0, (count, width)).astype(np.float32)
    return buf, view, buf.ctypes.data + lead


def round16(v):
    return (v + 15) // 16 * 16


def gather(lib, args, n):
    out = np.zeros((n, 7), dtype=np.float32)
    for i in range(n):
        lib.batchhost_gather(C.byref(args), i, out[i].ctypes.data_as(_vp))
    return out


@pytest.mark.parametrize("n", [1, 3, 65])
def test_packed_and_in_place_gather_the_arrays_values(batchhost, n):
    rng = np.random.default_rng(n)
    for os_, ds, ms in itertools.product(ORIGIN_STRIDES, DIR_STRIDES, MAX_DST):
        what = f"n {n}, strides {os_} {ds} {ms}"
        o_buf, o, o_at = exact(rng, n, os_, 3, lead=16 if os_ == 48 else 0)
        d_buf, d, d_at = exact(rng, n, ds, 3)
        m_buf, m, m_at = exact(rng, n, ms or 0, 1)
        b = hip.RayBatch(o_at, d_at, None if ms is None else m_at, os_, ds, ms or 0, MAX_DST_ALL, 0)
        expected = np.zeros((n, 7), dtype=np.float32)
        expected[:, 0:3], expected[:, 3:6] = o, d  # (the one direction: broadcast)
        expected[:, 6] = MAX_DST_ALL if ms is None else m[:, 0]

        # the plan: today's layout, stated here on its own
        n_dir, n_dst = (n if ds else 1), (0 if ms is None else (n if ms else 1))
        at_dir = 12 * n
        at_dst = at_dir + 12 * n_dir
        at_hits = round16(at_dst + 4 * n_dst)
        plan = (C.c_uint64 * 5)()
        batchhost.batchhost_plan(C.byref(b), n, plan)
        assert list(plan) == [n_dir, n_dst, at_dir, at_dst, at_hits] and plan[4] % 16 == 0, what

        scratch = np.full(at_hits + 64, 0x5a, dtype=np.uint8)
        packed, in_place = RayBatchArgs(), RayBatchArgs()
        batchhost.batchhost_pack(C.byref(b), n, scratch.ctypes.data_as(_vp), C.byref(packed))
        batchhost.batchhost_in_place(C.byref(b), C.byref(in_place))
        assert (scratch[at_dst + 4 * n_dst:] == 0x5a).all(), what  # nothing is written behind the last distance
        assert (packed.origin, packed.dir, packed.max_dst) == (scratch.ctypes.data, scratch.ctypes.data + at_dir, scratch.ctypes.data + at_dst), what
        assert (in_place.origin, in_place.dir, in_place.max_dst) == (o_at, d_at, None if ms is None else m_at), what
        assert (in_place.origin_stride, in_place.dir_stride, in_place.max_dst_stride) == (os_, ds, ms or 0), what
        # packed strides: 12 | 0 or 12 | 0 or 4 -- 0 where one value is kept for every ray; a single ray's direction is kept as the one, its
        # distance, where there is an array, as an array of one
        assert packed.origin_stride == 12, what
        assert packed.dir_stride == (12 if ds and n > 1 else 0), what
        assert packed.max_dst_stride == (4 if ms is not None and (ms or n == 1) else 0), what
        for a in (packed, in_place):
            assert a.has_max_dst == (0 if ms is None else 1) and a.max_dst_all == MAX_DST_ALL and a.translucent == 0, what

        got_packed, got_in_place = gather(batchhost, packed, n), gather(batchhost, in_place, n)
        assert got_packed.tobytes() == got_in_place.tobytes(), what
        assert got_packed.tobytes() == expected.tobytes(), what


def test_in_place_carries_the_translucent_flag(batchhost):
    o = np.zeros(3, dtype=np.float32)
    a = RayBatchArgs()
    batchhost.batchhost_in_place(C.byref(hip.RayBatch(o.ctypes.data, o.ctypes.data, None, 12, 0, 0, -1.0, hip.VX_RAYS_TRANSLUCENT)), C.byref(a))
    assert a.translucent == 1 and a.has_max_dst == 0 and a.max_dst_all == -1.0


@pytest.mark.parametrize("who", [b"raycast_batch", b"trace_rays"])
def test_the_rules_refuse_what_the_abi_tests_list(batchhost, who):
    """Every bad value of test_raycast_batch_abi.py and test_trace_rays_abi.py, with the field named behind the entry point's name; the rules in
    their order; what the ABI tests accept is accepted."""
    o, d, m = np.zeros((4, 3), dtype=np.float32), np.ones((4, 3), dtype=np.float32), np.full(4, 9.0, dtype=np.float32)

    def check(**kw):
        b = hip.RayBatch(o.ctypes.data, d.ctypes.data, m.ctypes.data, 12, 12, 4, -1.0, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return batchhost.batchhost_check(C.byref(b), who), batchhost.batchhost_last_error()

    def refused(word, **kw):
        rc, msg = check(**kw)
        assert rc == 1 and msg.startswith(who + b": ") and word in msg, (word, rc, msg)

    for stride in (0, 4, 8, 13, 14, 2):
        refused(b"origin_stride", origin_stride=stride)
    for stride in (4, 8, 13, 18, 2):
        refused(b"dir_stride", dir_stride=stride)
    for stride in (1, 2, 7):
        refused(b"max_dst_stride", max_dst_stride=stride)
    for flags in (2, 4, 0x80000000 | hip.VX_RAYS_TRANSLUCENT):
        refused(b"flags", flags=flags)
    refused(b"null origin", origin=None)
    refused(b"null dir", dir=None)
    order = [(b"flags", dict(flags=4)), (b"null origin", dict(origin=None)), (b"null dir", dict(dir=None)), (b"origin_stride", dict(origin_stride=2)),
             (b"dir_stride", dict(dir_stride=2)), (b"max_dst_stride", dict(max_dst_stride=2))]
    for k, (word, bad) in enumerate(order):  # each rule wins over every later one
        kw = dict(bad)
        for _, rest in order[k + 1:]:
            kw.update(rest)
        refused(word, **kw)
    for ok in (dict(), dict(dir_stride=0, max_dst_stride=0, flags=hip.VX_RAYS_TRANSLUCENT), dict(origin_stride=64, dir_stride=48, max_dst_stride=48),
               dict(max_dst=None, max_dst_stride=3)):
        assert check(**ok) == (0, b""), ok
