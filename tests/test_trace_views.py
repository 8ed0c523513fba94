"""vx_trace_views on the GPU: many small views shaded in one launch (voxel-rs_amd/csrc/trace: kernels_views.hip), against the oracle
(OracleScene.render, view by view) and against vx_render with hit records, in host and in device memory. Records are compared byte for byte,
colours within the project's 5e-6. The cases -- five 20 x 13 views of three worlds, the heightfield's three 64 x 48 views -- are those of
tests/views_cases.py, computed once and left unchanged; test_trace_views_on_host.py shows from the oracle's results that they hold what they
were specified to hold."""
import ctypes as C

import numpy as np
import pytest

import trace_cases as tc
import views_cases as vc
from helpers import orc, vra  # noqa: F401
from physics_cases import heightfield
from voxel_rs_amd import hip, scenes

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
FORMATS = [hip.VX_FORMAT_RGBA32F, hip.VX_FORMAT_RGBA8]
FORMAT_IDS = ["rgba32f", "rgba8"]
WORLDS = [(n, f) for n in ("heightfield", "glasshouse", "far_chunks") for f in ("esvo", "csvo")]


@pytest.fixture(scope="module")
def contexts():
    """One context per (world, format), made when first asked for and closed with the module."""
    made = {}

    def get(name, fmt):
        if (name, fmt) not in made:
            c = tc.camera_case(name, fmt)
            svo = hip.Svo(c.svo_type, c.world.size_in_bytes + (1 << 20))
            svo.set_materials(c.mats)
            svo.set_textures(c.tex, 6)
            svo.update_full(c.world)  # (the shared world keeps dirty ranges for one target only, and test_trace_rays.py's contexts had them)
            made[name, fmt] = svo
        return made[name, fmt]

    yield get
    for svo in made.values():
        svo.close()


def assert_pixels(fmt, got, exp_colors, what):
    """RGBA32F within 5e-6. RGBA8: a byte may differ by one step only where the expected float lies within 5e-6 * 255 of a rounding boundary
    (test_trace_rays.assert_pixels' rule)."""
    exp = np.asarray(exp_colors, dtype=np.float64).reshape(-1, 4)
    if fmt == hip.VX_FORMAT_RGBA32F:
        tc.assert_colors(got, exp, what)
        return
    scaled = np.clip(exp, 0.0, 1.0) * 255.0 + 0.5
    lo, hi = np.floor(scaled - tc.TOL * 255.0), np.floor(scaled + tc.TOL * 255.0)
    g = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    assert ((g >= lo) & (g <= np.minimum(hi, 255.0))).all(), f"{what}: an RGBA8 byte is not the packing of a colour within 5e-6 of the expected one"


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("name,fmt", WORLDS)
def test_small_views_are_the_oracles_renders(contexts, name, fmt, pixel_format):
    """1: case (a) in host memory: per view, records byte for byte and colours within 5e-6 of OracleScene.render."""
    c, svo = vc.small_views(name, fmt), contexts(name, fmt)
    rgba, hits = svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format)
    assert rgba.shape == (5, 13, 20, 4) and hits.shape == (5, 260)
    exp_img, exp_hits = vc.expected(c, pixel_format)
    for k in range(len(c.views)):
        tc.assert_records(hits[k], exp_hits[k], f"{name}-{fmt} view {k} against the oracle")
        assert_pixels(pixel_format, rgba[k], exp_img[k], f"{name}-{fmt} view {k} against the oracle")


def render_reference(svo, u, w, h, pixel_format):
    """(colours [H, W, 4], records [H * W]) of vx_render for a whole-image host target of that format. An RGBA8 target whose height is no multiple
    of 8 is not asked of vx_render: its cost notes (note_cost_wave, kernels_render.hip) look number_of_place up through the output index of the
    lanes outside the image too, and for an RGBA8 target that index underflows above the top row -- a read far outside the table (an illegal
    memory access on the GPU). There vx_render's RGBA32F image and records stand in, with the rows flipped as include/voxel_hip.h states for RGBA8."""
    if pixel_format == hip.VX_FORMAT_RGBA32F or h % 8 == 0:
        img, hits = svo.render(u, w, h, want_hits=True, fmt=pixel_format)
        return img, hits.reshape(-1)
    img, hits = svo.render(u, w, h, want_hits=True)
    return np.ascontiguousarray(img[::-1]), np.ascontiguousarray(hits[::-1]).reshape(-1)


def against_render(svo, c, pixel_format, what):
    rgba, hits = svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format)
    for k, u in enumerate(c.views):
        img, rhits = render_reference(svo, u, c.width, c.height, pixel_format)
        tc.assert_records(hits[k], rhits, f"{what} view {k} against vx_render")
        if img.dtype == np.uint8:  # the packing of colours within 5e-6 of each other: a step apart at the most, in vx_render's row order
            assert np.abs(rgba[k].astype(np.int32) - img.astype(np.int32)).max() <= 1
        else:
            assert_pixels(pixel_format, rgba[k], img, f"{what} view {k} against vx_render")


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("name,fmt", WORLDS)
def test_small_views_are_vx_renders(contexts, name, fmt, pixel_format):
    """2: case (a) against vx_render view by view: records byte for byte (so the row order of each view is vx_render's for that format), colours
    within 5e-6."""
    against_render(contexts(name, fmt), vc.small_views(name, fmt), pixel_format, f"{name}-{fmt}")


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_the_camera_batch_is_vx_renders_and_the_oracles(contexts, fmt, pixel_format):
    """2: case (b), the heightfield's three 64 x 48 views as one batch, against vx_render and the oracle."""
    c, svo = vc.camera_batch(fmt), contexts("heightfield", fmt)
    against_render(svo, c, pixel_format, f"heightfield-{fmt} camera batch")
    rgba, hits = svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format)
    exp_img, exp_hits = vc.expected(c, pixel_format)
    for k in range(3):
        tc.assert_records(hits[k], exp_hits[k], f"heightfield-{fmt} camera batch view {k} against the oracle")
        assert_pixels(pixel_format, rgba[k], exp_img[k], f"heightfield-{fmt} camera batch view {k} against the oracle")


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def small(request, contexts):
    """The heightfield's case (a), its context, and the host call in both formats."""
    c = vc.small_views("heightfield", request.param)
    svo = contexts("heightfield", request.param)
    plain = {f: svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=f) for f in FORMATS}
    return c, svo, plain


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_device_memory_equals_host_memory(small, pixel_format):
    """3: torch tensors, read only after vx_sync."""
    c, svo, plain = small
    rgba, hits = svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format, device=True)
    svo.sync()
    assert rgba.cpu().numpy().tobytes() == plain[pixel_format][0].tobytes()
    assert hip.trace_hits_to_numpy(hits).tobytes() == plain[pixel_format][1].tobytes()


def test_rgba8_is_the_packing_with_the_top_row_first(small):
    c, svo, plain = small
    assert plain[hip.VX_FORMAT_RGBA8][0].dtype == np.uint8
    assert (plain[hip.VX_FORMAT_RGBA8][0] == tc.pack_rgba8(plain[hip.VX_FORMAT_RGBA32F][0][:, ::-1].reshape(-1, 4)).reshape(5, 13, 20, 4)).all()
    assert plain[hip.VX_FORMAT_RGBA8][1].reshape(5, 13, 20).tobytes() == plain[hip.VX_FORMAT_RGBA32F][1].reshape(5, 13, 20)[:, ::-1].tobytes()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_either_output_alone(small, pixel_format, device):
    """4: colours only, records only and both together agree."""
    c, svo, plain = small

    def raw(a, records):
        if a is None or not device:
            return a
        return hip.trace_hits_to_numpy(a) if records else a.cpu().numpy()

    only_rgba, none = svo.trace_views(c.views, c.width, c.height, fmt=pixel_format, device=device)
    svo.sync()
    assert none is None and raw(only_rgba, False).tobytes() == plain[pixel_format][0].tobytes()
    none, only_hits = svo.trace_views(c.views, c.width, c.height, want_hits=True, want_rgba=False, fmt=pixel_format, device=device)
    svo.sync()
    assert none is None and raw(only_hits, True).tobytes() == plain[pixel_format][1].tobytes()


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_the_tail_of_the_outputs(small, pixel_format):
    """5: outputs one view longer than needed, prefilled: the tail stays as it was -- in host memory and in device memory."""
    import torch

    c, svo, plain = small
    px = 4 if pixel_format == hip.VX_FORMAT_RGBA8 else 16
    n, more = 5 * 260, 6 * 260
    rgba, hits = np.full(more * px, 0x5a, dtype=np.uint8), np.full(more * 48, 0xa5, dtype=np.uint8)
    svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format, out=(rgba, hits))
    assert rgba[:n * px].tobytes() == plain[pixel_format][0].tobytes() and hits[:n * 48].tobytes() == plain[pixel_format][1].tobytes()
    assert (rgba[n * px:] == 0x5a).all() and (hits[n * 48:] == 0xa5).all()
    d_rgba = torch.full((more * px,), 0x5a, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((more * 48,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fills run on torch's stream, the views on the context's)
    svo.trace_views(c.views, c.width, c.height, want_hits=True, fmt=pixel_format, out=(d_rgba, d_hits))
    svo.sync()
    assert d_rgba.cpu().numpy().tobytes() == rgba.tobytes() and d_hits.cpu().numpy().tobytes() == hits.tobytes()


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 7)], ids=["1x1", "8x8", "9x7"])
def test_one_view(small, size, pixel_format):
    """6: count = 1 at one pixel, one whole tile, and two tiles of which the second holds one column: vx_render's records, its colours within 5e-6,
    and nothing behind them."""
    c, svo, _ = small
    w, h = size
    u = c.views[0]
    rgba, hits = np.full((w * h + 64) * 16, 0x5a, dtype=np.uint8), np.full((w * h + 64) * 48, 0xa5, dtype=np.uint8)
    svo.trace_views([u], w, h, want_hits=True, fmt=pixel_format, out=(rgba, hits))
    img, rhits = render_reference(svo, u, w, h, pixel_format)
    px = 4 if pixel_format == hip.VX_FORMAT_RGBA8 else 16
    assert hits[:w * h * 48].tobytes() == rhits.tobytes() and (hits[w * h * 48:] == 0xa5).all() and (rgba[w * h * px:] == 0x5a).all()
    got = rgba[:w * h * px].view(np.uint8 if pixel_format == hip.VX_FORMAT_RGBA8 else np.float32).reshape(h, w, 4)
    if img.dtype == np.uint8:
        assert np.abs(got.astype(np.int32) - img.astype(np.int32)).max() <= 1
    else:
        assert_pixels(pixel_format, got, img, f"one {w} x {h} view against vx_render")
    _, ohits = c.scene.render(tc.as_oracle(u), w, h)
    exp = ohits if pixel_format == hip.VX_FORMAT_RGBA32F else ohits[::-1]
    assert np.ascontiguousarray(exp).tobytes() == rhits.tobytes()


def test_two_device_calls_back_to_back(small):
    """7: two device-memory calls with different view arrays and no sync between them, the first array overwritten as soon as the first call has
    returned: each output is its own views' images (the table of views a launch reads outlives the call)."""
    c, svo, plain = small
    first, second = list(c.views), list(reversed(c.views))
    table = vc.uniforms_array(first)
    svo.sync()
    a_rgba, a_hits = svo.trace_views(table, c.width, c.height, want_hits=True, device=True)
    for k, u in enumerate(second):
        table[k] = u
    b_rgba, b_hits = svo.trace_views(table, c.width, c.height, want_hits=True, device=True)
    C.memset(table, 0xff, C.sizeof(table))
    svo.sync()
    exp_rgba, exp_hits = plain[hip.VX_FORMAT_RGBA32F]
    assert a_rgba.cpu().numpy().tobytes() == exp_rgba.tobytes() and hip.trace_hits_to_numpy(a_hits).tobytes() == exp_hits.tobytes()
    assert b_rgba.cpu().numpy().tobytes() == exp_rgba[::-1].tobytes() and hip.trace_hits_to_numpy(b_hits).tobytes() == exp_hits[::-1].tobytes()
    # more calls in a row than the library can keep tables for without waiting
    outs = []
    for i in range(6):
        for k in range(5):
            table[k] = c.views[(k + i) % 5]
        outs.append(svo.trace_views(table, c.width, c.height, want_hits=True, want_rgba=False, device=True)[1])
    svo.sync()
    for i, h in enumerate(outs):
        assert hip.trace_hits_to_numpy(h).tobytes() == np.roll(exp_hits, -i, axis=0).tobytes(), i


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_state_and_ordering(fmt):
    """8: before the first commit VX_ERR_STATE; count = 0 is VX_OK and writes nothing; a device-memory call, then an incremental commit that
    removes a chunk column (test_trace_rays.test_state's world change), then a second call, no sync in between: the first shows the old world
    and the second the new, by the oracle on each world."""
    svo_type = tc.SVO[fmt]
    L = hip.lib()
    world, scene_old, tex, mats, h_max = heightfield(svo_type, 7)
    svo = hip.Svo(svo_type, world.size_in_bytes + (1 << 20))
    try:
        svo.set_materials(mats)
        svo.set_textures(tex, 6)
        w, h = 12, 9
        u0 = tc.free_uniforms()
        table = (hip.Uniforms * 1)(u0)
        rgba, hits = np.full(w * h * 16, 0x5a, dtype=np.uint8), np.full(w * h * 48, 0xa5, dtype=np.uint8)

        def call(count=1):
            rc = L.vx_trace_views(svo._h, table, count, w, h, hip.VX_MEM_HOST, rgba.ctypes.data_as(_vp), hip.VX_FORMAT_RGBA32F, hits.ctypes.data_as(_vp))
            return rc, L.vx_last_error()

        rc, msg = call()
        assert rc == 6 and b"committed" in msg
        svo.update(world)
        assert call(count=0)[0] == 0
        assert L.vx_trace_views(svo._h, None, 0, w, h, hip.VX_MEM_DEVICE, None, hip.VX_FORMAT_RGBA8, None) == 0
        assert (rgba == 0x5a).all() and (hits == 0xa5).all()

        # a chunk column whose ground lies in the lowest chunk, seen from above and a little to the side
        def ground(x, z):
            r, _, _ = scene_old.intersect(np.float32([x, h_max + 4.0, z]), np.float32([0, -1, 0]), -1.0, False)
            return r.pos[1]

        cx, cz = next((x, z) for x in range(1, 3) for z in range(1, 3) if all(ground(32 * x + fx, 32 * z + fz) < 31.0 for fx in (4, 16, 28) for fz in (4, 16, 28)))
        eye = (32.0 * cx + 16.0, h_max + 12.0, 32.0 * cz + 16.0)
        view = scenes.view_matrix(eye, (0.05, -1.0, 0.02), (0.0, 0.0, 1.0))
        u = hip.make_uniforms(view, np.radians(50.0), w / h, 0.3, tc.unit([-1.0, -1.0, -1.0]), eye, True, 200.0)
        old = svo.trace_views([u], w, h, want_hits=True, device=True)
        chunk = vra.Chunk(cx, 0, cz, 5)
        chunk.set_block(0, 0, 0, 1)  # (not quite empty)
        chunk.compact()
        world.set_chunk((cx, 0, cz), chunk)
        world.serialize()
        svo.update(world)
        new = svo.trace_views([u], w, h, want_hits=True, device=True)
        svo.sync()
        scene_new = orc.OracleScene(svo_type, world.frame(), mats.view(orc.MATERIAL_DTYPE), tex, 6)
        results = []
        for scene, (got_rgba, got_hits) in ((scene_old, old), (scene_new, new)):
            img, ohits = scene.render(tc.as_oracle(u), w, h)
            got_hits = hip.trace_hits_to_numpy(got_hits)
            tc.assert_records(got_hits, ohits.reshape(-1), f"{fmt}: a view of the {'old' if scene is scene_old else 'new'} world")
            tc.assert_colors(got_rgba.cpu().numpy(), img, f"{fmt}: a view of the {'old' if scene is scene_old else 'new'} world")
            results.append(got_hits)
        assert (results[0]["t"] > 0).sum() >= 50 and (results[0]["t"] != results[1]["t"]).sum() >= 20  # the column is gone
    finally:
        svo.close()
