"""Shared by the tests of vx_trace_views (test_trace_views_on_host.py, test_trace_views.py): (a) five 20 x 13 views of each of the three worlds of
trace_cases.build_world -- 3 x 2 tiles of 8 x 8 pixels whose last column holds 4 live columns and whose top row 5 live rows -- with five eyes and
forward vectors around trace_cases.VIEWS, three values of fovy, one aspect that is not W / H, and one view each with shadows on, shadows off,
another light, a highlighted block and a projective view matrix; (b) the three 64 x 48 views of trace_cases.camera_case("heightfield") as one
batch. Expected images and records are OracleScene.render's, view by view. Everything is seeded and computed once per (world, format); nothing
of the code under test is used."""
import ctypes as C
import functools

import numpy as np

import trace_cases as tc
from helpers import orc, vra  # noqa: F401
from voxel_rs_amd import hip, scenes

W, H = 20, 13
N_VIEWS = 5
# per view: the eye's offset from trace_cases.VIEWS[name]["eye"], what is added to its forward vector, fovy in degrees, aspect
CAMERAS = [
    dict(eye=(0.0, 0.0, 0.0), fwd=(0.0, 0.0, 0.0), fovy=72.0, aspect=W / H),
    dict(eye=(0.4, 0.3, -0.3), fwd=(0.12, 0.05, -0.08), fovy=60.0, aspect=W / H),
    dict(eye=(-0.35, 0.5, 0.2), fwd=(-0.15, 0.1, 0.05), fovy=85.0, aspect=1.0),  # (the aspect that is not W / H)
    dict(eye=(0.2, -0.2, 0.35), fwd=(0.05, -0.1, 0.1), fovy=72.0, aspect=W / H),
    dict(eye=(-0.2, 0.15, -0.4), fwd=(-0.06, -0.04, -0.12), fovy=60.0, aspect=W / H),
]
OTHER_LIGHT, OTHER_AMBIENT = (0.5, -1.0, -0.3), 0.45
# view 4's matrix: the look-at matrix with this last row instead of (0, 0, 0, 1), so that w depends on the pixel and primary_ray divides
PROJECTIVE_ROW = (0.125, -0.0625, 0.03125, 1.25)


class Case:
    pass


def uniforms_array(views):
    return (hip.Uniforms * len(views))(*views)


def is_outline(rec):
    """world.glsl:36-41 on a record's uv: the pixel is on the outline of its block, were that block the highlighted one."""
    return rec["t"] > 0 and max(abs(float(rec["uv"][0]) - 0.5), abs(float(rec["uv"][1]) - 0.5)) * 2.0 > 1.0 - 1.0 / 16.0


def build_views(name, anchor, scene):
    v = tc.VIEWS[name]
    sun = scenes._normalize((-1.0, -1.0, -1.0))
    out = []
    for k, cam in enumerate(CAMERAS):
        eye = np.float64(v["eye"]) + anchor + np.float64(cam["eye"])
        view = scenes.view_matrix(eye, tuple(np.float64(v["fwd"]) + np.float64(cam["fwd"])), (0.0, 1.0, 0.0))
        shadows, light, ambient, highlight = True, sun, 0.3, None
        if k == 1:
            shadows = False
        if k == 2:
            light, ambient = scenes._normalize(OTHER_LIGHT), OTHER_AMBIENT
        if k == 4:
            view[3], view[7], view[11], view[15] = PROJECTIVE_ROW
        u = hip.make_uniforms(view, np.radians(cam["fovy"]), cam["aspect"], ambient, light, eye, shadows, v["shadow_distance"], highlight)
        if k == 3:
            # the highlighted block: the one the oracle sees at the view's pick pixel -- the first pixel, bottom row first, that lies on the rim of its block's face
            _, plain = scene.render(tc.as_oracle(u), W, H)
            pick = next(i for i, rec in enumerate(plain.ravel()) if is_outline(rec))
            highlight = tuple(float(np.floor(p)) + 0.5 for p in plain.ravel()[pick]["pos"])
            u = hip.make_uniforms(view, np.radians(cam["fovy"]), cam["aspect"], ambient, light, eye, shadows, v["shadow_distance"], highlight)
        out.append(u)
    return out


def kind_counts(hits):
    f = hits["flags"].ravel()
    return dict(sky=int(((f & 1) == 0).sum()), hit=int(((f & 1) != 0).sum()), lit=int((((f & 2) != 0) & ((f & 4) == 0)).sum()),
                shadow=int(((f & 4) != 0).sum()), outline=int(((f & 8) != 0).sum()))


@functools.lru_cache(maxsize=None)
def small_views(name, fmt):
    """Case (a) of one world in one format: `views` (5 uniforms), `imgs` [5, H, W, 4] and `hits` [5, H, W] with row 0 at the bottom (the oracle's
    order, which is RGBA32F's), `counts` per view. The world is trace_cases.camera_case's."""
    w = tc.camera_case(name, fmt)
    c = Case()
    c.name, c.fmt, c.svo_type, c.world, c.scene, c.tex, c.mats = name, fmt, w.svo_type, w.world, w.scene, w.tex, w.mats
    c.width, c.height = W, H
    c.views = build_views(name, w.anchor, w.scene)
    rendered = [c.scene.render(tc.as_oracle(u), W, H) for u in c.views]
    c.imgs, c.hits = np.stack([r[0] for r in rendered]), np.stack([r[1] for r in rendered])
    c.counts = [kind_counts(h) for h in c.hits]
    for a in (c.imgs, c.hits):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def camera_batch(fmt):
    """Case (b): the heightfield's 64 x 48 views -- highlighted, cam_pos moved, plain -- as a batch of three."""
    w = tc.camera_case("heightfield", fmt)
    c = Case()
    c.name, c.fmt, c.svo_type, c.world, c.scene, c.tex, c.mats = "heightfield", fmt, w.svo_type, w.world, w.scene, w.tex, w.mats
    c.width, c.height = tc.W, tc.H
    plain = tc.view_of("heightfield", w.anchor)
    img_plain, hits_plain = c.scene.render(tc.as_oracle(plain), tc.W, tc.H)
    c.views = [w.u, w.u_moved, plain]
    c.imgs, c.hits = np.stack([w.img, w.img_moved, img_plain]), np.stack([w.hits, w.hits_moved, hits_plain])
    c.counts = [kind_counts(h) for h in c.hits]
    for a in (c.imgs, c.hits):
        a.setflags(write=False)
    return c


def expected(c, pixel_format):
    """(images [N, H, W, 4] float, records [N, H * W]) in the row order of the format: RGBA8 has the top row first, for both."""
    imgs, hits = (c.imgs, c.hits) if pixel_format == hip.VX_FORMAT_RGBA32F else (c.imgs[:, ::-1], c.hits[:, ::-1])
    return np.ascontiguousarray(imgs), np.ascontiguousarray(hits).reshape(len(c.views), -1)

