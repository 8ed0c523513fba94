"""vx_light_boxes' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_light.hpp compiled for the host by the stand-alone harness
tests/cpp/light_on_host.cpp -- box by box, the bricks, columns, rows and steps the kernel's workgroup walks -- against the numpy fields and
records of tests/light_cases.py, which come from the per-cell rule over the dense arrays the worlds were built from: five worlds, both formats,
every shape, stride, table of props and flag, byte for byte and record for record; the named boxes for what each was made to catch; and the
same program built with AddressSanitizer and UndefinedBehaviorSanitizer. test_light.py holds the GPU's bytes against the harness's."""
import subprocess

import numpy as np
import pytest

from blocks_cases import dense_region
from light_cases import (LIGHT_CASES, NO_BLOCKS, NO_SKY, SEALED, SEEDED, SHAPE, SHAPES, SIXTEEN, HostLight, calls_for, cells, differing, harness,
                         light_truth, make_light_case, tables, truth_for)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=LIGHT_CASES, ids=[f"{n}-{f}" for n, f in LIGHT_CASES])
def case(request, exe):
    c = make_light_case(*request.param)
    c.host = HostLight(exe, c)
    yield c
    c.host.close()


def the_call(c, name):
    return [call for call in calls_for(c) if call[0] == name][0]


def test_the_boxes_hold_what_the_tests_need(case):
    """By the dense arrays alone, among the seeded boxes at 16^3. A set that misses a condition gets another seed; the condition is never
    loosened. (`burrow` is rock with one sealed emitter and nothing transparent: `lantern` carries what it cannot show.)"""
    fields, info = truth_for(case, the_call(case, "16"))
    sky, block = cells(fields[:SEEDED], SIXTEEN)
    partly = int(((info["open_columns"][:SEEDED] > 0) & (info["open_columns"][:SEEDED] < 256)).sum())
    boxes = np.asarray(case.boxes[:SEEDED], dtype=np.int64)
    _, emits = tables(case.props)
    spread = 0
    for k, lo in enumerate(boxes):
        values = dense_region(case.info, case.truth, lo, SIXTEEN.size)
        spread += bool(((block[k] >= 1) & (emits[np.where(values < len(emits), values, 0)] == 0)).any())
    both = int(((sky > 0) & (block > 0)).any(axis=(1, 2, 3)).sum())
    print(f"\n{case.name}-{case.fmt}: {partly} boxes with a partly open top, {spread} with block light beside its sources, {both} with both channels in a cell")
    kinds = {int(p) for p in case.props[1:]}
    if case.name == "burrow":  # (light_cases.py's docstring: two ids, the emitter sealed in rock)
        assert 15 in kinds and partly >= 20 and spread >= 20 and both == 0
        return
    assert any(p in (14, 15) for p in kinds) and any(3 <= p <= 6 for p in kinds) and hip.VX_LIGHT_TRANSPARENT in kinds
    assert any(p & hip.VX_LIGHT_TRANSPARENT and p & 15 for p in kinds) and 0 in kinds
    assert partly >= 20 and spread >= 20 and both >= 10


def test_every_call_against_the_dense_array(case):
    """Every shape under the world's props, no props, a table cut short, each flag; the strides in turn."""
    for call in calls_for(case):
        name, shape, props, flags, stride = call
        exp_fields, exp_info = truth_for(case, call)
        got_fields, got_info = case.host.call(case, call)
        assert differing(got_fields, got_info, exp_fields, exp_info) is None, f"{name} (stride {stride}): {differing(got_fields, got_info, exp_fields, exp_info)}"
        assert (exp_fields[:, shape.voxels:] == 0).all()
        sky, block = cells(exp_fields, shape)
        if flags & NO_SKY:
            assert (sky == 0).all() and (exp_info["open_columns"] == 0).all()
        if flags & NO_BLOCKS or len(props) == 0:
            assert (block == 0).all() and (exp_info["sources"] == 0).all()
    # the table cut short differs from the whole one exactly when the highest id does something
    whole, cut = truth_for(case, the_call(case, "16_off"))[0], truth_for(case, the_call(case, "16_off-cut"))[0]
    assert case.props[-1] != 0 or (whole == cut).all()
    assert (truth_for(case, the_call(case, "16_off-no_sky"))[0] == (whole & 0x0F)).all()
    assert (truth_for(case, the_call(case, "16_off-no_blocks"))[0] == (whole & 0xF0)).all()


def test_the_named_boxes(case):
    """What each named box was made to catch, by the truth (which the harness equals, above)."""
    names = case.names
    fields, info = truth_for(case, the_call(case, "16"))
    sky, block = cells(fields, SIXTEEN)
    at = lambda name: info[names[name]]
    for name in ("above_world", "outside_x", "far"):
        assert (fields[names[name], :4096] == 0xF0).all() and tuple(at(name)) == (4096, 0, 256, 63), name
    # the top layer of the world: whatever is open there is open with no cell above it
    k = names["top_layer"]
    assert at("top_layer")["open_columns"] == (sky[k][:, 15, :] == 15).sum()
    # below y = 0 is air: the cells under the world are lit from the sides only, the bottom face is reached
    k = names["below_zero"]
    assert (sky[k][:, :5, :] < 15).any() or at("below_zero")["open_columns"] == 256
    assert at("negative_lo")["lit"] > 0
    if case.name == "burrow":
        assert (fields[names["in_rock"]] == 0).all() and tuple(at("in_rock")) == (0, 0, 0, 0)
    if case.name in ("tower", "far_chunks"):
        assert at("lod")["lit"] > 0 and (fields[names["lod"], :4096] == 0).any()
    if case.name != "lantern":
        return
    cell = lambda name, x, y, z: (int(sky[names[name]][z, y, x]), int(block[names[name]][z, y, x]))  # (box-relative)
    # the shaft under the roof's hole: 15 all the way down, 14 beside it, one open column
    assert at("roof_hole")["open_columns"] == 1
    assert all(cell("roof_hole", 6, y, 6)[0] == 15 for y in range(16)) and cell("roof_hole", 7, 8, 6)[0] == 14 and cell("roof_hole", 6, 8, 9)[0] == 12
    # under the panes the sky comes through; the panes themselves are passable and exposed
    assert cell("glass_roof", 6, 13, 6)[0] == 15 and cell("glass_roof", 6, 14, 6)[0] == 15 and cell("glass_roof", 2, 13, 2)[0] < 15
    # the lamp (15) at (6, 1, 6) of the box and the lava (12) at (10, 1, 6): the larger of the two wins in every cell
    assert cell("two_emitters", 6, 1, 6)[1] == 15 and cell("two_emitters", 10, 1, 6)[1] == 12
    assert cell("two_emitters", 8, 1, 6)[1] == 13 and cell("two_emitters", 11, 1, 6)[1] == 11 and cell("two_emitters", 9, 1, 6)[1] == 12
    assert cell("two_emitters", 8, 3, 10)[1] == 4  # the ember: an opaque block has just its emission
    # the wall at x = 13 (7 of the box): bright in front of it, dark right behind it
    assert cell("wall", 6, 1, 6)[1] == 13 and cell("wall", 7, 1, 6)[1] == 0 and cell("wall", 8, 1, 6)[1] == 0
    # the lamp sealed in rock: its own byte alone
    f, i = light_truth(case, np.array([SEALED[0]]), SEALED[1], case.props)
    assert tuple(i[0]) == (1, 1, 0, 0) and f[0, (2 * 5 + 2) * 5 + 2] == 15 and (f[0] != 0).sum() == 1
    got = case.host.light(np.array([SEALED[0]], dtype=np.int32), SEALED[1], case.props)
    assert differing(*got, f, i) is None


def test_outputs_and_strides(case):
    """Fields only, records only, a stride larger than the box (the bytes beyond the rounded voxel count keep their sentinel), one box, none."""
    call = the_call(case, "33x9x17")
    _, shape, props, flags, stride = call
    exp_fields, exp_info = truth_for(case, call)
    boxes = case.boxes
    f, i = case.host.light(boxes, shape.size, props, lo_stride=stride, fields=True, info=False)
    assert i is None and (f == exp_fields).all()
    f, i = case.host.light(boxes, shape.size, props, lo_stride=stride, fields=False, info=True)
    assert f is None and i.tobytes() == exp_info.tobytes()
    f, i = case.host.light(boxes, shape.size, props, lo_stride=stride, field_stride=shape.padded + 32)
    assert (f[:, :shape.padded] == exp_fields).all() and (f[:, shape.padded:] == 0x5a).all() and i.tobytes() == exp_info.tobytes()
    f, i = case.host.light(boxes[7:8], shape.size, props)
    assert (f == exp_fields[7:8]).all() and i.tobytes() == exp_info[7:8].tobytes()
    f, i = case.host.light(boxes[:0], shape.size, props)
    assert f.size == 0 and i.size == 0


@pytest.mark.parametrize("name", ["lantern", "tower"])
def test_the_sanitized_program(exe, name):
    """The same program under -fsanitize=address,undefined -fno-sanitize-recover=all, run directly: every call of `lantern` and `tower`, both
    formats, on the first 20 seeded boxes and every named one -- negative, overhanging and wrapping coordinates among them. A finding ends
    the program with a non-zero status; its bytes are the plain program's."""
    san = harness(sanitize=True)
    for fmt in ("esvo", "csvo"):
        c = make_light_case(name, fmt)
        plain, checked = HostLight(exe, c), HostLight(san, c)
        pick = np.concatenate([np.arange(20), np.arange(SEEDED, len(c.boxes))])
        try:
            for call in calls_for(c):
                (pf, pi), (cf, ci) = plain.call(c, call, pick), checked.call(c, call, pick)
                assert pf.tobytes() == cf.tobytes() and pi.tobytes() == ci.tobytes(), (fmt, call[0])
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_light.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "stride 64", "fields only", "info only", "info only, any stride", "count 0", "largest box", "smallest box", "flags 1", "flags 2",
               "props_count 4096", "no props", "field_stride 4096", "field_stride 4112", "field_stride 8192", "field bytes 2^24", "151 boxes of 46^3", "172 boxes of 46^3",
               "props byte 32 behind props_count", "props byte 128 behind props_count"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["too many"].startswith("count exceeds 16777216")
    assert said["null shape"] == "null shape" and said["null lo"] == "null lo" and said["no output"] == "fields and info are both null"
    for stride in (0, 4, 8, 13, 14):
        assert said[f"lo_stride {stride}"].startswith("lo_stride"), stride
    for off in (1, 2, 3):
        assert said[f"lo + {off}"].startswith("lo must be aligned"), off
    for a in range(3):
        for side in (0, 49, 0xFFFFFFFF):
            assert said[f"size[{a}] {side}"].startswith("size"), (a, side)
    for flags in (3, 4, 0x80000000):
        assert said[f"flags {flags}"].startswith("flags"), flags
    assert said["props_count 4097"].startswith("props_count") and said["null props"].startswith("null props")
    for bad in (32, 64, 128):
        assert said[f"props byte {bad}"].startswith("props: a byte"), bad
    for stride in (4097, 4104, 4080, 16):
        assert said[f"field_stride {stride}"].startswith("field_stride"), stride
    assert said["field bytes 2^24 + 8192"].startswith("count * field_stride") and said["173 boxes of 46^3"].startswith("count * field_stride")
    assert hip.LIGHT_INFO_DTYPE.itemsize == 16 and len(SHAPES) == 7 and SHAPE["48"].voxels == 110592
