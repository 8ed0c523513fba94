"""tests/gpu_harness.py without a GPU: the two checks of a sentinel-filled buffer, on CPU tensors at the smallest shapes that reach every
branch -- two fields of 40 bytes at a stride of 48 and the tail of 48; two records of four words and two more --, and the entities of
test_behind_physics_step against the lines the four modules had, which are kept here."""
import types

import numpy as np
import pytest

from gpu_harness import SENTINEL, TAIL, above_the_blocks, field_rows, flying_entities, records_head, sentinel_bytes, sentinel_words
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

COUNT, STRIDE, WRITTEN, WIDTH = 2, 48, 40, 4


def written_fields():
    """(the buffer after a call that wrote what it should, what it wrote)."""
    exp = np.arange(COUNT * WRITTEN, dtype=np.uint8).reshape(COUNT, WRITTEN)
    fields = sentinel_bytes(COUNT, STRIDE, device="cpu")
    fields[:COUNT * STRIDE].view(COUNT, STRIDE)[:, :WRITTEN] = torch_of(exp)
    return fields, exp


def torch_of(array):
    import torch

    return torch.from_numpy(array)


def test_the_buffers_are_sentinels_all_through():
    fields, words = sentinel_bytes(COUNT, STRIDE, device="cpu"), sentinel_words(COUNT, WIDTH, device="cpu")
    assert tuple(fields.shape) == (COUNT * STRIDE + TAIL,) and (fields.numpy() == 0x5A).all() and TAIL == 48
    assert tuple(words.shape) == (COUNT + 2, WIDTH) and (words.numpy().view(np.uint32) == SENTINEL).all() and SENTINEL == 0x5A5A5A5A


def test_field_rows_accepts_what_a_call_should_leave():
    fields, exp = written_fields()
    head = field_rows(fields, COUNT, STRIDE, WRITTEN, "written")
    assert head.shape == (COUNT, WRITTEN) and head.tobytes() == exp.tobytes()
    assert field_rows(sentinel_bytes(0, STRIDE, device="cpu"), 0, STRIDE, WRITTEN, "count 0").shape == (0, WRITTEN)
    assert field_rows(sentinel_bytes(COUNT, STRIDE, device="cpu"), 0, STRIDE, WRITTEN, "count 0 of a longer buffer").shape == (0, WRITTEN)


@pytest.mark.parametrize("at", [WRITTEN, STRIDE - 1, STRIDE + WRITTEN, COUNT * STRIDE - 1, COUNT * STRIDE, COUNT * STRIDE + TAIL - 1],
                         ids=["row0-first", "row0-last", "last-row-first", "last-row-last", "tail-first", "tail-last"])
def test_field_rows_refuses_a_byte_outside_the_written_part(at):
    """One byte changed in the padding of row 0, in the padding of the last row and in the tail, at either end of each."""
    fields, _ = written_fields()
    fields[at] = 0x5B
    with pytest.raises(AssertionError, match="changed"):
        field_rows(fields, COUNT, STRIDE, WRITTEN, "changed")


def test_field_rows_hands_a_changed_written_byte_to_the_caller():
    fields, exp = written_fields()
    fields[STRIDE + 3] ^= 0xFF
    head = field_rows(fields, COUNT, STRIDE, WRITTEN, "written")
    assert np.argwhere(head != exp).tolist() == [[1, 3]]


def test_records_head_accepts_what_a_call_should_leave():
    words = sentinel_words(COUNT, WIDTH, device="cpu")
    exp = np.arange(COUNT * WIDTH, dtype=np.int32).reshape(COUNT, WIDTH)
    words[:COUNT] = torch_of(exp)
    assert records_head(words, COUNT, "tensor").tobytes() == exp.tobytes()
    structured = words.numpy().view(np.dtype([("a", "<u4"), ("b", "<u4", (3,))])).reshape(-1)  # (as a *_to_numpy of hip gives them)
    head = records_head(structured, COUNT, "records")
    assert len(head) == COUNT and head.tobytes() == exp.tobytes()
    assert len(records_head(sentinel_words(0, WIDTH, device="cpu"), 0, "count 0")) == 0
    assert len(records_head(sentinel_words(COUNT, WIDTH, device="cpu"), 0, "count 0 of a longer buffer")) == 0


@pytest.mark.parametrize("row, word", [(COUNT, 0), (COUNT, WIDTH - 1), (COUNT + 1, WIDTH - 1)], ids=["first-word", "first-record-last-word", "last-word"])
def test_records_head_refuses_a_word_behind_the_count(row, word):
    words = sentinel_words(COUNT, WIDTH, device="cpu")
    words[:COUNT] = 7
    words[row, word] = SENTINEL ^ 0x100
    with pytest.raises(AssertionError, match="changed"):
        records_head(words, COUNT, "changed")
    with pytest.raises(AssertionError, match="changed"):
        records_head(words.numpy().view(np.dtype([("a", "<u4"), ("b", "<u4", (3,))])).reshape(-1), COUNT, "changed")


def test_records_head_hands_a_changed_record_to_the_caller():
    words = sentinel_words(COUNT, WIDTH, device="cpu")
    words[:COUNT] = 7
    words[1, 2] = 8
    assert np.argwhere(records_head(words, COUNT, "written") != 7).tolist() == [[1, 2]]


def a_floor():
    """A stand-in for a case of tests/boxes_cases.py: blocks [x][y][z] with a floor, a few columns on it and some without any block."""
    rng = np.random.default_rng(5)
    truth = np.zeros((32, 32, 32), dtype=np.uint32)
    truth[:, 0, :] = 3
    truth[rng.integers(0, 32, 40), rng.integers(1, 20, 40), rng.integers(0, 32, 40)] = 7
    truth[4:9, :, 11:13] = 0
    return truth, np.array([-3, 0, 5], dtype=np.int32)


def above_the_floor_as_it_was(seed, low, high):
    """tests/test_boxes.py (seed 71, 0.2 to 0.9 above the highest block) and tests/test_move.py (seed 91, 1.3 to 1.5), as they built them."""
    t, lo = a_floor()
    rng = np.random.default_rng(seed)
    top = np.where((t != 0).any(axis=1), t.shape[1] - 1 - (t[:, ::-1, :] != 0).argmax(axis=1), -1)  # [x][z]: the highest block
    held = np.argwhere(top >= 0)
    e = np.zeros(256, dtype=hip.ENTITY_DTYPE)
    for k in range(len(e)):
        x, z = (int(v) for v in held[rng.integers(len(held))])
        e["position"][k] = lo + (x + 0.5, top[x, z] + 1 + rng.uniform(low, high), z + 0.5)
    e["velocity"] = np.stack([rng.uniform(-30, 30, len(e)), np.full(len(e), -40.0), rng.uniform(-30, 30, len(e))], axis=1)
    e["aabb_offset"], e["aabb_extents"] = (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8)
    e["gravity"], e["max_fall_velocity"], e["flags"] = 20.0, 50.0, hip.ENTITY_FLYING
    return e


def in_the_air_as_it_was(seed, ceiling):
    """tests/test_flood.py (seed 91, up to y = 14) and tests/test_walk.py (seed 191, up to y = 6), as they built them."""
    rng = np.random.default_rng(seed)
    e = np.zeros(256, dtype=hip.ENTITY_DTYPE)
    e["position"] = rng.uniform((2.0, 2.0, 2.0), (30.0, ceiling, 30.0), (256, 3))
    e["velocity"] = np.stack([rng.uniform(-30, 30, len(e)), np.full(len(e), -40.0), rng.uniform(-30, 30, len(e))], axis=1)
    e["aabb_offset"], e["aabb_extents"] = (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8)
    e["gravity"], e["max_fall_velocity"], e["flags"] = 20.0, 50.0, hip.ENTITY_FLYING
    return e


@pytest.mark.parametrize("seed, low, high", [(71, 0.2, 0.9), (91, 1.3, 1.5)], ids=["boxes", "move"])
def test_flying_entities_above_the_floor_are_the_bytes_they_were(seed, low, high):
    truth, lo = a_floor()
    rng = np.random.default_rng(seed)
    e = flying_entities(256, above_the_blocks(types.SimpleNamespace(truth=truth, info={"lo": lo}), 256, rng, low, high), rng)
    assert e.tobytes() == above_the_floor_as_it_was(seed, low, high).tobytes() and (e["position"][:, 1] >= 1.0).all()


@pytest.mark.parametrize("seed, ceiling", [(91, 14.0), (191, 6.0)], ids=["flood", "walk"])
def test_flying_entities_in_the_air_are_the_bytes_they_were(seed, ceiling):
    rng = np.random.default_rng(seed)
    e = flying_entities(256, rng.uniform((2.0, 2.0, 2.0), (30.0, ceiling, 30.0), (256, 3)), rng)
    assert e.tobytes() == in_the_air_as_it_was(seed, ceiling).tobytes()
