"""What a block entry point's host-memory call keeps in pinned scratch, without a GPU: voxel-rs_amd/csrc/blocks/vx_block_scratch.hpp compiled
by the stand-alone program tests/cpp/block_scratch_on_host.cpp -- the strided 12-byte pack, the batch of boxes packed whole, the eight
layouts against offsets worked out by hand, and the fields spread to a caller's stride, every buffer a heap block of exactly the bytes the
ABI allows -- plain and under AddressSanitizer and UndefinedBehaviorSanitizer with every finding fatal. Both programs are run directly, as
child processes."""
import subprocess

import pytest

from host_harness import build_harness

SECTIONS = ("packing", "boxes", "layouts", "a call", "spreading")


def harness(sanitize=False):
    """tests/_build/block_scratch_on_host, or block_scratch_on_host_san: host_harness.build_harness's."""
    return build_harness("block_scratch_on_host", sanitize)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_the_program_passes(sanitize):
    """Every section reports its checks; a failed check or a sanitizer finding ends the program with a non-zero status."""
    r = subprocess.run([str(harness(sanitize))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    said = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert tuple(said) == SECTIONS, r.stdout
    for name in SECTIONS:
        word, checks = said[name].split(", ")
        assert word == "ok" and int(checks.split()[0]) > 0, (name, said[name])
