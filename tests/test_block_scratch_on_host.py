"""What a block entry point's host-memory call keeps in pinned scratch, without a GPU: voxel-rs_amd/csrc/blocks/vx_block_scratch.hpp compiled
by the stand-alone program tests/cpp/block_scratch_on_host.cpp -- the strided 12-byte pack, the batch of boxes packed whole, the eight
layouts against offsets worked out by hand, and the fields spread to a caller's stride, every buffer a heap block of exactly the bytes the
ABI allows -- plain and under AddressSanitizer and UndefinedBehaviorSanitizer with every finding fatal. Both programs are run directly, as
child processes."""
import subprocess
from pathlib import Path

import pytest

from helpers import ROOT

BUILD = Path(ROOT) / "tests" / "_build"
SECTIONS = ("packing", "boxes", "layouts", "a call", "spreading")


def harness(sanitize=False):
    """tests/_build/block_scratch_on_host (or block_scratch_on_host_san), built when it is older than its sources: the flags of
    `make block_scratch_harness` (voxel-rs_amd/Makefile)."""
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / ("block_scratch_on_host_san" if sanitize else "block_scratch_on_host")
    blocks = Path(ROOT) / "voxel-rs_amd" / "csrc" / "blocks"
    deps = [Path(ROOT) / "tests" / "cpp" / "block_scratch_on_host.cpp", blocks / "vx_block_scratch.hpp", Path(ROOT) / "include" / "voxel_hip.h"]
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, f"-I{ROOT}/include", f"-I{blocks}", str(deps[0]), "-o", str(exe)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


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
