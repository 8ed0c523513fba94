"""The stand-alone host programs of the block entry points (tests/cpp/*_on_host.cpp), for the *_cases.py modules that run them: one build
recipe, the runner the Host* classes are made of, and the comparison of two calls' outputs. Both programs of a pair -- plain, and under
AddressSanitizer and UndefinedBehaviorSanitizer -- are built here and run directly, as child processes."""
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from helpers import ROOT

BUILD = Path(ROOT) / "tests" / "_build"
BLOCKS = Path(ROOT) / "voxel-rs_amd" / "csrc" / "blocks"
CPP = Path(ROOT) / "tests" / "cpp"


def headers():
    """Every header a program can include: a rebuild too many costs a second, a rebuild too few tests an old program."""
    return [*BLOCKS.glob("*.hpp"), *CPP.glob("*.hpp"), *(CPP / "shims").iterdir(), Path(ROOT) / "include" / "voxel_hip.h"]


def build_harness(name, sanitize=False, float_cast=False):
    """tests/_build/<name> from tests/cpp/<name>.cpp, or <name>_san: the same program under AddressSanitizer and UndefinedBehaviorSanitizer
    (float_cast: with the float-to-integer conversion check), every finding fatal. Built when it is older than its source or any of headers().
    The flags of `make move_harness` and `make block_scratch_harness` (voxel-rs_amd/Makefile)."""
    BUILD.mkdir(exist_ok=True)
    exe, source = BUILD / (name + "_san" if sanitize else name), CPP / (name + ".cpp")
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in [source, *headers()]):
        flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", *(["-fsanitize=float-cast-overflow"] if float_cast else []), "-fno-sanitize-recover=all"] if sanitize else []
        cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, f"-I{ROOT}/include", f"-I{CPP}/shims", f"-I{BLOCKS}", str(source), "-o", str(exe)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


class HostRunner:
    """A program on one world: the frame is written once, every call is a run of the program. A Host* class adds its call: the argument
    list and the shape of what comes back."""

    def __init__(self, exe, c):
        self.exe, self.c = exe, c
        self.dir = tempfile.TemporaryDirectory()
        self.world = self.path("world.bin")
        c.frame.tofile(self.world)

    def path(self, name, wanted=True):
        """A file of the runner's directory; not wanted: "-", which the programs take as a null input or output."""
        return Path(self.dir.name) / name if wanted else "-"

    def put(self, name, data):
        """`data`'s bytes as a file: its path."""
        np.ascontiguousarray(data).view(np.uint8).tofile(self.path(name))
        return self.path(name)

    def run(self, *args):
        """<exe> <svo_type> <world.bin> <args...>: its output; any other return code than 0 fails with that output."""
        r = subprocess.run([str(a) for a in (self.exe, self.c.svo_type, self.world, *args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        return r.stdout

    def get(self, name, dtype, wanted=True, shape=(-1,)):
        """What the program wrote to path(name), in `shape`, or None for an output that was not wanted."""
        return np.fromfile(self.path(name), dtype=dtype).reshape(shape) if wanted else None

    def close(self):
        self.dir.cleanup()


def _words(a, n):
    """[n, k]: a row for each of the first axis' entries; records as their dwords (equal bytes: -0.0 is not 0.0, the padding counts)."""
    a = np.ascontiguousarray(a)
    a = a.view(np.uint32) if a.dtype.names else a
    return a.reshape(n, a.size // n)


def outputs_differing(got, exp):
    """got, exp: two tuples of arrays with the same first axis -- a call's boxes, queries or records: fields, record arrays, paths. A message
    naming the first row in which any of them differ, and what differs there, or None."""
    if [a.shape for a in got] != [a.shape for a in exp]:
        return f"shapes differ: {', '.join(str(a.shape) for a in got)} vs {', '.join(str(a.shape) for a in exp)}"
    n = len(got[0])
    if n == 0:
        return None
    differ = [_words(g, n) != _words(e, n) for g, e in zip(got, exp)]
    bad = np.flatnonzero(np.any([d.any(axis=1) for d in differ], axis=0))
    if not len(bad):
        return None
    i = int(bad[0])
    said = []
    for g, e, d in zip(got, exp, differ):
        at = np.flatnonzero(d[i])
        if g.dtype.names and g.ndim == 1:
            said.append(f"record {g[i]} expected {e[i]}")
        elif g.dtype.names and len(at):
            k = int(at[0]) * 4 // g.dtype.itemsize
            said.append(f"{len(np.unique(at * 4 // g.dtype.itemsize))} records differ, first {k}: {g[i].reshape(-1)[k]} expected {e[i].reshape(-1)[k]}")
        elif len(at):
            k = int(at[0])
            said.append(f"{len(at)} entries differ, first at {k}: {int(g[i].reshape(-1)[k]):#x} expected {int(e[i].reshape(-1)[k]):#x}")
    return f"{len(bad)} of {n} differ, first {i}: " + "; ".join(said)
