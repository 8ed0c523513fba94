"""What the tests of the entry points' C ABI (tests/test_*_abi.py) share: the layout probe compiled from include/voxel_hip.h with gcc, the way
the C-ABI client is compiled; the readers of the Rust declarations (integration/rust/voxel_hip_sys.rs); and the refusal check of a call with a
null context. Each test keeps its own tables -- fields, constants, sizes -- and every one of its cases."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "voxel_hip.h"
#define S(T) printf(#T " %zu\n", sizeof(T))
#define F(T, M) printf(#T "." #M " %zu %zu\n", offsetof(T, M), sizeof(((T*)0)->M))
#define K(N) printf(#N " %lld\n", (long long)(N))
int main(void) {
BODY
    return 0;
}
AFTER
"""


def probe(tmp_path, structs=(), constants=(), more="", after="", std="c11"):
    """What the C compiler says of the header: {"T": (sizeof,), "T.member": (offset, size), "CONSTANT": (value,)} for structs -- {T: its
    members}, or T alone for its size only -- and constants; `more`: further statements of the program, each printing a line of a name and
    integers, which come back the same way; `after`: declarations behind main, such as a static assertion, which the
    compiler checks (std: the dialect they need)."""
    structs = structs if isinstance(structs, dict) else {s: () for s in structs}
    lines = [f"S({s});" for s in structs] + [f"F({s}, {m});" for s, members in structs.items() for m in members] + [f"K({k});" for k in constants]
    (tmp_path / "probe.c").write_text(PROBE.replace("BODY", "\n".join("    " + ln for ln in lines) + "\n" + more).replace("AFTER", after))
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", f"-std={std}", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/include", str(tmp_path / "probe.c"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.splitlines()}


class Rust:
    """The Rust declarations, read with regular expressions: what tests/test_rust_shim.py's parser cannot see of a call."""

    def __init__(self):
        self.text = (ROOT / "integration" / "rust" / "voxel_hip_sys.rs").read_text()

    def struct(self, name):
        """[(field, type)] of `pub struct name`, in order."""
        body = re.search(rf"pub struct {name}\s*\{{(.*?)\}}", self.text, flags=re.S).group(1)
        return [(f, t.strip()) for f, t in re.findall(r"pub\s+(?:r#)?(\w+)\s*:\s*([^,\n/]+)", body)]

    def const(self, name):
        """(type, value as written) of `pub const name`, or None."""
        m = re.search(rf"pub const {name}\s*:\s*(\w+)\s*=\s*([^;]+?)\s*;", self.text)
        return m and (m.group(1), m.group(2))

    def const_int(self, name):
        """(type, value) of an integer constant (u32::MAX: 0xFFFFFFFF)."""
        found = self.const(name)
        assert found, name
        return found[0], 0xFFFFFFFF if found[1] == "u32::MAX" else int(found[1].replace("_", ""), 0)

    def args(self, fn):
        """The argument names of `pub fn fn(...) -> c_int;`."""
        decl = re.search(rf"pub fn {fn}\((.*?)\)\s*->\s*c_int;", self.text, flags=re.S).group(1)
        return [a.split(":")[0].strip() for a in decl.split(",")]

    def asserts_size(self, name, size):
        return f"size_of::<{name}>() == {size}" in self.text


def refusing(L, call, outputs):
    """refused(word, ...): call(...) must return 1 with `word` in vx_last_error(), and leave the sentinel-filled `outputs` (numpy arrays) as they
    were when this was made."""
    sentinel = b"".join(o.tobytes() for o in outputs)

    def refused(word, *args, **kwargs):
        rc = call(*args, **kwargs)
        assert rc == 1 and word in L.vx_last_error(), (word, rc, L.vx_last_error())
        assert b"".join(o.tobytes() for o in outputs) == sentinel

    return refused
