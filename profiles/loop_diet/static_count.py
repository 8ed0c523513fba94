#!/usr/bin/env python3
"""Static figures of kernels_render.hip's device assembly: per render_persistent build the code object's register and spill
figures, and per hand-scheduled traversal loop in it (vx_loop_gfx950.hpp) the instructions of one trip, tail by tail.

    hipcc <HIPFLAGS of voxel-rs_amd/Makefile> -Iinclude -Ivoxel-rs_amd/csrc/hip --cuda-device-only -S -o render.s \
        voxel-rs_amd/csrc/hip/kernels_render.hip
    python3 profiles/loop_diet/static_count.py render.s [--json]

A trip's common part runs from the trip's head to the branches that pick a tail; the merged tail is what follows them, the
ADVANCE-only tail starts at label 4, the PUSH-only tail at label 5. The POP block (between `s_cbranch_execz` and its target) is
counted apart: a trip runs it only where a lane leaves its parent. A loop with two copies of the trip gives two rows.
"""
import json
import re
import sys


def kind(ins):
    op = ins.split()[0]
    if op.startswith(("buffer_", "global_", "ds_", "flat_", "scratch_")):
        return "memory"
    if op.startswith("v_"):
        return "vector"
    return "scalar"


def count(lines):
    c = {"vector": 0, "scalar": 0, "memory": 0}
    for ins in lines:
        c[kind(ins)] += 1
    c["all"] = sum(c.values())
    return c


def split_pop(lines):
    """-> (lines outside the POP block, lines of the POP block)"""
    out, pop, inside, target = [], [], False, None
    for ins in lines:
        if inside and re.fullmatch(target + ":", ins):
            inside = False
            continue
        if re.fullmatch(r"\d+:", ins):
            continue
        (pop if inside else out).append(ins)
        m = re.match(r"s_cbranch_execz (\d+)f", ins)
        if m:
            inside, target = True, m.group(1)
    return out, pop


def trips_of(block):
    """the copies of the trip in one loop block: a copy starts behind `s_mov_b64 s[..], vcc` at a head and ends with the PUSH-only tail's back branch"""
    ins = [l.strip() for l in block if l.strip() and not l.strip().startswith(";")]
    heads = [i for i, l in enumerate(ins) if re.fullmatch(r"[13]:", l)]
    copies = []
    for h in heads:
        body = ins[h + 1:]
        i4 = next(i for i, l in enumerate(body) if l == "4:")
        i5 = next(i for i, l in enumerate(body) if l == "5:")
        end = next(i for i in range(i5, len(body)) if re.match(r"s_cbranch_(scc1|vccnz) (1b|3f)", body[i])) + 1
        pick = next(i for i, l in enumerate(body) if re.match(r"s_cbranch_scc1 5f", l)) + 1
        common = [l for l in body[:pick] if not re.fullmatch(r"\d+:", l)]
        merged = body[pick:i4]
        # the merged and ADVANCE-only tails end with the branch behind the loop, which a trip that goes on does not reach
        merged = merged[:-1] if merged[-1].startswith("s_branch") else merged
        adv = body[i4 + 1:i5]
        adv = adv[:-1] if adv[-1].startswith("s_branch") else adv
        push = body[i5 + 1:end]
        row = {"common": count(common)}
        for name, part in (("merged", merged), ("advance_only", adv), ("push_only", push)):
            out, pop = split_pop(part)
            row[name] = count(out)
            if pop:
                row[name + "_pop"] = count(pop)
        copies.append(row)
    return copies


def main():
    text = open(sys.argv[1]).read().split("\n")
    kernels = {}
    name = None
    meta = None
    for i, l in enumerate(text):
        m = re.match(r"(_Z\S*render_persistent\S*):", l)
        if m:
            name = re.search(r"render_persistentI(.*?)EEv", m.group(1)).group(1)
            name = "<" + ",".join(re.findall(r"L[ib](\d+)E", name + "E")) + ">"
            kernels[name] = {"loops": []}
        if name and l.strip() == ";;#ASMSTART":
            j = text.index("\t;;#ASMEND", i)
            if any("0x3e8" in b for b in text[i:j]):
                kernels[name]["loops"].append(trips_of(text[i + 1:j]))
        m = re.match(r"\s*\.name:\s*(\S+)", l)
        if m:  # (code-object metadata: a kernel's keys in alphabetical order, the figures behind its name)
            meta = None
            if "render_persistent" in m.group(1):
                n = re.search(r"render_persistentI(.*?)EEv", m.group(1)).group(1)
                meta = kernels["<" + ",".join(re.findall(r"L[ib](\d+)E", n + "E")) + ">"]
        m = re.match(r"\s*\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|sgpr_count|private_segment_fixed_size):\s*(\d+)", l)
        if m and meta is not None:
            meta[m.group(1)] = int(m.group(2))
    if "--json" in sys.argv:
        print(json.dumps(kernels, indent=1))
        return
    for n, k in kernels.items():
        meta = {a: b for a, b in k.items() if a != "loops"}
        print(n, meta)
        for li, loop in enumerate(k["loops"]):
            for ci, c in enumerate(loop):
                print("   loop %d copy %d: " % (li, ci) + "  ".join("%s %d (%dv %ds %dm)" % (p, v["all"], v["vector"], v["scalar"], v["memory"]) for p, v in c.items()))


if __name__ == "__main__":
    main()
