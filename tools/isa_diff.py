#!/usr/bin/env python3
"""Is the device code of two builds of libgs_amd.so the same, kernel by kernel?

    python tools/isa_diff.py <parent libgs_amd.so> <this tree's libgs_amd.so> [--renamed OLD=NEW ...] [--allow-changed SUBSTR ...]

The gate of a refactor that must not change what runs on the GPU.  For every kernel symbol it compares the sequence of
(mnemonic, operands) that llvm-objdump prints and the resource fields of the code object's metadata, and lists the kernels
only in the parent, the kernels only in this tree and the kernels that differ (with the index of the first differing
instruction).  `--renamed OLD=NEW` replaces the substring OLD of a parent symbol by NEW before the two sides are matched
(a kernel that lost a template parameter or an argument).  `--allow-changed SUBSTR`: a kernel whose symbol contains SUBSTR may
differ as long as it has no more instructions, registers, spills, scratch or LDS than the parent's (a change that only takes
work away from it); such a kernel is listed with "ok".  Exit status 0 only if nothing else differs and nothing is new.  CPU only.

Build the parent library from a checkout of the parent commit with the same gs_build.build(): never from this tree with
switches set."""
import argparse
import sys

from isa_loops import disassemble_library
from test_kernel_resources import code_objects, kernel_metadata

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")
NO_MORE = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def load(lib, renamed=()):
    """{kernel symbol: ([(mnemonic, operands)], {field: value})} of every kernel in the library."""
    meta = {}
    for elf in code_objects(open(lib, "rb").read()):
        meta.update(kernel_metadata(elf))
    dis = disassemble_library(lib)
    assert set(meta) <= set(dis), sorted(set(meta) - set(dis))
    out = {}
    for name, md in meta.items():
        new = name
        for old, to in renamed:
            new = new.replace(old, to)
        assert new not in out, (name, new)
        out[new] = ([(mn, ops) for _, mn, ops in dis[name]], {f: md[f] for f in FIELDS if f in md})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--allow-changed", action="append", default=[], metavar="SUBSTR")
    args = ap.parse_args()
    renamed = [tuple(r.split("=", 1)) for r in args.renamed]
    a, b = load(args.parent, renamed), load(args.tree)

    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = []
    for name in sorted(set(a) & set(b)):
        (ia, ma), (ib, mb) = a[name], b[name]
        first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), None)
        if first is None and len(ia) != len(ib):
            first = min(len(ia), len(ib))
        fields = [f"{f} {ma.get(f)} -> {mb.get(f)}" for f in FIELDS if ma.get(f) != mb.get(f)]
        ok = (any(s in name for s in args.allow_changed) and len(ib) <= len(ia) and
              all(mb.get(f, 0) <= ma.get(f, 0) for f in NO_MORE))
        if first is not None or fields:
            differ.append((name, first, len(ia), len(ib), fields, ok))

    for old, to in renamed:
        print(f"renamed: {old} -> {to}")
    print(f"kernels only in the parent: {len(gone)}")
    for name in gone:
        print(f"   {name}  ({len(a[name][0])} instructions)")
    print(f"kernels only in this tree: {len(new)}")
    for name in new:
        print(f"   {name}  ({len(b[name][0])} instructions)")
    print(f"kernels that differ: {len(differ)}")
    for name, first, na, nb, fields, ok in differ:
        where = "same instructions" if first is None else f"first differing instruction {first} ({na} -> {nb} instructions)"
        print(f"   {'ok ' if ok else ''}{name}: {where}" + "".join(f"; {f}" for f in fields))
    print(f"totals: parent {len(a)} kernels, {sum(len(v[0]) for v in a.values())} instructions; "
          f"this tree {len(b)} kernels, {sum(len(v[0]) for v in b.values())} instructions; "
          f"{len(set(a) & set(b))} common, {len(differ)} differing, {len(gone)} removed, {len(new)} new")
    return 1 if new or not all(d[-1] for d in differ) else 0


if __name__ == "__main__":
    sys.exit(main())
