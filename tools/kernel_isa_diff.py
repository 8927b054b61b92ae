#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings (hipcc ... --cuda-device-only -S).

For every kernel symbol: is the instruction stream textually the same (comment lines and compiler-generated label
numbers ignored), and do the kernel descriptors agree?  A kernel that differs is classed as

  same        identical instruction stream and descriptor numbers
  reordered   not identical, but the same count of every opcode and no descriptor number higher than before
  DIFFERENT   anything else

This is how a change to code shared by the chain kernels (csrc/chain_sync.hpp, csrc/chain_tile.hpp) is checked against its
parent before it goes to a GPU.  A kernel whose descriptor lacks one of FIELDS, or whose body is not
found, is an error: nothing that failed to parse may pass as equal.
CPU only.  usage: kernel_isa_diff.py BEFORE.s AFTER.s [--filter REGEX] [--all]
"""
import argparse
import collections
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def parse(path):
    """-> {kernel symbol: (normalised instruction lines, {descriptor field: int})}"""
    with open(path, errors="replace") as f:
        lines = f.read().split("\n")
    meta = {}
    cur = None
    in_meta = False
    for ln in lines:
        if ln.strip() == ".amdgpu_metadata":
            in_meta = True
            continue
        if ln.strip() == ".end_amdgpu_metadata":
            in_meta = False
            continue
        if not in_meta:
            continue
        m = re.match(r"^(  - |    )\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip()
        if key == "name":
            meta[val.strip("'\"")] = cur
        elif key in FIELDS:
            cur[key] = int(val)
    bodies = {}
    name, body, labels = None, None, None
    for ln in lines:
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
            if m and m.group(1) in meta:
                name, body, labels = m.group(1), [], {}
            continue
        s = ln.split(";", 1)[0].strip()
        if s.startswith(".Lfunc_end"):
            bodies[name] = body
            name = None
            continue
        if not s or s.startswith("//") or s.startswith(".p2align") or s.startswith(".loc") or s.startswith(".cfi") or s.startswith(".file"):
            continue
        s = LABEL.sub(lambda mm: labels.setdefault(mm.group(0), ".L%d" % len(labels)), s)
        body.append(re.sub(r"\s+", " ", s))
    if not meta:
        raise ValueError("%s: no kernel found in an .amdgpu_metadata block" % path)
    for k in meta:
        missing = [f for f in FIELDS if f not in meta[k]]
        if missing:
            raise ValueError("%s: kernel %s: descriptor field(s) not found: %s" % (path, k, ", ".join(missing)))
        if not bodies.get(k):
            raise ValueError("%s: kernel %s: no instructions found between its label and .Lfunc_end" % (path, k))
    return {k: (bodies[k], meta[k]) for k in meta}


def opcodes(body):
    return collections.Counter(ln.split(" ", 1)[0] for ln in body if not ln.endswith(":"))


def classify(before, after):
    """(body, descriptor) of one kernel before and after -> (verdict, note)"""
    (bo, mo), (bn, mn) = before, after
    changed = [f for f in FIELDS if mo[f] != mn[f]]
    note = " ".join("%s %s->%s" % (f, mo[f], mn[f]) for f in changed)
    if bo == bn and not changed:
        return "same", note
    if opcodes(bo) == opcodes(bn) and all(mn[f] <= mo[f] for f in FIELDS):
        return "reordered", note
    if bo == bn:
        return "DIFFERENT", note + " (instructions identical)"
    d = opcodes(bn)
    d.subtract(opcodes(bo))
    return "DIFFERENT", note + " opcodes: " + " ".join("%s%+d" % (o, n) for o, n in sorted(d.items()) if n)[:160]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--filter", default="", help="only kernels whose symbol matches this regular expression")
    ap.add_argument("--all", action="store_true", help="list the identical kernels too")
    a = ap.parse_args(argv)
    old, new = parse(a.before), parse(a.after)
    flt = re.compile(a.filter)
    count = collections.Counter()
    for k in sorted(set(old) | set(new)):
        if not flt.search(k):
            continue
        if k not in old or k not in new:
            verdict, note = "DIFFERENT", "only in " + ("AFTER" if k in new else "BEFORE")
        else:
            verdict, note = classify(old[k], new[k])
            bn, mn = new[k]
            note = ("%d instructions, vgpr %s agpr %s sgpr %s scratch %s spill %s lds %s  " % ((len(bn),) + tuple(mn[f] for f in FIELDS))) + note
        count[verdict] += 1
        if a.all or verdict != "same":
            print("%-10s %s\n           %s" % (verdict, k, note))
    print("kernels: %d  same: %d  reordered: %d  DIFFERENT: %d" % (sum(count.values()), count["same"], count["reordered"], count["DIFFERENT"]))
    return 1 if count["DIFFERENT"] else 0


if __name__ == "__main__":
    sys.exit(main())
