"""
Two device-only assembly files of lynx_hip.hip, function by function: did a host-side change leave every kernel alone?

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-slp-vectorize --offload-device-only -S \
        lynx_amd/csrc/lynx_hip.hip -o new.s          (and the same on the other commit: old.s)
    python scripts/compare_device_asm.py old.s new.s

A change in the order of template instantiation on the host moves kernels in the file and renumbers their labels
(`.LBB105_4`, `.Lfunc_end105`, "Header=BB105_4" in comments); nothing else may differ but the compilation unit's id
(`__hip_cuid_<hash of the source>`).  Exit status 1 if a function or any other line does.
"""
import collections
import re
import sys


def split(path):
    """({function: its lines, from .type to .size}, every other line), in file order."""
    functions, rest, name, body = collections.OrderedDict(), [], None, None
    for line in open(path).read().split("\n"):
        start = re.match(r"\t\.type\t(\S+),@function", line)
        if start and body is None:
            name, body = start.group(1), []
        if body is None:
            rest.append(line)
            continue
        body.append(line)
        if re.match(r"\t\.size\t" + re.escape(name) + ",", line):
            functions[name], body = body, None
    return functions, rest


def renumbered(lines):
    text = "\n".join(lines)
    for pattern, plain in ((r"BB\d+_", "BB_"), (r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1"), (r"\.Ltmp\d+", ".Ltmp"), (r"\.LJTI\d+_", ".LJTI_"),
                           (r"__hip_cuid_[0-9a-f]+", "__hip_cuid")):
        text = re.sub(pattern, plain, text)
    return text


(a, rest_a), (b, rest_b) = split(sys.argv[1]), split(sys.argv[2])
differing = sorted(set(a) ^ set(b)) + [name for name in a if name in b and renumbered(a[name]) != renumbered(b[name])]
other_a, other_b = (collections.Counter(renumbered(rest).split("\n")) for rest in (rest_a, rest_b))
print(f"{len(a)} | {len(b)} functions, same order: {list(a) == list(b)}, files identical: {open(sys.argv[1]).read() == open(sys.argv[2]).read()}")
print(f"functions that differ beyond label numbers: {len(differing)}" + "".join(f"\n  {name}" for name in differing))
print(f"lines outside functions (metadata, kernel descriptors), as multisets: {'equal' if other_a == other_b else 'DIFFERENT'}")
for line, count in list((other_a - other_b).items())[:10] + list((other_b - other_a).items())[:10]:
    print(f"  {count} x {line}")
sys.exit(1 if differing or other_a != other_b else 0)
