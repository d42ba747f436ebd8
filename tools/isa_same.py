#!/usr/bin/env python3
"""Are the kernel instances of two `make asm` outputs the same code?
python tools/isa_same.py A.s B.s [NAME]  (the gfx950 .s files under build/asm/)

Compares the instruction text of every symbol whose name contains NAME
(default render_tiles; query_kernel, occlusion_kernel, radiance_kernel and
guides_kernel for the `make asm-queries` files), without comments and
assembler directives and with the function's number taken out of its
.LBB<n>_ block labels (it shifts when other functions come or go).  Prints
the number of symbols and of differing ones; exit 1 if a symbol differs or is
in one file only."""
import re
import sys


KERNEL = sys.argv[3] if len(sys.argv) > 3 else "render_tiles"


def functions(path):
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"(\S*%s\S*):" % re.escape(KERNEL), line)
        if m and name is None:
            # the default material set (rt_path.h M_ANY) names the instance builds before MatSet knew
            name, body = m.group(1).replace("LN3rtp6MatSetE0E", ""), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
                continue
            text = line.split(";")[0].rstrip()
            if not text.strip() or re.match(r"\s+\.", text):  # comment / directive
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
only = sorted(set(a) ^ set(b))
differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
print("%d %s symbols in A, %d in B, %d in one file only, %d differing" % (len(a), KERNEL, len(b), len(only), len(differ)))
for k in only + differ:
    print("  " + k)
sys.exit(1 if only or differ or not a else 0)
