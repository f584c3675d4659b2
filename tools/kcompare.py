"""Compare the kernels of two builds of the library, symbol by symbol (tools/kcheck.py's parsers):

    python tools/kcompare.py OLD.so NEW.so [--arch gfx950]

Reports symbols missing on either side, symbols defined in more than one code object of NEW, and
every symbol whose instruction list or metadata (registers, LDS, scratch, spills) differs.  The
32-bit literals of the s_add_u32 / s_addc_u32 pair after an s_getpc_b64 are the distance to another
symbol, which moves with the layout: symbols that differ only there are listed apart; the padding
after a symbol's last instruction is not compared.  Exit status 1 on any other difference.
"""
from __future__ import annotations

import collections
import re
import sys

import kcheck

META = re.compile(r"\.(agpr_count|sgpr_count|vgpr_count|group_segment_fixed_size|private_segment_fixed_size|"
                  r"sgpr_spill_count|vgpr_spill_count):\s+(\d+)")


def load(lib, arch):
    text = kcheck.disassemble(lib, arch, kcheck.llvm_dir())
    ks = kcheck.kernels(text)
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count", "\n" + text.split(kcheck.NOTES_MARK, 1)[1]):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = sorted(META.findall("- .agpr_count" + blk))
    return ks, meta


def mask_pc(body):
    """The instruction list without its trailing padding (s_nop / s_code_end up to the next symbol or
    the end of the code object) and with the literals of the add pair after each s_getpc_b64 masked."""
    body = list(body)
    while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
        body.pop()
    out, left = [], 0
    for ins in body:
        if ins.startswith("s_getpc_b64"):
            left = 2
        elif left and ins.startswith(("s_add_u32", "s_addc_u32")):
            ins, left = ins.rsplit(",", 1)[0] + ", <pc-relative>", left - 1
        out.append(ins)
    return out


def main(old, new, arch="gfx950"):
    (ko, mo), (kn, mn) = load(old, arch), load(new, arch)
    dup = [n for n, c in collections.Counter(n for n, _ in kn).items() if c > 1]
    do, dn = dict(ko), dict(kn)
    gone, added = sorted(set(do) - set(dn)), sorted(set(dn) - set(do))
    literal = [n for n in do if n in dn and mask_pc(do[n]) == mask_pc(dn[n]) and
               [i for i in do[n] if i.startswith("s_add")] != [i for i in dn[n] if i.startswith("s_add")]]
    code = [n for n in do if n in dn and mask_pc(do[n]) != mask_pc(dn[n])]
    meta = [n for n in mo if n in mn and mo[n] != mn[n]]
    print(f"{len(do)} symbols in {old}, {len(dn)} in {new}; {len(mo)} / {len(mn)} kernels with metadata")
    for title, names in (("missing in NEW", gone), ("only in NEW", added), ("defined more than once in NEW", dup),
                         ("instructions differ", code), ("metadata differs", meta),
                         ("pc-relative literals only", literal)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", n)
    return 1 if gone or added or dup or code or meta else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    arch = sys.argv[sys.argv.index("--arch") + 1] if "--arch" in sys.argv else "gfx950"
    sys.exit(main(args[0], args[1], arch))
