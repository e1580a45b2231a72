#!/usr/bin/env python3
"""Device code of two builds of a library (or of one object file), compared per symbol: the acceptance check of a refactor that must not
move a kernel.  CPU only; a development aid, not a test.

    python tools/isa_diff.py OLD.so NEW.so            (exit status 0: nothing differs beyond the allowances)

Every gfx950 code object of both files is disassembled (llvm-objdump -d --no-show-raw-insn) and compared per demangled symbol.
Printed: the difference of the symbol sets, and for every symbol whose instructions differ the two instruction counts, whether
the opcode multisets are equal (if not: every opcode whose count differs), and the first differing instruction.  Treated as equal:
  * the two sources of a commutative two-source scalar instruction in either order (s_or_b64 s0, s0, vcc / s_or_b64 s0, vcc, s0);
  * the __hip_cuid_* symbol (a hash of the translation unit's text);
  * the literals of a pc-relative address (s_getpc_b64 + s_add_u32 / s_addc_u32) that resolve to the same symbol + offset.
It reports differences; it does not look for particular instructions.
"""
import bisect, collections, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import code_objects, LLVM

COMMUTATIVE = re.compile(r"^s_(and|or|xor|nand|nor|xnor)_b(32|64)$|^s_(add|addc|mul|min|max)_[iu]32$|^s_mul_hi_[iu]32$")


def demangle(text):
    return subprocess.run(["c++filt"], input=text, capture_output=True, text=True).stdout


def symbol_table(co):
    """-> sorted [(address, demangled name)] of the code object's defined symbols, data included"""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", co], capture_output=True, text=True).stdout
    rows = []
    for l in out.splitlines():
        m = re.match(r"^([0-9a-f]{8,16}) .{7} (\S+)\s+[0-9a-f]+ (?:\.\S+ )?(\S+)$", l)
        if m and m.group(2) not in ("*UND*", "*ABS*"):
            rows.append((int(m.group(1), 16), m.group(3)))
    names = demangle("\n".join(n for _, n in rows)).splitlines()
    return sorted((a, n) for (a, _), n in zip(rows, names))


def resolve(syms, addr):
    k = bisect.bisect_right(syms, (addr, "￿")) - 1
    if k < 0:
        return "0x%x" % addr
    return "<%s+0x%x>" % (syms[k][1], addr - syms[k][0])


def operands(text):
    return [o.strip() for o in text.split(",")] if text else []


def normalise(ins, syms):
    """ins: [(address, opcode, operand text)] of one symbol -> [instruction text] with the allowances applied"""
    lit = {}                                # index of an s_add_u32 / s_addc_u32 -> the pc its literal is relative to, half
    for k, (a, op, _) in enumerate(ins):
        if op != "s_getpc_b64":
            continue
        m = re.match(r"s\[(\d+):(\d+)\]", ins[k][2])
        if not m:
            continue
        lo, hi = "s" + m.group(1), "s" + m.group(2)
        pair = {}
        for j in range(k + 1, min(k + 8, len(ins))):
            o = operands(ins[j][2])
            if ins[j][1] == "s_add_u32" and lo in o[1:] and "lo" not in pair:
                pair["lo"] = j
            if ins[j][1] == "s_addc_u32" and hi in o[1:] and "hi" not in pair:
                pair["hi"] = j
        if len(pair) == 2:
            try:
                vlo = int(operands(ins[pair["lo"]][2])[-1], 0) & 0xffffffff
                vhi = int(operands(ins[pair["hi"]][2])[-1], 0) & 0xffffffff
            except ValueError:
                continue
            off = vhi << 32 | vlo
            off -= (1 << 64) if off >> 63 else 0
            target = resolve(syms, a + 4 + off)
            lit[pair["lo"]] = target + "@lo"; lit[pair["hi"]] = target + "@hi"
    out = []
    for k, (_, op, text) in enumerate(ins):
        o = operands(text)
        if k in lit:
            o[-1] = lit[k]
        if COMMUTATIVE.match(op) and len(o) == 3:
            o[1:] = sorted(o[1:])
        out.append((op + " " + ", ".join(o)).strip())
    return out


def symbols(lib):
    """-> {demangled symbol: [normalised instruction text]} over every gfx950 code object of the file"""
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            syms = symbol_table(co)
            dis = demangle(subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout)
            name, ins = None, []

            def close():
                if name is not None and not name.startswith("__hip_cuid_"):
                    key, n = name, 1
                    while key in table:         # the same symbol in two translation units (agt_step.hip is compiled twice)
                        n += 1; key = "%s  [#%d]" % (name, n)
                    table[key] = normalise(ins, syms)
            for l in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", l)
                if m:
                    close()
                    name, ins = m.group(1), []
                    continue
                m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
                if m and name is not None:
                    ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
            close()
    return table


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
    print("# isa_diff %s -> %s: %d / %d symbols" % (sys.argv[1], sys.argv[2], len(old), len(new)))
    bad = 0
    for s in sorted(set(old) - set(new)):
        print("only in old: %s" % s); bad += 1
    for s in sorted(set(new) - set(old)):
        print("only in new: %s" % s); bad += 1
    for s in sorted(set(old) & set(new)):
        a, b = old[s], new[s]
        if a == b:
            continue
        bad += 1
        ca, cb = collections.Counter(x.split()[0] for x in a), collections.Counter(x.split()[0] for x in b)
        print("differs: %s\n    instructions %d -> %d, opcode multisets %s" % (s, len(a), len(b), "equal" if ca == cb else "differ"))
        for op in sorted(set(ca) | set(cb)):
            if ca[op] != cb[op]:
                print("    %-24s %d -> %d" % (op, ca[op], cb[op]))
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print("    first difference at instruction %d:  %s  |  %s" % (k, a[k] if k < len(a) else "(end)", b[k] if k < len(b) else "(end)"))
    print("# %s" % ("identical beyond the allowances" if not bad else "%d symbols differ" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
