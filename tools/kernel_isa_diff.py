"""Do two builds hold the same gfx950 machine code, kernel by kernel?  (runs without a GPU):
python tools/kernel_isa_diff.py OLD.o [OLD.o ...] -- NEW.o [NEW.o ...]
Each side is a set of object files; a kernel may sit in another object on the other side.  Per demangled kernel: IDENTICAL / DIFFERENT with
the instruction lines of both sides, then the kernels that exist on one side only or more than once.  Compared is the disassembly's TEXT:
mnemonics, operands and branch targets relative to the kernel's start.  Left out: the line naming the file, addresses and encodings (a
kernel's place in its code object), and the s_nop / s_code_end padding behind a kernel's last instruction.  Exit status 1 unless all is IDENTICAL."""
import os, re, subprocess, sys, tempfile
llvm = "/opt/rocm/lib/llvm/bin"
if "--" not in sys.argv:
    sys.exit(__doc__)
cut = sys.argv.index("--")
sides = [sys.argv[1:cut], sys.argv[cut + 1:]]

def kernels(obj):
    """{mangled name: [instruction line, ...]} of the gfx950 code object inside a host object"""
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "k.o")
        subprocess.run(["cp", os.path.abspath(obj), tmp], check=True)
        subprocess.run([llvm + "/llvm-objdump", "--offloading", tmp], check=True, capture_output=True)
        co = [f for f in os.listdir(d) if "amdgcn" in f]
        if not co:
            sys.exit("no gfx code object in " + obj)
        dis = subprocess.run([llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", os.path.join(d, co[0])],
                             check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            text, _, note = line.partition("//")
            target = re.search(r"<\S+>\s*$", note)           # a branch's target: symbol + offset
            cur.append(text.strip() + (" " + target.group(0).strip() if target else ""))
    for body in out.values():
        while body and re.match(r"(s_nop 0|s_code_end|\.\.\.|)$", body[-1]):     # ("...": zero bytes the disassembler leaves out)
            body.pop()
    return out

found = [{}, {}]                                             # mangled name -> [(object, lines), ...]
for side, objs in zip(found, sides):
    for o in objs:
        for name, body in kernels(o).items():
            side.setdefault(name, []).append((os.path.basename(o), body))
names = sorted(set(found[0]) | set(found[1]))
dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines())) if names else {}
short = lambda n: dem[n].split("(")[0].replace("void ", "").replace("apsu_he::", "")
bad = 0
for n in names:
    a, b = found[0].get(n, []), found[1].get(n, [])
    if len(a) == 1 and len(b) == 1:
        same = a[0][1] == b[0][1]
        bad += not same
        print("%-9s %-72s %6d %6d lines  %s -> %s" % ("IDENTICAL" if same else "DIFFERENT", short(n)[:72], len(a[0][1]), len(b[0][1]), a[0][0], b[0][0]))
for n in names:
    a, b = found[0].get(n, []), found[1].get(n, [])
    if len(a) != 1 or len(b) != 1:
        bad += 1
        print("%-9s %-72s old: %s  new: %s" % ("ONE-SIDED" if not a or not b else "REPEATED", short(n)[:72], ",".join(o for o, _ in a) or "-", ",".join(o for o, _ in b) or "-"))
print("%d kernels, %d not IDENTICAL" % (len(names), bad))
sys.exit(1 if bad else 0)
