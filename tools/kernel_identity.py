#!/usr/bin/env python3
"""Compare the kernels of two builds of wgrt_trace.hip instruction for instruction.

  hipcc -S --cuda-device-only -O3 -std=c++17 -ffp-contract=off -fno-fast-math -mllvm -disable-machine-licm \\
        --offload-arch=gfx950 -I include -o A.s gpu_ray_tracing_for_waveguide_based_ar_display_amd/csrc/wgrt_trace.hip
  python tools/kernel_identity.py A.s B.s [--map]

Kernels pair by instantiation: a Jones kernel's key is (mode, locator form, cell width, fused, single wavelength, AMP),
read from its demangled name whether the build names the mode in the kernel's name (trace_jones_fate_kernel<...>) or
in a template argument (trace_jones_mode_kernel<..., (wgrt::TraceMode)4, ...>); every other kernel pairs by its name.
Compared are the instructions with comments stripped and block labels renumbered per kernel, and the .amdhsa_
resource lines (registers, scratch, LDS, kernarg size).  --map prints the name pairs.  Exit status 1 on any difference.
"""
import re
import subprocess
import sys

MODES = ["plain", "tl", "learn", "chain", "fate", "reps", "ev", "fp", "hits", "paths", "visits",
         "stokes"]   # wgrt::TraceMode's order
CELL = {"unsigned int": 32, "unsigned long": 64}


def key_of(name, sym):
    """The instantiation a demangled kernel name stands for."""
    b = lambda s: s.strip() == "true"
    m = re.search(r"trace_jones_(mode|learn)_kernel<wgrt::(Byte)?LocatorT<([^>]*)> ?(?:, \(wgrt::TraceMode\)(\d+), (\w+), (\w+), (\w+))?>", name)
    if m:   # the mode as a template argument
        mode = MODES[int(m.group(4))] if m.group(1) == "mode" else "learn"
        return (mode, bool(m.group(2)), CELL[m.group(3).strip()], *[b(m.group(k) or "false") for k in (5, 6, 7)])
    m = re.search(r"trace_jones_(b_)?(?:(tl|learn|chain|fate|reps|ev|fp)_)?kernel<([^>]*)>", name)
    if m:   # a name per mode and locator form
        byte, mode, args = bool(m.group(1)), m.group(2) or "plain", m.group(3).split(",")
        flags = [b(a) for a in args[1:]]
        fused, single, amp = {"plain": lambda: flags, "tl": lambda: flags + [False], "learn": lambda: [False] * 3,
                              "chain": lambda: [False, False] + flags}.get(mode, lambda: [False] + flags)()
        return (mode, byte, CELL[args[0].strip()], fused, single, amp)
    return sym


def kernels(path):
    """{key: (name, instructions, resource lines)} of an assembly file."""
    lines = open(path).read().split("\n")
    syms, res = [], {}
    for i, l in enumerate(lines):
        if l.startswith("\t.amdhsa_kernel "):
            sym = l.split()[1]
            syms.append(sym)
            j = i + 1
            res[sym] = []
            while not lines[j].startswith("\t.end_amdhsa_kernel"):
                res[sym].append(" ".join(lines[j].split()))
                j += 1
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith("_Z") and l.split(":")[0] in res}
    out = {}
    for sym, name in zip(syms, names):
        body, labels = [], {}
        for l in lines[start[sym] + 1:]:
            if l.startswith("\t.section"):   # the kernel descriptor follows the code
                break
            l = " ".join(l.split(";")[0].split())
            if l:
                body.append(l)
        # block labels carry the function's number in the file: renumbered in order of appearance
        text = re.sub(r"\.L(BB|tmp)[0-9_]+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(body))
        key = key_of(name, sym)
        assert key not in out, key
        out[key] = (name, text.split("\n"), res[sym])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b), key=str):
        if k not in a or k not in b:
            print("UNPAIRED", k, "only in", sys.argv[1] if k in a else sys.argv[2])
            bad += 1
            continue
        (na, ia, ra), (nb, ib, rb) = a[k], b[k]
        if "--map" in sys.argv and na != nb:
            print(re.sub(r"\(wgrt::TraceArgs.*", "", na), "->", re.sub(r"\(wgrt::TraceArgs.*", "", nb))
        if ia != ib or ra != rb:
            first = next((n for n, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            print("DIFFERENT", k, "instructions %d / %d, first difference at %d;" % (len(ia), len(ib), first),
                  "resource lines", "equal" if ra == rb else "differ")
            bad += 1
    print("%d kernels / %d kernels, %d pairs, %d not identical" % (len(a), len(b), len(set(a) & set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
