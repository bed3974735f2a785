#!/usr/bin/env python3
"""Mnemonic histogram of every barrier-to-barrier segment of one kernel of csrc/xq_conv_ip4.hip (--source: another file of csrc/), from `hipcc -S` with
the flags build.py gives that source (build.flags_for: the chain unit is compiled with -mllvm -amdgpu-mfma-vgpr-form; cross-compiles, no GPU; one compiler process).  The segments are in the order of the assembly text, which for the chained
tower kernel is the order of its phases: ... | K loop 1 | epilogue 1 | K loop 2 | epilogue 2 or staging | exit | fill.

    python tools/ip4_isa_phases.py [-DNAME[=V] ...] [--kernel SUBSTR] [--source xq_tower.hip] [--asm FILE] [--top N] [--json OUT]

--kernel: a substring of the (mangled) kernel symbol; default the c6 chain at 128 filters, k_resblock_ip4_c8<128, 1, 1, false>.
--asm: read an existing -S output instead of compiling.  Per segment: instructions, VALU / SALU / LDS / VMEM / MFMA counts and
the --top most frequent mnemonics (default: all of them).  Also the kernel's register, scratch and LDS figures as the
assembler directives state them.
"""
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))
DEFAULT_KERNEL = "k_resblock_ip4_c8ILi128ELi1ELi1ELb0E"


def klass(m):
    if "mfma" in m:
        return "MFMA"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_"):
        return "SALU"
    return "other"


def compile_asm(defines, source):
    import build
    tmp = tempfile.mkdtemp(prefix="ip4_isa_")
    out = os.path.join(tmp, "kernel.s")
    cmd = ["hipcc"] + build.flags_for(source) + list(defines) + ["-w", "-S", "--cuda-device-only", os.path.join(build.CSRC, source), "-o", out]
    try:
        subprocess.check_call(cmd)                  # (-w: the source's warnings belong to the build; errors are shown)
        return open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_text(text, sub):
    lines = text.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and sub in l]
    assert starts, f"no kernel symbol contains {sub!r}"
    assert len(starts) == 1, "ambiguous: " + ", ".join(lines[i] for i in starts)
    i0 = starts[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel"))
    body_end = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    meta = {}
    for l in lines[body_end:i1]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size)\s+(\S+)", l)
        if m:
            meta[m.group(1)] = m.group(2)
    return lines[i0].rstrip(":"), lines[i0 + 1:body_end + 1], meta


def segments(body):
    segs, cur = [], collections.Counter()
    for l in body:
        l = l.split(";")[0].strip()
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        m = l.split()[0]
        if m == "s_barrier":
            segs.append(cur)
            cur = collections.Counter()
        else:
            cur[m] += 1
    segs.append(cur)
    return segs


def main():
    argv = sys.argv[1:]
    opt = lambda k, d=None: argv[argv.index(k) + 1] if k in argv else d
    sub = opt("--kernel", DEFAULT_KERNEL)
    top = int(opt("--top", "0"))
    text = open(opt("--asm")).read() if opt("--asm") else compile_asm([a for a in argv if a.startswith("-D")], opt("--source", "xq_conv_ip4.hip"))
    name, body, meta = kernel_text(text, sub)
    segs = segments(body)
    print(name)
    print(" ".join(f"{k}={v}" for k, v in meta.items()))
    rows = []
    for i, s in enumerate(segs):
        by = collections.Counter()
        for m, n in s.items():
            by[klass(m)] += n
        total = sum(s.values())
        rows.append({"segment": i, "instructions": total, "classes": dict(by), "mnemonics": dict(s)})
        print(f"--- segment {i}: {total} instructions  " + "  ".join(f"{k} {by[k]}" for k in ("VALU", "SALU", "LDS", "VMEM", "MFMA", "other") if by[k]))
        common = s.most_common(top or None)
        for j in range(0, len(common), 6):
            print("    " + "  ".join(f"{m} {n}" for m, n in common[j:j + 6]))
    if opt("--json"):
        with open(opt("--json"), "w") as f:
            json.dump({"kernel": name, "resources": meta, "segments": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
