#!/usr/bin/env python
"""Does a kernel refactor leave the compiled instruction stream alone?   python tools/isa_diff.py fd_kernels_kp.hip [--base REV] [-D...]

Compiles fastdiff_amd/csrc/<file> for the device at REV (default HEAD, from `git archive`) and in the working tree with the compiler
and flags of fastdiff_amd.build plus `--cuda-device-only -S`, cuts out every kernel's body, drops comment lines, directives and
local-label definitions, renames `.LBB<n>_` to one prefix, and compares kernel by kernel (matched by name without the argument list).
A kernel whose stream differs is compared once more by what the hand-counted waits depend on -- the ordered mnemonics of its matrix,
buffer-store, LDS-DMA and LDS-read instructions and barriers together with every `s_waitcnt` that names vmcnt -- and by its resource
line (VGPRs / SGPRs / scratch / LDS / occupancy), which must not grow.  Needs no GPU.  Exit status 1 if any stream differs.
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastdiff_amd import build  # noqa: E402

KEEP = re.compile(r"v_mfma|buffer_store|global_load_lds|ds_read|ds_load|s_barrier")
RES = [("VGPRs", r"; NumVgprs: (\d+)"), ("SGPRs", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
       ("LDS", r"; LDSByteSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)")]


def plain_name(sym):
    """_ZN8fdk_fast8k_lvc_h2ILi64ELb1EEEvPKf -> fdk_fast::k_lvc_h2<Li64,Lb1>: the name without the argument list (which a refactor may change)"""
    parts, rest = [], sym[3:] if sym.startswith("_ZN") else ""
    while (m := re.match(r"(\d+)", rest)):
        n = int(m.group(1))
        parts.append(rest[m.end():m.end() + n])
        rest = rest[m.end() + n:]
    t = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
    return "::".join(parts) + ("<" + t.group(1)[:-1].replace("E", ",") + ">" if t else "") if parts else sym


def kernels(root, src, defs):
    """{name: (instruction lines, resource dict)} of every kernel of root/fastdiff_amd/csrc/src."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([build.HIPCC] + build.FLAGS + defs + ["--cuda-device-only", "-S", os.path.join(root, "fastdiff_amd", "csrc", src), "-o", out], check=True)
        txt = open(out).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M)
    res = {}
    for sym in syms:
        body, tail = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:\n(.*?; Occupancy: \d+)" % re.escape(sym), txt, re.M | re.S).groups()
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.strip()) for l in body.split("\n")]
        lines = [l for l in lines if l and not l.startswith((";", ".")) and not l.endswith(":")]
        res[plain_name(sym)] = (lines, {k: int(re.search(p, tail).group(1)) for k, p in RES})
    return res


def scheduled(lines):
    """the instructions the hand-counted waits are about, register names aside"""
    return [l if l.startswith("s_waitcnt") else l.split()[0] for l in lines if KEEP.match(l) or (l.startswith("s_waitcnt") and "vmcnt" in l)]


def main():
    args = sys.argv[1:]
    base = args.pop(args.index("--base") + 1) if "--base" in args else "HEAD"
    defs = [a for a in args if a.startswith("-D")]
    src = [a for a in args if a.endswith(".hip")][0]
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", base, "fastdiff_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        old = kernels(tmp, os.path.basename(src), defs)
    new = kernels(ROOT, os.path.basename(src), defs)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in {'the working tree' if name in new else base}")
            bad = 1
            continue
        (lo, ro), (ln, rn) = old[name], new[name]
        rline = " / ".join(f"{k} {ro[k]}" + (f" -> {rn[k]}" if rn[k] != ro[k] else "") for k, _ in RES)
        if lo == ln:
            print(f"{name}: identical ({len(ln)} lines, {sum(l.startswith('v_mfma') for l in ln)} v_mfma); {rline}")
            continue
        bad = 1
        so, sn = scheduled(lo), scheduled(ln)
        grew = [k for k, _ in RES if (rn[k] < ro[k] if k == "occupancy" else rn[k] > ro[k])]
        print(f"{name}: DIFFERS ({len(lo)} -> {len(ln)} lines); matrix / store / DMA / LDS-read / barrier / vmcnt sequence "
              f"{'identical' if so == sn else 'DIFFERS'} ({len(so)} -> {len(sn)}); {rline}" + (f"; GREW: {', '.join(grew)}" if grew else ""))
    return bad


if __name__ == "__main__":
    sys.exit(main())
