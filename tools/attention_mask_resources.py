#!/usr/bin/env python3
"""Register, scratch and LDS figures of every kernel of csrc/attention.hip, from the compiler's resource-usage remarks (no GPU).

    python tools/attention_mask_resources.py [--before PARENT_COPY_OF_attention.hip] > profiles/attention_mask_<date>_resources.txt

Compiles the file with the library's flags plus -Rpass-analysis=kernel-resource-usage and prints one line per kernel.  With
--before (the parent commit's file, e.g. from `git show HEAD~1:boosted_detr_amd/csrc/attention.hip`, compiled against the
parent's headers if they differ) it prints that file's table first and then compares: every kernel of the parent must appear
in the new file as the mask = none instantiation (MK = 0) with identical figures; exit status 1 otherwise."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from boosted_detr_amd import build as B  # noqa: E402

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
AR = {"0": "fp32", "1": "bf16", "2": "f16"}
MK = {"0": "none", "1": "f32-multiply", "2": "u8-exclude"}


def remarks(src: Path, include: Path):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [B._hipcc(), *B.COMMON_FLAGS, "-I", str(B.CSRC), "-I", str(include), "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
               str(src), "-o", str(Path(tmp) / "a.o")]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = list(out)
    plain = subprocess.run(["c++filt", *names], check=True, capture_output=True, text=True).stdout.splitlines()
    return {short(p): out[n] for n, p in zip(names, plain)}


def KO(args, i) -> str:
    return " key-only" if len(args) > i and args[i] in ("true", "1") else ""


def short(demangled: str) -> str:
    """attn_bwd_kernel<true, 1, 0>(...) -> 'attn_bwd_kernel KCOL=1 AR=bf16 MK=none' (a parent kernel without MK reads MK=none)."""
    m = re.search(r"(attn_\w+)(?:<([^>]*)>)?", demangled)
    name, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    if name == "attn_fwd_kernel":
        return "%s AR=%s MK=%s%s" % (name, AR[args[0]], MK[args[1] if len(args) > 1 else "0"], KO(args, 2))
    if name == "attn_bwd_kernel":
        return "%s KCOL=%d AR=%s MK=%s%s" % (name, args[0] in ("true", "1"), AR[args[1]], MK[args[2] if len(args) > 2 else "0"], KO(args, 3))
    if name == "attn_mask_apply_kernel":
        return "%s MK=%s" % (name, MK[args[0]])
    return name


def table(title, rows):
    print(title)
    print("  %-62s %5s %5s %5s %7s %5s %6s %6s %6s" % ("kernel", "SGPR", "VGPR", "AGPR", "scratch", "occ", "sspill", "vspill", "LDS"))
    for k in sorted(rows):
        print("  %-62s %5s %5s %5s %7s %5s %6s %6s %6s" % ((k,) + tuple(rows[k].get(f, "?") for f in FIELDS)))
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", type=Path, help="the parent commit's attention.hip")
    ap.add_argument("--before-include", type=Path, default=ROOT / "include", help="directory of the parent's bdetr.h")
    a = ap.parse_args()
    print("flags: %s (+ -Rpass-analysis=kernel-resource-usage)\n" % " ".join(B.COMMON_FLAGS))
    after = remarks(B.CSRC / "attention.hip", ROOT / "include")
    bad = []
    if a.before:
        before = remarks(a.before, a.before_include)
        table("BEFORE (parent commit): every kernel of csrc/attention.hip", before)
        for k, v in before.items():
            if after.get(k) != v:
                bad.append(k)
    table("AFTER: the mask = none instantiations (the kernels bdetr_attention_fwd / _bwd launch)", {k: v for k, v in after.items() if "MK=" not in k or "MK=none" in k})
    table("AFTER: the masked instantiations", {k: v for k, v in after.items() if "MK=" in k and "MK=none" not in k})
    if a.before:
        print("mask = none against the parent: %s" % ("IDENTICAL in every figure" if not bad else "DIFFERENT: " + ", ".join(bad)))
    scratch = [k for k, v in after.items() if v.get("ScratchSize [bytes/lane]") != "0"]
    print("scratch of every instantiation: %s" % ("0" if not scratch else "NON-ZERO: " + ", ".join(scratch)))
    return 1 if bad or scratch else 0


if __name__ == "__main__":
    sys.exit(main())
