#!/usr/bin/env python3
"""CPU only: compares the gfx950 assembly of named csrc files between two trees, kernel by kernel.

  tools/isa_diff.py --before <tree> --after <tree> --out profiles/x.json gemm_exact.hip gemm_fast.hip ...
  (a tree is a checkout root: `git archive <rev> | tar -x -C <dir>` gives the parent's)

Each file is compiled in each tree with the flags of the ISA tests (tests/test_isa_budget_cpu.py).  Per kernel the report holds
  * identical: the instruction stream is the same, line for line (comments dropped, and the function's ordinal in its file dropped from
    the block labels .LBB<fn>_<block>, so that a kernel does not differ because another one left or joined the file before it);
  * vgpr / sgpr / lds / scratch, before and after, from the code object's metadata;
  * fp: the histogram of the floating-point instructions (v_fma* v_fmac* v_mul_f* v_add_f* v_sub_f* v_pk_* v_mfma* v_exp* v_rcp*
    v_sqrt*), before and after - with -ffp-contract=fast this is what shows a changed contraction, i.e. changed bits.
Nothing else of the assembly is looked at.  Conditions (exit status 1 if one fails): same kernels on both sides, fp histogram equal,
scratch not larger, VGPRs in the same allocation granule (8 registers) or lower; for files after --identical, identical assembly.
--moved old_file:name=new_file:name pairs a kernel of the before tree with the kernel that replaces it in the after tree (another file,
another name; `name` is a part of the mangled name that fits exactly one kernel; several old kernels may name one new kernel).  The pair
meets the same conditions, and a leading `=` on the argument requires identical assembly.  The old kernel no longer counts as missing from its file.
--brief keeps the report small: a kernel whose assembly is identical is counted per file (kernels, identical, instructions), not listed;
every other kernel is reported in full."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only"]
CSRC = os.path.join("robust-multimodal-contrastive-learning_amd", "csrc")
FP = re.compile(r"v_(fma|fmac|mul_f|add_f|sub_f|pk_|mfma|exp|rcp|sqrt)")
VGPR_GRANULE = 8
META = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "lds": ".group_segment_fixed_size", "scratch": ".private_segment_fixed_size"}


def compile_asm(tree, f, tmp, tag):
    dst = os.path.join(tmp, f"{tag}_{f}.s")
    cmd = ["hipcc", *FLAGS, "-I" + os.path.join(tree, "include"), os.path.join(tree, CSRC, f), "-o", dst]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"isa_diff: {' '.join(cmd)} failed:\n{r.stderr[-3000:]}")
    return open(dst).read()


def kernels(text):
    """{mangled name: {vgpr, sgpr, lds, scratch, fp: {mnemonic: count}, body: [instruction lines]}}"""
    out = {}
    meta = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M).group(1)
        out[name] = {k: int(re.search(r"^\s*" + re.escape(key) + r":\s*(\d+)", entry, re.M).group(1)) for k, key in META.items()}
    lines = text.split("\n")
    for name, k in out.items():
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        body = []
        for l in lines[start + 1:]:
            l = l.split(";")[0].strip()
            if l.startswith(".Lfunc_end"):
                break
            if l:
                # (block labels carry the function's ordinal in its file, the descriptor's directives the kernel's own name: both dropped)
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", l).replace(name, "<kernel>"))
        k["body"] = body
        k["fp"] = dict(sorted(Counter(l.split()[0] for l in body if FP.match(l)).items()))
    return out


def compare(kb, kn, must_be_identical):
    """(report entry, the conditions the pair fails) of one kernel before / after"""
    r = {"identical": kb["body"] == kn["body"], "instructions": [len(kb["body"]), len(kn["body"])]}
    for key in META:
        r[key] = [kb[key], kn[key]]
    r["fp_equal"] = kb["fp"] == kn["fp"]
    r["fp"] = kb["fp"] if r["fp_equal"] else {"before": kb["fp"], "after": kn["fp"]}
    why = []
    if not r["fp_equal"]:
        why.append("fp histogram")
    if kn["scratch"] > kb["scratch"]:
        why.append("scratch")
    if -(-kn["vgpr"] // VGPR_GRANULE) > -(-kb["vgpr"] // VGPR_GRANULE):
        why.append("vgpr granule")
    if must_be_identical and not r["identical"]:
        why.append("assembly not identical")
    r["ok"] = not why
    return r, why


def pick(ks, f, part, tag):
    hits = [n for n in ks if part in n]
    if len(hits) != 1:
        sys.exit(f"isa_diff: --moved: {part!r} names {len(hits)} kernels of {f} ({tag}), not one: {hits}")
    return hits[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", required=True)
    ap.add_argument("--after", required=True)
    ap.add_argument("--out")
    ap.add_argument("--identical", nargs="*", default=[], help="files whose assembly must not change at all")
    ap.add_argument("--moved", nargs="*", default=[], metavar="OLD_FILE:NAME=NEW_FILE:NAME",
                    help="a kernel of the before tree that the after tree holds in another file / under another name (NAME: a part of the "
                         "mangled name that fits one kernel); compared with block labels normalised; a leading '=' (=OLD...=NEW...) "
                         "requires identical assembly")
    ap.add_argument("--brief", action="store_true", help="count identical kernels per file instead of listing them")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = a.files + [f for f in a.identical if f not in a.files]
    moved = []                                                # (old file, old part, new file, new part, must be identical)
    for m in a.moved:
        old, new = m.lstrip("=").split("=")
        moved.append((*old.split(":"), *new.split(":"), m.startswith("=")))
    need = {(f, tag) for f in files for tag in ("before", "after")} | {(m[0], "before") for m in moved} | {(m[2], "after") for m in moved}
    trees = {"before": a.before, "after": a.after}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.j) as ex:
        jobs = {(f, tag): ex.submit(compile_asm, trees[tag], f, tmp, tag) for f, tag in sorted(need)}
        asm = {k: kernels(j.result()) for k, j in jobs.items()}
    report, failed, moved_report = {}, [], {}
    gone, came = {}, {}                                       # per file: kernels a --moved takes out of the before set / adds to the after set
    for of, op, nf, np_, ident in moved:
        on, nn = pick(asm[(of, "before")], of, op, "before"), pick(asm[(nf, "after")], nf, np_, "after")
        gone.setdefault(of, set()).add(on)
        came.setdefault(nf, set()).add(nn)
        r, why = compare(asm[(of, "before")][on], asm[(nf, "after")][nn], ident)
        r["must_be_identical"] = ident
        if why:
            failed.append(f"{of}: {on} -> {nf}: {nn}: {', '.join(why)}")
        moved_report[f"{of}:{on}"] = {"now": f"{nf}:{nn}", **r}
    if moved:
        print(f"moved: {len(moved_report)} kernels, {sum(k['identical'] for k in moved_report.values())} identical, "
              f"{sum(k['fp_equal'] for k in moved_report.values())} with an equal fp histogram")
    for f in files:
        b, n = asm[(f, "before")], asm[(f, "after")]
        if set(b) - gone.get(f, set()) != set(n) - came.get(f, set()):
            failed.append(f"{f}: kernel sets differ: {sorted((set(b) - gone.get(f, set())) ^ (set(n) - came.get(f, set())))}")
        report[f] = {}
        for name in sorted(set(b) & set(n)):
            r, why = compare(b[name], n[name], f in a.identical)
            if why:
                failed.append(f"{f}: {name}: {', '.join(why)}")
            report[f][name] = r
        ks = report[f].values()
        print(f"{f}: {len(ks)} kernels, {sum(k['identical'] for k in ks)} identical, {sum(k['fp_equal'] for k in ks)} with an equal fp histogram, "
              f"{sum(k['scratch'][1] > 0 for k in ks)} with scratch")
    if a.brief:
        report = {f: {"kernels": len(ks), "identical": sum(k["identical"] for k in ks.values()),
                      "instructions_of_the_identical": sum(k["instructions"][0] for k in ks.values() if k["identical"]),
                      "not_identical": {n: k for n, k in ks.items() if not k["identical"]}} for f, ks in report.items()}
    result = {"flags": FLAGS, "vgpr_granule": VGPR_GRANULE, "must_be_identical": a.identical, "conditions_met": not failed, "failed": failed, "files": report}
    if moved:
        result["moved"] = moved_report
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    for m in failed:
        print("FAILED", m)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
