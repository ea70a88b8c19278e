#!/usr/bin/env python3
"""tools/device_code_diff.py PARENT_TREE NEW_TREE [--rename REGEX=REPLACEMENT ...]  -- did a host-side change move any device code?

Compiles every csrc/*.hip of both trees to device-only gfx950 assembly (hipcc --cuda-device-only -S), once with the product
flags and once with -DMG_LAB, each file with the EXTRA_FLAGS of its own tree's __graft_entry__.py, and compares per symbol:
  * the set of kernels (.amdhsa_kernel names) is equal,
  * each kernel's descriptor block (.amdhsa_kernel .. .end_amdhsa_kernel: VGPRs, SGPRs, LDS, scratch) is equal,
  * each function body is equal once the function ordinal in local labels (.LBB<k>_, .Lfunc_end<k>, ... -- it only encodes the
    order of emission) is normalised,
  * each device global (size, alignment, initialiser) is equal.
--rename: applied to the PARENT's assembly before it is parsed, for a kernel template that gained a defaulted parameter -- the Itanium mangling
spells defaulted template arguments out, so every old instantiation has a new symbol and would be listed as "only in PARENT" / "only in NEW"
with nothing said about its code.  --all: every report line, not the first 40 per file.
Prints one summary line per file and build, exits 1 if anything differs.  A tool, not a test: it compiles twenty times."""
import concurrent.futures
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S", "-Wno-unused-command-line-argument"]
# <prefix><function ordinal>: .LBB12_3, .Lfunc_begin12, .Lfunc_end12, .LJTI12_0, .LCPI12_0, .Ltmp are per function / per file counters
ORDINAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|LCPI)\d+")


def extra_flags(tree):
    spec = importlib.util.spec_from_file_location("_entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EXTRA_FLAGS


def compile_asm(tree, src, lab, out):
    csrc = os.path.join(tree, "endless-memory-gym_amd", "csrc")
    cmd = [HIPCC] + BASE + (["-DMG_LAB"] if lab else []) + extra_flags(tree).get(src, []) + [os.path.join(csrc, src), "-o", out]
    subprocess.check_call(cmd, cwd=os.path.join(tree, "endless-memory-gym_amd"))
    return out


def parse(path):
    """-> (functions {name: body}, descriptors {kernel: block}, globals {name: definition})"""
    funcs, descs, globs = {}, {}, {}
    lines = open(path).read().split("\n")
    types = {}
    for ln in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@(\w+)", ln)
        if m:
            types[m.group(1)] = m.group(2)
    i = 0
    while i < len(lines):  # the descriptor blocks (they sit inside the function's extent, in a section of their own)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            descs[m.group(1)] = "\n".join(l.strip() for l in lines[i:j + 1])
            lines[i:j + 1] = []
            continue
        i += 1
    i = 0
    while i < len(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", lines[i])
        if m and m.group(1) in types and not m.group(1).startswith("__hip_cuid_"):  # (__hip_cuid_<hash of the source>: not code)
            name, kind = m.group(1), types[m.group(1)]
            j = i + 1
            if kind == "function":
                while j < len(lines) and not re.match(r"\s*\.Lfunc_end\d+:", lines[j]):
                    j += 1
                body = [re.sub(r"\s*;.*$", "", l) for l in lines[i:j]]  # comments name loop headers by ordinal
                body = [l for l in body if l.strip() and not re.match(r"\s*(\.Ltmp\d+:|\.loc\s|\.file\s|\.cfi_)", l)]
                funcs[name] = ORDINAL.sub(lambda k: "." + k.group(1) + "#", "\n".join(body))
            else:
                while j < len(lines) and not re.match(r"\s*\.size\s", lines[j]):
                    j += 1
                globs[name] = "\n".join(lines[i:j + 1])
            i = j + 1
            continue
        i += 1
    return funcs, descs, globs


def compare(what, a, b, report):
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            report.append("  %s only in %s: %s" % (what, "NEW" if name not in a else "PARENT", name))
            bad += 1
        elif a[name] != b[name]:
            report.append("  %s differs: %s" % (what, name))
            bad += 1
    return bad


def main():
    args, renames, show_all = [], [], False
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--rename":
            rx, _, repl = next(it, "").partition("=")
            renames.append((re.compile(rx), repl))
        elif a == "--all":
            show_all = True
        else:
            args.append(a)
    if len(args) != 2:
        sys.exit(__doc__)
    parent, new = (os.path.abspath(p) for p in args)
    names = lambda t: sorted(os.path.basename(f) for f in glob.glob(os.path.join(t, "endless-memory-gym_amd", "csrc", "*.hip"))
                             if not os.path.basename(f).startswith("_"))
    if names(parent) != names(new):
        sys.exit("the two trees hold different csrc/*.hip files: %s / %s" % (names(parent), names(new)))
    tmp = tempfile.mkdtemp(prefix="device_code_diff_")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as pool:
        for src in names(new):
            for lab in (False, True):
                for side, tree in (("parent", parent), ("new", new)):
                    out = os.path.join(tmp, "%s.%s.%s.s" % (src, "lab" if lab else "product", side))
                    jobs[(src, lab, side)] = pool.submit(compile_asm, tree, src, lab, out)
        total_bad = 0
        for src in names(new):
            for lab in (False, True):
                parent_asm = jobs[(src, lab, "parent")].result()
                if renames:
                    text = open(parent_asm).read()
                    for rx, repl in renames:
                        text = rx.sub(repl, text)
                    open(parent_asm, "w").write(text)
                fa, da, ga = parse(parent_asm)
                fb, db, gb = parse(jobs[(src, lab, "new")].result())
                report = []
                bad = compare("kernel descriptor", da, db, report) + compare("function", fa, fb, report) + compare("global", ga, gb, report)
                total_bad += bad
                print("%-18s %-7s %3d kernels, %3d functions, %2d globals: %d differ" % (src, "lab" if lab else "product", len(db), len(fb), len(gb), bad))
                print("\n".join(report if show_all else report[:40]), end="\n" if report else "")
    print("device code: %s (assembly kept in %s)" % ("IDENTICAL" if not total_bad else "%d DIFFERENCES" % total_bad, tmp))
    sys.exit(1 if total_bad else 0)


if __name__ == "__main__":
    main()
