"""Is the device code of a translation unit the same in two trees?  No GPU needed.

    python profiles/sort_host/compare_device_code.py PARENT_TREE THIS_TREE [--text-may-differ] [FILE.hip ...] > device_code.md

Compiles esrecsys_amd/csrc/FILE.hip (default: esr_sort.hip) of both trees with the project's own flags, device side only
(--cuda-device-only -S -Rpass-analysis=kernel-resource-usage), and compares kernel symbol by kernel symbol: the set of
symbols, every kernel's instruction text (instantiation order in the file may differ, so not the file as a whole) and
its row of the resource-usage table, and the compiler's warnings.  Prints one table per file as Markdown; exit status 1
on any difference -- with --text-may-differ (a refactor of device code) a kernel whose instruction text differs is
listed but only symbols, warnings, VGPRs, AGPRs, scratch, LDS and occupancy count.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from esrecsys_amd.build import CFLAGS, HIPCC  # noqa: E402

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def compile_device(tree, name, out_s):
    src = os.path.join(tree, "esrecsys_amd", "csrc", name)
    r = subprocess.run([HIPCC] + CFLAGS + ["--cuda-device-only", "-S", src, "-o", out_s,
                                           "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return r.stderr


def kernels(asm):
    """symbol -> instruction text of every .amdhsa_kernel of the file (labels, directives and comments dropped: they carry
    block numbers and source lines, which move with the host code)"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    out = {}
    for name in names:
        m = re.search(r"^%s:.*?^\s*s_endpgm" % re.escape(name), asm, re.M | re.S)
        body = []
        for line in m.group(0).splitlines()[1:]:
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[name] = "\n".join(body)
    return out


def resources(remarks):
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name:
            out[name][key.strip()] = val
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
        lines = r.stdout.split("\n")[:len(names)] if r.returncode == 0 else names
    except OSError:
        lines = names
    return dict(zip(names, [re.sub(r"^(void )?esr::|\(.*$", "", s) for s in lines]))


def warnings(remarks):
    return sorted(re.sub(r"^.*?:\d+:\d+: ", "", ln) for ln in remarks.splitlines() if "warning:" in ln)


def compare(parent, this, name, text_may_differ):
    with tempfile.TemporaryDirectory() as tmp:
        pa, ta = os.path.join(tmp, "parent.s"), os.path.join(tmp, "this.s")
        pe, te = compile_device(parent, name, pa), compile_device(this, name, ta)
        pr, tr = resources(pe), resources(te)
        pk, tk = kernels(open(pa).read()), kernels(open(ta).read())
    bad, differ = 0, []
    print("## %s\n" % name)
    if warnings(pe) != warnings(te):
        bad += 1
        print("warnings differ: parent %s, here %s" % (warnings(pe), warnings(te)))
    if set(pk) != set(tk):
        bad += 1
        print("kernel symbols differ: only in parent %s, only here %s" % (sorted(set(pk) - set(tk)), sorted(set(tk) - set(pk))))
    nice = demangle(sorted(pk))
    print("| kernel | instructions | same text | " + " | ".join(FIELDS) + " |")
    print("|---|---|---|" + "---|" * len(FIELDS))
    for sym in sorted(set(pk) & set(tk), key=lambda s: nice[s]):
        same = pk[sym] == tk[sym]
        cells = []
        for f in FIELDS:
            a, b = pr[sym].get(f), tr[sym].get(f)
            cells.append(a if a == b else "%s -> %s" % (a, b))
            bad += a != b and not (text_may_differ and f == "TotalSGPRs")  # (scalar registers follow the schedule)
        if not same:
            differ.append(nice[sym])
            bad += not text_may_differ
        count = "%d" % (pk[sym].count("\n") + 1) if same else "%d -> %d" % (pk[sym].count("\n") + 1, tk[sym].count("\n") + 1)
        print("| `%s` | %s | %s | %s |" % (nice[sym], count, "yes" if same else "NO", " | ".join(cells)))
    print("\n%d kernels, %d warnings; instruction text differs in %d; %s\n"
          % (len(pk), len(warnings(te)), len(differ), "no difference that counts" if not bad else "%d DIFFERENCES" % bad))
    return bad


def main(argv):
    may = "--text-may-differ" in argv
    argv = [a for a in argv if a != "--text-may-differ"]
    bad = sum(compare(argv[0], argv[1], name, may) for name in (argv[2:] or ["esr_sort.hip"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
