"""Compare the device ISA of two builds, kernel by kernel.

Each directory holds the device assembly of the library's translation units, one file per csrc/*.hip, made with the
shipping flags (`hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only -S x.hip -o dir/x.s`; render, mlp_fp32 and adam
with -ffp-contract=off as in the Makefile).  For every kernel symbol the tool reports whether it is present on both
sides, whether the instruction streams are equal (comments, labels and directives ignored; a branch target counts as
the position of its label inside the function, so renumbered labels do not matter) and whether the register, spill,
scratch and LDS figures of the metadata are equal.  It only compares: what the instructions are is none of its business.

usage: python tools/isa_diff.py DIR_A DIR_B        (exit status 0: identical, 1: any difference)
"""
import os
import re
import sys

META_KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def functions(text):
    """{symbol: [instruction, ...]} of the function symbols of one .s file (the split of tools/check_vmcnt.py)."""
    out = {}
    for f in re.split(r"\n(?=_Z[_A-Za-z0-9.$]+:)", "\n" + text)[1:]:
        name, body = f.split(":", 1)
        body = body.split("\n.Lfunc_end", 1)[0]
        lines = [ln.split(";", 1)[0].strip() for ln in body.splitlines()]
        labels = {ln[:-1]: "<L%d>" % i for i, ln in enumerate(ln for ln in lines if re.fullmatch(r"[.\w$]+:", ln))}
        ins = [ln for ln in lines if ln and not ln.endswith(":") and not ln.startswith(".")]
        out[name.strip()] = [" ".join(labels.get(tok, tok) for tok in re.split(r"\s+", ln)) for ln in ins]
    return out


def metadata(text):
    """{kernel symbol: {key: value}} of the .amdgpu_metadata block."""
    out = {}
    block = text.split(".amdgpu_metadata", 1)[1] if ".amdgpu_metadata" in text else ""
    for entry in re.split(r"\n  - (?=\.)", block)[1:]:
        kv = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", entry, re.M))
        if ".name" in kv:
            out[kv[".name"]] = {k: kv.get(k) for k in META_KEYS}
    return out


def compare(text_a, text_b):
    """[(symbol, verdict)] for the kernels of one translation unit; verdict 'same' or what differs."""
    fa, fb, ma, mb = functions(text_a), functions(text_b), metadata(text_a), metadata(text_b)
    rows = []
    for sym in sorted(set(fa) | set(fb)):            # kernels, and device functions that were not inlined
        if sym not in fa or sym not in fb:
            rows.append((sym, "only in %s" % ("A" if sym in fa else "B")))
            continue
        if (sym in ma) != (sym in mb):
            rows.append((sym, "a kernel only in %s" % ("A" if sym in ma else "B")))
            continue
        what = []
        if fa.get(sym) != fb.get(sym):
            a, b = fa.get(sym, []), fb.get(sym, [])
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            what.append("instructions differ (%d vs %d, first at %d)" % (len(a), len(b), at))
        what += ["%s %s vs %s" % (k, ma[sym][k], mb[sym][k]) for k in META_KEYS if sym in ma and ma[sym][k] != mb[sym][k]]
        rows.append((sym, "; ".join(what) or "same"))
    return rows


def main(dir_a, dir_b):
    bad = 0
    units = sorted({f for d in (dir_a, dir_b) for f in os.listdir(d) if f.endswith(".s")})
    print("%-20s %8s %8s %14s" % ("translation unit", "symbols", "same", "instructions"))
    for u in units:
        pa, pb = os.path.join(dir_a, u), os.path.join(dir_b, u)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("%-20s only in %s" % (u, dir_a if os.path.exists(pa) else dir_b))
            bad += 1
            continue
        text_a = open(pa).read()
        rows = compare(text_a, open(pb).read())
        diff = [(s, v) for s, v in rows if v != "same"]
        fa = functions(text_a)
        print("%-20s %8d %8d %14d" % (u, len(rows), len(rows) - len(diff), sum(len(fa.get(s, [])) for s, _ in rows)))
        for s, v in diff:
            print("    %s: %s" % (s, v))
        bad += len(diff)
    print("IDENTICAL" if not bad else "%d DIFFERENCES" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
