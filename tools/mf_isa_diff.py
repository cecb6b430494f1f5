"""Compare the device code of two builds of one .hip file of csrc/ (mf_numeric.hip, kernels.hip, dense.hip, ...) kernel by
kernel: register counts, LDS, scratch and the instruction streams (label numbers normalised).  Inputs are the listings of
    hipcc $(CXXFLAGS of csrc/Makefile) --cuda-device-only -S FILE.hip -o X.s
Usage: python tools/mf_isa_diff.py OLD.s NEW.s  (exit status 1 on any difference)."""
import re
import sys

KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    meta = {}
    for entry in text.split("\n  - .")[1:]:                       # amdhsa.kernels metadata, one YAML item per kernel
        f = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)\s*$", entry, re.M))
        if ".symbol" in f:
            meta[f[".name"]] = tuple(int(f[k]) for k in KEYS)
    code = {}
    for name in meta:
        body = text.split(f"\n{name}:", 1)[1].split(".Lfunc_end", 1)[0]
        lines = (re.sub(r"\s*;.*$", "", ln).strip() for ln in body.split("\n"))
        code[name] = [re.sub(r"\.L(BB|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln) for ln in lines if ln]
    return meta, code


def main(old, new):
    (m0, c0), (m1, c1) = kernels(old), kernels(new)
    bad = sorted(set(m0) ^ set(m1))
    print(f"{len(m0)} kernels in {old}, {len(m1)} in {new}; only in one build: {bad or 'none'}")
    print(f"{'vgpr':>5} {'sgpr':>5} {'lds':>7} {'scratch':>7} {'instr':>6}  stream     kernel")
    for name in sorted(set(m0) & set(m1)):
        same_meta, same_code = m0[name] == m1[name], c0[name] == c1[name]
        if not (same_meta and same_code):
            bad.append(name)
        v, s, l, p = m1[name]
        print(f"{v:5d} {s:5d} {l:7d} {p:7d} {len(c1[name]):6d}  {'identical' if same_code else 'DIFFERS  '}  {name}"
              + ("" if same_meta else f"   COUNTS WERE {m0[name]}"))
    print("RESULT:", "all kernels equal" if not bad else f"{len(bad)} differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
