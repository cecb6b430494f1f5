"""Compare the device code of two builds of one .hip file of csrc/ (mf_numeric.hip, kernels.hip, dense.hip, ...) kernel by
kernel: register counts, LDS, scratch and the instruction streams (label numbers normalised).  Inputs are the listings of
    hipcc $(CXXFLAGS of csrc/Makefile) --cuda-device-only -S FILE.hip -o X.s
Usage: python tools/mf_isa_diff.py OLD.s NEW.s [--skip REGEX] [--pair OLD_REGEX NEW_REGEX]  (exit status 1 on any difference).
--skip leaves kernels whose symbol matches out (library kernels such as rocPRIM's).  --pair matches a renamed kernel of
OLD.s to the one of NEW.s whose regex groups are equal (a template argument, say); a pair is printed with both builds'
counts and counts as a difference only where a register, LDS or scratch count went up."""
import re
import sys

KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path, skip=None):
    text = open(path).read()
    meta = {}
    for entry in text.split("\n  - .")[1:]:                       # amdhsa.kernels metadata, one YAML item per kernel
        f = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)\s*$", entry, re.M))
        if ".symbol" in f and not (skip and re.search(skip, f[".name"])):
            meta[f[".name"]] = tuple(int(f[k]) for k in KEYS)
    code = {}
    for name in meta:
        body = text.split(f"\n{name}:", 1)[1].split(".Lfunc_end", 1)[0]
        lines = (re.sub(r"\s*;.*$", "", ln).strip() for ln in body.split("\n"))
        code[name] = [re.sub(r"\.L(BB|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln) for ln in lines if ln]
    return meta, code


def main(old, new, skip=None, pair=None):
    (m0, c0), (m1, c1) = kernels(old, skip), kernels(new, skip)
    pairs = []
    if pair:
        key0 = {re.search(pair[0], n).groups(): n for n in m0 if re.search(pair[0], n)}
        key1 = {re.search(pair[1], n).groups(): n for n in m1 if re.search(pair[1], n)}
        pairs = [(key0[k], key1[k]) for k in sorted(set(key0) & set(key1))]
    renamed = {n for p in pairs for n in p}
    bad = sorted((set(m0) ^ set(m1)) - renamed)
    print(f"{len(m0)} kernels in {old}, {len(m1)} in {new}; only in one build: {bad or 'none'}")
    print(f"{'vgpr':>5} {'sgpr':>5} {'lds':>7} {'scratch':>7} {'instr':>6}  stream     kernel")
    for name in sorted(set(m0) & set(m1)):
        same_meta, same_code = m0[name] == m1[name], c0[name] == c1[name]
        if not (same_meta and same_code):
            bad.append(name)
        v, s, l, p = m1[name]
        print(f"{v:5d} {s:5d} {l:7d} {p:7d} {len(c1[name]):6d}  {'identical' if same_code else 'DIFFERS  '}  {name}"
              + ("" if same_meta else f"   COUNTS WERE {m0[name]}"))
    for a, b in pairs:
        if any(x1 > x0 for x0, x1 in zip(m0[a], m1[b])):
            bad.append(b)
        for tag, m, c, n in (("old", m0, c0, a), ("new", m1, c1, b)):
            v, s, l, p = m[n]
            print(f"{v:5d} {s:5d} {l:7d} {p:7d} {len(c[n]):6d}  renamed {tag}  {n}")
    print("RESULT:", "all kernels equal" + (f", {len(pairs)} renamed with no count above the old build's" if pairs else "")
          if not bad else f"{len(bad)} differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    args, opt = sys.argv[1:], {}
    while "--skip" in args:
        i = args.index("--skip")
        opt["skip"] = args[i + 1]
        del args[i:i + 2]
    while "--pair" in args:
        i = args.index("--pair")
        opt["pair"] = (args[i + 1], args[i + 2])
        del args[i:i + 3]
    sys.exit(main(args[0], args[1], **opt))
